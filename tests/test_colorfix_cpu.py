"""Colour correction without a GPU: the float64 restatement (tests/_colorfix_ref.py) against an independent fp32 torch
composition, the argument errors of rs_color_fix - found before anything is launched - and the host plumbing from `color_fix=` down to
the engine call, on recording fakes in the manner of tests/test_feather_cpu.py."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers as H  # noqa: F401  (puts the repository root on sys.path)
import _colorfix_ref as R
from _fakes import FakeEngine, _OnDevice, fake_launches, fake_sampler, lib  # noqa: F401  (fixtures)
from resshift_amd import _lib, tiling
from resshift_amd.tilepool import TilePool, tile_windows


# ---------------------------------------------------------------------------------------------------------------- the restatement
def torch_wavelet(sr, lq, sf, order=R.DILATIONS, pad_mode="replicate"):
    """the definition composed from torch ops in fp32: F.interpolate, five depthwise dilated convs on replicate padding"""
    Cc = sr.shape[1]
    up = F.interpolate(lq, scale_factor=sf, mode="bicubic", align_corners=False) if sf > 1 else lq
    k1 = torch.tensor([0.25, 0.5, 0.25])
    k = torch.outer(k1, k1)[None, None].repeat(Cc, 1, 1, 1)
    d_img = sr - up
    for d in order:
        d_img = F.conv2d(F.pad(d_img, (d, d, d, d), mode=pad_mode), k, groups=Cc, dilation=d)
    return (sr - d_img).clamp(-1, 1)


def torch_adain(sr, lq):
    def stats(x):
        return x.mean(dim=(2, 3), keepdim=True), (torch.var(x, dim=(2, 3), keepdim=True) + 1e-5).sqrt()

    m_sr, s_sr = stats(sr)
    m_lq, s_lq = stats(lq)
    return ((sr - m_sr) * s_lq / s_sr + m_lq).clamp(-1, 1)


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_against_the_torch_composition(shape):
    """fp32 torch against float64 numpy: 1e-5 is the bound the device kernel gets (tests/test_colorfix_gpu.py); a missing level, reflect
    padding or the reversed level order move pixels by more than 0.04"""
    Hh, W, sf = shape
    sr, lq = R.inputs(Hh, W, sf)
    want = R.wavelet(sr.numpy(), lq.numpy(), sf)
    assert want.shape == tuple(sr.shape) and want.dtype == np.float64
    share = R.saturated_share(want)
    err = float(np.abs(torch_wavelet(sr, lq, sf).double().numpy() - want).max())
    moved = float(np.abs(want - sr.double().numpy()).max())
    print(f"wavelet {shape}: |torch fp32 - restatement| = {err:.2e}, share at +-1 = {share:.3f}, the correction moves pixels by up to {moved:.3f}")
    assert share < 0.10 and err <= 1e-5 and moved > 0.05
    if sf * min(Hh, W) > 20:   # (reflect padding by 16 needs a side above 16)
        wrong = {"one level missing": torch_wavelet(sr, lq, sf, order=R.DILATIONS[:-1]),
                 "reflect": torch_wavelet(sr, lq, sf, pad_mode="reflect"),
                 "reversed": torch_wavelet(sr, lq, sf, order=R.DILATIONS[::-1])}
        for name, t in wrong.items():
            assert float(np.abs(t.double().numpy() - want).max()) > 0.04, name
    # adain
    want = R.adain(sr.numpy(), lq.numpy())
    err = np.abs(torch_adain(sr, lq).double().numpy() - want)
    assert R.saturated_share(want) < 0.10 and np.all(err <= R.adain_tolerance(sr.numpy(), lq.numpy()))


def test_restatement_properties():
    sr, lq = R.inputs(12, 9, 4)
    # the decomposition is linear: high(sr) + low(up(lq)) is the form on the one difference image
    u = R.up(lq.numpy(), 4)
    s64 = sr.double().numpy()
    np.testing.assert_allclose(np.clip((s64 - R.low(s64)) + R.low(u), -1, 1), R.wavelet(s64, lq.numpy(), 4), rtol=0, atol=1e-14)
    assert R.REACH == 31
    # a constant image is a fixed point of every level, borders included, and the bicubic rows sum to one
    np.testing.assert_allclose(R.low(np.full((40, 33), 0.3)), 0.3, rtol=0, atol=1e-15)
    np.testing.assert_allclose(R.bicubic_matrix(7, 4).sum(axis=1), 1.0, rtol=0, atol=1e-15)
    assert R.up(lq.numpy(), 1) is not None and np.array_equal(R.up(lq.numpy(), 1), lq.double().numpy())
    # adain gives the output lq's statistics (before the clamp: use inputs that stay inside)
    out = R.adain(0.5 * s64, 0.5 * lq.numpy())
    m, s = R.plane_stats(out)
    m_lq, s_lq = R.plane_stats(0.5 * lq.numpy())
    if R.saturated_share(out) == 0:
        np.testing.assert_allclose(m, m_lq, rtol=0, atol=1e-12)
        np.testing.assert_allclose(s, s_lq, rtol=1e-4, atol=0)   # (the two 1e-5 under the roots do not cancel exactly)


def test_low_contrast_case_separates_the_two_variance_forms():
    """the centred fp32 form stays within the tolerance of the GPU test; E[x^2] - mean^2 in fp32 does not"""
    sr, lq = R.low_contrast_inputs()
    want = R.adain(sr.numpy(), lq.numpy())
    tol = R.adain_tolerance(sr.numpy(), lq.numpy())
    assert 1e-5 < float(tol.max()) < 3e-5 and R.saturated_share(want) < 0.10
    centred = np.abs(torch_adain(sr, lq).double().numpy() - want)
    n = sr.shape[2] * sr.shape[3]
    m = sr.mean(dim=(2, 3), keepdim=True)
    naive_var = ((sr * sr).mean(dim=(2, 3), keepdim=True) - m * m).clamp_min(0) * (n / (n - 1))
    m_lq = lq.mean(dim=(2, 3), keepdim=True)
    s_lq = (torch.var(lq, dim=(2, 3), keepdim=True) + 1e-5).sqrt()
    naive = np.abs(((sr - m) * s_lq / (naive_var + 1e-5).sqrt() + m_lq).clamp(-1, 1).double().numpy() - want)
    print(f"low contrast: centred fp32 {centred.max():.2e}, E[x^2] - mean^2 fp32 {naive.max():.2e}, tolerance {tol.max():.2e}")
    assert np.all(centred <= tol) and naive.max() > 4 * tol.max()


# ---------------------------------------------------------------------------------------------------------------- C ABI
PTR = 0x100000   # never dereferenced: every call below is refused before anything is launched
FAR = 0x40000000

ERRORS = {
    "null_sr": (dict(sr=None), "null tensor"),
    "null_lq": (dict(lq=None), "null tensor"),
    "null_out": (dict(out=None), "null tensor"),
    "batch": (dict(B=0), "must be positive"),
    "channels": (dict(C=0), "must be positive"),
    "height": (dict(H=0), "must be positive"),
    "width": (dict(W=-3), "must be positive"),
    "sf": (dict(sf=0), "sf must be positive"),
    "mode_zero": (dict(mode=0), "unknown mode"),
    "mode_three": (dict(mode=3), "unknown mode"),
    "out_is_sr": (dict(out=PTR), "overlaps"),
    "out_inside_sr": (dict(out=PTR + 2 * 3 * 160 * 208 * 4 - 4), "overlaps"),
    "out_before_sr": (dict(out=PTR - 4), "overlaps"),
    "out_on_lq": (dict(out=2 * FAR + 64), "overlaps"),
    "work_null": (dict(mode=2, work=None, work_bytes=1 << 20), "workspace is too small"),
    "work_small": (dict(mode=2, work_bytes=2 * 3 * (5 + 1) * 8 - 1), "workspace is too small"),   # (160 x 208: five chunks of 8192; lq: one)
}


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_color_fix_argument_errors(lib, name):
    kw, text = ERRORS[name]
    a = dict(sr=PTR, lq=2 * FAR, out=FAR, B=2, C=3, H=40, W=52, sf=4, mode=1, work=3 * FAR, work_bytes=0)
    a.update(kw)
    rc = lib.rs_color_fix(a["sr"], a["lq"], a["out"], a["B"], a["C"], a["H"], a["W"], a["sf"], a["mode"], a["work"], a["work_bytes"], None)
    assert rc == -2 and text in _lib.last_error() and _lib.last_error().startswith("rs_color_fix: "), (rc, _lib.last_error())


def test_symbols_are_declared_and_the_workspace_size(lib):
    for name, n_args in (("rs_color_fix", 12), ("rs_color_fix_work_bytes", 6)):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == n_args
    header = open(H.ROOT + "/include/resshift_hip.h").read()
    for text in ("#define RS_COLOR_FIX_WAVELET 1", "#define RS_COLOR_FIX_ADAIN 2", "size_t rs_color_fix_work_bytes(int B, int C, int H, int W, int sf, int mode);",
                 "int rs_color_fix(const float* sr, const float* lq, float* out, int B, int C, int H, int W, int sf, int mode, void* work, size_t work_bytes,"):
        assert text in header, text
    assert (_lib.RS_COLOR_FIX_WAVELET, _lib.RS_COLOR_FIX_ADAIN) == (1, 2) and _lib.COLOR_FIX_MODES == {"wavelet": 1, "adain": 2}
    for shape in [(2, 3, 40, 52, 4), (1, 3, 256, 256, 4), (32, 3, 64, 64, 4), (1, 1, 1, 1, 1)]:
        assert lib.rs_color_fix_work_bytes(*shape, _lib.RS_COLOR_FIX_WAVELET) == 0
        assert lib.rs_color_fix_work_bytes(*shape, _lib.RS_COLOR_FIX_ADAIN) > 0
        assert lib.rs_color_fix_work_bytes(*shape, 7) == 0
    # adain: one (mean, centred sum of squares) pair per 8192-element chunk of every sr and lq plane
    assert lib.rs_color_fix_work_bytes(2, 3, 40, 52, 4, 2) == 2 * 3 * (-(-160 * 208 // 8192) + 1) * 8
    # the workspace grows with the batch in proportion: a plane's partials do not depend on its neighbours
    assert lib.rs_color_fix_work_bytes(4, 3, 40, 52, 4, 2) == 2 * lib.rs_color_fix_work_bytes(2, 3, 40, 52, 4, 2)


def test_lib_color_fix_rejects_bad_tensors_before_the_library_is_called():
    sr, lq = torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 2, 2)
    with pytest.raises(ValueError, match="unknown colour fix 'ycbcr'"):
        _lib.color_fix(sr, lq, "ycbcr")
    with pytest.raises(ValueError, match="contiguous float32 device tensors"):
        _lib.color_fix(sr, lq, "wavelet")          # host tensors: there is no CPU arithmetic to fall back to


# ---------------------------------------------------------------------------------------------------------------- host plumbing
def test_unknown_color_fix_is_rejected_by_the_constructor():
    from resshift_amd.sampler import ResShiftSampler

    with pytest.raises(ValueError, match="unknown colour fix 'ycbcr'"):
        ResShiftSampler({}, color_fix="ycbcr")          # validated like `tile_blend`: before anything is built
    with pytest.raises(ValueError, match="unknown tile blend"):
        ResShiftSampler({}, tile_blend="gauss", color_fix="wavelet")
    with pytest.raises(ValueError, match="unknown colour fix"):
        tiling.check_color_fix(None)
    assert tiling.COLOR_FIXES == ("none", "wavelet", "adain")
    for ok in tiling.COLOR_FIXES:
        tiling.check_color_fix(ok)


@pytest.mark.parametrize("fix", ["none", "wavelet", "adain", None])
def test_tile_pool_fixes_each_completed_image_once(fake_launches, fix):
    """the fix is the sampler's; it sees whole blended images with their own LQ planes, never a tile; "none" - named, or a sampler
    without the attribute - never reaches the engine's call"""
    s = fake_sampler(**({"color_fix": fix} if fix else {}))
    tp = TilePool(s, max_batch=4, seeded=True)
    assert tp.color_fix == (fix or "none")
    sizes = [(40, 28), (13, 10)]          # six tiles; one whole image
    lqs = []
    for i, (Hh, W) in enumerate(sizes):
        lq = torch.zeros(3, Hh, W)
        for k, (h0, w0, _, _) in enumerate(tile_windows(Hh, W, 16, 12)):
            lq[0, h0, w0] = (16 * i + k + 1) * 1e-3
        lqs.append(lq)
        assert tp.submit(lq, seed=i) == i
    out = tp.drain()
    assert sorted(out) == [0, 1]
    if fix in (None, "none"):
        assert s.engine.fixes == [] and all(o.max().item() < 0.5 for o in out.values())
        return
    assert len(s.engine.fixes) == 2
    for (shape, lq_seen, mode), i in zip(sorted(s.engine.fixes, key=lambda f: -f[0][2]), (0, 1)):
        Hh, W = sizes[i]
        assert shape == (1, 3, Hh * 4, W * 4) and mode == fix and torch.equal(lq_seen, lqs[i][None])
    assert all(o.min().item() >= 1.0 for o in out.values())     # the pool returns what the fix returned


@pytest.mark.parametrize("size", [(40, 28), (16, 12)], ids=["tiled", "untiled"])
@pytest.mark.parametrize("fix", ["none", "adain"])
def test_sample_tiled_fixes_the_image_it_returns(monkeypatch, fix, size):
    from resshift_amd.sampler import ResShiftSampler

    fake_lib = SimpleNamespace(rs_tile_accumulate=lambda *a: 0, rs_tile_finalize=lambda *a: 0)
    monkeypatch.setattr(_lib, "load", lambda: fake_lib)
    monkeypatch.setattr(_lib, "window_copy", lambda x, h0, w0, ho, wo, out=None: out.copy_(x[..., h0:h0 + ho, w0:w0 + wo]))
    s = ResShiftSampler.__new__(ResShiftSampler)
    s.chop_size, s.chop_stride, s.chop_bs, s.sf, s.tile_blend, s.color_fix = 16, 12, 2, 4, "uniform", fix
    s.engine = FakeEngine()
    calls = []

    def sample_func(pch, noise_repeat=False, mask=None, noise=None, step_noises=None, seeds=None):
        calls.append(tuple(pch.shape))
        return torch.zeros(pch.shape[0], 3, pch.shape[2] * 4, pch.shape[3] * 4)

    s.sample_func = sample_func
    im = torch.rand(1, 3, *size).as_subclass(_OnDevice)
    out = s.sample_tiled(im, seed=3)
    assert tuple(out.shape) == (1, 3, size[0] * 4, size[1] * 4) and len(calls) == (3 if size[0] > 16 else 1)
    if fix == "none":
        assert s.engine.fixes == [] and out.max().item() == 0
    else:   # once, on the whole image, after the tiles
        assert [(f[0], f[2]) for f in s.engine.fixes] == [((1, 3, size[0] * 4, size[1] * 4), "adain")]
        assert torch.equal(s.engine.fixes[0][1].as_subclass(torch.Tensor), im.as_subclass(torch.Tensor)) and out.min().item() == 1.0


def test_a_mask_excludes_the_fix():
    """the input has a hole, so the correction is undefined: sample_tiled(mask=), inference(mask_path=) and a TilePool over a cond_mask
    model raise under any fix; under "none" the pool is built as ever"""
    from resshift_amd.sampler import ResShiftSampler

    s = ResShiftSampler.__new__(ResShiftSampler)
    s.chop_size, s.chop_stride, s.chop_bs, s.sf, s.tile_blend = 16, 12, 1, 4, "uniform"
    for fix in ("wavelet", "adain"):
        s.color_fix = fix
        with pytest.raises(ValueError, match=f"color_fix='{fix}' is undefined for a masked input"):
            s.sample_tiled(torch.zeros(1, 3, 16, 12), mask=torch.zeros(1, 1, 16, 12))
        with pytest.raises(ValueError, match=f"color_fix='{fix}' is undefined for masked"):
            s.inference("in", "out", mask_path="masks")
        with pytest.raises(ValueError, match=f"color_fix='{fix}' is undefined for a model conditioned on a mask"):
            TilePool(fake_sampler(cond_mask=True, color_fix=fix))
    assert TilePool(fake_sampler(cond_mask=True, color_fix="none")).color_fix == "none"
    assert TilePool(fake_sampler(cond_mask=True)).color_fix == "none"
    with pytest.raises(ValueError, match="unknown colour fix"):
        TilePool(fake_sampler(color_fix="ycbcr"))

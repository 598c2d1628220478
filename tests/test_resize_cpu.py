"""Antialiased resize without a GPU: the float64 restatement (tests/_resize_ref.py) against the recorded outputs of the
reference's imresize_np (tests/golden/reference_resize.npz, scripts/make_golden_resize.py) and against float64 F.interpolate away from
the borders, the mutations the bounds of the GPU test must catch, the argument errors of rs_resize and _lib.resize - found before
anything is launched - and the host plumbing from `out_scale=` down to the engine call, on recording fakes in the manner of
tests/test_colorfix_cpu.py."""
import hashlib
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers as H  # noqa: F401  (puts the repository root on sys.path)
import _resize_ref as R
from _fakes import FakeEngine, _OnDevice, fake_launches, fake_sampler, lib  # noqa: F401  (fixtures)
from resshift_amd import _lib, build, tiling
from resshift_amd.tilepool import TilePool, tile_windows


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", R.GOLDEN_CASES, ids=R.case_id)
def test_restatement_against_the_recorded_reference(case):
    """float64 against what imresize_np returned (fp32 arithmetic, fp32 linspace coordinates): 1e-5 on every element is the largest
    distance a correct restatement may have from that reference - measured 3.6e-6 (0.75) and 4.3e-6 (1.5) at worst, below 3e-7 at the
    other scales"""
    (Hh, W), _, scale = case
    gold = np.load(H.ROOT + "/tests/golden/reference_resize.npz")
    key = R.golden_key(case)
    x = R.inputs(Hh, W)[0]
    assert hashlib.sha256(x.tobytes()).digest() == gold["sha256_" + key].tobytes(), "the seeded input is not the recorded one"
    assert float(gold["scale_" + key]) == scale
    want = gold["out_" + key].transpose(2, 0, 1)
    got = R.resize(x, scale=scale)
    assert got.shape == want.shape == (3, R.out_size(Hh, scale), R.out_size(W, scale)) and got.dtype == np.float64
    err = float(np.abs(got - want).max())
    print(f"{key}: |float64 restatement - imresize_np| = {err:.2e}")
    assert err <= 1e-5


def test_every_scale_form_case_but_the_eighth_is_recorded():
    gold = np.load(H.ROOT + "/tests/golden/reference_resize.npz")
    assert sorted(k[4:] for k in gold.files if k.startswith("out_")) == sorted(R.golden_key(c) for c in R.GOLDEN_CASES)
    assert len(R.GOLDEN_CASES) == 7 and len(R.CASES) == 9
    assert [R.taps(s) for s in (0.5, 0.25, 0.125, 1.5, 1.0)] == [10, 18, 34, 6, 6]


@pytest.mark.parametrize("shape", [(160, 208, 0.5), (64, 96, 0.25), (72, 48, 0.75), (36, 60, 1.5), (33, 20, 2.0)], ids=str)
def test_restatement_against_float64_interpolate_away_from_the_borders(shape):
    """F.interpolate(mode="bicubic", antialias=True) in float64 is the same function in the interior (1e-12; measured <= 1.2e-14) and
    another one at the borders, where it clamps and renormalises and the definition mirrors: above 0.03 over the whole image"""
    Hh, W, s = shape
    x = R.inputs(Hh, W).astype(np.float64)
    Ho, Wo = R.out_size(Hh, s), R.out_size(W, s)
    assert (Ho, Wo) == (Hh * s, W * s)
    want = R.resize(x, scale=s)
    got = F.interpolate(torch.from_numpy(x), size=(Ho, Wo), mode="bicubic", antialias=True, align_corners=False).numpy()
    diff = np.abs(got - want)
    m = math.ceil(3 * max(s, 1)) + 1
    inner = float(diff[..., m:-m, m:-m].max())
    print(f"{shape}: interior (margin {m}) {inner:.2e}, whole image {diff.max():.3f}")
    assert diff[..., m:-m, m:-m].size > 0 and inner <= 1e-12
    assert diff.max() > 0.03


MUTATIONS = [
    ("no antialiasing", 0.5, dict(antialias=False)),
    ("clamp instead of mirror", 0.5, dict(border="clamp")),
    ("reflection without the repeated edge sample", 0.5, dict(border="reflect")),
    ("A = -0.75", 1.5, dict(A=-0.75)),
    ("no normalisation", 0.75, dict(normalise=False)),
    ("a half-pixel shift", 0.125, dict(shift=0.5)),
]


@pytest.mark.parametrize("name,scale,kw", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_each_mutation_of_the_restatement_moves_a_pixel(name, scale, kw):
    """on every case of that scale: more than 5e-3, 250 times the bound of the GPU test"""
    hit = [c for c in R.CASES if c[1] == "scale" and c[2] == scale]
    assert hit
    for (Hh, W), _, s in hit:
        x = R.inputs(Hh, W)
        moved = float(np.abs(R.resize(x, scale=s, **kw) - R.resize(x, scale=s)).max())
        print(f"{name} on ({Hh}, {W}) at {s}: {moved:.2e}")
        assert moved > 5e-3, (name, Hh, W)


def test_restatement_properties():
    # rows of every axis matrix sum to one: a constant image is a fixed point, borders included
    for n, m, s in [(20, 10, 0.5), (37, 28, 0.75), (3, 1, 0.125), (24, 36, 1.5), (40, 17, 17 / 40)]:
        np.testing.assert_allclose(R.axis_matrix(n, m, s).sum(axis=1), 1.0, rtol=0, atol=1e-14)
    # scale 1 is the identity: the weights are exactly 0 and 1
    x = R.inputs(9, 11)
    assert np.array_equal(R.resize(x, scale=1.0), x.astype(np.float64))
    # the mirror repeats the edge sample, as often as needed
    assert R.mirror(np.arange(-7, 8), 3).tolist() == [0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1]
    # the overshoot the clamp of the samplers removes: present on the upscale cases, rare everywhere
    for (Hh, W), kind, v in R.CASES:
        out = R.resize(R.inputs(Hh, W), **{kind: v}, clamp=True)
        share = R.saturated_share(out)
        assert (share > 0 or not (kind == "scale" and v > 1)) and share < 0.10, ((Hh, W), v, share)


def test_the_fraction_size_rule():
    assert math.ceil(100 * 0.07) == 8 and _lib.resize_len(100, 0.07) == 7          # what the rule is for
    assert _lib.resize_len(40, 0.3) == 12 and _lib.resize_len(70, 1 / 3) == 24
    assert tiling.out_size(40, 70, 0.3) == (12, 21) and tiling.out_size(70, 37, 1 / 3) == (24, 13)
    assert R.out_size(40, 0.3) == 12 and R.out_size(70, 1 / 3) == 24
    assert _lib.resize_len(37, 0.75) == 28 and _lib.resize_len(3, 0.125) == 1 and _lib.resize_len(24, Fraction(3, 2)) == 36
    assert tiling.out_size(40, 28, 2) == (80, 56) and tiling.out_size(5, 7, 3) == (15, 21)


# ---------------------------------------------------------------------------------------------------------------- C ABI
PTR = 0x100000   # never dereferenced: every call below is refused before anything is launched
FAR = 0x40000000

ERRORS = {
    "null_in": (dict(inp=None), "null tensor"),
    "null_out": (dict(out=None), "null tensor"),
    "batch": (dict(B=0), "must be positive"),
    "channels": (dict(C=-1), "must be positive"),
    "height": (dict(H=0), "must be positive"),
    "width": (dict(W=-3), "must be positive"),
    "out_height": (dict(Ho=0), "must be positive"),
    "out_width": (dict(Wo=0), "must be positive"),
    "scale_h_small": (dict(sh=0.1249), "must lie in [1/8, 8]"),
    "scale_w_large": (dict(sw=8.001), "must lie in [1/8, 8]"),
    "scale_zero": (dict(sh=0.0), "must lie in [1/8, 8]"),
    "scale_negative": (dict(sw=-0.5), "must lie in [1/8, 8]"),
    "scale_nan": (dict(sh=float("nan")), "must lie in [1/8, 8]"),
    "in_is_out": (dict(out=PTR), "overlaps"),
    "out_inside_in": (dict(out=PTR + 2 * 3 * 40 * 52 * 4 - 4), "overlaps"),
    "out_before_in": (dict(out=PTR - 4), "overlaps"),
    "clamp_two": (dict(clamp=2), "clamp must be 0 or 1"),
    "clamp_negative": (dict(clamp=-1), "clamp must be 0 or 1"),
}


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_resize_argument_errors(lib, name):
    kw, text = ERRORS[name]
    a = dict(inp=PTR, out=FAR, B=2, C=3, H=40, W=52, Ho=20, Wo=26, sh=0.5, sw=0.5, clamp=0)
    a.update(kw)
    rc = lib.rs_resize(a["inp"], a["out"], a["B"], a["C"], a["H"], a["W"], a["Ho"], a["Wo"], a["sh"], a["sw"], a["clamp"], None)
    assert rc == -2 and text in _lib.last_error() and _lib.last_error().startswith("rs_resize: "), (rc, _lib.last_error())


def test_the_symbol_is_declared(lib):
    assert hasattr(lib, "rs_resize") and len(_lib.SIGNATURES["rs_resize"][1]) == 12
    header = open(H.ROOT + "/include/resshift_hip.h").read()
    for text in ("int rs_resize(const float* in, float* out, int B, int C, int H, int W, int Ho, int Wo, double scale_h, double scale_w, int clamp,",
                 "u    = (i + 1) / s + 0.5 (1 - 1/s)", "left = floor(u - kw / 2)", "q = (j - 1) mod 2n,   q < n ? q : 2n - 1 - q",
                 "P = ceil(kw) + 2", "A = -0.5", "tests/_resize_ref.py"):
        assert text in header, text
    assert "resize.hip" in build.SOURCES and _lib.RESIZE_SCALES == (0.125, 8.0)


def test_lib_resize_rejects_bad_arguments_before_the_library_is_called(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was reached"))
    x = torch.zeros(1, 3, 40, 52)
    with pytest.raises(ValueError, match="contiguous float32 device tensor"):
        _lib.resize(x, scale=0.5)                      # a host tensor: there is no CPU arithmetic to fall back to
    d = x.as_subclass(_OnDevice)
    with pytest.raises(ValueError, match="contiguous float32 device tensor"):
        _lib.resize(d.double(), scale=0.5)
    with pytest.raises(ValueError, match="contiguous float32 device tensor"):
        _lib.resize(d[..., ::2], scale=0.5)
    with pytest.raises(ValueError, match="contiguous float32 device tensor"):
        _lib.resize(d[0], scale=0.5)
    for kw in (dict(), dict(scale=0.5, size=(20, 26))):
        with pytest.raises(ValueError, match="exactly one of scale and size"):
            _lib.resize(d, **kw)
    for bad in (0, -1.0, "2", True, float("nan")):
        with pytest.raises(ValueError, match="scale must be a positive number"):
            _lib.resize(d, scale=bad)
    for bad in ((20,), (20, 26, 3), (20.0, 26), (0, 26), (20, -1), 20, (True, 26)):
        with pytest.raises(ValueError, match="size must be two positive integers"):
            _lib.resize(d, size=bad)
    for kw in (dict(scale=0.12), dict(scale=8.5), dict(size=(4, 26)), dict(size=(20, 417))):
        with pytest.raises(ValueError, match=r"must lie in \[1/8, 8\]"):
            _lib.resize(d, **kw)


# ---------------------------------------------------------------------------------------------------------------- host plumbing
def test_out_scale_is_validated_by_the_constructor():
    from resshift_amd.sampler import ResShiftSampler

    for bad in (0, -2, "2", True, float("nan"), [2]):
        with pytest.raises(ValueError, match="out_scale must be None or a positive number"):
            ResShiftSampler({}, out_scale=bad)            # validated like `color_fix`: before anything is built
    for bad, sf in ((0.4, 4), (33, 4), (0.1, 1), (8.5, 1), (17, 2)):
        with pytest.raises(ValueError, match="is outside"):
            ResShiftSampler({}, sf=sf, out_scale=bad)
    with pytest.raises(ValueError, match="unknown colour fix"):
        ResShiftSampler({}, color_fix="ycbcr", out_scale=2)
    for ok, sf in ((None, 4), (4, 4), (4.0, 4), (2, 4), (3, 4), (0.5, 4), (32, 4), (1.5, 1), (0.125, 1), (8, 1), (Fraction(3, 2), 2)):
        tiling.check_out_scale(ok, sf)
    assert not tiling.resizes(None, 4) and not tiling.resizes(4, 4) and not tiling.resizes(4.0, 4)
    assert tiling.resizes(2, 4) and tiling.resizes(4, 2) and tiling.resizes(3.999, 4)


@pytest.mark.parametrize("fix", ["none", "wavelet"])
@pytest.mark.parametrize("out_scale", ["absent", None, 4, 4.0, 2, 0.7, 6])
def test_tile_pool_resizes_each_completed_image_once(fake_launches, out_scale, fix):
    """the scale is the sampler's; the resize sees whole blended images after the colour fix, never a tile; None, a sampler without the
    attribute and a value equal to sf never reach the engine's call"""
    s = fake_sampler(color_fix=fix, **({} if out_scale == "absent" else {"out_scale": out_scale}))
    tp = TilePool(s, max_batch=4, seeded=True)
    assert tp.out_scale == (None if out_scale == "absent" else out_scale)
    sizes = [(40, 28), (13, 10)]          # six tiles; one whole image
    for i, (Hh, W) in enumerate(sizes):
        lq = torch.zeros(3, Hh, W)
        for k, (h0, w0, _, _) in enumerate(tile_windows(Hh, W, 16, 12)):
            lq[0, h0, w0] = (16 * i + k + 1) * 1e-3
        assert tp.submit(lq, seed=i) == i
    out = tp.drain()
    assert sorted(out) == [0, 1]
    calls = s.engine.calls
    n_fix = 0 if fix == "none" else 2
    assert [c[0] for c in calls].count("color_fix") == n_fix
    if out_scale in ("absent", None, 4, 4.0):
        assert len(calls) == n_fix and all(tuple(out[i].shape) == (3, 4 * h, 4 * w) for i, (h, w) in enumerate(sizes))
        return
    assert len(calls) == n_fix + 2
    for i, (Hh, W) in enumerate(sizes):
        mine = [c for c in calls if c[1] == (1, 3, 4 * Hh, 4 * W)]
        assert [c[0] for c in mine] == (["color_fix"] if n_fix else []) + ["resize"]          # the fix first
        _, _, seen_min, scale, size, clamp = mine[-1]
        assert scale is None and clamp is True and size == tiling.out_size(Hh, W, out_scale)
        assert (seen_min >= 1.0) == (fix != "none")                                              # the resize saw the fixed image
        assert tuple(out[i].shape) == (3, *size) and out[i].min().item() >= 10.0               # the pool returns what the resize returned
    assert tiling.out_size(40, 28, 0.7) == (28, 20)


@pytest.mark.parametrize("size", [(40, 28), (16, 12)], ids=["tiled", "untiled"])
@pytest.mark.parametrize("fix", ["none", "adain"])
@pytest.mark.parametrize("out_scale", ["absent", None, 4, 2, 3])
def test_sample_tiled_resizes_the_image_it_returns(monkeypatch, out_scale, fix, size):
    from resshift_amd.sampler import ResShiftSampler

    fake_lib = SimpleNamespace(rs_tile_accumulate=lambda *a: 0, rs_tile_finalize=lambda *a: 0)
    monkeypatch.setattr(_lib, "load", lambda: fake_lib)
    monkeypatch.setattr(_lib, "window_copy", lambda x, h0, w0, ho, wo, out=None: out.copy_(x[..., h0:h0 + ho, w0:w0 + wo]))
    s = ResShiftSampler.__new__(ResShiftSampler)
    s.chop_size, s.chop_stride, s.chop_bs, s.sf, s.tile_blend, s.color_fix = 16, 12, 2, 4, "uniform", fix
    if out_scale != "absent":
        s.out_scale = out_scale
    s.engine = FakeEngine()
    tiles = []

    def sample_func(pch, noise_repeat=False, mask=None, noise=None, step_noises=None, seeds=None):
        tiles.append(tuple(pch.shape))
        return torch.zeros(pch.shape[0], 3, pch.shape[2] * 4, pch.shape[3] * 4)

    s.sample_func = sample_func
    im = torch.rand(1, 3, *size).as_subclass(_OnDevice)
    out = s.sample_tiled(im, seed=3)
    assert len(tiles) == (3 if size[0] > 16 else 1)               # tiles are sampled as ever, and never resized one by one
    full = (1, 3, size[0] * 4, size[1] * 4)
    want = [("color_fix", full, "adain")] if fix != "none" else []
    if out_scale in ("absent", None, 4):
        assert s.engine.calls == want and tuple(out.shape) == full
    else:   # once, on the whole image, after the tiles and after the fix
        target = (size[0] * out_scale, size[1] * out_scale)
        assert s.engine.calls == want + [("resize", full, 1.0 if fix != "none" else 0.0, None, target, True)]
        assert tuple(out.shape) == (1, 3, *target) and out.min().item() >= 10.0


def test_a_mask_excludes_another_output_scale():
    """inpainting blends with lq and mask at the model's size (sf = 1): sample_tiled(mask=), inference(mask_path=) and a TilePool over a
    cond_mask model raise when out_scale differs from sf; None and sf itself leave all three as they are"""
    from resshift_amd.sampler import ResShiftSampler

    s = ResShiftSampler.__new__(ResShiftSampler)
    s.chop_size, s.chop_stride, s.chop_bs, s.sf, s.tile_blend, s.color_fix = 16, 12, 1, 1, "uniform", "none"
    for scale in (2, 0.5):
        s.out_scale = scale
        with pytest.raises(ValueError, match=f"out_scale={scale!r} is undefined for a masked input"):
            s.sample_tiled(torch.zeros(1, 3, 16, 12), mask=torch.zeros(1, 1, 16, 12))
        with pytest.raises(ValueError, match=f"out_scale={scale!r} is undefined for masked"):
            s.inference("in", "out", mask_path="masks")
        with pytest.raises(ValueError, match=f"out_scale={scale!r} is undefined for a model conditioned on a mask"):
            TilePool(fake_sampler(cond_mask=True, out_scale=scale))
    assert TilePool(fake_sampler(cond_mask=True, out_scale=4)).out_scale == 4          # (TINY_DIFFUSION: sf = 4)
    assert TilePool(fake_sampler(cond_mask=True, out_scale=None)).out_scale is None
    assert TilePool(fake_sampler(cond_mask=True)).out_scale is None
    with pytest.raises(ValueError, match="out_scale must be None or a positive number"):
        TilePool(fake_sampler(out_scale="2"))
    with pytest.raises(ValueError, match="is outside"):
        TilePool(fake_sampler(out_scale=40))
    # a mask under out_scale = sf goes on to the sampler as ever
    s.out_scale, seen = 1, []
    s.sample_func = lambda im, mask=None, **kw: seen.append(mask is not None) or torch.zeros(1, 3, 16, 12)
    s.sample_tiled(torch.zeros(1, 3, 16, 12), mask=torch.zeros(1, 1, 16, 12))
    assert seen == [True]

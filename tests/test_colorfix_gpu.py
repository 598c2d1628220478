"""Colour correction on the GPU (tiny shapes, the file prints its wall time).  The reference is the float64 restatement of
the definition, tests/_colorfix_ref.py.  Every case is B = 2, C = 3:

    (5, 7, 4)    the 20 x 28 output is smaller than the 31-pixel reach: every level clamps on all sides
    (40, 52, 4)  160 x 208: several workgroup tiles with ragged edges
    (33, 20, 2)  sf = 2
    (70, 37, 1)  no up-sampling; widths that are no multiple of four

  * wavelet against the restatement, 1e-5 on every element;
  * launch-geometry independence, bit for bit: a crop whose origin is no multiple of any tile, and B = 1 calls against the batch;
  * adain against the restatement, with a low-contrast plane on which E[x^2] - mean^2 loses the variance in fp32;
  * end to end on the tiny parity-policy sampler of tests/test_feather_gpu.py: sample_tiled, the tile pool and inference.
"""
import time

import numpy as np
import pytest
import torch

import helpers as H
import _colorfix_ref as R
from oracle import make_golden_tiled as mt

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# absolute, wavelet: |D| <= 3; about 20 fp32 roundings go into a bicubic tap sum (weights of magnitude <= 1.2, taps in [-1, 1]) and about
# 30 through five convex levels (three per 1-D pass), each <= 2^-24 * 3 = 1.8e-7 and none amplified: 50 * 1.8e-7 = 9e-6 worst case, all
# aligned.  One level missing, reflect instead of clamp or the reversed level order move pixels by 0.05 .. 0.27 (tests/test_colorfix_cpu.py).
TOL_WAVELET = 1e-5
_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    yield
    print(f"\ntests/test_colorfix_gpu.py: {time.time() - _T0:.1f} s wall time")


_CASES = {}


def _case(shape, gpu):
    """inputs (host and device) of one shape, made once and never modified"""
    if shape not in _CASES:
        sr, lq = R.low_contrast_inputs() if shape == "low" else R.inputs(*shape)
        _CASES[shape] = (sr, lq, sr.to(gpu), lq.to(gpu))
    return _CASES[shape]


def _ids(s):
    return s if isinstance(s, str) else "x".join(map(str, s))


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("shape", R.SHAPES, ids=_ids)
def test_wavelet_against_the_float64_restatement(gpu, shape):
    from resshift_amd import _lib

    sr, lq, sr_d, lq_d = _case(shape, gpu)
    want = R.wavelet(sr.numpy(), lq.numpy(), shape[2])
    share = R.saturated_share(want)
    got = _lib.color_fix(sr_d, lq_d, "wavelet")
    assert got.data_ptr() != sr_d.data_ptr() and torch.equal(sr_d.cpu(), sr) and torch.equal(lq_d.cpu(), lq)   # the inputs are only read
    err = float(np.abs(got.cpu().double().numpy() - want).max())
    moved = float(np.abs(want - sr.double().numpy()).max())
    print(f"wavelet {shape}: max |device - float64 restatement| = {err:.3e} (bound {TOL_WAVELET:.0e}); share at +-1 = {share:.3f}; "
          f"the correction moves pixels by up to {moved:.3f}")
    assert share < 0.10, share
    assert err <= TOL_WAVELET, err


def test_wavelet_does_not_depend_on_the_launch_geometry(gpu):
    """(40, 52, 4) against the call on the crop LR rows 3..35, cols 5..50 (sr rows 12..140, cols 20..200): the crop's origin is no multiple
    of a workgroup tile, so a pixel lands in another tile, at another place of it.  Every output pixel at least 40 pixels from all four
    crop borders - 31 for the levels, 8 for the bicubic taps, one to spare - must be bit for bit the pixel of the full run (the bicubic
    fractions are exact at sf = 4)."""
    from resshift_amd import _lib

    _, _, sr_d, lq_d = _case((40, 52, 4), gpu)
    full = _lib.color_fix(sr_d, lq_d, "wavelet")
    crop = _lib.color_fix(sr_d[:, :, 12:140, 20:200].contiguous(), lq_d[:, :, 3:35, 5:50].contiguous(), "wavelet")
    assert tuple(crop.shape) == (2, 3, 128, 180)
    inner = crop[:, :, 40:-40, 40:-40]
    assert inner.shape[2] == 48 and inner.shape[3] == 100
    assert torch.equal(inner, full[:, :, 52:100, 60:160])
    assert not torch.equal(crop[:, :, :8], full[:, :, 12:20, 20:200])    # (near the crop's border the two images do differ)


@pytest.mark.parametrize("mode", ["wavelet", "adain"])
@pytest.mark.parametrize("shape", [(40, 52, 4), (70, 37, 1)], ids=_ids)
def test_an_image_does_not_depend_on_its_batch(gpu, shape, mode):
    from resshift_amd import _lib

    _, _, sr_d, lq_d = _case(shape, gpu)
    batch = _lib.color_fix(sr_d, lq_d, mode)
    for b in range(sr_d.shape[0]):
        alone = _lib.color_fix(sr_d[b:b + 1].clone(), lq_d[b:b + 1].clone(), mode)
        assert torch.equal(batch[b], alone[0]), (shape, mode, b)


@pytest.mark.parametrize("shape", R.SHAPES + ["low"], ids=_ids)
def test_adain_against_the_float64_restatement(gpu, shape):
    """per plane 2e-6 + 8 * 2^-24 * (1 + |mean_sr| / std_sr) * std_lq (_colorfix_ref.adain_tolerance).  The low-contrast case (sr = 0.9 +
    0.01 randn, lq = 0.2 + 0.3 randn): about 1.5e-5, where a centred fp32 computation measures 2e-6 and E[x^2] - mean^2 6e-4 on the CPU
    (tests/test_colorfix_cpu.py) - it separates the two forms."""
    from resshift_amd import _lib

    sr, lq, sr_d, lq_d = _case(shape, gpu)
    want = R.adain(sr.numpy(), lq.numpy())
    tol = R.adain_tolerance(sr.numpy(), lq.numpy())
    share = R.saturated_share(want)
    got = _lib.color_fix(sr_d, lq_d, "adain")
    err = np.abs(got.cpu().double().numpy() - want)
    print(f"adain {shape}: max |device - float64 restatement| = {err.max():.3e} (per-plane bounds {tol.min():.2e} .. {tol.max():.2e}); "
          f"share at +-1 = {share:.3f}")
    assert share < 0.10, share
    assert np.all(err <= tol), float((err / tol).max())


def test_engine_color_fix_is_the_library_call(gpu):
    """Engine.color_fix accepts what the samplers hand it (any float dtype, strided views) and defaults to wavelet"""
    s, _ = _sampler(1)
    _, _, sr_d, lq_d = _case((33, 20, 2), gpu)
    from resshift_amd import _lib

    want = _lib.color_fix(sr_d, lq_d, "wavelet")
    assert torch.equal(s.engine.color_fix(sr_d, lq_d), want)
    assert torch.equal(s.engine.color_fix(sr_d.double(), lq_d.flip(0).flip(0), mode="wavelet"), want)
    with pytest.raises(ValueError, match="unknown colour fix"):
        s.engine.color_fix(sr_d, lq_d, "ycbcr")
    with pytest.raises(ValueError, match="no integer multiple"):
        s.engine.color_fix(sr_d[:, :, :-1], lq_d, "adain")


# ---------------------------------------------------------------------------------------------------------------- end to end
_SAMPLER = []
SEED = 20240607


def _sampler(chop_bs, fix="wavelet"):
    """tests/test_feather_gpu.py::_sampler's tiny case under the parity policy, built once with color_fix="wavelet"; `color_fix` is a plain
    attribute like the tiling parameters"""
    from resshift_amd import ResShiftSampler
    from resshift_amd.config import ConfigNode

    up, ap, dp, _ = H.CASES["tiny"]
    if not _SAMPLER:
        usd, asd = H.weights(up, ap)
        cfg = ConfigNode(model=ConfigNode(target="models.unet.UNetModelSwin", ckpt_path=None, params=up),
                         diffusion=ConfigNode(target="models.script_util.create_gaussian_diffusion", params=dp),
                         autoencoder=ConfigNode(target="ldm.models.autoencoder.VQModelTorch", ckpt_path=None, params=ap))
        sd = {"model": usd, "autoencoder": asd}
        _SAMPLER.append(ResShiftSampler(cfg, sf=dp["sf"], seed=1, precision="parity", color_fix="wavelet", state_dicts=sd))
        assert _SAMPLER[0].color_fix == "wavelet" and _SAMPLER[0].tile_blend == "uniform"
        _SAMPLER.append(ResShiftSampler(cfg, sf=dp["sf"], seed=1, precision="parity", state_dicts=sd))   # constructed without the argument
        assert _SAMPLER[1].color_fix == "none"
    s = _SAMPLER[0]
    s.chop_size, s.chop_stride, s.chop_bs, s.padding_offset, s.color_fix = 16, 12, chop_bs, 16, fix
    return s, dp


def _plain_sampler(chop_bs):
    _sampler(chop_bs)
    s = _SAMPLER[1]
    s.chop_size, s.chop_stride, s.chop_bs, s.padding_offset = 16, 12, chop_bs, 16
    return s


@pytest.mark.parametrize("size", ["tiled", "untiled"])
def test_sample_tiled_fixes_the_image_it_returns(gpu, size):
    """the 40 x 28 fixture image (six tiles) and its 16 x 16 corner (straight to sample_func): under "wavelet" sample_tiled(seed=) is
    engine.color_fix of what it returns under "none"; under "none" it is what a sampler constructed without the argument returns"""
    y = mt.tiled_inputs(H.CASES["tiny"][2]["steps"])[0].to(gpu)
    assert tuple(y.shape) == (1, 3, 40, 28)
    if size == "untiled":
        y = y[:, :, :16, :16].contiguous()
    s, dp = _sampler(2, "none")
    plain = s.sample_tiled(y, seed=SEED)
    assert torch.equal(plain, _plain_sampler(2).sample_tiled(y, seed=SEED))
    s, _ = _sampler(2, "wavelet")
    fixed = s.sample_tiled(y, seed=SEED)
    assert tuple(fixed.shape) == (1, 3, y.shape[2] * dp["sf"], y.shape[3] * dp["sf"])
    assert torch.equal(fixed, s.engine.color_fix(plain, y, "wavelet"))
    moved = (fixed - plain).abs().max().item()
    print(f"sample_tiled {size}: the wavelet fix moves pixels by up to {moved:.3f}")
    assert moved > 0
    s, _ = _sampler(2, "adain")
    assert torch.equal(s.sample_tiled(y, seed=SEED), s.engine.color_fix(plain, y, "adain"))


def test_pool_equals_sample_tiled_under_the_fix_when_the_image_is_one_batch(gpu):
    from resshift_amd.tilepool import TilePool

    s, dp = _sampler(6, "wavelet")
    y = mt.tiled_inputs(dp["steps"])[0].to(gpu)
    ref = s.sample_tiled(y, seed=SEED)
    tp = TilePool(s, max_batch=6, keep_log=True, seeded=True)
    assert tp.color_fix == "wavelet"
    rid = tp.submit(y, seed=SEED)
    out = tp.drain()
    torch.cuda.synchronize()
    assert list(out) == [rid] and all(len(b) == 6 for b in tp.batches) and len(tp.batches) == dp["steps"]
    assert torch.equal(out[rid], ref[0])
    s.color_fix = "none"
    tp = TilePool(s, max_batch=6, seeded=True)
    rid = tp.submit(y, seed=SEED)
    assert not torch.equal(tp.drain()[rid], ref[0])


def test_inference_writes_the_fixed_image(gpu, tmp_path):
    """inference(seeded=True) on a one-file folder, with and without the pool: the PNG is output_to_u8 of the fixed tensor"""
    from PIL import Image

    from resshift_amd.tilepool import TilePool

    s, dp = _sampler(6, "wavelet")
    src = tmp_path / "in"
    src.mkdir()
    y = mt.tiled_inputs(dp["steps"])[0]
    Image.fromarray(((y[0].permute(1, 2, 0) * 0.5 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).numpy()).save(src / "a.png")
    lq = s.engine.u8_to_input(s._read_image_u8(src / "a.png").unsqueeze(0).to(gpu))
    want_t = s.sample_tiled(lq, seed=[s.image_seed(0)])
    want = s.engine.output_to_u8(want_t)[0].cpu().numpy()
    s.inference(src, tmp_path / "out", bs=1, seeded=True)
    got = np.asarray(Image.open(tmp_path / "out" / "a.png"))
    assert got.shape == (160, 112, 3) and np.array_equal(got, want)
    s.color_fix = "none"
    s.inference(src, tmp_path / "plain", bs=1, seeded=True)
    assert not np.array_equal(np.asarray(Image.open(tmp_path / "plain" / "a.png")), want)
    s.color_fix = "wavelet"
    s.inference(src, tmp_path / "pool", bs=1, seeded=True, pool=True)
    tp = TilePool(s, seeded=True)
    rid = tp.submit(lq, seed=s.image_seed(0))
    want_pool = s.engine.output_to_u8(tp.drain()[rid].unsqueeze(0))[0].cpu().numpy()
    assert np.array_equal(np.asarray(Image.open(tmp_path / "pool" / "a.png")), want_pool)

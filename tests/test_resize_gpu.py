"""Antialiased resize on the GPU (tiny shapes, the file prints its wall time).  The reference is the float64 restatement of
the definition, tests/_resize_ref.py; its cases (B = 2, C = 3, inputs uniform in (-1, 1) from a fixed numpy seed) are listed there.

  * every case against the restatement, 2e-5 on every element, clamp 0 and 1; the scale-form cases against the recorded outputs of the
    reference's imresize_np (tests/golden/reference_resize.npz);
  * scale 1 is the identity, bit for bit;
  * launch-geometry independence, bit for bit: B = 1 calls against the batch, and a crop whose origin is no multiple of any tile;
  * end to end on the tiny parity-policy sampler of tests/test_colorfix_gpu.py: sample_tiled, the tile pool and inference under
    out_scale = 2 on the x4 model.
"""
import time

import numpy as np
import pytest
import torch

import helpers as H
import _resize_ref as R
from oracle import make_golden_tiled as mt

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# absolute, on every element.  The reference's all-fp32 arithmetic (fp32 coordinates included) stays within 4.3e-6 of float64 on these
# cases (tests/test_resize_cpu.py); a kernel with exact coordinates has no reason to be farther away, and gets five times that.  The
# smallest mutation of the definition (no normalisation, 0.75) moves a pixel by 2.2e-2.
TOL = 2e-5
_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    yield
    print(f"\ntests/test_resize_gpu.py: {time.time() - _T0:.1f} s wall time")


_CASES = {}


def _case(case, gpu):
    """input (host numpy, host torch, device) and float64 restatement of one case, made once and never modified"""
    key = R.case_id(case)
    if key not in _CASES:
        (Hh, W), kind, v = case
        x = R.inputs(Hh, W)
        _CASES[key] = (x, torch.from_numpy(x), torch.from_numpy(x).to(gpu), R.resize(x, **{kind: v}))
    return _CASES[key]


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_resize_against_the_float64_restatement(gpu, case):
    from resshift_amd import _lib

    _, kind, v = case
    x, x_t, x_d, want = _case(case, gpu)
    got = _lib.resize(x_d, **{kind: v})
    assert got.data_ptr() != x_d.data_ptr() and torch.equal(x_d.cpu(), x_t)             # the input is only read
    assert tuple(got.shape) == want.shape and got.dtype == torch.float32
    err = float(np.abs(got.cpu().double().numpy() - want).max())
    clamped = _lib.resize(x_d, **{kind: v}, clamp=True)
    assert torch.equal(x_d.cpu(), x_t)
    want_c = np.clip(want, -1.0, 1.0)
    err_c = float(np.abs(clamped.cpu().double().numpy() - want_c).max())
    share = R.saturated_share(clamped.cpu().numpy())
    print(f"resize {R.case_id(case)}: max |device - float64 restatement| = {err:.3e}, clamped {err_c:.3e} (bound {TOL:.0e}); "
          f"share at +-1 = {share:.4f} (restatement {R.saturated_share(want_c):.4f}); overshoot up to {np.abs(want).max():.3f}")
    assert err <= TOL, err
    assert err_c <= TOL, err_c
    assert torch.equal(clamped, got.clamp(-1, 1))
    assert share < 0.10, share
    if kind == "scale" and v > 1:
        assert share > 0, "the upscale cases overshoot [-1, 1]: the clamp must have something to do"


@pytest.mark.parametrize("case", R.GOLDEN_CASES, ids=R.case_id)
def test_resize_against_the_recorded_reference(gpu, case):
    """image 0 against what the reference's imresize_np returned for it: 2e-5 plus the distance of the float64 restatement from that
    all-fp32 reference on the same case"""
    from resshift_amd import _lib

    _, _, scale = case
    _, _, x_d, want = _case(case, gpu)
    gold = np.load(H.ROOT + "/tests/golden/reference_resize.npz")["out_" + R.golden_key(case)].transpose(2, 0, 1).astype(np.float64)
    slack = float(np.abs(want[0] - gold).max())
    err = float(np.abs(_lib.resize(x_d, scale=scale)[0].cpu().double().numpy() - gold).max())
    print(f"resize {R.case_id(case)}: max |device - imresize_np| = {err:.3e} (restatement - imresize_np: {slack:.3e})")
    assert slack <= 1e-5 and err <= TOL + slack, (err, slack)


def test_scale_one_is_the_identity(gpu):
    from resshift_amd import _lib

    _, _, x_d, _ = _case(R.CASES[2], gpu)
    assert torch.equal(_lib.resize(x_d, scale=1), x_d)              # the weights are exactly 0 and 1
    assert torch.equal(_lib.resize(x_d, size=tuple(x_d.shape[2:])), x_d)
    assert torch.equal(_lib.resize(x_d, scale=1.0, clamp=True), x_d)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_an_image_does_not_depend_on_its_batch(gpu, case):
    from resshift_amd import _lib

    _, kind, v = case
    _, _, x_d, _ = _case(case, gpu)
    batch = _lib.resize(x_d, **{kind: v})
    for b in range(x_d.shape[0]):
        alone = _lib.resize(x_d[b:b + 1].clone(), **{kind: v})
        assert torch.equal(batch[b], alone[0]), (case, b)


def test_resize_does_not_depend_on_the_launch_geometry(gpu):
    """(40, 52) at 0.5 against the call on the crop rows 6..38, columns 10..50: the offsets are even, so the fractions and the fp64
    coordinates coincide, and the crop's origin is no multiple of a workgroup tile - a pixel lands in another tile, at another place of
    it.  Every output pixel at least 4 from the crop's border (the ten taps reach 5 input pixels = 2.5 output pixels) is bit for bit the
    pixel of the full run."""
    from resshift_amd import _lib

    x_d = torch.from_numpy(R.inputs(40, 52)).to(gpu)
    full = _lib.resize(x_d, scale=0.5)
    crop = _lib.resize(x_d[:, :, 6:38, 10:50].contiguous(), scale=0.5)
    assert tuple(full.shape) == (2, 3, 20, 26) and tuple(crop.shape) == (2, 3, 16, 20)
    assert torch.equal(crop[:, :, 4:-4, 4:-4], full[:, :, 7:15, 9:21])
    assert not torch.equal(crop[:, :, :2], full[:, :, 3:5, 5:25])      # (near the crop's border the two images do differ)
    # and the unpadded LDS image of the A/B knob holds the same bits
    import os

    os.environ["RS_RESIZE_LDS"] = "linear"
    try:
        assert torch.equal(_lib.resize(x_d, scale=0.5), full)
    finally:
        del os.environ["RS_RESIZE_LDS"]


# ---------------------------------------------------------------------------------------------------------------- end to end
_SAMPLER = []
SEED = 20240607


def _sampler(chop_bs, out_scale=2, fix="none"):
    """tests/test_colorfix_gpu.py::_sampler's tiny case under the parity policy (sf = 4), built once with out_scale=2; `out_scale` is a
    plain attribute like the tiling parameters"""
    from resshift_amd import ResShiftSampler
    from resshift_amd.config import ConfigNode

    up, ap, dp, _ = H.CASES["tiny"]
    if not _SAMPLER:
        usd, asd = H.weights(up, ap)
        cfg = ConfigNode(model=ConfigNode(target="models.unet.UNetModelSwin", ckpt_path=None, params=up),
                         diffusion=ConfigNode(target="models.script_util.create_gaussian_diffusion", params=dp),
                         autoencoder=ConfigNode(target="ldm.models.autoencoder.VQModelTorch", ckpt_path=None, params=ap))
        sd = {"model": usd, "autoencoder": asd}
        _SAMPLER.append(ResShiftSampler(cfg, sf=dp["sf"], seed=1, precision="parity", out_scale=2, state_dicts=sd))
        assert _SAMPLER[0].out_scale == 2 and _SAMPLER[0].color_fix == "none" and dp["sf"] == 4
        _SAMPLER.append(ResShiftSampler(cfg, sf=dp["sf"], seed=1, precision="parity", state_dicts=sd))   # constructed without the argument
        assert _SAMPLER[1].out_scale is None
    s = _SAMPLER[0]
    s.chop_size, s.chop_stride, s.chop_bs, s.padding_offset, s.out_scale, s.color_fix = 16, 12, chop_bs, 16, out_scale, fix
    return s, dp


def _plain_sampler(chop_bs, fix="none"):
    _sampler(chop_bs)
    s = _SAMPLER[1]
    s.chop_size, s.chop_stride, s.chop_bs, s.padding_offset, s.color_fix = 16, 12, chop_bs, 16, fix
    return s


def test_engine_resize_is_the_library_call(gpu):
    """Engine.resize accepts what the samplers hand it: any float dtype, strided views"""
    from resshift_amd import _lib

    s, _ = _sampler(1)
    _, _, x_d, _ = _case(R.CASES[8], gpu)
    want = _lib.resize(x_d, size=(17, 64))
    assert torch.equal(s.engine.resize(x_d, size=(17, 64)), want)
    assert torch.equal(s.engine.resize(x_d.double(), size=(17, 64)), want)
    wide = torch.zeros(2, 3, 40, 104, device=gpu)
    wide[..., ::2] = x_d
    assert not wide[..., ::2].is_contiguous() and torch.equal(s.engine.resize(wide[..., ::2], size=(17, 64)), want)
    assert torch.equal(s.engine.resize(x_d.flip(0).flip(0), scale=0.5, clamp=True), _lib.resize(x_d, scale=0.5, clamp=True))
    with pytest.raises(ValueError, match="exactly one of scale and size"):
        s.engine.resize(x_d)
    with pytest.raises(ValueError, match=r"must lie in \[1/8, 8\]"):
        s.engine.resize(x_d, size=(4, 52))


@pytest.mark.parametrize("size,fix", [("tiled", "none"), ("tiled", "wavelet"), ("untiled", "none")])
def test_sample_tiled_resizes_the_image_it_returns(gpu, size, fix):
    """the 40 x 28 fixture image (six tiles) and its 16 x 16 corner (straight to sample_func): under out_scale=2 sample_tiled(seed=) is
    engine.resize(size=(2 H, 2 W), clamp=True) of what it returns under None - with color_fix="wavelet", of the fixed image: the fix
    runs at the model's scale, before the resize; a sampler constructed without the argument, None and out_scale = sf are the same bits"""
    y = mt.tiled_inputs(H.CASES["tiny"][2]["steps"])[0].to(gpu)
    assert tuple(y.shape) == (1, 3, 40, 28)
    if size == "untiled":
        y = y[:, :, :16, :16].contiguous()
    s, dp = _sampler(2, None, fix)
    plain = s.sample_tiled(y, seed=SEED)
    assert tuple(plain.shape) == (1, 3, y.shape[2] * 4, y.shape[3] * 4)
    assert torch.equal(plain, _plain_sampler(2, fix).sample_tiled(y, seed=SEED))
    s, _ = _sampler(2, 4, fix)
    assert torch.equal(plain, s.sample_tiled(y, seed=SEED))
    s, _ = _sampler(2, 2, fix)
    half = s.sample_tiled(y, seed=SEED)
    target = (y.shape[2] * 2, y.shape[3] * 2)
    assert tuple(half.shape) == (1, 3, *target) and target == ((80, 56) if size == "tiled" else (32, 32))
    assert torch.equal(half, s.engine.resize(plain, size=target, clamp=True))
    assert half.abs().max().item() <= 1.0
    if fix != "none":   # the order: resize(fix(x)), not fix(resize(x))
        unfixed = _sampler(2, None, "none")[0].sample_tiled(y, seed=SEED)
        assert not torch.equal(half, s.engine.resize(unfixed, size=target, clamp=True))


def test_pool_equals_sample_tiled_under_out_scale_when_the_image_is_one_batch(gpu):
    from resshift_amd.tilepool import TilePool

    s, dp = _sampler(6, 2)
    y = mt.tiled_inputs(dp["steps"])[0].to(gpu)
    ref = s.sample_tiled(y, seed=SEED)
    assert tuple(ref.shape) == (1, 3, 80, 56)
    tp = TilePool(s, max_batch=6, keep_log=True, seeded=True)
    assert tp.out_scale == 2
    rid = tp.submit(y, seed=SEED)
    out = tp.drain()
    torch.cuda.synchronize()
    assert list(out) == [rid] and all(len(b) == 6 for b in tp.batches) and len(tp.batches) == dp["steps"]
    assert torch.equal(out[rid], ref[0])
    s.out_scale = None
    tp = TilePool(s, max_batch=6, seeded=True)
    rid = tp.submit(y, seed=SEED)
    assert tuple(tp.drain()[rid].shape) == (3, 160, 112)


def test_inference_writes_the_resized_image(gpu, tmp_path):
    """inference(seeded=True) on a one-file folder, with and without the pool: the PNG is output_to_u8 of the resized tensor"""
    from PIL import Image

    from resshift_amd.tilepool import TilePool

    s, dp = _sampler(6, 2)
    src = tmp_path / "in"
    src.mkdir()
    y = mt.tiled_inputs(dp["steps"])[0]
    Image.fromarray(((y[0].permute(1, 2, 0) * 0.5 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).numpy()).save(src / "a.png")
    lq = s.engine.u8_to_input(s._read_image_u8(src / "a.png").unsqueeze(0).to(gpu))
    want_t = s.sample_tiled(lq, seed=[s.image_seed(0)])
    assert tuple(want_t.shape) == (1, 3, 80, 56)
    want = s.engine.output_to_u8(want_t)[0].cpu().numpy()
    s.inference(src, tmp_path / "out", bs=1, seeded=True)
    got = np.asarray(Image.open(tmp_path / "out" / "a.png"))
    assert got.shape == (80, 56, 3) and np.array_equal(got, want)
    s.inference(src, tmp_path / "pool", bs=1, seeded=True, pool=True)
    tp = TilePool(s, seeded=True)
    rid = tp.submit(lq, seed=s.image_seed(0))
    want_pool = s.engine.output_to_u8(tp.drain()[rid].unsqueeze(0))[0].cpu().numpy()
    got_pool = np.asarray(Image.open(tmp_path / "pool" / "a.png"))
    assert got_pool.shape == (80, 56, 3) and np.array_equal(got_pool, want_pool)

"""The face recipe's operators on the GPU (tiny shapes, the file prints its wall time).

  * rs_jpeg_codec: EQUALITY ON EVERY ELEMENT, no tolerance, against the integer restatement tests/_jpeg_ref.py and against what Pillow's
    libjpeg returned (tests/golden/libjpeg_roundtrip.npz) - every size of J.SIZES with every content, every quality of J.QUALITIES, a
    batch of five qualities against its B = 1 calls, B = 65 for the chunking;
  * rs_blur_resize: against the float64 restatement tests/_face_ref.py within F.TOL = five times the distance of the reference's own fp32
    outputs from it, which tests/test_face_degrade_cpu.py measures and pins (1e-5 absolute, on every element); a delta kernel, B = 1
    against the batch and rs_filter2d at equal size bit for bit; without a kernel rs_interp's bits;
  * two hand-written FacePlans, every stage teacher-forced against the restatements; make_face_testset; make_lq / the command line /
    Engine.metrics.
"""
import json
import time

import numpy as np
import pytest
import torch

import helpers as H
import _degrade_ref as D
import _face_ref as F
import _jpeg_ref as J

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    yield
    print(f"\ntests/test_face_degrade_gpu.py: {time.time() - _T0:.1f} s wall time")


@pytest.fixture(scope="module")
def fixture():
    return np.load(H.ROOT + "/tests/golden/libjpeg_roundtrip.npz")


def _dev(x, gpu):
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


def _as_u8(y):
    """the codec's fp32 [B,3,H,W] output -> uint8 [B,H,W,3]; asserts that every value is v / 255 exactly"""
    y = y.cpu().numpy()
    u8 = np.rint(y * np.float32(255)).astype(np.uint8)
    assert np.array_equal(u8.astype(np.float32) / np.float32(255), y), "an output is not (float) v / 255.f"
    return u8.transpose(0, 2, 3, 1)


# ---------------------------------------------------------------------------------------------------------------- rs_jpeg_codec
@pytest.mark.parametrize("si", range(len(J.SIZES)), ids=[f"{h}x{w}" for h, w in J.SIZES])
def test_codec_equals_libjpeg_on_every_byte(gpu, fixture, si):
    """the five contents of one size as ONE batch with the recorded qualities: equal to Pillow's output and to the restatement"""
    from resshift_amd import _lib

    Hh, W = J.SIZES[si]
    mine = [c for c in J.cases() if c[1] == (Hh, W)]
    x = np.stack([J.content(kind, Hh, W, seed) for _, _, kind, seed, _ in mine])
    q = [c[4] for c in mine]
    for i, (key, *_) in enumerate(mine):
        assert np.array_equal(J.to_u8(x[i]), fixture["in_" + key]) and int(fixture["q_" + key]) == q[i]   # the generator has not drifted
    x_d = _dev(x, gpu)
    got = _lib.jpeg_codec(x_d, q)
    assert got.data_ptr() != x_d.data_ptr() and torch.equal(x_d.cpu(), torch.from_numpy(x)) and got.dtype == torch.float32
    u8 = _as_u8(got)
    for i, (key, *_) in enumerate(mine):
        diff = int((u8[i] != fixture["out_" + key]).sum())
        print(f"jpeg_codec {key} q = {q[i]}: {diff} of {u8[i].size} bytes differ from libjpeg's")
        assert diff == 0, (key, q[i], diff)
        assert np.array_equal(u8[i], J.roundtrip(fixture["in_" + key], q[i]))
    assert np.array_equal(got.cpu().numpy(), J.codec(x, q))                                       # the fp32 values themselves
    for i in range(len(mine)):   # an image does not depend on its batch or its position in it
        assert torch.equal(_lib.jpeg_codec(x_d[i:i + 1].clone(), [q[i]])[0], got[i]), (mine[i][0], "B = 1")


@pytest.mark.parametrize("q", J.QUALITIES)
def test_codec_equals_the_restatement_at_every_quality(gpu, q):
    """every size x every content at one quality (scripts/make_golden_jpeg.py confirmed the restatement against Pillow on all of these)"""
    from resshift_amd import _lib

    for si, (Hh, W) in enumerate(J.SIZES):
        x = np.stack([J.content(kind, Hh, W, 1000 + 10 * si + ci) for ci, kind in enumerate(J.CONTENTS)])
        got = _lib.jpeg_codec(_dev(x, gpu), q)
        assert np.array_equal(got.cpu().numpy(), J.codec(x, [q] * len(x))), ((Hh, W), q)


def test_codec_chunks_a_batch_of_65(gpu):
    from resshift_amd import _lib

    rng = np.random.default_rng(7)
    x = rng.uniform(-0.1, 1.1, (65, 3, 17, 33)).astype(np.float32)
    q = [int(v) for v in rng.integers(1, 101, 65)]
    got = _lib.jpeg_codec(_dev(x, gpu), q)
    assert np.array_equal(got.cpu().numpy(), J.codec(x, q))


def test_codec_through_the_engine_and_its_errors(gpu):
    from resshift_amd import _lib
    from resshift_amd.imageops import ImageOps

    x = _dev(J.content("smooth", 24, 72, 3)[None], gpu)
    assert torch.equal(ImageOps(gpu).jpeg_codec(x, [50]), _lib.jpeg_codec(x, 50))
    lib = _lib.load()
    out = torch.empty_like(x)
    import ctypes as C

    one = (C.c_int * 1)(50)
    call = lambda *a: lib.rs_jpeg_codec(*a, _lib.current_stream_ptr())
    for args, text in (((None, out.data_ptr(), one, 1, 3, 24, 72), "rs_jpeg_codec: null pointer (in / out / quality)"),
                       ((x.data_ptr(), out.data_ptr(), one, 0, 3, 24, 72), "rs_jpeg_codec: B must be 1 .. RS_MAX_ROWS (the qualities travel by value)"),
                       ((x.data_ptr(), out.data_ptr(), one, 1, 4, 24, 72), "rs_jpeg_codec: C must be 3 (RGB)"),
                       ((x.data_ptr(), out.data_ptr(), one, 1, 3, 7, 72), "rs_jpeg_codec: H and W must be at least 8"),
                       ((x.data_ptr(), out.data_ptr(), (C.c_int * 1)(0), 1, 3, 24, 72), "rs_jpeg_codec: every quality must be an integer in 1 .. 100"),
                       ((x.data_ptr(), out.data_ptr(), (C.c_int * 1)(101), 1, 3, 24, 72), "rs_jpeg_codec: every quality must be an integer in 1 .. 100"),
                       ((x.data_ptr(), x.data_ptr(), one, 1, 3, 24, 72), "rs_jpeg_codec: `out` overlaps `in` (a tile reads the chroma ring of its neighbours: not in place)")):
        assert call(*args) == -2 and _lib.last_error() == text, (args, _lib.last_error())


# ---------------------------------------------------------------------------------------------------------------- rs_blur_resize
@pytest.mark.parametrize("index", range(len(F.BLUR_KERNELS)), ids=[c[0] for c in F.BLUR_KERNELS])
def test_blur_resize_against_the_float64_restatement(gpu, index):
    from resshift_amd import _lib

    x, kernels = F.blur_case(index)
    x_d, k_d = _dev(x, gpu), _dev(kernels, gpu)
    for size in F.BLUR_SIZES + F.GPU_EXTRA_SIZES:
        want = F.blur_resize(x, kernels, size)
        got = _lib.blur_resize(x_d, k_d, size)
        assert tuple(got.shape) == want.shape and got.dtype == torch.float32 and torch.equal(x_d.cpu(), torch.from_numpy(x))
        err = float(np.abs(got.cpu().double().numpy() - want).max())
        print(f"blur_resize {F.BLUR_KERNELS[index][0]} {F.BLUR_SHAPE} -> {size}: max |device - float64 restatement| = {err:.3e} (bound {F.TOL:.1e})")
        assert err <= F.TOL, (size, err)
        assert torch.equal(_lib.blur_resize(x_d, k_d, size, clamp=True), got.clamp(0, 1))
        for b in range(2):   # an image does not depend on its batch
            kb = k_d if k_d.shape[0] == 1 else k_d[b:b + 1].clone()
            assert torch.equal(_lib.blur_resize(x_d[b:b + 1].clone(), kb, size)[0], got[b]), (size, b)
    if kernels.shape[-1] <= _lib.FILTER_KMAX:   # at equal size it is rs_filter2d, 0 ulp
        assert torch.equal(_lib.blur_resize(x_d, k_d, F.BLUR_SHAPE), _lib.filter2d(x_d, k_d))


@pytest.mark.parametrize("k", [3, 21, 41])
def test_a_delta_kernel_is_the_identity(gpu, k):
    from resshift_amd import _lib

    x_d = _dev(D.inputs((2, 3, *F.BLUR_SHAPE), 5), gpu)
    delta = torch.zeros(2, k, k, device=gpu)
    delta[:, k // 2, k // 2] = 1.0
    assert torch.equal(_lib.blur_resize(x_d, delta, F.BLUR_SHAPE), x_d)
    for size in F.BLUR_SIZES[1:]:   # and under a resize it is the resize
        assert torch.equal(_lib.blur_resize(x_d, delta, size), _lib.blur_resize(x_d, None, size)), size


@pytest.mark.parametrize("i", range(len(F.RESIZE_CASES)))
def test_resize_without_a_kernel(gpu, i):
    from resshift_amd import _lib

    shape, size = F.RESIZE_CASES[i]
    x = D.inputs((2, 3, *shape), F.RESIZE_SEED + i)
    x_d = _dev(x, gpu)
    got = _lib.blur_resize(x_d, None, size)
    err = float(np.abs(got.cpu().double().numpy() - F.blur_resize(x, None, size)).max())
    print(f"blur_resize without a kernel {shape} -> {size}: max |device - float64 restatement| = {err:.3e} (bound {F.TOL:.1e})")
    assert tuple(got.shape) == (2, 3, *size) and err <= F.TOL, err
    assert torch.equal(_lib.blur_resize(x_d[1:].clone(), None, size)[0], got[1])
    if all(0.125 <= o / n <= 8 for o, n in zip(size, shape)):   # inside rs_interp's range it is rs_interp
        assert torch.equal(got, _lib.interpolate(x_d, size=size, mode="bilinear"))


# ---------------------------------------------------------------------------------------------------------------- the recipe
GT_SHAPE = (256, 272)


def _gt(n=1):
    """natural 64 x 64 images enlarged to 256 x 272: float32 [n,3,256,272] in [0,1]"""
    x = torch.from_numpy(D.natural_images(H.ROOT)[:n])
    return torch.nn.functional.interpolate(x, size=GT_SHAPE, mode="bicubic", align_corners=False).clamp(0, 1).contiguous()


def _plans():
    from resshift_amd.degrade import face_plan

    return {"sf1": face_plan(*GT_SHAPE, sf=1.0, sig_x=4.5, sig_y=9.0, theta=0.6, nf=6.0, qf=55.7, noise_seed=201),
            "sf31.9": face_plan(*GT_SHAPE, sf=31.9, sig_x=12.0, sig_y=5.0, theta=2.2, nf=15.0, qf=30.2, noise_seed=202)}


@pytest.mark.parametrize("name", ["sf1", "sf31.9"])
def test_every_stage_of_a_face_plan_against_the_restatements(gpu, name):
    """teacher forcing: every operator call is checked against the restatement fed that call's DEVICE input; the JPEG stage is exact"""
    import ctypes as C

    from resshift_amd import _lib
    from resshift_amd.degrade import Degrader, FacePlan

    plan = _plans()[name]
    assert FacePlan.from_json(plan.to_json()) == plan
    assert plan.small == {"sf1": GT_SHAPE, "sf31.9": (8, 8)}[name] and plan.quality == {"sf1": 55, "sf31.9": 30}[name]
    gt = _gt()
    lq, log = Degrader(gpu).run_face(gt.to(gpu), plan, trace=True)
    assert [s[0] for s in log] == plan.stages() == ["blur_down", "noise", "jpeg", "up", "round"]
    assert torch.equal(log[0][1].cpu(), gt)
    for (stage, x_d, y_d), nxt in zip(log, log[1:] + [None]):
        assert nxt is None or nxt[1] is y_d
        x = x_d.cpu().numpy()
        if stage == "noise":
            n = torch.empty((1, *x_d.shape[1:]), device=gpu, dtype=torch.float32)
            _lib.check(_lib.load().rs_noise_fill(_lib.noise_keys([(plan.noise_seed, 0)]), (C.c_int * 1)(0), n.data_ptr(), n.numel(), 1,
                                                 _lib.current_stream_ptr()), "rs_noise_fill")
            want = F.stage(plan, stage, x, [n[0].cpu().numpy()])
            err = float(np.abs(y_d.cpu().double().numpy() - want).max())
            assert err <= 1e-6 and float(y_d.min()) >= 0.0 and float(y_d.max()) <= 1.0, err
            continue
        want = F.stage(plan, stage, x)
        if stage == "jpeg":
            assert tuple(y_d.shape) == (1, 3, *plan.small) and np.array_equal(y_d.cpu().numpy(), want)
        elif stage == "round":
            assert y_d.dtype == torch.uint8 and np.array_equal(y_d.cpu().numpy(), want)
            assert torch.equal(lq, y_d.permute(0, 3, 1, 2).float() / 255.0) and tuple(lq.shape) == (1, 3, *GT_SHAPE)
        else:
            err = float(np.abs(y_d.cpu().double().numpy() - want).max())
            print(f"{name} {stage} {tuple(x.shape[2:])} -> {tuple(want.shape[2:])}: {err:.3e} (bound {F.TOL:.1e})")
            assert tuple(y_d.shape) == want.shape and err <= F.TOL, (stage, err)


def _gt_folder(path, sides=((256, 272), (272, 256), (256, 256))):
    from PIL import Image

    path.mkdir()
    x = (_gt(3) * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).numpy()
    sizes = {}
    for i, (stem, (h, w)) in enumerate(zip("abc", sides)):
        Image.fromarray(np.ascontiguousarray(x[i].transpose(1, 0, 2) if (h, w) == (272, 256) else x[i, :h, :w])).save(path / f"{stem}.png")
        sizes[stem] = (h, w)
    return sizes


def test_make_face_testset(gpu, tmp_path):
    from PIL import Image

    from resshift_amd import degrade
    from resshift_amd.continuous import request_seed

    sizes = _gt_folder(tmp_path / "gt")
    plans = degrade.make_face_testset(tmp_path / "gt", tmp_path / "lq", device=gpu)
    assert sorted(plans) == ["a", "b", "c"] and sorted(p.name for p in (tmp_path / "lq").iterdir()) == ["a.png", "b.png", "c.png", "plans.json"]
    recorded = json.load(open(tmp_path / "lq" / "plans.json"))
    for i, (stem, (h, w)) in enumerate(sizes.items()):
        im = np.asarray(Image.open(tmp_path / "lq" / f"{stem}.png"))
        assert im.shape == (h, w, 3) and im.dtype == np.uint8 and im.std() > 1
        p = plans[stem]
        assert degrade.FacePlan.from_dict(recorded[stem]) == p == degrade.draw_face_plan(degrade.FACE_TESTING, h, w, request_seed(10000, i))
        gt = torch.from_numpy(np.asarray(Image.open(tmp_path / "gt" / f"{stem}.png")).copy()).unsqueeze(0).to(gpu)
        assert np.array_equal(degrade.Degrader(gpu).run_face_u8(gt, p)[0].cpu().numpy(), im)
    degrade.make_face_testset(tmp_path / "gt", tmp_path / "again", device=gpu)
    degrade.make_face_testset(tmp_path / "gt", tmp_path / "other", seed=10001, device=gpu)
    for stem in sizes:
        same = (tmp_path / "lq" / f"{stem}.png").read_bytes()
        assert (tmp_path / "again" / f"{stem}.png").read_bytes() == same
        assert (tmp_path / "other" / f"{stem}.png").read_bytes() != same
    assert (tmp_path / "again" / "plans.json").read_bytes() == (tmp_path / "lq" / "plans.json").read_bytes()
    Image.fromarray(np.zeros((200, 300, 3), np.uint8)).save(tmp_path / "gt" / "d.png")
    with pytest.raises(ValueError, match=r"d\.png: 200 x 300 has a side below 256"):
        degrade.make_face_testset(tmp_path / "gt", tmp_path / "bad", device=gpu)
    assert not (tmp_path / "bad").exists()


def test_make_lq_and_the_command_line_and_the_metrics(gpu, tmp_path):
    """GT folder -> make_lq(opts=FACE_TESTING) / the command line -> Engine.metrics of the LQ against the GT: finite scores; PSNR falls as
    sf rises across the two hand-written plans"""
    from PIL import Image

    from resshift_amd import ResShiftSampler, degrade
    from resshift_amd.config import ConfigNode

    up, ap, dp, _ = H.CASES["tiny"]
    usd, asd = H.weights(up, ap)
    cfg = ConfigNode(model=ConfigNode(target="models.unet.UNetModelSwin", ckpt_path=None, params=up),
                     diffusion=ConfigNode(target="models.script_util.create_gaussian_diffusion", params=dp),
                     autoencoder=ConfigNode(target="ldm.models.autoencoder.VQModelTorch", ckpt_path=None, params=ap))
    s = ResShiftSampler(cfg, sf=dp["sf"], seed=10000, precision="parity", state_dicts={"model": usd, "autoencoder": asd})
    sizes = _gt_folder(tmp_path / "gt")
    plans = s.make_lq(tmp_path / "gt", tmp_path / "lq", opts=degrade.FACE_TESTING)
    assert sorted(plans) == sorted(sizes) and all(isinstance(p, degrade.FacePlan) for p in plans.values())
    degrade.main([str(tmp_path / "gt"), str(tmp_path / "cli"), "--recipe", "face", "--seed", "10000"])
    for name in [f"{stem}.png" for stem in sizes] + ["plans.json"]:
        assert (tmp_path / "cli" / name).read_bytes() == (tmp_path / "lq" / name).read_bytes()
    load = lambda p: torch.from_numpy(np.asarray(Image.open(p).convert("RGB")).copy()).unsqueeze(0).to(gpu)
    for stem in sizes:
        m = s.engine.metrics(load(tmp_path / "lq" / f"{stem}.png"), load(tmp_path / "gt" / f"{stem}.png"))
        psnr, ssim = float(m["psnr"][0]), float(m["ssim"][0])
        print(f"face LQ {stem} (sf = {plans[stem].sf:.2f}, q = {plans[stem].quality}): PSNR {psnr:.2f} dB, SSIM {ssim:.4f}")
        assert np.isfinite(psnr) and np.isfinite(ssim) and 5.0 < psnr < 60.0 and ssim <= 1.0
    gt = _gt().to(gpu)
    gt_u8 = s.engine.unit_to_u8(gt)
    scores = {}
    for name, plan in _plans().items():
        lq_u8 = degrade.Degrader(s.engine).run_face_u8(gt_u8, plan)
        scores[name] = float(s.engine.metrics(lq_u8, gt_u8)["psnr"][0])
    print(f"PSNR of the two hand-written plans: {scores}")
    assert np.isfinite(scores["sf1"]) and np.isfinite(scores["sf31.9"]) and scores["sf31.9"] < scores["sf1"]

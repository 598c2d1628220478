"""The degradation operators on the GPU (tiny shapes, the file prints its wall time).  The reference is the float64
restatement tests/_degrade_ref.py; the bounds R.TOL are five times the distance of the reference's own fp32 outputs from it, which
tests/test_degrade_cpu.py measures and pins (filter 5e-6, interpolate 1.5e-5, JPEG 2.5e-6 - absolute, on every element).

  * filter2d, interpolate: every case against the restatement; a delta kernel and scale 1 are the identity, bit for bit;
  * jpeg: constructed inputs whose expected output is known in closed form (every element within the bound), an exact tie, natural
    inputs with and without padding (an MCU beyond the bound must hold a coefficient within 1e-3 of a rounding tie, at most 5 % may);
  * add_noise against torch on noise_fill's normals to 2 ulp, unit_to_u8 exactly;
  * three hand-written plans, every stage teacher-forced against the restatement; make_testset; the loop closed by inference(gt_path=);
  * B = 1 calls against the batch, bit for bit, for every kernel.
"""
import ctypes as C
import json
import time

import numpy as np
import pytest
import torch

import helpers as H
import _degrade_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    yield
    print(f"\ntests/test_degrade_gpu.py: {time.time() - _T0:.1f} s wall time")


def _dev(x, gpu):
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


def _err(got, want):
    return float(np.abs(got.cpu().double().numpy() - want).max())


def _noise_fill(gpu, keys, draws, shape):
    """rs_noise_fill: the normals of (keys[b], draws[b]) for an image of `shape`"""
    from resshift_amd import _lib

    out = torch.empty((len(keys), *shape), device=gpu, dtype=torch.float32)
    dr = (C.c_int * len(keys))(*draws)
    _lib.check(_lib.load().rs_noise_fill(_lib.noise_keys(keys), dr, out.data_ptr(), int(np.prod(shape)), len(keys), _lib.current_stream_ptr()), "rs_noise_fill")
    return out


# ---------------------------------------------------------------------------------------------------------------- filter2d
@pytest.mark.parametrize("case", R.GPU_FILTER_CASES, ids=[c[0] for c in R.GPU_FILTER_CASES])
def test_filter2d_against_the_float64_restatement(gpu, case):
    from resshift_amd import _lib

    x, kernels = R.filter_case(case)
    x_d, k_d = _dev(x, gpu), _dev(kernels, gpu)
    want = R.filter2d(x, kernels)
    got = _lib.filter2d(x_d, k_d)
    assert got.data_ptr() != x_d.data_ptr() and torch.equal(x_d.cpu(), torch.from_numpy(x)) and torch.equal(k_d.cpu(), torch.from_numpy(kernels))
    assert tuple(got.shape) == x.shape and got.dtype == torch.float32
    err = _err(got, want)
    clamped = _lib.filter2d(x_d, k_d, clamp=True)
    print(f"filter2d {case[0]} (k = {kernels.shape[-1]}): max |device - float64 restatement| = {err:.3e} (bound {R.TOL['filter']:.1e}); range "
          f"[{want.min():.3f}, {want.max():.3f}]")
    assert err <= R.TOL["filter"], err
    assert torch.equal(clamped, got.clamp(0, 1))
    for b in range(2):   # an image does not depend on its batch
        kb = k_d if k_d.shape[0] == 1 else k_d[b:b + 1].clone()
        assert torch.equal(_lib.filter2d(x_d[b:b + 1].clone(), kb)[0], got[b]), (case[0], b)


@pytest.mark.parametrize("k", [3, 13, 21])
def test_a_delta_kernel_is_the_identity(gpu, k):
    from resshift_amd import _lib

    x_d = _dev(R.inputs((2, 3, 24, 72), 5), gpu)
    delta = torch.zeros(2, k, k, device=gpu)
    delta[:, k // 2, k // 2] = 1.0
    assert torch.equal(_lib.filter2d(x_d, delta), x_d) and torch.equal(_lib.filter2d(x_d, delta[:1].contiguous()), x_d)


# ---------------------------------------------------------------------------------------------------------------- interpolate
@pytest.mark.parametrize("case", R.INTERP_CASES, ids=str)
def test_interpolate_against_float64(gpu, case):
    from resshift_amd import _lib

    mode, kind, v = case
    x = R.inputs((2, 3, *R.INTERP_SHAPE), R.INTERP_SEED)
    x_d = _dev(x, gpu)
    want = R.interpolate(x, mode=mode, **{kind: v})
    got = _lib.interpolate(x_d, mode=mode, **{kind: v})
    assert torch.equal(x_d.cpu(), torch.from_numpy(x)) and tuple(got.shape) == want.shape
    err = _err(got, want)
    print(f"interpolate {case}: {R.INTERP_SHAPE} -> {tuple(got.shape[2:])}, max |device - float64 F.interpolate| = {err:.3e} (bound {R.TOL['interp']:.1e})")
    assert err <= R.TOL["interp"], err
    assert torch.equal(_lib.interpolate(x_d, mode=mode, clamp=True, **{kind: v}), got.clamp(0, 1))
    for b in range(2):
        assert torch.equal(_lib.interpolate(x_d[b:b + 1].clone(), mode=mode, **{kind: v})[0], got[b]), (case, b)


@pytest.mark.parametrize("mode", ["bilinear", "area", "bicubic"])
def test_scale_one_is_the_identity(gpu, mode):
    from resshift_amd import _lib

    x_d = _dev(R.inputs((2, 3, *R.INTERP_SHAPE), R.INTERP_SEED), gpu)
    assert torch.equal(_lib.interpolate(x_d, scale_factor=1, mode=mode), x_d)      # the weights are exactly 0 and 1
    assert torch.equal(_lib.interpolate(x_d, size=R.INTERP_SHAPE, mode=mode), x_d)


# ---------------------------------------------------------------------------------------------------------------- jpeg
@pytest.mark.parametrize("case", R.JPEG_CASES, ids=[c[0] for c in R.JPEG_CASES])
def test_jpeg_on_constructed_inputs(gpu, case):
    """every pre-round coefficient sits 0.1 from a rounding tie, the expected output is the decode of the chosen integers: every element
    within the bound, no exclusions"""
    from resshift_amd import _lib

    key, (Hh, W), qualities, seed = case
    x, want, tie = R.constructed_jpeg_case(Hh, W, qualities, seed)
    x_d = _dev(x, gpu)
    got = _lib.jpeg(x_d, qualities)
    assert got.data_ptr() != x_d.data_ptr() and torch.equal(x_d.cpu(), torch.from_numpy(x))
    err = _err(got, want)
    print(f"jpeg {key} {qualities}: max |device - closed form| = {err:.3e} (bound {R.TOL['jpeg']:.1e}), smallest tie distance {tie:.4f}")
    assert tie >= 0.0999 and err <= R.TOL["jpeg"], err
    for b in range(2):
        assert torch.equal(_lib.jpeg(x_d[b:b + 1].clone(), [qualities[b]])[0], got[b]), (key, b)


def test_jpeg_rounds_an_exact_tie_to_even(gpu):
    from resshift_amd import _lib

    t = R.tie_image()
    want, coefs = R.jpeg(t, [R.TIE_QUALITY] * 2, return_coefficients=True)
    assert coefs[0][1][0, 0, 0, 0] == 22.5
    err = _err(_lib.jpeg(_dev(t, gpu), R.TIE_QUALITY), want)
    away = float(np.abs(R.jpeg(t, [R.TIE_QUALITY] * 2, half_away=True) - want).max())
    print(f"jpeg tie image: max |device - restatement| = {err:.3e}; rounding half away would move {away:.3e}")
    assert err <= R.TOL["jpeg"] < away


def _check_natural_jpeg(got, x, qualities, label):
    """the criterion for inputs whose coefficients fall where they fall: returns (MCUs beyond the bound, MCUs)"""
    want, coefs = R.jpeg(x, qualities, return_coefficients=True)
    d = np.abs(got.cpu().double().numpy() - want)
    Hh, W = x.shape[2:]
    Hp, Wp = -(-Hh // 16) * 16, -(-W // 16) * 16
    d = np.pad(d, ((0, 0), (0, 0), (0, Hp - Hh), (0, Wp - W)))
    worst = d.reshape(len(x), 3, Hp // 16, 16, Wp // 16, 16).max(axis=(1, 3, 5))          # [B, mcu rows, mcu columns]
    beyond, unexplained = 0, []
    for b in range(len(x)):
        tie = R.mcu_tie_distance(coefs[b])
        over = worst[b] > R.TOL["jpeg"]
        beyond += int(over.sum())
        unexplained += [(b, int(i), int(j), float(worst[b, i, j]), float(tie[i, j])) for i, j in zip(*np.nonzero(over & (tie > R.TIE_DELTA)))]
    inside = float(worst[worst <= R.TOL["jpeg"]].max()) if (worst <= R.TOL["jpeg"]).any() else float("nan")
    print(f"jpeg {label}: {beyond} of {worst.size} MCUs beyond the bound, the others within {inside:.3e} (bound {R.TOL['jpeg']:.1e})")
    assert not unexplained, f"MCUs beyond the bound without a coefficient within {R.TIE_DELTA} of a tie: {unexplained[:5]}"
    return beyond, worst.size


@pytest.mark.parametrize("crop", [None, (40, 56)], ids=["64x64", "40x56_padded"])
@pytest.mark.parametrize("quality", [30.0, 70.0, 95.0])
def test_jpeg_on_natural_inputs(gpu, quality, crop):
    from resshift_amd import _lib

    x = R.natural_images(H.ROOT, crop=crop)
    got = _lib.jpeg(_dev(x, gpu), quality)
    assert tuple(got.shape) == x.shape
    beyond, n = _check_natural_jpeg(got, x, [quality] * len(x), f"natural {x.shape[2]} x {x.shape[3]} at quality {quality:g}")
    assert n == 8 * 16 if crop is None else n == 8 * 12
    assert beyond <= 0.05 * n, (beyond, n)


# ---------------------------------------------------------------------------------------------------------------- add_noise, unit_to_u8
@pytest.mark.parametrize("clamp", [True, False])
def test_add_noise_against_torch_on_the_normals(gpu, clamp):
    """colour and gray images in one batch: x + sigma / 255 * n with the normals rs_noise_fill writes for (C, H, W) resp. (1, H, W), to 2
    ulp of the result (the kernel rounds the product and the sum separately, as torch does); equal keys give equal bits whatever the batch position"""
    from resshift_amd import _lib

    Hh, W = 19, 23                                               # 3 * 19 * 23 and 19 * 23 are no multiples of 4
    x_d = _dev(R.inputs((4, 3, Hh, W), 7), gpu)
    keys, draws = [(11, 0), (12, 0), (2 ** 63 + 5, 0), (12, 0)], [0, 1, 0, 1]
    sigma, gray = [15.0, 3.5, 8.0, 3.5], [False, True, True, False]
    got = _lib.add_noise(x_d, keys, sigma, gray=gray, draw=draws, clamp=clamp)
    n_color, n_gray = _noise_fill(gpu, keys, draws, (3, Hh, W)), _noise_fill(gpu, keys, draws, (1, Hh, W))
    worst = 0.0
    for b in range(4):
        n = n_gray[b] if gray[b] else n_color[b]
        want = x_d[b] + torch.tensor(sigma[b] / 255.0, dtype=torch.float32, device=gpu) * n
        ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126, device=gpu)).log2().floor().exp2() * 2.0 ** -23
        if clamp:
            want = want.clamp(0, 1)
        worst = max(worst, float(((got[b] - want).abs() / ulp).max()))
        assert torch.all((got[b] - want).abs() <= 2 * ulp), b
    print(f"add_noise clamp={clamp}: at most {worst:.2f} ulp from torch's x + c * n; range [{float(got.min()):.3f}, {float(got.max()):.3f}]")
    assert (float(got.min()) >= 0.0 and float(got.max()) <= 1.0) == clamp
    assert torch.equal(n_gray[1, 0], n_color[1, 0])              # (the gray normals are the first H * W of the colour ones)
    # batch position and batch size do not matter
    for b in range(4):
        alone = _lib.add_noise(x_d[b:b + 1].clone(), [keys[b]], [sigma[b]], gray=[gray[b]], draw=[draws[b]], clamp=clamp)
        assert torch.equal(alone[0], got[b]), b
    perm = [2, 0, 3, 1]
    shuffled = _lib.add_noise(x_d[perm].contiguous(), [keys[i] for i in perm], [sigma[i] for i in perm], gray=[gray[i] for i in perm],
                              draw=[draws[i] for i in perm], clamp=clamp)
    assert torch.equal(shuffled, got[perm])
    assert torch.equal(_lib.add_noise(x_d, keys, 0.0, clamp=False), x_d)


def test_unit_to_u8_is_exact(gpu):
    from resshift_amd import _lib

    v = np.arange(0, 255, dtype=np.float32)
    ties = ((v + np.float32(0.5)) / np.float32(255.0)).astype(np.float32)
    ties = ties[(ties * np.float32(255.0)) % 1 == 0.5]                       # float32 products that are exact ties
    rnd = R.inputs((2, 3, 9, 11), 9).ravel() * np.float32(1.2) - np.float32(0.1)     # and values on both sides of [0, 1]
    flat = np.concatenate([ties, rnd, np.float32([0.0, 1.0, -0.0, 2.0, -3.0, 0.5, 1e-9])])
    flat = np.resize(flat, 2 * 3 * 13 * 17).astype(np.float32)
    x = flat.reshape(2, 3, 13, 17)
    got = _lib.unit_to_u8(_dev(x, gpu))
    want = R.unit_to_u8(x)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 13, 17, 3) and len(ties) > 20
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(_lib.unit_to_u8(_dev(x[1:], gpu))[0], got[1])


# ---------------------------------------------------------------------------------------------------------------- the pipeline
def _plans():
    from resshift_amd.degrade import DegradePlan, KernelSpec, StagePlan

    K = KernelSpec
    pulse = K("pulse", 7, 7)
    a = DegradePlan(B=2, H=64, W=48, sf=4, seed=1,
                    first=StagePlan(kernels=(K("aniso", 11, 13, sig_x=0.7, sig_y=1.6, theta=0.5), K("sinc", 9, 13, cutoff=1.4)), scale=1.3, mode="bicubic",
                                    sigma=(12.0, 4.0), gray=(False, True)),
                    jpeg1=(75.0, 90.0), second=None, sinc_first=True, final_mode="area", final_kernels=(K("sinc", 5, 7, cutoff=2.2), pulse),
                    jpeg2=(85.0, 94.0), noise_seeds=(101, 102))
    b = DegradePlan(B=2, H=64, W=48, sf=4, seed=2,
                    first=StagePlan(kernels=(K("iso", 7, 13, sig_x=0.6, sig_y=0.6), K("generalized_iso", 5, 13, sig_x=0.8, sig_y=0.8, beta=1.3)), scale=0.6,
                                    mode="bilinear", sigma=(2.0, 14.0), gray=(True, False)),
                    jpeg1=(93.0, 71.0),
                    second=StagePlan(kernels=(K("aniso", 5, 7, sig_x=0.3, sig_y=0.5, theta=-1.0), K("iso", 3, 7, sig_x=0.4, sig_y=0.4)), scale=1.1, mode="bicubic",
                                     sigma=(9.0, 1.5), gray=(False, False)),
                    sinc_first=False, final_mode="bilinear", final_kernels=(pulse, K("sinc", 3, 7, cutoff=1.9)), jpeg2=(81.0, 92.0), noise_seeds=(103, 2 ** 62))
    c = DegradePlan(B=2, H=64, W=48, sf=4, seed=3,
                    first=StagePlan(kernels=(K("plateau_aniso", 9, 13, sig_x=0.8, sig_y=0.4, theta=2.0, beta=1.1), K("iso", 3, 13, sig_x=0.3, sig_y=0.3)), scale=1.0,
                                    mode="area", sigma=(6.0, 6.0), gray=(True, True)),
                    jpeg1=(80.0, 80.0), second=StagePlan(kernels=None, scale=0.85, mode="area", sigma=(5.0, 10.0), gray=(True, False)),
                    sinc_first=True, final_mode="bicubic", final_kernels=(K("sinc", 5, 7, cutoff=1.2), K("sinc", 3, 7, cutoff=3.0)), jpeg2=(88.0, 95.0),
                    noise_seeds=(104, 105))
    return {"up_sinc_then_jpeg": a, "down_second_blur_jpeg_then_sinc": b, "keep_second_no_blur": c}


_MCUS = {"beyond": 0, "all": 0}


@pytest.mark.parametrize("name", ["up_sinc_then_jpeg", "down_second_blur_jpeg_then_sinc", "keep_second_no_blur"])
def test_every_stage_of_a_plan_against_the_restatement(gpu, name):
    """teacher forcing: every operator call is checked against the restatement fed that call's DEVICE input, with the operator's own criterion"""
    from resshift_amd.degrade import Degrader, DegradePlan

    plan = _plans()[name]
    assert DegradePlan.from_json(plan.to_json()) == plan
    gt = R.natural_images(H.ROOT, crop=(64, 48))[2:4]
    lq, log = Degrader(gpu).run(_dev(gt, gpu), plan, trace=True)
    assert [s[0] for s in log] == plan.stages()
    assert ("blur2" in plan.stages()) == (name == "down_second_blur_jpeg_then_sinc") and ("resize2" in plan.stages()) == (plan.second is not None)
    assert torch.equal(log[0][1].cpu(), torch.from_numpy(gt))
    for (stage, x_d, y_d), nxt in zip(log, log[1:] + [None]):
        assert nxt is None or nxt[1] is y_d                                       # a stage's input is its predecessor's output
        x = x_d.cpu().numpy()
        if stage.startswith("noise"):
            st, draw = (plan.first, 0) if stage == "noise1" else (plan.second, 1)
            keys = [(s, 0) for s in plan.noise_seeds]
            nc, ng = _noise_fill(gpu, keys, [draw] * 2, tuple(x_d.shape[1:])), _noise_fill(gpu, keys, [draw] * 2, (1, *x_d.shape[2:]))
            for b in range(2):
                want = (x_d[b] + torch.tensor(st.sigma[b] / 255.0, dtype=torch.float32, device=gpu) * (ng[b] if st.gray[b] else nc[b]))
                ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126, device=gpu)).log2().floor().exp2() * 2.0 ** -23
                assert torch.all((y_d[b] - want.clamp(0, 1)).abs() <= 2 * ulp), (stage, b)
            want64 = R.stage(plan, stage, x, [(ng[b] if st.gray[b] else nc[b]).cpu().numpy() for b in range(2)])
            assert _err(y_d, want64) <= 1e-6 and float(y_d.min()) >= 0.0 and float(y_d.max()) <= 1.0
            continue
        want = R.stage(plan, stage, x)
        if stage == "round":
            assert y_d.dtype == torch.uint8 and np.array_equal(y_d.cpu().numpy(), want)
            assert torch.equal(lq, y_d.permute(0, 3, 1, 2).float() / 255.0) and tuple(lq.shape) == (2, 3, 16, 12)
        elif stage.startswith("jpeg"):
            assert float(x_d.min()) >= 0.0 and float(x_d.max()) <= 1.0            # whatever precedes a JPEG was clamped
            beyond, n = _check_natural_jpeg(y_d, x, plan.jpeg1 if stage == "jpeg1" else plan.jpeg2, f"{name} {stage} {tuple(x.shape[2:])}")
            _MCUS["beyond"] += beyond
            _MCUS["all"] += n
        else:
            op = "interp" if stage.startswith("resize") else "filter"
            err = _err(y_d, want)
            print(f"{name} {stage} {tuple(x.shape[2:])} -> {tuple(want.shape[2:])}: {err:.3e} (bound {R.TOL[op]:.1e})")
            assert tuple(y_d.shape) == want.shape and err <= R.TOL[op], (stage, err)
    # a plan is a function of its batch's images one by one
    alone = Degrader(gpu).run(_dev(gt[1:], gpu), _one_image(plan, 1))
    assert torch.equal(alone[0], lq[1])


def _one_image(plan, b):
    import dataclasses

    pick = lambda t: None if t is None else (t[b],)
    stage = lambda s: None if s is None else dataclasses.replace(s, kernels=pick(s.kernels), sigma=pick(s.sigma), gray=pick(s.gray))
    return dataclasses.replace(plan, B=1, first=stage(plan.first), second=stage(plan.second), jpeg1=pick(plan.jpeg1), jpeg2=pick(plan.jpeg2),
                               final_kernels=pick(plan.final_kernels), noise_seeds=pick(plan.noise_seeds))


def test_few_mcus_of_the_pipelines_lie_beyond_the_bound():
    """the 5 % rule over the JPEG stages of the three plans together (a stage at 16 x 12 has two MCUs)"""
    if _MCUS["all"] == 0:   # (run alone: do the three plans now)
        dev = torch.device("cuda:0")
        for name in _plans():
            test_every_stage_of_a_plan_against_the_restatement(dev, name)
    print(f"{_MCUS['beyond']} of {_MCUS['all']} MCUs of the pipelines' JPEG stages beyond the bound")
    assert _MCUS["all"] >= 60 and _MCUS["beyond"] <= 0.05 * _MCUS["all"]


# ---------------------------------------------------------------------------------------------------------------- files
def _gt_folder(path):
    from PIL import Image

    path.mkdir()
    u8 = np.load(H.ROOT + "/tests/golden/val_sr_lq.npz")["lq"]
    sizes = {"a": (64, 48), "b": (48, 64), "c": (64, 64)}
    for i, (stem, (h, w)) in enumerate(sizes.items()):
        Image.fromarray(u8[i, :h, :w]).save(path / f"{stem}.png")
    return sizes


def test_make_testset(gpu, tmp_path):
    from PIL import Image

    from resshift_amd import degrade
    from resshift_amd.continuous import request_seed

    sizes = _gt_folder(tmp_path / "gt")
    plans = degrade.make_testset(tmp_path / "gt", tmp_path / "lq", device=gpu)
    assert sorted(plans) == ["a", "b", "c"] and sorted(p.name for p in (tmp_path / "lq").iterdir()) == ["a.png", "b.png", "c.png", "plans.json"]
    recorded = json.load(open(tmp_path / "lq" / "plans.json"))
    for i, (stem, (h, w)) in enumerate(sizes.items()):
        im = np.asarray(Image.open(tmp_path / "lq" / f"{stem}.png"))
        assert im.shape == (h // 4, w // 4, 3) and im.dtype == np.uint8 and im.std() > 1
        p = plans[stem]
        assert degrade.DegradePlan.from_dict(recorded[stem]) == p == degrade.draw_plan(degrade.REALESRGAN_TESTING, 1, h, w, request_seed(10000, i))
        assert (p.B, p.H, p.W, p.sf, p.seed) == (1, h, w, 4, request_seed(10000, i))
        # the PNG is the plan executed on the file
        gt = torch.from_numpy(np.asarray(Image.open(tmp_path / "gt" / f"{stem}.png")).copy()).unsqueeze(0).to(gpu)
        assert np.array_equal(degrade.Degrader(gpu).run_u8(gt, p)[0].cpu().numpy(), im)
    degrade.make_testset(tmp_path / "gt", tmp_path / "again", device=gpu)
    degrade.make_testset(tmp_path / "gt", tmp_path / "other", seed=10001, device=gpu)
    for stem in sizes:
        same = (tmp_path / "lq" / f"{stem}.png").read_bytes()
        assert (tmp_path / "again" / f"{stem}.png").read_bytes() == same
        assert (tmp_path / "other" / f"{stem}.png").read_bytes() != same
    assert (tmp_path / "again" / "plans.json").read_bytes() == (tmp_path / "lq" / "plans.json").read_bytes()
    Image.fromarray(np.zeros((30, 48, 3), np.uint8)).save(tmp_path / "gt" / "d.png")
    with pytest.raises(ValueError, match=r"d\.png: 30 x 48 is no multiple of sf = 4"):
        degrade.make_testset(tmp_path / "gt", tmp_path / "bad", device=gpu)
    assert not (tmp_path / "bad").exists()


def test_the_loop_closes_through_inference(gpu, tmp_path):
    """GT folder -> make_lq -> inference(lq, out, gt_path=gt) on the tiny parity-policy sampler; the command line writes the same files"""
    from resshift_amd import ResShiftSampler, degrade
    from resshift_amd.config import ConfigNode

    up, ap, dp, _ = H.CASES["tiny"]
    usd, asd = H.weights(up, ap)
    cfg = ConfigNode(model=ConfigNode(target="models.unet.UNetModelSwin", ckpt_path=None, params=up),
                     diffusion=ConfigNode(target="models.script_util.create_gaussian_diffusion", params=dp),
                     autoencoder=ConfigNode(target="ldm.models.autoencoder.VQModelTorch", ckpt_path=None, params=ap))
    s = ResShiftSampler(cfg, sf=dp["sf"], seed=10000, precision="parity", state_dicts={"model": usd, "autoencoder": asd})
    s.chop_size, s.chop_stride, s.chop_bs, s.padding_offset = 16, 12, 2, 16
    sizes = _gt_folder(tmp_path / "gt")
    plans = s.make_lq(tmp_path / "gt", tmp_path / "lq")
    assert sorted(plans) == sorted(sizes) and (tmp_path / "lq" / "plans.json").is_file()
    degrade.main([str(tmp_path / "gt"), str(tmp_path / "cli"), "--sf", "4", "--seed", "10000"])
    for stem in sizes:
        assert (tmp_path / "cli" / f"{stem}.png").read_bytes() == (tmp_path / "lq" / f"{stem}.png").read_bytes()
    assert (tmp_path / "cli" / "plans.json").read_bytes() == (tmp_path / "lq" / "plans.json").read_bytes()
    (tmp_path / "lq" / "plans.json").unlink()                    # (inference lists images only; this keeps the folder to them all the same)
    rows = s.inference(tmp_path / "lq", tmp_path / "out", bs=1, seeded=True, gt_path=tmp_path / "gt")
    assert sorted(rows) == sorted(sizes) and all(np.isfinite(v[0]) and np.isfinite(v[1]) and v[1] <= 1 for v in rows.values())
    assert (tmp_path / "out" / "metrics.csv").is_file() and sorted(p.name for p in (tmp_path / "out").glob("*.png")) == ["a.png", "b.png", "c.png"]

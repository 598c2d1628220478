"""PSNR / SSIM against ground truth on the GPU (tiny shapes, the file prints its wall time).

  * Engine.rgb_to_y on all 2^24 RGB triples equals the integer restatement exactly;
  * Engine.metrics against the recorded outputs of the reference's calculate_psnr / calculate_ssim (tests/golden/reference_metrics.npz):
    SSE exact, PSNR within 1e-10 dB, SSIM within 1e-6 - a hundredth of the fourth decimal that results are quoted to, and what raw fp32
    moments miss (tests/test_metrics_cpu.py);
  * against the numpy restatement tests/_metrics_ref.py with the same bounds on seeded random uint8 images at the shapes where the kernel
    can go wrong.  A workgroup owns 32 x 32 map positions and reads 42 x 42 pixels: one window (11 x 11, 11 x 12, 12 x 11), sides of
    41 / 42 / 43 (one tile to the pixel, and one row or column more), 79 and 81 (two tiles and a bit), odd widths with C = 3 and with
    C = 1, borders 0 / 4 / 5, B = 1 and B = 3, ycbcr on and off;
  * float32 [-1,1] inputs equal the output_to_u8 route bit for bit; identical images give SSE 0, PSNR inf, SSIM exactly 1.0; all-0
    against all-255 at 256 x 256 x 3 gives SSE 12 784 435 200 > 2^32;
  * determinism: the same call twice, and image k alone against image k inside a batch of three, bit for bit;
  * ResShiftSampler.inference(gt_path=...) end to end on the tiny parity-policy sampler of tests/test_colorfix_gpu.py.
"""
import csv
import math
import time

import numpy as np
import pytest
import torch

import helpers as H
import _metrics_ref as M

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TOL_PSNR = 1e-10   # dB: the SSE is the same integer, the formula one float64 expression
TOL_SSIM = 1e-6
_T0 = time.time()
_WORST = {"reference": 0.0, "restatement": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    yield
    print(f"\ntests/test_metrics_gpu.py: {time.time() - _T0:.1f} s wall time; max |ssim - reference| = {_WORST['reference']:.3e}, "
          f"max |ssim - restatement| = {_WORST['restatement']:.3e} (bound {TOL_SSIM:.0e})")


_SAMPLER = []


def _sampler():
    """tests/test_colorfix_gpu.py::_sampler's tiny case under the parity policy (sf = 4), built once"""
    from resshift_amd import ResShiftSampler
    from resshift_amd.config import ConfigNode

    up, ap, dp, _ = H.CASES["tiny"]
    if not _SAMPLER:
        usd, asd = H.weights(up, ap)
        cfg = ConfigNode(model=ConfigNode(target="models.unet.UNetModelSwin", ckpt_path=None, params=up),
                         diffusion=ConfigNode(target="models.script_util.create_gaussian_diffusion", params=dp),
                         autoencoder=ConfigNode(target="ldm.models.autoencoder.VQModelTorch", ckpt_path=None, params=ap))
        _SAMPLER.append(ResShiftSampler(cfg, sf=dp["sf"], seed=1, precision="parity", state_dicts={"model": usd, "autoencoder": asd}))
        assert dp["sf"] == 4
    s = _SAMPLER[0]
    s.chop_size, s.chop_stride, s.chop_bs, s.padding_offset = 16, 12, 9, 16
    return s


@pytest.fixture(scope="module")
def engine(gpu):
    return _sampler().engine


def _check(got, want, what, against="restatement"):
    """a metrics dict against (sse, psnr, ssim) arrays: SSE exact, PSNR 1e-10 dB (inf where the SSE is 0), SSIM 1e-6"""
    sse, psnr, ssim = (np.asarray(v) for v in want)
    assert got["sse"].dtype == torch.int64 and got["psnr"].dtype == got["ssim"].dtype == torch.float64
    assert all(got[k].is_cuda and tuple(got[k].shape) == sse.shape for k in ("sse", "psnr", "ssim"))
    g_sse, g_psnr, g_ssim = got["sse"].cpu().numpy(), got["psnr"].cpu().numpy(), got["ssim"].cpu().numpy()
    finite = np.isfinite(psnr)
    e_psnr = float(np.abs(g_psnr[finite] - psnr[finite]).max()) if finite.any() else 0.0
    e_ssim = float(np.abs(g_ssim - ssim).max())
    _WORST[against] = max(_WORST[against], e_ssim)
    print(f"metrics {what}: |psnr - {against}| = {e_psnr:.2e} dB, |ssim - {against}| = {e_ssim:.2e}")
    assert np.array_equal(g_sse, sse), (what, g_sse, sse)
    assert np.array_equal(np.isinf(g_psnr), ~finite) and (g_psnr[~finite] > 0).all(), what
    assert e_psnr <= TOL_PSNR and e_ssim <= TOL_SSIM, (what, e_psnr, e_ssim)


# ---------------------------------------------------------------------------------------------------------------- Y
def test_rgb_to_y_on_every_triple(gpu, engine):
    t = M.all_triples()
    got = engine.rgb_to_y(torch.from_numpy(t).to(gpu))
    assert tuple(got.shape) == (4096, 4096) and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), M.rgb_to_y(t))
    flat = torch.from_numpy(t.reshape(-1)[:4096]).to(gpu)
    odd = flat[17:17 + 3003].view(1001, 3)                                   # a view at an odd byte offset, an odd count
    assert odd.is_contiguous() and odd.data_ptr() % 2 == 1
    assert np.array_equal(engine.rgb_to_y(odd).cpu().numpy(), M.rgb_to_y(t.reshape(-1)[17:17 + 3003].reshape(1001, 3)))


# ---------------------------------------------------------------------------------------------------------------- the reference
def test_metrics_against_the_recorded_reference(gpu, engine):
    z = M.load_golden(H.ROOT)
    cases = M.golden_cases(z)
    assert len(cases) == 54
    groups = {}
    for key, sr, gt, border, ycbcr in cases:                                 # one call per (shape, parameters): the pairs as a batch
        groups.setdefault((sr.shape, border, ycbcr), []).append((key, sr, gt))
    for (shape, border, ycbcr), rows in groups.items():
        sr = torch.from_numpy(np.stack([r[1] for r in rows])).to(gpu)
        gt = torch.from_numpy(np.stack([r[2] for r in rows])).to(gpu)
        got = engine.metrics(sr, gt, border=border, ycbcr=ycbcr)
        ref_p = np.array([float(z["psnr_" + r[0]]) for r in rows])
        ref_s = np.array([float(z["ssim_" + r[0]]) for r in rows])
        sse = M.batch([r[1] for r in rows], [r[2] for r in rows], border, ycbcr)[0]   # (equal to the reference's: tests/test_metrics_cpu.py)
        _check(got, (sse, ref_p, ref_s), f"fixture {shape} border {border} ycbcr {ycbcr} x {len(rows)}", against="reference")


# ---------------------------------------------------------------------------------------------------------------- the restatement
# (H, W, C, B, border, ycbcr)
SHAPES = [
    (11, 11, 3, 1, 0, True), (11, 12, 3, 1, 0, False), (12, 11, 1, 1, 0, False), (21, 22, 3, 3, 5, True),
    (41, 43, 3, 3, 0, True), (42, 42, 3, 1, 0, False), (43, 41, 1, 3, 0, False), (43, 43, 3, 1, 0, True), (42, 43, 1, 1, 0, False),
    (49, 51, 3, 3, 4, False), (52, 53, 1, 1, 5, False), (51, 50, 3, 1, 4, True),
    (79, 81, 3, 3, 0, False), (81, 79, 1, 1, 4, False), (79, 79, 3, 1, 5, True), (84, 85, 3, 3, 5, True),
]
_INPUTS = {}


def _inputs(case, gpu):
    """seeded uint8 batches of a case - b is a plus noise of a few levels, so that the SSIM is neither 0 nor 1 - and their restatement;
    made once, never modified"""
    if case not in _INPUTS:
        Hh, W, Cc, B, border, ycbcr = case
        rng = np.random.default_rng(1000 * Hh + W + 7 * Cc)
        a = rng.integers(0, 256, (B, Hh, W, Cc), dtype=np.uint8)
        b = np.clip(a.astype(np.int64) + rng.integers(-40, 41, a.shape), 0, 255).astype(np.uint8)
        if B > 1:
            b[-1] = rng.integers(0, 256, a.shape[1:], dtype=np.uint8)       # and one unrelated pair: SSIM near 0
        _INPUTS[case] = (a, b, torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu), M.batch(a, b, border, ycbcr))
    return _INPUTS[case]


@pytest.mark.parametrize("case", SHAPES, ids=str)
def test_metrics_against_the_restatement(gpu, engine, case):
    Hh, W, Cc, B, border, ycbcr = case
    a, b, a_d, b_d, want = _inputs(case, gpu)
    got = engine.metrics(a_d, b_d, border=border, ycbcr=ycbcr)
    assert torch.equal(a_d.cpu(), torch.from_numpy(a)) and torch.equal(b_d.cpu(), torch.from_numpy(b))      # the inputs are only read
    _check(got, want, str(case))
    again = engine.metrics(a_d, b_d, border=border, ycbcr=ycbcr)
    for k in ("sse", "psnr", "ssim"):
        assert torch.equal(got[k], again[k]), (case, k)                      # run to run: equal bits
    for i in range(B):                                                       # an image does not depend on its batch
        alone = engine.metrics(a_d[i:i + 1].clone(), b_d[i:i + 1].clone(), border=border, ycbcr=ycbcr)
        for k in ("sse", "psnr", "ssim"):
            assert torch.equal(alone[k], got[k][i:i + 1]), (case, i, k)


@pytest.mark.parametrize("case", [(43, 45, 3, 3, 0, True), (79, 43, 3, 1, 4, False), (42, 51, 1, 3, 5, False)], ids=str)
def test_float_inputs_equal_the_output_to_u8_route(gpu, engine, case):
    Hh, W, Cc, B, border, ycbcr = case
    g = torch.Generator().manual_seed(Hh * 100 + W)
    sr = (torch.rand(B, Cc, Hh, W, generator=g) * 2.2 - 1.1)                 # some of it beyond [-1, 1]: the clamp has work
    sr[0, 0, 0, :4] = torch.tensor([-1.0, 1.0, 0.0, 1.0 / 255])              # 0 -> 127.5 -> 128: a tie of the rounding
    gt = torch.randint(0, 256, (B, Hh, W, Cc), generator=g, dtype=torch.uint8)
    sr_d, gt_d = sr.to(gpu), gt.to(gpu)
    u8 = engine.output_to_u8(sr_d)
    assert np.array_equal(u8.cpu().numpy(), np.stack([M.quantise(x) for x in sr.numpy()]))
    via_u8 = engine.metrics(u8, gt_d, border=border, ycbcr=ycbcr)
    direct = engine.metrics(sr_d, gt_d, border=border, ycbcr=ycbcr)
    _check(direct, M.batch(u8.cpu().numpy(), gt.numpy(), border, ycbcr), f"float sr {case}")
    gt_f = engine.u8_to_input(gt_d)                                          # a float ground truth quantises back to itself
    assert torch.equal(engine.output_to_u8(gt_f), gt_d)
    for other in (direct, engine.metrics(sr_d, gt_f, border=border, ycbcr=ycbcr), engine.metrics(u8, gt_f, border=border, ycbcr=ycbcr),
                  engine.metrics(sr_d.double(), gt_d, border=border, ycbcr=ycbcr)):
        for k in ("sse", "psnr", "ssim"):
            assert torch.equal(other[k], via_u8[k]), (case, k)
    swapped = engine.metrics(gt_d, sr_d, border=border, ycbcr=ycbcr)         # the float batch as the second input
    assert torch.equal(swapped["sse"], via_u8["sse"])
    assert float((swapped["ssim"] - via_u8["ssim"]).abs().max()) <= 1e-12


def test_identical_images_and_the_largest_error(gpu, engine):
    a, _, a_d, _, _ = _inputs(SHAPES[12], gpu)
    for ycbcr in (True, False):
        got = engine.metrics(a_d, a_d.clone(), border=0, ycbcr=ycbcr)
        assert got["sse"].tolist() == [0, 0, 0]
        assert all(v == math.inf for v in got["psnr"].tolist())
        assert got["ssim"].tolist() == [1.0, 1.0, 1.0]                       # exactly
    zero = torch.zeros(1, 256, 256, 3, dtype=torch.uint8, device=gpu)
    full = torch.full_like(zero, 255)
    got = engine.metrics(zero, full, border=0, ycbcr=False)
    assert got["sse"].tolist() == [12_784_435_200] and 256 * 256 * 3 * 255 ** 2 == 12_784_435_200 > 2 ** 32
    assert got["psnr"].tolist() == [0.0]
    want = M.metrics(np.zeros((256, 256, 3), np.uint8), np.full((256, 256, 3), 255, np.uint8), 0, False)
    assert abs(got["ssim"].item() - want[2]) <= TOL_SSIM and want[0] == 12_784_435_200
    y = engine.metrics(zero, full, border=0, ycbcr=True)                     # Y: 16 against 235
    assert y["sse"].tolist() == [256 * 256 * 219 ** 2]


def test_engine_metrics_accepts_what_the_samplers_hand_it(gpu, engine):
    a, b, a_d, b_d, want = _inputs(SHAPES[9], gpu)
    ref = engine.metrics(a_d, b_d, border=4, ycbcr=False)
    wide = torch.zeros(3, 49, 102, 3, dtype=torch.uint8, device=gpu)
    wide[:, :, ::2] = a_d
    assert not wide[:, :, ::2].is_contiguous()
    got = engine.metrics(wide[:, :, ::2], b_d, border=4, ycbcr=False)       # a strided view
    for k in ("sse", "psnr", "ssim"):
        assert torch.equal(got[k], ref[k])
    with pytest.raises(ValueError, match=r"the cropped image is 9 x 11 \(49 x 51, border 20\)"):
        engine.metrics(a_d, b_d, border=20)
    with pytest.raises(ValueError, match="b is 3 images of 49 x 50 x 3"):
        engine.metrics(a_d, b_d[:, :, :50], ycbcr=False)
    with pytest.raises(ValueError, match="ycbcr=True needs C == 3"):
        engine.metrics(a_d[..., :1], b_d[..., :1])


# ---------------------------------------------------------------------------------------------------------------- end to end
def _read_png(path):
    from PIL import Image

    return np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)


def test_inference_scores_the_pngs_it_writes(gpu, tmp_path):
    """two 32 x 32 files through inference(seeded=True, gt_path=...), with and without the pool: every row is the restatement applied to
    the PNG that was written and the ground-truth file, read back with PIL; the table holds the rows; without gt_path nothing is returned
    or written.  Plain (bs = 2, chop_bs = 9) and pool both run the 18 tiles as one batch, so their PNGs and rows are the same."""
    from PIL import Image

    s = _sampler()
    src, gtd = tmp_path / "in", tmp_path / "gt"
    src.mkdir()
    gtd.mkdir()
    lq = np.load(H.ROOT + "/tests/golden/val_sr_lq.npz")["lq"]
    g = torch.Generator().manual_seed(77)
    for i, name in enumerate(("b", "a")):
        Image.fromarray(lq[i][16:48, 16:48]).save(src / f"{name}.png")
        Image.fromarray(torch.randint(0, 256, (128, 128, 3), generator=g, dtype=torch.uint8).numpy()).save(gtd / f"{name}.png")
    runs = {}
    for tag, pool in (("plain", False), ("pool", True)):
        out = tmp_path / tag
        rows = s.inference(src, out, bs=2, seeded=True, pool=pool, gt_path=gtd, metric_border=4, metric_ycbcr=True)
        assert sorted(rows) == ["a", "b"] and sorted(p.name for p in out.iterdir()) == ["a.png", "b.png", "metrics.csv"]
        for name in rows:
            png = _read_png(out / f"{name}.png")
            assert png.shape == (128, 128, 3)
            sse, psnr, ssim = M.metrics(png, _read_png(gtd / f"{name}.png"), 4, True)
            print(f"inference {tag} {name}: psnr {rows[name][0]:.6f} dB (restatement {psnr:.6f}), ssim {rows[name][1]:.8f} ({ssim:.8f})")
            assert abs(rows[name][0] - psnr) <= TOL_PSNR and abs(rows[name][1] - ssim) <= TOL_SSIM
        with open(out / "metrics.csv") as fh:
            table = list(csv.reader(fh))
        assert table[0] == ["name", "psnr", "ssim"] and [r[0] for r in table[1:]] == ["a", "b", "mean"]
        assert all((float(r[1]), float(r[2])) == rows[r[0]] for r in table[1:3])
        assert float(table[3][1]) == (rows["a"][0] + rows["b"][0]) / 2 and float(table[3][2]) == (rows["a"][1] + rows["b"][1]) / 2
        runs[tag] = rows
    assert runs["pool"] == runs["plain"]
    assert not np.array_equal(_read_png(tmp_path / "plain" / "a.png"), _read_png(tmp_path / "plain" / "b.png"))
    # other parameters reach the kernel
    rows = s.inference(src, tmp_path / "rgb", bs=2, seeded=True, gt_path=gtd, metric_border=0, metric_ycbcr=False)
    want = M.metrics(_read_png(tmp_path / "rgb" / "a.png"), _read_png(gtd / "a.png"), 0, False)
    assert abs(rows["a"][0] - want[1]) <= TOL_PSNR and abs(rows["a"][1] - want[2]) <= TOL_SSIM and rows["a"] != runs["plain"]["a"]
    # without gt_path
    assert s.inference(src, tmp_path / "none", bs=2, seeded=True) is None
    assert sorted(p.name for p in (tmp_path / "none").iterdir()) == ["a.png", "b.png"]
    assert np.array_equal(_read_png(tmp_path / "none" / "a.png"), _read_png(tmp_path / "plain" / "a.png"))
    # a ground truth of another size, a missing one
    Image.fromarray(np.zeros((128, 120, 3), np.uint8)).save(gtd / "b.png")
    with pytest.raises(ValueError, match=r"the ground truth of b.png is 128 x 120, the output is 128 x 128"):
        s.inference(src, tmp_path / "bad", bs=2, seeded=True, gt_path=gtd)
    (gtd / "b.png").unlink()
    with pytest.raises(FileNotFoundError, match="no ground truth for b.png"):
        s.inference(src, tmp_path / "bad", bs=2, seeded=True, gt_path=gtd)

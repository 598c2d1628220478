"""PSNR / SSIM against ground truth without a GPU: the numpy restatement tests/_metrics_ref.py against the recorded
outputs of the reference's calculate_psnr / calculate_ssim (tests/golden/reference_metrics.npz, scripts/make_golden_metrics.py), the
integer Y against the reference's float64 expression on all 2^24 triples, the C ABI's argument errors, and the host plumbing of
`ResShiftSampler.inference(gt_path=...)` on a stubbed engine."""
import csv
import math
import re

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401  (puts the repository root on sys.path)
import _metrics_ref as M
from _fakes import InstantPool, _OnDevice, lib  # noqa: F401  (fixtures)
from resshift_amd import _lib, build
from resshift_amd.sampler import ResShiftSampler


@pytest.fixture(scope="module")
def golden():
    return M.load_golden(H.ROOT)


@pytest.fixture(scope="module")
def triples():
    t = M.all_triples()
    return t, M.is_tie(t)


# ---------------------------------------------------------------------------------------------------------------- the definition
def test_restatement_against_the_recorded_reference(golden):
    """same integer SSE (so one float64 formula gives the PSNR: 1e-10 dB); separable against the reference's outer-product window in
    float64: 1e-12"""
    cases = M.golden_cases(golden)
    assert len(cases) == 12 * 4 + 2 + 4
    worst_p = worst_s = 0.0
    for key, sr, gt, border, ycbcr in cases:
        sse, psnr, ssim = M.metrics(sr, gt, border, ycbcr)
        ref_p, ref_s = float(golden["psnr_" + key]), float(golden["ssim_" + key])
        pa = M.planes(sr, border, ycbcr)
        assert sse > 0 and math.isfinite(ref_p)
        assert sse == round(pa.size * 255.0 ** 2 / 10 ** (ref_p / 10)), key       # the reference's own SSE, recovered from its PSNR
        worst_p, worst_s = max(worst_p, abs(psnr - ref_p)), max(worst_s, abs(ssim - ref_s))
    print(f"restatement against the reference: psnr {worst_p:.2e} dB, ssim {worst_s:.2e}")
    assert worst_p <= 1e-10 and worst_s <= 1e-12
    flat = float(golden["ssim_flat_y1_b0"])
    assert 0.9999 < flat < 1.0                                                    # the cancellation-sensitive case is what it says


def test_no_fixture_pixel_is_a_tie_triple(golden):
    assert golden["gt"].shape == (4, 64, 64, 3)
    seen = 0
    for name, sr, gt, colour in M.golden_pairs(golden):
        for im in (sr, gt):
            assert im.dtype == np.uint8
            if im.shape[2] == 3:
                assert not M.is_tie(im).any(), name
                seen += 1
    assert seen == 2 * 13
    assert {k for k in golden if k.startswith("sr_")} == {"sr_s2", "sr_s10", "sr_s40", "sr_gray", "sr_flat"}
    assert all(golden[k].dtype in (np.uint8, np.float64) for k in golden)         # uint8 images and scalars only


def test_integer_y_differs_from_the_float64_expressions_only_at_the_ties(triples):
    t, tie = triples
    assert int(tie.sum()) == M.N_TIES == 194
    y = M.rgb_to_y(t)
    assert y.min() == 16 and y.max() == 235
    f = t.astype(np.float64)
    coef = np.array([65.481, 128.553, 24.966]) / 255.0
    forms = {"left to right": M.rgb_to_y_float64(t),
             "np.dot 3-D": (np.dot(f, coef) + 16.0).round().astype(np.uint8),
             "np.dot 2-D": (np.dot(f.reshape(-1, 3), coef) + 16.0).round().astype(np.uint8).reshape(4096, 4096)}
    for name, other in forms.items():
        diff = y != other
        print(f"integer Y differs from the float64 {name} form at {int(diff.sum())} triples")
        assert not (diff & ~tie).any(), name
    # away from the ties the exact value is at least 1/255000 from a half: every float64 form rounds it the same way
    num = M.y_numerator(t)
    assert np.abs(2 * (num % M.Y_DEN) - M.Y_DEN)[~tie].min() >= 2


def test_restatement_properties():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (23, 31, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (23, 31, 3), dtype=np.uint8)
    sse, psnr, ssim = M.metrics(a, a, 0, True)
    assert sse == 0 and psnr == math.inf and ssim == 1.0
    s1 = M.metrics(a, b, 3, False)
    assert s1 == M.metrics(a[3:-3, 3:-3], b[3:-3, 3:-3], 0, False)                # the border is a crop
    assert s1[0] == M.metrics(b, a, 3, False)[0] and abs(s1[2] - M.metrics(b, a, 3, False)[2]) < 1e-15
    g = M.window()
    assert g.shape == (11,) and abs(g.sum() - 1) < 1e-15 and np.array_equal(g, g[::-1])
    assert abs(g[5] / g[4] - math.exp(1 / 4.5)) < 1e-15
    # a channel is scored on its own: the colour score is the mean of the three gray scores, the SSE their sum
    per = [M.metrics(a[:, :, c], b[:, :, c], 0, False) for c in range(3)]
    full = M.metrics(a, b, 0, False)
    assert full[0] == sum(p[0] for p in per) and abs(full[2] - np.mean([p[2] for p in per])) < 1e-15
    assert M.metrics(a, b, 0, True)[:3] == M.metrics(M.rgb_to_y(a), M.rgb_to_y(b), 0, False)[:3]
    with pytest.raises(ValueError, match="10 x 31"):
        M.metrics(a[:10], b[:10], 0, False)
    x = np.array([[[-1.0, 1.0, 0.0, 2.0, -3.0, 1.0 / 255]]], dtype=np.float32).repeat(3, 0)
    assert M.quantise(x)[0, :, 0].tolist() == [0, 255, 128, 255, 0, 128]         # 0 is 127.5: to the even neighbour; 128.0 stays


def test_raw_fp32_moments_miss_the_bound_the_gpu_test_sets(golden):
    """why the kernel is fp64: E[x^2] - mu^2 from fp32 moments cancels on the flat pair"""
    g32 = M.window().astype(np.float32)

    def valid32(x):
        wv, hv = x.shape[1] - 10, x.shape[0] - 10
        h = np.zeros((x.shape[0], wv), np.float32)
        for k in range(11):
            h += g32[k] * x[:, k:k + wv]
        v = np.zeros((hv, wv), np.float32)
        for k in range(11):
            v += g32[k] * h[k:k + hv]
        return v

    a = golden["sr_flat"][:, :, 0].astype(np.float32)
    b = golden["gt_flat"][:, :, 0].astype(np.float32)
    mu1, mu2 = valid32(a), valid32(b)
    s1, s2, s12 = valid32(a * a) - mu1 * mu1, valid32(b * b) - mu2 * mu2, valid32(a * b) - mu1 * mu2
    c1, c2 = np.float32(M.C1), np.float32(M.C2)
    m = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))
    err = abs(float(m.astype(np.float64).mean()) - float(golden["ssim_flat_y0_b0"]))
    print(f"raw fp32 moments on the flat pair: |ssim - reference| = {err:.2e}")
    assert err > 1e-6


# ---------------------------------------------------------------------------------------------------------------- C ABI
PTR = 0x100000   # never dereferenced: every call below is refused before anything is launched

ERRORS = {
    "null_a": (dict(a=None), "null tensor"),
    "null_b": (dict(b=None), "null tensor"),
    "null_sse": (dict(sse=None), "null tensor"),
    "null_ssim": (dict(ssim=None), "null tensor"),
    "a_flag": (dict(af=2), "must be 0 or 1"),
    "b_flag": (dict(bf=-1), "must be 0 or 1"),
    "batch": (dict(B=0), "must be positive"),
    "height": (dict(H=0), "must be positive"),
    "width": (dict(W=-4), "must be positive"),
    "channels_two": (dict(C=2), "C must be 1 or 3"),
    "channels_four": (dict(C=4), "C must be 1 or 3"),
    "ycbcr_gray": (dict(C=1, ycbcr=1), "ycbcr needs C == 3"),
    "ycbcr_two": (dict(ycbcr=2), "ycbcr must be 0 or 1"),
    "border_negative": (dict(border=-1), "border must not be negative"),
    "crop_rows": (dict(H=20, border=5), "the cropped image is 10 x 22 (20 x 32, border 5)"),
    "crop_cols": (dict(W=10), "the cropped image is 24 x 10 (24 x 10, border 0)"),
    "crop_negative": (dict(border=40), "the cropped image is -56 x -48"),
    "work_null": (dict(work=None), "workspace is too small: 0 bytes"),
    "work_small": (dict(work_bytes=15), "workspace is too small: 15 bytes, rs_metrics_work_bytes asks for 32"),
    "work_misaligned": (dict(work=PTR * 3 + 4), "aligned to 8 bytes"),
    "out_misaligned": (dict(ssim=PTR * 5 + 2), "aligned to 8 bytes"),
    "float_misaligned": (dict(a=PTR + 2, af=1), "aligned to 4 bytes"),
}


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_metrics_argument_errors(lib, name):
    kw, text = ERRORS[name]
    a = dict(a=PTR, b=PTR * 2, af=0, bf=0, B=2, C=3, H=24, W=32, border=0, ycbcr=1, sse=PTR * 4, ssim=PTR * 5, work=PTR * 3, work_bytes=1 << 20)
    a.update(kw)
    rc = lib.rs_metrics(a["a"], a["b"], a["af"], a["bf"], a["B"], a["C"], a["H"], a["W"], a["border"], a["ycbcr"], a["sse"], a["ssim"], a["work"],
                        a["work_bytes"], None)
    assert rc == -2 and text in _lib.last_error() and _lib.last_error().startswith("rs_metrics: "), (rc, _lib.last_error())


def test_the_workspace_is_one_partial_pair_per_image_channel_and_tile(lib):
    wb = lib.rs_metrics_work_bytes
    assert wb(1, 3, 11, 11, 0, 1) == 16 and wb(1, 3, 11, 11, 0, 0) == 48 and wb(1, 1, 11, 11, 0, 0) == 16
    assert wb(2, 3, 24, 32, 0, 1) == 32
    assert wb(1, 1, 42, 42, 0, 0) == 16 and wb(1, 1, 43, 42, 0, 0) == 32 and wb(1, 1, 43, 43, 0, 0) == 64       # 32 x 32 map positions per tile
    assert wb(1, 1, 51, 50, 4, 0) == 32 and wb(5, 3, 2048, 2048, 0, 0) == 5 * 3 * 64 * 64 * 16
    for bad in ((0, 3, 24, 32, 0, 1), (1, 2, 24, 32, 0, 0), (1, 1, 24, 32, 0, 1), (1, 3, 24, 32, 7, 1), (1, 3, 24, 32, -1, 1)):
        assert wb(*bad) == 0, bad


def test_rgb_to_y_argument_errors(lib):
    for args, text in (((None, PTR, 4), "null tensor"), ((PTR, None, 4), "null tensor"), ((PTR, PTR * 2, 0), "pixels must lie in"),
                       ((PTR, PTR + 11, 4), "overlaps"), ((PTR, PTR, 4), "overlaps")):
        rc = lib.rs_rgb_to_y_u8(*args, None)
        assert rc == -2 and text in _lib.last_error() and _lib.last_error().startswith("rs_rgb_to_y_u8: "), (rc, _lib.last_error())


def test_the_symbols_are_declared_and_the_source_is_built(lib):
    assert "metrics.hip" in build.SOURCES
    header = open(H.ROOT + "/include/resshift_hip.h").read()
    declared = set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", header)) - {"rs_engine"}
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name, n_args in (("rs_metrics_work_bytes", 6), ("rs_metrics", 15), ("rs_rgb_to_y_u8", 4)):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == n_args
    for text in ("size_t rs_metrics_work_bytes(int B, int C, int H, int W, int border, int ycbcr);",
                 "int rs_metrics(const void* a, const void* b, int a_is_float, int b_is_float, int B, int C, int H, int W, int border, int ycbcr,",
                 "int rs_rgb_to_y_u8(const uint8_t* rgb_hwc, uint8_t* y, size_t pixels, void* stream);",
                 "Y = 16 + round((65481 r + 128553 g + 24966 b) / 255000)", "C1 = 6.5025, C2 = 58.5225", "194 RGB triples", "tests/_metrics_ref.py"):
        assert text in header, text
    # one quantiser: rs_output_to_u8's kernel and the metric's float inputs call the same device function
    common = open(H.ROOT + "/resshift_amd/csrc/common.h").read()
    assert "unsigned char rs_unit_to_u8(float v)" in common and "unsigned char rs_sample_to_u8(float x)" in common
    assert "rs_unit_to_u8(v)" in open(H.ROOT + "/resshift_amd/csrc/elementwise.hip").read()
    src = open(H.ROOT + "/resshift_amd/csrc/metrics.hip").read()
    assert "rs_sample_to_u8(" in src and "rs_rgb_to_y(" in src and "atomic" not in src.replace("floating-point atomics", "")


def test_lib_metrics_rejects_bad_arguments_before_the_library_is_called(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was reached"))
    u8 = torch.zeros(2, 24, 32, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="a must be a contiguous device tensor"):
        _lib.metrics(u8, u8)                                   # host tensors: there is no CPU arithmetic to fall back to
    d = u8.as_subclass(_OnDevice)
    f = torch.zeros(2, 3, 24, 32).as_subclass(_OnDevice)
    with pytest.raises(ValueError, match="b must be a contiguous device tensor"):
        _lib.metrics(d, u8)
    for bad in (d.to(torch.int16), f.double(), d[0], d[:, :, ::2], f[..., ::2]):
        with pytest.raises(ValueError, match="a must be a contiguous device tensor"):
            _lib.metrics(bad, d)
    with pytest.raises(ValueError, match=r"a is 2 images of 24 x 32 x 3, b is 2 images of 24 x 30 x 3"):
        _lib.metrics(d, d[:, :, :30].contiguous())
    with pytest.raises(ValueError, match=r"a is 2 images of 24 x 32 x 3, b is 1 images of 24 x 32 x 3"):
        _lib.metrics(d, f[:1])
    with pytest.raises(ValueError, match=r"b is 2 images of 3 x 24 x 32"):
        _lib.metrics(d, torch.zeros(2, 32, 3, 24).as_subclass(_OnDevice))      # a float batch laid out like the uint8 one
    with pytest.raises(ValueError, match="C must be 1 or 3, not 2"):
        _lib.metrics(d[..., :2].contiguous(), d[..., :2].contiguous())
    with pytest.raises(ValueError, match="ycbcr=True needs C == 3, not 1"):
        _lib.metrics(d[..., :1].contiguous(), f[:, :1].contiguous())
    for bad in (-1, 1.0, True, "0"):
        with pytest.raises(ValueError, match="border must be a non-negative integer"):
            _lib.metrics(d, f, border=bad)
    with pytest.raises(ValueError, match=r"the cropped image is 10 x 18 \(24 x 32, border 7\)"):
        _lib.metrics(d, f, border=7)
    with pytest.raises(ValueError, match=r"the cropped image is 24 x 10 \(24 x 10, border 0\)"):
        _lib.metrics(d[:, :, :10].contiguous(), d[:, :, :10].contiguous(), ycbcr=False)
    for bad in (u8, d.float(), d[..., :2].contiguous(), d[:, :, ::2], d[:0]):
        with pytest.raises(ValueError, match="rgb_to_y: rgb must be"):
            _lib.rgb_to_y(bad)


# ---------------------------------------------------------------------------------------------------------------- host plumbing
class ScoringEngine:
    """u8_to_input / output_to_u8 of the plumbing tests plus `metrics`: the "sample" is the input itself, the score the restatement's"""

    def __init__(self):
        self.scored = []

    def u8_to_input(self, t):
        return t.permute(0, 3, 1, 2).float()

    def output_to_u8(self, sr, lq=None, mask=None):
        return sr.permute(0, 2, 3, 1).to(torch.uint8)

    def metrics(self, sr, gt, border=0, ycbcr=True):
        assert sr.dtype == gt.dtype == torch.uint8 and sr.shape == gt.shape
        self.scored.append((tuple(sr.shape), border, ycbcr))
        sse, psnr, ssim = M.batch(sr.numpy(), gt.numpy(), border, ycbcr)
        return {"psnr": torch.from_numpy(psnr), "ssim": torch.from_numpy(ssim), "sse": torch.from_numpy(sse)}


def _stub_sampler(rank=0, world=1):
    s = ResShiftSampler.__new__(ResShiftSampler)
    s.seed, s.rank, s.num_gpus, s.device, s.engine, s.chop_size, s.sf = 7, rank, world, torch.device("cpu"), ScoringEngine(), 128, 1
    s.sample_tiled = lambda lq, mask=None, noise_repeat=False, tile_noises=None, seed=None: lq
    return s


def _folder(tmp_path, golden, names=("b", "a", "c")):
    from PIL import Image

    src, gtd = tmp_path / "in", tmp_path / "gt"
    src.mkdir()
    gtd.mkdir()
    for i, n in enumerate(names):
        Image.fromarray(golden["sr_s10"][i]).save(src / f"{n}.png")
        Image.fromarray(golden["gt"][i]).save(gtd / f"{n}.png")
    return src, gtd


def _read_csv(path):
    with open(path) as fh:
        return list(csv.reader(fh))


@pytest.mark.parametrize("pool", [False, True])
def test_inference_scores_every_image_against_the_file_of_its_name(tmp_path, golden, monkeypatch, pool):
    from resshift_amd import tilepool

    monkeypatch.setattr(tilepool, "TilePool", InstantPool)   # completes every image at the next step: the "sample" is the input
    src, gtd = _folder(tmp_path, golden)
    s = _stub_sampler()
    rows = s.inference(src, tmp_path / "out", bs=2, pool=pool, gt_path=gtd, metric_border=4, metric_ycbcr=False)
    assert sorted(rows) == ["a", "b", "c"]
    assert all(sc[1:] == (4, False) for sc in s.engine.scored) and sum(sc[0][0] for sc in s.engine.scored) == 3
    for i, n in enumerate(("b", "a", "c")):
        _, psnr, ssim = M.metrics(golden["sr_s10"][i], golden["gt"][i], 4, False)
        assert rows[n] == (psnr, ssim)
        assert abs(psnr - float(golden[f"psnr_s10_im{i}_y0_b4"])) <= 1e-10 and abs(ssim - float(golden[f"ssim_s10_im{i}_y0_b4"])) <= 1e-12
    table = _read_csv(tmp_path / "out" / "metrics.csv")
    assert table[0] == ["name", "psnr", "ssim"] and [r[0] for r in table[1:]] == ["a", "b", "c", "mean"]
    for r in table[1:4]:
        assert (float(r[1]), float(r[2])) == rows[r[0]]                            # the CSV holds the float64 values exactly
    assert float(table[4][1]) == float(np.mean([rows[k][0] for k in "abc"])) and float(table[4][2]) == float(np.mean([rows[k][1] for k in "abc"]))
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["a.png", "b.png", "c.png", "metrics.csv"]
    # without gt_path: the same PNGs, no table, nothing returned, the engine's metrics never called
    s2 = _stub_sampler()
    assert s2.inference(src, tmp_path / "plain", bs=2, pool=pool) is None
    assert s2.engine.scored == [] and sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["a.png", "b.png", "c.png"]
    # the default parameters: border 0, the Y channel
    s3 = _stub_sampler()
    rows3 = s3.inference(src, tmp_path / "y", pool=pool, gt_path=gtd)
    assert all(sc[1:] == (0, True) for sc in s3.engine.scored)
    assert rows3["a"] == M.metrics(golden["sr_s10"][1], golden["gt"][1], 0, True)[1:]


def test_a_single_input_file_takes_gt_path_as_the_file_itself(tmp_path, golden):
    src, gtd = _folder(tmp_path, golden)
    s = _stub_sampler()
    rows = s.inference(src / "a.png", tmp_path / "out", gt_path=gtd / "c.png")
    assert rows == {"a": M.metrics(golden["sr_s10"][1], golden["gt"][2], 0, True)[1:]}
    with pytest.raises(FileNotFoundError, match="no ground truth for a.png"):
        s.inference(src / "a.png", tmp_path / "out", gt_path=gtd)                  # a directory is not the file


def test_missing_and_missized_ground_truth(tmp_path, golden):
    from PIL import Image

    src, gtd = _folder(tmp_path, golden)
    (gtd / "c.png").unlink()
    s = _stub_sampler()
    with pytest.raises(FileNotFoundError, match="no ground truth for c.png"):
        s.inference(src, tmp_path / "out", gt_path=gtd)
    assert s.engine.scored == [] and not (tmp_path / "out" / "a.png").exists()     # found before anything is sampled
    Image.fromarray(golden["gt"][2][:48]).save(gtd / "c.png")
    with pytest.raises(ValueError, match=r"the ground truth of c.png is 48 x 64, the output is 64 x 64"):
        s.inference(src, tmp_path / "out", gt_path=gtd)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="metric_border must be a non-negative integer"):
            s.inference(src, tmp_path / "out", gt_path=gtd, metric_border=bad)


def test_each_rank_scores_its_share_and_the_rows_are_combined(tmp_path, golden, monkeypatch):
    """two ranks, run one after the other with all_gather_object replaced by the exchange it performs"""
    import torch.distributed as dist

    src, gtd = _folder(tmp_path, golden)
    shares = {}
    for rank in (0, 1):
        s = _stub_sampler(rank, 2)
        monkeypatch.setattr(s, "_finish_metrics", lambda out_path, rows, rank=rank: shares.__setitem__(rank, dict(rows)) or rows)
        s.inference(src, tmp_path / "out", bs=2, gt_path=gtd)
    assert sorted(shares[0]) == ["a", "c"] and sorted(shares[1]) == ["b"]          # bs = 2 over two ranks: a | b, then c | -

    def gather(parts, mine):
        parts[:] = [shares[0], shares[1]]

    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda: 2)
    monkeypatch.setattr(dist, "all_gather_object", gather)
    for rank in (0, 1):
        s = _stub_sampler(rank, 2)
        (tmp_path / f"o{rank}").mkdir()
        rows = s._finish_metrics(tmp_path / f"o{rank}", shares[rank])
        assert sorted(rows) == ["a", "b", "c"]
        assert (tmp_path / f"o{rank}" / "metrics.csv").exists() == (rank == 0)


def test_the_csv_writer():
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        mean = ResShiftSampler._write_metrics(d, {"z": (30.0, 0.9), "a": (math.inf, 1.0), "m": (20.5, 0.125)})
        assert mean == (math.inf, float(np.mean([1.0, 0.125, 0.9])))
        assert _read_csv(d + "/metrics.csv") == [["name", "psnr", "ssim"], ["a", "inf", "1.0"], ["m", "20.5", "0.125"], ["z", "30.0", "0.9"],
                                                ["mean", "inf", repr(mean[1])]]

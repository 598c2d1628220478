"""The face recipe without a GPU: the integer restatement of libjpeg's round trip against the recorded and the live
Pillow, the mutations the recorded cases catch, the quantisation tables, the pinned fp32 distance of the reference's blur + resize from
the float64 restatement, the plans, every argument error of rs_jpeg_codec and rs_blur_resize, the wrappers, the command line and the
order in which `run_face` calls the operators."""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401  (puts the repository root on sys.path)
import _degrade_ref as D
import _face_ref as F
import _jpeg_ref as J
from _fakes import _OnDevice, lib  # noqa: F401  (fixture)
from resshift_amd import _lib, build, degrade


@pytest.fixture(scope="module")
def fixture():
    return np.load(H.ROOT + "/tests/golden/libjpeg_roundtrip.npz")


# ---------------------------------------------------------------------------------------------------------------- the codec's definition
def test_the_restatement_equals_the_recorded_libjpeg_on_every_byte(fixture):
    sizes, qualities = set(), set()
    for key, (Hh, W), kind, seed, q in J.cases():
        u8 = J.to_u8(J.content(kind, Hh, W, seed))
        assert np.array_equal(u8, fixture["in_" + key]) and int(fixture["q_" + key]) == q, key
        assert np.array_equal(J.roundtrip(u8, q), fixture["out_" + key]), key
        sizes.add((Hh, W))
        qualities.add(q)
    assert sizes == set(J.SIZES) and qualities == set(J.QUALITIES) == {1, 30, 49, 50, 69, 95, 100}
    assert {(8, 8), (16, 16), (9, 8), (17, 33), (24, 72), (40, 56), (31, 50), (64, 48), (48, 64)} <= sizes
    ties = J.content("float", 17, 33, 5)
    prod = ties * np.float32(255)
    assert (prod - np.floor(prod) == 0.5).sum() > 100 and ties.min() < 0 and ties.max() > 1       # exact .5 ties, values outside [0, 1]


def test_the_restatement_equals_the_live_pillow(fixture):
    """skips - printing both version strings - only where the live Pillow disagrees with the fixture's OWN outputs: another libjpeg build"""
    import PIL
    from PIL import features

    live = f"Pillow {PIL.__version__}, libjpeg {features.version('jpg')}"
    recorded = f"Pillow {fixture['pillow']}, libjpeg {fixture['libjpeg']}"
    for key, _, _, _, q in J.cases():
        if not np.array_equal(J.pillow_roundtrip(fixture["in_" + key], q), fixture["out_" + key]):
            pytest.skip(f"the live {live} does not reproduce the fixture recorded with {recorded} on {key}: another libjpeg build")
    rng = np.random.default_rng(3)
    for Hh, W in [(8, 8), (13, 21), (32, 5 + 16), (33, 47)]:
        u8 = rng.integers(0, 256, (Hh, W, 3), dtype=np.uint8)
        q = int(rng.integers(1, 101))
        assert np.array_equal(J.roundtrip(u8, q), J.pillow_roundtrip(u8, q)), (Hh, W, q, live)


@pytest.mark.parametrize("mut", J.MUTATIONS)
def test_the_recorded_cases_catch_the_mutation(fixture, mut):
    caught = [key for key, *_ in J.cases() if not np.array_equal(J.roundtrip(fixture["in_" + key], int(fixture["q_" + key]), mut), fixture["out_" + key])]
    print(f"{mut}: moves bytes in {len(caught)} of {len(J.cases())} recorded cases")
    assert len(caught) >= 5, (mut, caught)


def test_quantisation_tables():
    assert np.all(J.quant_table(J.LUMA, 1) == 255) and np.all(J.quant_table(J.CHROMA, 1) == 255)
    assert np.all(J.quant_table(J.LUMA, 100) == 1) and np.all(J.quant_table(J.CHROMA, 100) == 1)
    assert np.array_equal(J.quant_table(J.LUMA, 50), J.LUMA) and np.array_equal(J.quant_table(J.CHROMA, 50), J.CHROMA)
    assert J.quant_table(J.LUMA, 49)[0].tolist() == [16, 11, 10, 16, 24, 41, 52, 62]               # (base 102 + 50) / 100
    assert J.quant_table(J.CHROMA, 49)[0].tolist() == [17, 18, 24, 48, 101, 101, 101, 101]
    assert J.LUMA[0].tolist() == [16, 11, 10, 16, 24, 40, 51, 61] and J.LUMA[1].tolist() == [12, 12, 14, 19, 26, 58, 60, 55]
    assert np.array_equal(J.LUMA.T, D.Y_TABLE.astype(np.int64)) and np.array_equal(J.CHROMA.T, D.C_TABLE.astype(np.int64))   # degrade.hip's are transposed
    for bad in (0, 101):
        with pytest.raises(ValueError, match="outside 1 .. 100"):
            J.quant_table(J.LUMA, bad)


# ---------------------------------------------------------------------------------------------------------------- blur + resize
def test_the_pinned_error_of_the_reference_blur_resize_is_what_was_measured():
    """the reference's fp32 filter2D -> fp32 F.interpolate(bilinear), recorded, against the float64 restatement"""
    ref = np.load(H.ROOT + "/tests/golden/reference_face.npz")
    worst, n = 0.0, 0
    for i, (key, k, nk, seed) in enumerate(F.BLUR_KERNELS):
        x, kernels = F.blur_case(i)
        assert kernels.shape == (nk, k, k) and not np.allclose(kernels, kernels[:, ::-1, ::-1])    # a flipped kernel is another kernel
        for size in F.BLUR_SIZES:
            y = ref[f"blur_{key}_{size[0]}x{size[1]}"]
            assert y.dtype == np.float32 and y.shape == (2, 3, *size)
            worst = max(worst, float(np.abs(F.blur_resize(x, kernels, size) - y).max()))
            assert float(np.abs(F.blur_resize(x, kernels, size, flip=True) - y).max()) > (1e-2 if min(size) > 2 else 1e-4)
            n += 1
    for i, (shape, size) in enumerate(F.RESIZE_CASES):
        x = D.inputs((2, 3, *shape), F.RESIZE_SEED + i)[:1, :1]
        worst = max(worst, float(np.abs(F.blur_resize(x, None, size) - ref[f"resize_{i}"]).max()))
        n += 1
    print(f"{n} recorded cases: max |float64 restatement - reference fp32| = {worst:.3e} (pinned {F.REF_ERR:.1e}, GPU bound {F.TOL:.1e})")
    assert F.REF_ERR / 2 < worst <= F.REF_ERR and F.TOL == 5 * F.REF_ERR
    assert {c[1] for c in F.BLUR_KERNELS} == {41, 21, 3} and F.BLUR_SIZES == [(45, 52), (11, 13), (1, 2), (23, 31)]
    assert F.RESIZE_CASES == [((6, 10), (192, 320)), ((24, 40), (31, 47))]


# ---------------------------------------------------------------------------------------------------------------- plans
def test_face_plans_are_deterministic_and_round_trip_through_json():
    a, b = degrade.draw_face_plan(degrade.FACE_TESTING, 512, 512, 7), degrade.draw_face_plan(degrade.FACE_TESTING, 512, 512, 7)
    assert a == b and a != degrade.draw_face_plan(degrade.FACE_TESTING, 512, 512, 8)
    assert degrade.FacePlan.from_json(a.to_json()) == a and degrade.FacePlan.from_dict(a.to_dict()) == a
    assert a.stages() == ["blur_down", "noise", "jpeg", "up", "round"] and a.kernel().shape == (41, 41) and abs(a.kernel().sum() - 1) < 1e-6
    o = degrade.FACE_TESTING
    assert (o.sf, o.qf, o.nf, o.sig, o.kernel_size) == ((1.0, 32.0), (30.0, 70.0), (1.0, 20.0), (4.0, 16.0), 41) and o.theta == (0.0, math.pi)
    with pytest.raises(Exception):
        o.kernel_size = 3                                                                        # frozen


def test_every_drawn_face_value_lies_inside_its_range():
    seen = set()
    for seed in range(200):
        Hh, W = (256, 272) if seed % 2 else (512, 384)
        p = degrade.draw_face_plan(degrade.FACE_TESTING, Hh, W, seed)
        assert 1.0 <= p.sf < 32.0 and 1.0 <= p.nf < 20.0 and 4.0 <= p.sig_x < 16.0 and 4.0 <= p.sig_y < 16.0 and 0.0 <= p.theta < math.pi
        assert isinstance(p.quality, int) and 30 <= p.quality <= 69
        assert p.small == (int(Hh // p.sf), int(W // p.sf)) and min(p.small) >= 8 and (p.H, p.W, p.seed, p.kernel_size) == (Hh, W, seed, 41)
        seen.add(p.quality)
    assert len(seen) > 30


def test_face_plan_errors():
    with pytest.raises(ValueError, match="has a side below 256"):
        degrade.draw_face_plan(degrade.FACE_TESTING, 255, 512, 1)
    ok = dict(H=256, W=272, sf=4.0, sig_x=5.0, sig_y=6.0, theta=0.3, nf=3.0, qf=50.5)
    assert degrade.face_plan(**ok).quality == 50 and degrade.face_plan(**ok).small == (64, 68)
    assert degrade.face_plan(**{**ok, "sf": 31.9}).small == (8, 8)
    for kw, text in ((dict(sf=0.5), r"sf = 0.5 must lie in \[1, 64\]"), (dict(sf=33.0), "gives 7 x 8, below the JPEG codec's 8"), (dict(qf=0.5), "must lie in 1 .. 100"),
                     (dict(qf=101.0), "must lie in 1 .. 100"), (dict(kernel_size=43), "odd and at most 41"), (dict(kernel_size=4), "odd and at most 41"),
                     (dict(H=20, sf=1.0), "too small for a blur kernel of 41 taps"), (dict(nf=-1.0), "nf must not be negative"), (dict(H=0), "must be positive")):
        with pytest.raises(ValueError, match=text):
            degrade.face_plan(**{**ok, **kw})


def test_make_face_testset_names_the_small_file_before_anything_is_written(tmp_path, monkeypatch):
    from PIL import Image

    monkeypatch.setattr(degrade, "Degrader", lambda *a: pytest.fail("nothing is degraded before every file is checked"))
    Image.fromarray(np.zeros((256, 256, 3), np.uint8)).save(tmp_path / "a.png")
    Image.fromarray(np.zeros((300, 200, 3), np.uint8)).save(tmp_path / "b.png")
    with pytest.raises(ValueError, match=r"b\.png: 300 x 200 has a side below 256"):
        degrade.make_face_testset(tmp_path, tmp_path / "lq")
    assert not (tmp_path / "lq").exists()


def test_the_command_line_selects_the_recipe(tmp_path, monkeypatch, capsys):
    calls = []
    monkeypatch.setattr(degrade, "make_testset", lambda gt, lq, **kw: calls.append(("realesrgan", gt, lq, kw)) or {})
    monkeypatch.setattr(degrade, "make_face_testset", lambda gt, lq, **kw: calls.append(("face", gt, lq, kw)) or {"a": 1})
    degrade.main(["gt", "lq"])
    degrade.main(["gt", "lq", "--recipe", "realesrgan", "--sf", "2"])
    degrade.main(["gt", "lq", "--recipe", "face", "--seed", "5"])
    assert calls == [("realesrgan", "gt", "lq", dict(sf=4, seed=10000)), ("realesrgan", "gt", "lq", dict(sf=2, seed=10000)), ("face", "gt", "lq", dict(seed=5))]
    assert "1 images -> lq" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        degrade.main(["gt", "lq", "--recipe", "celeba"])


def test_make_lq_dispatches_on_the_type_of_the_options(monkeypatch):
    from resshift_amd import sampler as S

    calls = []
    monkeypatch.setattr(degrade, "list_images", lambda p: ["x.png", "y.png"])
    monkeypatch.setattr(degrade, "make_testset", lambda gt, lq, **kw: calls.append(("realesrgan", kw)) or {})
    monkeypatch.setattr(degrade, "make_face_testset", lambda gt, lq, **kw: calls.append(("face", kw)) or {})
    monkeypatch.setattr(degrade, "write_plans", lambda lq, plans: None)
    s = S.ResShiftSampler.__new__(S.ResShiftSampler)
    s.seed, s.sf, s.num_gpus, s.rank, s.device = 3, 4, 1, 0, torch.device("cpu")
    s.make_lq("gt", "lq")
    s.make_lq("gt", "lq", opts=degrade.FACE_TESTING, seed=9)
    assert [c[0] for c in calls] == ["realesrgan", "face"]
    assert calls[0][1]["opts"] is degrade.REALESRGAN_TESTING and calls[0][1]["sf"] == 4 and calls[0][1]["seed"] == 3 and calls[0][1]["positions"] == [0, 1]
    assert calls[1][1] == dict(opts=degrade.FACE_TESTING, seed=9, device=torch.device("cpu"), positions=[0, 1])


class _RecordingOps:
    """stands in for the engine: records the operator calls of run_face and returns tensors of the right shapes"""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def filter2d(self, *a, **kw):
        pytest.fail("run_face has no separate blur")

    def blur_resize(self, x, kernels, size, clamp=False):
        self.calls.append(("blur_resize", tuple(x.shape), None if kernels is None else tuple(kernels.shape), tuple(size), clamp))
        return torch.full((x.shape[0], x.shape[1], *size), 0.25)

    def add_noise(self, x, keys, sigma, gray=False, draw=0, clamp=True):
        self.calls.append(("add_noise", tuple(x.shape), list(keys), list(sigma), gray, draw, clamp))
        return x + 0.125

    def jpeg_codec(self, x, quality):
        self.calls.append(("jpeg_codec", tuple(x.shape), list(quality)))
        return x * 2.0

    def unit_to_u8(self, x):
        self.calls.append(("unit_to_u8", tuple(x.shape)))
        return (x * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def test_run_face_calls_the_operators_in_the_recipes_order():
    ops = _RecordingOps()
    plan = degrade.face_plan(256, 272, sf=4.0, sig_x=5.0, sig_y=6.0, theta=0.3, nf=3.5, qf=41.9, noise_seed=77)
    lq, log = degrade.Degrader(ops).run_face(torch.zeros(1, 3, 256, 272), plan, trace=True)
    assert ops.calls == [("blur_resize", (1, 3, 256, 272), (1, 41, 41), (64, 68), False),
                         ("add_noise", (1, 3, 64, 68), [(77, 0)], [3.5], False, 0, True),
                         ("jpeg_codec", (1, 3, 64, 68), [41]),
                         ("blur_resize", (1, 3, 64, 68), None, (256, 272), False),
                         ("unit_to_u8", (1, 3, 256, 272))]
    assert [s[0] for s in log] == plan.stages() and all(b[1] is a[2] for a, b in zip(log, log[1:]))
    assert tuple(lq.shape) == (1, 3, 256, 272) and torch.equal(lq, torch.full_like(lq, 64.0 / 255.0)) and log[-1][2].dtype == torch.uint8
    with pytest.raises(ValueError, match="the plan is for"):
        degrade.Degrader(ops).run_face(torch.zeros(2, 3, 256, 272), plan)


# ---------------------------------------------------------------------------------------------------------------- C ABI
PTR, FAR, KPTR = 0x100000, 0x40000000, 0x70000000   # never dereferenced: every call below is refused before anything is launched

CODEC_ERRORS = {
    "null_in": (dict(inp=None), "rs_jpeg_codec: null pointer (in / out / quality)"), "null_out": (dict(out=None), "rs_jpeg_codec: null pointer (in / out / quality)"),
    "null_quality": (dict(q=None), "rs_jpeg_codec: null pointer (in / out / quality)"),
    "batch": (dict(B=0), "rs_jpeg_codec: B must be 1 .. RS_MAX_ROWS (the qualities travel by value)"),
    "large_batch": (dict(B=65), "rs_jpeg_codec: B must be 1 .. RS_MAX_ROWS (the qualities travel by value)"),
    "channels": (dict(C=1), "rs_jpeg_codec: C must be 3 (RGB)"), "height": (dict(H=7), "rs_jpeg_codec: H and W must be at least 8"),
    "width": (dict(W=0), "rs_jpeg_codec: H and W must be at least 8"),
    "huge": (dict(W=(1 << 28) + 1), "rs_jpeg_codec: a plane is too large (a side above 2^28 or more than 2^40 pixels)"),
    "quality_0": (dict(q=[50, 0]), "rs_jpeg_codec: every quality must be an integer in 1 .. 100"),
    "quality_101": (dict(q=[101, 50]), "rs_jpeg_codec: every quality must be an integer in 1 .. 100"),
    "in_place": (dict(out=PTR), "rs_jpeg_codec: `out` overlaps `in` (a tile reads the chroma ring of its neighbours: not in place)"),
    "partial_overlap": (dict(out=PTR + 64), "rs_jpeg_codec: `out` overlaps `in` (a tile reads the chroma ring of its neighbours: not in place)"),
}


@pytest.mark.parametrize("name", sorted(CODEC_ERRORS))
def test_jpeg_codec_argument_errors(lib, name):
    kw, text = CODEC_ERRORS[name]
    a = dict(inp=PTR, out=FAR, q=[30, 70], B=2, C=3, H=40, W=52)
    a.update(kw)
    q = (C.c_int * 65)(*a["q"]) if a["q"] is not None else None
    rc = lib.rs_jpeg_codec(a["inp"], a["out"], q, a["B"], a["C"], a["H"], a["W"], None)
    assert rc == -2 and _lib.last_error() == text, (rc, _lib.last_error())


BLUR_ERRORS = {
    "null_in": (dict(inp=None), "rs_blur_resize: null tensor (in / out)"), "null_out": (dict(out=None), "rs_blur_resize: null tensor (in / out)"),
    "batch": (dict(B=0), "rs_blur_resize: B, C, H, W, Ho and Wo must be positive"), "out_width": (dict(Wo=0), "rs_blur_resize: B, C, H, W, Ho and Wo must be positive"),
    "no_kernel_but_k": (dict(kern=None), "rs_blur_resize: without kernels k must be 0"),
    "even_k": (dict(k=4), "rs_blur_resize: k must be odd and at most 41"), "large_k": (dict(k=43), "rs_blur_resize: k must be odd and at most 41"),
    "zero_k": (dict(k=0), "rs_blur_resize: k must be odd and at most 41"),
    "deep_reflection": (dict(H=20, Ho=10, k=41), "rs_blur_resize: k / 2 must be below min(H, W) (one reflection per border)"),
    "kernel_count": (dict(Bk=3), "rs_blur_resize: Bk must be 1 (one kernel for the batch) or B (one per image)"),
    "clamp": (dict(clamp=2), "rs_blur_resize: clamp must be 0 or 1"),
    "huge": (dict(Wo=(1 << 28) + 1), "rs_blur_resize: a plane is too large (a side above 2^28 or more than 2^40 pixels)"),
    "scale_small": (dict(H=130, Ho=2), "rs_blur_resize: the scales Ho / H and Wo / W must lie in [1/64, 64]"),
    "scale_large": (dict(Wo=52 * 64 + 1), "rs_blur_resize: the scales Ho / H and Wo / W must lie in [1/64, 64]"),
    "in_place": (dict(out=PTR), "rs_blur_resize: `out` overlaps `in` (not in place)"),
}


@pytest.mark.parametrize("name", sorted(BLUR_ERRORS))
def test_blur_resize_argument_errors(lib, name):
    kw, text = BLUR_ERRORS[name]
    a = dict(inp=PTR, kern=KPTR, out=FAR, B=2, C=3, H=40, W=52, Ho=20, Wo=13, k=13, Bk=2, clamp=0)
    a.update(kw)
    rc = lib.rs_blur_resize(a["inp"], a["kern"], a["out"], a["B"], a["C"], a["H"], a["W"], a["Ho"], a["Wo"], a["k"], a["Bk"], a["clamp"], None)
    assert rc == -2 and _lib.last_error() == text, (rc, _lib.last_error())


def test_the_header_declares_what_the_signatures_bind(lib):
    header = open(H.ROOT + "/include/resshift_hip.h").read()
    ctype = {"int": C.c_int, "void*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p, "const int*": C.POINTER(C.c_int)}
    for name in ("rs_jpeg_codec", "rs_blur_resize"):
        m = re.search(r"\nint " + name + r"\(([^;]*)\);", header)
        assert m, name
        want, last = [], None
        for a in [a.strip() for a in " ".join(m.group(1).split()).split(",")]:   # "int B" / "int C": a bare name takes the previous type
            t, _, n = a.rpartition(" ")
            last = t or last
            want.append(ctype[t or last])
        res, got = _lib.SIGNATURES[name]
        assert res is C.c_int and got == want, (name, got, want)
        assert hasattr(lib, name)
    for text in ("FIX16(c) = (int)(c 65536 + .5)", "(128 << 16) + 32767", "up to an EVEN row count only", "bias 1 on even output columns and 2 on odd ones",
                 "q = sign(c) ((|c| + (d >> 1)) / d)", "odd = (3 s[j] + s[j+1] + 7) >> 4", "tests/_jpeg_ref.py", "(float) v / 255.f", "[1/64, 64]",
                 "kernels == NULL"):
        assert text in header, text
    assert "jpeg_codec.hip" in build.SOURCES and "blur_resize.hip" in build.SOURCES
    assert _lib.BLUR_RESIZE_KMAX == 41 and _lib.FILTER_KMAX == 21 and _lib.RESIZE_SCALES == (0.125, 8.0)   # the pinned limits have not moved


def test_lib_wrappers_reject_bad_arguments_before_the_library_is_called(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was reached"))
    x = torch.zeros(2, 3, 64, 80)
    d = x.as_subclass(_OnDevice)
    k = torch.zeros(1, 41, 41).as_subclass(_OnDevice)
    for fn, args in ((_lib.jpeg_codec, (x, 50)), (_lib.blur_resize, (x, k, (8, 8)))):
        with pytest.raises(ValueError, match="contiguous float32 device tensor"):
            fn(*args)                                                  # a host tensor: there is no CPU arithmetic to fall back to
    with pytest.raises(ValueError, match="C must be 3"):
        _lib.jpeg_codec(torch.zeros(1, 1, 16, 16).as_subclass(_OnDevice), 50)
    with pytest.raises(ValueError, match="H and W must be at least 8, not 7 x 16"):
        _lib.jpeg_codec(torch.zeros(1, 3, 7, 16).as_subclass(_OnDevice), 50)
    for bad in (0, 101, 50.0, True, [50, 50.5], float("nan")):
        with pytest.raises(ValueError, match=r"every quality must be an integer in 1 \.\. 100"):
            _lib.jpeg_codec(d, bad)
    with pytest.raises(ValueError, match="2 images but 3 qualities"):
        _lib.jpeg_codec(d, [50, 60, 70])
    with pytest.raises(ValueError, match=r"kernels .* must be a contiguous float32 tensor on x's device \(or None\)"):
        _lib.blur_resize(d, torch.zeros(1, 7, 7), (8, 8))
    for bad, text in ((torch.zeros(1, 4, 4), "k must be odd"), (torch.zeros(1, 43, 43), "k must be odd and at most 41"), (torch.zeros(3, 7, 7), "3 kernels for 2 images")):
        with pytest.raises(ValueError, match=text):
            _lib.blur_resize(d, bad.as_subclass(_OnDevice), (8, 8))
    with pytest.raises(ValueError, match="below min"):
        _lib.blur_resize(torch.zeros(1, 3, 20, 80).as_subclass(_OnDevice), k, (8, 8))
    for bad in ((12,), (12.0, 20), (0, 20), 12, None):
        with pytest.raises(ValueError, match="size must be two positive integers"):
            _lib.blur_resize(d, k, bad)
    for size in ((64, 1), (64 * 64 + 1, 80)):
        with pytest.raises(ValueError, match=r"must lie in \[1/64, 64\]"):
            _lib.blur_resize(d, None, size)

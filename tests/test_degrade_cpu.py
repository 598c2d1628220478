"""The degradation operators without a GPU: the float64 restatement (tests/_degrade_ref.py) against the recorded outputs of
the reference's filter2D, DiffJPEG and kernel builders (tests/golden/reference_degrade.npz, scripts/make_golden_degrade.py), the
preset's numbers, the measurement the GPU bounds come from, the mutations those bounds must catch, the plans, the argument errors of
the five entry points - found before anything is launched - and the header text against the ctypes signatures."""
import ctypes as C
import dataclasses
import json
import math
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers as H  # noqa: F401  (puts the repository root on sys.path)
import _degrade_ref as R
from _fakes import _OnDevice, lib  # noqa: F401  (fixture)
from resshift_amd import _lib, build, degrade

GOLD = np.load(H.ROOT + "/tests/golden/reference_degrade.npz")
MEASURED = {}


def _pinned(op, err):
    """the measurement must be what REF_ERR pins: not above it, and not so far below that the GPU bound would be loose"""
    MEASURED[op] = max(MEASURED.get(op, 0.0), err)


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", R.FILTER_CASES, ids=[c[0] for c in R.FILTER_CASES])
def test_filter_restatement_against_the_recorded_reference(case):
    key = case[0]
    x, kernels = R.filter_case(case)
    assert np.array_equal(R.digest(x), GOLD["in_sha256_" + key]) and np.array_equal(R.digest(kernels), GOLD["kernels_sha256_" + key])
    want = GOLD["filter_" + key]
    assert want.dtype == np.float32 and want.shape == x.shape
    err = float(np.abs(R.filter2d(x, kernels) - want).max())
    print(f"filter2D {key} (k = {kernels.shape[-1]}, {kernels.shape[0]} kernel(s), min weight {kernels.min():+.3f}): |reference fp32 - float64 restatement| = {err:.2e}")
    _pinned("filter", err)
    assert err <= R.REF_ERR["filter"]


def test_the_recorded_filter_cases_cover_the_sizes_and_the_negative_lobes():
    ks = {R.filter_case(c)[1].shape[-1] for c in R.FILTER_CASES}
    assert ks == {3, 7, 13, 21}
    assert {R.filter_case(c)[1].shape[0] for c in R.FILTER_CASES} == {1, 2}
    assert sum(R.filter_case(c)[1].min() < -1e-3 for c in R.FILTER_CASES) >= 3          # sinc kernels
    assert sorted(k for k in GOLD.files if k.startswith("filter_")) == sorted("filter_" + c[0] for c in R.FILTER_CASES)


@pytest.mark.parametrize("case", R.JPEG_CASES, ids=[c[0] for c in R.JPEG_CASES])
def test_jpeg_restatement_and_closed_form_against_the_recorded_reference(case):
    key, (Hh, W), qualities, seed = case
    x, want, tie = R.constructed_jpeg_case(Hh, W, qualities, seed)
    assert np.array_equal(R.digest(x), GOLD["in_sha256_jpeg_" + key])
    ref = GOLD["jpeg_" + key]
    got, coefs = R.jpeg(x, qualities, return_coefficients=True)
    e_closed, e_rest = float(np.abs(want - ref).max()), float(np.abs(got - ref).max())
    print(f"DiffJPEG {key}: |reference fp32 - closed form| = {e_closed:.2e}, |reference fp32 - float64 restatement| = {e_rest:.2e}, "
          f"smallest tie distance {tie:.4f}; input range [{x.min():.3f}, {x.max():.3f}]")
    assert tie >= 0.0999                                            # every pre-round coefficient at least 0.1 from a tie
    assert np.abs(got - want).max() <= 1e-12                        # the restatement finds the chosen coefficients again
    assert coefs[0][0].shape == (Hh // 8, W // 8, 8, 8) and coefs[0][1].shape == (Hh // 16, W // 16, 8, 8)
    _pinned("jpeg", e_closed)
    assert e_closed <= R.REF_ERR["jpeg"] and e_rest <= R.REF_ERR["jpeg"]


@pytest.mark.parametrize("case", R.BUILDER_CASES, ids=[c[0] for c in R.BUILDER_CASES])
def test_kernel_builders_against_the_recorded_reference(case):
    """float32 of our float64 against the reference's float64: 1e-7 covers the float32 rounding of weights below 1 (6e-8) and, for the sinc
    kernels, torch's bessel_j1 against scipy's (measured 7.8e-8 together)"""
    want = GOLD["kernel_" + case[0]]
    got = R.builder_ours(case)
    assert got.dtype == np.float32 and got.shape == want.shape
    err = float(np.abs(got - want).max())
    print(f"{case[1]} {case[0]}: |ours - reference| = {err:.2e}, sum {got.sum(dtype=np.float64):.8f}")
    assert err <= 1e-7 and abs(float(got.sum(dtype=np.float64)) - 1.0) <= 1e-6


def test_kernel_specs():
    pulse = degrade.KernelSpec("pulse", 7, 7).array()
    assert pulse.shape == (7, 7) and pulse[3, 3] == 1.0 and pulse.sum() == 1.0
    k = degrade.KernelSpec("iso", 5, 13, sig_x=0.6, sig_y=0.6).array()
    assert k.shape == (13, 13) and np.all(k[:4] == 0) and np.all(k[:, 9:] == 0) and k[6, 6] == k.max()
    assert degrade.sinc_kernel(1.2, 11, 13).min() < 0
    with pytest.raises(ValueError, match="unknown blur kernel"):
        degrade.blur_kernel("skew", 5, 1.0)
    with pytest.raises(ValueError, match="must be odd"):
        degrade.blur_kernel("iso", 4, 1.0)


def test_the_preset_carries_the_yaml_numbers():
    conf = json.loads(str(GOLD["preset_json"]))
    opts = dataclasses.asdict(degrade.REALESRGAN_TESTING)
    assert sorted(conf) == sorted(opts)
    for k, v in conf.items():
        if k in ("gaussian_noise_prob", "gaussian_noise_prob2"):
            assert v == 0.5 and opts[k] == 1.0, k                     # the deviation: Poisson noise is not built
            continue
        assert (list(opts[k]) if isinstance(opts[k], tuple) else opts[k]) == v, k
    assert opts["sf"] == 4 and opts["blur_kernel_size"] == 13 and opts["blur_kernel_size2"] == 7 and opts["second_order_prob"] == 0.0


@pytest.mark.parametrize("case", R.INTERP_CASES, ids=str)
def test_interpolate_fp32_against_float64(case):
    """the reference's operator in its own precision against the definition: the measurement the GPU bound of rs_interp comes from"""
    mode, kind, v = case
    x = R.inputs((2, 3, *R.INTERP_SHAPE), R.INTERP_SEED)
    want = R.interpolate(x, mode=mode, **{kind: v})
    kw = {} if mode == "area" else dict(align_corners=False)
    got = F.interpolate(torch.from_numpy(x), mode=mode, **{kind: v}, **kw).numpy()
    assert got.shape == want.shape
    err = float(np.abs(got - want).max())
    print(f"F.interpolate {case}: |fp32 - float64| = {err:.2e}")
    _pinned("interp", err)
    assert err <= R.REF_ERR["interp"]
    if mode == "bicubic":   # the restated bicubic is F.interpolate's
        assert np.abs(R.bicubic(x, **{kind: v}) - want).max() <= 1e-13


def test_the_pinned_errors_are_what_was_measured():
    """each maximum over the measuring tests' cases lies in (REF_ERR / 2, REF_ERR], so the GPU bounds (five times REF_ERR) are between five
    and ten times the reference's own error"""
    MEASURED.clear()
    for case in R.FILTER_CASES:
        test_filter_restatement_against_the_recorded_reference(case)
    for case in R.JPEG_CASES:
        test_jpeg_restatement_and_closed_form_against_the_recorded_reference(case)
    for case in R.INTERP_CASES:
        test_interpolate_fp32_against_float64(case)
    for op, err in MEASURED.items():
        print(f"{op}: measured {err:.2e}, pinned {R.REF_ERR[op]:.1e}, GPU bound {R.TOL[op]:.1e}")
        assert R.REF_ERR[op] / 2 < err <= R.REF_ERR[op], op
        assert R.TOL[op] == 5 * R.REF_ERR[op]


# ---------------------------------------------------------------------------------------------------------------- mutations
def test_filter_mutations_move_a_pixel_beyond_the_bound():
    for case in R.GPU_FILTER_CASES:
        x, kernels = R.filter_case(case)
        want = R.filter2d(x, kernels)
        for name, kw in (("a flipped kernel", dict(flip=True)), ("an edge-repeating reflection", dict(repeat_edge=True))):
            moved = float(np.abs(R.filter2d(x, kernels, **kw) - want).max())
            print(f"{name} on {case[0]}: {moved:.2e} (bound {R.TOL['filter']:.1e})")
            symmetric = np.array_equal(kernels, kernels[:, ::-1, ::-1])
            if name == "a flipped kernel" and symmetric:
                continue                                              # (an iso or sinc kernel is its own flip)
            assert moved > 100 * R.TOL["filter"], (name, case[0])
    assert sum(not np.array_equal(R.filter_case(c)[1], R.filter_case(c)[1][:, ::-1, ::-1]) for c in R.GPU_FILTER_CASES) >= 3


def test_interpolate_mutations_move_a_pixel_beyond_the_bound():
    x = R.inputs((2, 3, *R.INTERP_SHAPE), R.INTERP_SEED)
    for _, kind, v in [c for c in R.INTERP_CASES if c[0] == "bicubic"]:
        moved = float(np.abs(R.bicubic(x, **{kind: v}, A=-0.5) - R.bicubic(x, **{kind: v})).max())
        print(f"cubic A = -0.5 at {kind} = {v}: {moved:.2e}")
        assert moved > 100 * R.TOL["interp"]
    for mode in ("bilinear", "bicubic"):
        for s in (0.73, 1.37):
            size = (R.out_size(R.INTERP_SHAPE[0], s), R.out_size(R.INTERP_SHAPE[1], s))
            moved = float(np.abs(R.interpolate(x, size=size, mode=mode) - R.interpolate(x, scale_factor=s, mode=mode)).max())
            print(f"coordinates from H / Ho where 1 / scale_factor is meant, {mode} at {s}: {moved:.2e}")
            assert moved > 100 * R.TOL["interp"]
    assert np.abs(R.bicubic(x, scale_factor=0.73, step_from_size=True) - R.interpolate(x, size=(17, 29), mode="bicubic")).max() <= 1e-13


def test_jpeg_mutations_move_a_pixel_beyond_the_bound():
    key, (Hh, W), qualities, seed = R.JPEG_CASES[0]
    x, want, _ = R.constructed_jpeg_case(Hh, W, qualities, seed)
    for name, kw in (("chroma not subsampled", dict(subsample=False)), ("the luma table used for chroma", dict(chroma_table=False))):
        moved = float(np.abs(R.jpeg(x, qualities, **kw) - want).max())
        print(f"{name} on {key}: {moved:.2e} (bound {R.TOL['jpeg']:.1e})")
        assert moved > 100 * R.TOL["jpeg"], name
    # padding: the natural images cropped to 40 x 56 (padded to 48 x 64); the pixels of MCUs that hold no padding do not move
    nat = R.natural_images(H.ROOT, crop=(40, 56))
    q = [70.0] * len(nat)
    a, b = R.jpeg(nat, q), R.jpeg(nat, q, replicate_pad=True)
    moved = float(np.abs(a - b).max())
    print(f"padding by replication on the cropped natural images: {moved:.2e}")
    assert moved > 100 * R.TOL["jpeg"] and np.array_equal(a[:, :, :32, :48], b[:, :, :32, :48])
    # rounding: an exact tie
    t = R.tie_image()
    even, coefs = R.jpeg(t, [R.TIE_QUALITY] * 2, return_coefficients=True)
    assert coefs[0][1][0, 0, 0, 0] == 22.5 and float(R.mcu_tie_distance(coefs[0]).min()) == 0.0
    near = sum(int((np.abs(np.abs(c - np.floor(c)) - 0.5) < 0.01).sum()) for c in coefs[0])
    assert near == coefs[0][1].shape[0] * coefs[0][1].shape[1]       # the designed tie of every MCU and no other coefficient near one
    moved = float(np.abs(R.jpeg(t, [R.TIE_QUALITY] * 2, half_away=True) - even).max())
    print(f"round half away from zero on the tie image: {moved:.2e}")
    assert moved > 100 * R.TOL["jpeg"]
    # and the final rounding: float32 products that are exact ties
    v = np.array([k + 0.5 for k in range(0, 255)], np.float32) / np.float32(255.0)
    ties = v[(v * np.float32(255.0)) % 1 == 0.5]
    assert len(ties) > 20
    u8 = R.unit_to_u8(ties.reshape(1, 1, 1, -1))[0, 0, :, 0]
    assert np.all(u8 % 2 == 0) and np.any(np.floor(ties * np.float32(255.0) + 0.5).astype(np.uint8) != u8)


# ---------------------------------------------------------------------------------------------------------------- plans
OPTS2 = dataclasses.replace(degrade.REALESRGAN_TESTING, second_order_prob=1.0, second_blur_prob=0.5, sinc_prob=0.5, final_sinc_prob=0.5,
                            kernel_prob=(1, 1, 1, 1, 1, 1), kernel_prob2=(1, 1, 1, 1, 1, 1))


def test_plans_are_deterministic_and_round_trip_through_json():
    for opts in (degrade.REALESRGAN_TESTING, OPTS2):
        for seed in range(6):
            p = degrade.draw_plan(opts, 3, 64, 48, seed)
            assert p == degrade.draw_plan(opts, 3, 64, 48, seed) and hash(p) == hash(degrade.draw_plan(opts, 3, 64, 48, seed))
            assert p != degrade.draw_plan(opts, 3, 64, 48, seed + 100)
            q = degrade.DegradePlan.from_json(p.to_json())
            assert q == p and isinstance(q.first.kernels[0], degrade.KernelSpec) and isinstance(q.jpeg1, tuple)
            assert all(np.array_equal(a.array(), b.array()) for a, b in zip(p.first.kernels + p.final_kernels, q.first.kernels + q.final_kernels))
            with pytest.raises(dataclasses.FrozenInstanceError):
                p.sf = 2
    assert degrade.draw_plan(degrade.REALESRGAN_TESTING, 1, 64, 48, 2 ** 64 + 5) == dataclasses.replace(degrade.draw_plan(degrade.REALESRGAN_TESTING, 1, 64, 48, 5), seed=2 ** 64 + 5)


def test_every_drawn_value_lies_inside_its_range():
    seen = {"second": 0, "blur2": 0, "sinc_first": 0, "sinc": 0, "pulse": 0, "modes": set(), "kinds": set(), "updown": set()}
    for seed in range(200):
        o = OPTS2 if seed % 2 else degrade.REALESRGAN_TESTING
        p = degrade.draw_plan(o, 2, 64, 48, seed)
        assert (p.B, p.H, p.W, p.sf, p.seed) == (2, 64, 48, 4, seed) and len(p.noise_seeds) == 2 and all(0 <= s < 2 ** 63 for s in p.noise_seeds)

        def stage(s, rr, nr, ksz, sizes, sig, bg, bp):
            assert s.mode in degrade.MODES and (min(rr[0], 1.0) <= s.scale <= rr[1])
            assert len(s.sigma) == len(s.gray) == 2 and all(nr[0] <= v <= nr[1] for v in s.sigma)
            for k in s.kernels or ():
                assert k.pad_to == ksz and k.size in sizes
                if k.kind == "sinc":
                    assert (math.pi / 3 if k.size < 13 else math.pi / 5) <= k.cutoff <= math.pi
                else:
                    assert k.kind in degrade.KERNEL_KINDS and sig[0] <= k.sig_x <= sig[1] and sig[0] <= k.sig_y <= sig[1] and -math.pi <= k.theta <= math.pi
                    lo, hi = bg if k.kind.startswith("generalized") else bp if k.kind.startswith("plateau") else (1.0, 1.0)
                    assert min(lo, 1.0) <= k.beta <= max(hi, 1.0)
                    if k.kind.endswith("_iso") or k.kind == "iso":
                        assert k.sig_y == k.sig_x and k.theta == 0.0
                assert k.array().shape == (ksz, ksz) and abs(float(k.array().sum(dtype=np.float64)) - 1) < 1e-5
                seen["kinds"].add(k.kind)
            seen["modes"].add(s.mode)
            seen["updown"].add("up" if s.scale > 1 else "down" if s.scale < 1 else "keep")

        stage(p.first, o.resize_range, o.noise_range, 13, range(3, 13, 2), o.blur_sigma, o.betag_range, o.betap_range)
        assert p.first.kernels is not None and len(p.first.kernels) == 2
        assert all(o.jpeg_range[0] <= q <= o.jpeg_range[1] for q in p.jpeg1)
        assert all(o.jpeg_range2[0] <= q < 100.0 and np.float32(q) < np.float32(100.0) for q in p.jpeg2)
        if p.second is not None:
            seen["second"] += 1
            seen["blur2"] += p.second.kernels is not None
            stage(p.second, o.resize_range2, o.noise_range2, 7, (3, 5), o.blur_sigma2, o.betag_range2, o.betap_range2)
            assert p.second_size() == (int(16 * p.second.scale), int(12 * p.second.scale))
        else:
            assert o is degrade.REALESRGAN_TESTING                    # second_order_prob is 0 there
        assert p.final_mode in degrade.MODES and len(p.final_kernels) == 2
        for k in p.final_kernels:
            assert k.pad_to == 7 and (k.kind == "pulse" or (k.kind == "sinc" and k.size in (3, 5) and math.pi / 3 <= k.cutoff <= math.pi))
            seen["sinc" if k.kind == "sinc" else "pulse"] += 1
        seen["sinc_first"] += p.sinc_first
        names = p.stages()
        assert names[:4] == ["blur1", "resize1", "noise1", "jpeg1"] and names[-1] == "round" and ("blur2" in names) == (p.second is not None and p.second.kernels is not None)
        assert names.index("resize3") + 1 == names.index("sinc") and (names.index("jpeg2") > names.index("sinc")) == p.sinc_first
    assert seen["second"] == 100 and 20 < seen["blur2"] < 80 and 60 < seen["sinc_first"] < 140 and seen["sinc"] > 30 and seen["pulse"] > 100
    assert seen["modes"] == set(degrade.MODES) and seen["updown"] == {"up", "down", "keep"} and seen["kinds"] == set(degrade.KERNEL_KINDS) | {"sinc"}


def test_draw_plan_rejects_what_is_not_built():
    o = degrade.REALESRGAN_TESTING
    for name in ("gaussian_noise_prob", "gaussian_noise_prob2"):
        with pytest.raises(ValueError, match=f"{name} = 0.5 asks for Poisson noise"):
            degrade.draw_plan(dataclasses.replace(o, **{name: 0.5}), 1, 64, 48, 0)
    with pytest.raises(ValueError, match="no multiple of sf"):
        degrade.draw_plan(o, 1, 66, 48, 0)
    with pytest.raises(ValueError, match="too small for the blur kernels"):
        degrade.draw_plan(o, 1, 12, 48, 0)
    with pytest.raises(ValueError, match="must be positive"):
        degrade.draw_plan(o, 0, 64, 48, 0)
    p = degrade.draw_plan(o, 1, 64, 48, 0)
    with pytest.raises(ValueError, match="the plan is for"):
        degrade.Degrader.run(degrade.Degrader.__new__(degrade.Degrader), torch.zeros(1, 3, 32, 48), p)


def test_make_testset_names_the_file_whose_side_is_no_multiple_of_sf(tmp_path, monkeypatch):
    from PIL import Image

    monkeypatch.setattr(degrade, "Degrader", lambda *a: pytest.fail("nothing is degraded before every file is checked"))
    Image.fromarray(np.zeros((64, 48, 3), np.uint8)).save(tmp_path / "a.png")
    Image.fromarray(np.zeros((64, 50, 3), np.uint8)).save(tmp_path / "b.png")
    with pytest.raises(ValueError, match=r"b\.png: 64 x 50 is no multiple of sf = 4"):
        degrade.make_testset(tmp_path, tmp_path / "lq")
    assert not (tmp_path / "lq").exists()
    assert [p.name for p in degrade.list_images(tmp_path)] == ["a.png", "b.png"] and degrade.list_images(tmp_path / "a.png") == [tmp_path / "a.png"]


# ---------------------------------------------------------------------------------------------------------------- C ABI
PTR, FAR, KPTR = 0x100000, 0x40000000, 0x70000000   # never dereferenced: every call below is refused before anything is launched

FILTER_ERRORS = {
    "null_in": (dict(inp=None), "null tensor"), "null_kernels": (dict(kern=None), "null tensor"), "null_out": (dict(out=None), "null tensor"),
    "batch": (dict(B=0), "must be positive"), "width": (dict(W=-1), "must be positive"),
    "even_k": (dict(k=4), "k must be odd and at most 21"), "large_k": (dict(k=23), "k must be odd and at most 21"), "zero_k": (dict(k=0), "k must be odd"),
    "deep_reflection": (dict(H=10, k=21), "below min(H, W)"), "kernel_count": (dict(Bk=3), "Bk must be 1"),
    "clamp": (dict(clamp=2), "clamp must be 0 or 1"), "in_place": (dict(out=PTR), "overlaps"),
}


@pytest.mark.parametrize("name", sorted(FILTER_ERRORS))
def test_filter2d_argument_errors(lib, name):
    kw, text = FILTER_ERRORS[name]
    a = dict(inp=PTR, kern=KPTR, out=FAR, B=2, C=3, H=40, W=52, k=13, Bk=2, clamp=0)
    a.update(kw)
    rc = lib.rs_filter2d(a["inp"], a["kern"], a["out"], a["B"], a["C"], a["H"], a["W"], a["k"], a["Bk"], a["clamp"], None)
    assert rc == -2 and text in _lib.last_error() and _lib.last_error().startswith("rs_filter2d: "), (rc, _lib.last_error())


INTERP_ERRORS = {
    "null_in": (dict(inp=None), "null tensor"), "null_out": (dict(out=None), "null tensor"), "height": (dict(H=0), "must be positive"),
    "out_width": (dict(Wo=0), "must be positive"), "mode": (dict(mode=3), "mode must be"), "clamp": (dict(clamp=-1), "clamp must be 0 or 1"),
    "one_scale": (dict(sw=0.0), "both 0"), "scale_small": (dict(sh=0.1, sw=0.1, Ho=4, Wo=5), "must lie in [1/8, 8]"),
    "scale_nan": (dict(sh=float("nan")), "must lie in [1/8, 8]"), "scale_large": (dict(sh=8.5, sw=8.5), "must lie in [1/8, 8]"),
    "size_small": (dict(sh=0.0, sw=0.0, Ho=4), "must lie in [1/8, 8]"), "size_large": (dict(sh=0.0, sw=0.0, Wo=417), "must lie in [1/8, 8]"),
    "not_the_floor": (dict(Ho=21), "floor(H * scale_h)"), "in_place": (dict(out=PTR), "overlaps"),
}


@pytest.mark.parametrize("name", sorted(INTERP_ERRORS))
def test_interp_argument_errors(lib, name):
    kw, text = INTERP_ERRORS[name]
    a = dict(inp=PTR, out=FAR, B=2, C=3, H=40, W=52, Ho=20, Wo=26, sh=0.5, sw=0.5, mode=2, clamp=0)
    a.update(kw)
    rc = lib.rs_interp(a["inp"], a["out"], a["B"], a["C"], a["H"], a["W"], a["Ho"], a["Wo"], a["sh"], a["sw"], a["mode"], a["clamp"], None)
    assert rc == -2 and text in _lib.last_error() and _lib.last_error().startswith("rs_interp: "), (rc, _lib.last_error())


JPEG_ERRORS = {
    "null_in": (dict(inp=None), "null pointer"), "null_quality": (dict(q=None), "null pointer"), "batch": (dict(B=0), "B must be 1 .. RS_MAX_ROWS"),
    "large_batch": (dict(B=65), "B must be 1 .. RS_MAX_ROWS"), "channels": (dict(C=1), "C must be 3"), "height": (dict(H=0), "must be positive"),
    "quality_100": (dict(q=[50.0, 100.0]), "must lie in (0, 100)"), "quality_0": (dict(q=[0.0, 50.0]), "must lie in (0, 100)"),
    "quality_nan": (dict(q=[float("nan"), 50.0]), "must lie in (0, 100)"), "partial_overlap": (dict(out=PTR + 64), "partly overlaps"),
}


@pytest.mark.parametrize("name", sorted(JPEG_ERRORS))
def test_jpeg_argument_errors(lib, name):
    kw, text = JPEG_ERRORS[name]
    a = dict(inp=PTR, out=FAR, q=[30.0, 70.0], B=2, C=3, H=40, W=52)
    a.update(kw)
    q = (C.c_float * 65)(*a["q"]) if a["q"] is not None else None
    rc = lib.rs_jpeg(a["inp"], a["out"], q, a["B"], a["C"], a["H"], a["W"], None)
    assert rc == -2 and text in _lib.last_error() and _lib.last_error().startswith("rs_jpeg: "), (rc, _lib.last_error())


NOISE_ERRORS = {
    "null_x": (dict(x=None), "null pointer"), "null_keys": (dict(keys=None), "null keys"), "null_sigma": (dict(sigma=None), "null pointer"),
    "batch": (dict(B=0), "B must be 1 .. RS_MAX_ROWS"), "large_batch": (dict(B=65), "B must be 1 .. RS_MAX_ROWS"), "channels": (dict(C=0), "must be positive"),
    "reserved": (dict(reserved=1), "reserved field"), "draw": (dict(draw=[0, -1]), "negative draw index"), "sigma": (dict(sigma=[1.0, -2.0]), "finite and not negative"),
    "sigma_nan": (dict(sigma=[float("nan"), 1.0]), "finite and not negative"), "gray": (dict(gray=[0, 2]), "gray flag"), "clamp": (dict(clamp=3), "clamp must be 0 or 1"),
    "partial_overlap": (dict(out=PTR + 16), "partly overlaps"),
}


@pytest.mark.parametrize("name", sorted(NOISE_ERRORS))
def test_add_noise_argument_errors(lib, name):
    kw, text = NOISE_ERRORS[name]
    a = dict(x=PTR, out=FAR, keys=[(1, 0), (2, 0)], draw=[0, 1], sigma=[3.0, 4.0], gray=[0, 1], B=2, C=3, H=40, W=52, clamp=1, reserved=0)
    a.update(kw)
    keys = None
    if a["keys"] is not None:
        keys = (_lib.NoiseKey * 65)()
        for d, (s, st) in zip(keys, a["keys"]):
            d.seed, d.stream = s, st
        keys[1].reserved = a["reserved"]
    arr = lambda t, v: (t * 65)(*v) if v is not None else None
    rc = lib.rs_add_noise(a["x"], a["out"], keys, arr(C.c_int, a["draw"]), arr(C.c_float, a["sigma"]), arr(C.c_int, a["gray"]), a["B"], a["C"],
                          a["H"], a["W"], a["clamp"], None)
    assert rc == -2 and text in _lib.last_error() and _lib.last_error().startswith("rs_add_noise: "), (rc, _lib.last_error())


@pytest.mark.parametrize("kw,text", [(dict(src=None), "null tensor"), (dict(dst=None), "null tensor"), (dict(B=0), "must be positive"), (dict(W=-2), "must be positive")], ids=str)
def test_unit_to_u8_argument_errors(lib, kw, text):
    a = dict(src=PTR, dst=FAR, B=2, C=3, H=40, W=52)
    a.update(kw)
    rc = lib.rs_unit_to_u8(a["src"], a["dst"], a["B"], a["C"], a["H"], a["W"], None)
    assert rc == -2 and text in _lib.last_error() and _lib.last_error().startswith("rs_unit_to_u8: "), (rc, _lib.last_error())


def test_the_header_declares_what_the_signatures_bind(lib):
    header = open(H.ROOT + "/include/resshift_hip.h").read()
    ctype = {"int": C.c_int, "double": C.c_double, "void*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p,
             "const rs_noise_key*": C.POINTER(_lib.NoiseKey), "const int*": C.POINTER(C.c_int)}
    host_arrays = {("rs_jpeg", "quality"): C.POINTER(C.c_float), ("rs_add_noise", "sigma"): C.POINTER(C.c_float)}
    for name in ("rs_filter2d", "rs_interp", "rs_jpeg", "rs_add_noise", "rs_unit_to_u8"):
        m = re.search(r"\nint " + name + r"\(([^;]*)\);", header)
        assert m, name
        args, want, last = [a.strip() for a in " ".join(m.group(1).split()).split(",")], [], None
        for a in args:   # "int B" / "int C" / "const float* in": a bare name takes the previous type
            t, _, n = a.rpartition(" ")
            last = t or last
            want.append(host_arrays.get((name, n), ctype[t or last]))
        res, got = _lib.SIGNATURES[name]
        assert res is C.c_int and got == want, (name, got, want)
        assert hasattr(lib, name)
    for text in ("A CROSS-CORRELATION - the kernel is not flipped", "refl(q, n) = |q| for q < n, 2 (n - 1) - q otherwise", "A = -0.75",
                 "src(i) = step * (i + 0.5) - 0.5", "[floor(i H / Ho), ceil((i + 1) H / Ho))", "factor = (q < 50 ? 5000 / q : 200 - 2 q) / 100",
                 "ties to even", "tests/_degrade_ref.py", "#define RS_INTERP_BICUBIC 2"):
        assert text in header, text
    assert "degrade.hip" in build.SOURCES and _lib.INTERP_MODES == {"area": 0, "bilinear": 1, "bicubic": 2} and _lib.FILTER_KMAX == 21


def test_lib_wrappers_reject_bad_arguments_before_the_library_is_called(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was reached"))
    x = torch.zeros(2, 3, 24, 40)
    d = x.as_subclass(_OnDevice)
    k = torch.zeros(1, 7, 7).as_subclass(_OnDevice)
    for fn, args in ((_lib.filter2d, (x, k)), (_lib.interpolate, (x,)), (_lib.jpeg, (x, 50)), (_lib.add_noise, (x, [1, 2], 3.0)), (_lib.unit_to_u8, (x,))):
        with pytest.raises(ValueError, match="contiguous float32 device tensor"):
            fn(*args)                                                  # a host tensor: there is no CPU arithmetic to fall back to
    with pytest.raises(ValueError, match="kernels .* must be a contiguous float32 tensor"):
        _lib.filter2d(d, torch.zeros(1, 7, 7))
    for bad, text in ((torch.zeros(1, 4, 4), "k must be odd"), (torch.zeros(1, 23, 23), "k must be odd and at most 21"), (torch.zeros(3, 7, 7), "3 kernels for 2 images")):
        with pytest.raises(ValueError, match=text):
            _lib.filter2d(d, bad.as_subclass(_OnDevice))
    with pytest.raises(ValueError, match="below min"):
        _lib.filter2d(torch.zeros(1, 3, 3, 40).as_subclass(_OnDevice), k)
    for kw in (dict(), dict(scale_factor=0.5, size=(12, 20))):
        with pytest.raises(ValueError, match="exactly one of scale_factor and size"):
            _lib.interpolate(d, **kw)
    with pytest.raises(ValueError, match="unknown mode"):
        _lib.interpolate(d, scale_factor=0.5, mode="nearest")
    for bad in (0, -1.0, "2", True, float("nan")):
        with pytest.raises(ValueError, match="scale_factor must be a positive number"):
            _lib.interpolate(d, scale_factor=bad)
    for bad in ((12,), (12.0, 20), (0, 20), 12):
        with pytest.raises(ValueError, match="size must be two positive integers"):
            _lib.interpolate(d, size=bad)
    for kw in (dict(scale_factor=0.12), dict(scale_factor=8.5), dict(size=(2, 20)), dict(size=(12, 321))):
        with pytest.raises(ValueError, match=r"must lie in \[1/8, 8\]"):
            _lib.interpolate(d, **kw)
    assert _lib.interp_size(24, 0.73) == 17 and _lib.interp_size(40, 1.37) == 54 and R.out_size(40, 0.73) == 29
    with pytest.raises(ValueError, match="C must be 3"):
        _lib.jpeg(torch.zeros(1, 1, 16, 16).as_subclass(_OnDevice), 50)
    for bad in (0, 100, [50, 101], float("nan")):
        with pytest.raises(ValueError, match=r"must lie in \(0, 100\)"):
            _lib.jpeg(d, bad)
    with pytest.raises(ValueError, match="2 images but 3 qualities"):
        _lib.jpeg(d, [50, 60, 70])
    with pytest.raises(ValueError, match="2 images but 1 keys"):
        _lib.add_noise(d, [1], 3.0)
    with pytest.raises(ValueError, match="finite and not negative"):
        _lib.add_noise(d, [1, 2], [-1.0, 2.0])
    with pytest.raises(ValueError, match="negative draw index"):
        _lib.add_noise(d, [1, 2], 2.0, draw=-1)

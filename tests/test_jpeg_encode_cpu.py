"""JPEG files without a GPU: the numpy restatement of libjpeg's baseline encoder against the recorded and the live Pillow on
every byte, the mutations the recorded files catch, the pinned header, the decoder's view of the files, every argument error of
rs_jpeg_encode and its two size queries through the built library, the wrappers on a fake device, `inference(out_ext=)` and the
degradation command line."""
import ctypes as C
import io
import re

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401  (puts the repository root on sys.path)
import _jpeg_enc_ref as E
import _jpeg_ref as J
from _fakes import InstantPool, _OnDevice, lib  # noqa: F401  (fixture)
from resshift_amd import _lib, build, degrade
from resshift_amd.sampler import ResShiftSampler


@pytest.fixture(scope="module")
def files():
    return np.load(H.ROOT + "/tests/golden/libjpeg_files.npz")


@pytest.fixture(scope="module")
def roundtrip():
    return np.load(H.ROOT + "/tests/golden/libjpeg_roundtrip.npz")


def _versions(files):
    import PIL
    from PIL import features

    return f"Pillow {PIL.__version__}, libjpeg {features.version('jpg')}", f"Pillow {files['pillow']}, libjpeg {files['libjpeg']}"


# ---------------------------------------------------------------------------------------------------------------- the definition
def test_the_restatement_equals_the_recorded_files_on_every_byte(files, roundtrip):
    total = 0
    for key, (Hh, W), kind, seed, q in J.cases():
        u8 = J.to_u8(J.content(kind, Hh, W, seed))
        assert np.array_equal(u8, roundtrip["in_" + key]) and int(roundtrip["q_" + key]) == q, key      # the inputs of the round-trip fixture
        want = files["file_" + key].tobytes()
        assert E.encode(u8, q) == want, key
        assert len(want) <= E.bound(Hh, W)
        total += len(want)
    assert len(J.cases()) == 50 and total == 86411
    assert str(files["pillow"]) == str(roundtrip["pillow"]) and str(files["libjpeg"]) == str(roundtrip["libjpeg"])


def test_the_cases_recorded_by_length_and_digest(files):
    import hashlib

    assert [c[0] for c in E.extra_cases()] == ["8x8_random_s0_q100", "8x8_random_s1_q95", "8x8_random_s2_q95", "8x8_random_s2_q100", "273x289_random", "273x289_smooth"]
    for key, (Hh, W), kind, seed, q in E.extra_cases():
        data = E.encode(J.to_u8(J.content(kind, Hh, W, seed)), q)
        assert len(data) == int(files["len_" + key]) and hashlib.sha256(data).hexdigest() == str(files["sha_" + key]), key
        if (Hh, W) == (8, 8):
            assert data[-4:] == b"\xff\x00\xff\xd9", key                                                 # the padded last byte is 0xFF: stuffed


def test_the_restatement_equals_the_live_pillow(files):
    """skips - printing both version strings - only where the live Pillow disagrees with the fixture's OWN files: another libjpeg build"""
    live, recorded = _versions(files)
    for key, (Hh, W), kind, seed, q in J.cases():
        if E.pillow_file(J.to_u8(J.content(kind, Hh, W, seed)), q) != files["file_" + key].tobytes():
            pytest.skip(f"the live {live} does not reproduce the files recorded with {recorded} on {key}: another libjpeg build")
    rng = np.random.default_rng(4)
    for Hh, W in [(8, 8), (13, 21), (32, 5 + 16), (33, 47), (1, 1), (7, 100)]:
        u8 = rng.integers(0, 256, (Hh, W, 3), dtype=np.uint8)
        q = int(rng.integers(1, 101))
        assert E.encode(u8, q) == E.pillow_file(u8, q), (Hh, W, q, live)


@pytest.mark.parametrize("mut", E.MUTATIONS)
def test_the_recorded_files_catch_the_mutation(files, mut):
    caught = [key for key, (Hh, W), kind, seed, q in J.cases() if E.encode(J.to_u8(J.content(kind, Hh, W, seed)), q, mut) != files["file_" + key].tobytes()]
    print(f"{mut}: moves bytes in {len(caught)} of {len(J.cases())} recorded files")
    assert len(caught) >= 5, (mut, caught)


def test_dummy_blocks_and_the_dc_predictor():
    """9 x 8 is one MCU with three dummy Y blocks: each repeats the DC of the block before it and has no AC; the chroma blocks are real"""
    u8 = J.to_u8(J.content("random", 9, 8, 1))
    blocks = E.scan_blocks(u8, 95)
    assert [c for c, _ in blocks] == [0, 0, 0, 0, 1, 2]
    y00, y01, y10, y11 = (b for _, b in blocks[:4])
    assert np.any(y00[1:] != 0) and np.any(y10[1:] != 0)                                # the 9th row makes Y10 a real block
    assert not np.any(y01[1:]) and y01[0] == y00[0] and not np.any(y11[1:]) and y11[0] == y10[0]
    y = [b for _, b in E.scan_blocks(J.to_u8(J.content("random", 8, 8, 1)), 95)[:4]]
    assert all(b[0] == y[0][0] and not np.any(b[1:]) for b in y[1:])                    # 8 x 8: Y01, Y10 and Y11 all repeat Y00
    real = E.scan_blocks(u8, 95, "real_dct_in_dummies")
    assert np.any(real[1][1][1:] != 0) or real[1][1][0] != y00[0]                       # the replicated pixels have a DCT of their own


def test_the_header_is_pinned(files):
    h = E.header(31, 50, 95)
    assert len(h) == E.SCAN_OFFSET == 623 and files["file_31x50_binary"].tobytes()[:623] == h
    assert h[:20] == b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    assert h[20:25] == b"\xff\xdb\x00\x43\x00" and h[89:94] == b"\xff\xdb\x00\x43\x01"
    assert list(h[25:89]) == [int(v) for v in J.quant_table(J.LUMA, 95).reshape(64)[E.ZIGZAG]] and h[25:28] == bytes([2, 1, 1])
    assert list(h[94:158]) == [int(v) for v in J.quant_table(J.CHROMA, 95).reshape(64)[E.ZIGZAG]]
    assert h[158:177] == b"\xff\xc0\x00\x11\x08\x00\x1f\x00\x32\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01"
    assert [(m.start(), h[m.start() + 4]) for m in re.finditer(b"\xff\xc4", h)] == [(177, 0x00), (210, 0x10), (393, 0x01), (426, 0x11)]
    assert h[609:] == b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    big = E.header(65535, 258, 1)
    assert big[163:167] == b"\xff\xff\x01\x02" and set(big[25:89]) == {255}
    diff = [i for i in range(623) if h[i] != big[i]]
    assert all(25 <= i < 89 or 94 <= i < 158 or 163 <= i < 167 for i in diff)           # only the DQT payloads and the SOF0 size move
    assert E.MAX_BLOCK_BITS == 1660
    assert max(n + s for s, (_, n) in E.DC_CODES[1].items()) == 22 and max(n + (s & 15) for t in E.AC_CODES for s, (_, n) in t.items()) == 26
    assert all(len(t) == 162 for t in E.AC_CODES) and all(len(t) == 12 for t in E.DC_CODES)


def test_pillow_decodes_the_restatements_files_to_the_round_trip(files, roundtrip):
    from PIL import Image

    live, recorded = _versions(files)
    for key, _, _, _, q in J.cases():
        u8 = roundtrip["in_" + key]
        dec = np.asarray(Image.open(io.BytesIO(E.encode(u8, q))).convert("RGB"))
        if not np.array_equal(dec, roundtrip["out_" + key]):
            if not np.array_equal(J.pillow_roundtrip(u8, q), roundtrip["out_" + key]):
                pytest.skip(f"the live {live} does not decode like the {recorded} of the fixture on {key}: another libjpeg build")
            pytest.fail(f"{key}: the restatement's file decodes to another image than libjpeg's")
        assert np.array_equal(dec, J.roundtrip(u8, q)), key


# ---------------------------------------------------------------------------------------------------------------- C ABI
IN, OUT, NB, WS = 0x100000, 0x40000000, 0x7000000, 0x80000000   # never dereferenced: every call below is refused before anything is launched
NULLS = "rs_jpeg_encode: null pointer (in / out / nbytes / quality / workspace)"
OVERLAP = "rs_jpeg_encode: in, out, nbytes and workspace must not overlap"

ENCODE_ERRORS = {
    "null_in": (dict(inp=None), NULLS), "null_out": (dict(out=None), NULLS), "null_nbytes": (dict(nb=None), NULLS), "null_quality": (dict(q=None), NULLS),
    "null_workspace": (dict(ws=None), NULLS),
    "batch": (dict(B=0), "rs_jpeg_encode: B must be 1 .. RS_MAX_ROWS (the qualities travel by value)"),
    "large_batch": (dict(B=65), "rs_jpeg_encode: B must be 1 .. RS_MAX_ROWS (the qualities travel by value)"),
    "channels_1": (dict(C=1), "rs_jpeg_encode: C must be 3 (RGB)"), "channels_4": (dict(C=4), "rs_jpeg_encode: C must be 3 (RGB)"),
    "height": (dict(H=7), "rs_jpeg_encode: H and W must be at least 8"), "width": (dict(W=0), "rs_jpeg_encode: H and W must be at least 8"),
    "tall": (dict(H=65536, pitch=1 << 40), "rs_jpeg_encode: H and W must be at most 65535 (the SOF0 fields)"),
    "wide": (dict(W=65536, pitch=1 << 40), "rs_jpeg_encode: H and W must be at most 65535 (the SOF0 fields)"),
    "megapixels": (dict(H=8000, W=8000, pitch=1 << 40), "rs_jpeg_encode: the image is too large (the stuffing pass scans two levels of 2048: about 55 megapixels)"),
    "quality_0": (dict(q=[50, 0]), "rs_jpeg_encode: every quality must be an integer in 1 .. 100"),
    "quality_101": (dict(q=[101, 50]), "rs_jpeg_encode: every quality must be an integer in 1 .. 100"),
    "pitch": (dict(pitch=E.bound(40, 52) - 1), "rs_jpeg_encode: out_pitch is below rs_jpeg_encode_bound(H, W)"),
    "alignment": (dict(ws=WS + 8), "rs_jpeg_encode: workspace must be 16-byte aligned"),
    "out_is_in": (dict(out=IN), OVERLAP), "workspace_in_out": (dict(ws=OUT + 4096), OVERLAP), "nbytes_in_workspace": (dict(nb=WS + 64), OVERLAP),
    "in_in_workspace": (dict(inp=WS + 1024), OVERLAP),
}


@pytest.mark.parametrize("name", sorted(ENCODE_ERRORS))
def test_jpeg_encode_argument_errors(lib, name):
    kw, text = ENCODE_ERRORS[name]
    a = dict(inp=IN, out=OUT, nb=NB, q=[30, 70], ws=WS, B=2, C=3, H=40, W=52, pitch=E.bound(40, 52))
    a.update(kw)
    q = (C.c_int * 65)(*a["q"]) if a["q"] is not None else None
    rc = lib.rs_jpeg_encode(a["inp"], a["out"], a["nb"], q, a["ws"], a["B"], a["C"], a["H"], a["W"], a["pitch"], None)
    assert rc == -2 and _lib.last_error() == text, (rc, _lib.last_error())


def test_the_size_queries(lib, files):
    for key, (Hh, W), *_ in J.cases():
        assert lib.rs_jpeg_encode_bound(Hh, W) == E.bound(Hh, W) >= len(files["file_" + key])
    assert lib.rs_jpeg_encode_bound(8, 8) == 623 + 2 * ((6 * 1660 + 7) // 8) + 2 == 3115
    sides = [8, 9, 16, 17, 31, 32, 33, 255, 256, 257, 1000, 4095, 7000]
    for query in (lib.rs_jpeg_encode_bound, lambda h, w: lib.rs_jpeg_encode_workspace(1, h, w), lambda h, w: lib.rs_jpeg_encode_workspace(64, h, w)):
        table = np.array([[query(h, w) for w in sides] for h in sides], dtype=np.float64)
        assert np.all(table > 0) and np.all(np.diff(table, axis=0) >= 0) and np.all(np.diff(table, axis=1) >= 0)      # monotone in H and in W
        assert table[0, 0] < table[-1, -1]
    assert lib.rs_jpeg_encode_workspace(2, 40, 52) > lib.rs_jpeg_encode_workspace(1, 40, 52) >= 6 * 3 * 4 * (128 + 1660 // 8)
    assert lib.rs_jpeg_encode_bound(65535, 65535) > 2 ** 32                                                        # size_t, not int
    for bad in ((7, 8), (8, 7), (65536, 8), (8, 65536), (0, 0), (-1, 64)):
        assert lib.rs_jpeg_encode_bound(*bad) == 0 and lib.rs_jpeg_encode_workspace(1, *bad) == 0
    assert lib.rs_jpeg_encode_workspace(0, 64, 64) == 0 and lib.rs_jpeg_encode_workspace(65, 64, 64) == 0
    assert lib.rs_jpeg_encode_workspace(1, 8000, 8000) == 0 and lib.rs_jpeg_encode_workspace(1, 7000, 7000) > 0      # the two-level scan's limit


def test_the_header_declares_what_the_signatures_bind(lib):
    header = open(H.ROOT + "/include/resshift_hip.h").read()
    ctype = {"int": C.c_int, "void*": C.c_void_p, "const void*": C.c_void_p, "int*": C.c_void_p, "const int*": C.POINTER(C.c_int), "size_t": C.c_size_t}
    for name, res in (("rs_jpeg_encode", "int"), ("rs_jpeg_encode_bound", "size_t"), ("rs_jpeg_encode_workspace", "size_t")):
        m = re.search(r"\n" + res + " " + name + r"\(([^;]*)\);", header)
        assert m, name
        want, last = [], None
        for a in [a.strip() for a in " ".join(m.group(1).split()).split(",")]:   # "int B" / "int C": a bare name takes the previous type
            t, _, n = a.rpartition(" ")
            last = t or last
            want.append(ctype[t or last])
        got_res, got = _lib.SIGNATURES[name]
        assert got_res is ctype[res] and got == want, (name, got, want)
        assert hasattr(lib, name)
    for text in ("DUMMY blocks (jccoefct.c compress_data)", "v + 2^n - 1", "padded with 1-bits", "followed by 0x00", "22 + 63 * 26 = 1660", "offset 623",
                 "tests/_jpeg_enc_ref.py", "NO byte at or beyond nbytes[b]", "no kernel waits for another workgroup"):
        assert text in header, text
    assert "jpeg_encode.hip" in build.SOURCES and "jpeg_common.h" in build.HEADERS
    codec, encode = (open(f"{H.ROOT}/resshift_amd/csrc/jpeg_{n}.hip").read() for n in ("codec", "encode"))
    for src in (codec, encode):                       # one forward path: both files take it from the header and define none of it
        assert '#include "jpeg_common.h"' in src and "jc_forward_block(" in src and "jc_quad(" in src and "void jc_fdct8" not in src and "JC_BASE[2][64]" not in src
    assert "asm" not in encode


# ---------------------------------------------------------------------------------------------------------------- wrappers
def test_the_wrapper_rejects_bad_arguments_before_the_library_is_called(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was reached"))
    u8 = torch.zeros(2, 64, 80, 3, dtype=torch.uint8)
    d = u8.as_subclass(_OnDevice)
    for bad in (u8, torch.zeros(2, 3, 64, 80), d.to(torch.int16).as_subclass(_OnDevice), d[0], d[:, :, ::2], None):
        with pytest.raises(ValueError, match="x must be a contiguous device tensor, uint8 .B,H,W,3. or float32 .B,3,H,W. in .0,1."):
            _lib.jpeg_encode(bad, 50)                                  # a host tensor: there is no CPU arithmetic to fall back to
    with pytest.raises(ValueError, match="C must be 3"):
        _lib.jpeg_encode(torch.zeros(1, 16, 16, 1, dtype=torch.uint8).as_subclass(_OnDevice), 50)
    with pytest.raises(ValueError, match="C must be 3"):
        _lib.jpeg_encode(torch.zeros(1, 1, 16, 16).as_subclass(_OnDevice), 50)
    with pytest.raises(ValueError, match="an empty batch"):
        _lib.jpeg_encode(d[:0], 50)
    with pytest.raises(ValueError, match="H and W must lie in 8 .. 65535, not 7 x 16"):
        _lib.jpeg_encode(torch.zeros(1, 7, 16, 3, dtype=torch.uint8).as_subclass(_OnDevice), 50)
    with pytest.raises(ValueError, match="H and W must lie in 8 .. 65535, not 16 x 7"):
        _lib.jpeg_encode(torch.zeros(1, 3, 16, 7).as_subclass(_OnDevice), 50)
    for bad in (0, 101, 50.0, True, [50, 50.5], float("nan")):
        with pytest.raises(ValueError, match=r"jpeg_encode: every quality must be an integer in 1 \.\. 100"):
            _lib.jpeg_encode(d, bad)
    with pytest.raises(ValueError, match="2 images but 3 qualities"):
        _lib.jpeg_encode(d, [50, 60, 70])
    assert _lib.JPEG_ENCODE_MAX == 65535 and _lib.JPEG_CODEC_MIN == 8


class _FileEngine:
    """u8_to_input / output_to_u8 of the plumbing tests (the "sample" is the input itself) and jpeg_encode as the restatement"""

    def __init__(self):
        self.encoded = []

    def u8_to_input(self, t):
        return t.permute(0, 3, 1, 2).float()

    def output_to_u8(self, sr, lq=None, mask=None):
        return sr.permute(0, 2, 3, 1).to(torch.uint8)

    def jpeg_encode(self, u8, quality):
        assert u8.dtype == torch.uint8 and u8.dim() == 4 and u8.shape[3] == 3
        self.encoded.append((tuple(u8.shape), quality))
        return [E.encode(im.numpy(), quality) for im in u8]


def _stub_sampler(out_ch=3):
    s = ResShiftSampler.__new__(ResShiftSampler)
    s.seed, s.rank, s.num_gpus, s.device, s.engine, s.chop_size, s.sf = 7, 0, 1, torch.device("cpu"), _FileEngine(), 128, 1
    s.configs = {"autoencoder": {"params": {"ddconfig": {"out_ch": out_ch}}}}
    s.sample_tiled = lambda lq, mask=None, noise_repeat=False, tile_noises=None, seed=None: lq
    return s


def _folder(tmp_path):
    from PIL import Image

    src = tmp_path / "in"
    src.mkdir()
    ims = {n: J.to_u8(J.content(kind, 24, 40, i)) for i, (n, kind) in enumerate((("b", "smooth"), ("a", "random")))}
    for n, im in ims.items():
        Image.fromarray(im).save(src / f"{n}.png")
    return src, ims


@pytest.mark.parametrize("pool", [False, True])
def test_inference_writes_jpeg_files_of_the_uint8_tensor(tmp_path, monkeypatch, pool):
    from resshift_amd import tilepool

    monkeypatch.setattr(tilepool, "TilePool", InstantPool)   # completes every image at the next step: the "sample" is the input
    src, ims = _folder(tmp_path)
    s = _stub_sampler()
    assert s.inference(src, tmp_path / "out", bs=2, pool=pool, out_ext="jpg", jpeg_quality=80) is None
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["a.jpg", "b.jpg"]
    for n, im in ims.items():
        assert (tmp_path / "out" / f"{n}.jpg").read_bytes() == E.encode(im, 80)
    assert sum(e[0][0] for e in s.engine.encoded) == 2 and all(e[1] == 80 for e in s.engine.encoded)
    s2 = _stub_sampler()
    s2.inference(src, tmp_path / "dflt", bs=2, pool=pool, out_ext="jpg")
    assert all(e[1] == 95 for e in s2.engine.encoded)
    s3 = _stub_sampler()
    del s3.configs                                            # the default never asks for the channel count, the encoder is never called
    s3.inference(src, tmp_path / "png", bs=2, pool=pool)
    assert sorted(p.name for p in (tmp_path / "png").iterdir()) == ["a.png", "b.png"] and s3.engine.encoded == []


def test_inference_checks_the_file_options_before_anything_is_sampled(tmp_path):
    src, _ = _folder(tmp_path)
    s = _stub_sampler()
    s.sample_tiled = lambda *a, **kw: pytest.fail("something was sampled")
    for bad in ("bmp", "jpeg", "JPG", None, ".jpg"):
        with pytest.raises(ValueError, match="out_ext must be 'png' or 'jpg'"):
            s.inference(src, tmp_path / "out", out_ext=bad)
    for bad in (0, 101, 95.0, True, None, "95"):
        with pytest.raises(ValueError, match=r"jpeg_quality must be an integer in 1 \.\. 100"):
            s.inference(src, tmp_path / "out", out_ext="jpg", jpeg_quality=bad)
    gray = _stub_sampler(out_ch=1)
    gray.sample_tiled = s.sample_tiled
    with pytest.raises(ValueError, match="out_ext='jpg' needs a three-channel .RGB. output; this model's has 1"):
        gray.inference(src, tmp_path / "out", out_ext="jpg")
    assert not (tmp_path / "out").exists() and s.engine.encoded == [] and gray.engine.encoded == []


# ---------------------------------------------------------------------------------------------------------------- degrade
def test_the_command_line_passes_the_file_format_only_when_asked(monkeypatch):
    calls = []
    monkeypatch.setattr(degrade, "make_testset", lambda gt, lq, **kw: calls.append(kw) or {})
    monkeypatch.setattr(degrade, "make_face_testset", lambda gt, lq, **kw: calls.append(kw) or {})
    degrade.main(["gt", "lq"])
    degrade.main(["gt", "lq", "--ext", "jpg"])
    degrade.main(["gt", "lq", "--ext", "jpg", "--quality", "70", "--sf", "2"])
    assert calls == [dict(sf=4, seed=10000), dict(sf=4, seed=10000, ext="jpg", quality=None), dict(sf=2, seed=10000, ext="jpg", quality=70)]
    for bad in (["--ext", "bmp"], ["--recipe", "face", "--ext", "jpg"], ["--recipe", "face", "--quality", "50"]):
        with pytest.raises(SystemExit):
            degrade.main(["gt", "lq"] + bad)
    assert degrade._file_format("png", None) == ("png", None) and degrade._file_format("jpg", None) == ("jpg", 95) and degrade._file_format("jpg", 1) == ("jpg", 1)
    for ext, q, text in (("bmp", None, "ext must be 'png' or 'jpg'"), ("png", 90, "quality belongs to ext='jpg'"), ("jpg", 0, "quality must be an integer in 1 .. 100"),
                         ("jpg", 90.0, "quality must be an integer in 1 .. 100"), ("jpg", True, "quality must be an integer in 1 .. 100")):
        with pytest.raises(ValueError, match=text):
            degrade._file_format(ext, q)


def test_make_testset_rejects_a_bad_format_before_anything_is_written(tmp_path):
    from PIL import Image

    (tmp_path / "gt").mkdir()
    Image.fromarray(np.zeros((64, 64, 3), np.uint8)).save(tmp_path / "gt" / "a.png")
    with pytest.raises(ValueError, match="quality must be an integer in 1 .. 100"):
        degrade.make_testset(tmp_path / "gt", tmp_path / "lq", ext="jpg", quality=101)
    assert not (tmp_path / "lq").exists()


def test_write_plans_records_the_file_format(tmp_path):
    import json

    plan = degrade.draw_plan(degrade.REALESRGAN_TESTING, 1, 64, 48, 5)
    degrade.write_plans(tmp_path, {"a": plan})
    plain = (tmp_path / "plans.json").read_bytes()
    assert list(json.loads(plain)) == ["a"] and degrade.DegradePlan.from_dict(json.loads(plain)["a"]) == plan
    degrade.write_plans(tmp_path, {"a": plan}, "png", None)
    assert (tmp_path / "plans.json").read_bytes() == plain
    degrade.write_plans(tmp_path, {"a": plan}, "jpg", 80)
    recorded = json.load(open(tmp_path / "plans.json"))
    assert recorded.pop("_files") == {"ext": "jpg", "quality": 80} and recorded == json.loads(plain)

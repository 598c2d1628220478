"""rs_jpeg_encode on the GPU (tiny shapes, the file prints its wall time): EQUALITY ON EVERY BYTE, no tolerance anywhere, against
the files Pillow's libjpeg wrote (tests/golden/libjpeg_files.npz) and against the numpy restatement tests/_jpeg_enc_ref.py.

  * every size of J.SIZES with its five contents as one batch of five qualities: the files, their lengths;
  * scans that end in a stuffed FF 00, and `binary` at quality 100 with its 99 stuffed bytes;
  * 273 x 289: 2052 blocks, the least count above the 2048 one workgroup of the prefix sums scans, with a dummy column and a dummy row;
  * a batch against its B = 1 calls, nothing written at or beyond nbytes[b], a workspace full of garbage;
  * Pillow decodes the files to Engine.jpeg_codec of the same input; float inputs with exact .5 ties equal the uint8 route;
  * inference(out_ext="jpg") on the tiny parity-policy sampler of tests/test_colorfix_gpu.py: the batch, the pool and the tiled route;
    degrade.make_testset(ext="jpg").
"""
import ctypes as C
import hashlib
import io
import time

import numpy as np
import pytest
import torch

import helpers as H
import _jpeg_enc_ref as E
import _jpeg_ref as J

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    yield
    print(f"\ntests/test_jpeg_encode_gpu.py: {time.time() - _T0:.1f} s wall time")


@pytest.fixture(scope="module")
def files():
    return np.load(H.ROOT + "/tests/golden/libjpeg_files.npz")


def _dev(x, gpu):
    return torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


def _raw_call(u8_d, q, fill=0xA5):
    """rs_jpeg_encode itself on uint8 [B,H,W,3]: `out` pre-filled with `fill`, the workspace with random bytes.  Returns (out rows, nbytes)."""
    from resshift_amd import _lib

    lib = _lib.load()
    B, Hh, W, _ = u8_d.shape
    pitch = int(lib.rs_jpeg_encode_bound(Hh, W)) + 3
    out = torch.full((B, pitch), fill, device=u8_d.device, dtype=torch.uint8)
    work = torch.randint(0, 256, (int(lib.rs_jpeg_encode_workspace(B, Hh, W)),), device=u8_d.device, dtype=torch.uint8)
    nbytes = torch.full((B,), -1, device=u8_d.device, dtype=torch.int32)
    _lib.check(lib.rs_jpeg_encode(u8_d.data_ptr(), out.data_ptr(), nbytes.data_ptr(), (C.c_int * B)(*q), work.data_ptr(), B, 3, Hh, W, pitch,
                                  _lib.current_stream_ptr()), "rs_jpeg_encode")
    return out.cpu().numpy(), nbytes.cpu().tolist()


@pytest.mark.parametrize("si", range(len(J.SIZES)), ids=[f"{h}x{w}" for h, w in J.SIZES])
def test_files_equal_libjpegs_on_every_byte(gpu, files, si):
    """the five contents of one size as ONE batch with the recorded qualities: every file is the recorded one and the restatement's"""
    from resshift_amd import _lib

    Hh, W = J.SIZES[si]
    mine = [c for c in J.cases() if c[1] == (Hh, W)]
    u8 = np.stack([J.to_u8(J.content(kind, Hh, W, seed)) for _, _, kind, seed, _ in mine])
    q = [c[4] for c in mine]
    u8_d = _dev(u8, gpu)
    got = _lib.jpeg_encode(u8_d, q)
    assert torch.equal(u8_d.cpu(), torch.from_numpy(u8)) and len(got) == len(mine) and all(isinstance(g, bytes) for g in got)
    rows, nbytes = _raw_call(u8_d, q)
    for i, (key, *_) in enumerate(mine):
        want = files["file_" + key].tobytes()
        n = min(len(want), len(got[i]))
        diff = sum(a != b for a, b in zip(got[i][:n], want[:n])) + abs(len(want) - len(got[i]))
        print(f"jpeg_encode {key} q = {q[i]}: {len(got[i])} bytes (libjpeg: {len(want)}), {diff} differ")
        assert got[i] == want, (key, q[i], diff)
        assert got[i] == E.encode(u8[i], q[i])
        assert nbytes[i] == len(want) and rows[i, :nbytes[i]].tobytes() == want
        assert len(want) <= _lib.jpeg_encode_bound(Hh, W) == E.bound(Hh, W)


def test_scans_that_end_in_a_stuffed_byte(gpu, files):
    """J.content("random", 8, 8, seed) at E.STUFFED_END: the padded last byte is 0xFF and takes its 0x00; `binary` 64 x 48 at quality 100 holds 99
    stuffed bytes (the 0xFF bytes of its unstuffed scan)"""
    from resshift_amd import _lib

    cases = [c for c in E.extra_cases() if c[1] == (8, 8)]
    assert len(cases) == 4
    u8 = np.stack([J.to_u8(J.content(kind, 8, 8, seed)) for _, _, kind, seed, _ in cases])
    got = _lib.jpeg_encode(_dev(u8, gpu), [c[4] for c in cases])
    for i, (key, _, _, _, q) in enumerate(cases):
        assert got[i][-4:] == b"\xff\x00\xff\xd9", key
        assert got[i] == E.encode(u8[i], q), key
        assert len(got[i]) == int(files["len_" + key]) and hashlib.sha256(got[i]).hexdigest() == str(files["sha_" + key]), key
    key = "64x48_binary"
    q = int(np.load(H.ROOT + "/tests/golden/libjpeg_roundtrip.npz")["q_" + key])
    want = files["file_" + key].tobytes()
    u8 = J.to_u8(J.content("binary", 64, 48, [c[3] for c in J.cases() if c[0] == key][0]))
    stuffed = E.scan(u8, q, "no_stuffing").count(b"\xff")
    assert q == 100 and stuffed == 99 and len(want) == E.SCAN_OFFSET + len(E.scan(u8, q, "no_stuffing")) + stuffed + 2
    assert _lib.jpeg_encode(_dev(u8[None], gpu), q)[0] == want


def test_a_scan_longer_than_one_workgroup_of_the_prefix_sums(gpu, files):
    """E.LARGE_SIZE = 273 x 289: 18 x 19 MCUs = 2052 blocks, the least MCU grid above the 2048 elements one workgroup scans (JE_SCAN in
    csrc/jpeg_encode.hip), so the bit offsets take the reduce + scan + scan path, and so do the stuffing counts (6653 elements of 64 raw
    bytes at the bound).  Both sides are odd and = 1 (mod 16): the last block column and the last block row of the MCUs are dummies."""
    from resshift_amd import _lib

    Hh, W = E.LARGE_SIZE
    assert 6 * (-(-Hh // 16)) * (-(-W // 16)) == 2052 and 6 * (-(-(Hh - 16) // 16)) * (-(-W // 16)) <= 2048 and Hh % 16 == W % 16 == 1
    cases = [c for c in E.extra_cases() if c[1] == E.LARGE_SIZE]
    u8 = np.stack([J.to_u8(J.content(kind, Hh, W, seed)) for _, _, kind, seed, _ in cases])
    q = [c[4] for c in cases]
    assert [(c[2], c[4]) for c in cases] == [("random", 95), ("smooth", 30)]
    got = _lib.jpeg_encode(_dev(u8, gpu), q)
    for i, (key, *_) in enumerate(cases):
        want = E.encode(u8[i], q[i])
        print(f"jpeg_encode {key} q = {q[i]}: {len(got[i])} bytes (restatement: {len(want)})")
        assert got[i] == want, key
        assert len(got[i]) == int(files["len_" + key]) and hashlib.sha256(got[i]).hexdigest() == str(files["sha_" + key]), key
        assert _lib.jpeg_encode(_dev(u8[i:i + 1], gpu), q[i]) == [got[i]]


def test_a_batch_is_its_single_calls_and_nothing_is_written_past_the_file(gpu):
    """31 x 50 (dummy blocks on both edges), five contents at five qualities: B = 5 against five B = 1 calls; `out` was 0xA5 (then 0x5A, so that
    a file's own 0xA5 bytes are not mistaken) and every byte from nbytes[b] to the end of the row still is; the workspace held random bytes"""
    Hh, W = 31, 50
    u8 = np.stack([J.to_u8(J.content(kind, Hh, W, 300 + i)) for i, kind in enumerate(J.CONTENTS)])
    q = [95, 1, 100, 50, 30]
    u8_d = _dev(u8, gpu)
    rows, nbytes = _raw_call(u8_d, q, 0xA5)
    rows2, nbytes2 = _raw_call(u8_d, q, 0x5A)
    assert nbytes == nbytes2
    for i in range(5):
        n = nbytes[i]
        assert rows[i, :n].tobytes() == E.encode(u8[i], q[i]) == rows2[i, :n].tobytes(), i
        assert np.all(rows[i, n:] == 0xA5) and np.all(rows2[i, n:] == 0x5A), i
        one, n1 = _raw_call(u8_d[i:i + 1].clone(), q[i:i + 1])
        assert n1 == [n] and one[0, :n].tobytes() == rows[i, :n].tobytes() and np.all(one[0, n:] == 0xA5), i


def test_pillow_decodes_the_files_to_the_codecs_output_and_floats_take_the_u8_route(gpu, files):
    from PIL import Image

    from resshift_amd import _lib
    from resshift_amd.imageops import ImageOps

    ops = ImageOps(gpu)
    Hh, W = 40, 56
    x = np.stack([J.content(kind, Hh, W, 500 + i) for i, kind in enumerate(("float", "smooth", "random"))])
    q = [69, 30, 95]
    prod = x[0] * np.float32(255)
    assert (prod - np.floor(prod) == 0.5).sum() > 100 and x[0].min() < 0 and x[0].max() > 1        # exact .5 ties, values outside [0, 1]
    x_d = _dev(x, gpu)
    got = ops.jpeg_encode(x_d, q)
    u8 = np.stack([J.to_u8(xi) for xi in x])
    assert np.array_equal(_lib.unit_to_u8(x_d).cpu().numpy(), u8)                                   # one rounding rule: the codec's input step
    assert got == ops.jpeg_encode(_dev(u8, gpu), q) == [E.encode(u8[i], q[i]) for i in range(3)]
    key = "40x56_float"
    live_agrees = E.pillow_file(J.to_u8(J.content("float", 40, 56, [c[3] for c in J.cases() if c[0] == key][0])),
                                [c[4] for c in J.cases() if c[0] == key][0]) == files["file_" + key].tobytes()
    if not live_agrees:
        print("the live Pillow writes other files than the recorded one: the decode comparison is left out")
        return
    codec = ops.jpeg_codec(x_d, q).cpu().numpy()
    for i in range(3):
        dec = np.asarray(Image.open(io.BytesIO(got[i])).convert("RGB"))
        assert np.array_equal(dec.transpose(2, 0, 1).astype(np.float32) / np.float32(255), codec[i]), i


def test_more_images_than_one_call_takes(gpu):
    """B = 66 > RS_MAX_ROWS: the wrapper's chunks"""
    from resshift_amd import _lib

    u8 = np.stack([J.to_u8(J.content("random" if i % 2 else "smooth", 9, 8, 700 + i)) for i in range(66)])
    q = [1 + (37 * i) % 100 for i in range(66)]
    got = _lib.jpeg_encode(_dev(u8, gpu), q)
    assert len(got) == 66
    for i in (0, 1, 63, 64, 65):
        assert got[i] == E.encode(u8[i], q[i]), i


# ---------------------------------------------------------------------------------------------------------------- inference
def test_inference_writes_jpeg_files(gpu, tmp_path):
    """two 16 x 16 inputs (one tile each, the smallest the inference tests sample) through inference(seeded=True): out_ext="jpg" writes the
    JPEG of the very uint8 tensor that the default run writes as a PNG, returns the same scores, and the pool route writes the same kind"""
    from PIL import Image

    from test_colorfix_gpu import _sampler
    from oracle import make_golden_tiled as mt

    s, dp = _sampler(2, "none")
    src, gtd = tmp_path / "in", tmp_path / "gt"
    src.mkdir()
    gtd.mkdir()
    y = mt.tiled_inputs(dp["steps"])[0]
    rng = np.random.default_rng(5)
    for name, (r, c) in (("a", (0, 0)), ("b", (20, 8))):
        t = y[0, :, r:r + 16, c:c + 16]
        Image.fromarray(((t.permute(1, 2, 0) * 0.5 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).numpy()).save(src / f"{name}.png")
        Image.fromarray(rng.integers(0, 256, (16 * dp["sf"], 16 * dp["sf"], 3), dtype=np.uint8)).save(gtd / f"{name}.png")
    rows_png = s.inference(src, tmp_path / "png", bs=2, seeded=True, gt_path=gtd)
    rows_jpg = s.inference(src, tmp_path / "jpg", bs=2, seeded=True, gt_path=gtd, out_ext="jpg", jpeg_quality=90)
    assert rows_jpg == rows_png and sorted(rows_png) == ["a", "b"]
    assert sorted(p.name for p in (tmp_path / "jpg").iterdir()) == ["a.jpg", "b.jpg", "metrics.csv"]
    assert sorted(p.name for p in (tmp_path / "png").iterdir()) == ["a.png", "b.png", "metrics.csv"]
    u8 = np.stack([np.asarray(Image.open(tmp_path / "png" / f"{n}.png")) for n in "ab"])          # the tensor handed to the encoder, as the PNGs hold it
    want = s.engine.jpeg_encode(_dev(u8, gpu), 90)
    for i, n in enumerate("ab"):
        data = (tmp_path / "jpg" / f"{n}.jpg").read_bytes()
        assert data == want[i] == E.encode(u8[i], 90), n
    s.inference(src, tmp_path / "pool", bs=2, seeded=True, pool=True, out_ext="jpg", jpeg_quality=90)
    s.inference(src, tmp_path / "pool_png", bs=2, seeded=True, pool=True)
    assert sorted(p.name for p in (tmp_path / "pool").iterdir()) == ["a.jpg", "b.jpg"]
    for n in "ab":
        assert (tmp_path / "pool" / f"{n}.jpg").read_bytes() == E.encode(np.asarray(Image.open(tmp_path / "pool_png" / f"{n}.png")), 90), n


def test_inference_writes_jpeg_files_on_the_tiled_route(gpu, tmp_path):
    """the 40 x 28 fixture image (six tiles of 16 at stride 12): the .jpg is the JPEG of the blended uint8 image the default run writes"""
    from PIL import Image

    from test_colorfix_gpu import _sampler
    from oracle import make_golden_tiled as mt

    s, dp = _sampler(6, "none")
    src = tmp_path / "in"
    src.mkdir()
    y = mt.tiled_inputs(dp["steps"])[0]
    Image.fromarray(((y[0].permute(1, 2, 0) * 0.5 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).numpy()).save(src / "a.png")
    s.inference(src, tmp_path / "png", bs=1, seeded=True)
    s.inference(src, tmp_path / "jpg", bs=1, seeded=True, out_ext="jpg", jpeg_quality=75)
    u8 = np.asarray(Image.open(tmp_path / "png" / "a.png"))
    assert u8.shape == (160, 112, 3) and [p.name for p in (tmp_path / "jpg").iterdir()] == ["a.jpg"]
    assert (tmp_path / "jpg" / "a.jpg").read_bytes() == E.encode(u8, 75)


def test_make_testset_writes_jpeg_files(gpu, tmp_path):
    """degrade.make_testset(ext="jpg"): the LQ files are the JPEGs of the uint8 images the default run writes as PNGs; plans.json says so"""
    import json

    from PIL import Image

    from resshift_amd import degrade

    gt = tmp_path / "gt"
    gt.mkdir()
    Image.fromarray(np.load(H.ROOT + "/tests/golden/val_sr_lq.npz")["lq"][0, :64, :48]).save(gt / "a.png")   # (tests/test_degrade_gpu.py's first file)
    plans = degrade.make_testset(gt, tmp_path / "png", device=gpu)
    assert degrade.make_testset(gt, tmp_path / "jpg", device=gpu, ext="jpg", quality=80) == plans
    assert sorted(p.name for p in (tmp_path / "jpg").iterdir()) == ["a.jpg", "plans.json"]
    lq = np.asarray(Image.open(tmp_path / "png" / "a.png"))
    assert lq.shape == (16, 12, 3) and (tmp_path / "jpg" / "a.jpg").read_bytes() == E.encode(lq, 80)
    recorded, plain = json.load(open(tmp_path / "jpg" / "plans.json")), json.load(open(tmp_path / "png" / "plans.json"))
    assert recorded.pop("_files") == {"ext": "jpg", "quality": 80} and recorded == plain

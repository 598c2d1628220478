"""JPEG files coded on the device: times of Engine.jpeg_encode against what a host does with the same uint8 device tensor, by
scripts/degrade_bench.py's method - the legs alternate in one process, a warm-up round, then `--rounds` rounds of back-to-back calls
between two device events; each figure is the median round, `spread` is (max - min) / median.  Natural-image content: the 32 images of
tests/golden/val_sr_lq.npz up-sampled x4 (bicubic) to 256 x 256 - as one batch of 32, and as an 8 x 8 mosaic of 2048 x 2048 - at quality 95
and 30.

  jpeg_encode        imageops.jpeg_encode: the launches, the copy of the lengths and of the used bytes to the host, the `bytes` objects
  encode_kernels     rs_jpeg_encode alone into buffers allocated once: what the device spends, nothing copied
  jpeg_codec         rs_jpeg_codec on the same images (fp32 in and out): the transform half is shared, the difference is the entropy stage
  png_host           the route of `inference` without out_ext="jpg": the uint8 tensor to the host, Pillow's PNG save per image, one after another
  pillow_jpeg_host   the tensor to the host, Pillow's JPEG save(quality, subsampling=2) per image, one after another
  pillow_jpeg_16     the same on a pool of 16 threads (Pillow releases the GIL while it codes)

Before timing, the device's files are compared with Pillow's: `files_differ`.  Prints ONE JSON line, writes it to
profiles/jpeg_encode_bench.json (`--out`) and makes sure profiles/INDEX.md has the file's line.

    python scripts/jpeg_encode_bench.py [--rounds 5] [--window 0.1]
"""
from __future__ import annotations

import argparse
import ctypes as C
import io
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from _timing import measure  # noqa: E402
from degrade_bench import MEASURE  # noqa: E402
from resshift_amd import _lib  # noqa: E402

QUALITIES = (95, 30)
THREADS = 16
INDEX_LINE = ("| `jpeg_encode_bench.json` | `scripts/jpeg_encode_bench.py` (DESIGN §7j): `Engine.jpeg_encode` with its device-to-host copies, its kernels alone and "
              "`rs_jpeg_codec` against the host's routes for the same uint8 device tensor - copy + Pillow PNG save, copy + Pillow JPEG save serially and on 16 "
              "threads - on natural images, 32 × 256² and 1 × 2048², quality 95 and 30; median of alternating rounds, spread |")


def images(dev):
    """{name: uint8 [B,H,W,3] on the device}"""
    lq = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "val_sr_lq.npz"))["lq"]).permute(0, 3, 1, 2).float()
    up = F.interpolate(lq, scale_factor=4, mode="bicubic", align_corners=False).round().clamp(0, 255).to(torch.uint8)      # [32,3,256,256]
    tiles = torch.cat([up, up.flip(3)])                                                                                     # 64 tiles
    mosaic = tiles.reshape(8, 8, 3, 256, 256).permute(2, 0, 3, 1, 4).reshape(1, 3, 2048, 2048)
    return {"32x256x256": up.permute(0, 2, 3, 1).contiguous().to(dev), "1x2048x2048": mosaic.permute(0, 2, 3, 1).contiguous().to(dev)}


def pillow_save(im, fmt, quality):
    from PIL import Image

    buf = io.BytesIO()
    if fmt == "PNG":
        Image.fromarray(im).save(buf, format="PNG")
    else:
        Image.fromarray(im).save(buf, format="JPEG", quality=quality, subsampling=2)
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.1, help="seconds of back-to-back calls per leg and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encode_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_encode_bench.py measures on the GPU: no device is visible (there is no CPU fallback)")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    pool = ThreadPoolExecutor(THREADS)
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window, "host_threads": THREADS, "cases": {}}
    for name, u8 in images(dev).items():
        B, Hh, W, _ = u8.shape
        x01 = u8.permute(0, 3, 1, 2).float().div(255.0).contiguous()
        pitch = int(lib.rs_jpeg_encode_bound(Hh, W))
        out = torch.empty((B, pitch), device=dev, dtype=torch.uint8)
        work = torch.empty(int(lib.rs_jpeg_encode_workspace(B, Hh, W)), device=dev, dtype=torch.uint8)
        nbytes = torch.empty(B, device=dev, dtype=torch.int32)
        for q in QUALITIES:
            qs = (C.c_int * B)(*([q] * B))
            got = _lib.jpeg_encode(u8, q)
            host = u8.cpu().numpy()
            differ = sum(a != pillow_save(im, "JPEG", q) for a, im in zip(got, host))
            legs = {
                "jpeg_encode": lambda: _lib.jpeg_encode(u8, q),
                "encode_kernels": lambda: _lib.check(lib.rs_jpeg_encode(u8.data_ptr(), out.data_ptr(), nbytes.data_ptr(), qs, work.data_ptr(), B, 3, Hh, W, pitch,
                                                                        _lib.current_stream_ptr()), "rs_jpeg_encode"),
                "jpeg_codec": lambda: _lib.jpeg_codec(x01, q),
                "png_host": lambda: [pillow_save(im, "PNG", None) for im in u8.cpu().numpy()],
                "pillow_jpeg_host": lambda: [pillow_save(im, "JPEG", q) for im in u8.cpu().numpy()],
                "pillow_jpeg_16": lambda: list(pool.map(lambda im: pillow_save(im, "JPEG", q), u8.cpu().numpy())),
            }
            res = measure(legs, args.rounds, args.window, **MEASURE)
            ms = {k: v["ms"] for k, v in res.items()}
            result["cases"][f"{name}_q{q}"] = {
                "legs": res, "files_differ": int(differ), "file_bytes": int(sum(len(g) for g in got)), "pixel_bytes": int(u8.numel()),
                "entropy_stage_ms": ms["encode_kernels"] - ms["jpeg_codec"], "copies_and_host_ms": ms["jpeg_encode"] - ms["encode_kernels"],
                "speedup_over_png_host": ms["png_host"] / ms["jpeg_encode"], "speedup_over_pillow_jpeg_host": ms["pillow_jpeg_host"] / ms["jpeg_encode"],
                "speedup_over_pillow_jpeg_16": ms["pillow_jpeg_16"] / ms["jpeg_encode"]}
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    index = os.path.join(os.path.dirname(os.path.abspath(args.out)), "INDEX.md")
    if os.path.exists(index):
        text = open(index).read()
        if "`jpeg_encode_bench.json`" not in text:
            head, sep, rest = text.partition("|---|---|\n")
            with open(index, "w") as fh:
                fh.write(head + sep + INDEX_LINE + "\n" + rest)


if __name__ == "__main__":
    main()

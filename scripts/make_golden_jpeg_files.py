"""tests/golden/libjpeg_files.npz: the JPEG FILES Pillow's libjpeg writes, which rs_jpeg_encode reproduces byte for byte.
Data only, made from Pillow alone:

  file_<key>            uint8 [n]: PIL save(format="JPEG", quality=q, subsampling=2) of the input of every case of tests/_jpeg_ref.py cases()
                        (the inputs and qualities are those of libjpeg_roundtrip.npz)
  len_<key>, sha_<key>  for tests/_jpeg_enc_ref.py extra_cases() - the 8 x 8 files that end in a stuffed FF 00 and the 273 x 289 ones that
                        span the device's scan chunks - the length and the SHA-256 digest of the file only
  pillow, libjpeg       the version strings

The script first confirms that the numpy restatement tests/_jpeg_enc_ref.py equals Pillow on every file it records and on every `random`
case at every quality, and refuses to write otherwise.

    python scripts/make_golden_jpeg_files.py
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import _jpeg_enc_ref as E  # noqa: E402
import _jpeg_ref as J  # noqa: E402
from make_golden_jpeg import GOLDEN, versions  # noqa: E402


def main():
    arrays, total = {}, 0
    for key, (H, W), kind, seed, q in J.cases():
        u8 = J.to_u8(J.content(kind, H, W, seed))
        data = E.pillow_file(u8, q)
        assert E.encode(u8, q) == data, f"the restatement differs from Pillow on {key} at quality {q}"
        arrays["file_" + key] = np.frombuffer(data, np.uint8)
        total += len(data)
    n = 0
    for si, (H, W) in enumerate(J.SIZES):
        for q in J.QUALITIES:
            u8 = J.to_u8(J.content("random", H, W, 1000 + 10 * si))
            assert E.encode(u8, q) == E.pillow_file(u8, q), (H, W, q)
            n += 1
    for key, (H, W), kind, seed, q in E.extra_cases():
        u8 = J.to_u8(J.content(kind, H, W, seed))
        data = E.pillow_file(u8, q)
        assert E.encode(u8, q) == data, f"the restatement differs from Pillow on {key} at quality {q}"
        arrays["len_" + key], arrays["sha_" + key] = np.int64(len(data)), np.array(hashlib.sha256(data).hexdigest())
    pillow, libjpeg = versions()
    arrays["pillow"], arrays["libjpeg"] = np.array(pillow), np.array(libjpeg)
    path = os.path.join(GOLDEN, "libjpeg_files.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(J.cases())} files of {total} bytes recorded, {len(E.extra_cases())} by length and digest, {n} `random` (size, quality) pairs "
          f"confirmed against Pillow {pillow}, libjpeg {libjpeg}; {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()

"""tests/golden/libjpeg_roundtrip.npz and tests/golden/reference_face.npz.  Run on the build machine only - the second
fixture needs the reference tree (oracle.ref_import.REF); the tests read the fixtures, never the reference.  Data only:

  libjpeg_roundtrip.npz   per case of tests/_jpeg_ref.py cases(): in_<key> (the uint8 [H,W,3] input), out_<key> (what Pillow's libjpeg
                          returns for save(quality=q, subsampling=2) + open), q_<key>; `pillow` and `libjpeg`, the version strings.
                          The script first confirms that the numpy restatement equals Pillow on every case it records and on every
                          (size, quality) pair of the GPU test, and refuses to write otherwise.
  reference_face.npz      blur_<kernel key>_<Ho>x<Wo>: the reference's fp32 filter2D (basicsr/utils/img_process_util.py, loaded by path)
                          followed by fp32 F.interpolate(mode="bilinear") on tests/_face_ref.py's BLUR_KERNELS x BLUR_SIZES;
                          resize_<i>: F.interpolate alone on RESIZE_CASES, the first plane.

    python scripts/make_golden_jpeg.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import _degrade_ref as D  # noqa: E402
import _face_ref as FR  # noqa: E402
import _jpeg_ref as J  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def versions():
    import PIL
    from PIL import features

    return PIL.__version__, f"{features.version('jpg')} (libjpeg-turbo: {features.check_feature('libjpeg_turbo')})"


def jpeg_fixture():
    arrays = {}
    for key, (H, W), kind, seed, q in J.cases():
        u8 = J.to_u8(J.content(kind, H, W, seed))
        out = J.pillow_roundtrip(u8, q)
        assert np.array_equal(J.roundtrip(u8, q), out), f"the restatement differs from Pillow on {key} at quality {q}"
        arrays["in_" + key], arrays["out_" + key], arrays["q_" + key] = u8, out, np.int32(q)
    n = 0
    for si, (H, W) in enumerate(J.SIZES):          # what the GPU test checks against the restatement alone
        for q in J.QUALITIES:
            for ci, kind in enumerate(J.CONTENTS):
                u8 = J.to_u8(J.content(kind, H, W, 1000 + 10 * si + ci))
                assert np.array_equal(J.roundtrip(u8, q), J.pillow_roundtrip(u8, q)), (H, W, q, kind)
                n += 1
    pillow, libjpeg = versions()
    arrays["pillow"], arrays["libjpeg"] = np.array(pillow), np.array(libjpeg)
    path = os.path.join(GOLDEN, "libjpeg_roundtrip.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(J.cases())} cases recorded, {n} (size, quality, content) triples confirmed against Pillow {pillow}, libjpeg {libjpeg}; "
          f"{os.path.getsize(path)} bytes")


def face_fixture():
    from make_golden_degrade import _load, _stub

    _stub("cv2")
    _stub("torchvision.transforms.functional_tensor")
    ip = _load("basicsr/utils/img_process_util.py")
    arrays, worst = {}, 0.0
    with torch.no_grad():
        for i, (key, k, n, seed) in enumerate(FR.BLUR_KERNELS):
            x, kernels = FR.blur_case(i)
            blurred = ip.filter2D(torch.from_numpy(x), torch.from_numpy(kernels))
            assert blurred.dtype == torch.float32
            for size in FR.BLUR_SIZES:
                y = F.interpolate(blurred, size=size, mode="bilinear", align_corners=False).numpy()
                arrays[f"blur_{key}_{size[0]}x{size[1]}"] = y
                worst = max(worst, float(np.abs(FR.blur_resize(x, kernels, size) - y).max()))
        for i, (shape, size) in enumerate(FR.RESIZE_CASES):
            x = D.inputs((2, 3, *shape), FR.RESIZE_SEED + i)
            y = F.interpolate(torch.from_numpy(x), size=size, mode="bilinear", align_corners=False).numpy()[:1, :1]
            arrays[f"resize_{i}"] = y
            worst = max(worst, float(np.abs(FR.blur_resize(x[:1, :1], None, size) - y).max()))
    path = os.path.join(GOLDEN, "reference_face.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: max |float64 restatement - reference fp32| = {worst:.3e} (tests/_face_ref.py REF_ERR = {FR.REF_ERR:.1e}); {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    jpeg_fixture()
    face_fixture()

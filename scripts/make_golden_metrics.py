"""tests/golden/reference_metrics.npz: what the reference's own `utils.util_image.calculate_psnr` / `calculate_ssim` return on the image
pairs of tests/_metrics_ref.py.  Run on the build machine only - it needs the reference tree (oracle.ref_import.REF);
the tests read the fixture, never the reference.

The reference module imports `cv2` and `skimage` at its top.  Where OpenCV is not installed a stand-in `cv2` module supplies the two
functions the metric uses: `getGaussianKernel(11, 1.5)` is the normalised exponential exp(-(i - 5)^2 / 4.5) / sum that OpenCV computes
for this size, and `filter2D(img, -1, window)` is `scipy.ndimage.correlate(img, window, mode="mirror")` - OpenCV's default border is
that reflection, and the border mode cannot matter: the reference crops the 5 pixels the window reaches over.  `skimage` gets an empty
stub (the metric does not use it).

The pairs: ground truth = images 0 - 3 of tests/golden/val_sr_lq.npz (64 x 64 x 3, not stored again); "restored" = those plus seeded
Gaussian noise of sigma 2, 10 and 40, rounded and clipped to uint8; a gray (C = 1) pair (the Y of image 0, sigma 10); a 32 x 32 x 3 flat
image against itself with one pixel changed (SSIM within 1e-4 of 1: the case where E[x^2] - mu^2 cancels).  Every pair is scored under
ycbcr in {True, False} (colour pairs) and border in {0, 4}.  No pixel of any image may be one of the 194 RGB triples whose exact Y is a
tie - only there is the reference's float64 Y not a function (numpy's dot paths disagree with each other); asserted here and in
tests/test_metrics_cpu.py.

The fixture holds uint8 images and float64 scalars only.  The archive is written with fixed time stamps: the script regenerates the
committed file byte for byte.  Data only; nothing of the reference's text is copied.

    python scripts/make_golden_metrics.py
"""
from __future__ import annotations

import importlib
import io
import os
import sys
import types
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _metrics_ref as M  # noqa: E402
from oracle import ref_import  # noqa: E402

OUT = os.path.join(ROOT, M.GOLDEN)


def cv2_stand_in():
    from scipy import ndimage

    cv2 = types.ModuleType("cv2")

    def getGaussianKernel(ksize, sigma):
        assert (ksize, sigma) == (11, 1.5)
        return M.window().reshape(-1, 1)

    def filter2D(img, ddepth, kernel):
        assert ddepth == -1
        return ndimage.correlate(img, kernel, mode="mirror")

    cv2.getGaussianKernel, cv2.filter2D = getGaussianKernel, filter2D
    return cv2


def reference_module():
    try:
        importlib.import_module("cv2")
    except ImportError:
        sys.modules["cv2"] = cv2_stand_in()
    try:
        importlib.import_module("skimage")
    except ImportError:
        stub = types.ModuleType("skimage")
        stub.img_as_ubyte = stub.img_as_float32 = None
        sys.modules["skimage"] = stub
    if ref_import.REF not in sys.path:
        sys.path.insert(0, ref_import.REF)
    return importlib.import_module("utils.util_image")


def images():
    gt = np.load(os.path.join(ROOT, "tests", "golden", "val_sr_lq.npz"))["lq"][:4]
    assert gt.shape == (4, 64, 64, 3) and gt.dtype == np.uint8
    rng = np.random.default_rng(M.NOISE_SEED)
    noisy = lambda x, s: np.clip(np.rint(x.astype(np.float64) + rng.normal(0.0, s, x.shape)), 0, 255).astype(np.uint8)
    z = {f"sr_s{s}": noisy(gt, s) for s in M.SIGMAS}
    z["gt_gray"] = M.rgb_to_y(gt[0])[:, :, None]
    z["sr_gray"] = noisy(z["gt_gray"], 10)
    z["gt_flat"] = np.full((32, 32, 3), 128, dtype=np.uint8)
    z["sr_flat"] = z["gt_flat"].copy()
    z["sr_flat"][16, 16] = (129, 129, 129)
    return z, gt


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps and a fixed order"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    ui = reference_module()
    arrays, gt = images()
    z = dict(arrays, gt=gt)
    for name, sr, g, colour in M.golden_pairs(z):
        for im in (sr, g):
            assert im.shape[2] == 1 or not M.is_tie(im).any(), f"{name}: a pixel is one of the {M.N_TIES} tie triples"
    worst_p = worst_s = 0.0
    for key, sr, g, border, ycbcr in M.golden_cases(z):
        a, b = (sr[:, :, 0], g[:, :, 0]) if sr.shape[2] == 1 else (sr, g)
        psnr = float(ui.calculate_psnr(a, b, border=border, ycbcr=ycbcr))
        ssim = float(ui.calculate_ssim(a, b, border=border, ycbcr=ycbcr))
        arrays["psnr_" + key], arrays["ssim_" + key] = np.float64(psnr), np.float64(ssim)
        _, p, s = M.metrics(sr, g, border, ycbcr)
        dp = 0.0 if p == psnr else abs(p - psnr)
        worst_p, worst_s = max(worst_p, dp), max(worst_s, abs(s - ssim))
        print(f"{key}: psnr {psnr:.6f} dB, ssim {ssim:.8f}   |restatement - reference| = {dp:.1e} dB, {abs(s - ssim):.1e}")
    write_npz(OUT, arrays)
    print(f"worst |restatement - reference|: psnr {worst_p:.2e} dB, ssim {worst_s:.2e}")
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()

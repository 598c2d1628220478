"""PSNR / SSIM in integer and float64 numpy: the restatement of the definition in include/resshift_hip.h ("image metrics"), and the
cases the CPU and GPU tests share.  It is the reference's utils/util_image.py calculate_psnr / calculate_ssim with one
stated deviation: Y is exact integer arithmetic, ties to even.

One image is uint8 [H,W,C] (C = 1 or 3) or [H,W]; a batch is a sequence of them.
"""
from __future__ import annotations

import math

import numpy as np

C1, C2 = 6.5025, 58.5225
TAPS = 11
Y_COEF = (65481, 128553, 24966)   # MATLAB's 65.481, 128.553, 24.966 times 1000
Y_DEN = 255000
N_TIES = 194                      # RGB triples whose exact Y is half way between two integers


def window() -> np.ndarray:
    g = np.exp(-((np.arange(TAPS) - 5.0) ** 2) / 4.5)
    return g / g.sum()


def quantise(x: np.ndarray) -> np.ndarray:
    """fp32 [C,H,W] in [-1,1] -> uint8 [H,W,C], as rs_output_to_u8 does it: x*0.5+0.5, clamp, *255, round half to even - every step fp32"""
    v = x.astype(np.float32) * np.float32(0.5) + np.float32(0.5)
    v = np.clip(v, np.float32(0), np.float32(1)) * np.float32(255)
    return np.rint(v).astype(np.uint8).transpose(1, 2, 0)


def y_numerator(rgb: np.ndarray) -> np.ndarray:
    rgb = rgb.astype(np.int64)
    return Y_COEF[0] * rgb[..., 0] + Y_COEF[1] * rgb[..., 1] + Y_COEF[2] * rgb[..., 2]


def rgb_to_y(rgb: np.ndarray) -> np.ndarray:
    """uint8 [...,3] -> uint8 [...]: 16 + round((65481 r + 128553 g + 24966 b) / 255000), exact, ties to even"""
    q, rem = np.divmod(y_numerator(rgb), Y_DEN)
    q = q + ((2 * rem > Y_DEN) | ((2 * rem == Y_DEN) & (q % 2 == 1)))
    return (16 + q).astype(np.uint8)


def is_tie(rgb: np.ndarray) -> np.ndarray:
    """True where the exact Y of the triple is a tie: only there is the reference's float64 expression ambiguous"""
    return 2 * (y_numerator(rgb) % Y_DEN) == Y_DEN


def rgb_to_y_float64(rgb: np.ndarray) -> np.ndarray:
    """the reference's expression (utils/util_image.py rgb2ycbcr), written left to right in float64"""
    f = rgb.astype(np.float64)
    c = np.array([65.481, 128.553, 24.966]) / 255.0
    return (f[..., 0] * c[0] + f[..., 1] * c[1] + f[..., 2] * c[2] + 16.0).round().astype(np.uint8)


def all_triples() -> np.ndarray:
    """uint8 [4096, 4096, 3]: every RGB triple once"""
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


def planes(im: np.ndarray, border: int, ycbcr: bool) -> np.ndarray:
    """uint8 image -> int64 [C', H', W']: Y when asked, then the crop"""
    im = np.asarray(im)
    assert im.dtype == np.uint8
    if im.ndim == 2:
        im = im[:, :, None]
    if ycbcr:
        assert im.shape[2] == 3
        im = rgb_to_y(im)[:, :, None]
    h, w = im.shape[:2]
    im = im[border:h - border, border:w - border]
    if im.shape[0] < TAPS or im.shape[1] < TAPS:
        raise ValueError(f"the cropped image is {im.shape[0]} x {im.shape[1]}: the 11 x 11 window needs at least 11 x 11")
    return im.transpose(2, 0, 1).astype(np.int64)


def psnr_of(sse: int, n: int) -> float:
    return math.inf if sse == 0 else 20.0 * math.log10(255.0 / math.sqrt(sse / n))


def _valid(x: np.ndarray, g: np.ndarray) -> np.ndarray:
    """the separable "valid" window over a float64 plane: along the columns of every row, then along the rows; taps ascending"""
    wv = x.shape[1] - TAPS + 1
    h = sum(g[k] * x[:, k:k + wv] for k in range(TAPS))
    hv = x.shape[0] - TAPS + 1
    return sum(g[k] * h[k:k + hv] for k in range(TAPS))


def ssim_plane(a: np.ndarray, b: np.ndarray) -> float:
    g = window()
    a, b = a.astype(np.float64), b.astype(np.float64)
    mu1, mu2 = _valid(a, g), _valid(b, g)
    s1 = _valid(a * a, g) - mu1 * mu1
    s2 = _valid(b * b, g) - mu2 * mu2
    s12 = _valid(a * b, g) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return float(m.mean())


def metrics(a: np.ndarray, b: np.ndarray, border: int = 0, ycbcr: bool = True):
    """(sse, psnr, ssim) of one image pair"""
    if np.asarray(a).shape != np.asarray(b).shape:
        raise ValueError("the images must have the same shape")
    pa, pb = planes(a, border, ycbcr), planes(b, border, ycbcr)
    sse = int(((pa - pb) ** 2).sum())
    ssim = float(np.mean([ssim_plane(x, y) for x, y in zip(pa, pb)]))
    return sse, psnr_of(sse, pa.size), ssim


def batch(a, b, border=0, ycbcr=True):
    """(sse int64 [B], psnr float64 [B], ssim float64 [B]) of two sequences of images"""
    rows = [metrics(x, y, border, ycbcr) for x, y in zip(a, b)]
    return (np.array([r[0] for r in rows], dtype=np.int64), np.array([r[1] for r in rows], dtype=np.float64),
            np.array([r[2] for r in rows], dtype=np.float64))


# ---- the fixture (scripts/make_golden_metrics.py writes it, the tests read it) ------------------------------------------------------
GOLDEN = "tests/golden/reference_metrics.npz"
SIGMAS = (2, 10, 40)
PARAMS = [(ycbcr, border) for ycbcr in (True, False) for border in (0, 4)]
NOISE_SEED = 20241019   # (20241018 draws four of the tie triples)


def load_golden(root):
    """the fixture as a dict; the ground truth of the colour pairs is images 0 - 3 of tests/golden/val_sr_lq.npz and is not stored twice"""
    z = dict(np.load(f"{root}/{GOLDEN}"))
    z["gt"] = np.load(f"{root}/tests/golden/val_sr_lq.npz")["lq"][:4]
    return z


def golden_pairs(z):
    """[(name, sr, gt, colour)] of the fixture `z` (load_golden): four 64 x 64 x 3 images at three noise levels, a gray (C = 1) pair, and
    the 32 x 32 x 3 flat image with one pixel changed"""
    out = []
    for s in SIGMAS:
        for i in range(4):
            out.append((f"s{s}_im{i}", z[f"sr_s{s}"][i], z["gt"][i], True))
    out.append(("gray", z["sr_gray"], z["gt_gray"], False))
    out.append(("flat", z["sr_flat"], z["gt_flat"], True))
    return out


def golden_cases(z):
    """[(key, sr, gt, border, ycbcr)]: every pair under every parameter set it allows; `key` names the recorded scalars psnr_<key>, ssim_<key>"""
    out = []
    for name, sr, gt, colour in golden_pairs(z):
        for ycbcr, border in PARAMS:
            if ycbcr and not colour:
                continue
            out.append((f"{name}_y{int(ycbcr)}_b{border}", sr, gt, border, ycbcr))
    return out

"""Antialiased resize in float64 numpy: the restatement of the definition in include/resshift_hip.h ("antialiased resize"), and the
reference of tests/test_resize_cpu.py and tests/test_resize_gpu.py.  x [..., H, W], any leading axes.

    one axis (n -> m, scale s):  a = min(s, 1), kw = 4 / a, P = ceil(kw) + 2;  output i, taps k = 0 .. P-1:
        u = (i + 1) / s + 0.5 (1 - 1/s),  left = floor(u - kw / 2),  j = left + k (1-based),  raw weight a * cubic(a * (u - j)),
        weights divided by their sum, the tap reads in[mirror(j - 1)],  mirror: q = (j - 1) mod 2n, q < n ? q : 2n - 1 - q
    cubic = Keys, A = -0.5.  H first, then W.

The keyword arguments of `axis_matrix` are the mutations of tests/test_resize_cpu.py; their defaults are the definition.
"""
import math
from fractions import Fraction

import numpy as np


def cubic(x, A=-0.5):
    ax = np.abs(x)
    near = (A + 2.0) * ax ** 3 - (A + 3.0) * ax ** 2 + 1.0
    far = A * ax ** 3 - 5.0 * A * ax ** 2 + 8.0 * A * ax - 4.0 * A
    return np.where(ax <= 1.0, near, np.where(ax <= 2.0, far, 0.0))


def taps(s):
    """P of scale s"""
    return math.ceil(4.0 / min(s, 1.0)) + 2


def mirror(q, n, repeat_edge=True):
    """0-based index of any sign -> [0, n): the symmetric reflection that repeats the edge sample (period 2n); `repeat_edge=False`: the
    reflection about the edge sample itself (period 2n - 2), a mutation"""
    q = np.asarray(q, dtype=np.int64)
    if not repeat_edge:
        p = max(2 * n - 2, 1)
        m = np.mod(q, p)
        return np.where(m < n, m, p - m)
    m = np.mod(q, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def axis_matrix(n, m, s, antialias=True, border="mirror", A=-0.5, normalise=True, shift=0.0):
    """float64 [m, n]: row i holds the weights of output i, added where reflected taps coincide"""
    a = min(s, 1.0) if antialias else 1.0
    kw = 4.0 / a
    P = math.ceil(kw) + 2
    i = np.arange(m, dtype=np.float64)
    u = (i + 1.0) / s + 0.5 * (1.0 - 1.0 / s) + shift
    left = np.floor(u - kw / 2.0)
    j = left[:, None] + np.arange(P, dtype=np.float64)[None, :]          # 1-based
    w = a * cubic(a * (u[:, None] - j), A)
    if normalise:
        w = w / w.sum(axis=1, keepdims=True)
    q = j.astype(np.int64) - 1
    if border == "mirror":
        idx = mirror(q, n)
    elif border == "clamp":
        idx = np.clip(q, 0, n - 1)
    elif border == "reflect":
        idx = mirror(q, n, repeat_edge=False)
    else:
        raise ValueError(border)
    mat = np.zeros((m, n), dtype=np.float64)
    np.add.at(mat, (np.repeat(np.arange(m), P), idx.ravel()), w.ravel())
    return mat


def out_size(n, scale):
    """ceil(n * scale), exactly: the scale as the nearest fraction of denominator <= 4096 (0.3 * 40 is 12, not ceil(12.000000000000002))"""
    return math.ceil(n * Fraction(scale).limit_denominator(4096))


def resize(x, scale=None, size=None, clamp=False, **mutation):
    """imresize with antialiasing: `scale` (both axes, output ceil(n * scale)) or `size` (Ho, Wo) (per-axis scales Ho / H, Wo / W)"""
    x = np.asarray(x, dtype=np.float64)
    H, W = x.shape[-2:]
    if (scale is None) == (size is None):
        raise ValueError("exactly one of scale and size")
    if scale is not None:
        Ho, Wo, sh, sw = out_size(H, scale), out_size(W, scale), float(scale), float(scale)
    else:
        Ho, Wo = size
        sh, sw = Ho / H, Wo / W
    out = axis_matrix(H, Ho, sh, **mutation) @ x @ axis_matrix(W, Wo, sw, **mutation).T
    return np.clip(out, -1.0, 1.0) if clamp else out


# ---- the cases of the tests: ((H, W), "scale" | "size", value), B = 2, C = 3
CASES = [
    ((20, 28), "scale", 0.5),        # output 10 x 14, smaller than any tile
    ((160, 208), "scale", 0.5),      # 80 x 104: 5 x 2 workgroup tiles of 16 x 64, ragged to the right
    ((37, 53), "scale", 0.75),       # non-dyadic
    ((64, 96), "scale", 0.25),       # P = 18
    ((70, 37), "scale", 1 / 3),      # fractions not representable
    ((24, 40), "scale", 1.5),        # upscale
    ((33, 20), "scale", 2.0),        # upscale
    ((3, 50), "scale", 0.125),       # P = 34, repeated reflection along H (restatement only: the reference's single reflection cannot run it)
    ((40, 52), "size", (17, 64)),    # down along H, up along W
]
GOLDEN_CASES = [c for c in CASES if c[1] == "scale" and c[2] != 0.125]


def case_id(case):
    (H, W), kind, v = case
    return f"{H}x{W}-{kind}-" + ("x".join(map(str, v)) if kind == "size" else f"{v:.4g}")


def golden_key(case):
    (H, W), _, v = case
    return f"{H}x{W}_{Fraction(v).limit_denominator(4096).numerator}over{Fraction(v).limit_denominator(4096).denominator}"


def inputs(H, W, seed=0, B=2, C=3):
    """uniform in (-1, 1) from a fixed numpy seed: float32 [B, C, H, W]"""
    rng = np.random.RandomState(3000 + seed)
    return (rng.uniform(-1.0, 1.0, size=(B, C, H, W))).astype(np.float32)


def saturated_share(out):
    """share of outputs sitting at +-1, where the clamp could hide an error"""
    return float(np.mean(np.abs(np.asarray(out)) >= 1.0))

"""Colour correction in float64 numpy: the restatement of the definition in include/resshift_hip.h ("colour correction"), and the
reference of tests/test_colorfix_cpu.py and tests/test_colorfix_gpu.py.  sr [..., H*sf, W*sf], lq [..., H, W], any leading axes.

    up(lq)  = bicubic, align_corners=False, A = -0.75, border-clamped taps; identity at sf = 1
    wavelet = clamp(sr - L(sr - up(lq))),  L = B_16 o B_8 o B_4 o B_2 o B_1 (B_1 first),
              B_d = horizontal then vertical  y[i] = (x[clamp(i-d)] + x[clamp(i+d)]) / 4 + x[i] / 2
    adain   = clamp((sr - mean_sr) * std_lq / std_sr + mean_lq) per plane, std = sqrt(unbiased variance + 1e-5)
"""
import numpy as np

A = -0.75
DILATIONS = (1, 2, 4, 8, 16)
REACH = sum(DILATIONS)   # 31


def _cubic1(x):
    return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0


def _cubic2(x):
    return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A


def bicubic_matrix(n, sf):
    """float64 [n*sf, n]: row o holds the four tap weights of output o, added where border-clamped taps coincide"""
    o = np.arange(n * sf, dtype=np.float64)
    f = (o + 0.5) / sf - 0.5
    i0 = np.floor(f)
    t = f - i0
    w = np.stack([_cubic2(t + 1.0), _cubic1(t), _cubic1(1.0 - t), _cubic2(2.0 - t)], axis=1)
    m = np.zeros((n * sf, n), dtype=np.float64)
    for j in range(4):
        idx = np.clip(i0.astype(np.int64) - 1 + j, 0, n - 1)
        np.add.at(m, (np.arange(n * sf), idx), w[:, j])
    return m


def up(lq, sf):
    lq = np.asarray(lq, dtype=np.float64)
    if sf == 1:
        return lq
    my, mx = bicubic_matrix(lq.shape[-2], sf), bicubic_matrix(lq.shape[-1], sf)
    return my @ lq @ mx.T


def _pass(x, d, axis):
    n = x.shape[axis]
    i = np.arange(n)
    lo, hi = np.clip(i - d, 0, n - 1), np.clip(i + d, 0, n - 1)
    return 0.25 * (np.take(x, lo, axis=axis) + np.take(x, hi, axis=axis)) + 0.5 * x


def blur(x, d):
    """B_d: the separable 1-2-1 kernel with dilation d, replicate padding of x itself"""
    return _pass(_pass(x, d, -1), d, -2)


def low(x, dilations=DILATIONS):
    """L: the levels in the order given"""
    x = np.asarray(x, dtype=np.float64)
    for d in dilations:
        x = blur(x, d)
    return x


def wavelet(sr, lq, sf, dilations=DILATIONS):
    sr = np.asarray(sr, dtype=np.float64)
    return np.clip(sr - low(sr - up(lq, sf), dilations), -1.0, 1.0)


def plane_stats(x):
    """(mean, std) per plane, keepdims: std = sqrt(unbiased variance + 1e-5)"""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=(-2, -1), keepdims=True)
    n = x.shape[-2] * x.shape[-1]
    var = ((x - mean) ** 2).sum(axis=(-2, -1), keepdims=True) / max(n - 1, 1)
    return mean, np.sqrt(var + 1e-5)


def adain(sr, lq):
    sr = np.asarray(sr, dtype=np.float64)
    m_sr, s_sr = plane_stats(sr)
    m_lq, s_lq = plane_stats(lq)
    return np.clip((sr - m_sr) * s_lq / s_sr + m_lq, -1.0, 1.0)


def color_fix(sr, lq, mode):
    sf = np.asarray(sr).shape[-2] // np.asarray(lq).shape[-2]
    return wavelet(sr, lq, sf) if mode == "wavelet" else adain(sr, lq)


# ---- the inputs of the tests: (H, W, sf), B = 2, C = 3
SHAPES = [(5, 7, 4), (40, 52, 4), (33, 20, 2), (70, 37, 1)]


def inputs(H, W, sf, seed=0, B=2, C=3):
    """lq uniform in [-1,1]; sr = clamp(0.8 nearest_up(lq) + 0.3 randn + 0.15), from a seeded CPU generator: float32 torch tensors"""
    import torch

    g = torch.Generator().manual_seed(1000 + seed)
    lq = torch.rand(B, C, H, W, generator=g) * 2 - 1
    near = lq.repeat_interleave(sf, dim=2).repeat_interleave(sf, dim=3)
    sr = (0.8 * near + 0.3 * torch.randn(B, C, H * sf, W * sf, generator=g) + 0.15).clamp(-1, 1)
    return sr.contiguous(), lq.contiguous()


def low_contrast_inputs(seed=0, B=2, C=3):
    """sr = 0.9 + 0.01 randn at 160 x 208, lq = 0.2 + 0.3 randn at 40 x 52: the plane on which E[x^2] - mean^2 loses the variance in fp32"""
    import torch

    g = torch.Generator().manual_seed(2000 + seed)
    sr = 0.9 + 0.01 * torch.randn(B, C, 160, 208, generator=g)
    lq = 0.2 + 0.3 * torch.randn(B, C, 40, 52, generator=g)
    return sr.contiguous(), lq.contiguous()


def saturated_share(out):
    """share of outputs sitting at +-1, where the clamp could hide an error"""
    out = np.asarray(out)
    return float(np.mean(np.abs(out) >= 1.0))


def adain_tolerance(sr, lq):
    """per plane, keepdims: 2e-6 + 8 * 2^-24 * (1 + |mean_sr| / std_sr) * std_lq - the rounding of sr - mean amplified by the gain, a margin
    of eight on it, and a floor for the remaining arithmetic"""
    m_sr, s_sr = plane_stats(sr)
    _, s_lq = plane_stats(lq)
    return 2e-6 + 8 * 2.0 ** -24 * (1 + np.abs(m_sr) / s_sr) * s_lq

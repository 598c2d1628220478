"""Feathered tile blending in float64 numpy: the restatement of the definition in include/resshift_hip.h ("feathered tile blending"),
and the reference of tests/test_feather_cpu.py and tests/test_feather_gpu.py.  Everything is in HR (canvas) pixels.

    w1(p, n, R) = 1 if R == 0 else min(1, (min(p, n-1-p) + 0.5) / R)
    w(i, j)     = w1(i, nh, Rh) * w1(j, nw, Rw)
    acc += w * tile, count += w;  output = acc / count
"""
import numpy as np


def w1(n, R):
    """the 1-D weights of an n-pixel tile side with ramp width R: float64 [n]"""
    if R == 0:
        return np.ones(n, dtype=np.float64)
    p = np.arange(n, dtype=np.float64)
    return np.minimum(1.0, (np.minimum(p, n - 1 - p) + 0.5) / R)


def weight(nh, nw, Rh, Rw):
    """the 2-D weight of an nh x nw tile: float64 [nh, nw]"""
    return np.outer(w1(nh, Rh), w1(nw, Rw))


def accumulate(acc, count, tile, y0, x0, Rh, Rw):
    """acc [..., H, W] and count [H, W] (float64, in place) += the weighted tile [..., nh, nw] at (y0, x0)"""
    nh, nw = tile.shape[-2:]
    w = weight(nh, nw, Rh, Rw)
    acc[..., y0:y0 + nh, x0:x0 + nw] += w * np.asarray(tile, dtype=np.float64)
    count[y0:y0 + nh, x0:x0 + nw] += w


def uniform_accumulate(acc, count, tile, y0, x0):
    """the reference's uniform average in the same form (R = 0)"""
    accumulate(acc, count, tile, y0, x0, 0, 0)


def blend(shape, tiles, Rh, Rw):
    """canvas of `shape` [..., H, W] from `tiles` = [(tile [..., nh, nw], y0, x0)]: acc / count, float64"""
    acc, count = np.zeros(shape, dtype=np.float64), np.zeros(shape[-2:], dtype=np.float64)
    for tile, y0, x0 in tiles:
        accumulate(acc, count, tile, y0, x0, Rh, Rw)
    assert np.all(count > 0), "a canvas pixel no tile covers"
    return acc / count


def ramp(chop_size, chop_stride, sf):
    """what the host passes for both ramp widths: the overlap of two neighbouring tiles in HR pixels"""
    return (chop_size - chop_stride) * sf

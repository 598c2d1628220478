"""Float64 numpy restatement of the per-request noise definition (include/resshift_hip.h rs_noise_key): the reference of
tests/test_noise_cpu.py and tests/test_noise_gpu.py - never the kernel itself.

Element i (index in the image's own latent, NCHW order) of draw k of key (seed, stream): q = i // 4; Philox4x32-10 with counter
(q, k, stream, 0) and key (seed & 0xffffffff, seed >> 32) gives w0 .. w3; elements 4q, 4q+1 come from (w0, w1), elements 4q+2, 4q+3 from
(w2, w3): u1 = ((wa >> 8) + 1) 2^-24, u2 = (wb >> 8) 2^-24, r = sqrt(-2 ln u1), pair = (r cos 2 pi u2, r sin 2 pi u2).
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit values, key: two; returns the four output words as uint64 arrays holding 32-bit values"""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]   # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def _pair(wa, wb):
    u1 = ((wa >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (wb >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    # cos / sin of 2 pi u2 with the quadrant taken out exactly (2 u2 is exact; as sincospi does), so that the float64 value is accurate
    x = 2.0 * u2                      # in [0, 2)
    return r * _cospi(x), r * _sinpi(x)


def _sinpi(x):
    n = np.round(2.0 * x)             # nearest multiple of 1/2
    f = x - 0.5 * n                   # exact, |f| <= 1/4
    s, c = np.sin(np.pi * f), np.cos(np.pi * f)
    m = n.astype(np.int64) % 4
    return np.where(m == 0, s, np.where(m == 1, c, np.where(m == 2, -s, -c)))


def _cospi(x):
    n = np.round(2.0 * x)
    f = x - 0.5 * n
    s, c = np.sin(np.pi * f), np.cos(np.pi * f)
    m = n.astype(np.int64) % 4
    return np.where(m == 0, c, np.where(m == 1, -s, np.where(m == 2, -c, s)))


def normals(seed, stream, draw, count):
    """float64 normals of elements 0 .. count-1 of draw `draw` of key (seed, stream)"""
    seed = int(seed) % 2 ** 64
    nq = (count + 3) // 4
    w = philox4x32_10((np.arange(nq, dtype=np.uint64), draw, stream, 0), (seed & 0xFFFFFFFF, seed >> 32))
    a0, a1 = _pair(w[0], w[1])
    a2, a3 = _pair(w[2], w[3])
    return np.stack([a0, a1, a2, a3], 1).reshape(-1)[:count]


def draws(seed, stream, steps, shape):
    """fp32 array [steps+1, *shape]: draw 0 (prior) .. draw steps of one image, the restatement rounded to fp32"""
    count = int(np.prod(shape))
    return np.stack([normals(seed, stream, k, count) for k in range(steps + 1)]).astype(np.float32).reshape((steps + 1,) + tuple(shape))

// Counter-based Gaussian noise: a draw is a pure function of (seed, stream, draw index, element index), computed in
// registers by the kernel that consumes it.  Replaces the torch.randn tensors of models/gaussian_diffusion.py:358,446 (p_sample's
// randn_like, the prior draw of p_sample_loop) for a caller that names its requests by seed.
//
//   Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants) with
//   counter (q, draw, stream, 0), q = element / 4, and key (seed & 0xffffffff, seed >> 32) gives four words;
//   (w0, w1) -> elements 4q, 4q + 1 and (w2, w3) -> elements 4q + 2, 4q + 3 by Box-Muller:
//   u1 = ((wa >> 8) + 1) 2^-24 in (0, 1], u2 = (wb >> 8) 2^-24 in [0, 1), r = sqrt(-2 ln u1), pair = (r cos 2 pi u2, r sin 2 pi u2).
//   u1, u2 and the sincospif argument 2 u2 are exact in fp32; |n| <= sqrt(48 ln 2) = 5.77.
// Accurate logf / sqrtf / sincospif: this file must never be compiled with a fast-math flag.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifdef __FAST_MATH__
#error "philox.h: the noise definition needs the accurate logf / sqrtf / sincospif (no fast-math)"
#endif

__device__ __forceinline__ void rs_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// one Box-Muller pair from two words
__device__ __forceinline__ void rs_box_muller(uint32_t wa, uint32_t wb, float& n0, float& n1) {
    const float u1 = (float)((wa >> 8) + 1u) * 0x1p-24f;
    const float u2 = (float)(wb >> 8) * 0x1p-24f;
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincospif(2.0f * u2, &s, &c);
    n0 = r * c;
    n1 = r * s;
}

// the normals of elements 4q .. 4q + 3 of draw `draw` of the image named by (seed, stream)
__device__ __forceinline__ void rs_noise4(uint64_t seed, uint32_t stream, uint32_t draw, uint32_t q, float n[4]) {
    uint32_t w[4];
    rs_philox4x32_10(q, draw, stream, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    rs_box_muller(w[0], w[1], n[0], n[1]);
    rs_box_muller(w[2], w[3], n[2], n[3]);
}

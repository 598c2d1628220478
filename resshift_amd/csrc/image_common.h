// What the image operators (colorfix, resize, metrics, degrade, jpeg_codec, blur_resize, and the bicubic / noise entries of elementwise)
// have in common: torch's sampling expressions on the device, the argument checks of their C entry points on the host.  Each exists ONCE,
// so "the same bits as the other operator" holds by construction.  Included by the operator files only.
#pragma once
#include "launchers.h"
#include <algorithm>
#include <string>

// ---- device ----------------------------------------------------------------------------------------------------------------------
// torch's `reflect`: the edge sample is not repeated; one reflection is enough for |overhang| < n
__device__ __forceinline__ int img_reflect(int q, int n) {
    if (q < 0) q = -q;
    return q < n ? q : 2 * (n - 1) - q;
}

struct ImgAxis {
    double step;   // source pixels per output pixel: 1 / scale_factor when a scale factor was given, n / m for a size
    int n, m;      // input and output length
};

// F.interpolate(align_corners=False): source coordinate of output index i (fp64), its floor, and the fraction rounded to fp32 once
__device__ __forceinline__ int img_source(const ImgAxis& ax, int i, bool clamp0, float* frac) {
    double s = ax.step * ((double)i + 0.5) - 0.5;
    if (clamp0 && s < 0.0) s = 0.0;
    const double f = floor(s);
    *frac = (float)(s - f);
    return (int)f;
}

// the bilinear tap pair: the first tap (clamped to the axis), the second, and the fraction
__device__ __forceinline__ void img_source2(const ImgAxis& ax, int i, int* i0, int* i1, float* frac) {
    *i0 = min(img_source(ax, i, true, frac), ax.n - 1);
    *i1 = min(*i0 + 1, ax.n - 1);
}

__device__ __forceinline__ float img_bilinear(float v00, float v01, float v10, float v11, float ty, float tx) {
    const float top = fmaf(tx, v01, (1.0f - tx) * v00);
    const float bot = fmaf(tx, v11, (1.0f - tx) * v10);
    return fmaf(ty, bot, (1.0f - ty) * top);
}

__device__ __forceinline__ float img_unit_clamp(float v, int clamp) { return clamp ? fminf(fmaxf(v, 0.0f), 1.0f) : v; }

// Keys' cubic with A = -0.75 (torch's bicubic): |x| <= 1 and 1 < |x| < 2
constexpr float IMG_CUBIC_A = -0.75f;
__device__ __forceinline__ float img_cubic1(float x) { return ((IMG_CUBIC_A + 2.f) * x - (IMG_CUBIC_A + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float img_cubic2(float x) { return ((IMG_CUBIC_A * x - 5.f * IMG_CUBIC_A) * x + 8.f * IMG_CUBIC_A) * x - 4.f * IMG_CUBIC_A; }
// the four weights of the taps floor(src) - 1 .. floor(src) + 2 for the fraction t
__device__ __forceinline__ void img_cubic_weights(float t, float w[4]) {
    w[0] = img_cubic2(t + 1.f);
    w[1] = img_cubic1(t);
    w[2] = img_cubic1(1.f - t);
    w[3] = img_cubic2(2.f - t);
}

// filter2D's LDS images, by all `threads` threads of the workgroup: the k x k kernel kp -> wk, and the mirrored footprint of a rows x cols
// block of filtered samples - the (rows + k - 1) x (cols + k - 1) pixels from (y0, x0), the block's first sample less k / 2, of the H x W
// plane inp -> tile (pitch dwords per row).  The caller's barrier follows.
__device__ __forceinline__ void img_stage_footprint(const float* inp, const float* kp, float* tile, float* wk, int pitch, int y0, int x0, int rows,
                                                    int cols, int k, int p, int H, int W, int tid, int threads) {
    for (int i = tid; i < k * k; i += threads) wk[i] = kp[i];
    const int sr = rows + k - 1, sc = cols + k - 1;      // staged rows / columns: the sources reach at most k / 2 past the image
    for (int i = tid; i < sr * sc; i += threads) {
        const int y = i / sc, x = i - y * sc;
        tile[y * pitch + x] = inp[(long long)img_reflect(y0 - p + y, H) * W + img_reflect(x0 - p + x, W)];
    }
}

// ---- host: the argument checks of the C entry points (the texts stay with the callers) ---------------------------------------------
static inline int img_fail(const std::string& who, const std::string& text) { return rs_set_last_error((who + text).c_str(), -2); }

static inline bool img_overlaps(const void* a, size_t bytes_a, const void* b, size_t bytes_b) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + bytes_a, b0 = (uintptr_t)b, b1 = b0 + bytes_b;
    return b0 < a1 && a0 < b1;
}

// a side of at most 2^28 and at most 2^40 pixels: what the operators' int / long long index arithmetic was written for
static inline bool img_plane_fits(int H, int W) { return std::max(H, W) <= (1 << 28) && (long long)H * W <= (1LL << 40); }

static inline bool img_is_flag(int v) { return v == 0 || v == 1; }

// The packed weight formats, host arrays in and host arrays out: no engine state, no HIP runtime call (tests/weight_pack_check.cpp runs
// them without a device).  The model packer (model.hip) and the op-level test entries (ops.hip) both pack through these functions, so the
// engine path and the test path cannot disagree about a byte.
//
// `w` is always the reference tensor [Cout][Cin][KH*KW] (taps = KH*KW).  Row forms are [Cout][K], K = taps * CinP, column k = tap * CinP + ci
// (IGemmParams::w); channels ci >= Cin of a padded row are left untouched: the caller's buffer is zero-initialised.
#pragma once
#include "common.h"
#include <cmath>
#include <algorithm>
#include <cstddef>
#include <vector>

// what a row packer saw, for the caller's policy (Model::add_conv: fp16 range, split precision, the |w| >= 30 flag)
struct PackStat { float max_abs = 0.f; bool non_finite = false; };

// THE row-form index walk: put(co, k, w) for every element, k = tap * CinP + ci
template <class Put>
static inline PackStat rs_pack_rows(const float* w, int Cout, int Cin, int taps, int CinP, Put put) {
    PackStat s;
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci)
            for (int t = 0; t < taps; ++t) {
                const float wv = w[((size_t)co * Cin + ci) * taps + t];
                if (!std::isfinite(wv)) s.non_finite = true;
                else s.max_abs = std::fmax(s.max_abs, std::fabs(wv));
                put(co, (size_t)t * CinP + ci, wv);
            }
    return s;
}
static inline PackStat rs_pack_rows_f32(const float* w, int Cout, int Cin, int taps, int CinP, float* o) {
    const size_t K = (size_t)taps * CinP;
    return rs_pack_rows(w, Cout, Cin, taps, CinP, [=](int co, size_t k, float wv) { o[co * K + k] = wv; });
}
static inline PackStat rs_pack_rows_f16(const float* w, int Cout, int Cin, int taps, int CinP, f16* o) {
    const size_t K = (size_t)taps * CinP;
    return rs_pack_rows(w, Cout, Cin, taps, CinP, [=](int co, size_t k, float wv) { o[co * K + k] = (f16)wv; });
}
// split storage: [Cout][K hi | K lo], lo = (w - hi) * 2^11 (common.h)
static inline PackStat rs_pack_rows_split(const float* w, int Cout, int Cin, int taps, int CinP, f16* o) {
    const size_t K = (size_t)taps * CinP;
    return rs_pack_rows(w, Cout, Cin, taps, CinP, [=](int co, size_t k, float wv) { rs_split(wv, o[co * 2 * K + k], o[co * 2 * K + K + k]); });
}
// fp32 [tap][Cin][Cout] (DirectConvParams::w, the fused head kernel of direct_conv.hip)
static inline void rs_pack_tap_major(const float* w, int Cout, int Cin, int taps, float* o) {
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci)
            for (int t = 0; t < taps; ++t) o[((size_t)t * Cin + ci) * Cout + co] = w[((size_t)co * Cin + ci) * taps + t];
}

// Fragment-major order of a [N][K] weight (ConvW::wh_frag / ws_frag): element e of lane (lr = lane & 15, lg = lane >> 4) of (16-row block
// nb, k step ks) is W[16 nb + lr][32 ks + 8 lg + e].  `hi(n, k)` / `lo(n, k)` fetch the fp16 planes; with a lo plane every (nb, ks) holds
// 1 KB of hi followed by 1 KB of lo.
template <class FH, class FL>
static inline void frag_major_fill(int N, int K, f16* dst, bool with_lo, FH hi, FL lo) {
    const int KS = K / 32, parts = with_lo ? 2 : 1;
    for (int nb = 0; nb < N / 16; ++nb)
        for (int ks = 0; ks < KS; ++ks)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 8; ++e) {
                    const int n = 16 * nb + (lane & 15), k = 32 * ks + 8 * (lane >> 4) + e;
                    const size_t o = (((size_t)(nb * KS + ks) * parts) * 64 + lane) * 8 + e;
                    dst[o] = hi(n, k);
                    if (with_lo) dst[o + 512] = lo(n, k);
                }
}
// from the reference fp32 weight: fp16 copy (out16) or split (hi, lo) copy (outsplit), rounded by the casts of the row packers
static inline void rs_pack_frag_major(const float* w, int N, int K, f16* out16, f16* outsplit) {
    if (out16) frag_major_fill(N, K, out16, false, [&](int n, int k) { return (f16)w[(size_t)n * K + k]; }, [&](int, int) { return (f16)0.f; });
    if (outsplit)
        frag_major_fill(N, K, outsplit, true, [&](int n, int k) { f16 h, l; rs_split(w[(size_t)n * K + k], h, l); return h; },
                        [&](int n, int k) { f16 h, l; rs_split(w[(size_t)n * K + k], h, l); return l; });
}

// Swin relative position bias (swin_transformer.py:93-102): row of the [225][heads] table that query token i and key token j of an 8 x 8
// window share
static inline int rs_rel_pos_index(int i, int j) { return ((i >> 3) - (j >> 3) + 7) * 15 + ((i & 7) - (j & 7) + 7); }
// bias_t [h][key j][query i] (WinAttnParams::bias_t) and bias_n [h][query i][key j] (bias_n): heads * 4096 floats each
static inline void rs_pack_bias_tables(const float* table, int heads, float* bias_t, float* bias_n) {
    for (int h = 0; h < heads; ++h)
        for (int i = 0; i < 64; ++i)
            for (int j = 0; j < 64; ++j) {
                const float v = table[(size_t)rs_rel_pos_index(i, j) * heads + h];
                if (bias_t) bias_t[((size_t)h * 64 + j) * 64 + i] = v;
                if (bias_n) bias_n[((size_t)h * 64 + i) * 64 + j] = v;
            }
}
// compact form for the split fused kernel (WinAttnParams::bias_c): the table itself, head-major, in units of log2; heads * 256 floats
static inline void rs_pack_bias_compact(const float* table, int heads, float* bias_c) {
    for (int h = 0; h < heads; ++h)
        for (int k = 0; k < 256; ++k) bias_c[h * 256 + k] = k < 225 ? table[(size_t)k * heads + h] * 1.44269504088896f : 0.0f;
}

// Sub-pixel form of "nearest x2 upsample, then conv3x3" (Model::add_upfold): the [C][C][2][2] weight of output parity (py, px) - the taps
// of w [C][C][3][3] that land on the same source pixel added up front, in double
static inline std::vector<float> rs_subpixel_weight(const float* w, int C, int py, int px) {
    // taps of one axis that land on source offset d (relative to y - 1 + par)
    auto taps = [](int par, int d, int (&k)[2]) -> int {
        int n = 0;
        for (int kk = 0; kk < 3; ++kk) {
            const int src = (par + kk - 1) >> 1;            // relative to y (arithmetic shift: -1 >> 1 = -1)
            if (src - (par - 1) == d) k[n++] = kk;
        }
        return n;
    };
    std::vector<float> out((size_t)C * C * 4, 0.f);
    for (int co = 0; co < C; ++co)
        for (int ci = 0; ci < C; ++ci) {
            const float* w9 = w + ((size_t)co * C + ci) * 9;
            for (int dy = 0; dy < 2; ++dy)
                for (int dx = 0; dx < 2; ++dx) {
                    int ky[2], kx[2];
                    const int ny = taps(py, dy, ky), nx = taps(px, dx, kx);
                    double a = 0.0;
                    for (int i = 0; i < ny; ++i)
                        for (int j = 0; j < nx; ++j) a += (double)w9[ky[i] * 3 + kx[j]];
                    out[((size_t)co * C + ci) * 4 + dy * 2 + dx] = (float)a;
                }
        }
    return out;
}

// patch_unembed folded into the last Swin block's MLP (Model::add_basiclayer): y = Wu (x + W2 h + b2) + bu = [Wu W2 | Wu] [h ; x] +
// (Wu b2 + bu).  wu [C][E], w2 [E][hidden] -> [C][hidden + E]; products in double
static inline std::vector<float> rs_unembed_fold_weight(const float* wu, const float* w2, int C, int E, int hidden) {
    std::vector<float> out((size_t)C * (hidden + E), 0.f);
    std::vector<double> row(hidden);
    for (int n = 0; n < C; ++n) {
        std::fill(row.begin(), row.end(), 0.0);
        for (int e = 0; e < E; ++e) {
            const double a = wu[(size_t)n * E + e];
            const float* w2r = w2 + (size_t)e * hidden;
            for (int h = 0; h < hidden; ++h) row[h] += a * (double)w2r[h];
        }
        float* o = out.data() + (size_t)n * (hidden + E);
        for (int h = 0; h < hidden; ++h) o[h] = (float)row[h];
        for (int e = 0; e < E; ++e) o[hidden + e] = wu[(size_t)n * E + e];
    }
    return out;
}
static inline std::vector<float> rs_unembed_fold_bias(const float* wu, const float* bu, const float* b2, int C, int E) {
    std::vector<float> out(C);
    for (int n = 0; n < C; ++n) {
        double a = bu[n];
        for (int e = 0; e < E; ++e) a += (double)wu[(size_t)n * E + e] * (double)b2[e];
        out[n] = (float)a;
    }
    return out;
}

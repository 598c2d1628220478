// Colour correction of a sampled image against its low-quality input (include/resshift_hip.h "colour correction").
//
// wavelet: out = clamp(sr - L(sr - up(lq))), L = five a-trous levels of the separable 1-2-1 kernel (dilations 1, 2, 4, 8, 16, replicate
//          padding of each level's own input).  ONE launch, no intermediate tensor in HBM: a workgroup owns a 64 x 64 output tile of one
//          (image, channel) plane, builds D = sr - up(lq) over the tile plus its 31-pixel halo in LDS (the 16 bicubic taps are gathered
//          from the LR plane, which stays in cache), runs the ten 1-D passes between two LDS buffers and writes its tile.
// adain:   out = clamp((sr - mean_sr) * std_lq / std_sr + mean_lq) per (image, channel) plane.  A statistics launch leaves one
//          (mean, centred sum of squares) pair per 8192-element chunk of every plane; the apply launch merges a plane's pairs in a fixed
//          order (Chan's update, fp64) and applies the affine.  No E[x^2] - mean^2, no floating-point atomics.
#include "image_common.h"

// ---- wavelet -------------------------------------------------------------------------------------------------------------------
// LDS image of a tile: rows / columns [tile origin - 31, tile origin + 64 + 31) of the plane, local index = global index - origin; only
// positions inside the image are ever written or read (every tap index is clamped to the image first).  After the level of dilation d
// the values within `margin - d` of the tile are those of the whole-image definition: 31 -> 30 -> 28 -> 24 -> 16 -> 0.
// Lanes run along a row in every pass (load, horizontal, vertical, store), so the LDS accesses of a wave are consecutive dwords -
// conflict-free at any row pitch; 128 keeps the rows 512-byte aligned.  2 buffers x 126 rows x 128 floats = 126 KiB of the CU's 160.
constexpr int CF_TILE = 64;
constexpr int CF_HALO = 31;
constexpr int CF_R = CF_TILE + 2 * CF_HALO;   // 126
constexpr int CF_PITCH = 128;
constexpr int CF_THREADS = 1024;
constexpr int CF_LDS_BYTES = 2 * CF_R * CF_PITCH * (int)sizeof(float);
// rows of the load phase / elements of a level pass a thread has in flight per iteration (A/B builds: -DCF_LOAD_ROWS=1 -DCF_PASS_UNROLL=1)
#ifndef CF_LOAD_ROWS
#define CF_LOAD_ROWS 4
#endif
#ifndef CF_PASS_UNROLL
#define CF_PASS_UNROLL 4
#endif

// the one expression of a 1-2-1 tap triple, for every pixel of every workgroup: (a + c) is symmetric in the two outer taps and the
// scalings are exact, so the value is a function of the three inputs alone
__device__ __forceinline__ float cf_121(float a, float b, float c) { return fmaf(0.25f, a + c, 0.5f * b); }

// tap weights and first tap index of output coordinate o (bicubic_up_kernel's expressions, elementwise.hip)
__device__ __forceinline__ int cf_bicubic_taps(int o, float rs, float* w) {
    const float f = ((float)o + 0.5f) * rs - 0.5f;
    const float ff = floorf(f);
    const float t = f - ff;
    img_cubic_weights(t, w);
    return (int)ff - 1;
}

// one level: horizontal pass a -> b over the rows the vertical pass will read, vertical pass b -> a.  MB = valid margin before the level.
template <int D, int MB>
__device__ __forceinline__ void cf_level(float* a, float* b, int ox0, int oy0, int Wo, int Ho) {
    constexpr int MA = MB - D;
    constexpr int NC = CF_TILE + 2 * MA;        // columns of both passes
    constexpr int NRH = CF_TILE + 2 * MB;       // rows of the horizontal pass
    // CF_PASS_UNROLL elements per thread and iteration: their LDS reads are issued together.  An element outside the rectangle or the
    // image reads at its position clamped into both (always inside the LDS image) and stores nothing.
    for (int i0 = threadIdx.x; i0 < NRH * NC; i0 += CF_THREADS * CF_PASS_UNROLL) {
        float v[CF_PASS_UNROLL];
#pragma unroll
        for (int u = 0; u < CF_PASS_UNROLL; ++u) {
            const int i = min(i0 + u * CF_THREADS, NRH * NC - 1);
            const int r = CF_HALO - MB + i / NC, c = CF_HALO - MA + i % NC;
            const int gy = min(max(oy0 + r, 0), Ho - 1), gx = min(max(ox0 + c, 0), Wo - 1);
            const float* row = a + (gy - oy0) * CF_PITCH - ox0;
            v[u] = cf_121(row[max(gx - D, 0)], row[gx], row[min(gx + D, Wo - 1)]);
        }
#pragma unroll
        for (int u = 0; u < CF_PASS_UNROLL; ++u) {
            const int i = i0 + u * CF_THREADS;
            const int r = CF_HALO - MB + i / NC, c = CF_HALO - MA + i % NC;
            const int gy = oy0 + r, gx = ox0 + c;
            if (i < NRH * NC && gy >= 0 && gy < Ho && gx >= 0 && gx < Wo) b[r * CF_PITCH + c] = v[u];
        }
    }
    __syncthreads();
    for (int i0 = threadIdx.x; i0 < NC * NC; i0 += CF_THREADS * CF_PASS_UNROLL) {
        float v[CF_PASS_UNROLL];
#pragma unroll
        for (int u = 0; u < CF_PASS_UNROLL; ++u) {
            const int i = min(i0 + u * CF_THREADS, NC * NC - 1);
            const int r = CF_HALO - MA + i / NC, c = CF_HALO - MA + i % NC;
            const int gy = min(max(oy0 + r, 0), Ho - 1), gx = min(max(ox0 + c, 0), Wo - 1);
            const float* col = b - oy0 * CF_PITCH + (gx - ox0);
            v[u] = cf_121(col[max(gy - D, 0) * CF_PITCH], col[gy * CF_PITCH], col[min(gy + D, Ho - 1) * CF_PITCH]);
        }
#pragma unroll
        for (int u = 0; u < CF_PASS_UNROLL; ++u) {
            const int i = i0 + u * CF_THREADS;
            const int r = CF_HALO - MA + i / NC, c = CF_HALO - MA + i % NC;
            const int gy = oy0 + r, gx = ox0 + c;
            if (i < NC * NC && gy >= 0 && gy < Ho && gx >= 0 && gx < Wo) a[r * CF_PITCH + c] = v[u];
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(CF_THREADS) void colorfix_wavelet_kernel(const float* __restrict__ sr, const float* __restrict__ lq,
                                                                      float* __restrict__ out, int H, int W, int sf, int tiles_x, int tiles_y,
                                                                      long long total) {
    extern __shared__ __attribute__((aligned(16))) float cf_smem[];
    float* a = cf_smem;
    float* b = cf_smem + CF_R * CF_PITCH;
    const int Ho = H * sf, Wo = W * sf;
    const float rs = 1.0f / (float)sf;
    const int lx = threadIdx.x & (CF_PITCH - 1), ly = threadIdx.x / CF_PITCH;   // 128 columns x 8 rows of threads
    for (long long t = blockIdx.x; t < total; t += gridDim.x) {
        const int tx = (int)(t % tiles_x);
        const long long q = t / tiles_x;
        const int ty = (int)(q % tiles_y);
        const long long plane = q / tiles_y;
        const int ox0 = tx * CF_TILE - CF_HALO, oy0 = ty * CF_TILE - CF_HALO;
        const float* srp = sr + plane * Ho * Wo;
        const float* lqp = lq + plane * H * W;
        float* outp = out + plane * Ho * Wo;
        // D = sr - up(lq) over the in-image part of the region; a thread keeps its column's tap weights and indices
        const int gx = ox0 + lx;
        if (lx < CF_R && gx >= 0 && gx < Wo) {
            float wx[4];
            int xi[4];
            if (sf > 1) {
                const int ix = cf_bicubic_taps(gx, rs, wx);
#pragma unroll
                for (int j = 0; j < 4; ++j) xi[j] = min(max(ix + j, 0), W - 1);
            }
            // CF_LOAD_ROWS rows per iteration, so that their 17 loads each are in flight together (a row outside the image loads at the
            // clamped row and stores nothing)
            constexpr int RSTEP = CF_THREADS / CF_PITCH;
            for (int r0 = ly; r0 < CF_R; r0 += RSTEP * CF_LOAD_ROWS) {
                float dv[CF_LOAD_ROWS];
#pragma unroll
                for (int u = 0; u < CF_LOAD_ROWS; ++u) {
                    const int gy = min(max(oy0 + r0 + u * RSTEP, 0), Ho - 1);
                    float up;
                    if (sf > 1) {
                        float wy[4];
                        const int iy = cf_bicubic_taps(gy, rs, wy);
                        up = 0.f;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float* src = lqp + (long long)min(max(iy + i, 0), H - 1) * W;
                            float rr = 0.f;
#pragma unroll
                            for (int j = 0; j < 4; ++j) rr += src[xi[j]] * wx[j];
                            up += rr * wy[i];
                        }
                    } else {
                        up = lqp[(long long)gy * W + gx];
                    }
                    dv[u] = srp[(long long)gy * Wo + gx] - up;
                }
#pragma unroll
                for (int u = 0; u < CF_LOAD_ROWS; ++u) {
                    const int r = r0 + u * RSTEP, gy = oy0 + r;
                    if (r < CF_R && gy >= 0 && gy < Ho) a[r * CF_PITCH + lx] = dv[u];
                }
            }
        }
        __syncthreads();
        cf_level<1, 31>(a, b, ox0, oy0, Wo, Ho);
        cf_level<2, 30>(a, b, ox0, oy0, Wo, Ho);
        cf_level<4, 28>(a, b, ox0, oy0, Wo, Ho);
        cf_level<8, 24>(a, b, ox0, oy0, Wo, Ho);
        cf_level<16, 16>(a, b, ox0, oy0, Wo, Ho);
        // a wave writes one whole 64-pixel row of the tile
        for (int i = threadIdx.x; i < CF_TILE * CF_TILE; i += CF_THREADS) {
            const int r = i / CF_TILE, c = i % CF_TILE;
            const int gy = ty * CF_TILE + r, gxo = tx * CF_TILE + c;
            if (gy >= Ho || gxo >= Wo) continue;
            const long long g = (long long)gy * Wo + gxo;
            outp[g] = fminf(fmaxf(srp[g] - a[(CF_HALO + r) * CF_PITCH + CF_HALO + c], -1.0f), 1.0f);
        }
        __syncthreads();   // (the next tile of this workgroup overwrites `a`)
    }
}

// ---- adain ---------------------------------------------------------------------------------------------------------------------
// A plane of n elements is cut into chunks of CF_CHUNK; chunk s of a plane yields (mean_s, M2_s = sum (x - mean_s)^2), both from the
// values the workgroup holds in registers.  Which thread holds which element, and the order of every sum, depend on the element's index
// in its plane only - not on the batch, the pointer alignment or the grid - so a plane's statistics are the same bits in any call.
constexpr int CF_CHUNK = 8192;
constexpr int CF_ST_THREADS = 256;
constexpr int CF_PER_THREAD = CF_CHUNK / CF_ST_THREADS;   // 32: eight groups of four consecutive elements

__device__ __forceinline__ float cf_block_sum(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();   // (red may still be read from the previous sum)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// the chunk's values: thread t holds elements (k * 256 + t) * 4 + {0, 1, 2, 3}, k = 0 .. 7; zeros past the end
__device__ __forceinline__ void cf_load_chunk(const float* __restrict__ p, int cnt, float* v) {
    const bool vec = ((uintptr_t)p & 15) == 0;
#pragma unroll
    for (int k = 0; k < CF_PER_THREAD / 4; ++k) {
        const int i = (k * CF_ST_THREADS + (int)threadIdx.x) * 4;
        if (vec && i + 3 < cnt) {
            const f32x4 q = *(const f32x4*)(p + i);
            v[4 * k] = q[0]; v[4 * k + 1] = q[1]; v[4 * k + 2] = q[2]; v[4 * k + 3] = q[3];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * k + j] = i + j < cnt ? p[i + j] : 0.f;
        }
    }
}

// part: [planes][S_sr + S_lq][2]
__global__ __launch_bounds__(CF_ST_THREADS) void colorfix_stats_kernel(const float* __restrict__ sr, const float* __restrict__ lq,
                                                                       float* __restrict__ part, long long n_sr, long long n_lq, int S_sr,
                                                                       int S_lq, long long total) {
    __shared__ float red[4];
    const int per = S_sr + S_lq;
    for (long long w = blockIdx.x; w < total; w += gridDim.x) {
        const long long plane = w / per;
        const int s = (int)(w % per);
        const bool is_sr = s < S_sr;
        const long long n = is_sr ? n_sr : n_lq;
        const long long e0 = (long long)(is_sr ? s : s - S_sr) * CF_CHUNK;
        const float* p = (is_sr ? sr + plane * n_sr : lq + plane * n_lq) + e0;
        const int cnt = (int)std::min<long long>(CF_CHUNK, n - e0);
        float v[CF_PER_THREAD];
        cf_load_chunk(p, cnt, v);
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < CF_PER_THREAD; ++k) sum += v[k];
        const float mean = cf_block_sum(sum, red) / (float)cnt;
        float sq = 0.f;
#pragma unroll
        for (int k = 0; k < CF_PER_THREAD; ++k) {
            const int i = ((k / 4) * CF_ST_THREADS + (int)threadIdx.x) * 4 + (k & 3);
            const float d = i < cnt ? v[k] - mean : 0.f;
            sq = fmaf(d, d, sq);
        }
        const float m2 = cf_block_sum(sq, red);
        if (threadIdx.x == 0) { part[w * 2] = mean; part[w * 2 + 1] = m2; }
    }
}

// Chan's update of (count, mean, centred sum of squares) a by b
__device__ __forceinline__ void cf_chan(double& an, double& am, double& aq, double bn, double bm, double bq) {
    if (bn == 0.0) return;
    if (an == 0.0) { an = bn; am = bm; aq = bq; return; }
    const double n = an + bn, d = bm - am;
    am += d * (bn / n);
    aq += bq + d * d * (an * bn / n);
    an = n;
}

// merge of a plane's S partials in a fixed order: thread t folds partials t, t + 256, ... in ascending order, then a binary tree over the
// 256 threads.  All threads call; the result is valid in thread 0.
__device__ __forceinline__ void cf_merge(const float* __restrict__ part, int S, long long n, double* sn, double* sm, double* sq, double& mean,
                                         double& m2) {
    double cn = 0.0, cm = 0.0, cq = 0.0;
    for (int i = threadIdx.x; i < S; i += CF_ST_THREADS)
        cf_chan(cn, cm, cq, (double)std::min<long long>(CF_CHUNK, n - (long long)i * CF_CHUNK), (double)part[2 * i], (double)part[2 * i + 1]);
    __syncthreads();   // (the arrays may still be read from the previous merge)
    sn[threadIdx.x] = cn; sm[threadIdx.x] = cm; sq[threadIdx.x] = cq;
    __syncthreads();
    for (int st = CF_ST_THREADS / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            cf_chan(sn[threadIdx.x], sm[threadIdx.x], sq[threadIdx.x], sn[threadIdx.x + st], sm[threadIdx.x + st], sq[threadIdx.x + st]);
        }
        __syncthreads();
    }
    mean = sm[0];
    m2 = sq[0];
}

__global__ __launch_bounds__(CF_ST_THREADS) void colorfix_adain_apply_kernel(const float* __restrict__ sr, float* __restrict__ out,
                                                                             const float* __restrict__ part, long long n_sr, long long n_lq,
                                                                             int S_sr, int S_lq, long long total) {
    __shared__ double sn[CF_ST_THREADS], sm[CF_ST_THREADS], sq[CF_ST_THREADS];
    __shared__ float coef[3];
    const int per = S_sr + S_lq;
    for (long long w = blockIdx.x; w < total; w += gridDim.x) {
        const long long plane = w / S_sr;
        const int s = (int)(w % S_sr);
        double mean_sr, m2_sr, mean_lq, m2_lq;
        cf_merge(part + plane * per * 2, S_sr, n_sr, sn, sm, sq, mean_sr, m2_sr);
        cf_merge(part + (plane * per + S_sr) * 2, S_lq, n_lq, sn, sm, sq, mean_lq, m2_lq);
        if (threadIdx.x == 0) {
            // unbiased variance (a one-pixel plane: 0) + 1e-5
            const double sd_sr = sqrt(m2_sr / (double)std::max<long long>(n_sr - 1, 1) + 1e-5);
            const double sd_lq = sqrt(m2_lq / (double)std::max<long long>(n_lq - 1, 1) + 1e-5);
            coef[0] = (float)mean_sr; coef[1] = (float)(sd_lq / sd_sr); coef[2] = (float)mean_lq;
        }
        __syncthreads();
        const float mu = coef[0], gain = coef[1], shift = coef[2];
        const long long e0 = (long long)s * CF_CHUNK;
        const float* p = sr + plane * n_sr + e0;
        float* o = out + plane * n_sr + e0;
        const int cnt = (int)std::min<long long>(CF_CHUNK, n_sr - e0);
        const bool vec = (((uintptr_t)p | (uintptr_t)o) & 15) == 0;
#pragma unroll
        for (int k = 0; k < CF_PER_THREAD / 4; ++k) {
            const int i = (k * CF_ST_THREADS + (int)threadIdx.x) * 4;
            if (vec && i + 3 < cnt) {
                f32x4 q = *(const f32x4*)(p + i);
#pragma unroll
                for (int j = 0; j < 4; ++j) q[j] = fminf(fmaxf(fmaf(q[j] - mu, gain, shift), -1.0f), 1.0f);
                *(f32x4*)(o + i) = q;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (i + j < cnt) o[i + j] = fminf(fmaxf(fmaf(p[i + j] - mu, gain, shift), -1.0f), 1.0f);
            }
        }
        __syncthreads();   // (coef is rewritten for the next chunk of this workgroup)
    }
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------
extern "C" {


static inline int cf_chunks(long long n) { return (int)((n + CF_CHUNK - 1) / CF_CHUNK); }
// what both entry points ask of the geometry; nullptr when it is fine
static const char* cf_geometry_error(int B, int C, int H, int W, int sf, int mode) {
    if (B < 1 || C < 1 || H < 1 || W < 1) return "B, C, H and W must be positive";
    if (sf < 1) return "sf must be positive";
    if (mode != RS_COLOR_FIX_WAVELET && mode != RS_COLOR_FIX_ADAIN) return "unknown mode (RS_COLOR_FIX_WAVELET or RS_COLOR_FIX_ADAIN)";
    if ((long long)H * sf > (1 << 30) || (long long)W * sf > (1 << 30) || (long long)H * sf * W * sf > (1LL << 40))
        return "the output plane is too large (a side above 2^30 or more than 2^40 pixels)";
    return nullptr;
}

size_t rs_color_fix_work_bytes(int B, int C, int H, int W, int sf, int mode) {
    if (cf_geometry_error(B, C, H, W, sf, mode) || mode != RS_COLOR_FIX_ADAIN) return 0;
    const long long n_lq = (long long)H * W, n_sr = n_lq * sf * sf;
    return (size_t)B * C * (size_t)(cf_chunks(n_sr) + cf_chunks(n_lq)) * 2 * sizeof(float);
}

int rs_color_fix(const float* sr, const float* lq, float* out, int B, int C, int H, int W, int sf, int mode, void* work, size_t work_bytes,
                 void* stream) {
    static RsAttrFlags attr_flags;
    const std::string who = "rs_color_fix: ";
    if (!sr || !lq || !out) return img_fail(who, "null tensor (sr / lq / out)");
    if (const char* e = cf_geometry_error(B, C, H, W, sf, mode)) return img_fail(who, e);
    const long long planes = (long long)B * C, n_lq = (long long)H * W, n_sr = n_lq * sf * sf;
    const size_t sr_bytes = planes * n_sr * sizeof(float);
    if (img_overlaps(out, sr_bytes, sr, sr_bytes) || img_overlaps(out, sr_bytes, lq, planes * n_lq * sizeof(float)))
        return img_fail(who, "`out` overlaps `sr` or `lq` (workgroups read their neighbours' pixels of sr: not in place)");
    const size_t need = rs_color_fix_work_bytes(B, C, H, W, sf, mode);
    if (need && (!work || work_bytes < need))
        return img_fail(who, "the workspace is too small: " + std::to_string(work ? work_bytes : 0) + " bytes, rs_color_fix_work_bytes asks for " +
                                  std::to_string(need));
    if (need && ((uintptr_t)work & 3)) return img_fail(who, "the workspace must be aligned to 4 bytes");
    const hipStream_t st = (hipStream_t)stream;
    if (mode == RS_COLOR_FIX_WAVELET) {
        const int tiles_x = (W * sf + CF_TILE - 1) / CF_TILE, tiles_y = (H * sf + CF_TILE - 1) / CF_TILE;
        const long long total = planes * tiles_x * tiles_y;
        if (attr_flags.need())
            (void)hipFuncSetAttribute((const void*)colorfix_wavelet_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, CF_LDS_BYTES);
        hipLaunchKernelGGL(colorfix_wavelet_kernel, dim3((unsigned)std::min<long long>(total, 1 << 20)), dim3(CF_THREADS), CF_LDS_BYTES, st, sr, lq,
                           out, H, W, sf, tiles_x, tiles_y, total);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    const int S_sr = cf_chunks(n_sr), S_lq = cf_chunks(n_lq);
    const long long t_stats = planes * (S_sr + S_lq), t_apply = planes * S_sr;
    hipLaunchKernelGGL(colorfix_stats_kernel, dim3((unsigned)std::min<long long>(t_stats, 1 << 20)), dim3(CF_ST_THREADS), 0, st, sr, lq, (float*)work,
                       n_sr, n_lq, S_sr, S_lq, t_stats);
    hipLaunchKernelGGL(colorfix_adain_apply_kernel, dim3((unsigned)std::min<long long>(t_apply, 1 << 20)), dim3(CF_ST_THREADS), 0, st, sr, out,
                       (const float*)work, n_sr, n_lq, S_sr, S_lq, t_apply);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}   // extern "C"

// Sampler-side elementwise kernels, layout conversion, bicubic upsampling and the VQ lookup.
//
//   layout:   reference tensors are NCHW fp32 (sampler.py / gaussian_diffusion.py); the engine is NHWC.
//   sampler:  prior_sample gaussian_diffusion.py:517-529; _scale_input :598-609; posterior mean
//             :210-221; p_sample noise add :358-364.
//   bicubic:  F.interpolate(mode='bicubic') gaussian_diffusion.py:503-504 (align_corners=False,
//             A=-0.75, border-clamped taps, no antialias).
//   VQ:       VectorQuantizer2.forward ldm/modules/vqvae/quantize.py:271-312 (expanded-form distance,
//             first-minimum argmin, straight-through expression z + (z_q - z)).
#include "image_common.h"
#include "philox.h"
#include <cmath>

namespace {

template <typename TO>
__global__ void nchw_to_nhwc_kernel(const float* in, TO* out, int B, int C, int HW, int ldo, int coff, float scale) {
    const long long n = (long long)B * C * HW;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(g % C);
        const long long bp = g / C;  // b*HW + pix
        const long long b = bp / HW;
        const long long pix = bp - b * HW;
        rs_st<TO>(out + bp * ldo * Store<TO>::PM + coff + c, ldo, in[(b * C + c) * HW + pix] * scale);
    }
}

// the same with one scale per image (by value: RS_MAX_ROWS images) - _scale_input of a batch whose images are at different steps, in the
// same expression as the scalar kernel's (the split-storage store sees the same product)
struct RowScale { float a[RS_MAX_ROWS]; };
template <typename TO>
__global__ void nchw_to_nhwc_rows_kernel(const float* in, TO* out, int B, int C, int HW, int ldo, int coff, RowScale s) {
    const long long n = (long long)B * C * HW;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(g % C);
        const long long bp = g / C;  // b*HW + pix
        const long long b = bp / HW;
        const long long pix = bp - b * HW;
        rs_st<TO>(out + bp * ldo * Store<TO>::PM + coff + c, ldo, in[(b * C + c) * HW + pix] * s.a[b]);
    }
}

template <typename TI>
__global__ void nhwc_to_nchw_kernel(const TI* in, float* out, int B, int C, int HW, int ldi, int coff) {
    const long long n = (long long)B * C * HW;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long long)gridDim.x * blockDim.x) {
        const long long pix = g % HW;
        const long long bc = g / HW;
        const long long c = bc % C, b = bc / C;
        out[g] = rs_ld<TI>(in + (b * HW + pix) * ldi * Store<TI>::PM + coff + c, ldi);
    }
}

// channel-block copy between NHWC tensors of one storage type (8 channels = one 16-byte chunk per thread; C % 8 == 0)
template <typename T>
__global__ void copy_channels_kernel(const T* src, int lds_, T* dst, int ldd, int C, long long npix) {
    const int nch = C >> 3;
    const long long n = npix * nch;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long long)gridDim.x * blockDim.x) {
        const long long pix = g / nch;
        const int c = (int)(g - pix * nch) * 8;
        Vec8<T> v;
        v.load(src + pix * lds_ * Store<T>::PM + c, lds_);
        v.store(dst + pix * ldd * Store<T>::PM + c, ldd);
    }
}

// storage conversion [npix][C] -> [npix][C] (dense tensors)
template <typename TI, typename TO>
__global__ void convert_kernel(const TI* src, TO* dst, int C, long long npix) {
    const long long n = npix * C;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long long)gridDim.x * blockDim.x) {
        const long long pix = g / C;
        const int c = (int)(g - pix * C);
        rs_st<TO>(dst + pix * C * Store<TO>::PM + c, C, rs_ld<TI>(src + pix * C * Store<TI>::PM + c, C));
    }
}

// the combine expression of every kernel of this family (tensor noise or generated noise): v = a x [+ b z] [+ c n].  ONE definition, so that
// a seeded step is bit for bit the tensor step fed with noise_fill_kernel's output.  One rounded product, then one fused multiply-add
// per further term - spelled with fmaf, so that the roundings do not depend on how the compiler contracts or if-converts a kernel's loop
// (they are the roundings `v = a * x; v += b * z; v += c * n` has always compiled to here: v_mul_f32, v_fmac_f32, v_fmac_f32).
__device__ __forceinline__ float axpbypcz_combine(float a, float x, bool has_z, float b, float z, bool has_n, float c, float n) {
    float v = a * x;
    if (has_z) v = fmaf(b, z, v);
    if (has_n) v = fmaf(c, n, v);
    return v;
}

// y = a*x + b*z + c*n   (all fp32, any layout as long as all operands share it)
__global__ void axpbypcz_kernel(const float* x, const float* z, const float* n, float* y, float a, float b, float c, long long cnt) {
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < cnt; g += (long long)gridDim.x * blockDim.x)
        y[g] = axpbypcz_combine(a, x[g], z != nullptr, b, z ? z[g] : 0.f, n != nullptr, c, n ? n[g] : 0.f);
}

// the same with one (a, b, c) per image: image r = g / per covers elements [r * per, (r + 1) * per).  The coefficients travel by value
// (kernel arguments, RS_MAX_ROWS images), so a mixed-timestep step needs no host round trip; the expressions are those of axpbypcz_kernel,
// so an image gets bit for bit what the scalar kernel gives it.  c == 0 (t = 0, models/gaussian_diffusion.py:358-364) skips the noise
// term, as the scalar path does with n == nullptr.
struct RowCoefs { float a[RS_MAX_ROWS], b[RS_MAX_ROWS], c[RS_MAX_ROWS]; };
__global__ void axpbypcz_rows_kernel(const float* x, const float* z, const float* n, float* y, RowCoefs k, long long per, long long cnt) {
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < cnt; g += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(g / per);
        const bool has_n = n && k.c[r] != 0.f;
        y[g] = axpbypcz_combine(k.a[r], x[g], z != nullptr, k.b[r], z ? z[g] : 0.f, has_n, k.c[r], has_n ? n[g] : 0.f);
    }
}

// ---- per-request seeds (philox.h) ---------------------------------------------------------------------
// Keys and draw indices travel by value next to RowCoefs (64 x 16 B + 64 x 4 B); blockIdx.y is the image, so key, draw and
// coefficients are wave-uniform.  A batch of more than RS_MAX_ROWS images (rs_sample_seeded: every image at one step) reads its keys
// from `kdev` (device copy) and shares row 0 of the coefficients and draws.
struct RowKeys { rs_noise_key k[RS_MAX_ROWS]; int draw[RS_MAX_ROWS]; };

// out[b][i] = normal i of draw nk.draw[b] of key nk.k[b]: the specification made callable.  Thread = one Philox call = four elements;
// V4: per % 4 == 0 and a 16-byte aligned `out` (one 16-byte store), else element by element (a latent that is no multiple of 4 drops
// the surplus).
template <bool V4>
__global__ __launch_bounds__(256) void noise_fill_kernel(float* out, RowKeys nk, long long per) {
    const int b = blockIdx.y;
    const rs_noise_key key = nk.k[b];
    const uint32_t draw = (uint32_t)nk.draw[b];
    float* o = out + (long long)b * per;
    const long long nq = (per + 3) / 4;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long long)gridDim.x * blockDim.x) {
        float n[4];
        rs_noise4(key.seed, key.stream, draw, (uint32_t)q, n);
        if constexpr (V4) {
            f32x4 v = {n[0], n[1], n[2], n[3]};
            *(f32x4*)(o + 4 * q) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * q + e < per) o[4 * q + e] = n[e];
        }
    }
}

// y = a[b] x + b[b] z + c[b] n(key[b], draw[b]) per image b: axpbypcz_rows_kernel with the noise made in registers.  c[b] == 0 (an
// image at t = 0) skips the generator.  In place (y == x) is fine: a thread reads its own four elements before it writes them.
template <bool V4>
__global__ __launch_bounds__(256) void axpbypcz_seeded_kernel(const float* x, const float* z, float* y, RowCoefs k, RowKeys nk,
                                                              const rs_noise_key* kdev, int uniform, long long per) {
    const int b = blockIdx.y, r = uniform ? 0 : b;
    const rs_noise_key key = kdev ? kdev[b] : nk.k[b];
    const uint32_t draw = (uint32_t)nk.draw[r];
    const float ca = k.a[r], cb = k.b[r], cc = k.c[r];
    const bool has_z = z != nullptr, has_n = cc != 0.f;
    const long long base = (long long)b * per, nq = (per + 3) / 4;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long long)gridDim.x * blockDim.x) {
        float n[4] = {0.f, 0.f, 0.f, 0.f};
        if (has_n) rs_noise4(key.seed, key.stream, draw, (uint32_t)q, n);
        const long long g = base + 4 * q;
        if constexpr (V4) {
            const f32x4 xv = *(const f32x4*)(x + g);
            f32x4 zv = {0.f, 0.f, 0.f, 0.f};
            if (has_z) zv = *(const f32x4*)(z + g);
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = axpbypcz_combine(ca, xv[e], has_z, cb, zv[e], has_n, cc, n[e]);
            *(f32x4*)(y + g) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * q + e < per) y[g + e] = axpbypcz_combine(ca, x[g + e], has_z, cb, has_z ? z[g + e] : 0.f, has_n, cc, n[e]);
        }
    }
}

// out = x + c[b] n per image b of an fp32 NCHW batch, optionally clamped to [0, 1]: the Gaussian noise of the degradation recipe (DESIGN.md
// 7h; basicsr/data/degradations.py add_gaussian_noise_pt with c = sigma / 255).  n = the normals noise_fill_kernel writes for the draw
// nk.draw[b] of key nk.k[b] and the shape (C, H, W) - or, for an image with gray[b] set, for the shape (1, H, W), shared by its channels.
// Thread = one Philox call = four noise elements.  The product and the sum are rounded separately (non-contracting intrinsics), as the
// reference's tensor operations round them.
struct NoiseRows { float c[RS_MAX_ROWS]; unsigned char gray[RS_MAX_ROWS]; };
__global__ __launch_bounds__(256) void add_noise_kernel(const float* __restrict__ x, float* __restrict__ out, NoiseRows k, RowKeys nk, int C, long long HW,
                                                        int clamp) {
    const int b = blockIdx.y;
    const rs_noise_key key = nk.k[b];
    const uint32_t draw = (uint32_t)nk.draw[b];
    const float c = k.c[b];
    const bool gray = k.gray[b] != 0;
    const long long base = (long long)b * C * HW, per = gray ? HW : C * HW, nq = (per + 3) / 4;
    const int reps = gray ? C : 1;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long long)gridDim.x * blockDim.x) {
        float n[4];
        rs_noise4(key.seed, key.stream, draw, (uint32_t)q, n);
        for (int ch = 0; ch < reps; ++ch)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long long i = 4 * q + e;
                if (i < per) {
                    float v = __fadd_rn(x[base + ch * HW + i], __fmul_rn(c, n[e]));
                    if (clamp) v = fminf(fmaxf(v, 0.0f), 1.0f);
                    out[base + ch * HW + i] = v;
                }
            }
    }
}

// planar fp32 [B,C,H,W] in [0,1] -> interleaved uint8 [B,H,W,C]: clamp, * 255, round half to even (rs_unit_to_u8 of common.h)
__global__ void unit_to_u8_kernel(const float* __restrict__ src, unsigned char* __restrict__ dst, long long npix, long long HW, int C) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long long)gridDim.x * blockDim.x) {
        const long long b = i / HW, hw = i - b * HW;
        for (int c = 0; c < C; ++c) dst[i * C + c] = rs_unit_to_u8(src[(b * C + c) * HW + hw]);
    }
}

// per-image FiLM table [B][total] gathered from cached per-timestep rows (one pointer per image, by value)
struct FilmRows { const float* row[RS_MAX_ROWS]; };
__global__ void film_gather_kernel(FilmRows s, float* out, int total, long long cnt) {
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < cnt; g += (long long)gridDim.x * blockDim.x) {
        const long long b = g / total;
        out[g] = s.row[b][g - b * total];
    }
}

__global__ void clamp_kernel(float* x, float lo, float hi, long long cnt) {
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < cnt; g += (long long)gridDim.x * blockDim.x)
        x[g] = fminf(fmaxf(x[g], lo), hi);
}

template <typename T>
__global__ void silu_kernel(const T* x, T* y, long long cnt) {
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < cnt; g += (long long)gridDim.x * blockDim.x)
        y[g] = (T)rs_silu((float)x[g]);
}

// out[r][n] = bias[n] + sum_k act_in(x[r][k]) * w[n][k]   (tiny fp32 linears: time embedding / FiLM tables).
// One wavefront per output: lanes stride over K (coalesced weight reads), fixed-order butterfly reduction.
__global__ __launch_bounds__(256) void small_linear_kernel(const float* x, const float* w, const float* bias, float* y, int R, int K, int N,
                                                           int silu_in, int silu_out) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);   // output index, one per wave
    if (g >= (long long)R * N) return;
    const int r = (int)(g / N), n = (int)(g - (long long)r * N);
    float acc = 0.f;
    for (int k = lane; k < K; k += 64) {
        float xv = x[(long long)r * K + k];
        if (silu_in) xv = xv / (1.0f + expf(-xv));
        acc = fmaf(xv, w[(long long)n * K + k], acc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) {
        acc += bias ? bias[n] : 0.f;
        if (silu_out) acc = acc / (1.0f + expf(-acc));
        y[g] = acc;
    }
}

// ---- bicubic ----------------------------------------------------------------
// in: NCHW fp32 [B,C,H,W]; out: NHWC TO [B,H*sf,W*sf,ldo] channels [0,C)
template <typename TO>
__global__ void bicubic_up_kernel(const float* in, TO* out, int B, int C, int H, int W, int sf, int ldo) {
    const int Ho = H * sf, Wo = W * sf;
    const long long n = (long long)B * Ho * Wo * C;
    const float rs = 1.0f / (float)sf;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(g % C);
        long long t = g / C;
        const int ox = (int)(t % Wo); t /= Wo;
        const int oy = (int)(t % Ho);
        const int b = (int)(t / Ho);
        const float fy = ((float)oy + 0.5f) * rs - 0.5f;
        const float fx = ((float)ox + 0.5f) * rs - 0.5f;
        const float fyf = floorf(fy), fxf = floorf(fx);
        const int iy = (int)fyf, ix = (int)fxf;
        const float ty = fy - fyf, tx = fx - fxf;
        float wy[4], wx[4];
        img_cubic_weights(ty, wy);
        img_cubic_weights(tx, wx);
        const float* src = in + ((long long)b * C + c) * H * W;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int yy = min(max(iy - 1 + i, 0), H - 1);
            float r = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int xx = min(max(ix - 1 + j, 0), W - 1);
                r += src[(long long)yy * W + xx] * wx[j];
            }
            acc += r * wy[i];
        }
        rs_st<TO>(out + (((long long)b * Ho + oy) * Wo + ox) * ldo * Store<TO>::PM + c, ldo, acc);
    }
}

// ---- VQ nearest codebook entry ------------------------------------------------
// z: [N][D] fp32 (NHWC latent, D = embed_dim), codebook E: [NE][D].  One thread per token; the
// codebook and its squared norms live in LDS.  d_j = (|z|^2 + |e_j|^2) - 2 z.e_j evaluated in fp32
// in the reference's order; strict '<' keeps the first minimum like torch.argmin.
template <int D>
__global__ __launch_bounds__(256) void vq_nearest_kernel(const float* z, const float* cb, float* zq, int* idx_out, long long N, int NE) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* e = (float*)smem;        // [NE][D]
    float* ee = e + (long long)NE * D;  // [NE]
    for (int i = threadIdx.x; i < NE * D; i += blockDim.x) e[i] = cb[i];
    __syncthreads();
    for (int j = threadIdx.x; j < NE; j += blockDim.x) {
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) s = __fadd_rn(s, __fmul_rn(e[j * D + d], e[j * D + d]));
        ee[j] = s;
    }
    __syncthreads();
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    float zv[D];
    float zz = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) { zv[d] = z[t * D + d]; zz = __fadd_rn(zz, __fmul_rn(zv[d], zv[d])); }
    float best = 3.4e38f;
    int bi = 0;
    for (int j = 0; j < NE; ++j) {
        float dot = 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) dot = fmaf(zv[d], e[j * D + d], dot);
        const float dist = __fsub_rn(__fadd_rn(zz, ee[j]), __fmul_rn(2.0f, dot));
        if (dist < best) { best = dist; bi = j; }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float q = e[bi * D + d];
        zq[t * D + d] = __fadd_rn(zv[d], __fsub_rn(q, zv[d]));  // z + (z_q - z), quantize.py:298
    }
    if (idx_out) idx_out[t] = bi;
}

// ---- overlap-average tiling (utils/util_image.py:889-979 ImageSpliterTh.update / gather) -----------------------------
// acc[b,c,h0+y,w0+x] += tile[b,c,y,x];  count[h0+y,w0+x] += 1 (one plane: the reference's per-(b,c) counts are all equal)
__global__ void tile_accumulate_kernel(float* acc, float* count, const float* tile, int B, int C, int H, int W, int h0, int w0, int th,
                                       int tw) {
    const long long n = (long long)B * C * th * tw;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(g % tw);
        long long t = g / tw;
        const int y = (int)(t % th);
        const long long bc = t / th;
        acc[(bc * H + h0 + y) * W + w0 + x] += tile[g];
        if (bc == 0) count[(long long)(h0 + y) * W + w0 + x] += 1.0f;
    }
}
// ---- feathered blending (include/resshift_hip.h "feathered tile blending") ------------------------------
// The weight and the update of BOTH weighted kernels below - ONE definition each, so that rs_tile_scatter_weighted is bit for bit
// rs_tile_accumulate_weighted tile by tile whatever the compiler does with either loop (as axpbypcz_combine above).  Contraction is
// switched off inside them: `count + w` after `w = wh * ww` would otherwise become fma(wh, ww, count) in one kernel and not in the other
// (the __f*_rn intrinsics are plain operators here and contract like them).  The one fused operation is the fmaf that is spelled out.
// inv_R = 1 / R, formed once per thread; R == 0 travels as 2, which makes every weight min(1, >= 1) = 1 exactly.
__device__ __forceinline__ float feather_inv(int R) { return R > 0 ? 1.0f / (float)R : 2.0f; }
__device__ __forceinline__ float feather_w1(int p, int n, float inv_R) {
#pragma clang fp contract(off)
    return fminf(1.f, ((float)min(p, n - 1 - p) + 0.5f) * inv_R);   // (an integer below 2^24 plus a half is exact)
}
__device__ __forceinline__ float feather_w2(float wh, float ww) {
#pragma clang fp contract(off)
    return wh * ww;
}
__device__ __forceinline__ void feather_update(float w, float v, float& sum, float& cnt) {
#pragma clang fp contract(off)
    sum = fmaf(w, v, sum);
    cnt = cnt + w;
}
// acc[b,c,h0+y,w0+x] += w(y, x) tile[b,c,y,x];  count[h0+y,w0+x] += w(y, x), w the feather weight of the th x tw tile
__global__ void tile_accumulate_weighted_kernel(float* acc, float* count, const float* tile, int B, int C, int H, int W, int h0, int w0,
                                                int th, int tw, int Rh, int Rw) {
    const long long n = (long long)B * C * th * tw;
    const float ih = feather_inv(Rh), iw = feather_inv(Rw);
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(g % tw);
        long long t = g / tw;
        const int y = (int)(t % th);
        const long long bc = t / th;
        const float w = feather_w2(feather_w1(y, th, ih), feather_w1(x, tw, iw));
        float* pa = acc + (bc * H + h0 + y) * W + w0 + x;
        float* pc = count + (long long)(h0 + y) * W + w0 + x;
        float s = *pa, cv = bc == 0 ? *pc : 0.f;
        feather_update(w, tile[g], s, cv);
        *pa = s;
        if (bc == 0) *pc = cv;
    }
}
__global__ void tile_finalize_kernel(float* acc, const float* count, long long BC, long long HW) {
    const long long n = BC * HW;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long long)gridDim.x * blockDim.x)
        acc[g] = acc[g] / count[g % HW];
}

// ---- tile pool (resshift_amd/tilepool.py): the same data movement for tiles of DIFFERENT images in one launch --------
// The descriptors travel by value (64 x 48 B = 3 KB of the 4 KB kernel-argument segment).  blockIdx.y is the tile, so a workgroup's
// descriptor - and every descriptor the scatter kernel walks - is wave-uniform: the compiler reads them with scalar loads.
// V = 4: every row group is four consecutive floats, 16-byte aligned on the output side (the launcher checks widths and pointers).
struct TileDescs { rs_tile_desc d[RS_MAX_ROWS]; };

// out_lq[k][c][i][j] = src_k[c][h0 + refl(i, th)][w0 + refl(j, tw)] (c < 3), out_mask[k][0][i][j] likewise from plane 3;
// refl(i, n) = i < n ? i : 2 (n - 1) - i as in window_copy_kernel, but relative to the tile's window: F.pad(mode='reflect') of the CROP
template <int V>
__global__ __launch_bounds__(256) void tile_gather_kernel(TileDescs ds, int C, float* out_lq, float* out_mask, int Hp, int Wp) {
    const int k = blockIdx.y;
    const float* src = ds.d[k].src;
    const int H = ds.d[k].H, W = ds.d[k].W, h0 = ds.d[k].h0, w0 = ds.d[k].w0, th = ds.d[k].th, tw = ds.d[k].tw;
    const int Wv = Wp / V, n = C * Hp * Wv;
    // a group that lies inside the window is one 16-byte load when the plane's rows and the window's origin keep the alignment
    const bool al = V > 1 && ((W | w0) % V) == 0 && ((uintptr_t)src % (V * sizeof(float))) == 0;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < n; g += gridDim.x * blockDim.x) {
        const int j = (g % Wv) * V, r = g / Wv;
        const int i = r % Hp, c = r / Hp;
        const int yi = i < th ? i : 2 * (th - 1) - i;
        const float* row = src + ((long long)c * H + h0 + yi) * W + w0;
        float* dst = c < 3 ? out_lq + (((long long)k * 3 + c) * Hp + i) * Wp + j : out_mask + ((long long)k * Hp + i) * Wp + j;
        if constexpr (V == 4) {
            f32x4 v;
            if (al && j + V <= tw) {
                v = *(const f32x4*)(row + j);
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) { const int x = j + e; v[e] = row[x < tw ? x : 2 * (tw - 1) - x]; }
            }
            *(f32x4*)dst = v;
        } else {
            *dst = row[j < tw ? j : 2 * (tw - 1) - j];
        }
    }
}

// does tile d of a launch cover canvas element (Y, X) of canvas `acc`?
__device__ __forceinline__ bool tile_covers(const rs_tile_desc& d, const float* acc, int sf, int Y, int X) {
    return d.acc == acc && Y >= d.h0 * sf && Y < (d.h0 + d.th) * sf && X >= d.w0 * sf && X < (d.w0 + d.tw) * sf;
}
// acc_k[c][h0 sf + i][w0 sf + j] += tiles[k][c][i][j] over the tile's (th sf) x (tw sf) window, count_k += 1 there.  Tiles of one launch
// may overlap in one canvas, so the thread of tile k's element owns its canvas element only when no tile j < k covers it, and then adds
// tiles k, k+1, ... n-1 that cover it, in that order, onto the value already there: the floating-point additions of n successive
// tile_accumulate_kernel launches in index order, one writer per element, no atomics.  (V = 4: all window edges are multiples of 4 canvas
// columns, so the four elements of a group are covered by the same tiles.)
template <int V>
__global__ __launch_bounds__(256) void tile_scatter_kernel(TileDescs ds, int n, int C, int sf, const float* tiles, int Hpo, int Wpo) {
    typedef float vec __attribute__((ext_vector_type(V)));
    const int k = blockIdx.y;
    float* acc = ds.d[k].acc;
    float* count = ds.d[k].count;
    const int Hc = ds.d[k].H * sf, Wc = ds.d[k].W * sf, y0 = ds.d[k].h0 * sf, x0 = ds.d[k].w0 * sf;
    const int hh = ds.d[k].th * sf, wv = ds.d[k].tw * sf / V, total = C * hh * wv;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < total; g += gridDim.x * blockDim.x) {
        const int r = g / wv;
        const int X = x0 + (g % wv) * V, Y = y0 + r % hh, c = r / hh;
        bool own = true;
        for (int j = 0; j < k && own; ++j) own = !tile_covers(ds.d[j], acc, sf, Y, X);
        if (!own) continue;
        float* pa = acc + ((long long)c * Hc + Y) * Wc + X;
        float* pc = count + (long long)Y * Wc + X;
        vec v = *(const vec*)pa;
        vec cv = c == 0 ? *(const vec*)pc : (vec)(0.0f);
        for (int j = k; j < n; ++j) {
            if (!tile_covers(ds.d[j], acc, sf, Y, X)) continue;
            v += *(const vec*)(tiles + (((long long)j * C + c) * Hpo + (Y - ds.d[j].h0 * sf)) * Wpo + (X - ds.d[j].w0 * sf));
            cv += 1.0f;
        }
        *(vec*)pa = v;
        if (c == 0) *(vec*)pc = cv;
    }
}
// The same walk with feather weights: acc_k += w tiles[k], count_k += w, w = feather_w1(i, th sf, 1 / Rh) feather_w1(j, tw sf, 1 / Rw) at
// (i, j) of tile k's window - computed from the indices, no table, no load.  The four elements of a group share their covering tiles
// (as above) and a tile's row weight, not its column weights.  Ownership, order and the one-writer rule are tile_scatter_kernel's, the
// arithmetic is tile_accumulate_weighted_kernel's (feather_update): n successive weighted accumulate launches in index order.
template <int V>
__global__ __launch_bounds__(256) void tile_scatter_weighted_kernel(TileDescs ds, int n, int C, int sf, const float* tiles, int Hpo, int Wpo,
                                                                    int Rh, int Rw) {
    typedef float vec __attribute__((ext_vector_type(V)));
    const int k = blockIdx.y;
    float* acc = ds.d[k].acc;
    float* count = ds.d[k].count;
    const int Hc = ds.d[k].H * sf, Wc = ds.d[k].W * sf, y0 = ds.d[k].h0 * sf, x0 = ds.d[k].w0 * sf;
    const int hh = ds.d[k].th * sf, wv = ds.d[k].tw * sf / V, total = C * hh * wv;
    const float ih = feather_inv(Rh), iw = feather_inv(Rw);
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < total; g += gridDim.x * blockDim.x) {
        const int r = g / wv;
        const int X = x0 + (g % wv) * V, Y = y0 + r % hh, c = r / hh;
        bool own = true;
        for (int j = 0; j < k && own; ++j) own = !tile_covers(ds.d[j], acc, sf, Y, X);
        if (!own) continue;
        float* pa = acc + ((long long)c * Hc + Y) * Wc + X;
        float* pc = count + (long long)Y * Wc + X;
        vec v = *(const vec*)pa;
        vec cv = c == 0 ? *(const vec*)pc : (vec)(0.0f);
        for (int j = k; j < n; ++j) {
            if (!tile_covers(ds.d[j], acc, sf, Y, X)) continue;
            const int i = Y - ds.d[j].h0 * sf, jx = X - ds.d[j].w0 * sf, nh = ds.d[j].th * sf, nw = ds.d[j].tw * sf;
            const vec t = *(const vec*)(tiles + (((long long)j * C + c) * Hpo + i) * Wpo + jx);
            const float wh = feather_w1(i, nh, ih);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float s = v[e], cnt = cv[e];
                feather_update(feather_w2(wh, feather_w1(jx + e, nw, iw)), t[e], s, cnt);
                v[e] = s;
                cv[e] = cnt;
            }
        }
        *(vec*)pa = v;
        if (c == 0) *(vec*)pc = cv;
    }
}

inline unsigned nblk(long long n, int bs = 256, long long cap = 65536) { return (unsigned)std::min<long long>((n + bs - 1) / bs, cap); }

}  // namespace

// ---------------------------------------------------------------- uint8 pre / post processing on the device
// pre:  datapipe/datasets.py:59-63 (ToTensor + Normalize(0.5, 0.5)): interleaved uint8 HWC -> planar fp32 in [-1, 1].
// post: sampler.py:218-222 + utils/util_image.py:245-269 (tensor2img): x*0.5+0.5, optional inpainting blend
//       sr*m + lq*(1-m), clamp to [0,1], *255, round half to even, optional RGB->BGR, planar fp32 -> interleaved uint8.
// The arithmetic is spelled with the non-contracting intrinsics so that it rounds exactly like the reference's
// separate torch / numpy ops (no fused multiply-add).
__global__ void u8_to_input_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, long long npix, int HW, int C) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long long)gridDim.x * blockDim.x) {   // pixel of B*H*W
        const long long b = i / HW, hw = i - b * HW;
        for (int c = 0; c < C; ++c) {
            const float v = __fdiv_rn((float)src[i * C + c], 255.0f);
            dst[(b * C + c) * HW + hw] = __fdiv_rn(__fsub_rn(v, 0.5f), 0.5f);
        }
    }
}

__global__ void output_to_u8_kernel(const float* __restrict__ sr, const float* __restrict__ lq, const float* __restrict__ mask,
                                    unsigned char* __restrict__ dst, long long npix, int HW, int C, int bgr) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long long)gridDim.x * blockDim.x) {
        const long long b = i / HW, hw = i - b * HW;
        float m = 1.0f;
        if (mask) m = __fadd_rn(__fmul_rn(mask[b * HW + hw], 0.5f), 0.5f);
        for (int c = 0; c < C; ++c) {
            float v = __fadd_rn(__fmul_rn(sr[(b * C + c) * HW + hw], 0.5f), 0.5f);
            if (mask) {
                const float l = __fadd_rn(__fmul_rn(lq[(b * C + c) * HW + hw], 0.5f), 0.5f);
                v = __fadd_rn(__fmul_rn(v, m), __fmul_rn(l, __fsub_rn(1.0f, m)));
            }
            const int oc = (bgr && C == 3) ? 2 - c : c;
            dst[i * C + oc] = rs_unit_to_u8(v);
        }
    }
}

template <typename TI>
static int convert_from(const TI* src, void* dst, int dst_dt, int C, long long npix, hipStream_t st) {
    const long long n = npix * C;
    if (dst_dt == RS_F16) hipLaunchKernelGGL((convert_kernel<TI, f16>), dim3(nblk(n)), dim3(256), 0, st, src, (f16*)dst, C, npix);
    else if (dst_dt == RS_F16S) hipLaunchKernelGGL((convert_kernel<TI, h2s>), dim3(nblk(n)), dim3(256), 0, st, src, (h2s*)dst, C, npix);
    else if (dst_dt == RS_F32) hipLaunchKernelGGL((convert_kernel<TI, float>), dim3(nblk(n)), dim3(256), 0, st, src, (float*)dst, C, npix);
    else return -2;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// out[pl][i][j] = scale * in[pl][refl(h0 + i, H)][refl(w0 + j, W)] on fp32 planes, refl(i, n) = i < n ? i : 2 (n - 1) - i.
// One kernel for the data movement the host mirror needs around the networks: bottom / right reflect padding of the LQ batch
// (sampler.py:130-138, F.pad mode 'reflect'), the tile crop of the tiled path (util_image.py:946-952) and the latent scaling
// of encode_first_stage (gaussian_diffusion.py:514).
__global__ void window_copy_kernel(const float* in, float* out, long long planes, int H, int W, int h0, int w0, int Ho, int Wo, float scale) {
    const long long n = planes * Ho * Wo;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(g % Wo);
        const long long t = g / Wo;
        const int i = (int)(t % Ho);
        const long long pl = t / Ho;
        int y = h0 + i, x = w0 + j;
        y = y < H ? y : 2 * (H - 1) - y;
        x = x < W ? x : 2 * (W - 1) - x;
        out[g] = scale * in[(pl * H + y) * W + x];
    }
}

extern "C" {

int rs_nchw_to_nhwc_launch(const float* in, void* out, int out_dt, int B, int C, int HW, int ldo, int coff, float scale, hipStream_t st) {
    const long long n = (long long)B * C * HW;
    if (out_dt == RS_F16) hipLaunchKernelGGL((nchw_to_nhwc_kernel<f16>), dim3(nblk(n)), dim3(256), 0, st, in, (f16*)out, B, C, HW, ldo, coff, scale);
    else if (out_dt == RS_F16S) hipLaunchKernelGGL((nchw_to_nhwc_kernel<h2s>), dim3(nblk(n)), dim3(256), 0, st, in, (h2s*)out, B, C, HW, ldo, coff, scale);
    else hipLaunchKernelGGL((nchw_to_nhwc_kernel<float>), dim3(nblk(n)), dim3(256), 0, st, in, (float*)out, B, C, HW, ldo, coff, scale);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_nchw_to_nhwc_rows_launch(const float* in, void* out, int out_dt, int B, int C, int HW, int ldo, int coff, const float* scale, hipStream_t st) {
    if (B < 1 || B > RS_MAX_ROWS || !scale) return -2;
    RowScale s{};
    for (int r = 0; r < B; ++r) s.a[r] = scale[r];
    const long long n = (long long)B * C * HW;
    if (out_dt == RS_F16) hipLaunchKernelGGL((nchw_to_nhwc_rows_kernel<f16>), dim3(nblk(n)), dim3(256), 0, st, in, (f16*)out, B, C, HW, ldo, coff, s);
    else if (out_dt == RS_F16S) hipLaunchKernelGGL((nchw_to_nhwc_rows_kernel<h2s>), dim3(nblk(n)), dim3(256), 0, st, in, (h2s*)out, B, C, HW, ldo, coff, s);
    else hipLaunchKernelGGL((nchw_to_nhwc_rows_kernel<float>), dim3(nblk(n)), dim3(256), 0, st, in, (float*)out, B, C, HW, ldo, coff, s);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_nhwc_to_nchw_launch(const void* in, int in_dt, float* out, int B, int C, int HW, int ldi, int coff, hipStream_t st) {
    const long long n = (long long)B * C * HW;
    if (in_dt == RS_F16) hipLaunchKernelGGL((nhwc_to_nchw_kernel<f16>), dim3(nblk(n)), dim3(256), 0, st, (const f16*)in, out, B, C, HW, ldi, coff);
    else if (in_dt == RS_F16S) hipLaunchKernelGGL((nhwc_to_nchw_kernel<h2s>), dim3(nblk(n)), dim3(256), 0, st, (const h2s*)in, out, B, C, HW, ldi, coff);
    else hipLaunchKernelGGL((nhwc_to_nchw_kernel<float>), dim3(nblk(n)), dim3(256), 0, st, (const float*)in, out, B, C, HW, ldi, coff);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_copy_channels_launch(const void* src, int lds_, void* dst, int ldd, int C, long long npix, int dt, hipStream_t st) {
    if ((C % 8) || (lds_ % 8) || (ldd % 8)) return -2;
    const long long n = npix * (C / 8);
    if (dt == RS_F16) hipLaunchKernelGGL((copy_channels_kernel<f16>), dim3(nblk(n)), dim3(256), 0, st, (const f16*)src, lds_, (f16*)dst, ldd, C, npix);
    else if (dt == RS_F16S) hipLaunchKernelGGL((copy_channels_kernel<h2s>), dim3(nblk(n)), dim3(256), 0, st, (const h2s*)src, lds_, (h2s*)dst, ldd, C, npix);
    else hipLaunchKernelGGL((copy_channels_kernel<float>), dim3(nblk(n)), dim3(256), 0, st, (const float*)src, lds_, (float*)dst, ldd, C, npix);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_convert_launch(const void* src, int src_dt, void* dst, int dst_dt, int C, long long npix, hipStream_t st) {
    if (src_dt == RS_F16) return convert_from((const f16*)src, dst, dst_dt, C, npix, st);
    if (src_dt == RS_F16S) return convert_from((const h2s*)src, dst, dst_dt, C, npix, st);
    if (src_dt == RS_F32) return convert_from((const float*)src, dst, dst_dt, C, npix, st);
    return -2;
}

int rs_axpbypcz_launch(const float* x, const float* z, const float* n, float* y, float a, float b, float c, long long cnt, hipStream_t st) {
    hipLaunchKernelGGL(axpbypcz_kernel, dim3(nblk(cnt)), dim3(256), 0, st, x, z, n, y, a, b, c, cnt);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_axpbypcz_rows_launch(const float* x, const float* z, const float* n, float* y, const float* a, const float* b, const float* c, long long per,
                            int B, hipStream_t st) {
    if (B < 1 || B > RS_MAX_ROWS || per < 1 || !x || !y || !a) return -2;
    RowCoefs k{};
    for (int r = 0; r < B; ++r) { k.a[r] = a[r]; k.b[r] = b ? b[r] : 0.f; k.c[r] = c ? c[r] : 0.f; }
    const long long cnt = per * B;
    hipLaunchKernelGGL(axpbypcz_rows_kernel, dim3(nblk(cnt)), dim3(256), 0, st, x, z, n, y, k, per, cnt);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}


static inline bool al16f(const void* p) { return ((uintptr_t)p & 15) == 0; }
// what the seeded entry points ask of a key array; nullptr when it is fine
static const char* noise_keys_error(const rs_noise_key* keys, int B) {
    if (!keys) return "null keys";
    for (int b = 0; b < B; ++b)
        if (keys[b].reserved != 0) return "a key's reserved field is not 0";
    return nullptr;
}
static inline dim3 seeded_grid(long long per, int B) { return dim3(nblk((per + 3) / 4, 256, 1024), (unsigned)B); }

int rs_noise_fill(const rs_noise_key* keys, const int* draw, float* out, long long per_image_count, int B, void* stream) {
    if (B < 1 || B > RS_MAX_ROWS) return rs_set_last_error("rs_noise_fill: B must be 1 .. RS_MAX_ROWS", -2);
    if (const char* e = noise_keys_error(keys, B)) return rs_set_last_error((std::string("rs_noise_fill: ") + e).c_str(), -2);
    if (!draw || !out) return rs_set_last_error("rs_noise_fill: null draw indices or output", -2);
    if (per_image_count < 1 || per_image_count > 0x3ffffffffLL) return rs_set_last_error("rs_noise_fill: per_image_count outside 1 .. 2^34 - 1", -2);
    RowKeys nk{};
    for (int b = 0; b < B; ++b) {
        if (draw[b] < 0) return rs_set_last_error("rs_noise_fill: negative draw index", -2);
        nk.k[b] = keys[b]; nk.draw[b] = draw[b];
    }
    const dim3 grid = seeded_grid(per_image_count, B);
    if ((per_image_count % 4) == 0 && al16f(out)) hipLaunchKernelGGL(noise_fill_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, out, nk, per_image_count);
    else hipLaunchKernelGGL(noise_fill_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, out, nk, per_image_count);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_add_noise(const float* x, float* out, const rs_noise_key* keys, const int* draw, const float* sigma, const int* gray, int B, int C, int H,
                 int W, int clamp, void* stream) {
    const std::string who = "rs_add_noise: ";
    if (B < 1 || B > RS_MAX_ROWS) return img_fail(who, "B must be 1 .. RS_MAX_ROWS");
    if (const char* e = noise_keys_error(keys, B)) return img_fail(who, e);
    if (!x || !out || !draw || !sigma || !gray) return img_fail(who, "null pointer (x / out / draw / sigma / gray)");
    if (C < 1 || H < 1 || W < 1) return img_fail(who, "C, H and W must be positive");
    if ((long long)C * H * W > 0x3ffffffffLL) return img_fail(who, "an image has more than 2^34 - 1 elements");
    if (!img_is_flag(clamp)) return img_fail(who, "clamp must be 0 or 1");
    const long long HW = (long long)H * W, n = (long long)B * C * HW;
    if (x != out && img_overlaps(x, n * sizeof(float), out, n * sizeof(float))) return img_fail(who, "`out` partly overlaps `x` (in place or apart)");
    NoiseRows k{};
    RowKeys nk{};
    bool any_color = false;
    for (int b = 0; b < B; ++b) {
        if (draw[b] < 0) return img_fail(who, "negative draw index");
        if (!(sigma[b] >= 0.0f) || !std::isfinite(sigma[b])) return img_fail(who, "every sigma must be finite and not negative");
        if (!img_is_flag(gray[b])) return img_fail(who, "every gray flag must be 0 or 1");
        k.c[b] = (float)((double)sigma[b] / 255.0);
        k.gray[b] = (unsigned char)gray[b];
        any_color |= gray[b] == 0;
        nk.k[b] = keys[b]; nk.draw[b] = draw[b];
    }
    hipLaunchKernelGGL(add_noise_kernel, seeded_grid(any_color ? C * HW : HW, B), dim3(256), 0, (hipStream_t)stream, x, out, k, nk, C, HW, clamp);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_unit_to_u8(const float* src_f32_nchw, void* dst_u8_nhwc, int B, int C, int H, int W, void* stream) {
    if (!src_f32_nchw || !dst_u8_nhwc) return rs_set_last_error("rs_unit_to_u8: null tensor (src / dst)", -2);
    if (B < 1 || C < 1 || H < 1 || W < 1) return rs_set_last_error("rs_unit_to_u8: B, C, H and W must be positive", -2);
    const long long HW = (long long)H * W, npix = (long long)B * HW;
    hipLaunchKernelGGL(unit_to_u8_kernel, dim3(nblk(npix)), dim3(256), 0, (hipStream_t)stream, src_f32_nchw, (unsigned char*)dst_u8_nhwc, npix, HW, C);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// y = a x + b z + c noise(keys, draw) per image.  B <= RS_MAX_ROWS: keys (host), a / b / c / draw (host, [B]) by value.  B > RS_MAX_ROWS:
// `keys_dev` (device, [B]) and ONE coefficient triple / draw index (a[0], b[0], c[0], draw[0]) for every image.
int rs_axpbypcz_seeded_launch(const float* x, const float* z, float* y, const float* a, const float* b, const float* c, const rs_noise_key* keys,
                              const rs_noise_key* keys_dev, const int* draw, long long per, int B, hipStream_t st) {
    const bool big = B > RS_MAX_ROWS;
    if (B < 1 || per < 1 || per > 0x3ffffffffLL || !x || !y || !a || !draw || (big ? !keys_dev : !keys)) return -2;
    RowCoefs k{};
    RowKeys nk{};
    for (int r = 0; r < (big ? 1 : B); ++r) {
        k.a[r] = a[r]; k.b[r] = b ? b[r] : 0.f; k.c[r] = c ? c[r] : 0.f;
        nk.draw[r] = draw[r];
        if (!big) nk.k[r] = keys[r];
    }
    const dim3 grid = seeded_grid(per, B);
    const bool v4 = (per % 4) == 0 && al16f(x) && al16f(y) && al16f(z);
    if (v4) hipLaunchKernelGGL(axpbypcz_seeded_kernel<true>, grid, dim3(256), 0, st, x, z, y, k, nk, big ? keys_dev : nullptr, big ? 1 : 0, per);
    else hipLaunchKernelGGL(axpbypcz_seeded_kernel<false>, grid, dim3(256), 0, st, x, z, y, k, nk, big ? keys_dev : nullptr, big ? 1 : 0, per);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_film_gather_launch(const float* const* rows, int B, int total, float* out, hipStream_t st) {
    if (B < 1 || B > RS_MAX_ROWS || total < 1) return -2;
    FilmRows s{};
    for (int r = 0; r < B; ++r) { if (!rows[r]) return -2; s.row[r] = rows[r]; }
    const long long cnt = (long long)B * total;
    hipLaunchKernelGGL(film_gather_kernel, dim3(nblk(cnt)), dim3(256), 0, st, s, out, total, cnt);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_clamp_launch(float* x, float lo, float hi, long long cnt, hipStream_t st) {
    hipLaunchKernelGGL(clamp_kernel, dim3(nblk(cnt)), dim3(256), 0, st, x, lo, hi, cnt);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_silu_launch(const void* x, void* y, int dt, long long cnt, hipStream_t st) {
    if (dt == RS_F16) hipLaunchKernelGGL((silu_kernel<f16>), dim3(nblk(cnt)), dim3(256), 0, st, (const f16*)x, (f16*)y, cnt);
    else hipLaunchKernelGGL((silu_kernel<float>), dim3(nblk(cnt)), dim3(256), 0, st, (const float*)x, (float*)y, cnt);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_small_linear_launch(const float* x, const float* w, const float* bias, float* y, int R, int K, int N, int silu_in, int silu_out,
                           hipStream_t st) {
    hipLaunchKernelGGL(small_linear_kernel, dim3((unsigned)(((long long)R * N + 3) / 4)), dim3(256), 0, st, x, w, bias, y, R, K, N, silu_in, silu_out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_bicubic_launch(const float* in, void* out, int out_dt, int B, int C, int H, int W, int sf, int ldo, hipStream_t st) {
    const long long n = (long long)B * H * sf * W * sf * C;
    if (out_dt == RS_F16) hipLaunchKernelGGL((bicubic_up_kernel<f16>), dim3(nblk(n)), dim3(256), 0, st, in, (f16*)out, B, C, H, W, sf, ldo);
    else if (out_dt == RS_F16S) hipLaunchKernelGGL((bicubic_up_kernel<h2s>), dim3(nblk(n)), dim3(256), 0, st, in, (h2s*)out, B, C, H, W, sf, ldo);
    else hipLaunchKernelGGL((bicubic_up_kernel<float>), dim3(nblk(n)), dim3(256), 0, st, in, (float*)out, B, C, H, W, sf, ldo);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_tile_accumulate(float* acc, float* count, const float* tile, int B, int C, int H, int W, int h0, int w0, int th, int tw,
                       void* stream) {
    if (h0 < 0 || w0 < 0 || h0 + th > H || w0 + tw > W) return -2;
    const long long n = (long long)B * C * th * tw;
    hipLaunchKernelGGL(tile_accumulate_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, acc, count, tile, B, C, H, W, h0, w0, th, tw);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_tile_accumulate_weighted(float* acc, float* count, const float* tile, int B, int C, int H, int W, int h0, int w0, int th, int tw,
                                int Rh, int Rw, void* stream) {
    if (!acc || !count || !tile) return rs_set_last_error("rs_tile_accumulate_weighted: null tensor (acc / count / tile)", -2);
    if (B < 1 || C < 1 || th < 1 || tw < 1 || h0 < 0 || w0 < 0 || h0 + th > H || w0 + tw > W)
        return rs_set_last_error("rs_tile_accumulate_weighted: the tile window leaves its canvas", -2);
    if (Rh < 0 || Rw < 0) return rs_set_last_error("rs_tile_accumulate_weighted: ramp widths Rh and Rw must not be negative", -2);
    const long long n = (long long)B * C * th * tw;
    hipLaunchKernelGGL(tile_accumulate_weighted_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, acc, count, tile, B, C, H, W, h0, w0,
                       th, tw, Rh, Rw);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_window_copy(const float* in, float* out, long long planes, int H, int W, int h0, int w0, int Ho, int Wo, float scale, void* stream) {
    // (one reflection at most, as torch: the window may overhang the plane by less than its size)
    if (planes <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || h0 < 0 || w0 < 0 || h0 + Ho > 2 * H - 1 || w0 + Wo > 2 * W - 1 || h0 >= H || w0 >= W)
        return -2;
    const long long n = planes * Ho * Wo;
    hipLaunchKernelGGL(window_copy_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, in, out, planes, H, W, h0, w0, Ho, Wo, scale);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// what both tile-pool entry points ask of a descriptor array; nullptr when it is fine
static const char* tile_descs_error(const rs_tile_desc* desc, int n) {
    if (n < 1 || n > RS_MAX_ROWS) return "tile count outside 1 .. RS_MAX_ROWS";
    if (!desc) return "null descriptor array";
    for (int k = 0; k < n; ++k) {
        const rs_tile_desc& d = desc[k];
        if (d.H < 1 || d.W < 1 || d.th < 1 || d.tw < 1 || d.h0 < 0 || d.w0 < 0 || d.h0 + d.th > d.H || d.w0 + d.tw > d.W)
            return "a tile window leaves its plane";
    }
    return nullptr;
}
static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int rs_tile_gather(const rs_tile_desc* desc, int n, int C_src, float* out_lq, float* out_mask, int Hp, int Wp, void* stream) {
    if (const char* e = tile_descs_error(desc, n)) return rs_set_last_error((std::string("rs_tile_gather: ") + e).c_str(), -2);
    if (C_src != 3 && C_src != 4) return rs_set_last_error("rs_tile_gather: C_src must be 3 (LR planes) or 4 (LR planes + mask)", -2);
    if (!out_lq) return rs_set_last_error("rs_tile_gather: null tensor (out_lq)", -2);
    if ((C_src == 4) != (out_mask != nullptr)) return rs_set_last_error("rs_tile_gather: out_mask goes with C_src == 4, and only with it", -2);
    TileDescs ds{};
    for (int k = 0; k < n; ++k) {
        const rs_tile_desc& d = desc[k];
        if (!d.src) return rs_set_last_error("rs_tile_gather: null tensor (desc.src)", -2);
        if (d.th > Hp || d.tw > Wp) return rs_set_last_error("rs_tile_gather: a tile is larger than the padded shape (th > Hp or tw > Wp)", -2);
        // (one reflection at most, as torch.nn.functional.pad requires: the pad is smaller than the padded side)
        if (Hp - d.th >= d.th || Wp - d.tw >= d.tw) return rs_set_last_error("rs_tile_gather: reflect padding of a full tile side or more", -2);
        ds.d[k] = d;
    }
    const bool v4 = (Wp % 4) == 0 && al16(out_lq) && al16(out_mask);
    const long long per = (long long)C_src * Hp * (v4 ? Wp / 4 : Wp);
    if (per > 0x7fffffffLL) return rs_set_last_error("rs_tile_gather: padded tile too large", -2);
    const dim3 grid(nblk(per, 256, 256), (unsigned)n);
    if (v4) hipLaunchKernelGGL(tile_gather_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, ds, C_src, out_lq, out_mask, Hp, Wp);
    else hipLaunchKernelGGL(tile_gather_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, ds, C_src, out_lq, out_mask, Hp, Wp);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// rs_tile_scatter (weighted = false: Rh, Rw unused) and rs_tile_scatter_weighted: one set of checks, one grid, one choice of path
static int tile_scatter_launch(const char* who, const rs_tile_desc* desc, int n, int C, int sf, const float* tiles, int Hp_out, int Wp_out,
                               bool weighted, int Rh, int Rw, void* stream) {
    const std::string pre = std::string(who) + ": ";
    if (const char* e = tile_descs_error(desc, n)) return rs_set_last_error((pre + e).c_str(), -2);
    if (C < 1 || sf < 1) return rs_set_last_error((pre + "C and sf must be positive").c_str(), -2);
    if (weighted && (Rh < 0 || Rw < 0)) return rs_set_last_error((pre + "ramp widths Rh and Rw must not be negative").c_str(), -2);
    if (!tiles) return rs_set_last_error((pre + "null tensor (tiles)").c_str(), -2);
    TileDescs ds{};
    bool v4 = (Wp_out % 4) == 0 && al16(tiles);
    long long per = 0;
    for (int k = 0; k < n; ++k) {
        const rs_tile_desc& d = desc[k];
        if (!d.acc || !d.count) return rs_set_last_error((pre + "null tensor (desc.acc / desc.count)").c_str(), -2);
        if ((long long)d.th * sf > Hp_out || (long long)d.tw * sf > Wp_out)
            return rs_set_last_error((pre + "a tile's window is larger than the tile tensor (th*sf > Hp_out or tw*sf > Wp_out)").c_str(), -2);
        for (int j = 0; j < k; ++j)
            if (desc[j].acc == d.acc && (desc[j].count != d.count || desc[j].H != d.H || desc[j].W != d.W))
                return rs_set_last_error((pre + "descriptors of one canvas disagree about its count plane or size").c_str(), -2);
        v4 = v4 && ((d.w0 * sf) % 4) == 0 && ((d.tw * sf) % 4) == 0 && ((d.W * sf) % 4) == 0 && al16(d.acc) && al16(d.count);
        per = std::max(per, (long long)C * d.th * sf * d.tw * sf);
        ds.d[k] = d;
    }
    if (per > 0x7fffffffLL) return rs_set_last_error((pre + "tile too large").c_str(), -2);
    const dim3 grid(nblk(v4 ? per / 4 : per, 256, 256), (unsigned)n);
    const hipStream_t st = (hipStream_t)stream;
    if (!weighted) {
        if (v4) hipLaunchKernelGGL(tile_scatter_kernel<4>, grid, dim3(256), 0, st, ds, n, C, sf, tiles, Hp_out, Wp_out);
        else hipLaunchKernelGGL(tile_scatter_kernel<1>, grid, dim3(256), 0, st, ds, n, C, sf, tiles, Hp_out, Wp_out);
    } else {
        if (v4) hipLaunchKernelGGL(tile_scatter_weighted_kernel<4>, grid, dim3(256), 0, st, ds, n, C, sf, tiles, Hp_out, Wp_out, Rh, Rw);
        else hipLaunchKernelGGL(tile_scatter_weighted_kernel<1>, grid, dim3(256), 0, st, ds, n, C, sf, tiles, Hp_out, Wp_out, Rh, Rw);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_tile_scatter(const rs_tile_desc* desc, int n, int C, int sf, const float* tiles, int Hp_out, int Wp_out, void* stream) {
    return tile_scatter_launch("rs_tile_scatter", desc, n, C, sf, tiles, Hp_out, Wp_out, false, 0, 0, stream);
}

int rs_tile_scatter_weighted(const rs_tile_desc* desc, int n, int C, int sf, const float* tiles, int Hp_out, int Wp_out, int Rh, int Rw,
                             void* stream) {
    return tile_scatter_launch("rs_tile_scatter_weighted", desc, n, C, sf, tiles, Hp_out, Wp_out, true, Rh, Rw, stream);
}

int rs_tile_finalize(float* acc, const float* count, int B, int C, int H, int W, void* stream) {
    const long long n = (long long)B * C * H * W;
    hipLaunchKernelGGL(tile_finalize_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, acc, count, (long long)B * C, (long long)H * W);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_u8_to_input(const void* src_u8_nhwc, float* dst_f32_nchw, int B, int H, int W, int C, void* stream) {
    const long long npix = (long long)B * H * W;
    hipLaunchKernelGGL(u8_to_input_kernel, dim3(nblk(npix)), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)src_u8_nhwc, dst_f32_nchw,
                       npix, H * W, C);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_output_to_u8(const float* sr_f32_nchw, const float* lq_f32_nchw, const float* mask_f32_n1hw, void* dst_u8_nhwc, int B, int H, int W,
                    int C, int bgr, void* stream) {
    if ((mask_f32_n1hw != nullptr) != (lq_f32_nchw != nullptr)) return -2;
    const long long npix = (long long)B * H * W;
    hipLaunchKernelGGL(output_to_u8_kernel, dim3(nblk(npix)), dim3(256), 0, (hipStream_t)stream, sr_f32_nchw, lq_f32_nchw, mask_f32_n1hw,
                       (unsigned char*)dst_u8_nhwc, npix, H * W, C, bgr);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_vq_launch(const float* z, const float* codebook, float* zq, int* idx, long long N, int NE, int D, hipStream_t st) {
    const size_t lds = (size_t)NE * (D + 1) * sizeof(float);
    if (lds > 160 * 1024) return -2;
    const unsigned blocks = (unsigned)((N + 255) / 256);
    if (D == 3) {
        (void)hipFuncSetAttribute((const void*)vq_nearest_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        hipLaunchKernelGGL((vq_nearest_kernel<3>), dim3(blocks), dim3(256), lds, st, z, codebook, zq, idx, N, NE);
    } else if (D == 4) {
        (void)hipFuncSetAttribute((const void*)vq_nearest_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        hipLaunchKernelGGL((vq_nearest_kernel<4>), dim3(blocks), dim3(256), lds, st, z, codebook, zq, idx, N, NE);
    } else if (D == 8) {
        (void)hipFuncSetAttribute((const void*)vq_nearest_kernel<8>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        hipLaunchKernelGGL((vq_nearest_kernel<8>), dim3(blocks), dim3(256), lds, st, z, codebook, zq, idx, N, NE);
    } else {
        return -2;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // extern "C"

// Real-ESRGAN degradation operators (include/resshift_hip.h "degradation"): the blur, the unantialiased resize and the
// JPEG stage of the reference's RealESRGANDataset.degrade_fun (basicsr/data/realesrgan_dataset.py:240-363), each ONE launch with no
// intermediate tensor in HBM.  fp32 NCHW contiguous, inputs only read.  Every output value is a function of its image and of its own
// index alone - no atomics, every sum in a fixed order - so a batch is bit for bit its B = 1 calls.
//
//   filter2d_kernel  basicsr/utils/img_process_util.py filter2D: k x k cross-correlation behind torch's `reflect` padding.  A workgroup
//                    of 256 threads owns a 16 x 64 output tile of one plane: it stages the mirrored (16 + k - 1) x (64 + k - 1) input
//                    tile and the image's kernel in LDS; lanes run along columns (consecutive dwords of LDS, the weight is a broadcast),
//                    a thread owns four rows of one column, taps accumulate in row-major ascending order.
//   interp_kernel    F.interpolate(mode = area | bicubic, align_corners=False), one thread per output value, lanes along a row; source
//                    coordinates in fp64, rounded to fp32 once.
//   interp_bilinear_kernel  mode = bilinear: a thread applies the coordinates of its position to eight planes.
//   jpeg_kernel      basicsr/utils/diffjpeg.py DiffJPEG(differentiable=False).  ONE WAVE PER 16 x 16 MCU, four MCUs per workgroup.  Lane
//                    l owns the 2 x 2 pixel quad (l / 8, l % 8) at both ends - the chroma mean and the pixel repetition stay in the
//                    lane - and the coefficient (l / 8, l % 8) of each of the MCU's six 8 x 8 blocks in between; the blocks live in
//                    two LDS images per wave, pitched 9 dwords per row of 8.
#include "image_common.h"
#include <cmath>

// ---- filter2D ------------------------------------------------------------------------------------------------------------------
constexpr int FL_TR = 16;
constexpr int FL_TC = 64;
constexpr int FL_THREADS = 256;
constexpr int FL_KMAX = 21;
constexpr int FL_PITCH = FL_TC + FL_KMAX - 1;   // 84 dwords: lanes read consecutive dwords of one row

__global__ __launch_bounds__(FL_THREADS) void filter2d_kernel(const float* __restrict__ in, const float* __restrict__ kern, float* __restrict__ out,
                                                              int C, int H, int W, int k, int per_image, int tiles_x, int tiles_y,
                                                              long long total, int clamp) {
    __shared__ float tile[(FL_TR + FL_KMAX - 1) * FL_PITCH];
    __shared__ float wk[FL_KMAX * FL_KMAX];
    const int tid = threadIdx.x, p = k / 2;
    const int c = tid & (FL_TC - 1), r0 = tid / FL_TC;   // the thread's column and the first of its four rows (r0, r0 + 4, ...)
    for (long long t = blockIdx.x; t < total; t += gridDim.x) {
        const int tx = (int)(t % tiles_x);
        const long long q = t / tiles_x;
        const int ty = (int)(q % tiles_y);
        const long long plane = q / tiles_y;
        const int oy0 = ty * FL_TR, ox0 = tx * FL_TC;
        const int nr = min(FL_TR, H - oy0), nc = min(FL_TC, W - ox0);
        const float* inp = in + plane * H * W;
        const float* kp = kern + (per_image ? (plane / C) * k * k : 0);
        img_stage_footprint(inp, kp, tile, wk, FL_PITCH, oy0, ox0, nr, nc, k, p, H, W, tid, FL_THREADS);
        __syncthreads();
        if (c < nc) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int ky = 0; ky < k; ++ky)
                for (int kx = 0; kx < k; ++kx) {
                    const float w = wk[ky * k + kx];
#pragma unroll
                    for (int j = 0; j < 4; ++j)   // (rows past nr read staged or stale LDS inside the array and are not stored)
                        acc[j] = fmaf(w, tile[(r0 + 4 * j + ky) * FL_PITCH + c + kx], acc[j]);
                }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = r0 + 4 * j;
                if (r < nr) out[plane * H * W + (long long)(oy0 + r) * W + ox0 + c] = img_unit_clamp(acc[j], clamp);
            }
        }
        __syncthreads();   // (the next tile of this workgroup overwrites the LDS images)
    }
}

// ---- F.interpolate -------------------------------------------------------------------------------------------------------------
// A workgroup of 64 x 4 threads owns 64 columns of 4 output rows (no index division); a thread forms the coordinates, tap indices and
// weights of its output position, which depend on the position only.  Area and bicubic: one plane per thread (interp_kernel).  Bilinear:
// four taps, the fp64 coordinates are half of its work, so a thread forms the column's ONCE, a row's once per row, and applies them to
// eight planes of blockIdx.z's share (interp_bilinear_kernel).  Measured (scripts/degrade_bench.py, B = 32, 512 x 512): eight planes per thread
// take bilinear x 1.3 from 133 to 78 us, but bicubic x 0.6 from 65 to 114 us and area / 4 from 27 to 34 us (sixteen gathers resp. a 4 x 4
// window per plane: fewer threads in flight cost more than the coordinates save).
__global__ __launch_bounds__(256) void interp_kernel(const float* __restrict__ in, float* __restrict__ out, ImgAxis ah, ImgAxis aw, long long planes,
                                                     int mode, int clamp) {
    const int H = ah.n, W = aw.n, Ho = ah.m, Wo = aw.m;
    const int ox = blockIdx.x * 64 + threadIdx.x;
    if (ox >= Wo) return;
    for (long long plane = blockIdx.z; plane < planes; plane += gridDim.z) {
        const float* inp = in + plane * H * W;
        for (int oy = blockIdx.y * 4 + threadIdx.y; oy < Ho; oy += gridDim.y * 4) {
            float* outp = out + plane * Ho * Wo + (long long)oy * Wo + ox;
            if (mode == RS_INTERP_AREA) {   // adaptive average pooling: the integer window [floor(i n / m), ceil((i + 1) n / m)), summed in row-major order
                const int y0 = (int)(((long long)oy * H) / Ho), y1 = (int)((((long long)oy + 1) * H + Ho - 1) / Ho);
                const int x0 = (int)(((long long)ox * W) / Wo), x1 = (int)((((long long)ox + 1) * W + Wo - 1) / Wo);
                float sum = 0.f;
                for (int y = y0; y < y1; ++y)
                    for (int x = x0; x < x1; ++x) sum += inp[(long long)y * W + x];
                *outp = img_unit_clamp(sum / (float)((y1 - y0) * (x1 - x0)), clamp);
            } else {
                float ty, tx, wy[4], wx[4];
                const int y0 = img_source(ah, oy, false, &ty), x0 = img_source(aw, ox, false, &tx);
                img_cubic_weights(ty, wy);
                img_cubic_weights(tx, wx);
                float v = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float* row = inp + (long long)min(max(y0 - 1 + j, 0), H - 1) * W;
                    float s = 0.f;
#pragma unroll
                    for (int i = 0; i < 4; ++i) s = fmaf(wx[i], row[min(max(x0 - 1 + i, 0), W - 1)], s);
                    v = fmaf(wy[j], s, v);
                }
                *outp = img_unit_clamp(v, clamp);
            }
        }
    }
}

constexpr int IP_PLANES_BILINEAR = 8;

__global__ __launch_bounds__(256) void interp_bilinear_kernel(const float* __restrict__ in, float* __restrict__ out, ImgAxis ah, ImgAxis aw, long long planes, int clamp) {
    const int H = ah.n, W = aw.n, Ho = ah.m, Wo = aw.m;
    const int ox = blockIdx.x * 64 + threadIdx.x;
    if (ox >= Wo) return;
    int x0, x1;
    float fx;
    img_source2(aw, ox, &x0, &x1, &fx);
    const long long HW = (long long)H * W, HWo = (long long)Ho * Wo;
    for (int oy = blockIdx.y * 4 + threadIdx.y; oy < Ho; oy += gridDim.y * 4) {
        int y0, y1;
        float fy;
        img_source2(ah, oy, &y0, &y1, &fy);
        const long long r0 = (long long)y0 * W, r1 = (long long)y1 * W;
        for (long long p0 = (long long)blockIdx.z * IP_PLANES_BILINEAR; p0 < planes; p0 += (long long)gridDim.z * IP_PLANES_BILINEAR) {
            const int np = (int)min((long long)IP_PLANES_BILINEAR, planes - p0);
            const float* inp = in + p0 * HW;
            float* outp = out + p0 * HWo + (long long)oy * Wo + ox;
            for (int p = 0; p < np; ++p, inp += HW, outp += HWo)
                *outp = img_unit_clamp(img_bilinear(inp[r0 + x0], inp[r0 + x1], inp[r1 + x0], inp[r1 + x1], fy, fx), clamp);
        }
    }
}

// ---- DiffJPEG ------------------------------------------------------------------------------------------------------------------
constexpr int JP_WAVES = 4;          // MCUs per workgroup
constexpr int JP_PITCH = 9;          // dwords per row of 8: rows 0 .. 7 of a block start in 8 different banks
constexpr int JP_BLOCK = 8 * JP_PITCH;
constexpr int JP_IMG = 6 * JP_BLOCK; // Y00 Y01 Y10 Y11 Cb Cr

// cos((2 y + 1) v pi / 16), [y][v]: the float32 roundings of the double values
__device__ const float JP_COS[8][8] = {
    {1.0f, 0.9807852506637573f, 0.9238795042037964f, 0.8314695954322815f, 0.7071067690849304f, 0.5555702447891235f, 0.3826834261417389f, 0.19509032368659973f},
    {1.0f, 0.8314695954322815f, 0.3826834261417389f, -0.19509032368659973f, -0.7071067690849304f, -0.9807852506637573f, -0.9238795042037964f, -0.5555702447891235f},
    {1.0f, 0.5555702447891235f, -0.3826834261417389f, -0.9807852506637573f, -0.7071067690849304f, 0.19509032368659973f, 0.9238795042037964f, 0.8314695954322815f},
    {1.0f, 0.19509032368659973f, -0.9238795042037964f, -0.5555702447891235f, 0.7071067690849304f, 0.8314695954322815f, -0.3826834261417389f, -0.9807852506637573f},
    {1.0f, -0.19509032368659973f, -0.9238795042037964f, 0.5555702447891235f, 0.7071067690849304f, -0.8314695954322815f, -0.3826834261417389f, 0.9807852506637573f},
    {1.0f, -0.5555702447891235f, -0.3826834261417389f, 0.9807852506637573f, -0.7071067690849304f, -0.19509032368659973f, 0.9238795042037964f, -0.8314695954322815f},
    {1.0f, -0.8314695954322815f, 0.3826834261417389f, 0.19509032368659973f, -0.7071067690849304f, 0.9807852506637573f, -0.9238795042037964f, 0.5555702447891235f},
    {1.0f, -0.9807852506637573f, 0.9238795042037964f, -0.8314695954322815f, 0.7071067690849304f, -0.5555702447891235f, 0.3826834261417389f, -0.19509032368659973f},
};
// the quantisation tables as the reference indexes them (its arrays are the transposes of the JPEG standard's Annex K tables), [u][v]
__device__ const float JP_YTAB[8][8] = {
    {16, 12, 14, 14, 18, 24, 49, 72},   {11, 12, 13, 17, 22, 35, 64, 92},   {10, 14, 16, 22, 37, 55, 78, 95},    {16, 19, 24, 29, 56, 64, 87, 98},
    {24, 26, 40, 51, 68, 81, 103, 112}, {40, 58, 57, 87, 109, 104, 121, 100}, {51, 60, 69, 80, 103, 113, 120, 103}, {61, 55, 56, 62, 77, 92, 101, 99},
};
__device__ const float JP_CTAB[8][8] = {
    {17, 18, 24, 47, 99, 99, 99, 99}, {18, 21, 26, 66, 99, 99, 99, 99}, {24, 26, 56, 99, 99, 99, 99, 99}, {47, 66, 99, 99, 99, 99, 99, 99},
    {99, 99, 99, 99, 99, 99, 99, 99}, {99, 99, 99, 99, 99, 99, 99, 99}, {99, 99, 99, 99, 99, 99, 99, 99}, {99, 99, 99, 99, 99, 99, 99, 99},
};

struct JpFactors { float f[RS_MAX_ROWS]; };

// one pass of the separable 8-point transform over the wave's six blocks: dst[a][b] = sum_j src[a][j] w[j] (ROWS) or sum_j w[j] src[j][b]
template <bool ROWS>
__device__ __forceinline__ void jp_pass(const float* src, const float w[8], int a, int b, float res[6]) {
#pragma unroll
    for (int blk = 0; blk < 6; ++blk) {
        const float* s = src + blk * JP_BLOCK;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = fmaf(ROWS ? s[a * JP_PITCH + j] : s[j * JP_PITCH + b], w[j], acc);
        res[blk] = acc;
    }
}

__device__ __forceinline__ void jp_put(float* dst, int a, int b, const float v[6]) {
#pragma unroll
    for (int blk = 0; blk < 6; ++blk) dst[blk * JP_BLOCK + a * JP_PITCH + b] = v[blk];
}

__global__ __launch_bounds__(64 * JP_WAVES) void jpeg_kernel(const float* __restrict__ in, float* __restrict__ out, JpFactors fac, int H, int W,
                                                             int mcus_x, int mcus_y, long long total, long long groups) {
    __shared__ float lds[JP_WAVES][2][JP_IMG];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int a = lane >> 3, b = lane & 7;
    float* A = lds[wave][0];
    float* Bm = lds[wave][1];
    // the lane's slices of the tables: forward rows C[j][b], forward columns C[j][a], inverse rows C[b][j], inverse columns C[a][j]
    float cfr[8], cfc[8], cir[8], cic[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        cfr[j] = JP_COS[j][b]; cfc[j] = JP_COS[j][a]; cir[j] = JP_COS[b][j]; cic[j] = JP_COS[a][j];
    }
    const float r2 = 0.7071067690849304f;                              // float32(1 / sqrt(2))
    const float alpha = (a == 0 && b == 0) ? 0.5f : (a == 0 || b == 0) ? r2 : 1.0f;                 // float32(outer(alpha, alpha))
    const float scale = (a == 0 && b == 0) ? 0.125f : (a == 0 || b == 0) ? 0.1767766922712326f : 0.25f;   // float32(0.25 outer(alpha, alpha))
    const float ytab = JP_YTAB[a][b], ctab = JP_CTAB[a][b];
    const long long HW = (long long)H * W;
    for (long long grp = blockIdx.x; grp < groups; grp += gridDim.x) {   // (the trip count is the workgroup's: every wave reaches every barrier)
        const long long mcu = grp * JP_WAVES + wave;
        const bool live = mcu < total;
        const long long m = live ? mcu : 0;
        const int mx = (int)(m % mcus_x);
        const long long q = m / mcus_x;
        const int my = (int)(q % mcus_y);
        const long long img = q / mcus_y;
        const float factor = fac.f[img];
        const float* inp = in + img * 3 * HW;
        float* outp = out + img * 3 * HW;
        const int py = my * 16 + 2 * a, px = mx * 16 + 2 * b;        // the lane's quad
        // forward: x 255, RGB -> YCbCr (+ shift), chroma 2 x 2 mean, - 128.  Pixels past the image are zeros in RGB.
        float cbs = 0.f, crs = 0.f;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int y = py + dy, x = px + dx;
                float r = 0.f, g = 0.f, bl = 0.f;
                if (live && y < H && x < W) {
                    const long long o = (long long)y * W + x;
                    r = inp[o] * 255.0f; g = inp[HW + o] * 255.0f; bl = inp[2 * HW + o] * 255.0f;
                }
                const float yy = fmaf(0.11400000005960464f, bl, fmaf(0.5870000123977661f, g, 0.29899999499320984f * r));
                const float cb = fmaf(0.5f, bl, fmaf(-0.3312639892101288f, g, -0.16873599588871002f * r)) + 128.0f;
                const float cr = fmaf(-0.08131200075149536f, bl, fmaf(-0.41868799924850464f, g, 0.5f * r)) + 128.0f;
                cbs += cb;
                crs += cr;
                const int ly = 2 * a + dy, lx = 2 * b + dx;
                A[((ly >> 3) * 2 + (lx >> 3)) * JP_BLOCK + (ly & 7) * JP_PITCH + (lx & 7)] = yy - 128.0f;
            }
        A[4 * JP_BLOCK + a * JP_PITCH + b] = cbs * 0.25f - 128.0f;
        A[5 * JP_BLOCK + a * JP_PITCH + b] = crs * 0.25f - 128.0f;
        __syncthreads();
        float v[6];
        jp_pass<true>(A, cfr, a, b, v);       // T[a][b] = sum_y img[a][y] C[y][b]
        jp_put(Bm, a, b, v);
        __syncthreads();
        jp_pass<false>(Bm, cfc, a, b, v);     // F[a][b] = sum_x C[x][a] T[x][b]
        // quantise (fp32 product of table and factor, a true division, ties to even), dequantise, x alpha
        const float qy = ytab * factor, qc = ctab * factor;
#pragma unroll
        for (int blk = 0; blk < 6; ++blk) {
            const float qt = blk < 4 ? qy : qc;
            v[blk] = (rintf(__fdiv_rn(scale * v[blk], qt)) * qt) * alpha;
        }
        jp_put(A, a, b, v);                   // (A's readers finished before the barrier above)
        __syncthreads();
        jp_pass<true>(A, cir, a, b, v);       // S[a][b] = sum_y G[a][y] C[b][y]
        jp_put(Bm, a, b, v);
        __syncthreads();
        jp_pass<false>(Bm, cic, a, b, v);     // out[a][b] = sum_x C[a][x] S[x][b]
#pragma unroll
        for (int blk = 0; blk < 6; ++blk) v[blk] = fmaf(0.25f, v[blk], 128.0f);
        jp_put(A, a, b, v);
        __syncthreads();
        // inverse: chroma by pixel repetition, the decoder's matrix on (Y, Cb - 128, Cr - 128), clamp to [0, 255], / 255
        const float cb = A[4 * JP_BLOCK + a * JP_PITCH + b] - 128.0f, cr = A[5 * JP_BLOCK + a * JP_PITCH + b] - 128.0f;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int y = py + dy, x = px + dx;
                const int ly = 2 * a + dy, lx = 2 * b + dx;
                const float yy = A[((ly >> 3) * 2 + (lx >> 3)) * JP_BLOCK + (ly & 7) * JP_PITCH + (lx & 7)];
                if (live && y < H && x < W) {
                    const long long o = (long long)y * W + x;
                    const float r = fmaf(1.4019999504089355f, cr, yy);
                    const float g = fmaf(-0.714136004447937f, cr, fmaf(-0.34413599967956543f, cb, yy));
                    const float bl = fmaf(1.7719999551773071f, cb, yy);
                    outp[o] = __fdiv_rn(fminf(fmaxf(r, 0.0f), 255.0f), 255.0f);
                    outp[HW + o] = __fdiv_rn(fminf(fmaxf(g, 0.0f), 255.0f), 255.0f);
                    outp[2 * HW + o] = __fdiv_rn(fminf(fmaxf(bl, 0.0f), 255.0f), 255.0f);
                }
            }
        __syncthreads();   // (the next MCU of this wave overwrites A)
    }
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------
extern "C" {

// the one launch of F.interpolate's kernels: rs_interp's, and rs_blur_resize's (bilinear) when it has no kernel.  The callers have checked.
int rs_interp_launch(const float* in, float* out, long long planes, int H, int W, int Ho, int Wo, double step_h, double step_w, int mode, int clamp,
                     hipStream_t st) {
    const ImgAxis ah{step_h, H, Ho}, aw{step_w, W, Wo};
    const int pp = mode == RS_INTERP_BILINEAR ? IP_PLANES_BILINEAR : 1;
    const dim3 grid((unsigned)((Wo + 63) / 64), (unsigned)std::min((Ho + 3) / 4, 65535), (unsigned)std::min<long long>((planes + pp - 1) / pp, 65535));
    if (mode == RS_INTERP_BILINEAR) hipLaunchKernelGGL(interp_bilinear_kernel, grid, dim3(64, 4), 0, st, in, out, ah, aw, planes, clamp);
    else hipLaunchKernelGGL(interp_kernel, grid, dim3(64, 4), 0, st, in, out, ah, aw, planes, mode, clamp);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_filter2d(const float* in, const float* kernels, float* out, int B, int C, int H, int W, int k, int Bk, int clamp, void* stream) {
    const std::string who = "rs_filter2d: ";
    if (!in || !kernels || !out) return img_fail(who, "null tensor (in / kernels / out)");
    if (B < 1 || C < 1 || H < 1 || W < 1) return img_fail(who, "B, C, H and W must be positive");
    if (k < 1 || k > FL_KMAX || k % 2 == 0) return img_fail(who, "k must be odd and at most 21");
    if (k / 2 >= std::min(H, W)) return img_fail(who, "k / 2 must be below min(H, W) (one reflection per border)");
    if (Bk != 1 && Bk != B) return img_fail(who, "Bk must be 1 (one kernel for the batch) or B (one per image)");
    if (!img_is_flag(clamp)) return img_fail(who, "clamp must be 0 or 1");
    if (!img_plane_fits(H, W)) return img_fail(who, "a plane is too large (a side above 2^28 or more than 2^40 pixels)");
    const long long planes = (long long)B * C;
    if (img_overlaps(in, planes * H * W * sizeof(float), out, planes * H * W * sizeof(float)))
        return img_fail(who, "`out` overlaps `in` (workgroups read their neighbours' pixels of in: not in place)");
    const int tiles_x = (W + FL_TC - 1) / FL_TC, tiles_y = (H + FL_TR - 1) / FL_TR;
    const long long total = planes * tiles_x * tiles_y;
    hipLaunchKernelGGL(filter2d_kernel, dim3((unsigned)std::min<long long>(total, 1 << 20)), dim3(FL_THREADS), 0, (hipStream_t)stream, in, kernels,
                       out, C, H, W, k, Bk == 1 ? 0 : 1, tiles_x, tiles_y, total, clamp);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_interp(const float* in, float* out, int B, int C, int H, int W, int Ho, int Wo, double scale_h, double scale_w, int mode, int clamp,
              void* stream) {
    const std::string who = "rs_interp: ";
    if (!in || !out) return img_fail(who, "null tensor (in / out)");
    if (B < 1 || C < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1) return img_fail(who, "B, C, H, W, Ho and Wo must be positive");
    if (mode != RS_INTERP_AREA && mode != RS_INTERP_BILINEAR && mode != RS_INTERP_BICUBIC) return img_fail(who, "mode must be 0 (area), 1 (bilinear) or 2 (bicubic)");
    if (!img_is_flag(clamp)) return img_fail(who, "clamp must be 0 or 1");
    if (!img_plane_fits(H, W) || !img_plane_fits(Ho, Wo)) return img_fail(who, "a plane is too large (a side above 2^28 or more than 2^40 pixels)");
    if ((scale_h == 0.0) != (scale_w == 0.0)) return img_fail(who, "scale_h and scale_w are both 0 (a size was given) or both a scale factor");
    double step_h, step_w;
    if (scale_h == 0.0) {
        const double sh = (double)Ho / H, sw = (double)Wo / W;
        if (!(sh >= 0.125 && sh <= 8.0) || !(sw >= 0.125 && sw <= 8.0)) return img_fail(who, "the scales Ho / H and Wo / W must lie in [1/8, 8]");
        step_h = (double)H / Ho;
        step_w = (double)W / Wo;
    } else {
        if (!(scale_h >= 0.125 && scale_h <= 8.0) || !(scale_w >= 0.125 && scale_w <= 8.0))
            return img_fail(who, "scale_h and scale_w must lie in [1/8, 8]");
        if ((double)Ho != std::floor((double)H * scale_h) || (double)Wo != std::floor((double)W * scale_w))
            return img_fail(who, "with a scale factor the output must be floor(H * scale_h) x floor(W * scale_w)");
        step_h = 1.0 / scale_h;
        step_w = 1.0 / scale_w;
    }
    const long long planes = (long long)B * C;
    if (img_overlaps(in, planes * H * W * sizeof(float), out, planes * Ho * Wo * sizeof(float))) return img_fail(who, "`out` overlaps `in` (not in place)");
    return rs_interp_launch(in, out, planes, H, W, Ho, Wo, step_h, step_w, mode, clamp, (hipStream_t)stream);
}

int rs_jpeg(const float* in, float* out, const float* quality, int B, int C, int H, int W, void* stream) {
    const std::string who = "rs_jpeg: ";
    if (!in || !out || !quality) return img_fail(who, "null pointer (in / out / quality)");
    if (B < 1 || B > RS_MAX_ROWS) return img_fail(who, "B must be 1 .. RS_MAX_ROWS (the qualities travel by value)");
    if (C != 3) return img_fail(who, "C must be 3 (RGB)");
    if (H < 1 || W < 1) return img_fail(who, "H and W must be positive");
    if (!img_plane_fits(H, W)) return img_fail(who, "a plane is too large (a side above 2^28 or more than 2^40 pixels)");
    JpFactors fac{};
    for (int b = 0; b < B; ++b) {
        const float q = quality[b];
        if (!(q > 0.0f && q < 100.0f)) return img_fail(who, "every quality must lie in (0, 100) (at 100 the factor is 0 and the quantiser divides by it)");
        fac.f[b] = (q < 50.0f ? 5000.0f / q : 200.0f - q * 2.0f) / 100.0f;   // fp32, as the reference's tensor arithmetic
    }
    const long long n = (long long)B * 3 * H * W;
    if (in != out && img_overlaps(in, n * sizeof(float), out, n * sizeof(float))) return img_fail(who, "`out` partly overlaps `in` (in place or apart)");
    const int mcus_x = (W + 15) / 16, mcus_y = (H + 15) / 16;
    const long long total = (long long)B * mcus_x * mcus_y, groups = (total + JP_WAVES - 1) / JP_WAVES;
    hipLaunchKernelGGL(jpeg_kernel, dim3((unsigned)std::min<long long>(groups, 1 << 20)), dim3(64 * JP_WAVES), 0, (hipStream_t)stream, in, out, fac, H, W,
                       mcus_x, mcus_y, total, groups);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}   // extern "C"

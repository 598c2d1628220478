// rs_blur_resize (include/resshift_hip.h "face degradation"): out = bilinear(filter2D(in, kernels), size = (Ho, Wo)) with a
// kernel of up to 41 taps, the filter evaluated ONLY where the resize reads it and no blurred tensor in HBM; without a kernel the resize
// alone.  filter2D is rs_filter2d's function (cross-correlation behind torch's `reflect`, taps in row-major ascending order with fmaf),
// bilinear is rs_interp's size-given rule - the same expressions, so equal sizes give rs_filter2d's bits and no kernel gives rs_interp's.
// Every output is a function of its image and its own index alone: a batch is bit for bit its B = 1 calls.
//
//   blur_resize_dense   both steps H / Ho, W / Wo <= BR_SWITCH_STEP.  A workgroup owns the outputs of a plane whose blurred samples lie in ONE
//                       contiguous block of at most 34 x 66 - floor(32 / step) x floor(64 / step) outputs, so the block is full at every
//                       step - whose mirrored source footprint (+ k - 1) is staged in LDS as rs_filter2d stages its own; a thread owns
//                       four rows of one blurred column; the block is blurred whole, read or not.
//   blur_resize_sparse  beyond: an output reads four blurred samples that its neighbours do not.  A workgroup owns 8 x 8 outputs: the 16
//                       rows {y0, y1} x 16 columns {x0, x1} they read are 256 blurred samples, one per thread, taps straight from global
//                       memory.
// kernels == NULL is rs_interp's own bilinear launch (rs_interp_launch, degrade.hip).
#include "image_common.h"

constexpr int BR_KMAX = 41;
constexpr int BR_THREADS = 256;
constexpr int BR_RMAX = 34, BR_CMAX = 66;                             // dense: the blurred block of a tile
constexpr int BR_TOY_MAX = 64, BR_TOX_MAX = 128;                      // its outputs at most (enlargements)
#ifndef BR_SWITCH_STEP
#define BR_SWITCH_STEP 4.5                                            // dense up to this step, sparse beyond (DESIGN.md 7i has the measurement)
#endif
constexpr int BR_PITCH = BR_CMAX + BR_KMAX - 1;
constexpr int BR_ROWS = BR_RMAX + BR_KMAX - 1 + 3;                    // (+ 3: the last thread's four rows may overhang the block)
constexpr int BR_SP = 8;                                              // sparse: 8 x 8 outputs

__global__ __launch_bounds__(BR_THREADS) void blur_resize_dense(const float* __restrict__ in, const float* __restrict__ kern, float* __restrict__ out,
                                                                ImgAxis ah, ImgAxis aw, int C, int k, int per_image, int toy, int tox, int tiles_x,
                                                                int tiles_y, long long total, int clamp) {
    __shared__ float tile[BR_ROWS * BR_PITCH];
    __shared__ float blur[BR_RMAX * BR_CMAX];
    __shared__ float wk[BR_KMAX * BR_KMAX];
    const int H = ah.n, W = aw.n, Ho = ah.m, Wo = aw.m;
    const int tid = threadIdx.x, p = k / 2;
    for (long long t = blockIdx.x; t < total; t += gridDim.x) {
        const int tx = (int)(t % tiles_x);
        const long long q = t / tiles_x;
        const int ty = (int)(q % tiles_y);
        const long long plane = q / tiles_y;
        const int oy0 = ty * toy, ox0 = tx * tox;
        const int ny = min(toy, Ho - oy0), nx = min(tox, Wo - ox0);
        int ylo, yhi, xlo, xhi, unused;
        float fr;
        img_source2(ah, oy0, &ylo, &unused, &fr);
        img_source2(ah, oy0 + ny - 1, &unused, &yhi, &fr);
        img_source2(aw, ox0, &xlo, &unused, &fr);
        img_source2(aw, ox0 + nx - 1, &unused, &xhi, &fr);
        const int R = min(yhi - ylo + 1, BR_RMAX), Cn = min(xhi - xlo + 1, BR_CMAX);   // (the launcher's tile keeps them inside)
        const float* inp = in + plane * H * W;
        const float* kp = kern + (per_image ? (plane / C) * k * k : 0);
        img_stage_footprint(inp, kp, tile, wk, BR_PITCH, ylo, xlo, R, Cn, k, p, H, W, tid, BR_THREADS);
        __syncthreads();
        const int groups = (R + 3) / 4;
        for (int i = tid; i < Cn * groups; i += BR_THREADS) {
            const int rg = i / Cn, c = i - rg * Cn, r0 = rg * 4;
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int ky = 0; ky < k; ++ky)
                for (int kx = 0; kx < k; ++kx) {
                    const float w = wk[ky * k + kx];
#pragma unroll
                    for (int j = 0; j < 4; ++j)   // (rows past R read staged or stale LDS inside the array and are not kept)
                        acc[j] = fmaf(w, tile[(r0 + j + ky) * BR_PITCH + c + kx], acc[j]);
                }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (r0 + j < R) blur[(r0 + j) * BR_CMAX + c] = acc[j];
        }
        __syncthreads();
        for (int i = tid; i < ny * nx; i += BR_THREADS) {
            const int ly = i / nx, lx = i - ly * nx;
            int y0, y1, x0, x1;
            float fy, fx;
            img_source2(ah, oy0 + ly, &y0, &y1, &fy);
            img_source2(aw, ox0 + lx, &x0, &x1, &fx);
            y0 = min(y0 - ylo, R - 1); y1 = min(y1 - ylo, R - 1); x0 = min(x0 - xlo, Cn - 1); x1 = min(x1 - xlo, Cn - 1);
            out[plane * Ho * Wo + (long long)(oy0 + ly) * Wo + ox0 + lx] =
                img_unit_clamp(img_bilinear(blur[y0 * BR_CMAX + x0], blur[y0 * BR_CMAX + x1], blur[y1 * BR_CMAX + x0], blur[y1 * BR_CMAX + x1], fy, fx), clamp);
        }
        __syncthreads();   // (the next tile of this workgroup overwrites the LDS images)
    }
}

__global__ __launch_bounds__(BR_THREADS) void blur_resize_sparse(const float* __restrict__ in, const float* __restrict__ kern, float* __restrict__ out,
                                                                 ImgAxis ah, ImgAxis aw, int C, int k, int per_image, int tiles_x, int tiles_y,
                                                                 long long total, int clamp) {
    __shared__ float blur[2 * BR_SP][2 * BR_SP];
    __shared__ float wk[BR_KMAX * BR_KMAX];
    const int H = ah.n, W = aw.n, Ho = ah.m, Wo = aw.m;
    const int tid = threadIdx.x, p = k / 2;
    const int ry = tid >> 4, rx = tid & 15;                 // the thread's blurred sample: tap (ry & 1) of output row ry / 2, likewise rx
    for (long long t = blockIdx.x; t < total; t += gridDim.x) {
        const int tx = (int)(t % tiles_x);
        const long long q = t / tiles_x;
        const int ty = (int)(q % tiles_y);
        const long long plane = q / tiles_y;
        const int oy0 = ty * BR_SP, ox0 = tx * BR_SP;
        const float* inp = in + plane * H * W;
        const float* kp = kern + (per_image ? (plane / C) * k * k : 0);
        for (int i = tid; i < k * k; i += BR_THREADS) wk[i] = kp[i];
        __syncthreads();
        int a0, a1;
        float fr;
        img_source2(ah, min(oy0 + (ry >> 1), Ho - 1), &a0, &a1, &fr);   // (outputs past the edge repeat the last one and are not stored)
        const int y = (ry & 1) ? a1 : a0;
        img_source2(aw, min(ox0 + (rx >> 1), Wo - 1), &a0, &a1, &fr);
        const int x = (rx & 1) ? a1 : a0;
        float acc = 0.f;
        for (int ky = 0; ky < k; ++ky) {
            const float* row = inp + (long long)img_reflect(y - p + ky, H) * W;
            for (int kx = 0; kx < k; ++kx) acc = fmaf(wk[ky * k + kx], row[img_reflect(x - p + kx, W)], acc);
        }
        blur[ry][rx] = acc;
        __syncthreads();
        if (tid < BR_SP * BR_SP) {
            const int ly = tid >> 3, lx = tid & 7;
            if (oy0 + ly < Ho && ox0 + lx < Wo) {
                int u0, u1;
                float fy, fx;
                img_source2(ah, oy0 + ly, &u0, &u1, &fy);
                img_source2(aw, ox0 + lx, &u0, &u1, &fx);
                out[plane * Ho * Wo + (long long)(oy0 + ly) * Wo + ox0 + lx] =
                    img_unit_clamp(img_bilinear(blur[2 * ly][2 * lx], blur[2 * ly][2 * lx + 1], blur[2 * ly + 1][2 * lx], blur[2 * ly + 1][2 * lx + 1], fy, fx), clamp);
            }
        }
        __syncthreads();   // (the next tile of this workgroup overwrites the LDS images)
    }
}

extern "C" int rs_blur_resize(const float* in, const float* kernels, float* out, int B, int C, int H, int W, int Ho, int Wo, int k, int Bk, int clamp,
                              void* stream) {
    const std::string who = "rs_blur_resize: ";
    if (!in || !out) return img_fail(who, "null tensor (in / out)");
    if (B < 1 || C < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1) return img_fail(who, "B, C, H, W, Ho and Wo must be positive");
    if (!kernels && k != 0) return img_fail(who, "without kernels k must be 0");
    if (kernels) {
        if (k < 1 || k > BR_KMAX || k % 2 == 0) return img_fail(who, "k must be odd and at most 41");
        if (k / 2 >= std::min(H, W)) return img_fail(who, "k / 2 must be below min(H, W) (one reflection per border)");
        if (Bk != 1 && Bk != B) return img_fail(who, "Bk must be 1 (one kernel for the batch) or B (one per image)");
    }
    if (!img_is_flag(clamp)) return img_fail(who, "clamp must be 0 or 1");
    if (!img_plane_fits(H, W) || !img_plane_fits(Ho, Wo)) return img_fail(who, "a plane is too large (a side above 2^28 or more than 2^40 pixels)");
    const double sh = (double)Ho / H, sw = (double)Wo / W;
    if (!(sh >= 1.0 / 64 && sh <= 64.0) || !(sw >= 1.0 / 64 && sw <= 64.0)) return img_fail(who, "the scales Ho / H and Wo / W must lie in [1/64, 64]");
    const long long planes = (long long)B * C;
    if (img_overlaps(in, planes * H * W * sizeof(float), out, planes * Ho * Wo * sizeof(float))) return img_fail(who, "`out` overlaps `in` (not in place)");
    const ImgAxis ah{(double)H / Ho, H, Ho}, aw{(double)W / Wo, W, Wo};
    const hipStream_t st = (hipStream_t)stream;
    if (!kernels) return rs_interp_launch(in, out, planes, H, W, Ho, Wo, ah.step, aw.step, RS_INTERP_BILINEAR, clamp, st);
    if (ah.step <= BR_SWITCH_STEP && aw.step <= BR_SWITCH_STEP && std::max(ah.step, aw.step) <= BR_RMAX - 2) {
        // the outputs whose blurred samples span at most BR_RMAX x BR_CMAX: floor(a + step (n - 1)) - floor(a) + 2 <= ceil(step (n - 1)) + 2
        const int toy = std::max(1, std::min(BR_TOY_MAX, (int)((BR_RMAX - 2) / ah.step))), tox = std::max(1, std::min(BR_TOX_MAX, (int)((BR_CMAX - 2) / aw.step)));
        const int tiles_x = (Wo + tox - 1) / tox, tiles_y = (Ho + toy - 1) / toy;
        const long long total = planes * tiles_x * tiles_y;
        hipLaunchKernelGGL(blur_resize_dense, dim3((unsigned)std::min<long long>(total, 1 << 20)), dim3(BR_THREADS), 0, st, in, kernels, out, ah, aw, C, k,
                           Bk == 1 ? 0 : 1, toy, tox, tiles_x, tiles_y, total, clamp);
    } else {
        const int tiles_x = (Wo + BR_SP - 1) / BR_SP, tiles_y = (Ho + BR_SP - 1) / BR_SP;
        const long long total = planes * tiles_x * tiles_y;
        hipLaunchKernelGGL(blur_resize_sparse, dim3((unsigned)std::min<long long>(total, 1 << 20)), dim3(BR_THREADS), 0, st, in, kernels, out, ah, aw, C, k,
                           Bk == 1 ? 0 : 1, tiles_x, tiles_y, total, clamp);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

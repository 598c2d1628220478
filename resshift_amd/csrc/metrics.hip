// PSNR / SSIM of two image batches against each other, on uint8 pixels (include/resshift_hip.h "image metrics").
//
// TWO launches, no intermediate tensor in HBM but the per-tile partials.
//   1. metrics_tile_kernel, one workgroup of 256 threads per (image, channel, 32 x 32 tile of SSIM-map positions):
//        a. the tile's 42 x 42 pixels (tile + the 10-pixel reach of the 11-tap window) of both images go to LDS as uint8 - a float input
//           is quantised by rs_sample_to_u8 (THE quantiser of rs_output_to_u8), an RGB pixel is reduced to Y by rs_rgb_to_y when asked;
//           the pixels the tile owns (its 32 x 32, and the 10 extra rows / columns when it is the last of its axis, so that the tiles
//           partition the cropped image) add (a - b)^2 to an int64;
//        b. horizontal 11-tap pass of the five moments (a, b, a^2, b^2, ab - the products formed as exact integers) in fp64 into LDS,
//           lanes along columns: 32 consecutive doubles per 32-lane half (no ds_read_b64 bank conflict);
//        c. vertical pass from there and the SSIM map value of each position, never stored;
//        d. the values and the SSE are summed within the wave (__shfl_down, a fixed tree) and across the four waves in wave order, and
//           ONE partial per (image, channel, tile) goes to the workspace.
//   2. metrics_sum_kernel, one workgroup per image: the partials of each channel in a fixed order (a strided sum per thread, then a
//      tree in LDS), the division by the number of positions, the mean over the channels.
// No floating-point atomics and no "last block" counter: every partial is a function of its tile's pixels alone, the order of every
// sum is fixed by the image's shape, so a result is the same bits run to run and whatever else the batch holds.
//
// fp64 throughout: E[a^2] - mu^2 cancels up to eight digits on flat regions, which raw fp32 moments do not survive.  The
// map expression is kept from contraction: for identical images the numerator and the denominator are then the same bits, and SSIM is 1.
#include "image_common.h"
#include <cmath>

constexpr int MT_T = 32;                   // SSIM-map positions per tile side
constexpr int MT_TAPS = 11;
constexpr int MT_IN = MT_T + MT_TAPS - 1;  // 42 pixels per tile side
constexpr int MT_PITCH = 44;               // bytes per LDS pixel row
constexpr int MT_THREADS = 256;

struct MtWindow { double g[MT_TAPS]; };    // exp(-(i - 5)^2 / 4.5) / their sum, in fp64

// the uint8 pixel (image n, channel c, row y, column x): uint8 [B,H,W,C] as stored, fp32 [B,C,H,W] in [-1,1] quantised
__device__ __forceinline__ int mt_pixel(const void* p, int is_float, long long n, int c, int y, int x, int C, int H, int W) {
    if (is_float) return rs_sample_to_u8(((const float*)p)[((n * C + c) * H + y) * W + x]);
    return ((const unsigned char*)p)[((n * H + y) * W + x) * C + c];
}

__device__ __forceinline__ int mt_value(const void* p, int is_float, long long n, int c, int y, int x, int C, int H, int W, int ycbcr) {
    if (!ycbcr) return mt_pixel(p, is_float, n, c, y, x, C, H, W);
    return rs_rgb_to_y(mt_pixel(p, is_float, n, 0, y, x, C, H, W), mt_pixel(p, is_float, n, 1, y, x, C, H, W),
                       mt_pixel(p, is_float, n, 2, y, x, C, H, W));
}

__device__ double mt_ssim(double mu1, double mu2, double e11, double e22, double e12) {
#pragma clang fp contract(off)
    const double C1 = 6.5025, C2 = 58.5225;
    const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
    const double s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu1_mu2;
    const double num = (2.0 * mu1_mu2 + C1) * (2.0 * s12 + C2);
    const double den = ((mu1_sq + mu2_sq) + C1) * ((s1 + s2) + C2);
    return num / den;
}

__global__ __launch_bounds__(MT_THREADS) void metrics_tile_kernel(const void* __restrict__ a, const void* __restrict__ b, int a_is_float,
                                                                  int b_is_float, int C, int H, int W, int border, int ycbcr, int tiles_x,
                                                                  int tiles_y, MtWindow win, double* __restrict__ part,
                                                                  long long* __restrict__ sse_part) {
    __shared__ unsigned char sa[MT_IN * MT_PITCH], sb[MT_IN * MT_PITCH];
    __shared__ double mid[5][MT_IN][MT_T];
    __shared__ double wsum[MT_THREADS / 64];
    __shared__ long long wsse[MT_THREADS / 64];
    const int tid = threadIdx.x;
    const int Ce = ycbcr ? 1 : C;
    const long long t = blockIdx.x;
    const int tx = (int)(t % tiles_x);
    long long q = t / tiles_x;
    const int ty = (int)(q % tiles_y);
    q /= tiles_y;
    const int c = (int)(q % Ce);
    const long long n = q / Ce;
    const int Hv = H - 2 * border - (MT_TAPS - 1), Wv = W - 2 * border - (MT_TAPS - 1);   // the SSIM map
    const int y0 = ty * MT_T, x0 = tx * MT_T;
    const int nr = min(MT_T, Hv - y0), nc = min(MT_T, Wv - x0);
    const int rows = nr + MT_TAPS - 1, cols = nc + MT_TAPS - 1;      // pixels under the tile: y0 + rows <= H - 2 border
    const int own_r = ty == tiles_y - 1 ? rows : nr, own_c = tx == tiles_x - 1 ? cols : nc;
    // a. pixels to LDS, SSE of the owned ones
    long long sse = 0;
    for (int i = tid; i < MT_IN * MT_IN; i += MT_THREADS) {
        const int r = i / MT_IN, x = i - r * MT_IN;
        if (r >= rows || x >= cols) continue;
        const int va = mt_value(a, a_is_float, n, c, border + y0 + r, border + x0 + x, C, H, W, ycbcr);
        const int vb = mt_value(b, b_is_float, n, c, border + y0 + r, border + x0 + x, C, H, W, ycbcr);
        sa[r * MT_PITCH + x] = (unsigned char)va;
        sb[r * MT_PITCH + x] = (unsigned char)vb;
        if (r < own_r && x < own_c) sse += (long long)((va - vb) * (va - vb));
    }
    __syncthreads();
    // b. horizontal pass
    for (int i = tid; i < rows * MT_T; i += MT_THREADS) {
        const int r = i / MT_T, x = i % MT_T;
        if (x >= nc) continue;
        double m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0;
#pragma unroll
        for (int k = 0; k < MT_TAPS; ++k) {
            const int pa = sa[r * MT_PITCH + x + k], pb = sb[r * MT_PITCH + x + k];
            const double w = win.g[k];
            m0 = fma(w, (double)pa, m0);
            m1 = fma(w, (double)pb, m1);
            m2 = fma(w, (double)(pa * pa), m2);
            m3 = fma(w, (double)(pb * pb), m3);
            m4 = fma(w, (double)(pa * pb), m4);
        }
        mid[0][r][x] = m0;
        mid[1][r][x] = m1;
        mid[2][r][x] = m2;
        mid[3][r][x] = m3;
        mid[4][r][x] = m4;
    }
    __syncthreads();
    // c. vertical pass and the map
    double sum = 0;
    for (int i = tid; i < nr * MT_T; i += MT_THREADS) {
        const int r = i / MT_T, x = i % MT_T;
        if (x >= nc) continue;
        double m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0;
#pragma unroll
        for (int k = 0; k < MT_TAPS; ++k) {
            const double w = win.g[k];
            m0 = fma(w, mid[0][r + k][x], m0);
            m1 = fma(w, mid[1][r + k][x], m1);
            m2 = fma(w, mid[2][r + k][x], m2);
            m3 = fma(w, mid[3][r + k][x], m3);
            m4 = fma(w, mid[4][r + k][x], m4);
        }
        sum += mt_ssim(m0, m1, m2, m3, m4);
    }
    // d. one partial per tile
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_down(sum, off);
        sse += __shfl_down(sse, off);
    }
    if ((tid & 63) == 0) {
        wsum[tid >> 6] = sum;
        wsse[tid >> 6] = sse;
    }
    __syncthreads();
    if (tid == 0) {
        part[t] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        sse_part[t] = wsse[0] + wsse[1] + wsse[2] + wsse[3];
    }
}

// image blockIdx.x: its channels' partials, [channel][tile], summed in an order the shape alone fixes
__global__ __launch_bounds__(MT_THREADS) void metrics_sum_kernel(const double* __restrict__ part, const long long* __restrict__ sse_part, int Ce,
                                                                 long long tiles, long long positions, long long* __restrict__ sse_out,
                                                                 double* __restrict__ ssim_out) {
    __shared__ double sd[MT_THREADS];
    __shared__ long long sl[MT_THREADS];
    const int tid = threadIdx.x;
    double total = 0;
    long long sse = 0;
    for (int c = 0; c < Ce; ++c) {
        const long long base = ((long long)blockIdx.x * Ce + c) * tiles;
        double s = 0;
        long long e = 0;
        for (long long i = tid; i < tiles; i += MT_THREADS) {
            s += part[base + i];
            e += sse_part[base + i];
        }
        sd[tid] = s;
        sl[tid] = e;
        __syncthreads();
        for (int st = MT_THREADS / 2; st > 0; st >>= 1) {
            if (tid < st) {
                sd[tid] += sd[tid + st];
                sl[tid] += sl[tid + st];
            }
            __syncthreads();
        }
        if (tid == 0) {
            total += sd[0] / (double)positions;
            sse += sl[0];
        }
        __syncthreads();
    }
    if (tid == 0) {
        ssim_out[blockIdx.x] = total / (double)Ce;
        sse_out[blockIdx.x] = sse;
    }
}

__global__ void rgb_to_y_kernel(const unsigned char* __restrict__ rgb, unsigned char* __restrict__ y, long long pixels) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += (long long)gridDim.x * blockDim.x)
        y[i] = rs_rgb_to_y(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------
namespace {

// null when the geometry is one the kernels take; the tile counts come back through tiles_x / tiles_y
const char* mt_geometry_error(int B, int C, int H, int W, int border, int ycbcr, std::string* text, int* tiles_x, int* tiles_y) {
    if (B < 1 || H < 1 || W < 1) return "B, H and W must be positive";
    if (C != 1 && C != 3) return "C must be 1 or 3";
    if (!img_is_flag(ycbcr)) return "ycbcr must be 0 or 1";
    if (ycbcr && C != 3) return "ycbcr needs C == 3";
    if (border < 0) return "border must not be negative";
    if (!img_plane_fits(H, W)) return "an image is too large (a side above 2^28 or more than 2^40 pixels)";
    const long long Hc = (long long)H - 2LL * border, Wc = (long long)W - 2LL * border;
    if (Hc < MT_TAPS || Wc < MT_TAPS) {
        *text = "the cropped image is " + std::to_string(Hc) + " x " + std::to_string(Wc) + " (" + std::to_string(H) + " x " + std::to_string(W) +
                ", border " + std::to_string(border) + "): the 11 x 11 window needs at least 11 x 11";
        return text->c_str();
    }
    *tiles_x = (int)((Wc - (MT_TAPS - 1) + MT_T - 1) / MT_T);
    *tiles_y = (int)((Hc - (MT_TAPS - 1) + MT_T - 1) / MT_T);
    if ((long long)B * (ycbcr ? 1 : C) * *tiles_x * *tiles_y > 0x7fffffffLL) return "more than 2^31 - 1 tiles in one call";
    return nullptr;
}

}   // namespace

extern "C" {

size_t rs_metrics_work_bytes(int B, int C, int H, int W, int border, int ycbcr) {
    std::string text;
    int tiles_x = 0, tiles_y = 0;
    if (mt_geometry_error(B, C, H, W, border, ycbcr, &text, &tiles_x, &tiles_y)) return 0;
    return (size_t)B * (ycbcr ? 1 : C) * tiles_x * tiles_y * (sizeof(double) + sizeof(long long));
}

int rs_metrics(const void* a, const void* b, int a_is_float, int b_is_float, int B, int C, int H, int W, int border, int ycbcr,
               long long* sse_out, double* ssim_out, void* work, size_t work_bytes, void* stream) {
    const std::string who = "rs_metrics: ";
    if (!a || !b || !sse_out || !ssim_out) return img_fail(who, "null tensor (a / b / sse_out / ssim_out)");
    if (!img_is_flag(a_is_float) || !img_is_flag(b_is_float)) return img_fail(who, "a_is_float and b_is_float must be 0 or 1");
    std::string text;
    int tiles_x = 0, tiles_y = 0;
    if (const char* e = mt_geometry_error(B, C, H, W, border, ycbcr, &text, &tiles_x, &tiles_y)) return img_fail(who, e);
    const size_t need = rs_metrics_work_bytes(B, C, H, W, border, ycbcr);
    if (!work || work_bytes < need)
        return img_fail(who, "the workspace is too small: " + std::to_string(work ? work_bytes : 0) + " bytes, rs_metrics_work_bytes asks for " +
                                  std::to_string(need));
    if (((uintptr_t)work & 7) || ((uintptr_t)sse_out & 7) || ((uintptr_t)ssim_out & 7))
        return img_fail(who, "the workspace, sse_out and ssim_out must be aligned to 8 bytes");
    if ((a_is_float && ((uintptr_t)a & 3)) || (b_is_float && ((uintptr_t)b & 3)))
        return img_fail(who, "a float input must be aligned to 4 bytes");
    MtWindow win;
    double total = 0;
    for (int i = 0; i < MT_TAPS; ++i) total += (win.g[i] = std::exp(-(double)((i - 5) * (i - 5)) / 4.5));
    for (int i = 0; i < MT_TAPS; ++i) win.g[i] /= total;
    const int Ce = ycbcr ? 1 : C;
    const long long tiles = (long long)tiles_x * tiles_y, all = (long long)B * Ce * tiles;
    double* part = (double*)work;
    long long* sse_part = (long long*)(part + all);
    hipLaunchKernelGGL(metrics_tile_kernel, dim3((unsigned)all), dim3(MT_THREADS), 0, (hipStream_t)stream, a, b, a_is_float, b_is_float, C, H, W,
                       border, ycbcr, tiles_x, tiles_y, win, part, sse_part);
    if (hipGetLastError() != hipSuccess) return -1;
    const long long positions = (long long)(H - 2 * border - (MT_TAPS - 1)) * (W - 2 * border - (MT_TAPS - 1));
    hipLaunchKernelGGL(metrics_sum_kernel, dim3((unsigned)B), dim3(MT_THREADS), 0, (hipStream_t)stream, (const double*)part,
                       (const long long*)sse_part, Ce, tiles, positions, sse_out, ssim_out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int rs_rgb_to_y_u8(const uint8_t* rgb_hwc, uint8_t* y, size_t pixels, void* stream) {
    const std::string who = "rs_rgb_to_y_u8: ";
    if (!rgb_hwc || !y) return img_fail(who, "null tensor (rgb_hwc / y)");
    if (pixels < 1 || pixels > ((size_t)1 << 40)) return img_fail(who, "pixels must lie in [1, 2^40]");
    if (img_overlaps(rgb_hwc, 3 * pixels, y, pixels)) return img_fail(who, "`y` overlaps `rgb_hwc`");
    const unsigned blocks = (unsigned)std::min<size_t>((pixels + 255) / 256, 65536);
    hipLaunchKernelGGL(rgb_to_y_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rgb_hwc, y, (long long)pixels);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}   // extern "C"

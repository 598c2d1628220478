// rs_jpeg_codec: libjpeg's baseline JPEG round trip (include/resshift_hip.h "face degradation") - 4:2:0, the "islow" integer
// DCT pair, the default tables, "fancy" chroma up-sampling - in ONE launch, the entropy stage (lossless) never materialised (jpeg_encode.hip
// materialises it; the forward half both share is jpeg_common.h).  Between the
// rounding of the input and the division of the output everything is 32-bit integer arithmetic, so the result is a function of the image
// and the quality alone, whatever the mapping, the batch or the position in it.
//
// Mapping.  A workgroup of 256 threads owns a tile of 8 x 4 MCUs (128 x 64 pixels) of one image and keeps three uint8 planes in LDS: the
// tile's Y and the Cb / Cr of the tile PLUS A RING OF ONE MCU (the up-sampler reads one chroma sample past the tile, and a decoded sample
// needs its whole 8 x 8 block).  Three phases, two barriers:
//   1. colour: a thread per 2 x 2 pixel quad of tile + ring: round to 8 bits, RGB -> YCbCr, the 2 x 2 chroma mean; libjpeg's edge rules
//      are clamped source indices.
//   2. blocks: a THREAD PER 8 x 8 BLOCK, the block in registers from the first load to the last store: forward DCT, quantise,
//      dequantise, inverse DCT, with no transposes and no barriers in between.  The tile has 128 Y blocks and, with the ring, 120
//      chroma blocks: 248 of the 256 threads, so the ring costs no time of its own.
//   3. pixels: a thread per output pixel, lanes along a row: triangle up-sampling from the chroma planes, YCbCr -> RGB, / 255.
#include "jpeg_common.h"

constexpr int JC_TX = 8, JC_TY = 4;                          // MCUs of a tile
constexpr int JC_THREADS = 256;
constexpr int JC_YW = JC_TX * 16, JC_YH = JC_TY * 16;        // the tile's Y plane: 128 x 64
constexpr int JC_YP = JC_YW + 8;                             // its pitch in bytes (rows of 8-byte block rows stay 8-byte aligned)
constexpr int JC_CW = (JC_TX + 2) * 8, JC_CH = (JC_TY + 2) * 8;   // a chroma plane with the ring: 80 x 48
constexpr int JC_YBLOCKS = 4 * JC_TX * JC_TY, JC_CBLOCKS = (JC_TX + 2) * (JC_TY + 2);
static_assert(JC_YBLOCKS + 2 * JC_CBLOCKS <= JC_THREADS, "a thread per block");
static_assert(JC_YW * 2 == JC_THREADS, "phase 3 maps a thread to a column of every other row");

// one 8-point pass of jidctint.c; COLS: the first (column) pass
template <bool COLS, int S>
__device__ __forceinline__ void jc_idct8(int* d) {
    const int z1 = (d[2 * S] + d[6 * S]) * JC_0_541;
    const int t2 = z1 - d[6 * S] * JC_1_847, t3 = z1 + d[2 * S] * JC_0_765;
    const int t0 = (d[0] + d[4 * S]) << 13, t1 = (d[0] - d[4 * S]) << 13;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int o0 = d[7 * S], o1 = d[5 * S], o2 = d[3 * S], o3 = d[S];
    jc_odd(o0, o1, o2, o3);
    constexpr int n = COLS ? 11 : 18;
    d[0] = jc_descale(t10 + o3, n);
    d[7 * S] = jc_descale(t10 - o3, n);
    d[S] = jc_descale(t11 + o2, n);
    d[6 * S] = jc_descale(t11 - o2, n);
    d[2 * S] = jc_descale(t12 + o1, n);
    d[5 * S] = jc_descale(t12 - o1, n);
    d[3 * S] = jc_descale(t13 + o0, n);
    d[4 * S] = jc_descale(t13 - o0, n);
}

// an 8 x 8 block of samples at p (pitch bytes per row, 8-byte aligned), coded in place
__device__ __forceinline__ void jc_code_block(unsigned char* p, int pitch, const int* tab, const float* rcp) {
    int d[64];
    jc_forward_block(p, pitch, tab, rcp, d);
#pragma unroll
    for (int i = 0; i < 64; ++i) d[i] *= tab[i];              // dequantise
#pragma unroll
    for (int c = 0; c < 8; ++c) jc_idct8<true, 8>(d + c);
#pragma unroll
    for (int r = 0; r < 8; ++r) jc_idct8<false, 1>(d + r * 8);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        uint2 v{0u, 0u};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v.x |= (unsigned)min(max(d[r * 8 + j] + 128, 0), 255) << (8 * j);
            v.y |= (unsigned)min(max(d[r * 8 + 4 + j] + 128, 0), 255) << (8 * j);
        }
        *reinterpret_cast<uint2*>(p + r * pitch) = v;
    }
}

__device__ __forceinline__ int jc_u8(float x) { return (int)rintf(fminf(fmaxf(x, 0.0f), 1.0f) * 255.0f); }

__global__ __launch_bounds__(JC_THREADS) void jpeg_codec_kernel(const float* __restrict__ in, float* __restrict__ out, JcQuality qual, int H, int W,
                                                                int mcus_x, int mcus_y, int tiles_x, int tiles_y, long long total) {
    __shared__ __align__(16) unsigned char Yp[JC_YH * JC_YP];
    __shared__ __align__(16) unsigned char Cp[2][JC_CH * JC_CW];
    __shared__ int tab[2][64];
    __shared__ float rcp[2][64];
    const int tid = threadIdx.x;
    const long long HW = (long long)H * W;
    const int CHr = (H + 1) >> 1, CWr = (W + 1) >> 1;         // the real chroma samples
    for (long long tile = blockIdx.x; tile < total; tile += gridDim.x) {
        const int tx = (int)(tile % tiles_x);
        const long long tq = tile / tiles_x;
        const int ty = (int)(tq % tiles_y);
        const long long img = tq / tiles_y;
        const int mx0 = tx * JC_TX, my0 = ty * JC_TY;        // the tile's first MCU
        const float* inp = in + img * 3 * HW;
        float* outp = out + img * 3 * HW;
        jc_stage_tables(qual.q[img], tid, tab, rcp);
        // 1. colour.  Quad (qy, qx) of tile + ring is the chroma sample (cy, cx) of the image's padded planes (jc_quad has libjpeg's edge rules)
        const auto px = [&](long long o, int& r, int& g, int& b) { r = jc_u8(inp[o]); g = jc_u8(inp[HW + o]); b = jc_u8(inp[2 * HW + o]); };
        for (int i = tid; i < JC_CH * JC_CW; i += JC_THREADS) {
            const int qy = i / JC_CW, qx = i - qy * JC_CW;
            const int my = my0 - 1 + (qy >> 3), mx = mx0 - 1 + (qx >> 3);
            if (my < 0 || my >= mcus_y || mx < 0 || mx >= mcus_x) continue;   // (no such MCU: its samples are never read)
            const JcQuad qd = jc_quad(px, my * 8 + (qy & 7), mx * 8 + (qx & 7), H, W);
            Cp[0][i] = (unsigned char)qd.cb;
            Cp[1][i] = (unsigned char)qd.cr;
            if (qy >= 8 && qy < JC_CH - 8 && qx >= 8 && qx < JC_CW - 8) jc_quad_store_y(qd, Yp + (qy - 8) * 2 * JC_YP + (qx - 8) * 2, JC_YP);
        }
        __syncthreads();
        // 2. blocks
        if (tid < JC_YBLOCKS) {
            const int by = tid / (2 * JC_TX), bx = tid - by * (2 * JC_TX);
            if (my0 + (by >> 1) < mcus_y && mx0 + (bx >> 1) < mcus_x) jc_code_block(Yp + by * 8 * JC_YP + bx * 8, JC_YP, tab[0], rcp[0]);
        } else if (tid < JC_YBLOCKS + 2 * JC_CBLOCKS) {
            const int c = (tid - JC_YBLOCKS) / JC_CBLOCKS, r = (tid - JC_YBLOCKS) - c * JC_CBLOCKS;
            const int by = r / (JC_TX + 2), bx = r - by * (JC_TX + 2);
            const int my = my0 - 1 + by, mx = mx0 - 1 + bx;
            if (my >= 0 && my < mcus_y && mx >= 0 && mx < mcus_x) jc_code_block(Cp[c] + by * 8 * JC_CW + bx * 8, JC_CW, tab[1], rcp[1]);
        }
        __syncthreads();
        // 3. pixels: "fancy" h2v2 up-sampling over the real chroma samples (the first / last real row and column stand in for their missing
        // neighbours), YCbCr -> RGB, clamp, / 255
        {
            const int lx = tid & (JC_YW - 1), x = mx0 * 16 + lx;
            const int cx = x >> 1, nx = (x & 1) ? min(cx + 1, CWr - 1) : max(cx - 1, 0);
            const int lcx = cx - (mx0 - 1) * 8, lnx = nx - (mx0 - 1) * 8;
            const int rnd = (x & 1) ? 7 : 8;
            if (x < W)
                for (int ly = tid >> 7; ly < JC_YH; ly += 2) {
                    const int y = my0 * 16 + ly;
                    if (y >= H) break;
                    const int cy = y >> 1, fy = (y & 1) ? min(cy + 1, CHr - 1) : max(cy - 1, 0);
                    const int near = (cy - (my0 - 1) * 8) * JC_CW, far = (fy - (my0 - 1) * 8) * JC_CW;
                    int ch[2];
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const int s = 3 * Cp[c][near + lcx] + Cp[c][far + lcx], sn = 3 * Cp[c][near + lnx] + Cp[c][far + lnx];
                        ch[c] = ((3 * s + sn + rnd) >> 4) - 128;
                    }
                    const int yy = Yp[ly * JC_YP + lx];
                    const int r = yy + ((jc_fix16(1.402) * ch[1] + 32768) >> 16);
                    const int b = yy + ((jc_fix16(1.772) * ch[0] + 32768) >> 16);
                    const int g = yy + ((-jc_fix16(.34414) * ch[0] - jc_fix16(.71414) * ch[1] + 32768) >> 16);
                    const long long o = (long long)y * W + x;
                    outp[o] = __fdiv_rn((float)min(max(r, 0), 255), 255.0f);
                    outp[HW + o] = __fdiv_rn((float)min(max(g, 0), 255), 255.0f);
                    outp[2 * HW + o] = __fdiv_rn((float)min(max(b, 0), 255), 255.0f);
                }
        }
        __syncthreads();   // (the next tile of this workgroup overwrites the planes and the tables)
    }
}

extern "C" int rs_jpeg_codec(const float* in, float* out, const int* quality, int B, int C, int H, int W, void* stream) {
    const std::string who = "rs_jpeg_codec: ";
    if (!in || !out || !quality) return img_fail(who, "null pointer (in / out / quality)");
    if (B < 1 || B > RS_MAX_ROWS) return img_fail(who, "B must be 1 .. RS_MAX_ROWS (the qualities travel by value)");
    if (C != 3) return img_fail(who, "C must be 3 (RGB)");
    if (H < 8 || W < 8) return img_fail(who, "H and W must be at least 8");
    if (!img_plane_fits(H, W)) return img_fail(who, "a plane is too large (a side above 2^28 or more than 2^40 pixels)");
    JcQuality qual{};
    for (int b = 0; b < B; ++b) {
        if (quality[b] < 1 || quality[b] > 100) return img_fail(who, "every quality must be an integer in 1 .. 100");
        qual.q[b] = quality[b];
    }
    const long long n = (long long)B * 3 * H * W;
    if (img_overlaps(in, n * sizeof(float), out, n * sizeof(float))) return img_fail(who, "`out` overlaps `in` (a tile reads the chroma ring of its neighbours: not in place)");
    const int mcus_x = (W + 15) / 16, mcus_y = (H + 15) / 16;
    const int tiles_x = (mcus_x + JC_TX - 1) / JC_TX, tiles_y = (mcus_y + JC_TY - 1) / JC_TY;
    const long long total = (long long)B * tiles_x * tiles_y;
    hipLaunchKernelGGL(jpeg_codec_kernel, dim3((unsigned)std::min<long long>(total, 1 << 20)), dim3(JC_THREADS), 0, (hipStream_t)stream, in, out, qual, H,
                       W, mcus_x, mcus_y, tiles_x, tiles_y, total);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

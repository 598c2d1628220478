// rs_jpeg_codec: libjpeg's baseline JPEG round trip (include/resshift_hip.h "face degradation") - 4:2:0, the "islow" integer
// DCT pair, the default tables, "fancy" chroma up-sampling - in ONE launch, the entropy stage (lossless) never materialised.  Between the
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
#include "image_common.h"

constexpr int JC_TX = 8, JC_TY = 4;                          // MCUs of a tile
constexpr int JC_THREADS = 256;
constexpr int JC_YW = JC_TX * 16, JC_YH = JC_TY * 16;        // the tile's Y plane: 128 x 64
constexpr int JC_YP = JC_YW + 8;                             // its pitch in bytes (rows of 8-byte block rows stay 8-byte aligned)
constexpr int JC_CW = (JC_TX + 2) * 8, JC_CH = (JC_TY + 2) * 8;   // a chroma plane with the ring: 80 x 48
constexpr int JC_YBLOCKS = 4 * JC_TX * JC_TY, JC_CBLOCKS = (JC_TX + 2) * (JC_TY + 2);
static_assert(JC_YBLOCKS + 2 * JC_CBLOCKS <= JC_THREADS, "a thread per block");
static_assert(JC_YW * 2 == JC_THREADS, "phase 3 maps a thread to a column of every other row");

constexpr int jc_fix16(double c) { return (int)(c * 65536 + .5); }
constexpr int jc_fix13(double c) { return (int)(c * 8192 + .5); }
constexpr int JC_0_298 = jc_fix13(0.298631336), JC_0_390 = jc_fix13(0.390180644), JC_0_541 = jc_fix13(0.541196100), JC_0_765 = jc_fix13(0.765366865),
              JC_0_899 = jc_fix13(0.899976223), JC_1_175 = jc_fix13(1.175875602), JC_1_501 = jc_fix13(1.501321110), JC_1_847 = jc_fix13(1.847759065),
              JC_1_961 = jc_fix13(1.961570560), JC_2_053 = jc_fix13(2.053119869), JC_2_562 = jc_fix13(2.562915447), JC_3_072 = jc_fix13(3.072711026);

// Annex K in natural order, [vertical frequency][horizontal]: luminance, chrominance
__constant__ int JC_BASE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99},
};

struct JcQuality { int q[RS_MAX_ROWS]; };

__device__ __forceinline__ int jc_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// the odd part both transforms share, on (t0, t1, t2, t3) = forward (t4, t5, t6, t7) / inverse (i7, i5, i3, i1)
__device__ __forceinline__ void jc_odd(int& t0, int& t1, int& t2, int& t3) {
    int z1 = t0 + t3, z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = (z3 + z4) * JC_1_175;
    t0 *= JC_0_298; t1 *= JC_2_053; t2 *= JC_3_072; t3 *= JC_1_501;
    z1 *= -JC_0_899; z2 *= -JC_2_562;
    z3 = z3 * -JC_1_961 + z5;
    z4 = z4 * -JC_0_390 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
}

// one 8-point pass of jfdctint.c on d[0], d[S], .. d[7 S]; ROWS: the first (row) pass
template <bool ROWS, int S>
__device__ __forceinline__ void jc_fdct8(int* d) {
    const int t0 = d[0] + d[7 * S], t1 = d[S] + d[6 * S], t2 = d[2 * S] + d[5 * S], t3 = d[3 * S] + d[4 * S];
    int t7 = d[0] - d[7 * S], t6 = d[S] - d[6 * S], t5 = d[2 * S] - d[5 * S], t4 = d[3 * S] - d[4 * S];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int n = ROWS ? 11 : 15;
    d[0] = ROWS ? (t10 + t11) << 2 : jc_descale(t10 + t11, 2);
    d[4 * S] = ROWS ? (t10 - t11) << 2 : jc_descale(t10 - t11, 2);
    const int z1 = (t12 + t13) * JC_0_541;
    d[2 * S] = jc_descale(z1 + t13 * JC_0_765, n);
    d[6 * S] = jc_descale(z1 - t12 * JC_1_847, n);
    jc_odd(t4, t5, t6, t7);
    d[7 * S] = jc_descale(t4, n);
    d[5 * S] = jc_descale(t5, n);
    d[3 * S] = jc_descale(t6, n);
    d[S] = jc_descale(t7, n);
}

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
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint2 v = *reinterpret_cast<const uint2*>(p + r * pitch);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            d[r * 8 + j] = (int)((v.x >> (8 * j)) & 255u) - 128;
            d[r * 8 + 4 + j] = (int)((v.y >> (8 * j)) & 255u) - 128;
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) jc_fdct8<true, 1>(d + r * 8);
#pragma unroll
    for (int c = 0; c < 8; ++c) jc_fdct8<false, 8>(d + c);
    // q = sign(c) ((|c| + (8 t >> 1)) / (8 t)), then q t.  The quotient comes from the fp32 reciprocal and is put right by its remainder:
    // the numerator is below 2^17, so the fp32 estimate is off by one at the most.
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const int t = tab[i], dv = t << 3;
        const int n = abs(d[i]) + (dv >> 1);
        int q = (int)((float)n * rcp[i]);
        const int rem = n - q * dv;
        q += (rem >= dv ? 1 : 0) - (rem < 0 ? 1 : 0);
        d[i] = (d[i] < 0 ? -q : q) * t;
    }
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
        if (tid < 128) {   // jpeg_set_quality(q, force_baseline) of Annex K
            const int q = qual.q[img], s = q < 50 ? 5000 / q : 200 - 2 * q;
            const int t = min(max((JC_BASE[tid >> 6][tid & 63] * s + 50) / 100, 1), 255);
            tab[tid >> 6][tid & 63] = t;
            rcp[tid >> 6][tid & 63] = 1.0f / (float)(t << 3);
        }
        // 1. colour.  Quad (qy, qx) of tile + ring is the chroma sample (cy, cx) of the image's padded planes.  libjpeg replicates pixels on
        // the right at full resolution, at the bottom at full resolution up to an even row count only, and from there the DOWN-SAMPLED chroma
        // rows and the Y rows: chroma row cy >= CHr is row CHr - 1, Y row y >= H is row H - 1.
        for (int i = tid; i < JC_CH * JC_CW; i += JC_THREADS) {
            const int qy = i / JC_CW, qx = i - qy * JC_CW;
            const int my = my0 - 1 + (qy >> 3), mx = mx0 - 1 + (qx >> 3);
            if (my < 0 || my >= mcus_y || mx < 0 || mx >= mcus_x) continue;   // (no such MCU: its samples are never read)
            const int cy = my * 8 + (qy & 7), cx = mx * 8 + (qx & 7);
            const int cyc = min(cy, CHr - 1);
            const int r0 = min(2 * cyc, H - 1), r1 = min(2 * cyc + 1, H - 1), c0 = min(2 * cx, W - 1), c1 = min(2 * cx + 1, W - 1);
            int yv[2][2], cb = 0, cr = 0;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const long long o = (long long)(dy ? r1 : r0) * W + (dx ? c1 : c0);
                    const int r = jc_u8(inp[o]), g = jc_u8(inp[HW + o]), b = jc_u8(inp[2 * HW + o]);
                    yv[dy][dx] = (jc_fix16(.299) * r + jc_fix16(.587) * g + jc_fix16(.114) * b + 32768) >> 16;
                    cb += (-jc_fix16(.16874) * r - jc_fix16(.33126) * g + jc_fix16(.5) * b + (128 << 16) + 32767) >> 16;
                    cr += (jc_fix16(.5) * r - jc_fix16(.41869) * g - jc_fix16(.08131) * b + (128 << 16) + 32767) >> 16;
                }
            const int bias = 1 + (cx & 1);
            Cp[0][i] = (unsigned char)((cb + bias) >> 2);
            Cp[1][i] = (unsigned char)((cr + bias) >> 2);
            if (qy >= 8 && qy < JC_CH - 8 && qx >= 8 && qx < JC_CW - 8) {
                const bool below = cy > cyc;                  // Y rows past the image: the last row (r1) twice
                unsigned char* yp = Yp + (qy - 8) * 2 * JC_YP + (qx - 8) * 2;
                yp[0] = (unsigned char)(below ? yv[1][0] : yv[0][0]);
                yp[1] = (unsigned char)(below ? yv[1][1] : yv[0][1]);
                yp[JC_YP] = (unsigned char)yv[1][0];
                yp[JC_YP + 1] = (unsigned char)yv[1][1];
            }
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

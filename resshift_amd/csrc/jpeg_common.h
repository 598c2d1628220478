// libjpeg's forward path, ONCE, for jpeg_codec.hip (the round trip) and jpeg_encode.hip (the file): the quantisation tables of a quality, the
// colour conversion with the 2 x 2 chroma mean and its edge rules, the "islow" forward DCT and the quantiser (include/resshift_hip.h "face
// degradation").  All of it is 32-bit integer arithmetic, so "the encoder's coefficients are the codec's" holds by
// construction.  Included by those two files only.
#pragma once
#include "image_common.h"

constexpr int jc_fix16(double c) { return (int)(c * 65536 + .5); }
constexpr int jc_fix13(double c) { return (int)(c * 8192 + .5); }
constexpr int JC_0_298 = jc_fix13(0.298631336), JC_0_390 = jc_fix13(0.390180644), JC_0_541 = jc_fix13(0.541196100), JC_0_765 = jc_fix13(0.765366865),
              JC_0_899 = jc_fix13(0.899976223), JC_1_175 = jc_fix13(1.175875602), JC_1_501 = jc_fix13(1.501321110), JC_1_847 = jc_fix13(1.847759065),
              JC_1_961 = jc_fix13(1.961570560), JC_2_053 = jc_fix13(2.053119869), JC_2_562 = jc_fix13(2.562915447), JC_3_072 = jc_fix13(3.072711026);

// Annex K in natural order, [vertical frequency][horizontal]: luminance, chrominance
static __constant__ int JC_BASE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99},
};

struct JcQuality { int q[RS_MAX_ROWS]; };

// jpeg_set_quality(q, force_baseline) of Annex K: entry i (natural order) of table c (0 luminance, 1 chrominance)
__device__ __forceinline__ int jc_table_entry(int q, int c, int i) {
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    return min(max((JC_BASE[c][i] * s + 50) / 100, 1), 255);
}

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

// an 8 x 8 block of samples at p (pitch bytes per row, 8-byte aligned) -> its quantised coefficients d[8 u + v] (natural order): - 128, the
// forward DCT (rows, then columns), q = sign(c) ((|c| + (8 t >> 1)) / (8 t)).  The quotient comes from the fp32 reciprocal rcp[i] = 1 / (8 t)
// and is put right by its remainder: the numerator is below 2^17, so the fp32 estimate is off by one at the most.
__device__ __forceinline__ void jc_forward_block(const unsigned char* p, int pitch, const int* tab, const float* rcp, int* d) {
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
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        const int dv = tab[i] << 3;
        const int n = abs(d[i]) + (dv >> 1);
        int q = (int)((float)n * rcp[i]);
        const int rem = n - q * dv;
        q += (rem >= dv ? 1 : 0) - (rem < 0 ? 1 : 0);
        d[i] = d[i] < 0 ? -q : q;
    }
}

// by the first 128 threads of a workgroup: the two tables of quality q and the reciprocals of 8 t
__device__ __forceinline__ void jc_stage_tables(int q, int tid, int (*tab)[64], float (*rcp)[64]) {
    if (tid < 128) {
        const int t = jc_table_entry(q, tid >> 6, tid & 63);
        tab[tid >> 6][tid & 63] = t;
        rcp[tid >> 6][tid & 63] = 1.0f / (float)(t << 3);
    }
}

// The colour step of one chroma sample (cy, cx) of the image's padded planes, i.e. of the 2 x 2 pixel quad it is the mean of.  libjpeg
// replicates pixels on the right at full resolution, at the bottom at full resolution up to an even row count only, and from there the
// DOWN-SAMPLED chroma rows and the Y rows: chroma row cy >= CHr = ceil(H / 2) is row CHr - 1, Y row y >= H is row H - 1.  `px(o, r, g, b)`
// gives the 8-bit pixel at offset o = row * W + column.  y[dy][dx]: the quad's Y samples (rows past the image: the last row, see
// jc_quad_store_y); cb, cr: the down-sampled chroma, (a + b + c + d + bias) >> 2 with bias 1 on even columns and 2 on odd ones.
struct JcQuad { int y[2][2], cb, cr; bool below; };

template <class Px>
__device__ __forceinline__ JcQuad jc_quad(Px px, int cy, int cx, int H, int W) {
    const int cyc = min(cy, ((H + 1) >> 1) - 1);
    const int r0 = min(2 * cyc, H - 1), r1 = min(2 * cyc + 1, H - 1), c0 = min(2 * cx, W - 1), c1 = min(2 * cx + 1, W - 1);
    JcQuad qd;
    int cb = 0, cr = 0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            int r, g, b;
            px((long long)(dy ? r1 : r0) * W + (dx ? c1 : c0), r, g, b);
            qd.y[dy][dx] = (jc_fix16(.299) * r + jc_fix16(.587) * g + jc_fix16(.114) * b + 32768) >> 16;
            cb += (-jc_fix16(.16874) * r - jc_fix16(.33126) * g + jc_fix16(.5) * b + (128 << 16) + 32767) >> 16;
            cr += (jc_fix16(.5) * r - jc_fix16(.41869) * g - jc_fix16(.08131) * b + (128 << 16) + 32767) >> 16;
        }
    const int bias = 1 + (cx & 1);
    qd.cb = (cb + bias) >> 2;
    qd.cr = (cr + bias) >> 2;
    qd.below = cy > cyc;                                      // Y rows past the image: the last row (r1) twice
    return qd;
}

// the quad's four Y samples into a Y plane in LDS at yp (pitch bytes per row)
__device__ __forceinline__ void jc_quad_store_y(const JcQuad& qd, unsigned char* yp, int pitch) {
    yp[0] = (unsigned char)(qd.below ? qd.y[1][0] : qd.y[0][0]);
    yp[1] = (unsigned char)(qd.below ? qd.y[1][1] : qd.y[0][1]);
    yp[pitch] = (unsigned char)qd.y[1][0];
    yp[pitch + 1] = (unsigned char)qd.y[1][1];
}

// Antialiased bicubic resize to any output size: MATLAB's imresize (include/resshift_hip.h "antialiased resize").
//
// ONE launch, no intermediate tensor in HBM.  A workgroup of 256 threads owns a 16 x 64 tile of output rows x columns of one (image,
// channel) plane:
//   1. tables in LDS: `left` and the P normalised weights of every output row and column of the tile - coordinates in fp64 (one thread
//      per index), the distance rounded to fp32 once, the raw weight per (index, tap), the sum per index in tap order, the division per
//      (index, tap) - the P mirrored input rows of every tile row, and the mirrored input column of every column of the tile's span.
//   2. vertical pass, lanes along input columns: for every tile row and every input column j of the tile's span [left of its first
//      column, left of its last column + P) the P taps of column mirror(j) are read from global memory (consecutive lanes, consecutive
//      addresses except where the span is reflected) and accumulated in ascending order; the result goes to the LDS image mid[row][j].
//   3. horizontal pass, lanes along output columns: P taps of mid per output, ascending; a wave writes a whole 64-pixel row of the tile.
// Every value is a function of the plane and of the output index alone: the tables depend on the index only, both sums run in tap order,
// and a reflected span column is computed by the same expression as the column it mirrors.
//
// LDS image: the horizontal pass reads mid at a lane stride of 1/s dwords - 2, 4 and 8 at s = 1/2, 1/4, 1/8, which is a 2-, 4- and 8-way
// bank conflict of ds_read_b32 (32 banks per 32-lane group) on a linear row.  Column x is kept at x + x / 32 (one pad dword per 32): a
// stride of 2^q, q <= 3, then visits 32 different banks per group.  Measured on an MI355X (scripts/resize_bench.py): the
// linear image is 0.1 %, 0.3 % and 1.5 % slower at 1/2, 1/4 and 1/8 - the vertical pass dominates.  RS_RESIZE_LDS=linear selects the
// linear image for that measurement; the values are the same bits.
#include "image_common.h"
#include <cmath>

constexpr int RZ_TR = 16;
constexpr int RZ_TC = 64;
constexpr int RZ_THREADS = 256;
constexpr int RZ_PMAX = 34;                                   // ceil(4 / (1/8)) + 2
constexpr int RZ_SPAN = (RZ_TC - 1) * 8 + 1 + RZ_PMAX + 1;    // 540: most input columns under a tile (u moves by 63 / s <= 504)
constexpr int RZ_U = 6;                                       // taps of a pass whose loads are in flight together (P = 6 when s >= 1)
constexpr int RZ_PITCH = RZ_SPAN + RZ_SPAN / 32 + 1;          // 557 dwords per row of the padded image

struct RzAxis {
    double s;      // scale of the axis
    double kw;     // 4 / min(s, 1)
    float a;       // min(s, 1)
    int P;         // ceil(kw) + 2
    int n;         // input length
    int m;         // output length
};

// symmetric reflection of period 2n that repeats the edge sample, applied as often as needed; q is a 0-based index of any sign
__device__ __forceinline__ int rz_mirror(int q, int n) {
    const int p = 2 * n;
    int m = q % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// Keys' cubic with A = -0.5; exact at 0, 1 and 2
__device__ __forceinline__ float rz_cubic(float x) {
    const float ax = fabsf(x);
    if (ax <= 1.f) return (1.5f * ax - 2.5f) * ax * ax + 1.f;
    if (ax <= 2.f) return ((-0.5f * ax + 2.5f) * ax - 4.f) * ax + 2.f;
    return 0.f;
}

// u (fp64) and `left` (1-based index of tap 0) of output index i
__device__ __forceinline__ int rz_left(const RzAxis& ax, int i, double* u) {
    *u = (double)(i + 1) / ax.s + 0.5 * (1.0 - 1.0 / ax.s);
    return (int)floor(*u - ax.kw / 2);
}

// raw weight of the tap with the 1-based index j: the distance is formed in fp64 and rounded to fp32 once
__device__ __forceinline__ float rz_raw(const RzAxis& ax, double u, int j) {
    const float d = (float)(u - (double)j);
    return ax.a * rz_cubic(ax.a * d);
}

__global__ __launch_bounds__(RZ_THREADS) void resize_kernel(const float* __restrict__ in, float* __restrict__ out, RzAxis ah, RzAxis aw,
                                                            int tiles_x, int tiles_y, long long total, int clamp, int pad) {
    __shared__ float mid[RZ_TR * RZ_PITCH];
    __shared__ float wh[RZ_TR * RZ_PMAX];      // [row][tap]: a wave reads one row's weight at a time (broadcast)
    __shared__ int rowi[RZ_TR * RZ_PMAX];      // [row][tap]: mirrored input row
    __shared__ float ww[RZ_PMAX * RZ_TC];      // [tap][column]: lanes along columns read consecutive dwords
    __shared__ double uh[RZ_TR], uw[RZ_TC];
    __shared__ float sumh[RZ_TR], sumw[RZ_TC];
    __shared__ int lefth[RZ_TR], leftw[RZ_TC];
    __shared__ int coli[RZ_SPAN];              // mirrored input column of every span column
    const int H = ah.n, W = aw.n, Ho = ah.m, Wo = aw.m;
    const int Ph = ah.P, Pw = aw.P;
    const int tid = threadIdx.x;
    for (long long t = blockIdx.x; t < total; t += gridDim.x) {
        const int tx = (int)(t % tiles_x);
        const long long q = t / tiles_x;
        const int ty = (int)(q % tiles_y);
        const long long plane = q / tiles_y;
        const int oy0 = ty * RZ_TR, ox0 = tx * RZ_TC;
        const int nr = min(RZ_TR, Ho - oy0), nc = min(RZ_TC, Wo - ox0);
        const float* inp = in + plane * H * W;
        float* outp = out + plane * Ho * Wo;
        // 1. tables: u and left per index; raw weights (and the rows' mirrored input rows) per (index, tap); the sums per index, taps in
        //    ascending order; the division per (index, tap)
        if (tid < nr) lefth[tid] = rz_left(ah, oy0 + tid, &uh[tid]);
        else if (tid >= 64 && tid - 64 < nc) leftw[tid - 64] = rz_left(aw, ox0 + tid - 64, &uw[tid - 64]);   // (a wave of their own)
        __syncthreads();
        for (int i = tid; i < nr * Ph; i += RZ_THREADS) {
            const int r = i / Ph, k = i - r * Ph;
            wh[r * RZ_PMAX + k] = rz_raw(ah, uh[r], lefth[r] + k);
            rowi[r * RZ_PMAX + k] = rz_mirror(lefth[r] + k - 1, H);
        }
        for (int i = tid; i < Pw * RZ_TC; i += RZ_THREADS) {
            const int c = i % RZ_TC;
            if (c < nc) ww[i] = rz_raw(aw, uw[c], leftw[c] + i / RZ_TC);
        }
        // the span of 1-based input columns [j0, j0 + span) under the tile; `left` does not decrease with the index
        const int j0 = leftw[0];
        const int span = min(leftw[nc - 1] + Pw - j0, RZ_SPAN);
        for (int x = tid; x < span; x += RZ_THREADS) coli[x] = rz_mirror(j0 + x - 1, W);
        __syncthreads();
        if (tid < nr) {
            float sum = 0.f;
            for (int k = 0; k < Ph; ++k) sum += wh[tid * RZ_PMAX + k];
            sumh[tid] = sum;
        } else if (tid >= 64 && tid - 64 < nc) {
            float sum = 0.f;
            for (int k = 0; k < Pw; ++k) sum += ww[k * RZ_TC + tid - 64];
            sumw[tid - 64] = sum;
        }
        __syncthreads();
        for (int i = tid; i < nr * Ph; i += RZ_THREADS) {
            const int r = i / Ph, k = i - r * Ph;
            wh[r * RZ_PMAX + k] = wh[r * RZ_PMAX + k] / sumh[r];
        }
        for (int i = tid; i < Pw * RZ_TC; i += RZ_THREADS) {
            const int c = i % RZ_TC;
            if (c < nc) ww[i] = ww[i] / sumw[c];
        }
        __syncthreads();
        // 2. vertical pass over the span.  RZ_U taps per step: their loads are issued together (a tap past the last loads the last one
        //    again and adds nothing)
        const float inv_span = 1.0f / (float)span;
        for (int i = tid; i < nr * span; i += RZ_THREADS) {
            const int r = (int)(((float)i + 0.5f) * inv_span), x = i - r * span;   // (= i / span: i < 2^14, so the product is far from an integer)
            const float* col = inp + coli[x];
            const float* w = wh + r * RZ_PMAX;
            const int* ri = rowi + r * RZ_PMAX;
            float acc = 0.f;
            for (int k0 = 0; k0 < Ph; k0 += RZ_U) {
                float v[RZ_U];
#pragma unroll
                for (int u = 0; u < RZ_U; ++u) v[u] = col[(long long)ri[min(k0 + u, Ph - 1)] * W];
#pragma unroll
                for (int u = 0; u < RZ_U; ++u)
                    if (k0 + u < Ph) acc = fmaf(w[k0 + u], v[u], acc);
            }
            mid[r * RZ_PITCH + x + (pad ? x >> 5 : 0)] = acc;
        }
        __syncthreads();
        // 3. horizontal pass
        for (int i = tid; i < nr * RZ_TC; i += RZ_THREADS) {
            const int r = i / RZ_TC, c = i % RZ_TC;
            if (c >= nc) continue;
            const int x0 = min(leftw[c] - j0, span - Pw);   // (= leftw[c] - j0: the span was sized for it)
            const float* row = mid + r * RZ_PITCH;
            float acc = 0.f;
            for (int k0 = 0; k0 < Pw; k0 += RZ_U) {
                float v[RZ_U];
#pragma unroll
                for (int u = 0; u < RZ_U; ++u) {
                    const int x = x0 + min(k0 + u, Pw - 1);
                    v[u] = row[x + (pad ? x >> 5 : 0)];
                }
#pragma unroll
                for (int u = 0; u < RZ_U; ++u)
                    if (k0 + u < Pw) acc = fmaf(ww[(k0 + u) * RZ_TC + c], v[u], acc);
            }
            if (clamp) acc = fminf(fmaxf(acc, -1.0f), 1.0f);
            outp[(long long)(oy0 + r) * Wo + ox0 + c] = acc;
        }
        __syncthreads();   // (the next tile of this workgroup overwrites the tables and mid)
    }
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------
extern "C" {

static RzAxis rz_axis(double s, int n, int m) {
    RzAxis ax;
    const double a = std::min(s, 1.0);
    ax.s = s;
    ax.kw = 4.0 / a;
    ax.a = (float)a;
    ax.P = (int)std::ceil(ax.kw) + 2;
    ax.n = n;
    ax.m = m;
    return ax;
}

int rs_resize(const float* in, float* out, int B, int C, int H, int W, int Ho, int Wo, double scale_h, double scale_w, int clamp,
              void* stream) {
    const std::string who = "rs_resize: ";
    if (!in || !out) return img_fail(who, "null tensor (in / out)");
    if (B < 1 || C < 1 || H < 1 || W < 1 || Ho < 1 || Wo < 1) return img_fail(who, "B, C, H, W, Ho and Wo must be positive");
    if (!(scale_h >= 0.125 && scale_h <= 8.0) || !(scale_w >= 0.125 && scale_w <= 8.0))
        return img_fail(who, "scale_h and scale_w must lie in [1/8, 8] (the kernel holds at most 34 taps per axis)");
    if (!img_is_flag(clamp)) return img_fail(who, "clamp must be 0 or 1");
    if (!img_plane_fits(H, W) || !img_plane_fits(Ho, Wo)) return img_fail(who, "a plane is too large (a side above 2^28 or more than 2^40 pixels)");
    const long long planes = (long long)B * C;
    if (img_overlaps(in, planes * H * W * sizeof(float), out, planes * Ho * Wo * sizeof(float)))
        return img_fail(who, "`out` overlaps `in` (workgroups read their neighbours' pixels of in: not in place)");
    const RzAxis ah = rz_axis(scale_h, H, Ho), aw = rz_axis(scale_w, W, Wo);
    if (ah.P > RZ_PMAX || aw.P > RZ_PMAX) return img_fail(who, "more than 34 taps per axis");
    const int pad = !rs_env_is("RS_RESIZE_LDS", "linear");   // A/B knob of scripts/resize_bench.py, read per call
    const int tiles_x = (Wo + RZ_TC - 1) / RZ_TC, tiles_y = (Ho + RZ_TR - 1) / RZ_TR;
    const long long total = planes * tiles_x * tiles_y;
    hipLaunchKernelGGL(resize_kernel, dim3((unsigned)std::min<long long>(total, 1 << 20)), dim3(RZ_THREADS), 0, (hipStream_t)stream, in, out, ah,
                       aw, tiles_x, tiles_y, total, clamp, pad);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}   // extern "C"

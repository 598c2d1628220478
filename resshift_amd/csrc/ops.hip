// Op-level test entry points and benchmark helpers (resshift_amd/ops.py, the GPU tests): one kernel family per call, operands packed by
// weight_pack.h - the same functions the model packer uses.  Part of the production library; errors go through rs_set_last_error.
#include "launchers.h"
#include "weight_pack.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" {

// -------------------------------------------------------------------- op-level test entry points
static void* dev_copy(const void* host, size_t bytes) {
    void* d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) return nullptr;
    (void)hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
    return d;
}
// fragment-major copy (weight_pack.h) of a row-major DEVICE operand: rows of `ld` halfs, lo plane at +lo_off halfs (< 0: fp16 only) -> device copy
// (the operand is the caller's, possibly still being written on the caller's stream `st`: the read-back waits for that stream first)
static void* frag_major_from_device_rows(const void* wdev, int N, int K, int ld, int lo_off, hipStream_t st) {
    std::vector<f16> rows((size_t)N * ld), out((size_t)N * K * (lo_off >= 0 ? 2 : 1));
    if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(rows.data(), wdev, rows.size() * sizeof(f16), hipMemcpyDeviceToHost) != hipSuccess) return nullptr;
    frag_major_fill(N, K, out.data(), lo_off >= 0, [&](int n, int k) { return rows[(size_t)n * ld + k]; },
                    [&](int n, int k) { return rows[(size_t)n * ld + (lo_off >= 0 ? lo_off : 0) + k]; });
    return dev_copy(out.data(), out.size() * sizeof(f16));
}
// device copy of the row form [Cout][taps * Cin] of a reference weight in the storage type `prec` (no channel padding: CinP = Cin)
static void* pack_rows_dev(const float* w_ref_host, int Cout, int Cin, int taps, int prec) {
    std::vector<char> o((size_t)Cout * taps * Cin * rs_dtype_size(prec));
    if (prec == RS_F16) rs_pack_rows_f16(w_ref_host, Cout, Cin, taps, Cin, (f16*)o.data());
    else if (prec == RS_F16S) rs_pack_rows_split(w_ref_host, Cout, Cin, taps, Cin, (f16*)o.data());
    else rs_pack_rows_f32(w_ref_host, Cout, Cin, taps, Cin, (float*)o.data());
    return dev_copy(o.data(), o.size());
}
// device copies of a Swin block's relative position bias (weight_pack.h): [h][j][i], [h][i][j] and the compact form; null: not wanted
static void bias_tables_dev(const float* table_host, int heads, float** bias_t, float** bias_n, float** bias_c) {
    std::vector<float> bt(bias_t ? (size_t)heads * 4096 : 0), bn(bias_n ? (size_t)heads * 4096 : 0), bc(bias_c ? (size_t)heads * 256 : 0);
    rs_pack_bias_tables(table_host, heads, bias_t ? bt.data() : nullptr, bias_n ? bn.data() : nullptr);
    if (bias_c) rs_pack_bias_compact(table_host, heads, bc.data());
    if (bias_t) *bias_t = (float*)dev_copy(bt.data(), bt.size() * 4);
    if (bias_n) *bias_n = (float*)dev_copy(bn.data(), bn.size() * 4);
    if (bias_c) *bias_c = (float*)dev_copy(bc.data(), bc.size() * 4);
}

// `reps` launches of a planned conv between two hipEvents: *ms_out = their average milliseconds
static int time_launches(const IGemmParams& p, int in_prec, int out_prec, const ConvPlan& pl, int reps, hipStream_t st, float* ms_out) {
    int rc = 0;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, st);
    for (int i = 0; i < reps; ++i) rc |= rs_conv_launch(&p, in_prec, out_prec, 1, &pl, st);
    (void)hipEventRecord(e1, st);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    if (ms_out) *ms_out = ms / (float)std::max(1, reps);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return rc;
}

// The op-level conv entries: plan the launch (rs_conv_plan), give it its split-K slab, launch it once and - `timed` - `reps` more times
// between two hipEvents (*ms_out = their average milliseconds), free the slab.  `halo_only`: fail unless the plan is the halo kernel's.
static int op_conv_run(IGemmParams p, int in_prec, int out_prec, hipStream_t st, bool halo_only = false, bool timed = false, int reps = 0, float* ms_out = nullptr,
                       ConvPlan* executed = nullptr) {
    ConvPlan pl{};
    (void)rs_conv_plan(&p, in_prec, out_prec, 1, &pl);
    if (halo_only && pl.kernel != CK_HALO && pl.kernel != CK_HALO_SEG) return rs_set_last_error("shape is not eligible for the halo kernel", -1);
    float* part = nullptr;
    if (pl.splitk > 1) { (void)hipMalloc((void**)&part, (size_t)pl.splitk * p.M * p.Cout * sizeof(float)); p.partial = part; }
    int rc = rs_conv_launch(&p, in_prec, out_prec, 1, &pl, st);
    if (executed) *executed = pl;   // the plan rs_conv_launch was handed, not a second answer of the planner
    if (rc) { if (rc != RS_ERR_OPERAND_BYTES) rs_set_last_error("igemm launch rejected the shape", -1); }   // (an oversize operand keeps the launcher's text)
    else if (timed) rc = time_launches(p, in_prec, out_prec, pl, reps, st, ms_out);
    (void)hipStreamSynchronize(st);
    if (part) (void)hipFree(part);
    return rc;
}

// The IGemmParams of a conv layer as the op-level entries describe it (rs_op_conv2d_ex and rs_op_conv_plan fill it here, nowhere else):
// ld0 / ld1 / ldy / ldres are the row strides in elements of the buffers the sources, y and the residual are views into
static IGemmParams op_conv_params(const void* x0, const void* x1, const void* wdev, const float* bias, const void* res, void* y, int B, int Hs, int Ws,
                                  int C0, int C1, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo, int up, int act, int ld0,
                                  int ld1, int ldy, int ldres) {
    IGemmParams p{};
    p.x0 = x0; p.x1 = x1; p.w = wdev; p.bias = bias; p.res = res; p.y = y; p.C0 = C0; p.C1 = C1; p.ld0 = ld0; p.ld1 = ld1;
    p.B = B; p.Hs = Hs; p.Ws = Ws; p.up = up; p.Ho = Ho; p.Wo = Wo; p.KH = KH; p.KW = KW; p.stride = stride; p.pad_t = pad_t; p.pad_l = pad_l;
    p.Cout = Cout; p.ldy = ldy; p.ldres = ldres; p.M = B * Ho * Wo; p.Ktot = KH * KW * (C0 + C1); p.act = act; p.out_scale = 1.f;
    return p;
}
// the layers rs_op_conv2d hands to the direct kernels: these never reach rs_conv_plan
static bool op_conv_is_direct(int C0, int C1, int Cout) { return ((C0 + C1) % 8 != 0) || (C0 % 8 != 0) || Cout <= 8; }
static void plan_to_ints(const ConvPlan& pl, int out[6]) {
    out[0] = pl.kernel; out[1] = pl.BP; out[2] = pl.BC; out[3] = pl.SEG; out[4] = pl.splitk; out[5] = pl.stats_px;
}

int rs_op_conv_plan(int B, int Hs, int Ws, int C0, int C1, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo, int up, int act,
                    int in_prec, int out_prec, int ld0, int ld1, int ldy, int ldres, int has_res, int nz, int out[6]) {
    static const char some_residual = 0;   // the planner asks only whether there is one
    for (int i = 0; i < 6; ++i) out[i] = 0;
    if (op_conv_is_direct(C0, C1, Cout)) return 0;
    const IGemmParams p = op_conv_params(nullptr, nullptr, nullptr, nullptr, has_res ? &some_residual : nullptr, nullptr, B, Hs, Ws, C0, C1, Cout, KH, KW,
                                         stride, pad_t, pad_l, Ho, Wo, up, act, ld0, ld1, ldy, ldres);
    ConvPlan pl{};
    const int rc = rs_conv_plan(&p, in_prec, out_prec, nz, &pl);
    plan_to_ints(pl, out);
    return rc;
}

int rs_op_conv2d_ex(const void* x0, const void* x1, const float* w_ref_host, const float* bias_host, const void* res, void* y, int B, int Hs,
                    int Ws, int C0, int C1, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo, int up, int act,
                    int in_prec, int out_prec, int force_direct, int ld0, int ld1, int ldy, int ldres, int plan_out[6], void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int Cin = C0 + C1;
    const size_t K = (size_t)KH * KW * Cin, n = K * Cout;
    const bool direct = force_direct || op_conv_is_direct(C0, C1, Cout);
    float* bias = bias_host ? (float*)dev_copy(bias_host, Cout * 4) : nullptr;
    int rc;
    void* wdev = nullptr;
    ConvPlan executed{};
    if (direct) {
        std::vector<float> o(n);
        rs_pack_tap_major(w_ref_host, Cout, Cin, KH * KW, o.data());
        wdev = dev_copy(o.data(), n * 4);
        DirectConvParams p{};
        p.x0 = x0; p.x1 = x1; p.w = (const float*)wdev; p.bias = bias; p.y = y; p.C0 = C0; p.C1 = C1; p.ld0 = ld0; p.ld1 = ld1;
        p.B = B; p.Hs = Hs; p.Ws = Ws; p.up = up; p.Ho = Ho; p.Wo = Wo; p.KH = KH; p.KW = KW; p.stride = stride; p.pad_t = pad_t; p.pad_l = pad_l;
        p.Cout = Cout; p.ldy = ldy; p.act = act;
        if (res) { rc = rs_set_last_error("direct conv has no residual path", -1); }
        else rc = rs_direct_conv_launch(&p, in_prec, out_prec, st);
    } else {
        wdev = pack_rows_dev(w_ref_host, Cout, Cin, KH * KW, in_prec);
        const IGemmParams p = op_conv_params(x0, x1, wdev, bias, res, y, B, Hs, Ws, C0, C1, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo, up, act, ld0, ld1,
                                             ldy, ldres);
        rc = op_conv_run(p, in_prec, out_prec, st, false, false, 0, nullptr, &executed);
    }
    if (plan_out) plan_to_ints(executed, plan_out);
    (void)hipStreamSynchronize(st);
    if (wdev) (void)hipFree(wdev);
    if (bias) (void)hipFree(bias);
    return rc;
}

int rs_op_conv2d(const void* x0, const void* x1, const float* w_ref_host, const float* bias_host, const void* res, void* y, int B, int Hs,
                 int Ws, int C0, int C1, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int Ho, int Wo, int up, int act,
                 int in_prec, int out_prec, int force_direct, void* stream) {
    return rs_op_conv2d_ex(x0, x1, w_ref_host, bias_host, res, y, B, Hs, Ws, C0, C1, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo, up, act, in_prec,
                           out_prec, force_direct, C0, C1, Cout, Cout, nullptr, stream);
}

// micro-benchmark of one implicit-GEMM conv shape (random device data is supplied by the caller): `reps` launches
// bracketed by hipEvents on the stream; returns the average milliseconds per launch in *ms_out.
int rs_op_conv2d_bench(const void* x0, const void* w_packed_dev, const float* bias_dev, const void* res, void* y, int B, int Hs, int Ws,
                       int Cin, int Cout, int KH, int KW, int stride, int pad, int Ho, int Wo, int up, int act, int in_prec, int out_prec,
                       int reps, float* ms_out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    IGemmParams p{};
    p.x0 = x0; p.w = w_packed_dev; p.bias = bias_dev; p.res = res; p.y = y; p.C0 = Cin; p.ld0 = Cin;
    p.B = B; p.Hs = Hs; p.Ws = Ws; p.up = up; p.Ho = Ho; p.Wo = Wo; p.KH = KH; p.KW = KW; p.stride = stride; p.pad_t = pad; p.pad_l = pad;
    p.Cout = Cout; p.ldy = Cout; p.ldres = Cout; p.M = B * Ho * Wo; p.Ktot = KH * KW * Cin; p.act = act; p.out_scale = 1.f;
    return op_conv_run(p, in_prec, out_prec, st, false, true, reps, ms_out);
}

// GroupNorm-affine + SiLU + 3x3 conv on the halo kernel (igemm4.hip): x raw fp16 NHWC, coef_dev [B][2][Cin] fp32 (scale row,
// shift row) or null, weights in the reference layout on the host; fails when the shape is not eligible for that kernel
int rs_op_conv3x3_halo(const void* x, const float* coef_dev, int act_in, const float* w_ref_host, const float* bias_host, const void* res, void* y,
                       int B, int H, int W, int Cin, int Cout, int prec, float* ystats_dev, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const size_t K = (size_t)9 * Cin;
    if (prec != RS_F16 && prec != RS_F16S) return rs_set_last_error("halo kernel: fp16 or split storage", -1);
    void* wdev = pack_rows_dev(w_ref_host, Cout, Cin, 9, prec);
    float* bias = bias_host ? (float*)dev_copy(bias_host, Cout * 4) : nullptr;
    IGemmParams p{};
    p.x0 = x; p.w = wdev; p.bias = bias; p.res = res; p.y = y; p.C0 = Cin; p.ld0 = Cin; p.B = B; p.Hs = H; p.Ws = W; p.up = 1; p.Ho = H; p.Wo = W;
    p.KH = 3; p.KW = 3; p.stride = 1; p.pad_t = 1; p.pad_l = 1; p.Cout = Cout; p.ldy = Cout; p.ldres = Cout; p.M = B * H * W; p.Ktot = (int)K;
    p.out_scale = 1.f; p.splitk = 1; p.xcoef = coef_dev; p.xact = act_in;
    p.ystats = ystats_dev; p.ystats_ld = Cout;
    const int rc = op_conv_run(p, prec, prec, st, true);
    if (wdev) (void)hipFree(wdev);
    if (bias) (void)hipFree(bias);
    return rc;
}

// The same layer on the Winograd F(2x2,3x3) kernel (wino.hip; split storage only): weights transformed and packed on the host, one checked
// launch; with reps > 0 the launch is then repeated `reps` times between two hipEvents and *ms_out receives the average milliseconds.
// `ystats_dev`: [B][H*W / 128][Cout][2] (one slab per 8 x 16 pixel tile).  Fails when the shape is not eligible.
int rs_op_conv3x3_wino(const void* x, const float* coef_dev, int act_in, const float* w_ref_host, const float* bias_host, const void* res, void* y,
                       int B, int H, int W, int Cin, int Cout, float* ystats_dev, int reps, float* ms_out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (Cin < 32 || (Cin % 32) || Cout < 32 || (Cout % 32)) return rs_set_last_error("wino kernel: channels in multiples of 32", -1);
    std::vector<char> packed(rs_wino_weight_bytes(Cin, Cout));
    const float mx = rs_wino_pack(w_ref_host, Cin, Cout, packed.data());
    if (!(mx < 30.0f)) return rs_set_last_error("wino kernel: |U| >= 30", -1);
    void* wdev = dev_copy(packed.data(), packed.size());
    float* bias = bias_host ? (float*)dev_copy(bias_host, Cout * 4) : nullptr;
    IGemmParams p{};
    p.x0 = x; p.ww = wdev; p.bias = bias; p.res = res; p.y = y; p.C0 = Cin; p.ld0 = Cin; p.B = B; p.Hs = H; p.Ws = W; p.up = 1; p.Ho = H; p.Wo = W;
    p.KH = 3; p.KW = 3; p.stride = 1; p.pad_t = 1; p.pad_l = 1; p.Cout = Cout; p.ldy = Cout; p.ldres = Cout; p.M = B * H * W; p.Ktot = 9 * Cin;
    p.out_scale = 1.f; p.splitk = 1; p.xcoef = coef_dev; p.xact = act_in; p.ystats = ystats_dev; p.ystats_ld = Cout;
    int rc = 0;
    float* stamps = nullptr;   // RS_WINO_STAMPS=1 with a -DRS_WINO_PHASES build: per-workgroup phase cycles of wave 0 (see wino.hip), averaged to stderr
    const int ntile = rs_wino_tiles(&p);
    p.dbg = 64;   // (an op-level entry: no fill-the-chip threshold)
    p.dbg |= (int)rs_env_int("RS_WINO_ABL", 0);   // (-DRS_WINO_PHASES builds: timing ablations, wino.hip)
    if (rs_env_set("RS_WINO_STAMPS")) { (void)hipMalloc((void**)&stamps, (size_t)ntile * 16 * sizeof(float)); (void)hipMemsetAsync(stamps, 0, (size_t)ntile * 16 * sizeof(float), st); p.partial = stamps; }
    ConvPlan pl{};
    (void)rs_conv_plan(&p, RS_F16S, RS_F16S, 1, &pl);
    if (pl.kernel != CK_WINO) rc = rs_set_last_error("shape is not eligible for the wino kernel", -1);
    else {
        rc = rs_conv_launch(&p, RS_F16S, RS_F16S, 1, &pl, st);
        if (rc && rc != RS_ERR_OPERAND_BYTES) rs_set_last_error("wino launch failed", -1);
        if (stamps) {
            (void)hipStreamSynchronize(st);
            std::vector<float> hs((size_t)ntile * 16);
            (void)hipMemcpy(hs.data(), stamps, hs.size() * sizeof(float), hipMemcpyDeviceToHost);
            double wide[16] = {}; int nw = 0;
            for (int t = 0; t < ntile; ++t) {
                for (int i = 0; i < 16; ++i) wide[i] += hs[(size_t)t * 16 + i];
                ++nw;
            }
            static const char* nm[8] = {"prologue", "wait+barrier", "halo issue", "B operand", "MFMA steps", "conversion", "epilogue", "total"};
            fprintf(stderr, "[wino phases] %dx%dx%d %d->%d, mean cycles of wave 0 over %d workgroups:", B, H, W, Cin, Cout, nw);
            for (int i = 0; i < 8; ++i) fprintf(stderr, " %s %.0f", nm[i], wide[i] / std::max(1, nw));
            static const char* nq[6] = {"drain", "barrier-1", "exchange writes", "barrier-2", "transform + stores", "statistics"};
            fprintf(stderr, "  | epilogue:");
            for (int i = 0; i < 6; ++i) fprintf(stderr, " %s %.0f", nq[i], wide[8 + i] / std::max(1, nw));
            fprintf(stderr, "\n");
        }
        if (!rc && reps > 0) rc = time_launches(p, RS_F16S, RS_F16S, pl, reps, st, ms_out);
    }
    (void)hipStreamSynchronize(st);
    if (stamps) (void)hipFree(stamps);
    if (wdev) (void)hipFree(wdev);
    if (bias) (void)hipFree(bias);
    return rc;
}

// pixels per statistics slab that rs_op_conv3x3_halo would use for this shape (0: not eligible / no statistics): the caller sizes ystats_dev
// as [B][H*W / slab][Cout][2]
int rs_op_conv3x3_halo_stats_px(int B, int H, int W, int Cin, int Cout, int prec) {
    IGemmParams p{};
    p.C0 = Cin; p.ld0 = Cin; p.B = B; p.Hs = H; p.Ws = W; p.up = 1; p.Ho = H; p.Wo = W;
    p.KH = 3; p.KW = 3; p.stride = 1; p.pad_t = 1; p.pad_l = 1; p.Cout = Cout; p.ldy = Cout; p.ldres = Cout; p.M = B * H * W; p.Ktot = 9 * Cin;
    ConvPlan pl{};
    (void)rs_conv_plan(&p, prec, prec, 1, &pl);
    return (pl.kernel == CK_HALO || pl.kernel == CK_HALO_SEG) ? pl.stats_px : 0;
}

int rs_op_gemm_nt(const void* a, const void* b, const float* bias_dev, void* y, int nz, int M, int N, int K, float scale, int in_prec,
                  int out_prec, void* stream) {
    IGemmParams p{};
    p.x0 = a; p.w = b; p.bias = bias_dev; p.y = y; p.C0 = K; p.ld0 = K; p.B = 1; p.Hs = M; p.Ws = 1; p.up = 1; p.Ho = M; p.Wo = 1;
    p.KH = 1; p.KW = 1; p.stride = 1; p.Cout = N; p.ldy = N; p.M = M; p.Ktot = K; p.out_scale = scale;
    p.bs_x0 = (long long)M * K; p.bs_w = (long long)N * K; p.bs_y = (long long)M * N;
    ConvPlan pl{};
    (void)rs_conv_plan(&p, in_prec, out_prec, nz, &pl);
    const int rc = rs_conv_launch(&p, in_prec, out_prec, nz, &pl, (hipStream_t)stream);
    if (rc && rc != RS_ERR_OPERAND_BYTES) rs_set_last_error("igemm launch rejected the shape", -1);   // (an oversize operand keeps the launcher's text)
    return rc;
}

int rs_op_groupnorm(const void* x, void* y, const float* gamma_host, const float* beta_host, const float* film_dev, int B, int HW, int C,
                    int groups, float eps, int act, int prec, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    float* g = (float*)dev_copy(gamma_host, C * 4);
    float* bt = (float*)dev_copy(beta_host, C * 4);
    int S = std::max(1, std::min(64, 1024 / std::max(1, B)));
    S = std::max(1, std::min(S, HW / 8));
    const int S2 = std::max(1, std::min(HW / 8, std::max(1, 2048 / std::max(1, B))));
    float* partial = nullptr;
    (void)hipMalloc((void**)&partial, (size_t)B * S * groups * 2 * 4);
    GNParams p{};
    p.x = x; p.y = y; p.gamma = g; p.beta = bt; p.film = film_dev; p.partial = partial; p.B = B; p.HW = HW; p.C = C; p.ldx = C; p.ldy = C;
    p.S = S; p.groups = groups; p.eps = eps; p.act = act;
    const int nk = rs_groupnorm_launch(&p, prec, S2, st);   // kernels launched, or < 0
    const int rc = nk < 0 ? nk : 0;
    if (rc) rs_set_last_error("groupnorm launch rejected the shape", -1);
    (void)hipStreamSynchronize(st);
    (void)hipFree(g); (void)hipFree(bt); (void)hipFree(partial);
    return rc;
}

int rs_op_window_attention(const void* qkv, void* out, const float* table_host, int B, int H, int W, int heads, int shift, int prec,
                           void* stream) {
    hipStream_t st = (hipStream_t)stream;
    float *d = nullptr, *dn = nullptr;
    bias_tables_dev(table_host, heads, &d, &dn, nullptr);
    WinAttnParams p{};
    p.bias_n = dn;
    p.qkv = qkv; p.out = out; p.bias_t = d; p.B = B; p.H = H; p.W = W; p.heads = heads; p.shift = shift; p.ldq = 3 * heads * 32;
    p.ldo = heads * 32; p.scale = 1.0f / std::sqrt(32.0f);
    const int rc = rs_win_attn_launch(&p, prec, st);
    if (rc) rs_set_last_error("window attention launch rejected the shape", -1);
    (void)hipStreamSynchronize(st);
    (void)hipFree(d);
    (void)hipFree(dn);
    return rc;
}

// the fused qkv + window attention (+ projection) kernels, fp16 (`split` false) or split storage: the bias tables from the host table, the
// caller's row-major weights (split: rows [K hi | K lo]) repacked in fragment-major order (ConvW::wh_frag / ws_frag)
static int op_window_attention_qkv(bool split, const void* x, const void* wqkv_dev, const float* bqkv_dev, const void* wproj_dev, const float* bproj_dev,
                                   const void* res, void* out, const float* table_host, const float* xcoef_dev, int B, int H, int W, int heads, int shift,
                                   hipStream_t st) {
    float *dn = nullptr, *dc = nullptr;
    bias_tables_dev(table_host, heads, nullptr, &dn, &dc);
    WinAttnParams p{};
    p.bias_n = dn; p.bias_c = dc; p.out = out; p.B = B; p.H = H; p.W = W; p.heads = heads; p.shift = shift; p.ldo = heads * 32; p.scale = 1.0f / std::sqrt(32.0f);
    const int E = heads * 32, ld = split ? 2 * E : E, lo_off = split ? E : -1;
    void* wq_f = frag_major_from_device_rows(wqkv_dev, 3 * E, E, ld, lo_off, st);
    void* wp_f = wproj_dev ? frag_major_from_device_rows(wproj_dev, E, E, ld, lo_off, st) : nullptr;
    p.x = x; p.wqkv = wq_f; p.bqkv = bqkv_dev; p.ldx = heads * 32; p.xcoef = xcoef_dev;
    p.wproj = wp_f; p.bproj = bproj_dev; p.res = res; p.ldres = heads * 32;
    const int rc = !(wq_f && (wp_f || !wproj_dev)) ? -1 : (split ? rs_win_attn_qkv_split_launch(&p, st) : rs_win_attn_qkv_launch(&p, st));
    if (rc && rc != RS_ERR_OPERAND_BYTES) rs_set_last_error(split ? "fused split qkv + window attention launch rejected the shape (split storage, 6 heads of 32 only)"
                                    : "fused qkv + window attention launch rejected the shape (fp16, 6 heads of 32 only)", -1);
    (void)hipStreamSynchronize(st);
    (void)hipFree(dn); (void)hipFree(dc); (void)hipFree(wq_f); (void)hipFree(wp_f);
    return rc;
}
int rs_op_window_attention_qkv(const void* x, const void* wqkv_dev, const float* bqkv_dev, const void* wproj_dev, const float* bproj_dev,
                               const void* res, void* out, const float* table_host, int B, int H, int W, int heads, int shift, void* stream) {
    return op_window_attention_qkv(false, x, wqkv_dev, bqkv_dev, wproj_dev, bproj_dev, res, out, table_host, nullptr, B, H, W, heads, shift, (hipStream_t)stream);
}
int rs_op_window_attention_qkv_split(const void* x, const void* wqkv_dev, const float* bqkv_dev, const void* wproj_dev, const float* bproj_dev,
                                     const void* res, void* out, const float* table_host, const float* xcoef_dev, int B, int H, int W, int heads,
                                     int shift, void* stream) {
    return op_window_attention_qkv(true, x, wqkv_dev, bqkv_dev, wproj_dev, bproj_dev, res, out, table_host, xcoef_dev, B, H, W, heads, shift, (hipStream_t)stream);
}

// the dense call block of the op-level attention entries: rows of C features
static AeFlashCall op_ae_flash_call(const void* q, const void* k, const void* vt, const float* bv_dev, void* o, int nz, int T, int C) {
    AeFlashCall c{};
    c.q = q; c.k = k; c.vt = vt; c.bv = bv_dev; c.o = o; c.ldq = c.ldk = c.ldo = C; c.nz = nz; c.T = T; c.C = C; c.scale = 1.0f / std::sqrt((float)C);
    return c;
}
int rs_op_ae_flash_attention(const void* q, const void* k, const void* vt, const float* bv_dev, void* o, int nz, int T, int C, void* stream) {
    const AeFlashCall c = op_ae_flash_call(q, k, vt, bv_dev, o, nz, T, C);
    const int rc = rs_ae_flash_launch(&c, (hipStream_t)stream);
    if (rc) rs_set_last_error("streaming AE attention launch rejected the shape (fp16, C in {128, 256, 512}, T a multiple of 128)", -1);
    return rc;
}

int rs_op_ae_flash_attention_split(const void* q, const void* k, const void* vt, const float* bv_dev, void* o, int nz, int T, int C, void* stream) {
    const AeFlashCall c = op_ae_flash_call(q, k, vt, bv_dev, o, nz, T, C);
    const int rc = rs_ae_flash_split_launch(&c, (hipStream_t)stream);
    if (rc) rs_set_last_error("split-storage streaming AE attention launch rejected the shape (C = 512, T a multiple of 64)", -1);
    return rc;
}

// the dense call block of the op-level MLP entries: rows of E features in, NO (0: E) out, no shortcut yet
static SwinMlpCall op_swin_mlp_call(const void* x, const void* w1_dev, const float* b1_dev, const void* w2_dev, const float* b2_dev, void* y, int M, int E) {
    SwinMlpCall c{};
    c.x = x; c.w1 = w1_dev; c.b1 = b1_dev; c.w2 = w2_dev; c.b2 = b2_dev; c.y = y; c.M = M; c.ldx = c.ldy = c.E = E;
    return c;
}
int rs_op_swin_mlp(const void* x, const void* w1_dev, const float* b1_dev, const void* w2_dev, const float* b2_dev, const void* res, void* y,
                   int M, int E, int HD, void* stream) {
    SwinMlpCall c = op_swin_mlp_call(x, w1_dev, b1_dev, w2_dev, b2_dev, y, M, E);
    c.HD = HD; c.res = res; c.ldres = E;
    const int rc = rs_swin_mlp_launch(&c, (hipStream_t)stream);
    if (rc) rs_set_last_error("swin_mlp launch rejected the shape (fp16, E = 192, HD = 768 only)", -1);
    return rc;
}
int rs_op_swin_mlp_split(const void* x, const void* w1_dev, const float* b1_dev, const void* w2_dev, const float* b2_dev, const void* res, void* y,
                         int M, int E, int HD, void* stream) {
    SwinMlpCall c = op_swin_mlp_call(x, w1_dev, b1_dev, w2_dev, b2_dev, y, M, E);
    c.HD = HD; c.res = res; c.ldres = E;
    const int rc = rs_swin_mlp_split_launch(&c, (hipStream_t)stream);
    if (rc) rs_set_last_error("swin_mlp_split launch rejected the shape (split storage, E = 192, HD = 768 only)", -1);
    return rc;
}
int rs_op_swin_mlp_split_unembed(const void* x, const float* xcoef_dev, const void* w1_dev, const float* b1_dev, const void* w2cat_dev, const float* bcat_dev,
                                 void* y, int M, int HW, int E, int HD, int NO, void* stream) {
    SwinMlpCall c = op_swin_mlp_call(x, w1_dev, b1_dev, w2cat_dev, bcat_dev, y, M, E);
    c.HD = HD; c.NO = c.ldy = NO; c.xcoef = xcoef_dev; c.HW = HW;
    const int rc = rs_swin_mlp_split_launch(&c, (hipStream_t)stream);
    if (rc) rs_set_last_error("swin_mlp_split (+ patch_unembed) launch rejected the shape (split storage, E = 192, HD = 768, NO = 160, HW % 128 == 0 only)", -1);
    return rc;
}
int rs_op_softmax_rows(const float* s, void* out, long long nrows, int ncols, int out_prec, void* stream) {
    return rs_softmax_rows_launch(s, out, out_prec, nrows, ncols, ncols, ncols, (hipStream_t)stream);
}
int rs_op_vq(const float* z, const float* codebook_dev, float* zq, int32_t* idx, long long N, int NE, int D, void* stream) {
    return rs_vq_launch(z, codebook_dev, zq, idx, N, NE, D, (hipStream_t)stream);
}
int rs_op_nchw_to_nhwc(const float* in, void* out, int B, int C, int HW, int out_prec, void* stream) {
    return rs_nchw_to_nhwc_launch(in, out, out_prec, B, C, HW, C, 0, 1.f, (hipStream_t)stream);
}
int rs_op_nhwc_to_nchw(const void* in, float* out, int B, int C, int HW, int in_prec, void* stream) {
    return rs_nhwc_to_nchw_launch(in, in_prec, out, B, C, HW, C, 0, (hipStream_t)stream);
}
int rs_op_convert(const void* src, int src_prec, void* dst, int dst_prec, int C, long long npix, void* stream) {
    return rs_convert_launch(src, src_prec, dst, dst_prec, C, npix, (hipStream_t)stream);
}

}  // extern "C"

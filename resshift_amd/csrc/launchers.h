// Every host entry point that one .hip file defines and another calls, declared once.  The defining file includes this header too: with C
// linkage a definition that disagrees with its declaration does not compile.
#pragma once
#include "common.h"
#include "../../include/resshift_hip.h"
#include <string>

// ---- the per-operand size limit (common.h: RS_BUFFER_BYTES_LIMIT), checked by name before anything is launched
#define RS_ERR_OPERAND_BYTES (-7)   // the code of such a refusal; rs_last_error() has the text below
struct RsOperand { const char* name; unsigned long long bytes, per_image; };   // per_image 0: the operand does not grow with the batch (weights)
// The first of `ops` at or above the limit, as "<layer>: operand <name> of <kernel> is <n> bytes ..."; false: all fit.  The batch it quotes
// is what fits THIS operand: a later layer of the graph may allow less.  ONE text for the graph
// layer (Exec::fail, in the dry pass) and for the launchers (rs_set_last_error).
static inline bool rs_operand_over(const std::string& layer, const char* kernel, const RsOperand* ops, int n, std::string* text) {
    for (int i = 0; i < n; ++i) {
        if (ops[i].bytes < RS_BUFFER_BYTES_LIMIT) continue;
        const unsigned long long fit = ops[i].per_image ? (RS_BUFFER_BYTES_LIMIT - 1) / ops[i].per_image : 0;
        *text = layer + ": operand " + ops[i].name + " of " + kernel + " is " + std::to_string(ops[i].bytes) + " bytes; the kernel addresses it with 32-bit byte "
                "offsets and takes operands below " + std::to_string(RS_BUFFER_BYTES_LIMIT) + " bytes (RS_BUFFER_BYTES_LIMIT); " +
                (ops[i].per_image ? "for this operand the largest batch that fits is " + std::to_string(fit) : std::string("no batch fits: the operand does not grow with it"));
        return true;
    }
    return false;
}
static inline const char* rs_conv_kernel_name(int k) {
    static const char* const nm[] = {"no kernel", "wino", "igemm4 (halo)", "igemm4 (halo, small planes)", "igemm_split", "igemm3", "igemm2", "igemm"};
    return k >= 0 && k < 8 ? nm[k] : "?";
}
// ... of a planned conv: the operands its kernel reaches through buffer descriptors (the launchers' own x_bytes / w_bytes / sx_bytes).  igemm.hip
// (CK_IGEMM) addresses everything through 64-bit pointers and has no limit.
static inline bool rs_conv_operand_over(const std::string& layer, const IGemmParams& p, int in_dt, const ConvPlan& pl, std::string* text) {
    if (pl.kernel == CK_NONE || pl.kernel == CK_IGEMM) return false;
    const unsigned long long esz = rs_dtype_size(in_dt), px = (unsigned long long)p.Hs * p.Ws;
    const RsOperand ops[3] = {{"x0", px * p.B * p.ld0 * esz, px * p.ld0 * esz},
                              {"w", pl.kernel == CK_WINO ? 0ull : (unsigned long long)p.Cout * p.Ktot * esz, 0},
                              {"sx", p.sC > 0 ? px * p.B * p.sld * esz : 0ull, px * p.sld * esz}};
    return rs_operand_over(layer, rs_conv_kernel_name(pl.kernel), ops, 3, text);
}
// ... of a fused qkv + window attention launch: the tokens and the shortcut
// (ldres 0: none - a dry pass of the graph layer has no pointers to ask)
static inline bool rs_win_attn_operand_over(const std::string& layer, int B, int H, int W, int ldx, int ldres, bool split, std::string* text) {
    const unsigned long long esz = split ? 4 : 2, px = (unsigned long long)H * W;
    const RsOperand ops[2] = {{"x", px * B * ldx * esz, px * ldx * esz}, {"res", px * B * ldres * esz, px * ldres * esz}};
    return rs_operand_over(layer, split ? "win_attn_qkv_split" : "win_attn_qkv", ops, 2, text);
}

extern "C" {
int rs_set_last_error(const char* text, int rc);   // engine.hip (rs_last_error's text); returns rc
// ---- the conv planner and what it routes to
int rs_conv_plan(const IGemmParams* p, int in_dt, int out_dt, int nz, ConvPlan* plan);   // igemm.hip: THE kernel / tile / split-K decision
int rs_conv_launch(const IGemmParams* p, int in_dt, int out_dt, int nz, const ConvPlan* plan, hipStream_t st);
int rs_splitk_reduce_launch(const IGemmParams* p, int out_dt, hipStream_t st);         // igemm.hip
int rs_splitk_reduce_stats_launch(const IGemmParams* p, int out_dt, hipStream_t st);   // igemm4.hip: reduce + statistics (+ GroupNorm tail)
int rs_igemm2_pick(int M, int Cout, int nz, int* BP, int* BC);   // *BP: 64 or 128 pixels per tile
int rs_igemm2_launch(const IGemmParams* pp, int in_dt, int out_dt, int BP, int BC, int nz, hipStream_t st);
int rs_igemm3_pick(int M, int Cout, int Ktot, int in_dt, int nz, int splitk, int* BC);
int rs_igemm3_launch(const IGemmParams* pp, int out_dt, int BC, hipStream_t st);
int rs_igemm4_plan(const IGemmParams* pp, int in_dt, int out_dt, int nz, ConvPlan* pl);
int rs_igemm4_launch(const IGemmParams* pp, int in_dt, const ConvPlan* pl, hipStream_t st);
int rs_igemm4_seg_launch(const IGemmParams* pp, int in_dt, int SEG, int BC, hipStream_t st);   // igemm4s.hip
int rs_wino_plan(const IGemmParams* pp, int in_dt, int out_dt, int nz, ConvPlan* pl);
int rs_wino_launch(const IGemmParams* pp, hipStream_t st);
void rs_igemm_split_plan(const IGemmParams* pp, int out_dt, int nz, int can_split, ConvPlan* pl);
int rs_igemm_split_launch(const IGemmParams* pp, int out_dt, int nz, const ConvPlan* pl, hipStream_t st);
// ---- everything else the engine launches
size_t rs_wino_weight_bytes(int Cin, int Cout);
float rs_wino_pack(const float* w_ref, int Cin, int Cout, void* dst);
int rs_wino_tiles(const IGemmParams* p);
int rs_direct_conv_launch(const DirectConvParams* p, int in_dt, int out_dt, hipStream_t st);
int rs_head_conv_launch(const void* x, int in_dt, const float* coef_dev, const float* w_dev, const float* bias_dev, float* y, int B, int H, int W, int C,
                        int ldx, int Cout, int ldy, hipStream_t st);
int rs_groupnorm_launch(const GNParams* p, int dt, int apply_slabs, hipStream_t st);
int rs_win_attn_launch(const WinAttnParams* p, int dt, hipStream_t st);
int rs_softmax_rows_launch(const float* s, void* out, int out_dt, long long nrows, int ncols, long long lds_, long long ldo, hipStream_t st);
int rs_nchw_to_nhwc_launch(const float* in, void* out, int out_dt, int B, int C, int HW, int ldo, int coff, float scale, hipStream_t st);
int rs_nhwc_to_nchw_launch(const void* in, int in_dt, float* out, int B, int C, int HW, int ldi, int coff, hipStream_t st);
int rs_axpbypcz_launch(const float* x, const float* z, const float* n, float* y, float a, float b, float c, long long cnt, hipStream_t st);
int rs_axpbypcz_rows_launch(const float* x, const float* z, const float* n, float* y, const float* a, const float* b, const float* c, long long per,
                            int B, hipStream_t st);
int rs_axpbypcz_seeded_launch(const float* x, const float* z, float* y, const float* a, const float* b, const float* c, const rs_noise_key* keys,
                              const rs_noise_key* keys_dev, const int* draw, long long per, int B, hipStream_t st);
int rs_film_gather_launch(const float* const* rows, int B, int total, float* out, hipStream_t st);
int rs_nchw_to_nhwc_rows_launch(const float* in, void* out, int out_dt, int B, int C, int HW, int ldo, int coff, const float* scale, hipStream_t st);
int rs_clamp_launch(float* x, float lo, float hi, long long cnt, hipStream_t st);
int rs_win_attn_qkv_supported(int heads, int E);
int rs_win_attn_qkv_launch(const WinAttnParams* p, hipStream_t st);
int rs_win_attn_qkv_split_launch(const WinAttnParams* p, hipStream_t st);
int rs_ae_flash_supported(int C, int T);
int rs_ae_flash_launch(const AeFlashCall* c, hipStream_t st);
int rs_ae_flash_split_supported(int C, int T);
int rs_ae_flash_split_launch(const AeFlashCall* c, hipStream_t st);
int rs_swin_mlp_supported(int E, int HD);
int rs_swin_mlp_launch(const SwinMlpCall* c, hipStream_t st);
int rs_swin_mlp_split_unembed_supported(int E, int HD, int NO);
int rs_swin_mlp_split_launch(const SwinMlpCall* c, hipStream_t st);   // (c->NO != E: + patch_unembed)
int rs_small_linear_launch(const float* x, const float* w, const float* bias, float* y, int R, int K, int N, int silu_in, int silu_out, hipStream_t st);
int rs_bicubic_launch(const float* in, void* out, int out_dt, int B, int C, int H, int W, int sf, int ldo, hipStream_t st);
int rs_interp_launch(const float* in, float* out, long long planes, int H, int W, int Ho, int Wo, double step_h, double step_w, int mode, int clamp,
                     hipStream_t st);   // degrade.hip: F.interpolate without antialiasing, mode = RS_INTERP_*; the caller has checked the arguments
int rs_vq_launch(const float* z, const float* codebook, float* zq, int* idx, long long N, int NE, int D, hipStream_t st);
int rs_copy_channels_launch(const void* src, int lds_, void* dst, int ldd, int C, long long npix, int dt, hipStream_t st);
int rs_convert_launch(const void* src, int src_dt, void* dst, int dst_dt, int C, long long npix, hipStream_t st);
}

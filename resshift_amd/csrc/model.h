// What is packed and where: the config, the checkpoint's host tensors, the weight blob's layout and the per-layer descriptors of the UNet
// (UNetModelSwin) and the autoencoder (VQModelTorch).  Host code: model.hip builds it, graphs.h executes it through a const Model&.
#pragma once
#include "launchers.h"
#include <cstdlib>
#include <functional>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

// The RS_* environment knobs (rs_env_on / rs_env_int / rs_env_set, common.h): a call site keeps the value in a function-local static (read
// once per process, at first use; nothing sets an RS_ knob after the first engine call), a knob that two places need has ONE accessor below.
static inline bool rs_knob_gn_epi_stats() { static const bool on = rs_env_on("RS_GN_EPI_STATS"); return on; }
static inline bool rs_knob_gn_gen_stats() { static const bool on = rs_env_on("RS_GN_GEN_STATS"); return on; }
static inline bool rs_knob_gn_conv_fold() { static const bool on = rs_env_on("RS_GN_CONV_FOLD"); return on; }

struct HostTensor { std::vector<float> data; std::vector<int64_t> shape; };

// ------------------------------------------------------------------ weight blob
struct Blob {
    char* base = nullptr;
    size_t off = 0;
    bool fill = false;
    std::vector<char> staging;
    void* add(size_t bytes, const std::function<void(char*)>& filler) {
        const size_t o = (off + 255) & ~(size_t)255;
        off = o + bytes;
        if (fill) filler(staging.data() + o);
        return base + o;  // only meaningful once bound
    }
};

struct ConvW {
    int Cin = 0, CinP = 0, Cout = 0, KH = 1, KW = 1;
    void* wh = nullptr; void* wf = nullptr; void* ws = nullptr; float* wd = nullptr; float* bias = nullptr;
    // fragment-major copies for the fused window-attention kernels (add_frag_copies): [16-row block][32-wide k step][lane] x 16 B (fp16;
    // split: 1 KB of hi then 1 KB of lo per block and k step), so that a wave's A-operand fragment is ONE contiguous 1 KB read
    void* wh_frag = nullptr; void* ws_frag = nullptr;
    void* ww = nullptr;   // Winograd F(2x2,3x3) form of a 3x3 conv's split weights (wino.hip: rs_wino_pack order), packed only with RS_WINO=1
    bool direct = false;
    int idx = -1;   // position in Model::big_w (per-layer "|w| >= 30" flags, see there)
    const void* w_for(int dt) const { return dt == RS_F16 ? wh : (dt == RS_F16S ? ws : wf); }
    const void* w_frag_for(int dt) const { return dt == RS_F16 ? wh_frag : (dt == RS_F16S ? ws_frag : nullptr); }
};
struct GNW { float* gamma = nullptr; float* beta = nullptr; int C = 0; };
struct ResBlockW { GNW n1, n2; ConvW c1, c2, skip; bool has_skip = false; int Cin = 0, Cout = 0; int film_off = -1; ConvW emb; };
struct SwinBlockW { GNW n1, n2; ConvW qkv, proj, fc1, fc2; float* bias_t = nullptr; float* bias_n = nullptr; float* bias_c = nullptr; int shift = 0; };
struct BasicLayerW { ConvW embed, unembed; std::vector<SwinBlockW> blocks; int C = 0, E = 0;
                     ConvW unfold; bool has_unfold = false; };   // unfold: [Wu W2 | Wu] of the last block's fc2 and patch_unembed (basiclayer())
struct UBlock {
    bool has_conv = false, has_res = false, has_swin = false, has_down = false, has_up = false;
    ConvW conv; ResBlockW res; BasicLayerW swin; int out_ch = 0; int level = 0;
    ConvW upf[4]; bool has_upf = false;   // sub-pixel form of the upsampling conv (add_upfold())
};
struct AttnW { GNW norm; ConvW q, k, v, proj; int C = 0; };
struct AELevel { std::vector<ResBlockW> blocks; bool has_resample = false; ConvW resample; ConvW upf[4]; bool has_upf = false; };

struct Model {
    rs_config cfg;
    std::unordered_map<std::string, HostTensor> host;
    Blob blob;
    size_t blob_bytes = 0;
    std::string build_err;
    // Split precision is optional per checkpoint: the halo kernel scales the hi weight fragment by 2^11 in fp16, which is exact only
    // for |w| < 32 (igemm4.hip).  A checkpoint with a larger (or non-finite) conv / linear weight still loads and runs in fp16 /
    // fp32; only a call that asks for RS_PREC_SPLIT fails (rs_engine::split_ok).
    std::string split_err;
    // ... and a layer whose weights reach |w| >= 30 is not a reason to refuse the policy: only the kernels that scale the hi fragment by
    // 2^11 (the halo conv, the fused split Swin kernels) cannot take it, the generic split kernel (igemm_split.hip: two accumulators, no
    // scaling) can.  One flag byte per conv / linear in build order, written into the blob by the packing rank (it travels with the
    // broadcast) and read back by rs_weights_ready; ConvCall (IGemmParams::unscaled_w) / basiclayer() route a flagged layer to the generic kernels.
    std::vector<unsigned char> big_w;
    int conv_count = 0;
    unsigned char* big_w_dev = nullptr;
    bool big(const ConvW& c) const { return c.idx >= 0 && c.idx < (int)big_w.size() && big_w[c.idx] != 0; }
    // UNet
    std::vector<UBlock> in_blocks, out_blocks;
    ResBlockW mid_res1, mid_res2; BasicLayerW mid_swin;
    std::vector<ConvW> fe_convs, fe_downs;
    GNW out_norm; ConvW out_conv;
    ConvW te0, te2;  // time_embed linears
    std::vector<int> skip_ch, h_ch;  // per input block / per output block
    int film_total = 0, fe_out_ch = 0;
    std::vector<ResBlockW*> film_blocks;
    // AE
    ConvW enc_in, enc_out, dec_in, dec_out, quant_conv, post_quant_conv;
    std::vector<AELevel> enc_levels, dec_levels;
    ResBlockW enc_mid1, enc_mid2, dec_mid1, dec_mid2;
    AttnW enc_attn, dec_attn;
    GNW enc_norm, dec_norm;
    float* codebook = nullptr;

    // ---------------------------------------------------------------- build
    // tensors the packer derives from checkpoint tensors (products of two linear maps that run as one GEMM): made on first use
    std::map<std::string, std::function<bool(HostTensor&)>> derived;
    const HostTensor* find(const std::string& k);
    const float* find_data(const std::string& k, size_t n);   // ... of exactly n floats ("bad size for" otherwise)
    // the blob's layout (fill == false: offsets and pointers only) or its bytes, into blob.staging; returns the blob's size
    size_t build(char* base, bool fill);
    void collect_film_blocks();

private:
    float* add_f32(const std::string& key, size_t n);
    ConvW add_conv(const std::string& prefix, int Cin, int Cout, int KH, int KW, bool has_bias = true, bool force_direct = false, bool head = false);
    bool add_upfold(const std::string& prefix, int C, ConvW (&upf)[4]);
    void add_frag_copies(ConvW& c, const std::string& prefix);
    ConvW add_linear_f32(const std::string& prefix, int K, int N);
    GNW add_gn(const std::string& prefix, int C);
    ResBlockW add_resblock(const std::string& p, int Cin, int Cout, int emb_ch);
    BasicLayerW add_basiclayer(const std::string& p, int C, int ds);
    bool in_attn_res(int ds) const;
    void build_unet();
    ResBlockW add_resnet(const std::string& p, int Cin, int Cout);
    AttnW add_attn(const std::string& p, int C);
    void build_ae();
};

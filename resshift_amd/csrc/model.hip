// The model packer: walks the config once per build() and lays every tensor of the checkpoint into ONE device blob whose layout is a pure
// function of the config (a multi-GPU host broadcasts it with a single RCCL call).  build(nullptr, false) sizes the blob, build(dev, false)
// resolves the descriptors' pointers, build(dev, true) also fills blob.staging through the packers of weight_pack.h.  Host code apart from
// rs_wino_weight_bytes / rs_wino_pack (wino.hip) and rs_swin_mlp_split_unembed_supported (swin_mlp.hip).
// Reference construction: models/unet.py:632-865, ldm/modules/diffusionmodules/model.py:452-660 (file:line into the reference repo).
#include "model.h"
#include "weight_pack.h"
#include <algorithm>
#include <cmath>
#include <cstring>

const HostTensor* Model::find(const std::string& k) {
    auto it = host.find(k);
    if (it == host.end()) {
        auto d = derived.find(k);
        if (d != derived.end()) {
            HostTensor t;
            if (d->second(t)) it = host.emplace(k, std::move(t)).first;
        }
    }
    if (it == host.end()) { if (build_err.empty()) build_err = "missing state_dict key: " + k; return nullptr; }
    return &it->second;
}
const float* Model::find_data(const std::string& k, size_t n) {
    const HostTensor* t = find(k);
    if (!t) return nullptr;
    if (t->data.size() != n) { if (build_err.empty()) build_err = "bad size for " + k; return nullptr; }
    return t->data.data();
}
float* Model::add_f32(const std::string& key, size_t n) {
    return (float*)blob.add(n * sizeof(float), [&](char* dst) {
        if (const float* t = find_data(key, n)) memcpy(dst, t, n * sizeof(float));
    });
}
// Every conv runs on the MFMA implicit GEMM; input channels are zero-padded to a multiple of 8 (CinP) so that the
// 16-byte K chunks stay aligned (3/6-channel image and latent inputs become 8-channel tensors; the staging buffer is
// zero-initialised, so padded input channels keep zero weights).  `force_direct`
// keeps the scalar kernel for the fp32-in/fp32-out 1x1 quant convs and for two-source convs whose first source is
// not chunk aligned.
// `head`: an output head (3x3, <= 4 output channels, Cin % 8 == 0): ALSO the fp32 [tap][Cin][Cout] form for the fused GroupNorm + SiLU +
// conv kernel (direct_conv.hip: gn_silu_head_conv_kernel)
// The formats are weight_pack.h's; the policy - what a weight's magnitude means for build_err, split_err and big_w - is decided here.
ConvW Model::add_conv(const std::string& prefix, int Cin, int Cout, int KH, int KW, bool has_bias, bool force_direct, bool head) {
    ConvW c; c.Cin = Cin; c.Cout = Cout; c.KH = KH; c.KW = KW;
    c.idx = conv_count++;
    if ((int)big_w.size() < conv_count) big_w.resize(conv_count, 0);
    const int cidx = c.idx;
    c.direct = force_direct;
    c.CinP = c.direct ? Cin : (Cin + 7) / 8 * 8;
    const int CinP = c.CinP, taps = KH * KW;
    const size_t n = (size_t)taps * Cin * Cout, np = (size_t)taps * CinP * Cout;
    const std::string wkey = prefix + ".weight";
    auto get = [&]() { return find_data(wkey, n); };
    if (c.direct) {
        c.wd = (float*)blob.add(n * 4, [&](char* dst) { if (const float* w = get()) rs_pack_tap_major(w, Cout, Cin, taps, (float*)dst); });
    } else {
        if (cfg.enable_f16)
            c.wh = blob.add(np * 2, [&](char* dst) {
                const float* w = get(); if (!w) return;
                const PackStat s = rs_pack_rows_f16(w, Cout, Cin, taps, CinP, (f16*)dst);
                // (a derived weight - the sub-pixel form's summed taps - can reach 4 |w|: outside the fp16 range it would become inf silently)
                if ((s.non_finite || s.max_abs > 65504.0f) && build_err.empty()) build_err = "fp16 storage needs weights inside the fp16 range: " + wkey;
            });
        if (cfg.enable_split)
            c.ws = blob.add(np * 4, [&](char* dst) {
                const float* w = get(); if (!w) return;
                const PackStat s = rs_pack_rows_split(w, Cout, Cin, taps, CinP, (f16*)dst);
                // (the halo kernel and the fused Swin kernels scale the hi fragment by 2^11 in fp16: exact below 32 - a layer
                // beyond that runs on the generic split kernel; a non-finite weight rules the policy out)
                if (s.non_finite || s.max_abs > 60000.0f) { if (split_err.empty()) split_err = "split precision needs finite fp16-range weights: " + wkey; }
                if (s.max_abs >= 30.0f) big_w[cidx] = 1;
            });
        // Winograd F(2x2,3x3) form (wino.hip).  RS_WINO=0 when the engine is CREATED switches it off (the blob layout depends on it: every rank
        // of a run has to agree, like RS_UPFOLD).  Only the layers whose whole output fits 160-channel blocks (the UNet's 160 / 320-channel ResBlock
        // convs, + 200 MB of blob): on those the kernel measured 1.07 - 1.12 x the halo kernel - 243.6 -> 238.6 ms per parity pass on one box,
        // two pairs - on the autoencoder's 128 / 256 / 512-channel layers 0.92 - 1.04 x (profiles/r6_wino_bench.txt).
        static const bool wino_on = rs_env_on("RS_WINO");
        if (wino_on && cfg.enable_split && KH == 3 && KW == 3 && (Cin % 32) == 0 && Cin <= 640 && (Cout % 160) == 0 && Cout <= 320)
            c.ww = blob.add(rs_wino_weight_bytes(Cin, Cout), [&](char* dst) {
                const float* w = get(); if (!w) return;
                if (!(rs_wino_pack(w, Cin, Cout, dst) < 30.0f)) big_w[cidx] = 1;   // (the kernel scales the hi fragment by 2^11 in fp16, like the halo kernel)
            });
        if (cfg.enable_f32)
            c.wf = blob.add(np * 4, [&](char* dst) { if (const float* w = get()) rs_pack_rows_f32(w, Cout, Cin, taps, CinP, (float*)dst); });
    }
    if (head && !c.direct && KH == 3 && KW == 3 && Cout <= 4 && (Cin % 8) == 0)
        c.wd = (float*)blob.add(n * 4, [&](char* dst) { if (const float* w = get()) rs_pack_tap_major(w, Cout, Cin, taps, (float*)dst); });
    if (has_bias) c.bias = add_f32(prefix + ".bias", Cout);
    return c;
}
// Sub-pixel form of "nearest x2 upsample, then conv3x3" (models/unet.py:53-81 Upsample, ldm/modules/diffusionmodules/model.py:50-65):
// every output pixel (2y + py, 2x + px) sees only a 2 x 2 neighbourhood of the LOW-resolution input, because the taps that land on the
// same source pixel can be added up front - rows: py = 0: {y - 1: w[0], y: w[1] + w[2]}, py = 1: {y: w[0] + w[1], y + 1: w[2]}, columns
// alike; zero padding of the upsampled image IS zero padding of the source (rows -1 and 2H map to -1 and H).  Four 2x2 convs (one per
// output parity, pad_t = 1 - py, pad_l = 1 - px) with K = 4 Cin instead of one 3x3 conv with K = 9 Cin on four times the pixels: 2.25 x
// fewer multiply-adds, the same result up to the rounding of the summed weights (rs_subpixel_weight: formed in double from the
// checkpoint's tensor, like the other derived matrices).  The generic kernels scatter their rows into the big tensor (IGemmParams::osc).
// RS_UPFOLD=0: off.
bool Model::add_upfold(const std::string& prefix, int C, ConvW (&upf)[4]) {
    static const bool on = rs_env_on("RS_UPFOLD");
    if (!on || (C % 8)) return false;
    for (int q = 0; q < 4; ++q) {
        const int py = q >> 1, px = q & 1;
        const std::string fk = prefix + ".upfold" + std::to_string(q);
        derived[fk + ".weight"] = [this, prefix, C, py, px](HostTensor& t) {
            const HostTensor* w = find(prefix + ".weight");
            if (!w || w->data.size() != (size_t)C * C * 9) return false;
            t.data = rs_subpixel_weight(w->data.data(), C, py, px);
            t.shape = {C, C, 2, 2};
            return true;
        };
        derived[fk + ".bias"] = [this, prefix, C](HostTensor& t) {
            const HostTensor* b = find(prefix + ".bias");
            if (!b || b->data.size() != (size_t)C) return false;
            t = *b;
            return true;
        };
        upf[q] = add_conv(fk, C, C, 2, 2);
    }
    return true;
}
// Fragment-major copies of a 1x1 weight [N][K] (N % 16 == 0, K % 32 == 0) for win_attn_qkv_kernel / win_attn_qkv_split_kernel: lane
// (lr, lg) of the wave that multiplies rows 16 nb .. 16 nb + 15 with k step ks reads W[16 nb + lr][32 ks + 8 lg .. + 7] - from the
// row-major weight that is 16 different cache lines per wave instruction, from this copy 8 full ones.
void Model::add_frag_copies(ConvW& c, const std::string& prefix) {
    const int N = c.Cout, K = c.Cin;
    if (c.KH != 1 || c.KW != 1 || (N % 16) || (K % 32)) return;
    const std::string wkey = prefix + ".weight";
    const size_t n = (size_t)N * K;
    auto get = [this, wkey, n]() -> const float* {
        const HostTensor* t = find(wkey);
        return (t && t->data.size() == n) ? t->data.data() : nullptr;
    };
    if (cfg.enable_f16)
        c.wh_frag = blob.add(n * 2, [=](char* dst) { if (const float* w = get()) rs_pack_frag_major(w, N, K, (f16*)dst, nullptr); });
    if (cfg.enable_split)
        c.ws_frag = blob.add(n * 4, [=](char* dst) { if (const float* w = get()) rs_pack_frag_major(w, N, K, nullptr, (f16*)dst); });
}
// plain fp32 linear kept in the reference [N][K] layout (time embedding MLP, emb_layers)
ConvW Model::add_linear_f32(const std::string& prefix, int K, int N) {
    ConvW c; c.Cin = K; c.Cout = N;
    c.wd = add_f32(prefix + ".weight", (size_t)K * N);
    c.bias = add_f32(prefix + ".bias", N);
    return c;
}
GNW Model::add_gn(const std::string& prefix, int C) {
    GNW g; g.C = C; g.gamma = add_f32(prefix + ".weight", C); g.beta = add_f32(prefix + ".bias", C); return g;
}
ResBlockW Model::add_resblock(const std::string& p, int Cin, int Cout, int emb_ch) {
    ResBlockW r; r.Cin = Cin; r.Cout = Cout;
    r.n1 = add_gn(p + ".in_layers.0", Cin);
    r.c1 = add_conv(p + ".in_layers.2", Cin, Cout, 3, 3);
    r.emb = add_linear_f32(p + ".emb_layers.1", emb_ch, 2 * Cout);
    r.n2 = add_gn(p + ".out_layers.0", Cout);
    r.c2 = add_conv(p + ".out_layers.3", Cout, Cout, 3, 3);
    r.has_skip = Cin != Cout;
    if (r.has_skip) r.skip = add_conv(p + ".skip_connection", Cin, Cout, 1, 1);
    r.film_off = film_total; film_total += 2 * Cout;
    return r;
}
BasicLayerW Model::add_basiclayer(const std::string& p, int C, int ds) {
    const rs_unet_config& u = cfg.unet;
    BasicLayerW b; b.C = C; b.E = u.swin_embed_dim;
    const int E = b.E, heads = u.num_heads, hidden = (int)(E * u.mlp_ratio);
    b.embed = add_conv(p + ".patch_embed.proj", C, E, 1, 1);
    for (int d = 0; d < u.swin_depth; ++d) {
        const std::string q = p + ".blocks." + std::to_string(d);
        SwinBlockW s;
        // shift_size is fixed at construction from the *constructed* resolution (swin_transformer.py:189-194)
        s.shift = (d % 2 == 1 && ds > u.window_size) ? u.window_size / 2 : 0;
        s.n1 = add_gn(q + ".norm1", E);
        s.qkv = add_conv(q + ".attn.qkv", E, 3 * E, 1, 1);
        add_frag_copies(s.qkv, q + ".attn.qkv");
        // the relative position bias in its three forms (weight_pack.h); a table of the wrong size is reported once, by the first
        const std::string tkey = q + ".attn.relative_position_bias_table";
        auto table = [this, tkey, heads](bool report) -> const float* {
            const HostTensor* t = find(tkey);
            if (t && (int)t->data.size() == 225 * heads) return t->data.data();
            if (t && report && build_err.empty()) build_err = "bad size for " + tkey;
            return nullptr;
        };
        s.bias_t = (float*)blob.add((size_t)heads * 64 * 64 * 4, [=](char* dst) { if (const float* t = table(true)) rs_pack_bias_tables(t, heads, (float*)dst, nullptr); });
        s.bias_n = (float*)blob.add((size_t)heads * 64 * 64 * 4, [=](char* dst) { if (const float* t = table(false)) rs_pack_bias_tables(t, heads, nullptr, (float*)dst); });
        s.bias_c = (float*)blob.add((size_t)heads * 256 * 4, [=](char* dst) { if (const float* t = table(false)) rs_pack_bias_compact(t, heads, (float*)dst); });
        s.proj = add_conv(q + ".attn.proj", E, E, 1, 1);
        add_frag_copies(s.proj, q + ".attn.proj");
        s.n2 = add_gn(q + ".norm2", E);
        s.fc1 = add_conv(q + ".mlp.fc1", E, hidden, 1, 1);
        s.fc2 = add_conv(q + ".mlp.fc2", hidden, E, 1, 1);
        b.blocks.push_back(s);
    }
    b.unembed = add_conv(p + ".patch_unembed.proj", E, C, 1, 1);
    // patch_unembed folded into the last block's fused split MLP (swin_mlp.hip, NO != E): a [C][hidden + E] matrix and a C-vector
    // (rs_unembed_fold_weight / _bias: products in double from the checkpoint's tensors)
    if (cfg.enable_split && u.swin_depth > 0 && rs_swin_mlp_split_unembed_supported(E, hidden, C)) {
        const std::string fk = p + ".patch_unembed.fold", uk = p + ".patch_unembed.proj", mk = p + ".blocks." + std::to_string(u.swin_depth - 1) + ".mlp.fc2";
        derived[fk + ".weight"] = [this, uk, mk, E, hidden, C](HostTensor& t) {
            const HostTensor* wu = find(uk + ".weight"); const HostTensor* w2 = find(mk + ".weight");
            if (!wu || !w2 || wu->data.size() != (size_t)C * E || w2->data.size() != (size_t)E * hidden) return false;
            t.data = rs_unembed_fold_weight(wu->data.data(), w2->data.data(), C, E, hidden);
            t.shape = {C, hidden + E, 1, 1};
            return true;
        };
        derived[fk + ".bias"] = [this, uk, mk, E, C](HostTensor& t) {
            const HostTensor* wu = find(uk + ".weight"); const HostTensor* bu = find(uk + ".bias"); const HostTensor* b2 = find(mk + ".bias");
            if (!wu || !bu || !b2 || wu->data.size() != (size_t)C * E || bu->data.size() != (size_t)C || b2->data.size() != (size_t)E) return false;
            t.data = rs_unembed_fold_bias(wu->data.data(), bu->data.data(), b2->data.data(), C, E);
            t.shape = {C};
            return true;
        };
        b.unfold = add_conv(fk, hidden + E, C, 1, 1);
        b.has_unfold = true;
    }
    return b;
}
bool Model::in_attn_res(int ds) const {
    for (int i = 0; i < cfg.unet.n_attn_res; ++i) if (cfg.unet.attention_resolutions[i] == ds) return true;
    return false;
}
void Model::build_unet() {
    const rs_unet_config& u = cfg.unet;
    in_blocks.clear(); out_blocks.clear(); fe_convs.clear(); fe_downs.clear(); skip_ch.clear(); h_ch.clear();
    film_total = 0;
    const int mc = u.model_channels, emb_ch = 4 * mc;
    te0 = add_linear_f32("time_embed.0", mc, emb_ch);
    te2 = add_linear_f32("time_embed.2", emb_ch, emb_ch);
    int base_chn;
    if (u.cond_lq && u.lq_size == u.image_size) {
        base_chn = u.cond_mask ? 4 : 3;
    } else {
        int feature_chn = u.cond_mask ? 4 : 3;
        base_chn = 16;
        const int stages = (int)std::lround(std::log2((double)u.lq_size / u.image_size));
        for (int ii = 0; ii < stages; ++ii) {
            fe_convs.push_back(add_conv("feature_extractor." + std::to_string(3 * ii), feature_chn, base_chn, 3, 3));
            fe_downs.push_back(add_conv("feature_extractor." + std::to_string(3 * ii + 2) + ".op", base_chn, base_chn * 2, 3, 3));
            base_chn *= 2;
            feature_chn = base_chn;
        }
    }
    fe_out_ch = u.cond_lq ? base_chn : 0;
    int ch = u.channel_mult[0] * mc;
    const int input_ch = ch;
    {
        UBlock b; b.has_conv = true; b.level = 0; b.out_ch = ch;
        // with a feature extractor the conv reads two sources (x | features): both must be 16-byte chunk aligned
        const bool two_src_unaligned = !fe_convs.empty() && (u.in_channels % 8 != 0);
        b.conv = add_conv("input_blocks.0.0", u.in_channels + fe_out_ch, ch, 3, 3, true, two_src_unaligned);
        in_blocks.push_back(b);
    }
    std::vector<int> chans{ch};
    int ds = u.image_size;
    for (int level = 0; level < u.n_levels; ++level) {
        const int mult = u.channel_mult[level];
        for (int jj = 0; jj < u.num_res_blocks[level]; ++jj) {
            UBlock b; b.level = level;
            const std::string p = "input_blocks." + std::to_string(in_blocks.size());
            b.has_res = true; b.res = add_resblock(p + ".0", ch, mult * mc, emb_ch);
            ch = mult * mc;
            if (in_attn_res(ds) && jj == 0) { b.has_swin = true; b.swin = add_basiclayer(p + ".1", ch, ds); }
            b.out_ch = ch;
            in_blocks.push_back(b); chans.push_back(ch);
        }
        if (level != u.n_levels - 1) {
            UBlock b; b.level = level + 1; b.has_down = true; b.out_ch = ch;
            b.conv = add_conv("input_blocks." + std::to_string(in_blocks.size()) + ".0.op", ch, ch, 3, 3);
            in_blocks.push_back(b); chans.push_back(ch);
            ds /= 2;
        }
    }
    skip_ch = chans;
    mid_res1 = add_resblock("middle_block.0", ch, ch, emb_ch);
    mid_swin = add_basiclayer("middle_block.1", ch, ds);
    mid_res2 = add_resblock("middle_block.2", ch, ch, emb_ch);
    for (int level = u.n_levels - 1; level >= 0; --level) {
        const int mult = u.channel_mult[level];
        for (int i = 0; i <= u.num_res_blocks[level]; ++i) {
            const int ich = chans.back(); chans.pop_back();
            UBlock b; b.level = level;
            const std::string p = "output_blocks." + std::to_string(out_blocks.size());
            h_ch.push_back(ch);
            int sub = 0;
            b.has_res = true; b.res = add_resblock(p + "." + std::to_string(sub++), ch + ich, mc * mult, emb_ch);
            ch = mc * mult;
            if (in_attn_res(ds) && i == 0) { b.has_swin = true; b.swin = add_basiclayer(p + "." + std::to_string(sub++), ch, ds); }
            if (level && i == u.num_res_blocks[level]) {
                b.has_up = true;
                b.conv = add_conv(p + "." + std::to_string(sub) + ".conv", ch, ch, 3, 3);
                b.has_upf = add_upfold(p + "." + std::to_string(sub++) + ".conv", ch, b.upf);
                ds *= 2;
            }
            b.out_ch = ch;
            out_blocks.push_back(b);
        }
    }
    out_norm = add_gn("out.0", ch);
    out_conv = add_conv("out.2", input_ch, u.out_channels, 3, 3, true, false, /*head=*/true);
}
ResBlockW Model::add_resnet(const std::string& p, int Cin, int Cout) {
    ResBlockW r; r.Cin = Cin; r.Cout = Cout;
    r.n1 = add_gn(p + ".norm1", Cin);
    r.c1 = add_conv(p + ".conv1", Cin, Cout, 3, 3);
    r.n2 = add_gn(p + ".norm2", Cout);
    r.c2 = add_conv(p + ".conv2", Cout, Cout, 3, 3);
    r.has_skip = Cin != Cout;
    if (r.has_skip) r.skip = add_conv(p + ".nin_shortcut", Cin, Cout, 1, 1);
    return r;
}
AttnW Model::add_attn(const std::string& p, int C) {
    AttnW a; a.C = C;
    a.norm = add_gn(p + ".norm", C);
    a.q = add_conv(p + ".q", C, C, 1, 1);
    a.k = add_conv(p + ".k", C, C, 1, 1);
    a.v = add_conv(p + ".v", C, C, 1, 1);
    a.proj = add_conv(p + ".proj_out", C, C, 1, 1);
    return a;
}
void Model::build_ae() {
    const rs_ae_config& a = cfg.ae;
    enc_levels.clear(); dec_levels.clear();
    // Encoder (model.py:452-547)
    enc_in = add_conv("encoder.conv_in", a.in_channels, a.ch, 3, 3);
    int block_in = a.ch;
    for (int l = 0; l < a.n_levels; ++l) {
        AELevel L;
        block_in = a.ch * (l == 0 ? 1 : a.ch_mult[l - 1]);
        const int block_out = a.ch * a.ch_mult[l];
        for (int i = 0; i < a.num_res_blocks[l]; ++i) {
            L.blocks.push_back(add_resnet("encoder.down." + std::to_string(l) + ".block." + std::to_string(i), block_in, block_out));
            block_in = block_out;
        }
        if (l != a.n_levels - 1) {
            L.has_resample = true;
            L.resample = add_conv("encoder.down." + std::to_string(l) + ".downsample.conv", block_in, block_in, 3, 3);
        }
        enc_levels.push_back(L);
    }
    enc_mid1 = add_resnet("encoder.mid.block_1", block_in, block_in);
    enc_attn = add_attn("encoder.mid.attn_1", block_in);
    enc_mid2 = add_resnet("encoder.mid.block_2", block_in, block_in);
    enc_norm = add_gn("encoder.norm_out", block_in);
    enc_out = add_conv("encoder.conv_out", block_in, a.z_channels, 3, 3, true, false, /*head=*/true);
    quant_conv = add_conv("quant_conv", a.z_channels, a.embed_dim, 1, 1, true, /*force_direct=*/true);  // fp32 in / fp32 out
    // Decoder (model.py:550-660)
    post_quant_conv = add_conv("post_quant_conv", a.embed_dim, a.z_channels, 1, 1, true, /*force_direct=*/true);  // fp32 VQ output in
    block_in = a.ch * a.ch_mult[a.n_levels - 1];
    dec_in = add_conv("decoder.conv_in", a.z_channels, block_in, 3, 3);
    dec_mid1 = add_resnet("decoder.mid.block_1", block_in, block_in);
    dec_attn = add_attn("decoder.mid.attn_1", block_in);
    dec_mid2 = add_resnet("decoder.mid.block_2", block_in, block_in);
    dec_levels.resize(a.n_levels);
    for (int l = a.n_levels - 1; l >= 0; --l) {
        AELevel L;
        const int block_out = a.ch * a.ch_mult[l];
        for (int i = 0; i <= a.num_res_blocks[l]; ++i) {
            L.blocks.push_back(add_resnet("decoder.up." + std::to_string(l) + ".block." + std::to_string(i), block_in, block_out));
            block_in = block_out;
        }
        if (l != 0) {
            L.has_resample = true;
            L.resample = add_conv("decoder.up." + std::to_string(l) + ".upsample.conv", block_in, block_in, 3, 3);
            L.has_upf = add_upfold("decoder.up." + std::to_string(l) + ".upsample.conv", block_in, L.upf);
        }
        dec_levels[l] = L;
    }
    dec_norm = add_gn("decoder.norm_out", block_in);
    dec_out = add_conv("decoder.conv_out", block_in, a.out_ch, 3, 3, true, false, /*head=*/true);
    codebook = add_f32("quantize.embedding.weight", (size_t)a.n_embed * a.embed_dim);
}
size_t Model::build(char* base, bool fill) {
    blob.base = base; blob.off = 0; blob.fill = fill;
    build_err.clear();
    split_err.clear();
    if (fill) blob.staging.assign(blob_bytes, 0);
    (void)blob.add(256, [](char*) {});   // header: word 0 = flags (bit 0: split weights usable), written by rs_pack_weights
    conv_count = 0;
    if (fill) std::fill(big_w.begin(), big_w.end(), 0);
    if (cfg.has_unet) build_unet();
    if (cfg.has_ae) build_ae();
    // (the fillers run in order: by the time this one copies the table every split-weight filler has set its flag)
    big_w_dev = (unsigned char*)blob.add((size_t)conv_count, [&](char* dst) { memcpy(dst, big_w.data(), (size_t)conv_count); });
    return (blob.off + 255) & ~(size_t)255;
}
void Model::collect_film_blocks() {
    film_blocks.clear();
    if (!cfg.has_unet) return;
    for (auto& b : in_blocks) if (b.has_res) film_blocks.push_back(&b.res);
    film_blocks.push_back(&mid_res1); film_blocks.push_back(&mid_res2);
    for (auto& b : out_blocks) if (b.has_res) film_blocks.push_back(&b.res);
}

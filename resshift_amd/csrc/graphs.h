// How a call executes: the model graphs (UNetModelSwin, VQModelTorch, the sampling loop's three parts) over a const Model&; Exec is the state
// of one pass - rs_engine::run (engine.hip) walks a graph twice per call: a dry sizing pass, then the real pass.
// Reference behaviour reproduced here (file:line into the reference repo):
//   UNetModelSwin forward                     models/unet.py:866-895
//   ResBlock                                  models/unet.py:110-206
//   BasicLayer / SwinTransformerBlock         models/swin_transformer.py:163-281,348-442
//   VQModelTorch encode/decode                ldm/models/autoencoder.py:28-40
//   Encoder / Decoder / ResnetBlock / AttnBlock  ldm/modules/diffusionmodules/model.py:90-203,452-660
//   p_sample_loop                             models/gaussian_diffusion.py:367-529
//
// Design notes
//   * NHWC activations; every conv/linear is one implicit-GEMM launch with fused bias/GELU/residual.
//   * Skip concatenations (unet.py:891) are zero-copy: each input block writes its output straight
//     into the upper channel slice of the buffer the matching output block will read, and the
//     decoder path writes into the lower slice (pixel stride = total channels).
//   * FiLM vectors (time_embed + every ResBlock's emb_layers) depend only on t: computed once per
//     distinct t on device and cached (rs_engine::film_row).
//   * A conv of a graph is a ConvCall, built by name at its call site (Graphs::k3 / k1 + setters) and consumed whole by everything that
//     plans, asks about or launches it; the other kernel families and the bodies take one parameter block each (common.h, Graphs::*Call).
//   * Debug-trace names nest through Exec::Scope: a block's inner records under "<block>.", its output under the enclosing prefix.
#pragma once
#include "model.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

namespace {

struct View {
    void* p = nullptr; int B = 0, H = 0, W = 0, C = 0, ld = 0, dt = RS_F16;
    // optional per-channel partial statistics of this tensor, [B][stS][stld][2] floats (IGemmParams::ystats): set by whoever
    // allocates the tensor when its producer is the halo conv kernel; the consuming GroupNorm then skips its statistics pass
    float* st = nullptr; int stS = 0, stld = 0;
    int st_prod = -1;   // sequence number of the launch that produces `st` (Exec::prod_seq): key of the GroupNorm tail plan
    // a channel concatenation (models/unet.py:891) whose halves have different producers: `st` covers channels [0, st_n0), `st2` the
    // rest (column 0 of an st2 row = channel st_n0).  st2 == nullptr: `st` covers all C channels.
    float* st2 = nullptr; int st2S = 0, st2ld = 0, st_n0 = 0;
    bool stats_complete() const { return st != nullptr; }
    void drop_stats() { st = nullptr; st2 = nullptr; st_prod = -1; }
    long long pixels() const { return (long long)B * H * W; }
    View slice(int c0, int c) const {
        View v = *this; v.p = (char*)p + (size_t)c0 * rs_dtype_chan_bytes(dt); v.C = c;
        if (st2) {   // a slice of a concatenation keeps statistics only when it is exactly one of the halves
            v.st2 = nullptr; v.st2S = v.st2ld = v.st_n0 = 0;
            if (c0 == 0 && c == st_n0) { /* first half: st as is */ }
            else if (c0 == st_n0 && c == C - st_n0) { v.st = st2; v.stS = st2S; v.stld = st2ld; v.st_prod = -1; }
            else { v.st = nullptr; v.stS = v.stld = 0; v.st_prod = -1; }
        } else if (st) v.st = st + 2 * (size_t)c0;
        return v;
    }
};

struct Arena {
    char* base = nullptr; size_t cap = 0, off = 0, peak = 0;
    void* alloc(size_t n) {
        off = (off + 255) & ~(size_t)255;
        void* p = base + off;
        off += n;
        peak = std::max(peak, off);
        return p;
    }
};

// GroupNorm tail plan (gn_tail.h): the launch that completes a tensor's statistics also writes the coefficients of the GroupNorm that
// consumes it.  The producer runs BEFORE the consumer is known, so the plan is made by the dry sizing pass - which walks the same
// control flow as the real pass - and keyed by the producer's sequence number: the consuming gn_coef() call of the dry pass claims its
// producer, the real pass attaches the tail at the producer's launch and skips the coefficient launch at the consumer.
struct TailPlan {
    bool on = false; int consumer = -1;
    const float* gamma = nullptr; const float* beta = nullptr; float eps = 0.f;
    long long film_off = -1;   // the consumer's FiLM rows relative to Exec::film_base (-1: no FiLM); an offset because a per-image table
                               // lives in the scratch arena, whose address the dry pass does not know yet
    int C = 0, HW = 0; size_t coef_off = 0;
    bool two = false; size_t st2_off = 0; int st2S = 0, st2ld = 0;   // the other half of a concatenation (statistics live in the pool)
    mutable bool drawn = false;   // (real pass: the producer's launch attached the tail - checked against the plan at the end of the call)
};

struct TraceRec { std::string name; int B = 0, C = 0, H = 0, W = 0; size_t off = 0; };   // (one debug-trace record: Exec::tr)

struct Exec {
    hipStream_t st = nullptr; Arena* arena = nullptr; bool dry = false; long long launches = 0; int err = 0;
    std::vector<TailPlan>* plan = nullptr;   // by producer sequence number
    int prod_seq = 0, gn_seq = 0;
    // FiLM rows of the network body being walked (unet_body): one row shared by the batch (film_ld 0) or a per-image table [B][film_ld]
    const float* film_base = nullptr; int film_ld = 0;
    // coefficient pool ([B][2][C] affines; behind the scratch arena, reset per network body - stream order keeps reuse safe) and the
    // ticket pool of the tails (zeroed once per call)
    char* pool_base = nullptr; size_t pool_off = 0, pool_peak = 0;
    unsigned* ticket_base = nullptr; size_t ticket_used = 0;
    float* pool(size_t bytes) {
        pool_off = (pool_off + 255) & ~(size_t)255;
        float* q = (float*)(pool_base + pool_off);
        pool_off += bytes;
        pool_peak = std::max(pool_peak, pool_off);
        return q;
    }
    // give a tensor that is about to be produced a statistics buffer of `slabs` partial sets per image, rows of `ld` channels, in the pool
    // (reset per network body: a block's output may carry it to whoever consumes it later) and its producer the next sequence number
    void attach_stats(View& v, int slabs, int ld) {
        v.stS = slabs; v.stld = ld;
        v.st = pool((size_t)v.B * slabs * ld * 2 * sizeof(float));
        v.st_prod = prod_seq++;
    }
    unsigned* tickets(int n) { unsigned* q = ticket_base + ticket_used; ticket_used += (size_t)n; return q; }
    const TailPlan* tail_of(int prod) const { return (plan && prod >= 0 && prod < (int)plan->size() && (*plan)[prod].on) ? &(*plan)[prod] : nullptr; }
    // the GNTail block of a producer's launch from its plan entry (real pass): the consuming GroupNorm's parameters, its coefficient slot, B
    // fresh tickets and the other half of a concatenation; the launcher adds the arrival count and segment 0 (= this launch's statistics)
    bool fill_tail(int prod, int B, GNTail& g) {
        const TailPlan* t = tail_of(prod);
        if (!t) return false;
        t->drawn = true;
        g.gamma = t->gamma; g.beta = t->beta; g.eps = t->eps;
        g.film = t->film_off >= 0 ? film_base + t->film_off : nullptr; g.film_ld = g.film ? film_ld : 0;
        g.coef = (float*)(pool_base + t->coef_off); g.ticket = tickets(B);
        g.C = t->C; g.groups = 32; g.HW = t->HW;
        if (t->two) { g.st1 = (const float*)(pool_base + t->st2_off); g.S1 = t->st2S; g.ld1 = t->st2ld; }
        return true;
    }
    bool used_split = false;   // a split-storage tensor was allocated: the call needs the split weights (checked after the dry run)
    View T(int B, int H, int W, int C, int dt) {
        if (dt == RS_F16S) used_split = true;
        View v; v.B = B; v.H = H; v.W = W; v.C = C; v.ld = C; v.dt = dt;
        v.p = arena->alloc((size_t)B * H * W * C * rs_dtype_size(dt));
        return v;
    }
    void* raw(size_t bytes) { return arena->alloc(bytes); }
    size_t mark() const { return arena->off; }
    // Debug trace (rs_debug_enable): a record copies the view, on the pass's stream and at the point of the graph where it is recorded, into
    // the trace's own capture region as dense fp32 NCHW.  The region is sized by the dry pass and lives outside the scratch arena, the
    // coefficient pool and the tickets, so a traced pass runs exactly the kernels, parameters and scratch layout of an untraced one; the
    // copies are counted in trace_copies, not in `launches`.  A fused path has no record for a tensor it never stores.
    bool tracing = false;
    std::vector<TraceRec>* trace = nullptr;
    char* cap_base = nullptr; size_t cap_off = 0; long long trace_copies = 0;
    std::string prefix;
    // a block's records go under "<enclosing prefix><name>."; the enclosing prefix comes back when the scope ends, so scopes nest
    struct Scope {
        Exec& ex; size_t keep;
        Scope(Exec& e, const std::string& name) : ex(e), keep(e.prefix.size()) { ex.prefix += name + "."; }
        Scope(const Scope&) = delete;
        ~Scope() { ex.prefix.resize(keep); }
    };
    Scope scope(const std::string& name) { return Scope(*this, name); }
    void reset(size_t m) { arena->off = m; }
    void tr(const std::string& name, const View& v) {
        if (!tracing) return;
        cap_off = (cap_off + 255) & ~(size_t)255;
        const size_t o = cap_off;
        cap_off += (size_t)v.B * v.C * v.H * v.W * sizeof(float);
        if (dry) return;
        trace->push_back(TraceRec{prefix + name, v.B, v.C, v.H, v.W, o});
        ++trace_copies;
        const int rc = rs_nhwc_to_nchw_launch(v.p, v.dt, (float*)(cap_base + o), v.B, v.C, v.H * v.W, v.ld, 0, st);
        if (rc != 0) fail(rc, "launch failed: debug trace copy of " + prefix + name);
    }
    // the first error of a pass wins: its code and its text
    void fail(int rc, const std::string& text) {
        if (err) return;
        err = rc; rs_set_last_error(text.c_str(), rc);
    }
    void check(int rc, const char* what) {
        ++launches;
        if (rc != 0) fail(rc, std::string("launch failed: ") + what);
    }
    // MFMA implicit-GEMM launches are the roofline-relevant kernel family: count their algorithmic FLOPs
    // (2*M*N*K per batch entry, K = taps*Cin as in the usual conv FLOP count) and, when profiling is on, bracket
    // every launch with hipEvents on the launch stream.
    struct Prof { bool on = false; std::vector<hipEvent_t> ev; size_t used = 0; } * prof = nullptr, *prof_gn = nullptr;
    double gn_bytes = 0.0;               // algorithmic HBM bytes of the GroupNorm family: input read once + output written once
    long long gn_launches = 0;
    // event pair of one bracketed launch (null pair when profiling is off)
    static void bracket(Prof* pr, hipStream_t st, hipEvent_t& e0, hipEvent_t& e1) {
        e0 = e1 = nullptr;
        if (!pr || !pr->on) return;
        if (pr->used + 2 > pr->ev.size()) {
            const size_t old = pr->ev.size();
            pr->ev.resize(old + 1024);
            for (size_t i = old; i < pr->ev.size(); ++i) (void)hipEventCreate(&pr->ev[i]);
        }
        e0 = pr->ev[pr->used++]; e1 = pr->ev[pr->used++];
        (void)hipEventRecord(e0, st);
    }
    double igemm_flops[3] = {0.0, 0.0, 0.0};  // per input precision (fp16, fp32, split)
    double igemm_bytes = 0.0;            // algorithmic (compulsory) HBM bytes: source tensor + weights + output (+ residual), once each
    long long igemm_launches = 0;
    // per kernel family of the MFMA path (rs_profile_families): algorithmic FLOPs, launches, and the family of every bracket
    enum Fam { F_HALO16 = 0, F_HALO_SPLIT, F_IGEMM16, F_IGEMM_SPLIT, F_IGEMM32, F_WINATTN, F_SWINMLP, F_WINATTN_S, F_SWINMLP_S, F_AEFLASH, F_AEFLASH_S, F_WINO_S, F_COUNT };
    double fam_flops[F_COUNT] = {};
    long long fam_launches[F_COUNT] = {};
    std::vector<unsigned char> fam_of;   // family of bracket k (profiling pass only)
    // RS_PROF_SHAPES=1 (debugging aid): the profiling pass also keeps one "family M N K" tag per bracket and the engine prints
    // the time per distinct shape to stderr
    std::vector<std::string> tag_of;
    std::vector<double> tag_flops;
    // which network the launches belong to (rs_profile_shapes: "encoder" / "unet" / "decoder") and, profiling passes only, an event at every
    // change of part: the wall time of the parts between them (every kernel, not just the bracketed MFMA family)
    const char* part = "";
    std::vector<std::pair<std::string, hipEvent_t>> part_marks;
    void enter_part(const char* name) {
        part = name;
        if (dry || !prof || !prof->on) return;
        hipEvent_t ev = nullptr;
        if (hipEventCreate(&ev) != hipSuccess) return;
        (void)hipEventRecord(ev, st);
        part_marks.emplace_back(name, ev);
    }
    void fam_note(int f, double flops, long long M = 0, int N = 0, int K = 0, int nz = 1) {
        fam_flops[f] += flops; ++fam_launches[f];
        if (prof && prof->on) {
            fam_of.push_back((unsigned char)f);
            char b[128]; snprintf(b, sizeof b, "%s f%d M=%lld N=%d K=%d z=%d", part, f, M, N, K, nz);
            tag_of.emplace_back(b); tag_flops.push_back(flops);
        }
    }
    // One bracketed launch (gn(): prof_gn; the MFMA family: mfma()): the event pair, `launch()` - its launcher's 0 / error code - checked, the closing event
    template <class L> void bracketed(Prof* pr, const char* what, L launch) {
        hipEvent_t e0, e1;
        bracket(pr, st, e0, e1);
        check(launch(), what);
        if (e1) (void)hipEventRecord(e1, st);
    }
    // ... of the MFMA family: books `flops` under the input precision (slot 0 fp16, 1 fp32, 2 split), `fam_flops` + the shape tag under family `fam`, the bytes
    struct MfmaNote { int slot, fam; double flops, fam_flops, bytes; long long M; int N, K, nz; };
    template <class L> void mfma(const MfmaNote& n, const char* what, L launch) {
        igemm_flops[n.slot] += n.flops;
        fam_note(n.fam, n.fam_flops, n.M, n.N, n.K, n.nz);
        igemm_bytes += n.bytes;
        ++igemm_launches;
        bracketed(prof, what, launch);
    }
    // (`pl`: the launch's plan, made once by the caller - the family it is booked under, the reduce launch of its split-K slices)
    void igemm(const IGemmParams& p, const ConvPlan& pl, int in_dt, int out_dt, int nz, const char* what) {
        const int Kall = p.Ktot + p.sC;   // (+ the K columns of a folded 1x1 shortcut)
        const double fl = 2.0 * (double)p.M * (double)p.Cout * (double)Kall * (double)nz;
        const bool halo = pl.kernel == CK_HALO || pl.kernel == CK_HALO_SEG;
        const int f = pl.kernel == CK_WINO ? F_WINO_S : (in_dt == RS_F16 ? (halo ? F_HALO16 : F_IGEMM16) : (in_dt == RS_F16S ? (halo ? F_HALO_SPLIT : F_IGEMM_SPLIT) : F_IGEMM32));
        const double isz = in_dt == RS_F16 ? 2.0 : 4.0, osz = out_dt == RS_F16 ? 2.0 : 4.0;
        const double src = (double)p.B * p.Hs * p.Ws * (double)(p.C0 + p.C1 + p.sC) * isz;
        const double out = (double)p.M * p.Cout * osz;
        mfma({in_dt == RS_F16 ? 0 : (in_dt == RS_F16S ? 2 : 1), f, fl, fl, (double)nz * (src + (double)p.Cout * Kall * isz + out + (p.res ? out : 0.0)), p.M, p.Cout, Kall, nz},
             what, [&] { return rs_conv_launch(&p, in_dt, out_dt, nz, &pl, st); });
        if (pl.splitk > 1) ++launches;   // (the slices' reduce kernel)
    }
    // fused qkv projection + window attention: the projection's FLOPs / compulsory bytes stay in the MFMA-family bookkeeping
    void win_attn_qkv(const WinAttnParams& p, int E, int dt = RS_F16) {
        const double M = (double)p.B * p.H * p.W;
        const int sp = dt == RS_F16S;
        const double fl = 2.0 * M * (p.wproj ? 4.0 : 3.0) * E * E;
        mfma({sp ? 2 : 0, sp ? F_WINATTN_S : F_WINATTN, fl, 2.0 * M * (p.wproj ? 4.0 : 3.0) * E * E + 2.0 * 2.0 * M * 64.0 * E,   // + QK^T and PV of the 64-token windows
              (sp ? 4.0 : 2.0) * (M * E * (p.res ? 3.0 : 2.0) + (p.wproj ? 4.0 : 3.0) * E * E), (long long)M, E, E, 1}, sp ? "win_attn_qkv_split" : "win_attn_qkv",
             [&] { return sp ? rs_win_attn_qkv_split_launch(&p, st) : rs_win_attn_qkv_launch(&p, st); });
    }
    // streaming AE attention (ae_attn.hip): QK^T and PV of nz images, q / k / v^T read once, o written once
    void ae_flash(const AeFlashCall& c, int dt) {
        const int sp = dt == RS_F16S;
        const double fl = 4.0 * (double)c.nz * (double)c.T * (double)c.T * (double)c.C;
        mfma({sp ? 2 : 0, sp ? F_AEFLASH_S : F_AEFLASH, fl, fl, (sp ? 4.0 : 2.0) * 4.0 * (double)c.nz * c.T * c.C, c.T, c.T, c.C, c.nz},
             sp ? "ae_flash_attn_split" : "ae_flash_attn", [&] { return sp ? rs_ae_flash_split_launch(&c, st) : rs_ae_flash_launch(&c, st); });
    }
    // the fused Swin MLP belongs to the same MFMA family for the roofline bookkeeping: both GEMMs' FLOPs, compulsory bytes
    void swin_mlp(const SwinMlpCall& c, int dt) {
        const int sp = dt == RS_F16S, M = c.M, E = c.E, HD = c.HD;
        const int NO = c.NO <= 0 ? E : c.NO;   // (NO != E: patch_unembed folded in - fc1, then the product matrix over [h ; x])
        const double fl = 2.0 * (double)M * ((double)E * HD + (double)NO * (NO != E ? HD + E : HD));
        mfma({sp ? 2 : 0, sp ? F_SWINMLP_S : F_SWINMLP, fl, fl,
              (sp ? 4.0 : 2.0) * ((double)M * (E * ((c.res || NO != E) ? 2.0 : 1.0) + NO) + (double)E * HD + (double)NO * (NO != E ? HD + E : HD)), M, NO, HD, 1},
             sp ? "swin_mlp_split" : "swin_mlp", [&] { return sp ? rs_swin_mlp_split_launch(&c, st) : rs_swin_mlp_launch(&c, st); });
    }
};

// One convolution of the graph, one value from plan to launch: the layer's weights, its views, the geometry, what the launch fuses in, and the
// ConvPlan made from exactly these fields (rs_conv_plan: the kernel, its split-K factor, the statistics it can leave).  Every field that feeds
// the plan is private and changes only through a setter that drops the plan; plan() makes it again on demand, so want_stats(), fuses_gn(),
// Graphs::skip_fold(), Graphs::gn_silu_conv3() and launch() all see the one plan of the arguments that are launched, made once.  The dry and
// the real pass get the same plan: it depends on the layout only.
class ConvCall {
    const ConvW* w_;
    bool big_;                            // |w| >= 30 (Model::big): no 2^11 scaling of the hi fragment - the generic split kernel takes it
    View x_, y_, x1_, res_, skx_;         // (x1_ / res_ / skx_ count only with two_ / has_res_ / skw_: a dry pass's pointers are all null)
    bool two_ = false, has_res_ = false;
    const ConvW* skw_ = nullptr;          // folded 1x1 shortcut (IGemmParams::sx) over the block input skx_
    int stride_ = 1, pad_t_, pad_l_, up_ = 1, act_ = 0;
    int osc_ = 0, ooy_ = 0, oox_ = 0;     // the scattered rows of the sub-pixel form (IGemmParams::osc)
    // what only the launch reads: no part of the plan, free to set at any time
    float out_scale_ = 1.f;
    const float* xcoef_ = nullptr; int xact_ = RS_ACT_NONE;
    mutable ConvPlan plan_{}; mutable bool planned_ = false;
    ConvCall& replan() { planned_ = false; return *this; }
    int rows() const { return osc_ == 2 ? y_.H / 2 : y_.H; }   // the grid a launch computes: the low-resolution one of the sub-pixel form
    int cols() const { return osc_ == 2 ? y_.W / 2 : y_.W; }

public:
    // the layer's KH x KW taps at stride 1 with `pad` zeros on every side (Graphs::k3 / k1)
    ConvCall(const ConvW& w, bool big, const View& x, const View& y, int pad) : w_(&w), big_(big), x_(x), y_(y), pad_t_(pad), pad_l_(pad) {}
    // stride s with `pad` zeros above and to the left (below / right: whatever the output size implies - F.pad(x,(0,1,0,1)) + pad 0 is pad = 0)
    ConvCall& strided(int s, int pad) { stride_ = s; pad_t_ = pad_l_ = pad; return replan(); }
    ConvCall& upsampled() { up_ = 2; return replan(); }   // nearest x2 folded into the conv's addressing
    ConvCall& act(int a) { act_ = a; return replan(); }
    ConvCall& source(const View& x) { x_ = x; two_ = false; return replan(); }
    ConvCall& second_source(const View& x1) { x1_ = x1; two_ = true; return replan(); }   // channels concatenated after x
    ConvCall& residual(const View& r) { res_ = r; has_res_ = true; return replan(); }
    ConvCall& shortcut(const ConvW& skw, const View& skx) { skw_ = &skw; skx_ = skx; return replan(); }
    ConvCall& no_shortcut() { skw_ = nullptr; return replan(); }
    // class (py, px) of the sub-pixel form of "nearest x2 + conv3x3": a 2x2 conv over the low-resolution grid whose rows go to the pixels of that parity
    ConvCall& subpixel(int py, int px) { osc_ = 2; ooy_ = py; oox_ = px; pad_t_ = 1 - py; pad_l_ = 1 - px; return replan(); }
    // ... and another class of the same form: its weights and parity, and THIS call's plan - the four launches have one shape
    ConvCall sibling(const ConvW& w, int py, int px) const {
        (void)plan();
        ConvCall c = *this;
        c.w_ = &w; c.ooy_ = py; c.oox_ = px; c.pad_t_ = 1 - py; c.pad_l_ = 1 - px;
        return c;
    }
    ConvCall& out_scale(float s) { out_scale_ = s; return *this; }
    // act(x * coef[b][0][c] + coef[b][1][c]) is what the conv sees (halo and Winograd kernels: fuses_gn())
    ConvCall& input_transform(const float* coef, int act) { xcoef_ = coef; xact_ = act; return *this; }

    const View& x() const { return x_; }
    const View& y() const { return y_; }   // (after want_stats(): with the statistics buffer the launch fills)
    const View& shortcut_x() const { return skx_; }
    bool has_shortcut() const { return skw_ != nullptr; }

    // THE place that turns the call into the parameter block of an implicit-GEMM launch, for the planner and for launch() (which adds the
    // split-K slabs, the statistics and the tail: state of the pass, not of the call)
    IGemmParams params() const {
        const ConvW& w = *w_;
        const int C1 = two_ ? x1_.C : 0;
        IGemmParams p{};
        p.x0 = x_.p; p.x1 = two_ ? x1_.p : nullptr; p.w = w.w_for(x_.dt); p.bias = w.bias;
        p.res = has_res_ ? res_.p : nullptr; p.y = y_.p;
        p.C0 = x_.C; p.C1 = C1; p.ld0 = x_.ld; p.ld1 = two_ ? x1_.ld : 0;
        p.B = x_.B; p.Hs = x_.H; p.Ws = x_.W; p.up = up_; p.Ho = rows(); p.Wo = cols(); p.KH = w.KH; p.KW = w.KW;
        p.stride = stride_; p.pad_t = pad_t_; p.pad_l = pad_l_; p.Cout = w.Cout; p.ldy = y_.ld; p.ldres = has_res_ ? res_.ld : 0;
        p.M = y_.B * rows() * cols(); p.Ktot = w.KH * w.KW * (x_.C + C1); p.act = act_; p.out_scale = out_scale_;
        p.splitk = 1;
        p.ww = (x_.dt == RS_F16S && !two_) ? w.ww : nullptr;
        p.unscaled_w = (x_.dt == RS_F16S && big_) ? 1 : 0;
        p.xcoef = xcoef_; p.xact = xact_;
        if (skw_) { p.sx = skx_.p; p.sw = skw_->w_for(x_.dt); p.sbias = skw_->bias; p.sC = skx_.C; p.sld = skx_.ld; }
        p.osc = osc_; p.ooy = ooy_; p.oox = oox_;
        return p;
    }
    const ConvPlan& plan() const {
        if (planned_) return plan_;
        plan_ = ConvPlan{};   // (CK_NONE: the direct kernel, or a launch that launch() refuses)
        planned_ = true;
        if (w_->direct || x_.C + (two_ ? x1_.C : 0) != w_->CinP) return plan_;
        const IGemmParams p = params();
        (void)rs_conv_plan(&p, x_.dt, y_.dt, 1, &plan_);
        return plan_;
    }
    // the conv can apply a GroupNorm affine + SiLU to its input while the tile sits in LDS
    bool fuses_gn() const { const int k = plan().kernel; return k == CK_WINO || k == CK_HALO || k == CK_HALO_SEG; }
    // Attach a statistics buffer to the output IF the planned kernel can leave them: the halo kernel (one partial set per 256- or 128-pixel
    // tile of one image), the generic split-storage kernel (RS_GN_GEN_STATS, default on: one set per 128- / 64-pixel tile), or - split-K
    // launches of either - the reduce kernel (slabs of 256 pixels / the whole small image).  The sub-pixel form: the generic split kernel
    // only, one slab per low-resolution pixel tile and parity class.  The buffer lives in the coefficient pool (reset per network body), so
    // a block's output may carry it to whoever consumes it later (the next block, the decoder's concatenation).
    void want_stats(Exec& ex) {
        const ConvPlan& pl = plan();
        const bool sub = osc_ == 2;
        const int HW = rows() * cols(), spx = pl.stats_px;
        y_.drop_stats();
        if (!rs_knob_gn_epi_stats() || (pl.kernel == CK_SPLIT && !rs_knob_gn_gen_stats()) || (sub && pl.kernel != CK_SPLIT) || spx <= 0 || (HW % spx)) return;
        ex.attach_stats(y_, (sub ? 4 : 1) * (HW / spx), y_.C);
    }
    // The planned kernel's per-operand size limit (RS_BUFFER_BYTES_LIMIT): true, with Exec::fail, when an operand of this call reaches it.
    // Every planned conv passes here in the dry pass (launch(); Graphs::upfold for its four launches), so the call ends before any launch.
    bool oversize(Exec& ex) const {
        const ConvW& w = *w_;
        const int C1 = two_ ? x1_.C : 0;
        if (w.direct || x_.C + C1 != w.CinP) return false;
        std::string text;
        const IGemmParams p = params();
        if (!rs_conv_operand_over(std::string(), p, x_.dt, plan(), &text)) return false;   // (the layer's name is put together only for a refusal)
        const std::string layer = ex.prefix + "conv " + std::to_string(w.KH) + "x" + std::to_string(w.KW) + " " + std::to_string(x_.C + C1) + "->" + std::to_string(w.Cout);
        (void)rs_conv_operand_over(layer, p, x_.dt, plan(), &text);
        ex.fail(RS_ERR_OPERAND_BYTES, text);
        return true;
    }
    // `shared`: the tail of a group of launches that fill ONE statistics buffer (the sub-pixel form); null: this launch draws its own
    void launch(Exec& ex, const GNTail* shared = nullptr) const {
        const ConvW& w = *w_;
        const int C1 = two_ ? x1_.C : 0;
        // split storage has no two-source implicit GEMM: gather the channel concatenation once (only the first conv of the
        // feature-extractor configs, unet.py:882)
        if (!w.direct && two_ && x_.dt == RS_F16S) {
            View xcat = ex.T(x_.B, x_.H, x_.W, x_.C + C1, x_.dt);
            if (!ex.dry) {
                ex.check(rs_copy_channels_launch(x_.p, x_.ld, xcat.p, xcat.ld, x_.C, x_.pixels(), x_.dt, ex.st), "concat copy");
                ex.check(rs_copy_channels_launch(x1_.p, x1_.ld, xcat.slice(x_.C, C1).p, xcat.ld, C1, x_.pixels(), x_.dt, ex.st), "concat copy");
            }
            // the gathered tensor is another layout with another plan: what was decided on the two-source plan does not carry over (statistics
            // that the new plan cannot serve are refused by the launch itself)
            if (xcoef_ || skw_) { ex.fail(-3, "two-source conv in split storage cannot take an input transform or a folded shortcut"); return; }
            ConvCall(*this).source(xcat).launch(ex, shared);
            return;
        }
        const ConvPlan& pl = plan();
        // split-K for launches that cannot fill the chip (8x8 / 16x16 UNet levels): fp32 slabs live in the arena
        float* const partial = pl.splitk > 1 ? (float*)ex.raw((size_t)pl.splitk * y_.B * y_.H * y_.W * w.Cout * sizeof(float)) : nullptr;
        if (oversize(ex)) return;   // (both passes: the dry pass ends the call before anything is launched)
        if (ex.dry) return;
        if (x_.C + C1 != w.CinP) { ex.fail(-3, "conv input channels do not match the packed weights"); return; }
        if (w.direct) {
            DirectConvParams p{};
            p.x0 = x_.p; p.x1 = two_ ? x1_.p : nullptr; p.w = w.wd; p.bias = w.bias; p.y = y_.p;
            p.C0 = x_.C; p.C1 = C1; p.ld0 = x_.ld; p.ld1 = two_ ? x1_.ld : 0;
            p.B = x_.B; p.Hs = x_.H; p.Ws = x_.W; p.up = up_; p.Ho = y_.H; p.Wo = y_.W; p.KH = w.KH; p.KW = w.KW;
            p.stride = stride_; p.pad_t = pad_t_; p.pad_l = pad_l_; p.Cout = w.Cout; p.ldy = y_.ld; p.act = act_;
            if (has_res_) { ex.fail(-3, "direct conv has no residual path"); return; }
            ex.check(rs_direct_conv_launch(&p, x_.dt, y_.dt, ex.st), "direct_conv");
            return;
        }
        IGemmParams p = params();
        p.partial = partial;
        if (y_.st) {   // statistics for the consuming GroupNorm: the kernel's epilogue or its split-K reduce (want_stats() asked the same plan)
            if (!pl.stats_px) { ex.fail(-3, "output statistics requested from a conv whose kernel cannot produce them"); return; }
            p.ystats = y_.st; p.ystats_ld = y_.stld;
            if (shared) p.tail = *shared;
            else (void)ex.fill_tail(y_.st_prod, y_.B, p.tail);   // ... and that GroupNorm's coefficients too (gn_tail.h)
        }
        if (!p.w) { ex.fail(-3, "weights for this precision were not packed (enable_f16/enable_f32/enable_split)"); return; }
        ex.igemm(p, pl, x_.dt, y_.dt, 1, "igemm");
    }
};

// The graphs themselves: they read the model and drive an Exec, nothing else
struct Graphs {
    const Model& m;
    // ---------------------------------------------------------------- ops
    ConvCall k3(const ConvW& w, const View& x, const View& y) const { return ConvCall(w, m.big(w), x, y, 1); }   // 3x3 (any KH x KW), pad 1
    ConvCall k1(const ConvW& w, const View& x, const View& y) const { return ConvCall(w, m.big(w), x, y, 0); }   // 1x1 / linear, pad 0
    // a conv whose epilogue also leaves the statistics (+ coefficients) for the GroupNorm that consumes its output: the output view, with them
    View conv_for_gn(Exec& ex, ConvCall c, bool stats = true) {
        if (stats) c.want_stats(ex);
        c.launch(ex);
        return c.y();
    }
    // the four launches of the sub-pixel form: x [B,H,W,C] -> y [B,2H,2W,C].  Taken when the low-resolution grid alone fills the chip
    // (the 8 x 8 -> 16 x 16 and 16 x 16 -> 32 x 32 steps at batch 32 do not: they keep the folded-address form).
    bool upfold_ok(const ConvW (&upf)[4], const View& x, const View& y) const {
        if (x.dt != y.dt || (x.dt != RS_F16 && x.dt != RS_F16S) || y.H != 2 * x.H || y.W != 2 * x.W || x.C != upf[0].CinP) return false;
        if (!upf[0].w_for(x.dt) || (x.ld % 8) || (y.ld % 8)) return false;   // (the scattered-row launches' alignment preconditions)
        // (measured, profiles/r5_upfold_ab.txt: with the 16 -> 32 and 8 -> 16 steps as well - 8192 / 2048 low-resolution pixels at batch 32, four
        // launches that cannot fill the chip each - the pass is 0.9 ms slower than with the 32 -> 64 step alone)
        return (long long)x.B * x.H * x.W >= 16384;
    }
    // ... as four calls that share class 0's plan, ONE statistics buffer and ONE tail (one ticket per image); returns y (with the statistics)
    View upfold(Exec& ex, const ConvW (&upf)[4], const View& x, const View& y, bool stats) {
        ConvCall c0 = k3(upf[0], x, y).subpixel(0, 0);
        if (stats) c0.want_stats(ex);
        if (c0.oversize(ex) || ex.dry) return c0.y();   // (the four launches share x, the weights' size and the plan)
        GNTail tl{};
        if (c0.y().st) (void)ex.fill_tail(c0.y().st_prod, y.B, tl);
        for (int q = 0; q < 4; ++q) c0.sibling(upf[q], q >> 1, q & 1).launch(ex, &tl);
        return c0.y();
    }
    void zero(Exec& ex, const View& v) {
        if (ex.dry) return;
        const hipError_t e = hipMemsetAsync(v.p, 0, (size_t)v.B * v.H * v.W * v.ld * rs_dtype_size(v.dt), ex.st);
        ex.check(e == hipSuccess ? 0 : -1, "memset");
    }
    // A ResBlock's 1x1 shortcut (models/unet.py:178-183,205-206; ldm/modules/diffusionmodules/model.py:121-127,148-149) as extra K columns
    // of its second 3x3 conv (IGemmParams::sx) instead of a GEMM launch + a tensor + a residual read: split storage on the halo kernel's
    // 8-wave big-plane tiles, whole 32-channel chunks of the block input, no weight that needs the unscaled path.  RS_SKIP_FOLD=0: off.
    // `c2`: conv2 WITH the shortcut in it.
    bool skip_fold(const ResBlockW& r, const ConvCall& c2) const {
        static const bool on = rs_env_on("RS_SKIP_FOLD");
        static const bool on16 = rs_env_on("RS_SKIP_FOLD_F16");   // (fp16 storage: the decoder's nin_shortcuts, the fp16 policy's UNet)
        const View &X = c2.shortcut_x(), &Y = c2.y();
        if (!on || !rs_knob_gn_conv_fold() || !r.has_skip || (X.dt != RS_F16S && !(X.dt == RS_F16 && on16)) || Y.dt != X.dt) return false;
        if (X.dt == RS_F16S && (m.big(r.skip) || m.big(r.c2))) return false;
        if (!r.skip.w_for(X.dt) || r.skip.KH != 1 || X.C != r.skip.CinP || (X.C % 32) || (X.ld % 8) || X.H != Y.H || X.W != Y.W) return false;
        return c2.plan().kernel == CK_HALO;   // (the HALO kernel's big-plane tiles, no split-K: the fold - a GEMM launch saved - beats the Winograd kernel's 10 %)
    }
    // GroupNorm (+FiLM) + SiLU + 3x3 conv (models/unet.py:128-147,198-203; ldm/modules/diffusionmodules/model.py:129-147): on the
    // halo kernel the GroupNorm only produces per-(image, channel) affine coefficients and the conv applies them to the RAW tensor
    // in LDS (bit-identical to normalising first); otherwise normalise into a scratch tensor and convolve that
    void gn_silu_conv3(Exec& ex, ConvCall& c, const GNW& g, float eps, const float* film) {
        if (rs_knob_gn_conv_fold() && c.fuses_gn()) {
            c.input_transform(gn_coef(ex, g, c.x(), eps, film), RS_ACT_SILU).launch(ex);
            return;
        }
        if (c.has_shortcut()) { ex.fail(-3, "folded shortcut planned for a conv that does not run on the halo kernel"); return; }
        const View X = c.x();
        View t = ex.T(X.B, X.H, X.W, X.C, X.dt);
        gn(ex, g, X, t, eps, RS_ACT_SILU, film);
        c.source(t).launch(ex);   // (another launch - the dense scratch tensor is its input: planned again)
    }
    // GroupNorm + SiLU + conv3x3 to <= 4 channels (the UNet's `out`, Encoder / Decoder norm_out + conv_out) -> fp32 NHWC `o`: one fused pass
    // (gn_silu_head_conv_kernel) over the raw tensor with the GroupNorm as coefficients; RS_HEAD_FUSED=0: normalise, then
    // the implicit-GEMM conv (the round-3 path)
    void head(Exec& ex, const GNW& g, const ConvW& w, const View& X, const View& o, float eps) {
        static const bool fused = rs_env_on("RS_HEAD_FUSED");
        if (fused && w.wd && !w.direct && o.dt == RS_F32 && X.C == w.Cin && (X.C % 8) == 0 && (X.ld % 8) == 0 && w.Cout <= 4) {
            const float* coef = gn_coef(ex, g, X, eps, nullptr);
            if (!ex.dry) ex.check(rs_head_conv_launch(X.p, X.dt, coef, w.wd, w.bias, (float*)o.p, X.B, X.H, X.W, X.C, X.ld, w.Cout, o.ld, ex.st), "head conv");
            return;
        }
        const size_t mk = ex.mark();
        View t = ex.T(X.B, X.H, X.W, X.C, X.dt);
        gn(ex, g, X, t, eps, RS_ACT_SILU);
        k3(w, t, o).launch(ex);
        ex.reset(mk);
    }
    // The per-(image, channel) affine [B][2][C] of a GroupNorm whose consumer applies it while loading x (halo conv, fused Swin kernels).
    // Three ways to get it, cheapest first: the launch that produced x's statistics wrote it already (tail, planned by the dry pass);
    // ONE statistics launch whose last workgroup per image writes it (x has no producer statistics); or the coefficient kernel over the
    // producer's partials (RS_GN_TAIL=0, or a producer that is claimed by another GroupNorm).
    const float* gn_coef(Exec& ex, const GNW& g, const View& x, float eps, const float* film) {
        static const bool tails = rs_env_on("RS_GN_TAIL");
        float* coef = ex.pool((size_t)x.B * 2 * x.C * sizeof(float));
        const int me = ex.gn_seq++;
        if (tails && x.st && x.st_prod >= 0 && ex.plan && x.C <= 1280) {
            std::vector<TailPlan>& pl = *ex.plan;
            if (ex.dry) {
                if ((int)pl.size() <= x.st_prod) pl.resize(x.st_prod + 1);
                TailPlan& t = pl[x.st_prod];
                if (!t.on) {
                    t.on = true; t.consumer = me; t.gamma = g.gamma; t.beta = g.beta; t.film_off = film ? (long long)(film - ex.film_base) : -1; t.eps = eps; t.C = x.C; t.HW = x.H * x.W;
                    t.coef_off = (size_t)((char*)coef - ex.pool_base);
                    if (x.st2) { t.two = true; t.st2_off = (size_t)((char*)x.st2 - ex.pool_base); t.st2S = x.st2S; t.st2ld = x.st2ld; }
                    ex.ticket_used += (size_t)x.B;   // (drawn by the producer's launch in the real pass)
                }
            }
            const TailPlan* t = ex.tail_of(x.st_prod);
            if (t && t->consumer == me) return coef;   // written by the producer's tail: nothing to launch
        }
        gn(ex, g, x, x, eps, RS_ACT_NONE, film, coef);
        return coef;
    }
    // `coef` non-null: statistics + affine coefficients only ([B][2][C] floats), y is not written (fused consumer kernels)
    void gn(Exec& ex, const GNW& g, const View& x, const View& y, float eps, int act, const float* film = nullptr, float* coef = nullptr) {
        const int HW = x.H * x.W;
        // slab counts: enough workgroups to fill the chip, but every apply workgroup re-derives the per-channel
        // coefficients, so slabs must stay fat enough to amortise that (RS_GN_BLOCKS_* override the targets for tuning)
        static const int tgt1 = (int)rs_env_int("RS_GN_BLOCKS_STATS", 1024);
        static const int tgt2 = (int)rs_env_int("RS_GN_BLOCKS_APPLY", 2048);
        static const int minpx = (int)rs_env_int("RS_GN_MIN_PIXELS", 8);
        int S = std::max(1, std::min(64, tgt1 / std::max(1, x.B)));
        S = std::max(1, std::min(S, HW / minpx));
        int S2 = std::max(1, std::min(HW / minpx, std::max(1, tgt2 / std::max(1, x.B))));
        float* partial = (float*)ex.raw((size_t)x.B * S * 32 * 2 * sizeof(float));
        // coefficient-only without producer statistics: one launch, the statistics kernel's last workgroup per image finishes (gn_tail.h)
        const bool have_cp = x.st != nullptr;   // per-channel partials from the producer(s): no statistics pass
        unsigned* ticket = (coef && !have_cp && HW > 256) ? ex.tickets(x.B) : nullptr;
        if (ex.dry) return;
        GNParams p{};
        p.ticket = ticket;
        p.x = x.p; p.y = y.p; p.gamma = g.gamma; p.beta = g.beta; p.film = film; p.film_ld = film ? ex.film_ld : 0; p.partial = partial;
        p.B = x.B; p.HW = HW; p.C = x.C; p.ldx = x.ld; p.ldy = y.ld; p.S = S; p.groups = 32; p.eps = eps; p.act = act; p.coef = coef;
        if (x.st) { p.cpartial = x.st; p.cp_ld = x.stld; p.S = x.stS; }   // per-channel partials from the producing conv: no statistics pass
        if (x.st && x.st2) { p.cpartial2 = x.st2; p.cp2_ld = x.st2ld; p.cp2_S = x.st2S; p.cp_n0 = x.st_n0; }   // ... of both halves of a concatenation
        // algorithmic bytes: normalise = read once + write once; coefficients only = read once, or nothing when the statistics
        // come from the producing conv's epilogue
        ex.gn_bytes += (double)x.B * HW * x.C * (double)rs_dtype_size(x.dt) * (coef ? (have_cp ? 0.0 : 1.0) : 2.0);
        ++ex.gn_launches;
        ex.bracketed(ex.prof_gn, "groupnorm", [&] {
            const int nk = rs_groupnorm_launch(&p, x.dt, S2, ex.st);   // number of kernels launched, or < 0
            if (nk > 1) ex.launches += nk - 1;
            return nk < 0 ? nk : 0;
        });
    }
    // models/unet.py:186-206 (use_scale_shift_norm path); eps 1e-5 (basic_ops.py:96 default GroupNorm eps)
    // `out_stats`: conv2's epilogue also leaves the statistics (and, when the dry pass planned it, the coefficients) for the GroupNorm that
    // consumes Y - the next block's in_layers[0], possibly through the decoder's concatenation
    void resblock(Exec& ex, const ResBlockW& r, const View& X, View& Y, const float* film_row, bool out_stats = true, float eps = 1e-5f) {
        const size_t mk = ex.mark();
        View h1 = ex.T(X.B, X.H, X.W, r.Cout, X.dt);
        ConvCall c1 = k3(r.c1, X, h1);
        c1.want_stats(ex);   // conv1's epilogue leaves the statistics norm2 needs
        gn_silu_conv3(ex, c1, r.n1, eps, nullptr);
        h1 = c1.y();
        ex.tr("conv1", h1);
        const float* film = film_row ? film_row + r.film_off : nullptr;
        // the shortcut: folded into conv2 (skip_fold()), a 1x1 conv whose output conv2 adds, or the block input itself
        ConvCall c2 = k3(r.c2, h1, Y);
        if (!r.has_skip) c2.residual(X);
        else if (!skip_fold(r, c2.shortcut(r.skip, X))) {
            View sk = ex.T(X.B, X.H, X.W, r.Cout, X.dt);
            k1(r.skip, X, sk).launch(ex);
            c2.no_shortcut().residual(sk);
        }
        if (out_stats) c2.want_stats(ex);
        gn_silu_conv3(ex, c2, r.n2, eps, film);
        Y = c2.y();
        ex.reset(mk);
    }
    // ldm/modules/diffusionmodules/model.py:129-149 (temb=None), GroupNorm eps 1e-6 (model.py:46-47)
    void resnet(Exec& ex, const ResBlockW& r, const View& X, View& Y, bool out_stats = true) { resblock(ex, r, X, Y, nullptr, out_stats, 1e-6f); }
    // models/swin_transformer.py:427-442 with the two SwinTransformerBlocks (:238-281) inlined
    void basiclayer(Exec& ex, const BasicLayerW& b, const View& X, View& Y, bool out_stats = true) {
        const size_t mk = ex.mark();
        const int E = b.E, heads = m.cfg.unet.num_heads;
        View e = ex.T(X.B, X.H, X.W, E, X.dt);
        e = conv_for_gn(ex, k1(b.embed, X, e));   // patch_embed's epilogue: statistics (+ coefficients) for the first block's norm1
        ex.tr("embed", e);
        int bi = 0;
        for (const SwinBlockW& s : b.blocks) {
            const std::string bp = "blk" + std::to_string(bi++) + ".";
            // fp16 storage: qkv projection fused into the attention kernel (the [M][3E] tensor never reaches HBM); RS_ATTN_FUSED=0
            // keeps the two launches.  RS_GN_FOLD (default on): the fused consumer kernels
            // also apply the GroupNorm affine while they load their input, so norm1 / norm2 only produce [B][2][E] coefficients.
            static const int attn_fused = (int)rs_env_int("RS_ATTN_FUSED", 2);
            static const int gn_fold = (int)rs_env_int("RS_GN_FOLD", 1);
            // split storage: the same fusion in win_attn_split.hip (RS_ATTN_FUSED_SPLIT=0: separate qkv GEMM, attention, projection GEMM)
            static const int attn_fused_split = (int)rs_env_int("RS_ATTN_FUSED_SPLIT", 1);
            const bool big_attn = X.dt == RS_F16S && (m.big(s.qkv) || m.big(s.proj)), big_mlp = X.dt == RS_F16S && (m.big(s.fc1) || m.big(s.fc2));   // (|w| >= 30: unfused path)
            const bool fuse_qkv = rs_win_attn_qkv_supported(heads, E) && s.bias_n && !big_attn &&
                                  ((attn_fused && X.dt == RS_F16 && s.qkv.wh_frag) || (attn_fused_split && X.dt == RS_F16S && s.qkv.ws_frag && s.proj.ws_frag));
            const bool fold1 = fuse_qkv && gn_fold;
            View n;
            const float* coef1 = nullptr;
            if (fold1) coef1 = gn_coef(ex, s.n1, e, 1e-5f, nullptr);
            else { n = ex.T(X.B, X.H, X.W, E, X.dt); gn(ex, s.n1, e, n, 1e-5f, RS_ACT_NONE); }
            View qkv;
            if (!fuse_qkv) {
                qkv = ex.T(X.B, X.H, X.W, 3 * E, X.dt);
                k1(s.qkv, n, qkv).launch(ex);
                ex.tr(bp + "qkv", qkv);
            }
            const bool fuse_proj = fuse_qkv && (X.dt == RS_F16S || (attn_fused >= 2 && s.proj.wh_frag));   // ... and the output projection + shortcut as well
            View a, e2;
            if (fuse_proj) e2 = ex.T(X.B, X.H, X.W, E, X.dt); else a = ex.T(X.B, X.H, X.W, E, X.dt);
            // fp16 storage: one fused MLP launch, the [M][4E] hidden tensor never reaches HBM (swin_mlp.hip); RS_MLP_FUSED=0 or a
            // small token count (RS_MLP_FUSED_MINM) keep the two GEMMs
            static const int mlp_fused = (int)rs_env_int("RS_MLP_FUSED", 3);   // bit 0: fp16, bit 1: split storage
            static const int mlp_minm = (int)rs_env_int("RS_MLP_FUSED_MINM", 16384);   // (8192 tokens: 32 us fused vs 14 + 15 us apart)
            const int Mtok = X.B * X.H * X.W, HWt = X.H * X.W;
            const bool fuse_mlp = mlp_fused && !big_mlp && (X.dt == RS_F16 || (X.dt == RS_F16S && (mlp_fused & 2))) && rs_swin_mlp_supported(E, s.fc1.Cout) &&
                                  s.fc2.Cout == E && Mtok >= mlp_minm && s.fc1.w_for(X.dt) && s.fc2.w_for(X.dt);
            const bool fold2 = fuse_mlp && gn_fold && HWt % 128 == 0;
            // the fused MLP over input `in` into `out`, with out's statistics (+ tail) if it carries any (real pass); the caller adds fc2's side
            GNTail mlp_tail{};
            auto mlp_call = [&](const View& in, const View& out) {
                SwinMlpCall c{};
                c.x = in.p; c.ldx = in.ld; c.w1 = s.fc1.w_for(X.dt); c.b1 = s.fc1.bias; c.y = out.p; c.ldy = out.ld;
                c.M = Mtok; c.E = E; c.HD = s.fc1.Cout; c.HW = HWt; c.ystats = out.st; c.ystats_ld = out.stld;
                if (out.st && ex.fill_tail(out.st_prod, X.B, mlp_tail)) c.tail = &mlp_tail;
                return c;
            };
            // The fused kernels' epilogues leave the statistics of their outputs for the GroupNorm that reads them (attention -> norm2: one
            // partial set per window; MLP -> the next block's norm1: one per 128-token tile) and - round 4 - the launch that completes an
            // image's statistics writes that GroupNorm's coefficients (tail): no pass over those tensors, no coefficient launch.
            //   split storage: default on (RS_GN_SWIN_STATS_SPLIT=0: statistics pass + tail as for any tensor without producer statistics);
            //   fp16 storage: never (round 3's form - statistics only, coefficient kernel - measured slower than the passes it removes,
            //   profiles/r3_negative_results.txt; its knob left the tree in round 5).
            static const bool swin_stats_split = rs_env_on("RS_GN_SWIN_STATS_SPLIT");
            const bool sstats = X.dt == RS_F16S && swin_stats_split;
            if (fuse_proj && sstats && fold2) ex.attach_stats(e2, (X.H / 8) * (X.W / 8), E);   // (only where norm2 is a coefficient-only GroupNorm: the fused MLP applies it)
            if (fuse_qkv) {
                {   // the fused kernels' per-operand size limit (RS_BUFFER_BYTES_LIMIT), both passes: the dry pass ends the call before anything is launched
                    std::string text;
                    const View& xin = fold1 ? e : n;
                    if (rs_win_attn_operand_over(std::string(), X.B, X.H, X.W, xin.ld, fuse_proj ? e.ld : 0, X.dt == RS_F16S, &text)) {
                        (void)rs_win_attn_operand_over(ex.prefix + bp + "attn", X.B, X.H, X.W, xin.ld, fuse_proj ? e.ld : 0, X.dt == RS_F16S, &text);
                        ex.fail(RS_ERR_OPERAND_BYTES, text);
                        ex.reset(mk);
                        return;
                    }
                }
                if (!ex.dry) {
                    WinAttnParams p{};
                    p.bias_n = s.bias_n; p.bias_c = s.bias_c; p.B = X.B; p.H = X.H; p.W = X.W; p.heads = heads; p.shift = s.shift;
                    p.scale = 1.0f / std::sqrt((float)(E / heads));
                    if (fold1) { p.x = e.p; p.ldx = e.ld; p.xcoef = coef1; } else { p.x = n.p; p.ldx = n.ld; }
                    p.wqkv = s.qkv.w_frag_for(X.dt); p.bqkv = s.qkv.bias;
                    if (fuse_proj) { p.out = e2.p; p.ldo = e2.ld; p.wproj = s.proj.w_frag_for(X.dt); p.bproj = s.proj.bias; p.res = e.p; p.ldres = e.ld;
                                     p.ystats = e2.st; p.ystats_ld = e2.stld;
                                     if (e2.st) (void)ex.fill_tail(e2.st_prod, X.B, p.tail); }
                    else { p.out = a.p; p.ldo = a.ld; }
                    ex.win_attn_qkv(p, E, X.dt);
                }
            } else if (!ex.dry) {
                WinAttnParams p{};
                p.qkv = qkv.p; p.out = a.p; p.bias_t = s.bias_t; p.bias_n = s.bias_n; p.B = X.B; p.H = X.H; p.W = X.W; p.heads = heads;
                p.shift = s.shift; p.ldq = qkv.ld; p.ldo = a.ld; p.scale = 1.0f / std::sqrt((float)(E / heads));
                ex.check(rs_win_attn_launch(&p, X.dt, ex.st), "win_attn");
            }
            if (!fuse_proj) {
                ex.tr(bp + "attn", a);
                e2 = ex.T(X.B, X.H, X.W, E, X.dt);
                k1(s.proj, a, e2).residual(e).launch(ex);
            }
            ex.tr(bp + "proj", e2);
            View e3;
            View n2;
            const float* coef2 = nullptr;
            if (fold2) coef2 = gn_coef(ex, s.n2, e2, 1e-5f, nullptr);
            else { n2 = ex.T(X.B, X.H, X.W, E, X.dt); gn(ex, s.n2, e2, n2, 1e-5f, RS_ACT_NONE); }
            // patch_unembed inside the last block's MLP launch (swin_mlp.hip, NO != E): split storage, norm2 folded (the kernel's x is the block's
            // raw input = its shortcut), the product matrix below the scaled-fragment limit.  RS_UNEMBED_FOLD=0: the 1x1 conv as a launch.
            static const bool unfold_on = rs_env_on("RS_UNEMBED_FOLD");
            const bool unfold = unfold_on && fuse_mlp && fold2 && X.dt == RS_F16S && &s == &b.blocks.back() && b.has_unfold && b.unfold.ws &&
                                !m.big(b.unfold) && Y.dt == RS_F16S && Y.C == b.C && rs_swin_mlp_split_unembed_supported(E, s.fc1.Cout, b.C) &&
                                (Y.ld % 8) == 0 && (e2.ld % 8) == 0;   // (the launcher's alignment preconditions: an unaligned view falls back to the separate 1x1 conv instead of failing the pass - ADVICE r5)
            if (unfold) {
                Y.drop_stats();
                if (out_stats && sstats && HWt % 128 == 0 && Mtok % 128 == 0) ex.attach_stats(Y, HWt / 128, Y.C);   // statistics (+ tail) for the GroupNorm that consumes the layer's output
                if (!ex.dry) {
                    SwinMlpCall c = mlp_call(e2, Y);
                    c.w2 = b.unfold.ws; c.b2 = b.unfold.bias; c.NO = b.C; c.xcoef = coef2;
                    ex.swin_mlp(c, X.dt);
                }
                ex.reset(mk);
                return;
            }
            if (fuse_mlp) {
                e3 = ex.T(X.B, X.H, X.W, E, X.dt);
                const bool is_last = &s == &b.blocks.back();   // (the last block's output feeds patch_unembed, not a GroupNorm)
                if (sstats && !is_last && HWt % 128 == 0 && Mtok % 128 == 0) ex.attach_stats(e3, HWt / 128, E);
                if (!ex.dry) {
                    SwinMlpCall c = mlp_call(fold2 ? e2 : n2, e3);   // (norm2 folded: the raw tensor and its coefficients)
                    c.w2 = s.fc2.w_for(X.dt); c.b2 = s.fc2.bias; c.res = e2.p; c.ldres = e2.ld; c.xcoef = fold2 ? coef2 : nullptr;
                    ex.swin_mlp(c, X.dt);
                }
            } else {
                View f = ex.T(X.B, X.H, X.W, s.fc1.Cout, X.dt);
                k1(s.fc1, n2, f).act(RS_ACT_GELU).launch(ex);
                e3 = ex.T(X.B, X.H, X.W, E, X.dt);
                k1(s.fc2, f, e3).residual(e2).launch(ex);
            }
            ex.tr(bp + "out", e3);
            e = e3;
        }
        Y = conv_for_gn(ex, k1(b.unembed, e, Y), out_stats);
        ex.reset(mk);
    }
    // a block under its debug-trace name: the records `body` makes go under "<name>.", then the block's output `y` under the name itself
    template <class F> void traced(Exec& ex, const std::string& nm, const View& y, F body) {
        { const Exec::Scope sc = ex.scope(nm); body(); }
        ex.tr(nm, y);
    }
    // model.py:179-203: x + proj_out(softmax(q k^T / sqrt(C)) v); S is materialised in fp32 per image chunk
    void attnblock(Exec& ex, const AttnW& a, const View& X, View& Y) {
        const size_t mk = ex.mark();
        const int C = a.C, T = X.H * X.W, dt = X.dt;
        View n = ex.T(X.B, X.H, X.W, C, dt);
        gn(ex, a.norm, X, n, 1e-6f, RS_ACT_NONE);
        View q = ex.T(X.B, X.H, X.W, C, dt), k = ex.T(X.B, X.H, X.W, C, dt);
        k1(a.q, n, q).launch(ex);
        k1(a.k, n, k).launch(ex);
        ex.tr("norm", n); ex.tr("q", q); ex.tr("k", k);
        View o = ex.T(X.B, X.H, X.W, C, dt);
        // fp16 storage: streaming attention (ae_attn.hip) - S never reaches HBM; RS_AE_FLASH=0 keeps the row-block path below (A/B runs),
        // which also serves fp32 / split storage and token counts that are not multiples of 128
        static const bool flash_on = rs_env_on("RS_AE_FLASH");
        // split storage (the encoder of the parity policy): the same on (hi, lo) pairs, ae_attn_split.hip (round 4)
        const bool flash16 = dt == RS_F16 && rs_ae_flash_supported(C, T) && a.v.wh;
        const bool flash_s = dt == RS_F16S && rs_ae_flash_split_supported(C, T) && a.v.ws;
        if (flash_on && (flash16 || flash_s)) {
            char* vTa = (char*)ex.raw((size_t)X.B * C * T * rs_dtype_size(dt));
            if (!ex.dry) {
                // vT[z][c][t] = sum_k Wv[c][k] n[z][t][k]   (bias added to the attention output: softmax rows sum to 1)
                gemm_nt(ex, {a.v.w_for(dt), 0}, {n.p, (long long)T * C}, nullptr, vTa, (long long)C * T, {X.B, C, T, C, 1.f, dt, dt});
                AeFlashCall c{};
                c.q = q.p; c.ldq = q.ld; c.k = k.p; c.ldk = k.ld; c.vt = vTa; c.bv = a.v.bias; c.o = o.p; c.ldo = o.ld;
                c.nz = X.B; c.T = T; c.C = C; c.scale = 1.0f / std::sqrt((float)C);
                ex.ae_flash(c, dt);
            }
            ex.tr("o", o);
            Y = conv_for_gn(ex, k1(a.proj, o, Y).residual(X));
            ex.reset(mk);
            return;
        }
        // The score matrix is materialised, but never more than `budget` floats of it at a time (4 GiB of fp32 S + the same
        // number of P elements): several images per pass while a whole T x T matrix fits (the 64 x 64 latents of the shipped
        // configs: T = 4096), otherwise one image in blocks of query rows (softmax is row-wise, so row blocks are independent).
        // That is what lets the tiled path run the reference's real tile sizes (inference_resshift.py:149-161): a 256 x 256 LR
        // tile is T = 65 536 tokens, 512 x 512 T = 262 144.  At d = 512 a flash-style kernel would have to stream a 64 KB K
        // tile AND a 64 KB V tile through LDS per 64 keys (one ds_read_b128 per MFMA: LDS-bound); the two GEMMs + row softmax
        // run on the tuned implicit-GEMM path instead and their scratch is bounded here.
        static const size_t budget = (size_t)rs_env_int("RS_ATTN_S_FLOATS", 1LL << 30);
        const size_t tt = (size_t)T * T;
        const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)X.B, budget / tt));
        int rows = T;
        if (tt > budget) rows = (int)std::max<size_t>(128, std::min<size_t>((size_t)T, (budget / (size_t)T) / 128 * 128));
        const size_t es = rs_dtype_size(dt);
        char* vT = (char*)ex.raw((size_t)chunk * C * T * es);
        float* S = (float*)ex.raw((size_t)chunk * rows * T * sizeof(float));
        char* P = (char*)ex.raw((size_t)chunk * rows * T * es);
        if (!ex.dry) {
            for (int b0 = 0; b0 < X.B; b0 += chunk) {
                const int nz = std::min(chunk, X.B - b0);
                const size_t boff = (size_t)b0 * T * C * es;
                // vT[z][c][t] = sum_k Wv[c][k] n[z][t][k]   (bias folded into the PV epilogue: softmax rows sum to 1)
                gemm_nt(ex, {a.v.w_for(dt), 0}, {(char*)n.p + boff, (long long)T * C}, nullptr, vT, (long long)C * T, {nz, C, T, C, 1.f, dt, dt});
                for (int r0 = 0; r0 < T; r0 += rows) {
                    const int nr = std::min(rows, T - r0);   // (rows == T unless a single image is processed in row blocks)
                    const size_t roff = boff + (size_t)r0 * C * es;
                    gemm_nt(ex, {(char*)q.p + roff, (long long)T * C}, {(char*)k.p + boff, (long long)T * C}, nullptr, S, (long long)nr * T,
                            {nz, nr, T, C, 1.0f / std::sqrt((float)C), dt, RS_F32});
                    ex.check(rs_softmax_rows_launch(S, P, dt, (long long)nz * nr, T, T, T, ex.st), "softmax");
                    gemm_nt(ex, {P, (long long)nr * T}, {vT, (long long)C * T}, a.v.bias, (char*)o.p + roff, (long long)T * C, {nz, nr, C, T, 1.f, dt, dt});
                }
            }
        }
        ex.tr("o", o);
        Y = conv_for_gn(ex, k1(a.proj, o, Y).residual(X));
        ex.reset(mk);
    }
    // y[z][m][n] = scale * sum_k A[z][m][k] B[z][n][k] (+bias[n]): nz dense matrices each, `bs` elements apart (0: one shared by all z)
    struct Mat { const void* p; long long bs; };
    struct GemmShape { int nz, M, N, K; float scale; int in_dt, out_dt; };
    void gemm_nt(Exec& ex, Mat A, Mat Bm, const float* bias, void* y, long long bsY, const GemmShape& g) {
        if (!A.p || !Bm.p) { ex.fail(-3, "gemm operand missing (precision not packed?)"); return; }
        IGemmParams p{};
        p.x0 = A.p; p.w = Bm.p; p.bias = bias; p.y = y; p.C0 = g.K; p.ld0 = g.K; p.B = 1; p.Hs = g.M; p.Ws = 1; p.up = 1; p.Ho = g.M; p.Wo = 1;
        p.KH = 1; p.KW = 1; p.stride = 1; p.Cout = g.N; p.ldy = g.N; p.M = g.M; p.Ktot = g.K; p.out_scale = g.scale;
        p.bs_x0 = A.bs; p.bs_w = Bm.bs; p.bs_y = bsY;
        ConvPlan pl{};
        (void)rs_conv_plan(&p, g.in_dt, g.out_dt, g.nz, &pl);
        ex.igemm(p, pl, g.in_dt, g.out_dt, g.nz, "gemm_nt");
    }
    // per-image FiLM table [B][film_total] for a batch whose images are at different timesteps: ONE gather launch from the cached rows
    // (rows[b] = film_row(t_b)), so that every image sees exactly the values the shared row of a homogeneous batch would give it.  Lives in
    // the scratch arena; the dry pass gets a non-null stand-in (never dereferenced) so that "has FiLM" reads the same in both passes.
    const float* film_table(Exec& ex, const float* const* rows, int B) {
        float* tab = (float*)ex.raw((size_t)B * m.film_total * sizeof(float));
        if (ex.dry) return (const float*)(uintptr_t)4096;
        ex.check(rs_film_gather_launch(rows, B, m.film_total, tab, ex.st), "film gather");
        return tab;
    }
    // ---------------------------------------------------------------- UNet forward
    struct UNetCall {
        const float* x;             // NCHW fp32 [B,Cz,H,W] (already scaled by _scale_input when called through the drop-in API) ...
        float xscale;               // ... times this factor,
        const float* xscale_rows;   // or (non-null) times one factor per image
        const View* lq_feat;        // optional NHWC view of the (feature-extracted) conditioning
        const float* lq_nchw; const float* mask_nchw;
        float* out;                 // NCHW fp32
        int B, H, W, dt;
        const float* film; int film_ld;   // the FiLM row of the batch's timestep, or (film_ld > 0) a per-image table [B][film_ld], film_table()
    };
    void unet_body(Exec& ex, const UNetCall& c) {
        const float* const x = c.x; const float* const film = c.film; const View* const lq_feat = c.lq_feat;
        const int B = c.B, H = c.H, W = c.W, dt = c.dt;
        ex.enter_part("unet");
        ex.film_base = film; ex.film_ld = c.film_ld;
        const rs_unet_config& u = m.cfg.unet;
        const int n_in = (int)m.in_blocks.size(), n_out = (int)m.out_blocks.size();
        const size_t mk0 = ex.mark();
        ex.pool_off = 0;   // coefficient pool: every slot is consumed within this forward; the next one may reuse them (stream order)
        auto lvH = [&](int level) { return H >> level; };
        auto lvW = [&](int level) { return W >> level; };
        // zero-copy concat buffers, one per output block
        std::vector<View> cat(n_out);
        for (int j = 0; j < n_out; ++j) {
            const int i = n_in - 1 - j, lvl = m.in_blocks[i].level;
            cat[j] = ex.T(B, lvH(lvl), lvW(lvl), m.h_ch[j] + m.skip_ch[i], dt);
        }
        auto skip_view = [&](int i) { const int j = n_in - 1 - i; return cat[j].slice(m.h_ch[j], m.skip_ch[i]); };
        // statistics of the two halves of every concat buffer (want_stats): the decoder side is channels [0, h_ch), the encoder's skip the
        // rest; once both are known the output block's in_layers[0] GroupNorm needs no pass over the tensor, and the launch that writes
        // the decoder half - always the later one - carries its tail
        struct Half { float* st = nullptr; int S = 0, ld = 0, prod = -1; };
        std::vector<Half> cat_lo(n_out), cat_hi(n_out);
        auto note = [](Half& hf, const View& v) { if (v.st && !v.st2) { hf.st = v.st; hf.S = v.stS; hf.ld = v.stld; hf.prod = v.st_prod; } };
        auto cat_view = [&](int j) {
            View X = cat[j];
            if (cat_lo[j].st && cat_hi[j].st) {
                X.st = cat_lo[j].st; X.stS = cat_lo[j].S; X.stld = cat_lo[j].ld; X.st_prod = cat_lo[j].prod;
                X.st2 = cat_hi[j].st; X.st2S = cat_hi[j].S; X.st2ld = cat_hi[j].ld; X.st_n0 = m.h_ch[j];
            }
            return X;
        };
        // ---- input conv (unet.py:876-886): cat[x, lq(,mask)]
        const int Cz = u.in_channels;
        auto x_to_nhwc = [&](const View& v) {   // x (times _scale_input: one factor, or one per image) into channels [0, Cz) of v
            if (c.xscale_rows) ex.check(rs_nchw_to_nhwc_rows_launch(x, v.p, dt, B, Cz, H * W, v.ld, 0, c.xscale_rows, ex.st), "x->nhwc (per image)");
            else ex.check(rs_nchw_to_nhwc_launch(x, v.p, dt, B, Cz, H * W, v.ld, 0, c.xscale, ex.st), "x->nhwc");
        };
        View h;
        {
            const size_t mk = ex.mark();
            View y0 = skip_view(0);
            if (m.fe_convs.empty()) {
                const int cl = m.fe_out_ch;  // 3 or 4 raw conditioning channels at latent resolution
                // cat[x, lq(, mask)] as one channel-padded NHWC tensor in the working precision (6/7 -> 8 channels)
                View in0 = ex.T(B, H, W, m.in_blocks[0].conv.CinP, dt);
                if (!ex.dry) {
                    zero(ex, in0);
                    x_to_nhwc(in0);
                    if (cl) ex.check(rs_nchw_to_nhwc_launch(c.lq_nchw, in0.p, dt, B, 3, H * W, in0.ld, Cz, 1.f, ex.st), "lq->nhwc");
                    if (cl == 4) ex.check(rs_nchw_to_nhwc_launch(c.mask_nchw, in0.p, dt, B, 1, H * W, in0.ld, Cz + 3, 1.f, ex.st), "mask->nhwc");
                }
                y0 = conv_for_gn(ex, k3(m.in_blocks[0].conv, in0, y0));
            } else {
                // conditioning goes through the strided-conv feature extractor (unet.py:693-702); lq_feat precomputed
                View xin = ex.T(B, H, W, Cz, dt);
                if (!ex.dry) x_to_nhwc(xin);
                ConvCall c0 = k3(m.in_blocks[0].conv, xin, y0);
                if (lq_feat) c0.second_source(*lq_feat);
                c0.launch(ex);
            }
            ex.reset(mk);
            h = y0;
            note(cat_hi[n_in - 1], y0);
            ex.tr("in.0", h);
        }
        // ---- input blocks
        for (int i = 1; i < n_in; ++i) {
            const UBlock& b = m.in_blocks[i];
            const size_t mk = ex.mark();
            View y = skip_view(i);
            const std::string nm = "in." + std::to_string(i);
            if (b.has_down) {
                y = conv_for_gn(ex, k3(b.conv, h, y).strided(2, 1));
            } else if (b.has_swin) {
                View r = ex.T(B, h.H, h.W, b.out_ch, dt);
                traced(ex, nm + ".res", r, [&] { resblock(ex, b.res, h, r, film, /*out_stats=*/false); });   // (r feeds patch_embed, not a GroupNorm)
                const Exec::Scope sc = ex.scope(nm + ".swin");
                basiclayer(ex, b.swin, r, y);
            } else {
                const Exec::Scope sc = ex.scope(nm + ".res");
                resblock(ex, b.res, h, y, film);
            }
            ex.tr(nm, y);
            ex.reset(mk);
            h = y;
            note(cat_hi[n_in - 1 - i], y);
        }
        // ---- middle (unet.py:889)
        {
            const size_t mk = ex.mark();
            View r1 = ex.T(B, h.H, h.W, h.C, dt), r2 = ex.T(B, h.H, h.W, h.C, dt);
            traced(ex, "mid.res1", r1, [&] { resblock(ex, m.mid_res1, h, r1, film, /*out_stats=*/false); });
            traced(ex, "mid.swin", r2, [&] { basiclayer(ex, m.mid_swin, r1, r2); });
            View y = cat[0].slice(0, m.h_ch[0]);
            traced(ex, "mid.res2", y, [&] { resblock(ex, m.mid_res2, r2, y, film); });
            note(cat_lo[0], y);
            ex.reset(mk);
        }
        // ---- output blocks (unet.py:890-892)
        View last;
        for (int j = 0; j < n_out; ++j) {
            const UBlock& b = m.out_blocks[j];
            const View X = cat_view(j);
            View y;
            if (j + 1 < n_out) {
                y = cat[j + 1].slice(0, m.h_ch[j + 1]);
            } else {
                last = ex.T(B, X.H, X.W, b.out_ch, dt);  // stays live for the out head
                y = last;
            }
            const size_t mk = ex.mark();
            const std::string nm = "out." + std::to_string(j);
            if (!b.has_swin && !b.has_up) {
                const Exec::Scope sc = ex.scope(nm + ".res");
                resblock(ex, b.res, X, y, film);
            } else {
                View cur = ex.T(B, X.H, X.W, b.out_ch, dt);
                traced(ex, nm + ".res", cur, [&] { resblock(ex, b.res, X, cur, film, /*out_stats=*/false); });   // (feeds patch_embed or the upsampling conv)
                if (b.has_swin && b.has_up) {
                    View r2 = ex.T(B, X.H, X.W, b.out_ch, dt);
                    traced(ex, nm + ".swin", r2, [&] { basiclayer(ex, b.swin, cur, r2, /*out_stats=*/false); });
                    cur = r2;
                } else if (b.has_swin) {
                    const Exec::Scope sc = ex.scope(nm + ".swin");
                    basiclayer(ex, b.swin, cur, y);
                }
                if (b.has_up) {
                    if (b.has_upf && upfold_ok(b.upf, cur, y)) y = upfold(ex, b.upf, cur, y, /*stats=*/true);
                    else y = conv_for_gn(ex, k3(b.conv, cur, y).upsampled());
                }
            }
            if (j + 1 < n_out) note(cat_lo[j + 1], y); else last = y;
            ex.tr(nm, y);
            ex.reset(mk);
        }
        // ---- out head (unet.py:893-894)
        {
            View o = ex.T(B, H, W, u.out_channels, RS_F32);
            head(ex, m.out_norm, m.out_conv, last, o, 1e-5f);
            if (!ex.dry) ex.check(rs_nhwc_to_nchw_launch(o.p, RS_F32, c.out, B, u.out_channels, H * W, o.ld, 0, ex.st), "out->nchw");
        }
        ex.reset(mk0);
    }
    // feature_extractor(cat[lq, mask]) (unet.py:876-881, 693-702): Conv3x3 -> SiLU -> Downsample conv s2
    View feature_extract(Exec& ex, const float* lq, const float* mask, int B, int Hl, int Wl, int dt) {
        const int cin = m.cfg.unet.cond_mask ? 4 : 3;
        View cur = ex.T(B, Hl, Wl, m.fe_convs[0].CinP, dt);  // 3/4 -> 8 zero-padded channels
        if (!ex.dry) {
            zero(ex, cur);
            ex.check(rs_nchw_to_nhwc_launch(lq, cur.p, dt, B, 3, Hl * Wl, cur.ld, 0, 1.f, ex.st), "lq->nhwc");
            if (cin == 4) ex.check(rs_nchw_to_nhwc_launch(mask, cur.p, dt, B, 1, Hl * Wl, cur.ld, 3, 1.f, ex.st), "mask->nhwc");
        }
        for (size_t s = 0; s < m.fe_convs.size(); ++s) {
            View a = ex.T(B, cur.H, cur.W, m.fe_convs[s].Cout, dt);
            k3(m.fe_convs[s], cur, a).act(RS_ACT_SILU).launch(ex);
            View d = ex.T(B, cur.H / 2, cur.W / 2, m.fe_downs[s].Cout, dt);
            k3(m.fe_downs[s], a, d).strided(2, 1).launch(ex);
            cur = d;
        }
        return cur;
    }

    // ---------------------------------------------------------------- AE
    // img NCHW fp32 [B,3,H,W] (or NHWC view if `img_nhwc`) -> z NCHW fp32 [B,embed,H/f,W/f]
    void encode_body(Exec& ex, const View& in_nhwc, float* z_nchw, int dt) {
        ex.enter_part("encoder");
        const rs_ae_config& a = m.cfg.ae;
        const size_t mk0 = ex.mark();
        ex.pool_off = 0;
        const int B = in_nhwc.B;
        View h = ex.T(B, in_nhwc.H, in_nhwc.W, a.ch, dt);
        h = conv_for_gn(ex, k3(m.enc_in, in_nhwc, h));
        // debug-trace names: the blocks of oracle.resshift_oracle.ae_encode_plan, inner records under their block's prefix
        ex.tr("enc.in", h);
        for (int l = 0; l < a.n_levels; ++l) {
            const AELevel& L = m.enc_levels[l];
            const std::string lv = "enc.down." + std::to_string(l);
            int bi = 0;
            for (const ResBlockW& r : L.blocks) {
                View y = ex.T(B, h.H, h.W, r.Cout, dt);
                traced(ex, lv + ".block." + std::to_string(bi++), y, [&] { resnet(ex, r, h, y); });
                h = y;
            }
            if (L.has_resample) {
                // F.pad(x,(0,1,0,1)) + conv stride 2 pad 0 (model.py:80-84)
                View y = ex.T(B, h.H / 2, h.W / 2, h.C, dt);
                y = conv_for_gn(ex, k3(L.resample, h, y).strided(2, 0));
                ex.tr(lv + ".ds", y);
                h = y;
            }
        }
        View m1 = ex.T(B, h.H, h.W, h.C, dt); traced(ex, "enc.mid.block_1", m1, [&] { resnet(ex, m.enc_mid1, h, m1); });
        View m2 = ex.T(B, h.H, h.W, h.C, dt); traced(ex, "enc.mid.attn", m2, [&] { attnblock(ex, m.enc_attn, m1, m2); });
        View m3 = ex.T(B, h.H, h.W, h.C, dt); traced(ex, "enc.mid.block_2", m3, [&] { resnet(ex, m.enc_mid2, m2, m3); });
        View zc = ex.T(B, h.H, h.W, a.z_channels, RS_F32);
        head(ex, m.enc_norm, m.enc_out, m3, zc, 1e-6f);
        ex.tr("enc.out", zc);   // (enc.z, the quant_conv, is the call's output)
        View zq = ex.T(B, h.H, h.W, a.embed_dim, RS_F32);
        k1(m.quant_conv, zc, zq).launch(ex);
        if (!ex.dry) ex.check(rs_nhwc_to_nchw_launch(zq.p, RS_F32, z_nchw, B, a.embed_dim, h.H * h.W, zq.ld, 0, ex.st), "z->nchw");
        ex.reset(mk0);
    }
    // z NCHW fp32 [B,embed,h,w] (times zscale) -> img NCHW fp32; idx_out: the VQ codes, unless force_nq skips the quantiser
    struct DecodeCall { const float* z; float zscale; float* img; int32_t* idx_out; int B, h, w, force_nq, dt; };
    void decode_body(Exec& ex, const DecodeCall& c) {
        const float* const z_nchw = c.z; float* const img = c.img;
        const int B = c.B, h_ = c.h, w_ = c.w, dt = c.dt;
        ex.enter_part("decoder");
        const rs_ae_config& a = m.cfg.ae;
        const size_t mk0 = ex.mark();
        ex.pool_off = 0;
        View z = ex.T(B, h_, w_, a.embed_dim, RS_F32);
        if (!ex.dry) ex.check(rs_nchw_to_nhwc_launch(z_nchw, z.p, RS_F32, B, a.embed_dim, h_ * w_, z.ld, 0, c.zscale, ex.st), "z->nhwc");
        View q = z;
        if (!c.force_nq) {
            q = ex.T(B, h_, w_, a.embed_dim, RS_F32);
            if (!ex.dry) ex.check(rs_vq_launch((const float*)z.p, m.codebook, (float*)q.p, c.idx_out, (long long)B * h_ * w_, a.n_embed, a.embed_dim, ex.st), "vq");
            // debug-trace names: the blocks of oracle.resshift_oracle.ae_decode_plan, inner records under their block's prefix
            ex.tr("dec.zq.z", z);   // (the latents the argmin saw: the call's input times zscale)
            ex.tr("dec.zq", q);
        }
        View pq = ex.T(B, h_, w_, m.dec_in.CinP, dt);  // z_channels zero-padded to the decoder conv_in's chunk size
        zero(ex, pq);
        k1(m.post_quant_conv, q, pq.slice(0, a.z_channels)).launch(ex);
        ex.tr("dec.pq", pq.slice(0, a.z_channels));
        View h = ex.T(B, h_, w_, m.dec_in.Cout, dt);
        k3(m.dec_in, pq, h).launch(ex);
        ex.tr("dec.in", h);
        View m1 = ex.T(B, h.H, h.W, h.C, dt); traced(ex, "dec.mid.block_1", m1, [&] { resnet(ex, m.dec_mid1, h, m1); });
        View m2 = ex.T(B, h.H, h.W, h.C, dt); traced(ex, "dec.mid.attn", m2, [&] { attnblock(ex, m.dec_attn, m1, m2); });
        View m3 = ex.T(B, h.H, h.W, h.C, dt); traced(ex, "dec.mid.block_2", m3, [&] { resnet(ex, m.dec_mid2, m2, m3); });
        h = m3;
        for (int l = a.n_levels - 1; l >= 0; --l) {
            const AELevel& L = m.dec_levels[l];
            const std::string lv = "dec.up." + std::to_string(l);
            int bi = 0;
            for (const ResBlockW& r : L.blocks) {
                View y = ex.T(B, h.H, h.W, r.Cout, dt);
                traced(ex, lv + ".block." + std::to_string(bi++), y, [&] { resnet(ex, r, h, y); });
                h = y;
            }
            if (L.has_resample) {
                View y = ex.T(B, h.H * 2, h.W * 2, h.C, dt);
                if (L.has_upf && upfold_ok(L.upf, h, y)) upfold(ex, L.upf, h, y, /*stats=*/false);
                else k3(L.resample, h, y).upsampled().launch(ex);
                ex.tr(lv + ".us", y);
                h = y;
            }
        }
        View o = ex.T(B, h.H, h.W, a.out_ch, RS_F32);
        head(ex, m.dec_norm, m.dec_out, h, o, 1e-6f);
        if (!ex.dry) ex.check(rs_nhwc_to_nchw_launch(o.p, RS_F32, img, B, a.out_ch, h.H * h.W, o.ld, 0, ex.st), "img->nchw");
        ex.reset(mk0);
    }

    // ---------------------------------------------------------------- the sampling loop in three parts
    // (rs_sample runs them in one call; rs_sample_begin / rs_sample_step / rs_sample_end one at a time, for a scheduler that admits and
    // retires images at every step)
    int latent_div() const { return 1 << (m.cfg.ae.n_levels - 1); }
    // encode_first_stage(y, up_sample=True) -> * scale_factor -> prior_sample (gaussian_diffusion.py:500-529): x_T = z_y + prior_scale * noise0
    // `keys` (seeded calls): the prior draw is draw 0 of keys[b], generated by the kernel in place of the read of noise0 (keys_dev: the device
    // copy of a batch above RS_MAX_ROWS)
    void sample_prologue(Exec& ex, const rs_sample_args* a, float* z_y, float* xt, const float* noise0, const rs_noise_key* keys = nullptr,
                         const rs_noise_key* keys_dev = nullptr) {
        const rs_ae_config& ae = m.cfg.ae;
        const int B = a->B, Hi = a->h * a->sf, Wi = a->w * a->sf, f = latent_div();
        const long long zcount = (long long)B * ae.embed_dim * (Hi / f) * (Wi / f);
        {
            const size_t mk = ex.mark();
            View in = ex.T(B, Hi, Wi, m.enc_in.CinP, a->prec_encode);  // RGB zero-padded to 8 channels
            zero(ex, in);
            if (!ex.dry) {
                if (a->sf != 1) ex.check(rs_bicubic_launch(a->y, in.p, a->prec_encode, B, ae.in_channels, a->h, a->w, a->sf, in.ld, ex.st), "bicubic");
                else ex.check(rs_nchw_to_nhwc_launch(a->y, in.p, a->prec_encode, B, ae.in_channels, Hi * Wi, in.ld, 0, 1.f, ex.st), "y->nhwc");
            }
            encode_body(ex, in, z_y, a->prec_encode);
            ex.reset(mk);
        }
        if (!ex.dry) {
            // z_y * scale_factor, then prior_sample: x_T = z_y + kappa*sqrt(eta_T)*noise (gaussian_diffusion.py:512,529)
            if (a->scale_factor != 1.0f) ex.check(rs_axpbypcz_launch(z_y, nullptr, nullptr, z_y, a->scale_factor, 0.f, 0.f, zcount, ex.st), "scale z_y");
            if (keys) {
                const int nr = B > RS_MAX_ROWS ? 1 : B;
                float ca[RS_MAX_ROWS], cc[RS_MAX_ROWS];
                int dr[RS_MAX_ROWS];
                for (int b = 0; b < nr; ++b) { ca[b] = 1.f; cc[b] = a->prior_scale; dr[b] = 0; }
                ex.check(rs_axpbypcz_seeded_launch(z_y, nullptr, xt, ca, nullptr, cc, keys, keys_dev, dr, zcount / B, B, ex.st), "prior_sample (seeded)");
            } else
                ex.check(rs_axpbypcz_launch(z_y, nullptr, noise0, xt, 1.f, 0.f, a->prior_scale, zcount, ex.st), "prior_sample");
        }
    }
    // one p_sample (gaussian_diffusion.py:332-365) of every image b at its own step index t[b]: pred = model(_scale_input(x_t), tmap[t], lq),
    // x_{t-1} = coef1 x_t + coef2 pred + [t > 0] sigma noise, in place.  Equal indices: exactly the scalar launches of rs_sample.  Otherwise
    // the per-image FiLM table (+ one gather launch), _scale_input per image inside the UNet's input conversion and the per-image
    // elementwise kernel: every image gets bit for bit what it would get in a homogeneous batch of the same size.  films[i]: cached FiLM row of step index i (rows not used may be null).
    struct StepCall {
        float* xt; float* pred;                                        // [B,Cz,hz,wz] NCHW fp32: x_t (updated in place), the UNet's prediction
        const View* feat; const float* y; const float* mask;           // the UNet's conditioning (UNetCall::lq_feat / lq_nchw / mask_nchw)
        int B, hz, wz, prec;
        const int* t;                                                  // [B] step indices
        const rs_sample_args* a; const float* const* films;
        const float* noise;                                            // the step's noise, or (seeded calls) ...
        const rs_noise_key* keys; const rs_noise_key* keys_dev;        // ... the images' keys (keys_dev: sample_prologue())
    };
    void sample_step(Exec& ex, const StepCall& c) {
        float* const xt = c.xt; float* const pred = c.pred; const int* const t = c.t; const rs_sample_args* const a = c.a; const rs_noise_key* const keys = c.keys;
        const int B = c.B, hz = c.hz, wz = c.wz;
        UNetCall u{};
        u.x = xt; u.lq_feat = c.feat; u.lq_nchw = c.y; u.mask_nchw = c.mask; u.out = pred; u.B = B; u.H = hz; u.W = wz; u.dt = c.prec;
        bool mixed = false;
        for (int b = 1; b < B; ++b) mixed |= t[b] != t[0];
        const long long zcount = (long long)B * m.cfg.unet.in_channels * hz * wz, per = zcount / B;
        float ca[RS_MAX_ROWS], cb[RS_MAX_ROWS], cc[RS_MAX_ROWS];
        int dr[RS_MAX_ROWS];
        // mean = c1*x_t + c2*x0 (:218-221); sample = mean + [t>0]*sigma_t*eps (:358-364), per image; the draw of the step at step index i is
        // draw steps - i of the image's key
        auto posterior = [&](int nr) {
            for (int b = 0; b < nr; ++b) { const int i = t[b]; ca[b] = a->coef1[i]; cb[b] = a->coef2[i]; cc[b] = i > 0 ? a->sigma[i] : 0.f; dr[b] = a->steps - i; }
        };
        if (!mixed) {
            const int i = t[0];
            u.xscale = a->inv_std[i]; u.film = c.films[i];
            unet_body(ex, u);
            if (ex.dry) return;
            if (keys) {
                posterior(B > RS_MAX_ROWS ? 1 : B);
                ex.check(rs_axpbypcz_seeded_launch(xt, pred, xt, ca, cb, cc, keys, c.keys_dev, dr, per, B, ex.st), "posterior step (seeded)");
            } else
                ex.check(rs_axpbypcz_launch(xt, pred, i > 0 ? c.noise : nullptr, xt, a->coef1[i], a->coef2[i], a->sigma[i], zcount, ex.st), "posterior step");
            return;
        }
        const size_t mk = ex.mark();
        const float* rows[RS_MAX_ROWS];
        for (int b = 0; b < B; ++b) rows[b] = c.films[t[b]];
        const float* tab = film_table(ex, rows, B);
        for (int b = 0; b < B; ++b) ca[b] = a->inv_std[t[b]];   // _scale_input per image (:598-609)
        u.xscale = 1.0f; u.xscale_rows = ca; u.film = tab; u.film_ld = m.film_total;
        unet_body(ex, u);
        if (!ex.dry) {
            posterior(B);
            if (keys) ex.check(rs_axpbypcz_seeded_launch(xt, pred, xt, ca, cb, cc, keys, nullptr, dr, per, B, ex.st), "posterior step (per image, seeded)");
            else ex.check(rs_axpbypcz_rows_launch(xt, pred, c.noise, xt, ca, cb, cc, per, B, ex.st), "posterior step (per image)");
        }
        ex.reset(mk);
    }
    // z_out, then decode_first_stage: z / scale_factor -> VQ -> post_quant_conv -> Decoder (gaussian_diffusion.py:474-498)
    void sample_epilogue(Exec& ex, const rs_sample_args* a, const float* xt) {
        const int f = latent_div(), hz = a->h * a->sf / f, wz = a->w * a->sf / f;
        const long long zcount = (long long)a->B * m.cfg.ae.embed_dim * hz * wz;
        if (a->z_out && !ex.dry) (void)hipMemcpyAsync(a->z_out, xt, zcount * 4, hipMemcpyDeviceToDevice, ex.st);
        decode_body(ex, DecodeCall{xt, 1.0f / a->scale_factor, a->out, a->idx_out, a->B, hz, wz, 0, a->prec_decode});
    }
};

}  // namespace

// The engine object and the C ABI declared in include/resshift_hip.h: rs_engine is a Model (model.h: what is packed and where) plus the
// runtime state of its calls - scratch arena, GroupNorm tail plan, profiling, debug trace, FiLM cache, staged noise keys - and run(),
// which walks a graph of graphs.h twice: a dry sizing pass, then the real pass.  The op-level test entries live in ops.hip.
//
// All weights live in ONE caller-owned device blob whose layout is a pure function of the config, so a multi-GPU host can broadcast
// it with a single RCCL call.
#include "graphs.h"
#include <dlfcn.h>
#include <array>
#include <cstring>

namespace {

thread_local std::string g_err;
int fail(const std::string& m) { g_err = m; return -1; }

}  // namespace

// Test hook, compiled ONLY into the test-hooks library (-DRS_TEST_HOOKS: resshift_amd.build.build_testhooks(), loaded by tests/_fake_device_plumbing.py
// alone - the production libresshift_hip.so does not contain it): with RS_FAKE_DEVICE=1 on a host WITHOUT a HIP device the engine's real pass walks
// its control flow on a host-memory arena while every launch fails - a CPU test compares its bookkeeping with the dry pass.
#ifdef RS_TEST_HOOKS
static bool rs_fake_device() {
    static const bool fake = []() {
        if (!rs_env_set("RS_FAKE_DEVICE")) return false;
        int n = 0;
        const hipError_t e = hipGetDeviceCount(&n);
        // (only the definite answer "this host has no HIP device" enables the hook - a driver hiccup on a GPU box must not)
        return e == hipErrorNoDevice || (e == hipSuccess && n == 0);
    }();
    return fake;
}
#else
static constexpr bool rs_fake_device() { return false; }
#endif

struct rs_engine : Model {
    Graphs g{*this};
    bool bound = false, ready = false;
    bool split_ok = true;   // (the verdict travels IN the blob - first word of a 256-byte header - so ranks that receive the blob by broadcast know it too)
    Arena arena;
    long long last_launches = 0;
    Exec::Prof prof, prof_gn;
    double last_flops[3] = {0.0, 0.0, 0.0}, last_igemm_ms = 0.0, last_igemm_bytes = 0.0, last_gn_ms = 0.0, last_gn_bytes = 0.0;
    double last_fam[Exec::F_COUNT][3] = {};   // flops, ms, launches per kernel family
    std::string last_shapes;                  // rs_profile_shapes: one line per (part, family, M, N, K) and per part of the last profiled call
    long long last_igemm_launches = 0, last_gn_launches = 0;
    bool debug = false;
    std::vector<TraceRec> trace;                        // records of the last traced call (Exec::tr)
    // per-request seeds (philox.h): the keys of a seeded batch of more than RS_MAX_ROWS images, copied to the device once per call
    // The copy does not wait for the stream (a blocking copy would hold the host until everything queued before the call has run): the
    // keys go through a pinned staging array, and an event says when the previous call's copy has read it.
    rs_noise_key* keys_dev = nullptr; rs_noise_key* keys_pin = nullptr; size_t keys_cap = 0;
    hipEvent_t keys_ev = nullptr; bool keys_ev_set = false;
    void free_keys() {
        if (keys_dev) (void)hipFree(keys_dev);
        if (keys_pin) (void)hipHostFree(keys_pin);
        if (keys_ev) (void)hipEventDestroy(keys_ev);
        keys_dev = keys_pin = nullptr; keys_cap = 0; keys_ev = nullptr; keys_ev_set = false;
    }
    const rs_noise_key* stage_keys(const rs_noise_key* keys, int B, hipStream_t st) {
        if (rs_fake_device()) return (const rs_noise_key*)(uintptr_t)4096;   // (never dereferenced: every launch fails there)
        const size_t bytes = (size_t)B * sizeof(rs_noise_key);
        if ((size_t)B > keys_cap) {
            (void)hipStreamSynchronize(st);
            if (keys_ev_set) (void)hipEventSynchronize(keys_ev);
            free_keys();
            if (hipMalloc((void**)&keys_dev, bytes) != hipSuccess || hipHostMalloc((void**)&keys_pin, bytes, hipHostMallocDefault) != hipSuccess ||
                hipEventCreateWithFlags(&keys_ev, hipEventDisableTiming) != hipSuccess) { free_keys(); return nullptr; }
            keys_cap = (size_t)B;
        }
        if (keys_ev_set) (void)hipEventSynchronize(keys_ev);   // the previous call's copy has left the staging array (long done in a serial caller)
        memcpy(keys_pin, keys, bytes);                          // (the caller's host array may go away on return)
        // stream-ordered: an earlier call's kernels on this stream no longer read the device buffer when the copy lands
        if (hipMemcpyAsync(keys_dev, keys_pin, bytes, hipMemcpyHostToDevice, st) != hipSuccess) return nullptr;
        keys_ev_set = hipEventRecord(keys_ev, st) == hipSuccess;
        if (!keys_ev_set) (void)hipStreamSynchronize(st);
        return keys_dev;
    }
    char* cap_base = nullptr; size_t cap_bytes = 0; bool cap_host = false;   // their capture region (run(); freed by rs_debug_enable(0))
    void free_capture() {
        if (cap_base) { if (cap_host) free(cap_base); else (void)hipFree(cap_base); }
        cap_base = nullptr; cap_bytes = 0; trace.clear();
    }
    std::vector<TailPlan> tail_plan;   // made by the dry pass of a call, read by its real pass (Exec::plan)
    // ---------------------------------------------------------------- FiLM cache
    // emb = time_embed(timestep_embedding(t)) (unet.py:874, basic_ops.py:99-117); per ResBlock
    // emb_out = Linear(SiLU(emb)) (unet.py:161-167,195).  Row layout: [film_total], block r at r.film_off.
    std::map<int, float*> film_cache;
    void drop_film_cache() { for (auto& kv : film_cache) (void)hipFree(kv.second); film_cache.clear(); }
    const float* film_row(int t, hipStream_t st) {
        auto it = film_cache.find(t);
        if (it != film_cache.end()) return it->second;
        if (rs_fake_device()) { film_cache[t] = (float*)malloc((size_t)film_total * 4); return film_cache[t]; }   // (plumbing check without a GPU, see run())
        const int mc = cfg.unet.model_channels, half = mc / 2, emb_ch = 4 * mc;
        std::vector<float> e0(mc, 0.f);
        for (int k = 0; k < half; ++k) {
            const float freq = expf((float)(-std::log(10000.0)) * (float)k / (float)half);
            const float arg = (float)t * freq;
            e0[k] = cosf(arg); e0[half + k] = sinf(arg);
        }
        float *d0, *d1, *d2, *row;
        if (hipMalloc(&d0, mc * 4) != hipSuccess || hipMalloc(&d1, emb_ch * 4) != hipSuccess || hipMalloc(&d2, emb_ch * 4) != hipSuccess ||
            hipMalloc(&row, (size_t)film_total * 4) != hipSuccess)
            return nullptr;
        (void)hipMemcpyAsync(d0, e0.data(), mc * 4, hipMemcpyHostToDevice, st);
        (void)hipStreamSynchronize(st);  // e0 is a stack-lifetime host buffer
        rs_small_linear_launch(d0, te0.wd, te0.bias, d1, 1, mc, emb_ch, 0, 1, st);
        rs_small_linear_launch(d1, te2.wd, te2.bias, d2, 1, emb_ch, emb_ch, 0, 0, st);
        for (ResBlockW* r : film_blocks) rs_small_linear_launch(d2, r->emb.wd, r->emb.bias, row + r->film_off, 1, emb_ch, 2 * r->Cout, 1, 0, st);
        (void)hipStreamSynchronize(st);
        (void)hipFree(d0); (void)hipFree(d1); (void)hipFree(d2);
        film_cache[t] = row;
        return row;
    }
    // ---------------------------------------------------------------- run helper (dry sizing pass, then real pass)
    int run(hipStream_t st, const std::function<void(Exec&)>& fn) {
        if (!ready) return fail("weights are not ready (rs_pack_weights / rs_weights_ready not called)");
        Exec d; d.st = st; d.arena = &arena; d.dry = true; d.tracing = debug;
        tail_plan.clear();
        d.plan = &tail_plan;
        d.pool_base = (char*)4096;   // never dereferenced; non-null so that "has statistics" (View::st != nullptr) reads the same in both passes
        d.ticket_base = (unsigned*)4096;
        arena.off = 0; arena.peak = 0;
        fn(d);
        if (d.err) { last_launches = 0; return d.err; }   // refused while planning (Exec::fail has the text, e.g. an operand over RS_BUFFER_BYTES_LIMIT): nothing was launched
        if (d.used_split && !(cfg.enable_split && split_ok))
            return fail(!cfg.enable_split ? "split precision requested but the engine was created without enable_split"
                                          : "split precision is not available for these weights: " +
                                                (split_err.empty() ? std::string("a non-finite or out-of-fp16-range conv / linear weight (the packing rank has its name)") : split_err));
        // behind the scratch arena: the GroupNorm coefficient pool and the tails' tickets (gn_tail.h), sized by the dry pass
        const size_t scratch_end = (arena.peak + 255) & ~(size_t)255;
        const size_t pool_bytes = (d.pool_peak + 255) & ~(size_t)255, ticket_bytes = d.ticket_used * sizeof(unsigned);
        const size_t need = scratch_end + pool_bytes + ticket_bytes + 4096;
        // RS_FAKE_DEVICE=1 (plumbing check in a container without a GPU): the scratch arena comes from host memory and every launch simply
        // fails, but the real pass walks its whole control flow - enough to check that it agrees with the dry pass about pools and tickets
        const bool fake = rs_fake_device();
        if (fake && need > arena.cap) { arena.base = (char*)malloc(64); arena.cap = (size_t)1 << 62; }
        if (need > arena.cap) {
            (void)hipStreamSynchronize(st);
            if (arena.base) (void)hipFree(arena.base);
            arena.base = nullptr; arena.cap = 0;
            const size_t want = need + need / 8;
            if (hipMalloc((void**)&arena.base, want) != hipSuccess) return fail("hipMalloc of scratch arena failed (" + std::to_string(want) + " bytes)");
            arena.cap = want;
        }
        // the debug trace's capture region (sized by the dry pass; allocated only while tracing is on, apart from everything above)
        trace.clear();
        if (debug && d.cap_off > cap_bytes) {
            if (cap_base) {
                (void)hipStreamSynchronize(st);
                if (cap_host) free(cap_base); else (void)hipFree(cap_base);
            }
            cap_base = nullptr; cap_bytes = 0;
            cap_host = fake;   // (RS_FAKE_DEVICE: host memory, as the arena there)
            if (fake) cap_base = (char*)malloc(d.cap_off);
            else if (hipMalloc((void**)&cap_base, d.cap_off) != hipSuccess) cap_base = nullptr;
            if (!cap_base) return fail("allocation of the debug trace's capture region failed (" + std::to_string(d.cap_off) + " bytes)");
            cap_bytes = d.cap_off;
        }
        Exec r; r.st = st; r.arena = &arena; r.dry = false; r.tracing = debug;
        if (debug) { r.trace = &trace; r.cap_base = cap_base; }
        r.plan = &tail_plan;
        r.pool_base = arena.base + scratch_end;
        r.ticket_base = (unsigned*)(arena.base + scratch_end + pool_bytes);
        if (!fake && ticket_bytes && hipMemsetAsync(r.ticket_base, 0, ticket_bytes, st) != hipSuccess) return fail("hipMemsetAsync of the ticket pool failed");
        arena.off = 0; arena.peak = 0;
        r.prof = &prof; prof.used = 0;
        r.prof_gn = &prof_gn; prof_gn.used = 0; prof_gn.on = prof.on;
        fn(r);
        if (fake) fprintf(stderr, "[fake device] dry: tickets %zu pool %zu prod %d gn %d | real: tickets %zu pool %zu prod %d gn %d launches %lld\n", d.ticket_used,
                          d.pool_peak, d.prod_seq, d.gn_seq, r.ticket_used, r.pool_peak, r.prod_seq, r.gn_seq, r.launches);
        for (size_t k = 0; k < tail_plan.size(); ++k)
            if (tail_plan[k].on && !tail_plan[k].drawn) {
                if (fake) fprintf(stderr, "[fake device] planned tail of producer %zu (C %d, HW %d, consumer GroupNorm %d) was never attached\n", k, tail_plan[k].C, tail_plan[k].HW, tail_plan[k].consumer);
                r.err = -4; g_err = "internal: a planned GroupNorm tail was never attached to its producer";
            }
        if (r.ticket_used != d.ticket_used || r.pool_peak != d.pool_peak) { r.err = -4; g_err = "internal: dry and real pass disagree about the GroupNorm tail plan"; }
        if (r.cap_off != d.cap_off) { r.err = -4; g_err = "internal: dry and real pass disagree about the debug trace's capture region"; }
        last_launches = r.launches + (ticket_bytes ? 1 : 0);   // (the network's launches: the trace's capture copies are not counted here)
        last_flops[0] = r.igemm_flops[0]; last_flops[1] = r.igemm_flops[1]; last_flops[2] = r.igemm_flops[2]; last_igemm_launches = r.igemm_launches;
        last_igemm_bytes = r.igemm_bytes;
        last_igemm_ms = 0.0;
        last_gn_ms = 0.0; last_gn_bytes = r.gn_bytes; last_gn_launches = r.gn_launches;
        for (int f = 0; f < Exec::F_COUNT; ++f) { last_fam[f][0] = r.fam_flops[f]; last_fam[f][1] = 0.0; last_fam[f][2] = (double)r.fam_launches[f]; }
        if (prof.on && prof.used) {
            // The event pair itself costs stream time (two marker packets bracket every launch): measure that cost with
            // empty pairs on the same stream and take it out, so that the per-launch figure is the kernel's own duration
            // (checked against the rocprofv3 kernel trace of the same command).
            constexpr int NCAL = 32;
            hipEvent_t cal[2 * NCAL];
            for (auto& ev : cal) (void)hipEventCreate(&ev);
            for (int i = 0; i < NCAL; ++i) { (void)hipEventRecord(cal[2 * i], st); (void)hipEventRecord(cal[2 * i + 1], st); }
            (void)hipStreamSynchronize(st);
            std::vector<float> empty(NCAL);
            for (int i = 0; i < NCAL; ++i) { empty[i] = 0.f; (void)hipEventElapsedTime(&empty[i], cal[2 * i], cal[2 * i + 1]); }
            for (auto& ev : cal) (void)hipEventDestroy(ev);
            std::sort(empty.begin(), empty.end());
            const float overhead = empty[NCAL / 2];   // median
            auto span = [&](const Exec::Prof& p, size_t i) {   // kernel milliseconds of the bracket whose events are i, i + 1
                float ms = 0.f;
                (void)hipEventElapsedTime(&ms, p.ev[i], p.ev[i + 1]);
                return std::max(0.f, ms - overhead);
            };
            for (size_t i = 0; i + 1 < prof.used; i += 2) {
                last_igemm_ms += span(prof, i);
                if (i / 2 < r.fam_of.size()) last_fam[r.fam_of[i / 2]][1] += span(prof, i);
            }
            if (!r.tag_of.empty()) {
                std::map<std::string, std::array<double, 3>> agg;
                for (size_t i = 0; i + 1 < prof.used && i / 2 < r.tag_of.size(); i += 2) {
                    auto& a = agg[r.tag_of[i / 2]];
                    a[0] += span(prof, i); a[1] += 1.0; a[2] += r.tag_flops[i / 2];
                }
                std::vector<std::pair<double, std::string>> rows;
                last_shapes.clear();
                for (auto& kv : agg) {
                    char b[200]; snprintf(b, sizeof b, "%-40s n=%4.0f  %8.3f ms  %7.1f us/launch  %7.1f TF/s", kv.first.c_str(), kv.second[1], kv.second[0],
                                          1e3 * kv.second[0] / kv.second[1], kv.second[2] / (kv.second[0] * 1e-3) / 1e12);
                    rows.emplace_back(-kv.second[0], b);
                    char c[200]; snprintf(c, sizeof c, "shape %s n=%.0f ms=%.4f flops=%.6e\n", kv.first.c_str(), kv.second[1], kv.second[0], kv.second[2]);
                    last_shapes += c;
                }
                std::sort(rows.begin(), rows.end());
                static const bool shapes = rs_env_set("RS_PROF_SHAPES");
                if (shapes) for (auto& rw : rows) fprintf(stderr, "[shapes] %s\n", rw.second.c_str());
            }
            // wall time of the parts (events at every change of part, the call's end closes the last one)
            if (!r.part_marks.empty()) {
                hipEvent_t endev = nullptr;
                (void)hipEventCreate(&endev); (void)hipEventRecord(endev, st); (void)hipEventSynchronize(endev);
                std::map<std::string, double> pm; std::vector<std::string> order;
                for (size_t i = 0; i < r.part_marks.size(); ++i) {
                    float ms = 0.f;
                    (void)hipEventElapsedTime(&ms, r.part_marks[i].second, i + 1 < r.part_marks.size() ? r.part_marks[i + 1].second : endev);
                    if (!pm.count(r.part_marks[i].first)) order.push_back(r.part_marks[i].first);
                    pm[r.part_marks[i].first] += ms;
                }
                for (auto& nm : order) { char c[96]; snprintf(c, sizeof c, "part %s ms=%.4f\n", nm.c_str(), pm[nm]); last_shapes += c; }
                (void)hipEventDestroy(endev);
            }
            for (size_t i = 0; i + 1 < prof_gn.used; i += 2) last_gn_ms += span(prof_gn, i);
        }
        for (auto& pmk : r.part_marks) (void)hipEventDestroy(pmk.second);
        if (r.err) return r.err;
        return 0;
    }
};

// ==================================================================== C ABI
extern "C" {

const char* rs_last_error(void) { return g_err.c_str(); }
// (internal, not in the header: the entry points of the other translation units report their argument errors through this)
int rs_set_last_error(const char* text, int rc) { g_err = text; return rc; }

rs_engine* rs_create(const rs_config* cfg) {
    if (!cfg) { g_err = "null config"; return nullptr; }
    const rs_unet_config& u = cfg->unet;
    if (!cfg->has_unet && !cfg->has_ae) { g_err = "config has neither a UNet nor an autoencoder"; return nullptr; }
    if (cfg->has_unet) {
        if (u.window_size != 8) { g_err = "only window_size 8 is supported"; return nullptr; }
        if (u.num_heads < 1 || u.swin_embed_dim != u.num_heads * 32) { g_err = "swin_embed_dim / num_head_channels: the swin head dim must be 32"; return nullptr; }
        if (u.n_levels < 1 || u.n_levels > RS_MAX_LEVELS) { g_err = "bad n_levels"; return nullptr; }
        if ((u.image_size >> (u.n_levels - 1)) < 8) { g_err = "image_size / channel_mult: the coarsest UNet level must be >= 8x8"; return nullptr; }
    }
    if (cfg->has_ae && cfg->ae.n_attn_res != 0) { g_err = "AE attn_resolutions must be empty"; return nullptr; }
    if (cfg->has_ae) {
        // what the VQ search (elementwise.hip: rs_vq_launch) is instantiated for and keeps in LDS: refused here, not at the first decode
        const rs_ae_config& a = cfg->ae;
        if (a.embed_dim != 3 && a.embed_dim != 4 && a.embed_dim != 8) { g_err = "AE embed_dim must be 3, 4 or 8 (the VQ search kernel)"; return nullptr; }
        if (a.n_embed < 1 || (long long)a.n_embed * (a.embed_dim + 1) * 4 > 160 * 1024) {
            g_err = "AE n_embed: the codebook and its norms, n_embed * (embed_dim + 1) * 4 bytes, must fit 160 KiB of LDS"; return nullptr;
        }
    }
    if (!cfg->enable_f16 && !cfg->enable_f32 && !cfg->enable_split) { g_err = "enable at least one precision"; return nullptr; }
    rs_engine* e = new rs_engine();
    e->cfg = *cfg;
    e->blob_bytes = e->build(nullptr, false);
    return e;
}

void rs_destroy(rs_engine* e) {
    if (!e) return;
    if (!rs_fake_device()) {
        for (auto& kv : e->film_cache) (void)hipFree(kv.second);
        if (e->arena.base) (void)hipFree(e->arena.base);
        e->free_keys();
    }
    e->free_capture();
    delete e;
}

int rs_load_tensor(rs_engine* e, const char* key, const float* host, const int64_t* shape, int ndim) {
    if (!e || !key || !host) return fail("rs_load_tensor: null argument");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.data.assign(host, host + n);
    e->host[key] = std::move(t);
    return 0;
}

size_t rs_weight_bytes(rs_engine* e) { return e ? e->blob_bytes : 0; }

int rs_bind_weight_blob(rs_engine* e, void* dev, size_t bytes) {
    if (!e || !dev) return fail("rs_bind_weight_blob: null argument");
    if (bytes < e->blob_bytes) return fail("weight blob too small");
    if (((uintptr_t)dev & 255) != 0) return fail("weight blob must be 256-byte aligned");
    e->build((char*)dev, false);  // resolve pointers
    e->collect_film_blocks();
    e->bound = true; e->ready = false;
    e->drop_film_cache();
    return 0;
}

// Broadcast the bound weight blob from rank `root` over an RCCL communicator the HOST owns (sampler.py:66-77: the reference's
// ranks each load the checkpoint - here rank 0 packs once and the blob travels over xGMI).  `rccl_comm` is an ncclComm_t; RCCL is looked up at
// call time (dlopen of librccl.so - the library has no link-time dependency on it: a single-GPU host never needs it).  One ncclBroadcast of
// rs_weight_bytes() bytes on `stream`, in place; the caller then calls rs_weights_ready() on every rank.  (The Python host mirror broadcasts the
// same buffer through torch.distributed, backend nccl = RCCL: resshift_amd/sharding.py.)
int rs_bcast_weights(rs_engine* e, void* rccl_comm, int root, void* stream) {
    if (!e || !e->bound || !rccl_comm) return fail("rs_bcast_weights: bind a weight blob first and pass an RCCL communicator");
    typedef int (*bcast_t)(const void*, void*, size_t, int, int, void*, hipStream_t);
    static bcast_t fn = []() -> bcast_t {
        void* h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        return h ? (bcast_t)dlsym(h, "ncclBroadcast") : nullptr;
    }();
    if (!fn) return fail("rs_bcast_weights: librccl.so (ncclBroadcast) not found");
    const int rc = fn(e->blob.base, e->blob.base, e->blob_bytes, /* ncclUint8 */ 1, root, rccl_comm, (hipStream_t)stream);
    if (rc != 0) return fail("rs_bcast_weights: ncclBroadcast failed (ncclResult_t " + std::to_string(rc) + ")");
    e->ready = false;   // (the receiving ranks' flags are read back by rs_weights_ready)
    // rs_weights_ready reads the blob header and the per-layer flags with copies that wait for no caller stream: the received bytes must be
    // there when this call returns (once per process; a non-blocking stream would otherwise leave a window for a stale read)
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return fail("rs_bcast_weights: the broadcast did not complete on its stream");
    return 0;
}

int rs_pack_weights(rs_engine* e) {
    if (!e || !e->bound) return fail("rs_pack_weights: bind a weight blob first");
    char* base = e->blob.base;
    e->build(base, true);
    e->collect_film_blocks();
    if (!e->build_err.empty()) { e->blob.staging.clear(); e->blob.staging.shrink_to_fit(); return fail(e->build_err); }
    e->split_ok = e->split_err.empty();
    {
        const uint32_t flags = e->split_ok ? 1u : 0u;
        memcpy(e->blob.staging.data(), &flags, sizeof flags);
    }
    if (hipMemcpy(base, e->blob.staging.data(), e->blob_bytes, hipMemcpyHostToDevice) != hipSuccess) return fail("hipMemcpy of weight blob failed");
    e->blob.staging.clear(); e->blob.staging.shrink_to_fit();
    e->blob.fill = false;
    e->host.clear();
    e->drop_film_cache();
    e->ready = true;
    return 0;
}

int rs_weights_ready(rs_engine* e) {
    if (!e || !e->bound) return fail("rs_weights_ready: bind a weight blob first");
    uint32_t flags = 0;   // header word of the blob (packed here, read from a cache file, or received by broadcast)
    if (rs_fake_device()) { e->split_ok = true; e->ready = true; return 0; }   // (plumbing check without a GPU, see run())
    if (hipMemcpy(&flags, e->blob.base, sizeof flags, hipMemcpyDeviceToHost) != hipSuccess) return fail("rs_weights_ready: cannot read the blob header");
    e->split_ok = (flags & 1u) != 0;
    if (e->conv_count > 0 && e->big_w_dev &&
        hipMemcpy(e->big_w.data(), e->big_w_dev, (size_t)e->conv_count, hipMemcpyDeviceToHost) != hipSuccess) return fail("rs_weights_ready: cannot read the per-layer flags");
    e->drop_film_cache();
    e->ready = true;
    return 0;
}

size_t rs_arena_bytes(rs_engine* e) { return e ? e->arena.cap : 0; }

// ---- profiling of the MFMA implicit-GEMM kernel family (bench.py roofline block)
int rs_profile_enable(rs_engine* e, int on) { if (!e) return -1; e->prof.on = on != 0; return 0; }
// out[0] = fp16-input igemm FLOPs of the last call, out[1] = fp32-input igemm FLOPs, out[2] = summed igemm kernel
// time in ms (hipEvents on the launch stream; 0 unless profiling was enabled), out[3] = igemm launch count,
// out[4] = algorithmic HBM bytes of those launches (each operand / result counted once), out[5] = split-input igemm FLOPs,
// out[6..8] = GroupNorm family: summed kernel ms (events as above), launch count (one per GroupNorm), algorithmic bytes
int rs_profile_get(rs_engine* e, double* out) {
    if (!e || !out) return -1;
    out[0] = e->last_flops[0]; out[1] = e->last_flops[1]; out[2] = e->last_igemm_ms; out[3] = (double)e->last_igemm_launches;
    out[4] = e->last_igemm_bytes; out[5] = e->last_flops[2];
    out[6] = e->last_gn_ms; out[7] = (double)e->last_gn_launches; out[8] = e->last_gn_bytes;
    return 0;
}

// per kernel family of the MFMA path, in the order of Exec::Fam: halo conv fp16 (igemm4), halo conv split, implicit GEMM fp16 (igemm2 /
// igemm3 / igemm), implicit GEMM split, implicit GEMM fp32, fused qkv + window attention + projection, fused Swin MLP, their
// split-storage variants, streaming AE attention and its split variant, Winograd conv (split).  A conv launch is booked under the family
// of the kernel its plan names (ConvPlan::kernel), so the launch counts are the routing decisions:
// out[3 f + 0] = algorithmic FLOPs, out[3 f + 1] = kernel ms (0 unless profiling was on), out[3 f + 2] = launches.  Returns the family count.
int rs_profile_families(rs_engine* e, double* out, int cap) {
    if (!e || !out || cap < 3 * Exec::F_COUNT) return -1;
    for (int f = 0; f < Exec::F_COUNT; ++f) { out[3 * f] = e->last_fam[f][0]; out[3 * f + 1] = e->last_fam[f][1]; out[3 * f + 2] = e->last_fam[f][2]; }
    return Exec::F_COUNT;
}

// Text table of the last PROFILED call (rs_profile_enable): one line per distinct launch shape of the MFMA family,
//   "shape <part> f<family> M=.. N=.. K=.. z=.. n=<launches> ms=<summed kernel ms> flops=<algorithmic flops>"
// (part = encoder / unet / decoder; family numbering as rs_profile_families), then one line per part, "part <name> ms=<wall ms between the
// part's first launch and the next part's>" (every kernel of the part, whatever its family).  Returns the length needed (incl. the
// terminating 0); copies at most cap bytes.
int rs_profile_shapes(rs_engine* e, char* buf, int cap) {
    if (!e) return -1;
    const int need = (int)e->last_shapes.size() + 1;
    if (buf && cap > 0) { const int n = std::min(cap - 1, need - 1); memcpy(buf, e->last_shapes.data(), n); buf[n] = 0; }
    return need;
}

// ---- debug trace (tests only): named intermediate activations of the next network calls, copied as they are produced (Exec::tr)
int rs_debug_enable(rs_engine* e, int on) {
    if (!e) return -1;
    e->debug = on != 0;
    if (!e->debug) {
        if (e->cap_base && !e->cap_host) (void)hipDeviceSynchronize();   // (copies of the last traced call may still be in flight)
        e->free_capture();
    }
    e->trace.clear();
    return 0;
}
int rs_debug_count(rs_engine* e) { return e ? (int)e->trace.size() : 0; }
int rs_debug_info(rs_engine* e, int i, char* name, int cap, int* dims /* B,C,H,W */) {
    if (!e || i < 0 || i >= (int)e->trace.size()) return -1;
    const TraceRec& t = e->trace[i];
    snprintf(name, cap, "%s", t.name.c_str());
    dims[0] = t.B; dims[1] = t.C; dims[2] = t.H; dims[3] = t.W;
    return 0;
}
int rs_debug_fetch(rs_engine* e, int i, float* out_nchw, void* stream) {
    if (!e || i < 0 || i >= (int)e->trace.size() || !e->cap_base) return -1;
    const TraceRec& t = e->trace[i];
    const size_t bytes = (size_t)t.B * t.C * t.H * t.W * sizeof(float);
    return hipMemcpyAsync(out_nchw, e->cap_base + t.off, bytes, hipMemcpyDefault, (hipStream_t)stream) == hipSuccess ? 0 : -1;
}
int rs_debug_fetch_rows(rs_engine* e, int i, int b0, int nb, float* out_nchw, void* stream) {
    if (!e || i < 0 || i >= (int)e->trace.size() || !e->cap_base) return -1;
    const TraceRec& t = e->trace[i];
    if (b0 < 0 || nb < 1 || b0 > t.B - nb) return -2;
    const size_t per = (size_t)t.C * t.H * t.W * sizeof(float);
    return hipMemcpyAsync(out_nchw, e->cap_base + t.off + (size_t)b0 * per, (size_t)nb * per, hipMemcpyDefault, (hipStream_t)stream) == hipSuccess ? 0 : -1;
}
long long rs_last_launch_count(rs_engine* e) { return e ? e->last_launches : 0; }

int rs_unet_forward(rs_engine* e, const float* x, const int* t_host, const float* lq, const float* mask, float* out, int B, int H, int W,
                    int Hl, int Wl, int prec, void* stream) {
    if (!e || !e->cfg.has_unet) return fail("engine has no UNet");
    {
        const int sh = e->cfg.unet.n_levels - 1;
        if ((H % (8 << sh)) || (W % (8 << sh))) return fail("UNet input H/W must be multiples of 8*2^(levels-1)");
    }
    hipStream_t st = (hipStream_t)stream;
    if (!e->ready) return fail("weights are not ready");
    if (B < 1 || !x || !out || !t_host) return fail("rs_unet_forward: bad batch / null tensor");
    if (e->cfg.unet.cond_lq && !lq) return fail("rs_unet_forward: this UNet is conditioned on lq (cond_lq) but lq is NULL");
    if (e->cfg.unet.cond_mask && !mask) return fail("rs_unet_forward: this UNet is conditioned on a mask (cond_mask) but mask is NULL");
    if (e->cfg.unet.cond_lq && e->fe_convs.empty() && (Hl != H || Wl != W))
        return fail("rs_unet_forward: without a feature extractor lq must have the latent resolution");
    if (!e->fe_convs.empty() && ((Hl >> (int)e->fe_convs.size()) != H || (Wl >> (int)e->fe_convs.size()) != W))
        return fail("rs_unet_forward: lq resolution does not match the feature extractor's down-sampling");
    bool mixed = false;
    for (int b = 1; b < B; ++b) mixed |= t_host[b] != t_host[0];
    if (mixed && B > RS_MAX_ROWS) return fail("rs_unet_forward: unequal timesteps in a batch of more than RS_MAX_ROWS (" + std::to_string(RS_MAX_ROWS) + ") images");
    // FiLM: the cached row of the batch's timestep, or (unequal timesteps) one row per image gathered from the cached rows
    std::vector<const float*> rows(mixed ? B : 1);
    for (size_t b = 0; b < rows.size(); ++b)
        if (!(rows[b] = e->film_row(t_host[b], st))) return fail("FiLM table allocation failed");
    return e->run(st, [&](Exec& ex) {
        View feat; const View* fp = nullptr;
        if (!e->fe_convs.empty()) { feat = e->g.feature_extract(ex, lq, mask, B, Hl, Wl, prec); fp = &feat; }
        Graphs::UNetCall u{};
        u.x = x; u.xscale = 1.0f; u.lq_feat = fp; u.lq_nchw = lq; u.mask_nchw = mask; u.out = out; u.B = B; u.H = H; u.W = W; u.dt = prec;
        u.film = mixed ? e->g.film_table(ex, rows.data(), B) : rows[0];
        u.film_ld = mixed ? e->film_total : 0;
        e->g.unet_body(ex, u);
    });
}

int rs_vq_encode(rs_engine* e, const float* img, float* z, int B, int H, int W, int prec, void* stream) {
    if (!e || !e->cfg.has_ae) return fail("engine has no autoencoder");
    hipStream_t st = (hipStream_t)stream;
    return e->run(st, [&](Exec& ex) {
        View in = ex.T(B, H, W, e->enc_in.CinP, prec);  // RGB zero-padded to 8 channels in the working precision
        e->g.zero(ex, in);
        if (!ex.dry) ex.check(rs_nchw_to_nhwc_launch(img, in.p, prec, B, e->cfg.ae.in_channels, H * W, in.ld, 0, 1.f, st), "img->nhwc");
        e->g.encode_body(ex, in, z, prec);
    });
}

int rs_vq_decode(rs_engine* e, const float* z, float* img, int32_t* idx_out, int B, int h, int w, int force_not_quantize, int prec,
                 void* stream) {
    if (!e || !e->cfg.has_ae) return fail("engine has no autoencoder");
    hipStream_t st = (hipStream_t)stream;
    return e->run(st, [&](Exec& ex) { e->g.decode_body(ex, Graphs::DecodeCall{z, 1.0f, img, idx_out, B, h, w, force_not_quantize, prec}); });
}

int rs_bicubic(rs_engine* e, const float* y, float* out, int B, int C, int H, int W, int sf, void* stream) {
    if (!e) return fail("null engine");
    hipStream_t st = (hipStream_t)stream;
    const bool was_ready = e->ready;
    e->ready = true;  // no weights involved
    const int rc = e->run(st, [&](Exec& ex) {
        View t = ex.T(B, H * sf, W * sf, C, RS_F32);
        if (ex.dry) return;
        ex.check(rs_bicubic_launch(y, t.p, RS_F32, B, C, H, W, sf, t.ld, st), "bicubic");
        ex.check(rs_nhwc_to_nchw_launch(t.p, RS_F32, out, B, C, H * sf * W * sf, t.ld, 0, st), "bicubic->nchw");
    });
    e->ready = was_ready;
    return rc;
}

int rs_axpbypcz(const float* x, const float* z, const float* n, float* y, float a, float b, float c, long long count, void* stream) {
    return rs_axpbypcz_launch(x, z, n, y, a, b, c, count, (hipStream_t)stream);
}

int rs_axpbypcz_rows(const float* x, const float* z, const float* n, float* y, const float* a, const float* b, const float* c, long long per_image_count,
                     int B, void* stream) {
    if (B < 1 || B > RS_MAX_ROWS) return fail("rs_axpbypcz_rows: B must be 1 .. RS_MAX_ROWS (" + std::to_string(RS_MAX_ROWS) + ")");
    if (!x || !y || !a || per_image_count < 1) return fail("rs_axpbypcz_rows: null tensor / coefficients or empty image");
    if ((z && !b) || (n && !c)) return fail("rs_axpbypcz_rows: a z / n operand needs its b / c coefficients");
    const int rc = rs_axpbypcz_rows_launch(x, z, n, y, a, b, c, per_image_count, B, (hipStream_t)stream);
    return rc ? fail("rs_axpbypcz_rows: launch failed") : 0;
}

// checks shared by rs_sample / rs_sample_begin / rs_sample_end: the batch geometry and the conditioning; "" when fine
static std::string sample_args_error(rs_engine* e, const rs_sample_args* a, bool encode, bool decode) {
    if (!e || !a) return "null argument";
    if (!e->cfg.has_ae || !e->cfg.has_unet) return "the sampling loop needs both the UNet and the autoencoder";
    auto bad = [](int p) { return p != RS_F16 && p != RS_F32 && p != RS_F16S; };
    if ((encode && bad(a->prec_encode)) || (decode && bad(a->prec_decode))) return "bad precision";
    if (!e->ready) return "weights are not ready";
    const int f = e->g.latent_div(), Hi = a->h * a->sf, Wi = a->w * a->sf, hz = Hi / f, wz = Wi / f;
    if (e->cfg.unet.in_channels != e->cfg.ae.embed_dim) return "UNet in_channels != AE embed_dim";
    if (a->B < 1 || a->h < 1 || a->w < 1 || a->sf < 1) return "bad batch / size";
    if ((Hi % f) || (Wi % f)) return "h*sf and w*sf must be multiples of the autoencoder's down-sampling factor";
    const int sh = e->cfg.unet.n_levels - 1;
    if ((hz % (8 << sh)) || (wz % (8 << sh))) return "latent H/W must be multiples of 8*2^(levels-1) (pad the input, sampler.py:130-138)";
    if (e->cfg.unet.cond_lq && e->fe_convs.empty() && (a->h != hz || a->w != wz))
        return "without a feature extractor the LQ image is concatenated at latent resolution: h*sf/f must equal h";
    if (encode && !a->y) return "null tensor (y)";
    if (decode && !a->out) return "null tensor (out)";
    return "";
}

// gaussian_diffusion.py:367-472: encode_first_stage(up_sample) -> prior_sample -> T x p_sample -> decode_first_stage
// what the seeded entry points ask of their keys (house style of the by-value calls: -2 and rs_last_error's text); 0 when fine
static int noise_keys_check(const char* who, const rs_noise_key* keys, int B) {
    if (!keys) return rs_set_last_error((std::string(who) + ": null keys").c_str(), -2);
    if (B < 1 || B > 65535) return rs_set_last_error((std::string(who) + ": B must be 1 .. 65535").c_str(), -2);
    for (int b = 0; b < B; ++b)
        if (keys[b].reserved != 0) return rs_set_last_error((std::string(who) + ": keys[" + std::to_string(b) + "].reserved is not 0").c_str(), -2);
    return 0;
}

// rs_sample (keys == nullptr: a->noise) and rs_sample_seeded (keys: a->noise is ignored)
static int sample_impl(rs_engine* e, const rs_sample_args* a, const rs_noise_key* keys) {
    if (!e || !a) return fail("null argument");
    if (a->steps < 1 || a->steps > RS_MAX_STEPS) return fail("bad step count");
    for (int i = 0; i < a->steps; ++i) if (a->prec_unet[i] != RS_F16 && a->prec_unet[i] != RS_F32 && a->prec_unet[i] != RS_F16S) return fail("bad precision");
    {
        const std::string err = sample_args_error(e, a, true, true);
        if (!err.empty()) return fail("rs_sample: " + err);
    }
    if (!keys && !a->noise) return fail("rs_sample: bad batch / size / null tensor");
    if (e->cfg.unet.cond_mask && !a->mask) return fail("rs_sample: this UNet is conditioned on a mask (cond_mask) but mask is NULL");
    hipStream_t st = (hipStream_t)a->stream;
    const int B = a->B, f = e->g.latent_div(), hz = a->h * a->sf / f, wz = a->w * a->sf / f;
    std::vector<const float*> films(a->steps);
    for (int t = 0; t < a->steps; ++t) {
        films[t] = e->film_row(a->tmap[t], st);
        if (!films[t]) return fail("FiLM table allocation failed");
    }
    const long long zcount = (long long)B * e->cfg.ae.embed_dim * hz * wz;
    const rs_noise_key* kd = nullptr;
    if (keys && B > RS_MAX_ROWS && !(kd = e->stage_keys(keys, B, st))) return fail("rs_sample_seeded: device copy of the keys failed");
    return e->run(st, [&](Exec& ex) {
        float* z_y = (float*)ex.raw(zcount * 4);
        float* xt = (float*)ex.raw(zcount * 4);
        float* pred = (float*)ex.raw(zcount * 4);
        // conditioning for the UNet: raw lq at latent resolution, or the feature-extractor output (step invariant: hoisted)
        View feat[3]; bool have_feat[3] = {false, false, false};
        if (!e->fe_convs.empty())
            for (int i = 0; i < a->steps; ++i) {
                const int pr = a->prec_unet[i];
                if (!have_feat[pr]) { feat[pr] = e->g.feature_extract(ex, a->y, a->mask, B, a->h, a->w, pr); have_feat[pr] = true; }
            }
        e->g.sample_prologue(ex, a, z_y, xt, a->noise, keys, kd);
        std::vector<int> tb(B);
        Graphs::StepCall sc{};
        sc.xt = xt; sc.pred = pred; sc.y = a->y; sc.mask = a->mask; sc.B = B; sc.hz = hz; sc.wz = wz; sc.t = tb.data(); sc.a = a; sc.films = films.data();
        sc.keys = keys; sc.keys_dev = kd;
        for (int i = a->steps - 1, k = 1; i >= 0; --i, ++k) {
            std::fill(tb.begin(), tb.end(), i);
            sc.prec = a->prec_unet[i];
            sc.feat = e->fe_convs.empty() ? nullptr : &feat[sc.prec];
            sc.noise = keys ? nullptr : a->noise + (long long)k * zcount;
            e->g.sample_step(ex, sc);
        }
        e->g.sample_epilogue(ex, a, xt);
    });
}

int rs_sample(rs_engine* e, const rs_sample_args* a) { return sample_impl(e, a, nullptr); }

int rs_sample_seeded(rs_engine* e, const rs_sample_args* a, const rs_noise_key* keys) {
    if (!e || !a) return fail("rs_sample_seeded: null argument");
    if (const int rc = noise_keys_check("rs_sample_seeded", keys, a->B)) return rc;
    return sample_impl(e, a, keys);
}

static int sample_begin_impl(rs_engine* e, const rs_sample_args* a, float* x_T, const rs_noise_key* keys) {
    const std::string err = sample_args_error(e, a, true, false);
    if (!err.empty()) return fail("rs_sample_begin: " + err);
    if (!keys && !a->noise) return fail("rs_sample_begin: null tensor (noise / x_T)");
    if (!x_T) return fail("rs_sample_begin: null tensor (noise / x_T)");
    const int f = e->g.latent_div();
    const long long zcount = (long long)a->B * e->cfg.ae.embed_dim * (a->h * a->sf / f) * (a->w * a->sf / f);
    const rs_noise_key* kd = nullptr;
    if (keys && a->B > RS_MAX_ROWS && !(kd = e->stage_keys(keys, a->B, (hipStream_t)a->stream))) return fail("rs_sample_begin_seeded: device copy of the keys failed");
    return e->run((hipStream_t)a->stream, [&](Exec& ex) {
        float* z_y = (float*)ex.raw(zcount * 4);
        e->g.sample_prologue(ex, a, z_y, x_T, a->noise, keys, kd);
    });
}

int rs_sample_begin(rs_engine* e, const rs_sample_args* a, float* x_T) { return sample_begin_impl(e, a, x_T, nullptr); }

int rs_sample_begin_seeded(rs_engine* e, const rs_sample_args* a, float* x_T, const rs_noise_key* keys) {
    if (!e || !a) return fail("rs_sample_begin_seeded: null argument");
    if (const int rc = noise_keys_check("rs_sample_begin_seeded", keys, a->B)) return rc;
    return sample_begin_impl(e, a, x_T, keys);
}

static int sample_step_impl(rs_engine* e, const rs_step_args* s, const rs_noise_key* keys) {
    if (!e || !s || !s->sched) return fail("rs_sample_step: null argument");
    const rs_sample_args* a = s->sched;
    if (a->steps < 1 || a->steps > RS_MAX_STEPS) return fail("rs_sample_step: bad step count in the schedule");
    if (s->prec != RS_F16 && s->prec != RS_F32 && s->prec != RS_F16S) return fail("rs_sample_step: bad precision");
    rs_sample_args g = *a;   // (geometry checks with this call's batch)
    g.B = s->B;
    {
        const std::string err = sample_args_error(e, &g, false, false);
        if (!err.empty()) return fail("rs_sample_step: " + err);
    }
    if (!s->x || !s->t) return fail("rs_sample_step: null tensor (x) or step indices (t)");
    if (e->cfg.unet.cond_lq && !s->y) return fail("rs_sample_step: this UNet is conditioned on lq (cond_lq) but y is NULL");
    if (e->cfg.unet.cond_mask && !s->mask) return fail("rs_sample_step: this UNet is conditioned on a mask (cond_mask) but mask is NULL");
    const int B = s->B;
    bool mixed = false, noisy = false;
    for (int b = 0; b < B; ++b) {
        if (s->t[b] < 0 || s->t[b] >= a->steps)
            return fail("rs_sample_step: step index t[" + std::to_string(b) + "] = " + std::to_string(s->t[b]) + " is outside [0, " + std::to_string(a->steps) + ")");
        mixed |= s->t[b] != s->t[0];
        noisy |= s->t[b] > 0;
    }
    if (mixed && B > RS_MAX_ROWS) return fail("rs_sample_step: mixed step indices in a batch of more than RS_MAX_ROWS (" + std::to_string(RS_MAX_ROWS) + ") images");
    if (noisy && !keys && !s->noise) return fail("rs_sample_step: noise is NULL but an image is at t > 0");
    const rs_noise_key* kd = nullptr;
    if (keys && B > RS_MAX_ROWS && !(kd = e->stage_keys(keys, B, (hipStream_t)s->stream))) return fail("rs_sample_step_seeded: device copy of the keys failed");
    hipStream_t st = (hipStream_t)s->stream;
    std::vector<const float*> films(a->steps, nullptr);
    for (int b = 0; b < B; ++b) {
        const int i = s->t[b];
        if (!films[i] && !(films[i] = e->film_row(a->tmap[i], st))) return fail("FiLM table allocation failed");
    }
    const int f = e->g.latent_div(), hz = a->h * a->sf / f, wz = a->w * a->sf / f;
    const long long zcount = (long long)B * e->cfg.ae.embed_dim * hz * wz;
    return e->run(st, [&](Exec& ex) {
        float* pred = s->pred_xstart ? s->pred_xstart : (float*)ex.raw(zcount * 4);
        // (feature-extractor configs: the conditioning features of this batch, per call)
        View feat; const View* fp = nullptr;
        if (!e->fe_convs.empty()) { feat = e->g.feature_extract(ex, s->y, s->mask, B, a->h, a->w, s->prec); fp = &feat; }
        Graphs::StepCall sc{};
        sc.xt = s->x; sc.pred = pred; sc.feat = fp; sc.y = s->y; sc.mask = s->mask; sc.B = B; sc.hz = hz; sc.wz = wz; sc.prec = s->prec; sc.t = s->t;
        sc.a = a; sc.films = films.data(); sc.noise = keys ? nullptr : s->noise; sc.keys = keys; sc.keys_dev = kd;
        e->g.sample_step(ex, sc);
    });
}

int rs_sample_step(rs_engine* e, const rs_step_args* s) { return sample_step_impl(e, s, nullptr); }

int rs_sample_step_seeded(rs_engine* e, const rs_step_args* s, const rs_noise_key* keys) {
    if (!e || !s) return fail("rs_sample_step_seeded: null argument");
    if (const int rc = noise_keys_check("rs_sample_step_seeded", keys, s->B)) return rc;
    return sample_step_impl(e, s, keys);
}

int rs_film_prewarm(rs_engine* e, const int* timesteps, int n, void* stream) {
    if (!e || !e->cfg.has_unet) return fail("engine has no UNet");
    if (!e->ready) return fail("weights are not ready");
    if (n < 0 || (n && !timesteps)) return fail("rs_film_prewarm: bad timestep list");
    for (int i = 0; i < n; ++i)
        if (!e->film_row(timesteps[i], (hipStream_t)stream)) return fail("FiLM table allocation failed");
    return 0;
}

int rs_sample_end(rs_engine* e, const rs_sample_args* a, const float* x_0) {
    const std::string err = sample_args_error(e, a, false, true);
    if (!err.empty()) return fail("rs_sample_end: " + err);
    if (!x_0) return fail("rs_sample_end: null tensor (x_0)");
    return e->run((hipStream_t)a->stream, [&](Exec& ex) { e->g.sample_epilogue(ex, a, x_0); });
}

}  // extern "C"

// Test-only probe of the normalisation passes (k_misc.hip: InstanceNorm, layernorm_cf, the TCM branch head; k_cln.hip: cumulative LayerNorm)
// and of the TCM block (blocks.h run_tcm: k_tcm.hip's one-workgroup-per-utterance kernel or the multi-launch path), called as the
// models call them - through blocks.h norm2d_prelu / tcm_head / run_tcm / TcmBlock::load where the models go through those, through
// the launchers otherwise - on device buffers the caller owns, with a record of every dispatch (norm_set_launch_log).  Ragged
// batches go through set_ragged_ctx, frame-online chunks through StreamSlots / StreamScope.  Plain C entry points for ctypes:
// tests/test_gpu_norm_forms.py compares every launch with float64.  Not linked into libse_engine.so.
#include "../blocks.h"
#include <string>
#include <vector>

using namespace se;

namespace {
thread_local std::string g_err;
thread_local std::vector<NormLaunchRec> g_log;
thread_local std::vector<GCLaunchRec> g_gclog;

struct Stream {
    StreamSlots slots;
    int B = 0;
};

struct Tcm {
    TcmBlock blk;
    float* scratch = nullptr;
    size_t cap = 0;
    ~Tcm() {
        blk.free();
        if (scratch) (void)hipFree(scratch);
    }
};

// tlen (device [B] or null) published as the engine publishes a ragged batch; sc (optional): one frame-online chunk
template <typename F>
int guarded(const int* tlen, F&& f) {
    Ragged rg;
    rg.tlen = tlen;
    try {
        SE_HIP(hipDeviceSynchronize());
        g_log.clear();
        g_gclog.clear();
        norm_set_launch_log(&g_log);
        gc_set_launch_log(&g_gclog);
        if (tlen) set_ragged_ctx(&rg);
        f();
        set_ragged_ctx(nullptr);
        norm_set_launch_log(nullptr);
        gc_set_launch_log(nullptr);
        SE_HIP(hipDeviceSynchronize());
        return 0;
    } catch (const std::exception& e) {
        set_ragged_ctx(nullptr);
        set_stream_ctx(nullptr);
        norm_set_launch_log(nullptr);
        gc_set_launch_log(nullptr);
        g_err = e.what();
        return -1;
    }
}

NormAct norm_act(const float* g, const float* b, const float* s, bool cum) {
    NormAct n;
    n.g = const_cast<float*>(g);
    n.b = const_cast<float*>(b);
    n.s = const_cast<float*>(s);
    n.cum = cum;
    return n;      // (not owned: NormAct::free is never called on it)
}
}  // namespace

extern "C" {

const char* np_last_error() { return g_err.c_str(); }

// dispatches of the last call (norm / TCM launchers), and the tap-table conv launches next to them (run_tcm's multi-launch path)
int np_launch_count() { return (int)g_log.size(); }
const char* np_launch_kernel(int i) { return i >= 0 && i < (int)g_log.size() ? g_log[i].kernel : ""; }
// W, VPT, KS, GATED, CUM, strip, ragged, c0, WP, grid, block, shmem, res
int np_launch_get(int i, long long* out, int n) {
    if (i < 0 || i >= (int)g_log.size()) return -1;
    const NormLaunchRec& r = g_log[i];
    const long long v[13] = {r.W, r.VPT, r.KS, r.GATED, r.CUM, r.strip, r.ragged, r.c0, r.WP, r.grid, r.block, r.shmem, r.res};
    for (int k = 0; k < n && k < 13; ++k) out[k] = v[k];
    return 13;
}
int np_gc_launch_count() { return (int)g_gclog.size(); }

// blocks.h norm2d_prelu on x [B][C][F][T]: InstanceNorm (cum = 0) or cumulative LayerNorm (cum = 1), PReLU slope s [C], residual
// (optional, may alias y: the offline cLN forms take it in their apply pass, a frame-online chunk outside the register form adds it
// with launch_add); st (optional): the call is one chunk (H history columns + n new frames, T = H + n, first new frame t0) of a stream
int np_norm2d_prelu(int cum, const float* x, float* y, const float* g, const float* b, const float* s, int B, int C, int F, int T,
                    const float* res, const int* tlen, void* st, int H, int n, long t0) {
    return guarded(tlen, [&] {
        const NormAct na = norm_act(g, b, s, cum != 0);
        if (st) {
            Stream* sm = static_cast<Stream*>(st);
            StreamScope sc(sm->slots, H, n, t0, sm->B);
            norm2d_prelu(na, x, y, B, C, F, T, 0, res);
        } else {
            norm2d_prelu(na, x, y, B, C, F, T, 0, res);
        }
    });
}
// the launcher itself (slope may be null: no PReLU)
int np_instnorm_prelu(const float* x, float* y, const float* g, const float* b, const float* s, int B, int C, int P, const float* res,
                      int T, const int* tlen) {
    return guarded(tlen, [&] { launch_instnorm_prelu(x, y, g, b, s, B, C, P, 0, res, T); });
}
int np_instnorm_prelu_stats(const float* x, float* y, const float* g, const float* b, const float* s, const float* stats, int nslot,
                            int B, int C, int P, const float* res, int T, const int* tlen) {
    return guarded(tlen, [&] { launch_instnorm_prelu_stats(x, y, g, b, s, stats, nslot, B, C, P, 0, res, T); });
}
int np_instnorm_finalize(const float* stats, int nslot, const float* g, const float* b, const float* s, float* nrm, int B, int C, int P,
                         int T, const int* tlen) {
    return guarded(tlen, [&] { launch_instnorm_finalize(stats, nslot, g, b, s, nrm, B, C, P, 0, T); });
}
int np_instnorm_apply2(const float* xa, const float* na, const float* xb, const float* nb, float* y, int B, int C, int P) {
    return guarded(nullptr, [&] { launch_instnorm_apply2(xa, na, xb, nb, y, B, C, P, 0); });
}
// blocks.h tcm_head: PReLU -> InstanceNorm1d / cLN -> shared causal FIR (K = 0: none) on x [B][C][T]; st: as np_norm2d_prelu
int np_tcm_head(int cum, const float* x, float* y, const float* s, const float* g, const float* b, const float* fir, int K, int B, int C,
                int T, const int* tlen, void* st, int H, int n, long t0) {
    return guarded(tlen, [&] {
        const NormAct na = norm_act(g, b, s, cum != 0);
        if (st) {
            Stream* sm = static_cast<Stream*>(st);
            StreamScope sc(sm->slots, H, n, t0, sm->B);
            tcm_head(na, fir, K, x, y, B, C, T, 0);
        } else {
            tcm_head(na, fir, K, x, y, B, C, T, 0);
        }
    });
}
int np_cln(const float* x, float* y, const float* gain, const float* bias, const float* pre, const float* post, const float* fir, int K,
           int B, int C, int F, int T, const float* res) {
    return guarded(nullptr, [&] { launch_cln(x, y, gain, bias, pre, post, fir, K, B, C, F, T, 0, res); });
}
int np_cln_parts(const float* x, float* y, const float* gain, const float* bias, const float* post, const float* parts, int B, int C,
                 int F, int T, const float* res) {
    return guarded(nullptr, [&] { launch_cln_parts(x, y, gain, bias, post, parts, B, C, F, T, 0, res); });
}
int np_layernorm_cf(const float* x, const float* res, const float* w, const float* b, float* out, int B, int C, int F, int T, float eps,
                    int post, const float* prelu) {
    return guarded(nullptr, [&] { launch_layernorm_cf(x, res, w, b, out, B, C, F, T, eps, 0, post, prelu); });
}

// frame-online stream of B rows: zero state, as a model's begin_stream leaves it
void* np_stream_create(int B) {
    Stream* sm = nullptr;
    guarded(nullptr, [&] {
        sm = new Stream();
        sm->B = B;
        sm->slots.begin(B, 0);
    });
    return sm;
}
void np_stream_destroy(void* h) {
    (void)hipDeviceSynchronize();
    delete static_cast<Stream*>(h);
}
// state slot i of the stream (call order; it exists once a chunk has taken it) from / to host memory, `bytes` = its whole size: a test
// reads the carried sums a chunk left, or puts the sums of a stream that is far on in their place
int np_slot_read(void* h, int i, void* host, long long bytes) {
    return guarded(nullptr, [&] {
        const Stream* sm = static_cast<Stream*>(h);
        SE_CHECK(sm && host && i >= 0 && i < (int)sm->slots.v.size() && bytes == (long long)sm->slots.v[i].second, "np_slot_read: no such slot / size");
        SE_HIP(hipMemcpy(host, sm->slots.v[i].first, (size_t)bytes, hipMemcpyDeviceToHost));
    });
}
int np_slot_write(void* h, int i, const void* host, long long bytes) {
    return guarded(nullptr, [&] {
        Stream* sm = static_cast<Stream*>(h);
        SE_CHECK(sm && host && i >= 0 && i < (int)sm->slots.v.size() && bytes == (long long)sm->slots.v[i].second, "np_slot_write: no such slot / size");
        SE_HIP(hipMemcpy(sm->slots.v[i].first, host, (size_t)bytes, hipMemcpyHostToDevice));
    });
}

// ---- TCM block: a state dict in torch layout -> TcmBlock::load (the fused weights through tcm_fused_build) -> run_tcm
void* np_sd_create() { return new StateDict(); }
void np_sd_destroy(void* h) { delete static_cast<StateDict*>(h); }
void np_sd_put(void* h, const char* key, const float* host, const long long* shape, int nd) {
    HostTensor t;
    for (int i = 0; i < nd; ++i) t.shape.push_back(shape[i]);
    t.data.assign(host, host + t.numel());
    (*static_cast<StateDict*>(h))[key] = std::move(t);
}
void* np_tcm_create(void* sd, const char* prefix, int dil, const char* left, const char* right, int conv_idx, int fir_k, int ks,
                    int gated) {
    Tcm* t = nullptr;
    guarded(nullptr, [&] {
        Tcm* p = new Tcm();
        try {
            const TrackedSD tsd(*static_cast<StateDict*>(sd));
            p->blk.load(tsd, prefix, dil, left, right, conv_idx, fir_k, ks, gated != 0);
        } catch (...) {
            delete p;
            throw;
        }
        t = p;
    });
    return t;
}
void np_tcm_destroy(void* h) {
    (void)hipDeviceSynchronize();
    delete static_cast<Tcm*>(h);
}
// x, y [B][256][T]; min_batch: tcm_fused_min_override() for this call (1: the fused kernel from one row on where the shape allows
// it; a value above B: the multi-launch path)
int np_tcm_run(void* h, const float* x, float* y, int B, int T, int min_batch, const int* tlen) {
    return guarded(tlen, [&] {
        Tcm* t = static_cast<Tcm*>(h);
        const size_t need = (size_t)4 * B * 64 * T * sizeof(float) + 64;      // (+ the <= 12 B a 16 B staging group may read past a row)
        if (need > t->cap) {
            if (t->scratch) SE_HIP(hipFree(t->scratch));
            t->scratch = nullptr;
            SE_HIP(hipMalloc(&t->scratch, need));
            t->cap = need;
        }
        const size_t q = (size_t)B * 64 * T;
        const TcmScratch ts{t->scratch, t->scratch + q, t->scratch + 2 * q, t->scratch + 3 * q};
        // as the engine registers its arenas: the pointwise layers of the multi-launch path stage 16 B groups, which at T % 4 != 0
        // read <= 12 B past a tensor's last row (the caller's buffers carry slack behind them)
        const size_t xbytes = (size_t)B * 256 * T * sizeof(float);
        gc_register_overread_range(x, xbytes);
        gc_register_overread_range(t->scratch, need);
        const int old = tcm_fused_min_override();
        tcm_fused_min_override() = min_batch;
        auto restore = [&] {
            tcm_fused_min_override() = old;
            gc_unregister_overread_range(x);
            gc_unregister_overread_range(t->scratch);
        };
        try {
            run_tcm(t->blk, x, y, ts, B, T, 0, nullptr);
        } catch (...) {
            restore();
            throw;
        }
        restore();
    });
}

}  // extern "C"

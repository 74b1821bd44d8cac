// Test-only probe of the frame-online layer path: the chain kernel of the cLN TCM blocks (k_tcm_stream.hip, through blocks.h
// run_tcm_chain or the launcher itself), one conv / transposed-conv layer on a window of a chunk (layers.hip run_conv / run_deconv
// under a published StreamScope - gc_launch_prof adds the history exchange and sets t_base - or with explicit t_base / t_out /
// tb_soft, as the models without a stream context call them), and the history movers (k_misc.hip stream_exchange,
// stream_exchange_pair, launch_hist_restore / save / batch), on device buffers the caller owns.  A stream's state slots can be
// counted, read and written.  Every call is synchronised on both sides; the norm, online (online_log.h) and conv launch logs record every dispatch
// since op_log_clear.  Plain C entry points for ctypes: tests/test_gpu_online_forms.py compares every chunk with float64.  Not
// linked into libse_engine.so.
#include "../blocks.h"
#include "../online_log.h"
#include <memory>
#include <string>
#include <vector>

using namespace se;

namespace {
thread_local std::string g_err;
thread_local std::vector<NormLaunchRec> g_log;
thread_local std::vector<GCLaunchRec> g_gclog;
thread_local std::unique_ptr<StreamScope> g_scope;      // the chunk published by op_scope_open

struct Stream {
    StreamSlots slots;
    int B = 0;
};

struct Tcm {
    TcmBlock blk;
    ~Tcm() { blk.free(); }
};

struct Plan {
    bool deconv = false;
    int M = 0, Cin = 0, C0 = 0;
    GCPlan conv;
    DeconvPlan dec;
    ~Plan() {
        if (deconv) free_deconv_plan(dec);
        else gc_free_plan(conv);
    }
};

DenseW dense(const float* w, const float* bias, int M, int Cin, int nkf, int nkt) {
    DenseW d;
    d.M = M;
    d.Cin = Cin;
    d.nkf = nkf;
    d.nkt = nkt;
    d.w.assign(w, w + (size_t)M * Cin * nkf * nkt);
    d.bias = bias ? std::vector<float>(bias, bias + M) : std::vector<float>(M, 0.f);
    return d;
}

// The history movers have no launch record of their own (k_misc.hip and layers.hip are kept as they are); each launcher dispatches
// one kernel, which the probe names: stream_exchange -> stream_hist_kernel, stream_exchange_pair -> stream_hist_pair_kernel (two
// stream_hist_kernel under SE_STREAM_HIST_PAIR=0), launch_hist_restore / save -> hist_kernel, launch_hist_batch -> hist_batch_kernel.
// Inside a layer call the exchange is seen by the state slots it takes (StreamCtx::cursor): one for a source, two for a pair.
void named(const char* kernel) {
    NormLaunchRec r;
    r.kernel = kernel;
    g_log.push_back(r);
}
bool pair_on() { return !(getenv("SE_STREAM_HIST_PAIR") && atoi(getenv("SE_STREAM_HIST_PAIR")) == 0); }

template <typename F>
int guarded(F&& f) {
    try {
        SE_HIP(hipDeviceSynchronize());
        norm_set_launch_log(&g_log);
        online_set_launch_log(&g_log);
        gc_set_launch_log(&g_gclog);
        f();
        norm_set_launch_log(nullptr);
        online_set_launch_log(nullptr);
        gc_set_launch_log(nullptr);
        SE_HIP(hipDeviceSynchronize());
        return 0;
    } catch (const std::exception& e) {
        g_scope.reset();
        set_stream_ctx(nullptr);
        norm_set_launch_log(nullptr);
        online_set_launch_log(nullptr);
        gc_set_launch_log(nullptr);
        g_err = e.what();
        return -1;
    }
}
}  // namespace

extern "C" {

const char* op_last_error() { return g_err.c_str(); }

// ---- launch logs: dispatches since op_log_clear (norm / TCM / history launchers; tap-table conv launches)
void op_log_clear() {
    g_log.clear();
    g_gclog.clear();
}
int op_launch_count() { return (int)g_log.size(); }
const char* op_launch_kernel(int i) { return i >= 0 && i < (int)g_log.size() ? g_log[i].kernel : ""; }
// W, VPT, KS, GATED, CUM, strip, ragged, c0, WP, grid, block, shmem, res
int op_launch_get(int i, long long* out, int n) {
    if (i < 0 || i >= (int)g_log.size()) return -1;
    const NormLaunchRec& r = g_log[i];
    const long long v[13] = {r.W, r.VPT, r.KS, r.GATED, r.CUM, r.strip, r.ragged, r.c0, r.WP, r.grid, r.block, r.shmem, r.res};
    for (int k = 0; k < n && k < 13; ++k) out[k] = v[k];
    return 13;
}
int op_gc_launch_count() { return (int)g_gclog.size(); }
// family, BM, BN, flat_upr, upt, flat_rows, qt2, nrm, res, trim, stats, ragged, flat_nrm_refused, nblk, epi
int op_gc_launch_get(int i, long long* out, int n) {
    if (i < 0 || i >= (int)g_gclog.size()) return -1;
    const GCLaunchRec& r = g_gclog[i];
    const long long v[15] = {r.family, r.BM,  r.BN,   r.flat_upr, r.upt,    r.flat_rows,        r.qt2, r.nrm,
                             r.res,    r.trim, r.stats, r.ragged,  r.flat_nrm_refused, r.nblk, r.epi};
    for (int k = 0; k < n && k < 15; ++k) out[k] = v[k];
    return 15;
}

// ---- frame-online stream of B rows: zero state, as a model's begin_stream leaves it
void* op_stream_create(int B) {
    Stream* sm = nullptr;
    guarded([&] {
        sm = new Stream();
        sm->B = B;
        sm->slots.begin(B, 0);
    });
    return sm;
}
// a new stream on the same slots (StreamSlots::begin: the state is zeroed, the slots stay)
int op_stream_begin(void* h) {
    return guarded([&] {
        Stream* sm = static_cast<Stream*>(h);
        sm->slots.begin(sm->B, 0);
    });
}
void op_stream_destroy(void* h) {
    (void)hipDeviceSynchronize();
    g_scope.reset();
    delete static_cast<Stream*>(h);
}
int op_slot_count(void* h) { return (int)static_cast<Stream*>(h)->slots.v.size(); }
long long op_slot_bytes(void* h, int i) {
    const Stream* sm = static_cast<Stream*>(h);
    return i >= 0 && i < (int)sm->slots.v.size() ? (long long)sm->slots.v[i].second : -1;
}
int op_slot_read(void* h, int i, void* host, long long bytes) {
    return guarded([&] {
        const Stream* sm = static_cast<Stream*>(h);
        SE_CHECK(i >= 0 && i < (int)sm->slots.v.size() && bytes == (long long)sm->slots.v[i].second, "op_slot_read: no such slot / size");
        SE_HIP(hipMemcpy(host, sm->slots.v[i].first, (size_t)bytes, hipMemcpyDeviceToHost));
    });
}
int op_slot_write(void* h, int i, const void* host, long long bytes) {
    return guarded([&] {
        const Stream* sm = static_cast<Stream*>(h);
        SE_CHECK(i >= 0 && i < (int)sm->slots.v.size() && bytes == (long long)sm->slots.v[i].second, "op_slot_write: no such slot / size");
        SE_HIP(hipMemcpy(sm->slots.v[i].first, host, (size_t)bytes, hipMemcpyHostToDevice));
    });
}
// one chunk of the stream: H history columns + n new frames, first new frame t0; every run call below until op_scope_close is
// a launch of this chunk (state slots are taken in call order)
int op_scope_open(void* h, int H, int n, long long t0) {
    return guarded([&] {
        Stream* sm = static_cast<Stream*>(h);
        g_scope.reset();
        g_scope.reset(new StreamScope(sm->slots, H, n, (long)t0, sm->B));
    });
}
void op_scope_close() { g_scope.reset(); }
int op_scope_cursor() { return g_scope ? (int)g_scope->cx.cursor : -1; }

// ---- TCM blocks: a state dict in torch layout -> TcmBlock::load -> run_tcm_chain / launch_tcm_chain
void* op_sd_create() { return new StateDict(); }
void op_sd_destroy(void* h) { delete static_cast<StateDict*>(h); }
void op_sd_put(void* h, const char* key, const float* host, const long long* shape, int nd) {
    HostTensor t;
    for (int i = 0; i < nd; ++i) t.shape.push_back(shape[i]);
    t.data.assign(host, host + t.numel());
    (*static_cast<StateDict*>(h))[key] = std::move(t);
}
void* op_tcm_create(void* sd, const char* prefix, int dil, const char* left, const char* right, int conv_idx, int fir_k, int ks,
                    int gated) {
    Tcm* t = nullptr;
    guarded([&] {
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
void op_tcm_destroy(void* h) {
    (void)hipDeviceSynchronize();
    delete static_cast<Tcm*>(h);
}
// blocks.h run_tcm_chain over nblk blocks on the window x [B][256][T] of the open chunk; X0 / X1: the ping-pong buffers;
// *which = the buffer that holds the result.  Every block must have the stream form (cLN `gain` keys): nothing else is built here.
int op_tcm_chain_run(void* const* blocks, int nblk, const float* x, float* X0, float* X1, int B, int T, int* which) {
    return guarded([&] {
        std::vector<TcmBlock> blk;
        for (int i = 0; i < nblk; ++i) {
            const TcmBlock& k = static_cast<const Tcm*>(blocks[i])->blk;
            SE_CHECK(k.sfused.w_in && k.nL.cum && k.nO.cum, "op_tcm_chain_run: a block without the frame-online form");
            blk.push_back(k);      // (a shallow copy: the Tcm keeps the ownership)
        }
        SE_CHECK(stream_ctx(), "op_tcm_chain_run: no chunk is open");
        float* const X[2] = {X0, X1};
        const TcmScratch none{nullptr, nullptr, nullptr, nullptr};
        const float* y = run_tcm_chain(blk.data(), nblk, x, X, none, B, T, 0, nullptr);
        *which = y == X0 ? 0 : (y == X1 ? 1 : -1);
    });
}
// the launcher itself on the open chunk (its own refusals: 9 blocks, mixed tap counts, a FIR above 64 taps)
int op_tcm_chain_launch(void* const* blocks, int nblk, const float* x, float* y) {
    return guarded([&] {
        std::vector<const TcmStreamW*> f;
        std::vector<TcmFusedHeads> hd;
        std::vector<int> dil, K;
        for (int i = 0; i < nblk; ++i) {
            const TcmBlock& k = static_cast<const Tcm*>(blocks[i])->blk;
            f.push_back(&k.sfused);
            hd.push_back(TcmFusedHeads{k.nL.s, k.nL.g, k.nL.b, k.firL, k.nR.s, k.nR.g, k.nR.b, k.firR, k.nO.s, k.nO.g, k.nO.b});
            dil.push_back(k.d);
            K.push_back(k.K);
        }
        launch_tcm_chain(f.data(), hd.data(), dil.data(), K.data(), nblk, x, y, 0);
    });
}

// ---- history movers
int op_exchange(float* x, long long sb, long long sc, long long sf, int B, int C, int F, int need) {
    return guarded([&] {
        stream_exchange(x, (long)sb, (long)sc, (long)sf, B, C, F, need, 0);
        named("stream_hist");
    });
}
int op_exchange_pair(float* x0, long long sb0, long long sc0, long long sf0, int C0, int F0, float* x1, long long sb1, long long sc1,
                     long long sf1, int C1, int F1, int B, int need) {
    return guarded([&] {
        stream_exchange_pair(x0, (long)sb0, (long)sc0, (long)sf0, C0, F0, x1, (long)sb1, (long)sc1, (long)sf1, C1, F1, B, need, 0);
        if (pair_on()) named("stream_hist_pair");
        else named("stream_hist"), named("stream_hist");
    });
}
int op_hist_restore(float* buf, const float* state, int B, long long rows, int Tw, int hc) {
    return guarded([&] {
        launch_hist_restore(buf, state, B, (long)rows, Tw, hc, 0);
        named("hist");
    });
}
int op_hist_save(const float* buf, float* state, int B, long long rows, int Tw, int hc) {
    return guarded([&] {
        launch_hist_save(buf, state, B, (long)rows, Tw, hc, 0);
        named("hist");
    });
}
int op_hist_batch(float* const* bufs, float* const* states, const long long* rows, int cnt, int B, int Tw, int hc, int save) {
    return guarded([&] {
        SE_CHECK(cnt >= 0 && cnt <= HistBatch::MAX, "op_hist_batch: 0..16 tensors");
        HistBatch hb;
        for (int e = 0; e < cnt; ++e) hb.add(bufs[e], states[e], (long)rows[e]);
        launch_hist_batch(hb, B, Tw, hc, save != 0, 0);
        if (cnt > 0) named("hist_batch");
    });
}

// ---- conv / transposed-conv plans, built as gc_probe.hip's gcp_conv_create / gcp_deconv_create build them
// w: [M][Cin][nkf][nkt]; out[f][t] = sum w[kf][kt] x[f sf - pf + kf dil_f][t - pt_left + kt dil_t]; channels >= c0split: second source
void* op_conv_create(const float* w, const float* bias, const float* slope, int M, int Cin, int nkf, int nkt, int sf, int pf,
                     int pt_left, int dil_f, int dil_t, int act, int epi, int c0split) {
    Plan* pr = nullptr;
    guarded([&] {
        auto* p = new Plan();
        p->M = M;
        p->Cin = Cin;
        p->C0 = c0split < 0 ? Cin : c0split;
        const std::vector<float> sl = slope ? std::vector<float>(slope, slope + M) : std::vector<float>();
        try {
            p->conv = make_conv_plan(dense(w, bias, M, Cin, nkf, nkt), sf, pf, pt_left, dil_f, dil_t, act, sl, epi, 401, c0split);
        } catch (...) {
            delete p;
            throw;
        }
        pr = p;
    });
    return pr;
}
// out[fo][to] = sum_{(fo + pf - kf) % sf == 0} x[(fo + pf - kf) / sf][to + toff - kt] w[kf][kt]
void* op_deconv_create(const float* w, const float* bias, const float* slope, int M, int Cin, int nkf, int nkt, int sf, int pf,
                       int toff, int act, int epi, int c0split) {
    Plan* pr = nullptr;
    guarded([&] {
        auto* p = new Plan();
        p->deconv = true;
        p->M = M;
        p->Cin = Cin;
        p->C0 = c0split < 0 ? Cin : c0split;
        const std::vector<float> sl = slope ? std::vector<float>(slope, slope + M) : std::vector<float>();
        try {
            p->dec = make_deconv_plan(dense(w, bias, M, Cin, nkf, nkt), sf, pf, toff, act, sl, 401, c0split, nullptr, epi);
        } catch (...) {
            delete p;
            throw;
        }
        pr = p;
    });
    return pr;
}
void op_plan_destroy(void* h) {
    (void)hipDeviceSynchronize();
    delete static_cast<Plan*>(h);
}
// [0] plans (parity classes), [1] frames of look-back (the deepest class), [2] channels per staged chunk, [3] direct (<= 4
// channel) path, [4] BM, [5] fused parity pair
int op_plan_info(void* h, int* out, int n) {
    const Plan* p = static_cast<const Plan*>(h);
    const int np = p->deconv ? (int)p->dec.par.size() : 1;
    const GCPlan& g = p->deconv ? p->dec.par[0] : p->conv;
    int lb = 0;
    if (p->deconv)
        for (const auto& c : p->dec.par) lb = std::max(lb, c.lookback);
    else lb = p->conv.lookback;
    const int v[6] = {np, lb, g.p.CI_C, g.p.Ws != nullptr, g.BM, p->deconv ? (int)p->dec.has_pair : 0};
    for (int i = 0; i < n && i < 6; ++i) out[i] = v[i];
    return 6;
}
// One layer call.  Sources [B][C][Fin][Tp] (x1: the channels >= c0split), dst [B][dstC][Fout][Tp]; aux (EPI_ADD / EPI_MUL of a
// conv): laid out like dst.  With a chunk open (op_scope_open) T must be its window H + n and t_base / t_out / tb_soft are not
// read by the conv (gc_launch_prof sets t_base = H); with none they are the caller's: the models without a stream context.
int op_layer_run(void* h, const float* x0, const float* x1, int Fin, float* dst, int dstC, int Fout, const float* aux, int B, int T,
                 int Tp, int t_base, int t_out, int tb_soft) {
    return guarded([&] {
        const Plan* p = static_cast<const Plan*>(h);
        SE_CHECK(p->C0 == p->Cin || x1, "op_layer_run: the plan has a second source");
        const Act4 a0 = act4(x0, p->C0, Fin, Tp);
        const Act4 a1 = act4(x1, p->Cin - p->C0, Fin, Tp);
        const Act4* s1 = p->C0 < p->Cin ? &a1 : nullptr;
        const size_t cur0 = g_scope ? g_scope->cx.cursor : 0;
        struct Seen {       // the exchanges of this call, by the slots they took (also when the call throws after them)
            size_t c0;
            ~Seen() {
                const size_t d = g_scope ? g_scope->cx.cursor - c0 : 0;
                if (d == 2 && pair_on()) named("stream_hist_pair");
                else for (size_t i = 0; i < d; ++i) named("stream_hist");
            }
        } seen{cur0};
        if (p->deconv) {
            SE_CHECK(!aux, "op_layer_run: aux with a transposed conv");
            run_deconv(p->dec, a0, s1, dst, dstC, Fout, B, T, Tp, 0, nullptr, nullptr, t_base, t_out, tb_soft != 0);
        } else {
            GCPlan pl = p->conv;      // (a shallow copy that names the aux tensor, as blocks.h run_tcm fills it in)
            if (aux) {
                pl.p.aux = aux;
                pl.p.x_b = (long)dstC * Fout * Tp;
                pl.p.x_c = (long)Fout * Tp;
                pl.p.x_f = Tp;
            }
            run_conv(pl, a0, s1, dst, dstC, Fout, B, T, Tp, 0, nullptr, nullptr, t_base);
        }
    });
}

// device ranges whose tensors the 16 B staging may over-read by <= 12 B (as the engine registers its arenas)
void op_register_overread(const void* p, size_t bytes) { gc_register_overread_range(p, bytes); }
void op_unregister_overread(const void* p) { gc_unregister_overread_range(p); }

}  // extern "C"

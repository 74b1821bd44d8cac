// Test-only probe of the recurrent kernels (k_lstm_coop.hip, k_lstm.hip, k_lstm_short.hip and the EPI_LSTM step epilogue of
// gemmconv.hip): one LSTM / GRU layer or stack, built from torch.nn tensors by the engine's own loaders (rnn.h lstm_from_torch /
// gru_from_torch: the gate interleave is under test too) and run through the entry points the models call (rnn.h LstmBig,
// lstm_stack_fm, lstm_stack_chunked_fm, run_lstm_pair; launch_lstm_persist / launch_lstm_short with the strides the models pass),
// on device buffers the caller owns, with a record of every dispatch (lstm_set_launch_log, gc_set_launch_log).  Plain C entry
// points for ctypes: tests/test_gpu_lstm_forms.py compares the launches with a float64 LSTM.  Not linked into libse_engine.so.
#include "../rnn.h"
#include "../k_lstm_short.h"
#include <string>
#include <vector>

using namespace se;

namespace {
thread_local std::string g_err;
thread_local std::vector<LstmLaunchRec> g_log;
thread_local std::vector<GCLaunchRec> g_gclog;

// one layer: the engine's LstmBig plus device copies of the (interleaved) matrices for the launchers that take raw pointers
struct Layer {
    LstmW w;
    LstmBig big;
    float *whh = nullptr, *wih = nullptr, *bias = nullptr;
    ~Layer() {
        big.free();
        if (whh) (void)hipFree(whh);
        if (wih) (void)hipFree(wih);
        if (bias) (void)hipFree(bias);
    }
};

HostTensor host(const float* p, int rows, int cols) {
    HostTensor t;
    t.shape = rows > 0 && cols > 0 ? std::vector<int64_t>{rows, cols} : std::vector<int64_t>{rows};
    t.data.assign(p, p + (size_t)rows * std::max(cols, 1));
    return t;
}

// [Z][n] device copy of one host vector per layer
float* stack_dev(const std::vector<const std::vector<float>*>& v) {
    std::vector<float> all;
    for (const auto* p : v) all.insert(all.end(), p->begin(), p->end());
    return to_device(all);
}

template <typename F>
int guarded(F&& f) {
    try {
        SE_HIP(hipDeviceSynchronize());
        g_log.clear();
        g_gclog.clear();
        lstm_set_launch_log(&g_log);
        gc_set_launch_log(&g_gclog);
        f();
        lstm_set_launch_log(nullptr);
        gc_set_launch_log(nullptr);
        SE_HIP(hipDeviceSynchronize());
        return 0;
    } catch (const std::exception& e) {
        lstm_set_launch_log(nullptr);
        gc_set_launch_log(nullptr);
        g_err = e.what();
        return -1;
    }
}

const Layer* L_(const void* h) { return static_cast<const Layer*>(h); }
}  // namespace

extern "C" {

const char* lsp_last_error() { return g_err.c_str(); }

// torch.nn.LSTM (gru = 0: gate rows i, f, g, o) or torch.nn.GRU (gru = 1: r, z, n) tensors of one layer: weight_ih [G H][I],
// weight_hh [G H][H], bias_ih / bias_hh [G H].  fuse_x / coop256: LstmBig::build's opt-ins; s_hint: its sequence-count hint.
void* lsp_layer_create(const float* wih, const float* whh, const float* bih, const float* bhh, int I, int H, int gru, int fuse_x,
                       int coop256, int s_hint) {
    Layer* out = nullptr;
    try {
        auto* l = new Layer();
        try {
            const int G = gru ? 3 : 4;
            const HostTensor wi = host(wih, G * H, I), wh = host(whh, G * H, H), bi = host(bih, G * H, 0), bh = host(bhh, G * H, 0);
            l->w = gru ? gru_from_torch(wi, wh, bi, bh, I, H) : lstm_from_torch(wi, wh, bi, bh, I, H);
            l->big.build(l->w, s_hint, gru != 0, fuse_x != 0, coop256 != 0);
            l->whh = to_device(l->w.whh.w);
            l->wih = to_device(l->w.wih.w);
            l->bias = to_device(l->w.wih.bias);
        } catch (...) {
            delete l;
            throw;
        }
        out = l;
    } catch (const std::exception& e) {
        g_err = e.what();
    }
    return out;
}

void lsp_layer_destroy(void* h) { delete static_cast<Layer*>(h); }

// LstmBig::run_cols: x [T][I][S] rows at pitch x_t, G [T][4H][S], cell [H][S], out: h_t unit j at out + t out_t + j out_rs S
int lsp_run_cols(void* h, const float* x, long x_t, float* G, float* cell, float* out, long out_t, int out_rs, int T, int S, int c0,
                 int Sn) {
    return guarded([&] { L_(h)->big.run_cols(x, x_t, G, cell, out, out_t, out_rs, T, S, c0, Sn, 0, nullptr); });
}

// LstmBig::run_fm (the callers' precondition fm_ok checked first): x [I][T][S] -> out [H][T][S], G [4H][T][S]
int lsp_run_fm(void* h, const float* x, float* G, float* cell, float* out, int T, int S) {
    return guarded([&] {
        SE_CHECK(L_(h)->big.fm_ok(S), "lsp_run_fm: the layer has no feature-major form at this sequence count");
        L_(h)->big.run_fm(x, G, cell, out, T, S, 0, nullptr);
    });
}

// LstmBig::run_stream_strided: continues from (h_state, cell) [H][S] (first: the stream's first step) and leaves the state there
int lsp_run_stream(void* h, const float* x, long x_t, float* G, float* cell, float* h_state, float* out, long out_t, int out_rs, int T,
                   int S, int first) {
    return guarded(
        [&] { L_(h)->big.run_stream_strided(x, x_t, G, cell, h_state, out, out_t, out_rs, T, S, first != 0, 0, nullptr); });
}

// LstmBig::run_cols_x (the input projection inside the step GEMM); hz: zeros [H][S]
int lsp_run_cols_x(void* h, const float* x, long x_t, float* cell, const float* hz, float* out, long out_t, int out_rs, int T, int S,
                   int c0, int Sn) {
    return guarded([&] { L_(h)->big.run_cols_x(x, x_t, cell, hz, out, out_t, out_rs, T, S, c0, Sn, 0, nullptr); });
}

// run_lstm_pair with the [2][4H][H] recurrent matrices built as GCRN builds them; G [2][T][4H][S], cell [2][H][S]
int lsp_run_pair(void* h0, void* h1, const float* x0, const float* x1, long x_t, float* G, float* cell, float* out0, long out_z,
                 long out_t, int out_rs, int T, int S) {
    float* whh2 = nullptr;
    const int rc = guarded([&] {
        whh2 = stack_dev({&L_(h0)->w.whh.w, &L_(h1)->w.whh.w});
        run_lstm_pair(L_(h0)->big, L_(h1)->big, whh2, x0, x1, x_t, G, cell, out0, out_z, out_t, out_rs, T, S, 0, nullptr);
    });
    if (whh2) (void)hipFree(whh2);
    return rc;
}

// lstm_stack_fm (one sequence): x [I][T] -> out [H][T] of the last layer.  *ran = 0: not applicable (nothing launched)
int lsp_stack_fm(void* const* hs, int L, const float* x, float* G, float* out, int T, int* ran) {
    return guarded([&] {
        std::vector<const LstmBig*> ly;
        for (int l = 0; l < L; ++l) ly.push_back(&L_(hs[l])->big);
        *ran = lstm_stack_fm(ly.data(), L, x, G, out, T, 0, nullptr) ? 1 : 0;
    });
}

// lstm_stack_chunked_fm: x [I][T][S], outs[l] [H][T][S] (may alias outs[l - 2]), G [4H][T][S], cells [L][H][S]
int lsp_stack_chunked_fm(void* const* hs, int L, const float* x, float* G, float* cells, float* const* outs, int T, int S, int* ran) {
    return guarded([&] {
        std::vector<const LstmBig*> ly;
        for (int l = 0; l < L; ++l) ly.push_back(&L_(hs[l])->big);
        *ran = lstm_stack_chunked_fm(ly.data(), L, x, G, cells, outs, T, S, 0, nullptr) ? 1 : 0;
    });
}

// launch_lstm_persist over Z layers (H = 64 / 128) and O outer items: x element (o, t, i, n) at o x_o + t x_t + i S + n; the input
// projection of layer z on item o goes to G + (o Z + z) T 4H S as [T][4H][S] (the engine's pointwise plan); out / reverse / st_h /
// st_c as LstmPersistArgs (st_z = H S)
int lsp_persist(void* const* hs, int Z, const float* x, long x_o, long x_t, int O, float* G, float* out, long out_o, long out_z,
                long out_t, long out_row, int T, int S, int reverse, float* st_h, float* st_c) {
    float* whh = nullptr;
    const int rc = guarded([&] {
        const int H = L_(hs[0])->w.H;
        std::vector<const std::vector<float>*> v;
        for (int z = 0; z < Z; ++z) v.push_back(&L_(hs[z])->w.whh.w);
        whh = stack_dev(v);
        const long gz = (long)T * 4 * H * S;
        for (int o = 0; o < O; ++o)
            for (int z = 0; z < Z; ++z)
                run_pointwise(L_(hs[z])->big.gin, x + (long)o * x_o, x_t, S, G + ((long)o * Z + z) * gz, 4L * H * S, S, T, S, 0, nullptr);
        LstmPersistArgs a{};
        a.gx = G; a.whh = whh; a.out = out;
        a.gx_o = (long)Z * gz; a.gx_z = gz; a.gx_t = 4L * H * S; a.gx_row = S;
        a.whh_z = 4L * H * H;
        a.out_o = out_o; a.out_z = out_z; a.out_t = out_t; a.out_row = out_row;
        a.H = H; a.T = T; a.S = S; a.Z = Z; a.O = O; a.reverse = reverse;
        a.st_h = st_h; a.st_c = st_c; a.st_z = (long)H * S;
        launch_lstm_persist(a, 0);
    });
    if (whh) (void)hipFree(whh);
    return rc;
}

// launch_lstm_short over Z layers (H = 64, I = 128): x element (o, c, t, n) at o x_o + c x_c + t x_t + n, out as LstmShortArgs
int lsp_short(void* const* hs, int Z, const float* x, long x_o, long x_c, long x_t, float* out, long out_o, long out_z, long out_t,
              long out_row, int T, int S, int O, int reverse) {
    float *wih = nullptr, *whh = nullptr, *bias = nullptr;
    const int rc = guarded([&] {
        const LstmW& w0 = L_(hs[0])->w;
        SE_CHECK(lstm_short_supported(w0.H, w0.I, T), "lsp_short: no short-sequence kernel for this shape");
        std::vector<const std::vector<float>*> vi, vh, vb;
        for (int z = 0; z < Z; ++z) {
            vi.push_back(&L_(hs[z])->w.wih.w);
            vh.push_back(&L_(hs[z])->w.whh.w);
            vb.push_back(&L_(hs[z])->w.wih.bias);
        }
        wih = stack_dev(vi);
        whh = stack_dev(vh);
        bias = stack_dev(vb);
        LstmShortArgs a{};
        a.x = x; a.x_o = x_o; a.x_c = x_c; a.x_t = x_t;
        a.wih = wih; a.whh = whh; a.bias = bias;
        a.wih_z = 4L * w0.H * w0.I; a.whh_z = 4L * w0.H * w0.H; a.bias_z = 4L * w0.H;
        a.out = out; a.out_o = out_o; a.out_z = out_z; a.out_t = out_t; a.out_row = out_row;
        a.T = T; a.S = S; a.Z = Z; a.O = O; a.reverse = reverse;
        launch_lstm_short(a, 0);
    });
    for (float* p : {wih, whh, bias})
        if (p) (void)hipFree(p);
    return rc;
}

// recurrent dispatches of the last run: name, then [0] H, NS, TAG, LEAD, NW, L, Z, SS, chunk, grid, shmem, lz[4], t0[4], Tz[4]
int lsp_launch_count() { return (int)g_log.size(); }
const char* lsp_launch_kernel(int i) { return i >= 0 && i < (int)g_log.size() ? g_log[i].kernel : ""; }
int lsp_launch_get(int i, long long* out, int n) {
    if (i < 0 || i >= (int)g_log.size()) return -1;
    const LstmLaunchRec& r = g_log[i];
    const long long v[23] = {r.H,     r.NS,    r.TAG,   r.LEAD,  r.NW,    r.L,     r.Z,     r.SS,    r.chunk, r.grid,  r.shmem, r.lz[0],
                             r.lz[1], r.lz[2], r.lz[3], r.t0[0], r.t0[1], r.t0[2], r.t0[3], r.Tz[0], r.Tz[1], r.Tz[2], r.Tz[3]};
    for (int k = 0; k < n && k < 23; ++k) out[k] = v[k];
    return 23;
}
// gemmconv dispatches of the last run: [0] epi, [1] gru, [2] workgroups
int lsp_gc_count() { return (int)g_gclog.size(); }
int lsp_gc_get(int i, long long* out, int n) {
    if (i < 0 || i >= (int)g_gclog.size()) return -1;
    const long long v[3] = {g_gclog[i].epi, g_gclog[i].gru, g_gclog[i].nblk};
    for (int k = 0; k < n && k < 3; ++k) out[k] = v[k];
    return 3;
}

// device ranges whose tensors a step GEMM's 16 B staging may over-read by <= 12 B (as the engine registers its arenas)
void lsp_register_overread(const void* p, size_t bytes) { gc_register_overread_range(p, bytes); }
void lsp_unregister_overread(const void* p) { gc_unregister_overread_range(p); }

}  // extern "C"

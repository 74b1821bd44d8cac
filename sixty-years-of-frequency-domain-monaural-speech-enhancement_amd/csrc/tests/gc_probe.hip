// Test-only probe of the tap-table conv (gemmconv.hip): one conv or transposed-conv layer built and launched exactly as the
// engine builds and launches it (layers.hip make_conv_plan / run_conv, make_deconv_plan / run_deconv), on device buffers the
// caller owns, with a record of the geometry every dispatch took (gc_set_launch_log).  Plain C entry points for ctypes:
// tests/test_gpu_gemmconv_geometry.py compares the launches with a float64 reference.  Not linked into libse_engine.so.
#include "../layers.h"
#include "../kernels.h"
#include "../gauss.h"
#include "gc_selin_flat.h"
#include <string>
#include <vector>

using namespace se;

namespace {
thread_local std::string g_err;
thread_local std::vector<GCLaunchRec> g_log;
thread_local std::vector<GCSelIn> g_sel;

struct Probe {
    bool deconv = false;
    int M = 0, Cin = 0, C0 = 0;
    GCPlan conv;
    DeconvPlan dec;
    ~Probe() {
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

template <typename F>
int guarded(F&& f) {
    try {
        f();
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}
}  // namespace

extern "C" {

const char* gcp_last_error() { return g_err.c_str(); }

// w: [M][Cin][nkf][nkt] (row-major, frequency taps major); bias [M] or null; slope [M] (ACT_PRELU) or null.
// out[f][t] = sum w[kf][kt] x[f sf - pf + kf dil_f][t - pt_left + kt dil_t]; input channels >= c0split come from the second source
void* gcp_conv_create(const float* w, const float* bias, const float* slope, int M, int Cin, int nkf, int nkt, int sf, int pf,
                      int pt_left, int dil_f, int dil_t, int act, int epi, int c0split) {
    Probe* pr = nullptr;
    guarded([&] {
        auto* p = new Probe();
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

// w: [M][Cin][nkf][nkt] as above (M = output channels).
// out[fo][to] = sum_{(fo + pf - kf) % sf == 0} x[(fo + pf - kf) / sf][to + toff - kt] w[kf][kt]
void* gcp_deconv_create(const float* w, const float* bias, const float* slope, int M, int Cin, int nkf, int nkt, int sf, int pf,
                        int toff, int act, int epi, int c0split) {
    Probe* pr = nullptr;
    guarded([&] {
        auto* p = new Probe();
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

// DCCRN's (5, 2) layer with edge-row classes (gc_make_plan: edge_Fin / edge_Q), planned for rows of `tout` frames on a plane of
// edge_Fin input rows: deconv = 0 the conv (frequency stride 2, pad 2, one frame of look-back, as make_conv_plan(w, 2, 2, 1, 1, 1, ..)),
// else both parity classes of its transposed form (make_deconv_plan(w, 2, 2, toff, ..)).  w [M][Cin][5][2].  Run with gcp_run.
// edge_Fin = 0: the same plans without classes
void* gcp_edge_create(const float* w, const float* bias, const float* slope, int M, int Cin, int deconv, int toff, int act, int c0split,
                      int tout, int edge_Fin) {
    Probe* pr = nullptr;
    guarded([&] {
        auto* p = new Probe();
        p->M = M;
        p->Cin = Cin;
        p->C0 = c0split < 0 ? Cin : c0split;
        p->deconv = deconv != 0;
        const DenseW d = dense(w, bias, M, Cin, 5, 2);
        const std::vector<float> sl = slope ? std::vector<float>(slope, slope + M) : std::vector<float>();
        try {
            if (!deconv) {
                p->conv = gc_make_plan(M, Cin, gauss::conv52_taps(), d.w, d.bias, sl, act, EPI_ACT, 2, 1, 0, tout, 1, c0split, edge_Fin, edge_Fin / 2);
            } else {
                p->dec.sf = 2;
                for (int par = 0; par < 2; ++par) {
                    std::vector<int> sel;
                    const TapSpec ts = gauss::deconv52_taps(par, toff, sel);
                    std::vector<float> wc((size_t)M * Cin * ts.ntaps);
                    for (int m = 0; m < M; ++m)
                        for (int c = 0; c < Cin; ++c)
                            for (int j = 0; j < ts.ntaps; ++j) wc[((size_t)m * Cin + c) * ts.ntaps + j] = d.w[((size_t)m * Cin + c) * 10 + sel[j]];
                    p->dec.par.push_back(gc_make_plan(M, Cin, ts, wc, d.bias, sl, act, EPI_ACT, 1, 2, par, tout, 1, c0split, edge_Fin, edge_Fin));
                }
            }
        } catch (...) {
            delete p;
            throw;
        }
        pr = p;
    });
    return pr;
}
// edge-row classes of plan `cls`: [0] classes built, [1] class of row 0, [2] class of row Q - 1, [3] Fin, [4] Q, [5] K rows per
// chunk of class 0, [6] / [7] of classes 1 / 2
int gcp_edge_info(void* h, int cls, int* out, int n) {
    const Probe* p = static_cast<const Probe*>(h);
    const int np = p->deconv ? (int)p->dec.par.size() : 1;
    if (cls < 0 || cls >= np) return -1;
    const GCPlan& g = p->deconv ? p->dec.par[cls] : p->conv;
    const int v[8] = {g.edge.nclass, g.edge.cls_lo, g.edge.cls_hi, g.edge.Fin, g.edge.Q, g.p.KCp, g.edge.KCp[0], g.edge.KCp[1]};
    for (int i = 0; i < n && i < 8; ++i) out[i] = v[i];
    return 8;
}

void gcp_destroy(void* h) { delete static_cast<Probe*>(h); }

// facts of plan `cls` (a transposed conv: its parity class; a conv: 0) that decide a launch's geometry: [0] BM, [1] BN,
// [2] plans (parity classes), [3] on-the-fly InstanceNorm supported (whole layer), [4] statistics supported (whole layer),
// [5] LDS columns per flattened unit (0: none), [6] direct (<= 4 channel) path, [7] 128-column flattened geometry,
// [8] 256-column flattened geometry, [9] 256-column plain geometry, [10] two-row geometry, [11] 64-column geometry,
// [12] 32-column tail geometry, [13] channels per staged chunk, [14] patch rows, [15] LDS row stride of the 256-column
// geometry, [16] tail launches allowed, [17] output parity (po), [18] output row stride (so)
int gcp_info(void* h, int cls, int* out, int n) {
    const Probe* p = static_cast<const Probe*>(h);
    const int np = p->deconv ? (int)p->dec.par.size() : 1;
    if (cls < 0 || cls >= np) return -1;
    const GCPlan& g = p->deconv ? p->dec.par[cls] : p->conv;
    const int v[19] = {g.BM,
                       g.BN,
                       np,
                       p->deconv ? (int)deconv_nrm_supported(p->dec) : (int)conv_nrm_supported(p->conv),
                       p->deconv ? (int)deconv_stats_supported(p->dec) : (int)conv_stats_supported(p->conv),
                       g.flat_uw,
                       g.p.Ws != nullptr,
                       g.geom[GC_G_FLAT128].BN,
                       g.geom[GC_G_FLAT256].BN,
                       g.geom[GC_G_N256].BN,
                       g.geom[GC_G_QT2].BN,
                       g.geom[GC_G_N64].BN,
                       g.geom[GC_G_N32].BN,
                       g.p.CI_C,
                       g.p.nrows,
                       g.geom[GC_G_N256].Wp,
                       (int)g.tail_split,
                       g.p.po,
                       g.p.so};
    for (int i = 0; i < n && i < 19; ++i) out[i] = v[i];
    return 19;
}

// One layer launch on the null stream, synchronised on both sides.  Sources [B][C][Fin][Tp] (x1 / nrm1: the channels >= c0split);
// nrm*: [B][C] float4 {scale, shift, slope - 1, -shift / scale} or null; dst [B][dstC][Fout][Tp]; stats (optional)
// [B][dstC][Fout][ceil(T / 32)][2]; tlen (optional, device [B]): the ragged rows' frame counts, published as the engine does.
int gcp_run(void* h, const float* x0, const float* nrm0, const float* x1, const float* nrm1, int Fin, float* dst, int dstC, int Fout,
            int B, int T, int Tp, float* stats, const int* tlen) {
    return guarded([&] {
        const Probe* p = static_cast<const Probe*>(h);
        SE_CHECK(p->C0 == p->Cin || x1, "gcp_run: the plan has a second source");
        const Act4 a0 = act4(x0, p->C0, Fin, Tp).with_nrm(nrm0);
        const Act4 a1 = act4(x1, p->Cin - p->C0, Fin, Tp).with_nrm(nrm1);
        const Act4* s1 = p->C0 < p->Cin ? &a1 : nullptr;
        Ragged rg;
        rg.tlen = tlen;
        SE_HIP(hipDeviceSynchronize());
        g_log.clear();
        g_sel.clear();
        gc_set_launch_log(&g_log);
        gc_set_select_log(&g_sel);
        if (tlen) set_ragged_ctx(&rg);
        try {
            if (p->deconv) run_deconv(p->dec, a0, s1, dst, dstC, Fout, B, T, Tp, 0, nullptr, stats);
            else run_conv(p->conv, a0, s1, dst, dstC, Fout, B, T, Tp, 0, nullptr, stats);
        } catch (...) {
            set_ragged_ctx(nullptr);
            gc_set_launch_log(nullptr);
            gc_set_select_log(nullptr);
            throw;
        }
        set_ragged_ctx(nullptr);
        gc_set_launch_log(nullptr);
        gc_set_select_log(nullptr);
        SE_HIP(hipDeviceSynchronize());
    });
}

// dispatches of the last gcp_run
int gcp_launch_count() { return (int)g_log.size(); }
// fields of dispatch i: family, BM, BN, flat_upr, upt, flat_rows, qt2, nrm, res, trim, stats, ragged, flat_nrm_refused, nblk
int gcp_launch_get(int i, long long* out, int n) {
    if (i < 0 || i >= (int)g_log.size()) return -1;
    const GCLaunchRec& r = g_log[i];
    const long long v[14] = {r.family, r.BM,    r.BN,     r.flat_upr, r.upt,  r.flat_rows,        r.qt2,
                             r.nrm,    r.res,   r.trim,   r.stats,    r.ragged, r.flat_nrm_refused, r.nblk};
    for (int k = 0; k < n && k < 14; ++k) out[k] = v[k];
    return 14;
}

// gc_launch calls of the last gcp_run, and what call i gave gc_select: GCSelIn as GC_SELIN_FIELDS integers in the order of the
// struct's declaration (gc_selin_flat.h; tests/test_gc_select_host.py SELIN names them)
int gcp_select_count() { return (int)g_sel.size(); }
int gcp_select_get(int i, long long* out, int n) {
    if (i < 0 || i >= (int)g_sel.size() || n < GC_SELIN_FIELDS) return -1;
    gc_selin_flatten(g_sel[i], out);
    return GC_SELIN_FIELDS;
}

int gcp_flat_rows_spanned(int B, int upr, int upt) { return gc_flat_rows_spanned(B, upr, upt); }

// device ranges whose tensors the 16 B staging may over-read by <= 12 B (as the engine registers its arenas)
void gcp_register_overread(const void* p, size_t bytes) { gc_register_overread_range(p, bytes); }
void gcp_unregister_overread(const void* p) { gc_unregister_overread_range(p); }

}  // extern "C"

// Test-only probe of the tap-table conv's epilogues and of the three-product complex layers (gauss.h): one conv / transposed-conv
// layer with the full argument set of make_conv_plan / make_deconv_plan (any activation, EPI_ACT / ADD / MUL / GLU, dilation, two
// sources, a post-gate BatchNorm, a left frequency pad with its own bias) launched through run_conv / run_deconv with every optional
// operand (aux, dst_elu, the statistics riders, fz, ragged rows), and one gauss::GaussLayer built and run as model_dccrn.hip /
// model_uformer.hip build and run theirs.  Plain C entry points for ctypes (tests/test_gpu_conv_epilogues.py), with the record of
// every dispatch (gc_set_launch_log).  Not linked into libse_engine.so.
#include "../gauss.h"
#include "../kernels.h"
#include "../layers.h"
#include <string>
#include <vector>

using namespace se;

namespace {
thread_local std::string g_err;
thread_local std::vector<GCLaunchRec> g_log;

struct Layer {
    bool deconv = false;
    int M = 0, Cin = 0, C0 = 0;
    GCPlan conv;
    DeconvPlan dec;
    ~Layer() {
        if (deconv) free_deconv_plan(dec);
        else gc_free_plan(conv);
    }
};
struct Gauss {
    gauss::GaussLayer g;
    int ci = 0, C0 = 0;
    ~Gauss() { g.free(); }
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
HostTensor host(const float* v, int n) {
    HostTensor t;
    t.shape = {n};
    t.data.assign(v, v + n);
    return t;
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

// the launch log and the ragged rows around one call, taken down again whatever the call does
template <typename F>
void logged(const int* tlen, F&& f) {
    Ragged rg;
    rg.tlen = tlen;
    SE_HIP(hipDeviceSynchronize());
    g_log.clear();
    gc_set_launch_log(&g_log);
    if (tlen) set_ragged_ctx(&rg);
    try {
        f();
    } catch (...) {
        set_ragged_ctx(nullptr);
        gc_set_launch_log(nullptr);
        throw;
    }
    set_ragged_ctx(nullptr);
    gc_set_launch_log(nullptr);
    SE_HIP(hipDeviceSynchronize());
}

// the residual / factor of EPI_ADD / EPI_MUL on a shallow copy of the plan, laid out like dst (blocks.h run_tcm, model_uformer.hip
// pointwise layers: x_f = 0 on tensors of one frequency row)
void set_aux(GCParams& p, const float* aux, int dstC, int Fout, int Tp, bool xf0) {
    p.aux = aux;
    p.x_b = (long)dstC * Fout * Tp;
    p.x_c = (long)Fout * Tp;
    p.x_f = xf0 ? 0 : Tp;
}
}  // namespace

extern "C" {

const char* epp_last_error() { return g_err.c_str(); }

// w: [M][Cin][nkf][nkt]; bias [M] or null; slope [M] or null (EPI_GLU: [M / 2]); post_bn: null or 4 x [M / 2] {gamma, beta, mean, var}
// (EPI_GLU: set_post_bn).  out[f][t] = sum w[kf][kt] x[f sf - pf + kf dil_f][t - pt_left + kt dil_t]
void* epp_conv_create(const float* w, const float* bias, const float* slope, int nslope, const float* post_bn, int M, int Cin, int nkf,
                      int nkt, int sf, int pf, int pt_left, int dil_f, int dil_t, int act, int epi, int c0split) {
    Layer* out = nullptr;
    guarded([&] {
        auto* p = new Layer();
        p->M = M;
        p->Cin = Cin;
        p->C0 = c0split < 0 ? Cin : c0split;
        const std::vector<float> sl = slope ? std::vector<float>(slope, slope + nslope) : std::vector<float>();
        try {
            p->conv = make_conv_plan(dense(w, bias, M, Cin, nkf, nkt), sf, pf, pt_left, dil_f, dil_t, act, sl, epi, 401, c0split);
            if (post_bn) {
                const int h = M / 2;
                set_post_bn(p->conv, host(post_bn, h), host(post_bn + h, h), host(post_bn + 2 * h, h), host(post_bn + 3 * h, h));
            }
        } catch (...) {
            delete p;
            throw;
        }
        out = p;
    });
    return out;
}

// out[fo][to] = sum_{(fo + pf - kf) % sf == 0} x[(fo + pf - kf) / sf][to + toff - kt] w[kf][kt]; pf < 0: bias_pad [M] is the bias
// of the output rows fo < -pf
void* epp_deconv_create(const float* w, const float* bias, const float* slope, int nslope, const float* post_bn, const float* bias_pad,
                        int M, int Cin, int nkf, int nkt, int sf, int pf, int toff, int act, int epi, int c0split) {
    Layer* out = nullptr;
    guarded([&] {
        auto* p = new Layer();
        p->deconv = true;
        p->M = M;
        p->Cin = Cin;
        p->C0 = c0split < 0 ? Cin : c0split;
        const std::vector<float> sl = slope ? std::vector<float>(slope, slope + nslope) : std::vector<float>();
        const std::vector<float> bp = bias_pad ? std::vector<float>(bias_pad, bias_pad + M) : std::vector<float>();
        try {
            p->dec = make_deconv_plan(dense(w, bias, M, Cin, nkf, nkt), sf, pf, toff, act, sl, 401, c0split, bias_pad ? &bp : nullptr, epi);
            if (post_bn) {
                const int h = M / 2;
                for (auto& g : p->dec.par)
                    set_post_bn(g, host(post_bn, h), host(post_bn + h, h), host(post_bn + 2 * h, h), host(post_bn + 3 * h, h));
            }
        } catch (...) {
            delete p;
            throw;
        }
        out = p;
    });
    return out;
}
void epp_destroy(void* h) { delete static_cast<Layer*>(h); }

// [0] BM, [1] BN, [2] plans, [3] direct path, [4] statistics supported, [5] folds the branch interaction, [6] zeroes ragged tails,
// [7] pair launch (both parity classes on the direct path)
int epp_info(void* h, int* out, int n) {
    const Layer* p = static_cast<const Layer*>(h);
    const GCPlan& g = p->deconv ? p->dec.par[0] : p->conv;
    const int v[8] = {g.BM,
                      g.BN,
                      p->deconv ? (int)p->dec.par.size() : 1,
                      g.p.Ws != nullptr,
                      p->deconv ? (int)deconv_stats_supported(p->dec) : (int)conv_stats_supported(p->conv),
                      p->deconv ? (int)conv_folds_interaction(p->dec) : (int)conv_folds_interaction(p->conv),
                      p->deconv ? (int)conv_zeroes_tail(p->dec) : (int)conv_zeroes_tail(p->conv),
                      p->deconv ? (int)p->dec.has_pair : 0};
    for (int i = 0; i < n && i < 8; ++i) out[i] = v[i];
    return 8;
}

// One layer launch on the null stream, synchronised on both sides.  Sources [B][C][Fin][Tp]; dst [B][dstC][Fout][Tp]; aux
// (EPI_ADD / EPI_MUL) and dst_elu (EPI_GLU, convs) laid out like dst; stats [B][dstC][Fout][ceil(T / 32)][2] or, with colstats,
// [B][Fout][T][2]; fz [B][fz_planes * dstC][Fout][Tp] (three planes: S | R | I); tlen device [B]
int epp_run(void* h, const float* x0, const float* x1, int Fin, float* dst, int dstC, int Fout, int B, int T, int Tp, const float* aux,
            int aux_xf0, float* dst_elu, float* stats, int colstats, float* fz, int fz_planes, const int* tlen) {
    return guarded([&] {
        const Layer* p = static_cast<const Layer*>(h);
        SE_CHECK(p->C0 == p->Cin || x1, "epp_run: the plan has a second source");
        SE_CHECK(!aux_xf0 || Fout == 1, "epp_run: x_f = 0 is the form of one-row tensors");
        SE_CHECK(!dst_elu || !p->deconv, "epp_run: run_deconv has no second (ELU) store");
        const Act4 a0 = act4(x0, p->C0, Fin, Tp);
        const Act4 a1 = act4(x1, p->Cin - p->C0, Fin, Tp);
        const Act4* s1 = p->C0 < p->Cin ? &a1 : nullptr;
        float* fzp = fz && fz_planes == 3 ? fz + (long)dstC * Fout * Tp : fz;      // three planes: fz names the R plane
        logged(tlen, [&] {
            if (p->deconv) {
                DeconvPlan d = p->dec;      // (shallow: the device tables stay the layer's)
                if (aux)
                    for (auto& g : d.par) set_aux(g.p, aux, dstC, Fout, Tp, aux_xf0 != 0);
                run_deconv(d, a0, s1, dst, dstC, Fout, B, T, Tp, 0, nullptr, stats, 0, -1, false, fzp, fz_planes, colstats != 0);
            } else {
                GCPlan c = p->conv;
                if (aux) set_aux(c.p, aux, dstC, Fout, Tp, aux_xf0 != 0);
                run_conv(c, a0, s1, dst, dstC, Fout, B, T, Tp, 0, nullptr, stats, 0, fzp, fz_planes, colstats != 0, dst_elu);
            }
        });
    });
}

// dispatches of the last run
int epp_launch_count() { return (int)g_log.size(); }
// fields of dispatch i: family, BM, BN, form, Z, epi, qt2, res, trim, stats, ragged, flat_upr, nblk
int epp_launch_get(int i, long long* out, int n) {
    if (i < 0 || i >= (int)g_log.size()) return -1;
    const GCLaunchRec& r = g_log[i];
    const long long v[13] = {r.family, r.BM, r.BN, r.form, r.Z, r.epi, r.qt2, r.res, r.trim, r.stats, r.ragged, r.flat_upr, r.nblk};
    for (int k = 0; k < n && k < 13; ++k) out[k] = v[k];
    return 13;
}

void epp_register_overread(const void* p, size_t bytes) { gc_register_overread_range(p, bytes); }
void epp_unregister_overread(const void* p) { gc_unregister_overread_range(p); }

// ---- three-product layers.  wr / wi [co][ci][5][2]; bias, bn = {gamma, beta, mean, var}, slope: [2 co] rows [real; imag]
// deconv = 0: the (5, 2) conv, frequency stride 2, pad 2, one frame of look-back; else its transposed form with toff / c0split
static void* gauss_create(const float* wr, const float* wi, const float* bias, const float* bn, const float* slope, int co, int ci, int deconv,
                          int toff, int c0split, int tout, int edge_Fin) {
    Gauss* out = nullptr;
    guarded([&] {
        auto* p = new Gauss();
        p->ci = ci;
        p->C0 = c0split < 0 ? ci : c0split;
        try {
            const DenseW dr = dense(wr, nullptr, co, ci, 5, 2), di = dense(wi, nullptr, co, ci, 5, 2);
            if (deconv) gauss::make_deconv_plans(p->g, dr, di, toff, c0split, tout, edge_Fin);
            else gauss::make_conv_plans(p->g, dr, di, tout, edge_Fin);
            const int n = 2 * co;
            gauss::fold_tail(p->g, std::vector<float>(bias, bias + n), host(bn, n), host(bn + n, n), host(bn + 2 * n, n), host(bn + 3 * n, n),
                             std::vector<float>(slope, slope + n));
        } catch (...) {
            delete p;
            throw;
        }
        out = p;
    });
    return out;
}
void* epp_gauss_create(const float* wr, const float* wi, const float* bias, const float* bn, const float* slope, int co, int ci, int deconv,
                       int toff, int c0split) {
    return gauss_create(wr, wi, bias, bn, slope, co, ci, deconv, toff, c0split, 401, 0);
}
// the same layer planned for rows of `tout` frames, with edge-row classes for a plane of edge_Fin input rows (0: none)
void* epp_gauss_create_edge(const float* wr, const float* wi, const float* bias, const float* bn, const float* slope, int co, int ci,
                            int deconv, int toff, int c0split, int tout, int edge_Fin) {
    return gauss_create(wr, wi, bias, bn, slope, co, ci, deconv, toff, c0split, tout, edge_Fin);
}
// edge-row classes of the layer's plan `cls`: [0] classes built, [1] class of row 0, [2] class of row Q - 1
int epp_gauss_edge_info(void* h, int cls, int* out) {
    const Gauss* p = static_cast<const Gauss*>(h);
    if (cls < 0 || cls >= (int)p->g.pl.size()) return -1;
    const GCEdgeShape& e = p->g.pl[cls].edge;
    out[0] = e.nclass; out[1] = e.cls_lo; out[2] = e.cls_hi;
    return 3;
}
void epp_gauss_destroy(void* h) { delete static_cast<Gauss*>(h); }

// src0 / src1: three-plane tensors [B][3 C][Fin][T] of C0 / ci - C0 complex channels; dst [B][(dst3 ? 3 : 2) co][Fout][T]; K: scratch
int epp_gauss_run(void* h, const float* src0, const float* src1, int Fin, int Fout, int B, int T, float* dst, int dst3, int sum_plane, float* K,
                  const int* tlen) {
    return guarded([&] {
        const Gauss* p = static_cast<const Gauss*>(h);
        SE_CHECK(p->C0 == p->ci || src1, "epp_gauss_run: the layer has a second source");
        Profiler pf;      // (on = false)
        logged(tlen, [&] {
            gauss::run_layer(p->g, src0, p->C0, p->C0 < p->ci ? src1 : nullptr, p->ci - p->C0, Fin, Fout, B, T, dst, dst3 != 0, sum_plane != 0, K,
                             0, &pf);
        });
    });
}
// t3 [B][3 C][F][T]: S = R + I
int epp_gauss_sum(float* t3, int B, int C, int F, int T) {
    return guarded([&] {
        Profiler pf;
        SE_HIP(hipDeviceSynchronize());
        gauss::launch_sum(t3, B, C, F, T, 0, &pf);
        SE_HIP(hipDeviceSynchronize());
    });
}
// x2 [B][2][CP] -> x3 [B][3][CP] = [R + I | R | I]
int epp_gauss_planes23(const float* x2, float* x3, int B, long CP) {
    return guarded([&] {
        Profiler pf;
        SE_HIP(hipDeviceSynchronize());
        gauss::launch_planes23(x2, x3, B, CP, 0, &pf);
        SE_HIP(hipDeviceSynchronize());
    });
}

}  // extern "C"

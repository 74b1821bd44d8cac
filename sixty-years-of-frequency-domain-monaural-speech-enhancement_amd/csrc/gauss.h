// Gauss' three-product complex (de)conv: the kernels, the per-layer record, its builders and its launchers, shared by the models
// that run their wide complex layers this way (model_dccrn.hip, model_uformer.hip).  DESIGN.md 3.6.
#pragma once
#include "common.h"
#include "gemmconv.h"
#include "kernels.h"
#include "layers.h"
#include <vector>

namespace se {
namespace gauss {

// ---- Gauss' three-product complex (de)conv (measure it) -------------------------------------------------
// The reference computes a complex conv as four real ones (complexnn: r2r - i2i, r2i + i2r); the engine runs them as ONE real
// conv over the 2 x 2 block matrix.  Gauss: k1 = Wr (xr + xi), k2 = (Wi - Wr) xr, k3 = (Wr + Wi) xi, yr = k1 - k3, yi = k1 + k2 -
// three real convs of half the rows and half the K: 3/4 of the matrix instructions.  Here as a GROUPED launch of the same
// gc_kernel (blockIdx.z = product, sources = the planes [xr + xi | xr | xi] of a three-plane tensor, outputs k1..k3 in a scratch
// tensor) and one elementwise pass that combines them, applies BatchNorm / bias / PReLU and writes the next layer's three planes.
// tools/gcbench.cpp `gauss` (profiles/r04_gauss_gcbench.log): 128 -> 128 complex channels 0.81x the block GEMM's time, 64 -> 128
// 0.87x, 32 -> 64 0.97x, 16 -> 32 1.28x (the combine pass is as big as the GEMM there) - so the layers with >= 128 complex output
// channels take this path: encoder 3 - 5, decoder 0 - 1 (50 % of the step).  Rounding: the products are formed on sums of
// weights / inputs - 4e-7 ... 1e-6 relative per layer against the four-product form (bar 1e-4 on the waveform).
// x3 [B][3 C][P] planes (S | R | I): S = R + I
static __global__ __launch_bounds__(256) void gauss_sum_kernel(float* __restrict__ x3, long CP) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4, b = blockIdx.y;
    if (i >= CP) return;
    float* xb = x3 + b * 3 * CP;
    if (i + 3 < CP && (CP & 3) == 0) {
        const float4 r = *reinterpret_cast<const float4*>(xb + CP + i), m = *reinterpret_cast<const float4*>(xb + 2 * CP + i);
        *reinterpret_cast<float4*>(xb + i) = make_float4(r.x + m.x, r.y + m.y, r.z + m.z, r.w + m.w);
    } else {
        for (long j = i; j < CP && j < i + 4; ++j) xb[j] = xb[CP + j] + xb[2 * CP + j];
    }
}
// k [3][B][Co][F][T] -> y: yr = act((k1 - k3) sc[c] + sh[c]), yi = act((k1 + k2) sc[Co + c] + sh[Co + c]); planes of batch item b at
// y + b ob + {oS, oR, oI} (oS < 0: no sum plane); frames >= tlen[b] are stored as zeros (ragged rows: the decoder looks ahead)
static __global__ __launch_bounds__(128) void gauss_combine_kernel(const float* __restrict__ k, float* __restrict__ y, int Co, int F, int T,
                                                            long kz, long ob, long oS, long oR, long oI,
                                                            const float* __restrict__ sc, const float* __restrict__ sh,
                                                            const float* __restrict__ slope, const int* __restrict__ tlen) {
    const int f = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const long row = (((long)b * Co + c) * F + f) * T, orow = (long)b * ob + ((long)c * F + f) * T;
    const float s_r = sc[c], h_r = sh[c], s_i = sc[Co + c], h_i = sh[Co + c], a_r = slope[c], a_i = slope[Co + c];
    const int tv = tlen ? tlen[b] : T;
    const bool v4 = (T & 3) == 0;
    for (int t = threadIdx.x * 4; t < T; t += 512) {
        float k1[4], k2[4], k3[4], yr[4], yi[4];
        if (v4) {
            *reinterpret_cast<float4*>(k1) = *reinterpret_cast<const float4*>(k + row + t);
            *reinterpret_cast<float4*>(k2) = *reinterpret_cast<const float4*>(k + kz + row + t);
            *reinterpret_cast<float4*>(k3) = *reinterpret_cast<const float4*>(k + 2 * kz + row + t);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int tt = min(t + j, T - 1);
                k1[j] = k[row + tt]; k2[j] = k[kz + row + tt]; k3[j] = k[2 * kz + row + tt];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float r = (k1[j] - k3[j]) * s_r + h_r, m = (k1[j] + k2[j]) * s_i + h_i;
            r = r >= 0.f ? r : a_r * r;
            m = m >= 0.f ? m : a_i * m;
            const bool live = t + j < tv;
            yr[j] = live ? r : 0.f;
            yi[j] = live ? m : 0.f;
        }
        if (v4) {
            *reinterpret_cast<float4*>(y + orow + oR + t) = *reinterpret_cast<const float4*>(yr);
            *reinterpret_cast<float4*>(y + orow + oI + t) = *reinterpret_cast<const float4*>(yi);
            if (oS >= 0) *reinterpret_cast<float4*>(y + orow + oS + t) = make_float4(yr[0] + yi[0], yr[1] + yi[1], yr[2] + yi[2], yr[3] + yi[3]);
        } else {
            for (int j = 0; j < 4 && t + j < T; ++j) {
                y[orow + oR + t + j] = yr[j];
                y[orow + oI + t + j] = yi[j];
                if (oS >= 0) y[orow + oS + t + j] = yr[j] + yi[j];
            }
        }
    }
}
struct GaussLayer {
    std::vector<GCPlan> pl;      // encoder: one grouped plan (Z = 3); decoder: one per output-parity class
    float *sc = nullptr, *sh = nullptr, *slope = nullptr;      // [2 co] rows [real; imag]
    int co = 0;
    void free() {
        for (auto& g : pl) gc_free_plan(g);
        pl.clear();
        for (float** p : {&sc, &sh, &slope})
            if (*p) { (void)hipFree(*p); *p = nullptr; }
    }
};
// the combine's per-row parameters (rows [real; imag] of 2 co): eval BatchNorm and the conv's row bias as scale / shift, the PReLU
// slopes.  bias and the BatchNorm tensors are [2 co] (a BatchNorm shared by both parts comes duplicated: Uformer's dup2)
inline void fold_tail(GaussLayer& g, const std::vector<float>& bias, const HostTensor& ga, const HostTensor& be, const HostTensor& mu,
                      const HostTensor& va, const std::vector<float>& slope) {
    const int n = 2 * g.co;
    SE_CHECK((int)bias.size() == n && (int)ga.numel() == n && (int)be.numel() == n && (int)mu.numel() == n && (int)va.numel() == n &&
                 (int)slope.size() == n, "three-product layer: BatchNorm / bias / PReLU row count");
    std::vector<float> sc(n), sh(n);
    for (int m = 0; m < n; ++m) {
        const double k = (double)ga.data[m] / std::sqrt((double)va.data[m] + 1e-5);
        sc[m] = (float)k;
        sh[m] = (float)((double)be.data[m] - (double)mu.data[m] * k + (double)bias[m] * k);
    }
    g.sc = to_device(sc);
    g.sh = to_device(sh);
    g.slope = to_device(slope);
}

// a two-plane tensor [B][2 C][P] = [R | I] -> three planes [B][3 C][P] = [R + I | R | I] (a tensor produced by block-form layers
// that a three-product layer reads)
static __global__ __launch_bounds__(256) void gauss_planes23_kernel(const float* __restrict__ x2, float* __restrict__ x3, long CP) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4, b = blockIdx.y;
    if (i >= CP) return;
    const float* xb = x2 + b * 2 * CP;
    float* yb = x3 + b * 3 * CP;
    if (i + 3 < CP && (CP & 3) == 0) {
        const float4 r = *reinterpret_cast<const float4*>(xb + i), m = *reinterpret_cast<const float4*>(xb + CP + i);
        *reinterpret_cast<float4*>(yb + i) = make_float4(r.x + m.x, r.y + m.y, r.z + m.z, r.w + m.w);
        *reinterpret_cast<float4*>(yb + CP + i) = r;
        *reinterpret_cast<float4*>(yb + 2 * CP + i) = m;
    } else {
        for (long j = i; j < CP && j < i + 4; ++j) {
            const float r = xb[j], m = xb[CP + j];
            yb[j] = r + m;
            yb[CP + j] = r;
            yb[2 * CP + j] = m;
        }
    }
}

// the three weight matrices of a layer, stacked along z: Wr | Wi - Wr | Wr + Wi
inline std::vector<float> three_products(const std::vector<float>& r, const std::vector<float>& i) {
    std::vector<float> w(3 * r.size());
    for (size_t k = 0; k < r.size(); ++k) { w[k] = r[k]; w[r.size() + k] = i[k] - r[k]; w[2 * r.size() + k] = r[k] + i[k]; }
    return w;
}
// tap sets as make_conv_plan(w, 2, 2, 1, 1, 1, ..) / one output-parity class of make_deconv_plan(w, 2, 2, toff, ..) build them
inline TapSpec conv52_taps() {
    TapSpec ts;
    ts.ntaps = 10;
    for (int kf = 0; kf < 5; ++kf)
        for (int kt = 0; kt < 2; ++kt) { ts.df[kf * 2 + kt] = kf - 2; ts.dt[kf * 2 + kt] = kt - 1; }
    return ts;
}
inline TapSpec deconv52_taps(int par, int toff, std::vector<int>& sel) {
    TapSpec ts;
    sel.clear();
    for (int kf = 0; kf < 5; ++kf) {
        const int num = par + 2 - kf;
        if (((num % 2) + 2) % 2 != 0) continue;
        for (int kt = 0; kt < 2; ++kt) {
            ts.df[ts.ntaps] = num / 2;
            ts.dt[ts.ntaps] = toff - kt;
            ts.ntaps++;
            sel.push_back(kf * 2 + kt);
        }
    }
    return ts;
}
// grouped plans of a (5, 2) conv, stride 2 along frequency (encoder) / of both parity classes of its transposed form (decoder;
// wr / wi: [co][ci][10] real matrices, ci = all complex input channels, the first c0split of them from the first source)
// edge_Fin > 0 (opt-in, the deep layers of DCCRN): the input plane's rows - output rows whose frequency taps partly lie outside it
// run on the live K rows only (gc_make_plan: edge classes)
inline void make_conv_plans(GaussLayer& g, const DenseW& wr, const DenseW& wi, int tout, int edge_Fin = 0) {
    g.co = wr.M;
    g.pl.push_back(gc_make_plan(wr.M, wr.Cin, conv52_taps(), three_products(wr.w, wi.w), {}, {}, ACT_NONE, EPI_ACT, 2, 1, 0, tout, 3, -1,
                                edge_Fin, edge_Fin / 2));
    g.pl.back().flop_scale = 4.0 / 3.0;          // the profiler books the reference's four products
}
inline void make_deconv_plans(GaussLayer& g, const DenseW& wr, const DenseW& wi, int toff, int c0split, int tout, int edge_Fin = 0) {
    const int co = wr.M, ci = wr.Cin;
    g.co = co;
    for (int par = 0; par < 2; ++par) {
        std::vector<int> sel;
        TapSpec ts = deconv52_taps(par, toff, sel);
        std::vector<float> r((size_t)co * ci * ts.ntaps), i(r.size());
        for (int m = 0; m < co; ++m)
            for (int c = 0; c < ci; ++c)
                for (int j = 0; j < ts.ntaps; ++j) {
                    r[((size_t)m * ci + c) * ts.ntaps + j] = wr.w[((size_t)m * ci + c) * 10 + sel[j]];
                    i[((size_t)m * ci + c) * ts.ntaps + j] = wi.w[((size_t)m * ci + c) * 10 + sel[j]];
                }
        g.pl.push_back(gc_make_plan(co, ci, ts, three_products(r, i), {}, {}, ACT_NONE, EPI_ACT, 1, 2, par, tout, 3, c0split, edge_Fin,
                                    edge_Fin));      // (each parity class makes Fin of the 2 Fin output rows)
        g.pl.back().flop_scale = 4.0 / 3.0;
    }
}

// ---- launchers.  A three-plane tensor [B][3 C][F][T]: S = R + I at +0, R at + C F T, I at + 2 C F T
inline Act4 view3(const float* t3, int C, int F, int T) {      // its [R | I] planes as a 2 C-channel tensor
    return Act4{t3 + (long)C * F * T, 2 * C, F, 3L * C * F * T, (long)F * T, (long)T};
}
static void launch_sum(float* t3, int B, int C, int F, int T, hipStream_t st, Profiler* pf) {      // S = R + I
    const long CP = (long)C * F * T;
    const bool timed = pf->on;
    if (timed) pf->begin(st);
    hipLaunchKernelGGL(gauss_sum_kernel, dim3((unsigned)((CP / 4 + 255) / 256 + 1), B), dim3(256), 0, st, t3, CP);
    SE_HIP(hipGetLastError());
    if (timed) pf->end(st, 0.0);
}
static void launch_planes23(const float* x2, float* x3, int B, long CP, hipStream_t st, Profiler* pf) {
    const bool timed = pf->on;
    if (timed) pf->begin(st);
    hipLaunchKernelGGL(gauss_planes23_kernel, dim3((unsigned)((CP / 4 + 255) / 256 + 1), B), dim3(256), 0, st, x2, x3, CP);
    SE_HIP(hipGetLastError());
    if (timed) pf->end(st, 0.0);
}
// y = PReLU(BN(complex (de)conv(x))) of one layer: the grouped three-product launch(es), then (without the combine epilogue) the
// combine pass.  src0 / src1: three-plane tensors of C0 / C1 complex channels (src1 = null: one source); dst3: a three-plane output
// (else [R | I] only); sum_plane (dst3 only): the layer stores S = R + I as well - else its caller does, as Uformer's folded branch
// interaction must; K: scratch of the products
static void run_layer(const GaussLayer& g, const float* src0, int C0, const float* src1, int C1, int Fin, int Fout, int B, int T,
                      float* dst, bool dst3, bool sum_plane, float* K, hipStream_t st, Profiler* pf) {
    SE_CHECK(dst3 || !sum_plane, "three-product layer: a sum plane needs a three-plane output");
    const int co = g.co;
    // SE_GAUSS_CMB=0: three products into scratch + the combine pass (round 4).  Rows of whole 16 B groups only (the combine
    // epilogue has no trimming variant; PadFrames gives every offline decode such rows)
    static const bool cmb_env = !(getenv("SE_GAUSS_CMB") && atoi(getenv("SE_GAUSS_CMB")) == 0);
    const bool cmb = cmb_env && T % 4 == 0 && co >= 64;
    const long CP = (long)co * Fout * T, kz = (long)B * CP, oR = dst3 ? CP : 0L, oI = dst3 ? 2 * CP : CP;
    const Ragged* rg = ragged_ctx();
    for (const GCPlan& pl : g.pl) {
        GCParams p = pl.p;
        p.src0 = src0; p.C0 = C0; p.s0_b = 3L * C0 * Fin * T; p.s0_c = (long)Fin * T; p.s0_f = T; p.src0_z = (long)C0 * Fin * T;
        if (src1) {
            p.src1 = src1; p.C1 = C1; p.s1_b = 3L * C1 * Fin * T; p.s1_c = (long)Fin * T; p.s1_f = T; p.src1_z = (long)C1 * Fin * T;
        } else {
            p.src1 = nullptr; p.C1 = 0;
        }
        p.Fin = Fin; p.Tin = T; p.B = B; p.Tout = T;
        p.Q = (Fout - p.po + p.so - 1) / p.so;
        p.dst = K; p.d_b = CP; p.d_c = (long)Fout * T; p.d_f = T; p.dst_z = kz;
        if (rg) p.tlen = rg->tlen;
        if (!cmb) {
            gc_launch_prof(pl, p, st, pf);
            continue;
        }
        // k1 = Wr (xr + xi) alone, then k2 / k3 as a grouped launch of two whose epilogue (EPI_CMB) reads k1 and stores the
        // finished planes: I = f(k1 + k2), R = f(k1 - k3) - no k2 / k3 scratch, no combine pass (round 4: 5 % of a step)
        GCParams p1 = p;
        p1.Z = 1;
        p1.tlen = nullptr;
        gc_launch_prof(pl, p1, st, pf);
        GCParams q = p;
        q.Z = 2;
        q.A = pl.p.A + pl.p.A_z;
        q.src0 = p.src0 + p.src0_z;
        if (src1) q.src1 = p.src1 + p.src1_z;
        q.epi = EPI_CMB;
        q.bias = nullptr;
        q.aux = K; q.x_b = p.d_b; q.x_c = p.d_c; q.x_f = p.d_f; q.aux_z = 0;
        q.post_scale = g.sc + co; q.post_shift = g.sh + co; q.slope = g.slope + co; q.ps_z = -co;
        q.cmb_neg = 2;                                   // z = 0: I = f(k1 + k2); z = 1: R = f(k1 - k3)
        q.dst = dst + oI; q.dst_z = oR - oI; q.d_b = (dst3 ? 3 : 2) * CP;
        if (!sum_plane) {
            gc_launch_prof(pl, q, st, pf);
            continue;
        }
        // I first, then R in a launch of its own whose epilogue reads the finished I and writes S = R + I with it - no gauss_sum
        // pass over the tensor (2.7 % of a DCCRN step; its 3 units of traffic become 1 re-read)
        GCParams qi = q;
        qi.Z = 1;
        gc_launch_prof(pl, qi, st, pf);
        GCParams qr = q;
        qr.Z = 1;
        qr.A = q.A + pl.p.A_z;
        qr.src0 = q.src0 + p.src0_z;
        if (src1) qr.src1 = q.src1 + p.src1_z;
        qr.post_scale = g.sc; qr.post_shift = g.sh; qr.slope = g.slope;
        qr.cmb_neg = 1;
        qr.dst = dst + oR;
        qr.cmb_i = dst + oI;
        qr.cmb_s = dst;
        gc_launch_prof(pl, qr, st, pf);
    }
    if (cmb) return;
    const bool timed = pf->on;
    if (timed) pf->begin(st);
    hipLaunchKernelGGL(gauss_combine_kernel, dim3(Fout, co, B), dim3(128), 0, st, K, dst, co, Fout, T, kz, dst3 ? 3 * CP : 2 * CP,
                       sum_plane ? 0L : -1L, oR, oI, g.sc, g.sh, g.slope, rg ? rg->tlen : nullptr);
    SE_HIP(hipGetLastError());
    if (timed) pf->end(st, 0.0);
}

}  // namespace gauss
}  // namespace se

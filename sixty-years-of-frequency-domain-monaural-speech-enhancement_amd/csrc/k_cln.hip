// CumulativeLayerNorm (the `_new` variants): its seven kernels and the one launcher that executes the choice of cln_select.h.
#include "kernels.h"
#include "common.h"
#include "cln_select.h"

namespace se {

// Frame t is normalised with the mean / variance of ALL rows of frames 0..t (CTSNet_new/Step1_network.py:213-286).
// x [B][R][T] with R = C * F rows (F = 1 for the 1-D flavour); three passes: per-frame sums over the rows, an
// in-LDS prefix scan per utterance, then normalise + affine (+ PReLU before / after, + the TCM branch FIR).
// Frame-online chunks (c0 > 0 / carry): only columns [c0, T) of the window are summed and scanned, the scan starts from
// the carried totals of the frames before column c0 (`tg0` = stream index of column 0; columns before the start of the
// stream do not count) and leaves the totals up to column c0 + n - 1 - the frames before the next window's column c0.
__global__ __launch_bounds__(256) void cln_stats_kernel(const float* __restrict__ x, const float* __restrict__ pre_slope,
                                                        double* __restrict__ sum, double* __restrict__ sq, int R, int F,
                                                        int T, int c0, int WP) {
    // WP columns per workgroup, 256 / WP threads share a column's rows (whole utterances: 64 x 4; narrow frame-online
    // windows put more threads on each column)
    __shared__ double sh[2][256];
    const int NL = 256 / WP, tl = threadIdx.x % WP, rg = threadIdx.x / WP, t = c0 + blockIdx.x * WP + tl, b = blockIdx.y;
    double s = 0.0, q = 0.0;
    if (t < T) {
        const float* xp = x + (long)b * R * T + t;
        auto take = [&](int r, float v) {
            if (pre_slope) v = v >= 0.f ? v : pre_slope[r / F] * v;
            s += v;
            q += (double)v * v;
        };
        int r = rg;
        for (; r + NL * (NU - 1) < R; r += NL * NU) {         // NU rows in flight per thread, summed in row order
            float xr[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) xr[u] = xp[(long)(r + NL * u) * T];
#pragma unroll
            for (int u = 0; u < NU; ++u) take(r + NL * u, xr[u]);
        }
        for (; r < R; r += NL) take(r, xp[(long)r * T]);
    }
    sh[0][rg * WP + tl] = s;
    sh[1][rg * WP + tl] = q;
    __syncthreads();
    if (rg == 0 && t < T) {
        double a = sh[0][tl], c = sh[1][tl];
        for (int l = 1; l < NL; ++l) {
            a += sh[0][l * WP + tl];
            c += sh[1][l * WP + tl];
        }
        sum[(long)b * T + t] = a;
        sq[(long)b * T + t] = c;
    }
}

// Running totals (sum a, sum of squares q) over cnt values -> the frame's mean and 1 / sqrt(var + eps), in double precision
__device__ __forceinline__ void cln_mean_rstd(double a, double q, double cnt, float& mean, float& rstd) {
    const double m = a / cnt;
    const double var = (q - 2.0 * m * a) / cnt + m * m;
    mean = (float)m;
    rstd = (float)(1.0 / sqrt(var + 1e-5));
}

// In-LDS inclusive prefix sums of sc[c0 .. T) and sc[T + c0 .. 2T), starting from (a0, q0), by ONE wave: a lane sums its contiguous
// segment, the 64 segment totals are scanned on the shuffle network, the lane walks its segment again with its offset.  The serial
// loop of rounds 2-5 (thread 0 over all frames, two dependent LDS round trips per frame) was 29 us for T = 416 - hidden behind the
// other utterances' blocks at batch 256, but 144 launches x 29 us = 4.2 of the 10 ms of a single clip's decode (round 6).
// Sums in double precision; only the association order differs from the serial loop (~1e-16 relative).
__device__ __forceinline__ void cln_wave_scan(double* sc, int T, int c0, double a0, double q0) {
    const int lane = threadIdx.x;            // (called by threads 0..63)
    const int n = T - c0, L = (n + 63) >> 6;
    const int lo = c0 + lane * L, hi = min(lo + L, T);
    double a = 0.0, q = 0.0;
    for (int t = lo; t < hi; ++t) {
        a += sc[t];
        q += sc[T + t];
    }
    double ia = a, iq = q;                   // inclusive scan of the segment totals
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double ua = __shfl_up(ia, o, 64), uq = __shfl_up(iq, o, 64);
        if (lane >= o) {
            ia += ua;
            iq += uq;
        }
    }
    // exclusive offset of this lane's segment: the inclusive totals of the lane in front.  (Not `ia - a`: a segment that holds frames
    // behind a ragged row's end would take their NaN - or, by cancellation, their magnitude - into its own live frames.)
    const double ea = __shfl_up(ia, 1, 64), eq = __shfl_up(iq, 1, 64);
    a = a0 + (lane ? ea : 0.0);
    q = q0 + (lane ? eq : 0.0);
    for (int t = lo; t < hi; ++t) {
        a += sc[t];
        q += sc[T + t];
        sc[t] = a;
        sc[T + t] = q;
    }
}

__global__ __launch_bounds__(256) void cln_scan_kernel(const double* __restrict__ sum, const double* __restrict__ sq,
                                                       float* __restrict__ mean, float* __restrict__ rstd, int R, int T,
                                                       int c0, long tg0, int n_new, double* __restrict__ carry,
                                                       const int32_t* __restrict__ origin) {
    extern __shared__ double sc[];       // [2][T]
    const int b = blockIdx.x;
    if (origin) tg0 -= origin[b];        // the row's own frame index of column 0 (wave-uniform: one read)
    for (int t = c0 + threadIdx.x; t < T; t += 256) {
        const bool live = tg0 + t >= 0;
        sc[t] = live ? sum[(long)b * T + t] : 0.0;
        sc[T + t] = live ? sq[(long)b * T + t] : 0.0;
    }
    __syncthreads();
    if (threadIdx.x < 64 && c0 < T) {
        cln_wave_scan(sc, T, c0, carry ? carry[2 * b] : 0.0, carry ? carry[2 * b + 1] : 0.0);
        // (the carry was read by every lane before any lane writes it: the wave runs in lockstep through the scan)
        const int tc = c0 + n_new - 1;
        const int L = (T - c0 + 63) >> 6;
        if (carry && tc >= c0 && tc < T && (int)threadIdx.x == (tc - c0) / L) {
            carry[2 * b] = sc[tc];
            carry[2 * b + 1] = sc[T + tc];
        }
    }
    __syncthreads();
    for (int t = c0 + threadIdx.x; t < T; t += 256) {
        const double cnt = (double)R * (double)(tg0 + t >= 0 ? tg0 + t + 1 : 1);
        cln_mean_rstd(sc[t], sc[T + t], cnt, mean[(long)b * T + t], rstd[(long)b * T + t]);
    }
}

// The scan with the per-frame sums handed over by the producing conv's epilogue (GCParams::cstats: parts [B][F][T][2] floats - per
// output row and frame the sums over all channels): the rows are added in double precision in row order, then the serial scan as above
__global__ __launch_bounds__(256) void cln_scan_parts_kernel(const float* __restrict__ parts, int F, float* __restrict__ mean,
                                                             float* __restrict__ rstd, int R, int T) {
    extern __shared__ double sc[];       // [2][T]
    const int b = blockIdx.x;
    const float2* pb = reinterpret_cast<const float2*>(parts) + (long)b * F * T;
    for (int t = threadIdx.x; t < T; t += 256) {
        double a = 0.0, q = 0.0;
        int f = 0;
        for (; f + 7 < F; f += 8) {           // eight rows in flight (one workgroup per utterance: the loads' latency is the pass)
            float2 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = pb[(long)(f + u) * T + t];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                a += v[u].x;
                q += v[u].y;
            }
        }
        for (; f < F; ++f) {
            const float2 v = pb[(long)f * T + t];
            a += v.x;
            q += v.y;
        }
        sc[t] = a;
        sc[T + t] = q;
    }
    __syncthreads();
    if (threadIdx.x < 64) cln_wave_scan(sc, T, 0, 0.0, 0.0);
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += 256) {
        const double cnt = (double)R * (double)(t + 1);
        cln_mean_rstd(sc[t], sc[T + t], cnt, mean[(long)b * T + t], rstd[(long)b * T + t]);
    }
}

__global__ __launch_bounds__(256) void cln_apply_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        const float* __restrict__ gain, const float* __restrict__ bias,
                                                        const float* __restrict__ pre_slope,
                                                        const float* __restrict__ post_slope, const float* __restrict__ fir,
                                                        int K, int R, int F, int T, int t_first, long tg0,
                                                        const int32_t* __restrict__ origin) {
    const int t = t_first + blockIdx.x * 256 + threadIdx.x, b = blockIdx.z;
    if (origin) tg0 -= origin[b];        // (b is a grid dimension: uniform over the workgroup)
    if (t >= T) return;
    const float* mu = mean + (long)b * T;
    const float* rs = rstd + (long)b * T;
    for (int r = blockIdx.y * 8; r < min(R, blockIdx.y * 8 + 8); ++r) {
        const int c = r / F;
        const float* xp = x + ((long)b * R + r) * T;
        const float g = gain[c], bt = bias[c], ps = pre_slope ? pre_slope[c] : 1.f;
        auto nrm = [&](int ti) {
            float v = xp[ti];
            v = v >= 0.f ? v : ps * v;
            return (v - mu[ti]) * rs[ti] * g + bt;
        };
        float o;
        if (K <= 0) {
            o = nrm(t);
            if (post_slope) o = o >= 0.f ? o : post_slope[c] * o;
        } else {
            o = 0.f;
            for (int k = 0; k < K; ++k) {
                const int ti = t - (K - 1) + k;
                if (tg0 + ti >= 0) o += fir[k] * nrm(ti);
            }
        }
        y[((long)b * R + r) * T + t] = o;
    }
}

// Offline form of the apply pass for the 2-D norms of the U-Net levels (no pre-activation, no FIR): one workgroup per (b, c) plane
// of F * T contiguous values, the utterance's per-frame (mean, rstd) in LDS, 16 B accesses with four of them in flight per thread
// (cln_apply_kernel above walks eight rows of one column with one 4 B load in flight: 8.7 ms per G2Net_new step for the traffic
// the InstanceNorm pass of the base model moved in 6.3), and the residual of the module's last level added here instead of by
// an add_kernel pass behind it (4 % / 7 % of a G2Net_new / TaylorSENet_new step).  res may alias y.
__global__ __launch_bounds__(256) void cln_apply_plane_kernel(const float* x, float* y, const float* __restrict__ mean,
                                                              const float* __restrict__ rstd, const float* __restrict__ gain,
                                                              const float* __restrict__ bias, const float* __restrict__ post_slope,
                                                              const float* res, int C, int F, int T) {
    extern __shared__ float cl_sm[];      // mu [T], rs [T]
    const int c = blockIdx.x % C, b = blockIdx.x / C, tid = threadIdx.x;
    float* mu = cl_sm;
    float* rs = cl_sm + T;
    for (int t = tid; t < T; t += 256) {
        mu[t] = mean[(long)b * T + t];
        rs[t] = rstd[(long)b * T + t];
    }
    __syncthreads();
    const int P = F * T;
    const float* xp = x + (long)blockIdx.x * P;
    float* yp = y + (long)blockIdx.x * P;
    const float* rp = res ? res + (long)blockIdx.x * P : nullptr;
    const float g = gain[c], bt = bias[c], sl = post_slope ? post_slope[c] : 1.f;
    auto one = [&](float v, int t, float r) {
        float o = (v - mu[t]) * rs[t] * g + bt;
        o = o >= 0.f ? o : sl * o;
        return rp ? o + r : o;
    };
    if (((((size_t)xp ^ (size_t)yp) & 15) == 0) && (!rp || ((((size_t)xp ^ (size_t)rp) & 15) == 0))) {
        const int head = min(P, (int)((4 - (((size_t)xp >> 2) & 3)) & 3));
        if (tid < head) yp[tid] = one(xp[tid], tid % T, rp ? rp[tid] : 0.f);
        const int n4 = (P - head) >> 2;
        const float4* x4 = reinterpret_cast<const float4*>(xp + head);
        float4* y4 = reinterpret_cast<float4*>(yp + head);
        const float4* r4 = rp ? reinterpret_cast<const float4*>(rp + head) : nullptr;
        auto f4 = [&](float4 v, float4 r, int t) {        // t: frame of the first element (< T); the group may wrap into the next row
            float in[4] = {v.x, v.y, v.z, v.w}, rr[4] = {r.x, r.y, r.z, r.w}, o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int tk = t + k;
                if (tk >= T) {      // (T <= 2 - a one- or two-frame spectrogram through se_forward: the group wraps more than once)
                    tk -= T;
                    if (tk >= T) tk %= T;
                }
                o[k] = one(in[k], tk, rr[k]);
            }
            return make_float4(o[0], o[1], o[2], o[3]);
        };
        constexpr int NV = 4;
        const int step1 = 1024 % T;                    // frames one 256-thread sweep of 16 B groups advances, mod T
        int i = tid;
        int t = (head + 4 * tid) % T;
        for (; i + (NV - 1) * 256 < n4; i += NV * 256) {
            float4 v[NV], r[NV];
            int tu[NV];
#pragma unroll
            for (int u = 0; u < NV; ++u) {
                v[u] = x4[i + u * 256];
                r[u] = r4 ? r4[i + u * 256] : make_float4(0.f, 0.f, 0.f, 0.f);
                tu[u] = t;
                t += step1;
                t = t >= T ? t - T : t;
            }
#pragma unroll
            for (int u = 0; u < NV; ++u) y4[i + u * 256] = f4(v[u], r[u], tu[u]);
        }
        for (; i < n4; i += 256) {
            y4[i] = f4(x4[i], r4 ? r4[i] : make_float4(0.f, 0.f, 0.f, 0.f), t);
            t += step1;
            t = t >= T ? t - T : t;
        }
        const int done = head + 4 * n4;
        if (done + tid < P) yp[done + tid] = one(xp[done + tid], (done + tid) % T, rp ? rp[done + tid] : 0.f);
        return;
    }
    for (int i = tid; i < P; i += 256) yp[i] = one(xp[i], i % T, rp ? rp[i] : 0.f);
}

// Frame-online windows are a few columns wide: one workgroup per utterance does the three passes in one launch (sums in
// double precision like the kernels above, the same serial scan; the order inside a column's row sum differs).
__global__ __launch_bounds__(256) void cln_window_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                         const float* __restrict__ gain, const float* __restrict__ bias,
                                                         const float* __restrict__ pre_slope,
                                                         const float* __restrict__ post_slope, const float* __restrict__ fir,
                                                         int K, int R, int F, int T, int c0, int t_first, long tg0, int n_new,
                                                         double* __restrict__ carry, const int32_t* __restrict__ origin) {
    extern __shared__ double sc[];       // [2][T] totals, then [2][T] floats mean / rstd behind them
    __shared__ double sh[2][256];
    const int b = blockIdx.x;
    if (origin) tg0 -= origin[b];        // the row's own frame index of column 0 (wave-uniform: one read)
    float* mu = reinterpret_cast<float*>(sc + 2 * T);
    float* rs = mu + T;
    // per-column sums over the rows: WP columns at a time (WP = the window width rounded up to a power of two, at most 64),
    // 256 / WP threads share one column's rows and are folded by a tree in double precision
    int WP = 1;
    while (WP < T - c0 && WP < 64) WP <<= 1;
    const int NL = 256 / WP, col = threadIdx.x % WP, ln = threadIdx.x / WP;
    for (int tb = c0; tb < T; tb += WP) {
        const int t = tb + col;
        double s = 0.0, q = 0.0;
        if (t < T) {
            const float* xp = x + (long)b * R * T + t;
            auto take = [&](int r, float v) {
                if (pre_slope) v = v >= 0.f ? v : pre_slope[r / F] * v;
                s += v;
                q += (double)v * v;
            };
            int r = ln;
            for (; r + NL * 3 < R; r += NL * 4) {
                float xr[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) xr[u] = xp[(long)(r + NL * u) * T];
#pragma unroll
                for (int u = 0; u < 4; ++u) take(r + NL * u, xr[u]);
            }
            for (; r < R; r += NL) take(r, xp[(long)r * T]);
        }
        sh[0][threadIdx.x] = s;
        sh[1][threadIdx.x] = q;
        __syncthreads();
        for (int h = NL >> 1; h >= 1; h >>= 1) {
            if (ln < h) {
                sh[0][threadIdx.x] += sh[0][threadIdx.x + h * WP];
                sh[1][threadIdx.x] += sh[1][threadIdx.x + h * WP];
            }
            __syncthreads();
        }
        if (ln == 0 && t < T) {
            const bool live = tg0 + t >= 0;
            sc[t] = live ? sh[0][col] : 0.0;
            sc[T + t] = live ? sh[1][col] : 0.0;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double a = carry[2 * b], q = carry[2 * b + 1];
        for (int t = c0; t < T; ++t) {
            a += sc[t];
            q += sc[T + t];
            sc[t] = a;
            sc[T + t] = q;
            if (t == c0 + n_new - 1) {
                carry[2 * b] = a;
                carry[2 * b + 1] = q;
            }
        }
    }
    __syncthreads();
    for (int t = c0 + threadIdx.x; t < T; t += 256) {
        const double cnt = (double)R * (double)(tg0 + t >= 0 ? tg0 + t + 1 : 1);
        cln_mean_rstd(sc[t], sc[T + t], cnt, mu[t], rs[t]);
    }
    __syncthreads();
    const int nn = T - t_first, W = T - c0;
    float* nw = rs + T;                  // [R][W] normalised window (FIR flavour only: the launcher sizes the LDS for it)
    if (K > 0) {
        for (long i = threadIdx.x; i < (long)R * W; i += 256) {
            const int r = (int)(i / W), ti = c0 + (int)(i - (long)r * W), c = r / F;
            float v = x[((long)b * R + r) * T + ti];
            v = v >= 0.f ? v : (pre_slope ? pre_slope[c] : 1.f) * v;
            nw[i] = (tg0 + ti >= 0) ? (v - mu[ti]) * rs[ti] * gain[c] + bias[c] : 0.f;
        }
        __syncthreads();
    }
    for (long i = threadIdx.x; i < (long)R * nn; i += 256) {
        const int r = (int)(i / nn), t = t_first + (int)(i - (long)r * nn), c = r / F;
        float o;
        if (K <= 0) {
            float v = x[((long)b * R + r) * T + t];
            v = v >= 0.f ? v : (pre_slope ? pre_slope[c] : 1.f) * v;
            o = (v - mu[t]) * rs[t] * gain[c] + bias[c];
            if (post_slope) o = o >= 0.f ? o : post_slope[c] * o;
        } else {
            o = 0.f;
            const float* wp = nw + (long)r * W + (t - c0) - (K - 1);
            for (int k = 0; k < K; ++k) {
                if (tg0 + t - (K - 1) + k >= 0) o += fir[k] * wp[k];
            }
        }
        y[((long)b * R + r) * T + t] = o;
    }
}

// One or two new frames (the latency-critical push): a thread keeps its share of the C * F * W values in registers - one
// batch of loads, column sums folded by wave shuffles and one LDS step in float64 (fixed order), the stream's running sums
// continued by one thread, normalise + PReLU straight from the registers.  cln_window_kernel walks the rows twice with a
// load per loop iteration (9 us on a 64 x 161 layer; this form: the kernel floor + one round trip).
template <int W, int VPT>
__global__ __launch_bounds__(256) void cln_window_reg_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                             const float* __restrict__ gain, const float* __restrict__ bias,
                                                             const float* __restrict__ post_slope, int R, int F, int T, int c0,
                                                             long tg0, double* __restrict__ carry, const float* res,
                                                             const int32_t* __restrict__ origin) {
    __shared__ double sh[4][2 * W];
    __shared__ float s_mu[W], s_rs[W];
    __shared__ float s_par[3][256];          // gain, bias, PReLU slope per channel (C = R / F <= 256, checked by the launcher)
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = R * W;
    const float* xb = x + (long)b * R * T + c0;
    float* yb = y + (long)b * R * T + c0;
    // Everything the kernel reads from global memory is requested here, in ONE batch: the frame, the running sums and the
    // channel parameters.  (Round 5 read the sums behind the block reduction and the parameters behind the second barrier: three
    // dependent round trips in a kernel whose floor is one - 6.6 us a launch, 75 launches per one-frame push of TaylorSENet_new.)
    float v[VPT], rv[VPT];
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
        const int e = tid + 256 * u;
        const int ec = e < N ? e : 0;
        v[u] = xb[(long)(ec / W) * T + (ec % W)];
    }
    // res (optional, may be y itself: an element is read and written by one thread): the residual of a module's last layer rides
    // here instead of on an add_kernel launch behind this one (12 per one-frame push of TaylorSENet_new)
    const float* rb = res ? res + (long)b * R * T + c0 : nullptr;
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
        const int e = tid + 256 * u;
        const int ec = e < N ? e : 0;
        rv[u] = rb ? rb[(long)(ec / W) * T + (ec % W)] : 0.f;
    }
    double ca = 0.0, cq = 0.0;
    if (tid == 0) {
        ca = carry[2 * b];
        cq = carry[2 * b + 1];
        if (origin) tg0 -= origin[b];        // the row's own frame index (read in the same batch; only thread 0 counts frames)
    }
    {
        const int C = R / F;
        const float pg = tid < C ? gain[tid] : 0.f, pb = tid < C ? bias[tid] : 0.f;
        const float ps = (tid < C && post_slope) ? post_slope[tid] : 1.f;
        s_par[0][tid] = pg;
        s_par[1][tid] = pb;
        s_par[2][tid] = ps;
    }
    double s[W], q[W];
#pragma unroll
    for (int t = 0; t < W; ++t) s[t] = q[t] = 0.0;
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
        const int e = tid + 256 * u;
        if (e < N) {
            // (W divides 256: a thread's elements all belong to column tid % W)
#pragma unroll
            for (int t = 0; t < W; ++t)
                if (W == 1 || (tid % W) == t) {
                    s[t] += v[u];
                    q[t] += (double)v[u] * v[u];
                }
        }
    }
#pragma unroll
    for (int t = 0; t < W; ++t)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s[t] += __shfl_xor(s[t], o, 64);
            q[t] += __shfl_xor(q[t], o, 64);
        }
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < W; ++t) {
            sh[wave][2 * t] = s[t];
            sh[wave][2 * t + 1] = q[t];
        }
    }
    __syncthreads();
    if (tid == 0) {
        double a = ca, qq = cq;
#pragma unroll
        for (int t = 0; t < W; ++t) {
            a += (sh[0][2 * t] + sh[1][2 * t]) + (sh[2][2 * t] + sh[3][2 * t]);
            qq += (sh[0][2 * t + 1] + sh[1][2 * t + 1]) + (sh[2][2 * t + 1] + sh[3][2 * t + 1]);
            cln_mean_rstd(a, qq, (double)R * (double)(tg0 + c0 + t + 1), s_mu[t], s_rs[t]);
        }
        carry[2 * b] = a;
        carry[2 * b + 1] = qq;
    }
    __syncthreads();
    const bool act = post_slope != nullptr;
#pragma unroll
    for (int u = 0; u < VPT; ++u) {
        const int e = tid + 256 * u;
        if (e < N) {
            const int r = e / W, t = e % W, c = r / F;
            float o = (v[u] - s_mu[t]) * s_rs[t] * s_par[0][c] + s_par[1][c];
            if (act) o = o >= 0.f ? o : s_par[2][c] * o;
            yb[(long)r * T + t] = o + rv[u];
        }
    }
}


// ---- the launcher -----------------------------------------------------------------------------------------------
bool cln_stream_takes_res(int C, int F) {
    const StreamCtx* cx = stream_ctx();
    return cx && cln_chunk_takes_res(cx->B, C, F, cx->H, cx->n, cln_tuning_env());
}

namespace {
struct ClnArgs {
    const float *x, *gain, *bias, *pre_slope, *post_slope, *fir, *parts, *res;
    float* y;
};
// launch_cln / launch_cln_parts: the choice of cln_select for the call, the pointer work, then the choice's launches in order
void cln_run(ClnSelIn in, const ClnArgs& a, hipStream_t s) {
    StreamCtx* cx = stream_ctx();
    in.ragged = ragged_ctx() != nullptr;
    in.pre = a.pre_slope != nullptr; in.post = a.post_slope != nullptr; in.res = a.res != nullptr;
    if (cx) {
        in.stream = true;
        in.H = cx->H; in.n = cx->n; in.sB = cx->B;
    }
    const ClnChoice ch = cln_select(in, cln_tuning_env());
    SE_CHECK(ch.form != CLN_FORM_REFUSED, ch.refusal);
    SE_CHECK(in.K <= 0 || a.x != a.y, "cLN + FIR cannot run in place");
    const int B = in.B, F = in.F, T = in.T, K = in.K, R = in.C * F;
    // per-(b, t) statistics live in a small engine-lifetime buffer (grown on first use, never on the steady-state path)
    double* sum = (double*)device_scratch(1, ch.scratch, s);
    double* sq = sum + (size_t)B * T;
    float* mean = (float*)(sq + (size_t)B * T);
    float* rstd = mean + (size_t)B * T;
    // frame-online chunk: the history columns the FIR reads are brought in here; the running totals of the stream are its state
    double* carry = nullptr;
    const int32_t* origin = nullptr;
    long tg0 = 0;          // stream index of column 0
    int t_first = 0, n_new = 0;
    if (cx) {
        if (ch.back > 0) stream_exchange(const_cast<float*>(a.x), (long)R * T, (long)F * T, T, B, in.C, F, ch.back, s);
        cx->memo_src = nullptr;
        carry = static_cast<double*>(cx->slot(SlotRow{2 * sizeof(double)}, s));
        origin = cx->origin;
        tg0 = cx->t0 - cx->H;
        t_first = cx->H;
        n_new = cx->n;
    }
    for (int i = 0; i < ch.n_launch; ++i) {
        const ClnLaunch& l = ch.launch[i];
        const dim3 grid(l.gx, l.gy, l.gz), block(l.block);
        norm_log_launch(l.name, (long)l.gx * l.gy * l.gz, l.block, l.lds, 0, ch.c0, l.kernel == CLN_K_STATS ? ch.WP : 0, ch.W, ch.VPT);
        if (l.res) norm_log_res(a.res);
        switch (l.kernel) {
            case CLN_K_STATS:
                hipLaunchKernelGGL(cln_stats_kernel, grid, block, l.lds, s, a.x, a.pre_slope, sum, sq, R, F, T, ch.c0, ch.WP);
                break;
            case CLN_K_SCAN:
                hipLaunchKernelGGL(cln_scan_kernel, grid, block, l.lds, s, sum, sq, mean, rstd, R, T, ch.c0, tg0, n_new, carry, origin);
                break;
            case CLN_K_SCAN_PARTS:
                hipLaunchKernelGGL(cln_scan_parts_kernel, grid, block, l.lds, s, a.parts, F, mean, rstd, R, T);
                break;
            case CLN_K_APPLY:
                hipLaunchKernelGGL(cln_apply_kernel, grid, block, l.lds, s, a.x, a.y, mean, rstd, a.gain, a.bias, a.pre_slope, a.post_slope,
                                   a.fir, K, R, F, T, t_first, tg0, origin);
                break;
            case CLN_K_APPLY_PLANE:
                hipLaunchKernelGGL(cln_apply_plane_kernel, grid, block, l.lds, s, a.x, a.y, mean, rstd, a.gain, a.bias, a.post_slope, a.res,
                                   in.C, F, T);
                break;
            case CLN_K_WINDOW:
                hipLaunchKernelGGL(cln_window_kernel, grid, block, l.lds, s, a.x, a.y, a.gain, a.bias, a.pre_slope, a.post_slope, a.fir, K, R,
                                   F, T, ch.c0, t_first, tg0, n_new, carry, origin);
                break;
            case CLN_K_WINDOW_REG:
                // (every frame of the chunk is live: tg0 + c0 = the stream index of the first new frame >= 0)
                if (ch.W == 1)
                    hipLaunchKernelGGL((cln_window_reg_kernel<1, 41>), grid, block, l.lds, s, a.x, a.y, a.gain, a.bias, a.post_slope, R, F,
                                       T, ch.c0, tg0, carry, a.res, origin);
                else
                    hipLaunchKernelGGL((cln_window_reg_kernel<2, 82>), grid, block, l.lds, s, a.x, a.y, a.gain, a.bias, a.post_slope, R, F,
                                       T, ch.c0, tg0, carry, a.res, origin);
                break;
        }
    }
    SE_HIP(hipGetLastError());
}
}  // namespace

void launch_cln(const float* x, float* y, const float* gain, const float* bias, const float* pre_slope,
                const float* post_slope, const float* fir, int K, int B, int C, int F, int T, hipStream_t s, const float* res) {
    ClnSelIn in;
    in.B = B; in.C = C; in.F = F; in.T = T; in.K = K;
    cln_run(in, ClnArgs{x, gain, bias, pre_slope, post_slope, fir, nullptr, res, y}, s);
}

// offline 2-D cLN + PReLU (+ residual) behind a conv that emitted its per-frame sums (GCParams::cstats): scan + apply, no statistics pass
void launch_cln_parts(const float* x, float* y, const float* gain, const float* bias, const float* post_slope, const float* parts,
                      int B, int C, int F, int T, hipStream_t s, const float* res) {
    ClnSelIn in;
    in.B = B; in.C = C; in.F = F; in.T = T;
    in.parts = true;
    cln_run(in, ClnArgs{x, gain, bias, nullptr, post_slope, nullptr, parts, res, y}, s);
}

}  // namespace se

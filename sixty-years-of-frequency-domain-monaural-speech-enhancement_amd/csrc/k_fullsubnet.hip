// FullSubNet's private kernels: the four norms of norm_wrapper (utterance mean, cumulative mean, utterance mean / std, cumulative
// mean / std), the sub-band unfold and the mask back end, offline and frame-online.  Reference lines as in model_fullsubnet.hip:
// FullSubNet/fullsubnet_net_sa/model.py:68-118, base_model.py:13-42 (unfold), :197-209 (offline_laplace_norm), :212-240
// (cumulative_laplace_norm), :242-255 (offline_gaussian_norm), :258-294 (cumulative_layer_norm),
// fullsubnet_sa_decode_vb.py:56-66 (the complex mask and the decompress, applied in the script).
//
// Layouts (time-major, sequences contiguous): full band [T+la][257][B]; sub bands [T+la][W][257*B], sequence s = n*B + b is
// sub-band n of utterance b.  The look-ahead `la` (Model(look_ahead=), 0..6) and the sub-band width W = (2 sbn + 1) + (2 fbn + 1)
// (sb_num_neighbors, fb_num_neighbors, 0..15 each) are kernel arguments; the two kernels that keep a sub band's W values in
// registers have an instance for the decode script's W = 32 (fsn::SBW) and a run-time form that reads the rows twice - the same
// float32 operations in the same order either way.
#include "k_fullsubnet.h"

namespace se {

using namespace fsn;

namespace {

// sum over (f, t) of mag[b][f][t]  ->  mu[b] = sum / (F * (T + la))   (the look-ahead pad frames are zeros)
// ragged batch (tlen != null): frames >= tlen[b] of mag are zeros (the STFT wrote them), so only the denominator changes
__global__ __launch_bounds__(256) void fsn_mean_kernel(const float* __restrict__ mag, int n, float denom,
                                                       float* __restrict__ mu, const int* __restrict__ tlen, int la) {
    const int b = blockIdx.x;
    if (tlen) denom = (float)NBIN * (tlen[b] + la);
    const float* x = mag + (long)b * n;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += x[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    __shared__ double part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) mu[b] = (float)((part[0] + part[1] + part[2] + part[3]) / denom);
}

// y[i] = x[i] / (mu[i % B] + 1e-5)   for time-major tensors whose innermost index is the utterance
__global__ __launch_bounds__(256) void fsn_scale_kernel(const float* __restrict__ x, float* __restrict__ y, long n,
                                                        int B, const float* __restrict__ mu) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = x[i] / (mu[i % B] + 1e-5f);
}

// sub-band input before normalisation: sb[t][k][n*B + b], W = (2 sbn + 1) + (2 fbn + 1) rows per sub band n (model.py:88-96):
//   k <  2 sbn + 1: noisy magnitude of bin reflect(n - sbn + k)                   unfold(noisy_mag, sbn)
//   k >= 2 sbn + 1: full-band output of bin reflect(n - fbn + k - (2 sbn + 1))    unfold(fb_output, fbn)
// base_model.py:29-42 pads the frequency axis by num_neighbor bins with mode="reflect" (the edge bin is not repeated: bin -j is bin j,
// bin 256 + j is bin 256 - j) and cuts windows of 2 num_neighbor + 1 bins; num_neighbor = 0 returns the input as it is (:25-27),
// which is the same rule with nothing to reflect.  One reflection is enough: the launcher keeps sbn, fbn <= 15 < NBIN.
// A pure gather; consecutive threads write consecutive sequences s.
__global__ __launch_bounds__(256) void fsn_build_sb_kernel(const float* __restrict__ magT, const float* __restrict__ fbo,
                                                           float* __restrict__ sb, int B, int sbn, int fbn) {
    const int S = NBIN * B;
    const int s = blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y, t = blockIdx.z;
    if (s >= S) return;
    const int n = s / B, b = s - n * B;
    const int nw = 2 * sbn + 1, W = nw + 2 * fbn + 1;
    const bool noisy = k < nw;
    int f = noisy ? n - sbn + k : n - fbn + (k - nw);
    if (f < 0) f = -f;
    if (f >= NBIN) f = 2 * (NBIN - 1) - f;
    const float* src = noisy ? magT : fbo;
    sb[((long)t * W + k) * S + s] = src[((long)t * NBIN + f) * B + b];
}

// column sums of a [rows][B] matrix (utterance = innermost index) -> mu[b] = sum / rows; two deterministic stages
// (per-block partials in a fixed order, then a fixed-order fp64 sum) - no float atomics, so repeated decodes are
// bit-identical
// ragged batch: rows are (t, k, n) t-major, frame_rows = W * 257 of them per frame; utterance b only counts its own tlen[b] + la frames
__global__ __launch_bounds__(256) void fsn_colsum_kernel(const float* __restrict__ x, long rows, int B,
                                                         float* __restrict__ part, const int* __restrict__ tlen, long frame_rows,
                                                         int la) {
    __shared__ float sh[256];
    // thread handles column (tid % B) of rows tid / B + k * (256 / B)
    const int per = 256 / B;
    const int b = threadIdx.x % B, r0 = threadIdx.x / B;
    float s = 0.f;
    if (per > 0 && r0 < per) {
        const long rmax = tlen ? (long)(tlen[b] + la) * frame_rows : rows;
        for (long r = (long)blockIdx.x * per + r0; r < rmax; r += (long)gridDim.x * per) s += x[r * B + b];
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    if (per > 0 && r0 == 0) {
        float t = 0.f;
        for (int k = 0; k < per; ++k) t += sh[k * B + b];
        part[(long)blockIdx.x * B + b] = t;
    }
}
__global__ void fsn_finish_mean_kernel(const float* __restrict__ part, float* __restrict__ mu, float denom, int B,
                                       const int* __restrict__ tlen, long frame_rows, int la) {
    const int b = threadIdx.x;
    if (b >= B) return;
    if (tlen) denom = (float)((long)(tlen[b] + la) * frame_rows);
    double s = 0.0;
    for (int k = 0; k < FSN_SUM_BLOCKS; ++k) s += part[(long)k * B + b];
    mu[b] = (float)(s / denom);
}

// out[b][c][n][t] = mask[(n*B + b)][c][t + la]                       (forward hook), or
// est = mask (x) spec, decompressed (fullsubnet_sa_decode_vb.py:56-66)  (decode path)
__global__ __launch_bounds__(256) void fsn_mask_kernel(const float* __restrict__ maskBT, const float* __restrict__ spec,
                                                       float* __restrict__ out, int B, int T, float p_out, int la) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int n = blockIdx.y, b = blockIdx.z;
    if (t >= T) return;
    const int Tp = T + la;
    const float* m = maskBT + ((long)(n * B + b) * 2) * Tp + t + la;
    const float mr = m[0], mi = m[Tp];
    const long o = (((long)b * 2) * NBIN + n) * T + t;
    const long plane = (long)NBIN * T;
    if (!spec) {
        out[o] = mr;
        out[o + plane] = mi;
        return;
    }
    const float xr = spec[o], xi = spec[o + plane];
    float er = mr * xr - mi * xi, ei = mr * xi + mi * xr;
    if (p_out != 1.f) {
        const float mg = sqrtf(er * er + ei * ei);
        const float sc = mg > 0.f ? ((p_out == 2.f) ? mg : powf(mg, p_out - 1.f)) : 0.f;
        er *= sc;
        ei *= sc;
    }
    out[o] = er;
    out[o + plane] = ei;
}

// ---- cumulative_laplace_norm (base_model.py:212-240): x / (mean over (features, frames <= t) + EPSILON), float32 sums in the
// reference's order - the features of a frame first, then a running sum over the frames.  `csum` (optional) carries the running
// sum across the chunks of a frame-online stream; step 0 of the call is frame t_first of the utterance.
// full band: x / y [n][257][B] time-major, one workgroup per utterance
__global__ __launch_bounds__(256) void fsn_cum_fb_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int B,
                                                         float* __restrict__ csum, int t_first,
                                                         const int32_t* __restrict__ origin) {
    __shared__ float part[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (origin) t_first -= origin[b];      // the row's own frame index (one workgroup per row: uniform, read once)
    float run = (csum && t_first > 0) ? csum[b] : 0.f;
    for (int t = 0; t < n; ++t) {
        const float* xr = x + (long)t * NBIN * B + b;
        const float v0 = xr[(long)tid * B], v1 = tid + 256 < NBIN ? xr[(long)(tid + 256) * B] : 0.f;
        float s = v0 + v1;
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        __syncthreads();
        if ((tid & 63) == 0) part[tid >> 6] = s;
        __syncthreads();
        run += (part[0] + part[1]) + (part[2] + part[3]);
        const float d = run / ((float)NBIN * (float)(t_first + t + 1)) + FSN_EPS;
        float* yr = y + (long)t * NBIN * B + b;
        yr[(long)tid * B] = v0 / d;
        if (tid + 256 < NBIN) yr[(long)(tid + 256) * B] = v1 / d;
    }
    if (csum && tid == 0) csum[b] = run;
}
// sub bands: sb [n][W][S] in place, one thread per sequence s (sub-band of an utterance)
// origin (optional, [B]): sequence s = n * B + b belongs to row s % B, whose own frame index is t_first - origin[s % B]
// WC = SBW: the decode script's width, the W values of a frame held in registers;  WC = 0: any width W, the rows read a second time
// for the divide (the same values: nothing else writes them) - the sum runs over k = 0..W-1 in order in both forms
template <int WC>
__global__ __launch_bounds__(256) void fsn_cum_sb_kernel(float* __restrict__ sb, int n, int S, float* __restrict__ csum, int t_first,
                                                         const int32_t* __restrict__ origin, int B, int W) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    if (origin) t_first -= origin[s % B];
    float run = (csum && t_first > 0) ? csum[s] : 0.f;
    if constexpr (WC > 0) {
        for (int t = 0; t < n; ++t) {
            float* xr = sb + (long)t * WC * S + s;
            float v[WC], sum = 0.f;
#pragma unroll
            for (int k = 0; k < WC; ++k) {
                v[k] = xr[(long)k * S];
                sum += v[k];
            }
            run += sum;
            const float d = run / ((float)WC * (float)(t_first + t + 1)) + FSN_EPS;
#pragma unroll
            for (int k = 0; k < WC; ++k) xr[(long)k * S] = v[k] / d;
        }
    } else {
        for (int t = 0; t < n; ++t) {
            float* xr = sb + (long)t * W * S + s;
            float sum = 0.f;
            for (int k = 0; k < W; ++k) sum += xr[(long)k * S];
            run += sum;
            const float d = run / ((float)W * (float)(t_first + t + 1)) + FSN_EPS;
            for (int k = 0; k < W; ++k) xr[(long)k * S] = xr[(long)k * S] / d;
        }
    }
    if (csum) csum[s] = run;
}
// ---- offline_gaussian_norm (base_model.py:242-255): (x - mean) / (std + 1e-5), mean and the unbiased std (torch.std: N - 1) over the
// whole utterance.  Both moments in ONE pass over a [rows][B] matrix (utterance = innermost index: the full band is [Tp * 257][B], the
// sub bands [Tp * W * 257][B]), accumulated in float64 (the square of a float is exact there, so S2 - N mean^2 cancels nothing
// that float32 holds), in the two deterministic stages of fsn_colsum / fsn_finish_mean: per-block partials in a fixed order, then
// a fixed-order sum - no atomics, repeated decodes are bit-identical.  part [gridDim.x][2][B] float64.
// ragged batch: rows are t-major, frame_rows of them per frame; utterance b only counts its own tlen[b] + la frames
__global__ __launch_bounds__(256) void fsn_moments_kernel(const float* __restrict__ x, long rows, int B, double* __restrict__ part,
                                                          const int* __restrict__ tlen, long frame_rows, int la) {
    __shared__ double sh[2][256];
    // thread handles column (tid % B) of rows tid / B + k * (256 / B), as fsn_colsum_kernel
    const int per = 256 / B;
    const int b = threadIdx.x % B, r0 = threadIdx.x / B;
    double s1 = 0.0, s2 = 0.0;
    if (per > 0 && r0 < per) {
        long rmax = rows;
        if (tlen && (long)(tlen[b] + la) * frame_rows < rows) rmax = (long)(tlen[b] + la) * frame_rows;
#pragma unroll 4
        for (long r = (long)blockIdx.x * per + r0; r < rmax; r += (long)gridDim.x * per) {
            const double v = x[r * B + b];
            s1 += v;
            s2 += v * v;
        }
    }
    sh[0][threadIdx.x] = s1;
    sh[1][threadIdx.x] = s2;
    __syncthreads();
    if (per > 0 && r0 == 0) {
        double t1 = 0.0, t2 = 0.0;
        for (int k = 0; k < per; ++k) {
            t1 += sh[0][k * B + b];
            t2 += sh[1][k * B + b];
        }
        part[((long)blockIdx.x * 2) * B + b] = t1;
        part[((long)blockIdx.x * 2 + 1) * B + b] = t2;
    }
}
// part [FSN_SUM_BLOCKS][2][B] -> stat[b] = mean, stat[B + b] = std + 1e-5 (float32, the divisor of :253);  N = rows, or the row's own
// (tlen[b] + la) * frame_rows;  var = (S2 - N mean^2) / (N - 1) in float64
__global__ void fsn_finish_gauss_kernel(const double* __restrict__ part, float* __restrict__ stat, long rows, int B,
                                        const int* __restrict__ tlen, long frame_rows, int la) {
    const int b = threadIdx.x;
    if (b >= B) return;
    long cnt = rows;
    if (tlen && (long)(tlen[b] + la) * frame_rows < rows) cnt = (long)(tlen[b] + la) * frame_rows;
    const double N = (double)cnt;
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < FSN_SUM_BLOCKS; ++k) {
        s1 += part[((long)k * 2) * B + b];
        s2 += part[((long)k * 2 + 1) * B + b];
    }
    const double mean = s1 / N;
    const double var = fmax(s2 - N * mean * mean, 0.0) / fmax(N - 1.0, 1.0);
    stat[b] = (float)mean;
    stat[B + b] = (float)sqrt(var) + 1e-5f;
}
// y[i] = (x[i] - mean[i % B]) / (std[i % B] + 1e-5)   for time-major tensors whose innermost index is the utterance
__global__ __launch_bounds__(256) void fsn_gauss_apply_kernel(const float* __restrict__ x, float* __restrict__ y, long n, int B,
                                                              const float* __restrict__ stat) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = (int)(i % B);
    y[i] = (x[i] - stat[b]) / stat[B + b];
}

// ---- cumulative_layer_norm (base_model.py:258-294): the two-sum forms of the cumulative kernels above.  Running float32 sums of x and
// x^2 in the reference's order (the features of a frame first, then over the frames), and the reference's expression as written
// (:285-287, :292) - no fused multiply-add, which would round differently than the tensor expression does:
//   mean = S1 / n;  var = (S2 - 2 mean S1) / n + mean^2;  std = sqrt(var + EPSILON);  y = (x - mean) / std
// A stream that starts with frames of zeros has S1 = S2 = 0: mean = 0, std = sqrt(EPSILON), y = exact zeros.
__device__ __forceinline__ void fsn_cln_stats(float s1, float s2, float cnt, float& mean, float& sd) {
#pragma clang fp contract(off)
    mean = s1 / cnt;
    const float twice = 2.f * mean;
    const float cross = twice * s1;
    const float mm = mean * mean;
    const float var = (s2 - cross) / cnt + mm;
    sd = sqrtf(var + FSN_EPS);
}
// full band: x / y [n][257][B] time-major, one workgroup per utterance; csum / csum2 [B]: the running sums of x and x^2
__global__ __launch_bounds__(256) void fsn_cln_fb_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int B,
                                                         float* __restrict__ csum, float* __restrict__ csum2, int t_first,
                                                         const int32_t* __restrict__ origin) {
    __shared__ float part[2][4];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (origin) t_first -= origin[b];      // the row's own frame index (one workgroup per row: uniform, read once)
    const bool carry = csum && t_first > 0;
    float run = carry ? csum[b] : 0.f, run2 = carry ? csum2[b] : 0.f;
    for (int t = 0; t < n; ++t) {
        const float* xr = x + (long)t * NBIN * B + b;
        const float v0 = xr[(long)tid * B], v1 = tid + 256 < NBIN ? xr[(long)(tid + 256) * B] : 0.f;
        float s, q;
        {
#pragma clang fp contract(off)
            const float q0 = v0 * v0, q1 = v1 * v1;
            s = v0 + v1;
            q = q0 + q1;
        }
        for (int o = 32; o > 0; o >>= 1) {
            s += __shfl_down(s, o, 64);
            q += __shfl_down(q, o, 64);
        }
        __syncthreads();
        if ((tid & 63) == 0) {
            part[0][tid >> 6] = s;
            part[1][tid >> 6] = q;
        }
        __syncthreads();
        run += (part[0][0] + part[0][1]) + (part[0][2] + part[0][3]);
        run2 += (part[1][0] + part[1][1]) + (part[1][2] + part[1][3]);
        float mean, sd;
        fsn_cln_stats(run, run2, (float)NBIN * (float)(t_first + t + 1), mean, sd);
        float* yr = y + (long)t * NBIN * B + b;
        yr[(long)tid * B] = (v0 - mean) / sd;
        if (tid + 256 < NBIN) yr[(long)(tid + 256) * B] = (v1 - mean) / sd;
    }
    if (csum && tid == 0) {
        csum[b] = run;
        csum2[b] = run2;
    }
}
// sub bands: sb [n][W][S] in place, one thread per sequence s (consecutive threads read consecutive s: coalesced); csum / csum2 [S]
// origin (optional, [B]): sequence s = n * B + b belongs to row s % B, whose own frame index is t_first - origin[s % B]
// WC as fsn_cum_sb_kernel: SBW keeps a frame's values in registers, 0 takes any W and reads the rows twice
template <int WC>
__global__ __launch_bounds__(256) void fsn_cln_sb_kernel(float* __restrict__ sb, int n, int S, float* __restrict__ csum,
                                                         float* __restrict__ csum2, int t_first, const int32_t* __restrict__ origin,
                                                         int B, int W) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    if (origin) t_first -= origin[s % B];
    const bool carry = csum && t_first > 0;
    float run = carry ? csum[s] : 0.f, run2 = carry ? csum2[s] : 0.f;
    if constexpr (WC > 0) {
        for (int t = 0; t < n; ++t) {
            float* xr = sb + (long)t * WC * S + s;
            float v[WC], sum = 0.f, sq = 0.f;
#pragma unroll
            for (int k = 0; k < WC; ++k) {
#pragma clang fp contract(off)
                v[k] = xr[(long)k * S];
                const float q = v[k] * v[k];
                sum += v[k];
                sq += q;
            }
            run += sum;
            run2 += sq;
            float mean, sd;
            fsn_cln_stats(run, run2, (float)WC * (float)(t_first + t + 1), mean, sd);
#pragma unroll
            for (int k = 0; k < WC; ++k) xr[(long)k * S] = (v[k] - mean) / sd;
        }
    } else {
        for (int t = 0; t < n; ++t) {
            float* xr = sb + (long)t * W * S + s;
            float sum = 0.f, sq = 0.f;
            for (int k = 0; k < W; ++k) {
#pragma clang fp contract(off)
                const float v = xr[(long)k * S];
                const float q = v * v;
                sum += v;
                sq += q;
            }
            run += sum;
            run2 += sq;
            float mean, sd;
            fsn_cln_stats(run, run2, (float)W * (float)(t_first + t + 1), mean, sd);
            for (int k = 0; k < W; ++k) xr[(long)k * S] = (xr[(long)k * S] - mean) / sd;
        }
    }
    if (csum) {
        csum[s] = run;
        csum2[s] = run2;
    }
}
// frame-online: mask of network step tau (maskT [ns][2][S], s = n B + b) applied to the spectrum of frame tau - la, which sits in
// column col0 + tau of the chunk window ([B][2][257][Tw]); frames before the start of the stream (gt0 + tau < la) do not exist
__global__ __launch_bounds__(256) void fsn_stream_apply_kernel(const float* __restrict__ maskT, const float* __restrict__ spec,
                                                               float* __restrict__ est, int B, int Tw, int ns, int col0, int gt0,
                                                               float p_out, const int32_t* __restrict__ origin, int la) {
    const int i = blockIdx.x * 256 + threadIdx.x, tau = blockIdx.y;
    const int S = NBIN * B;
    if (i >= S) return;
    if (origin) gt0 -= origin[i % B];      // the row's own frame index: a row younger than the look-ahead skips its steps alone
    if (gt0 + tau < la) return;
    const int n = i / B, b = i - n * B, col = col0 + tau;
    const float mr = maskT[((long)tau * 2) * S + i], mi = maskT[((long)tau * 2 + 1) * S + i];
    const long o = (((long)b * 2) * NBIN + n) * Tw + col, plane = (long)NBIN * Tw;
    const float xr = spec[o], xi = spec[o + plane];
    float er = mr * xr - mi * xi, ei = mr * xi + mi * xr;
    if (p_out != 1.f) {
        const float mg = sqrtf(er * er + ei * ei);
        const float sc = mg > 0.f ? ((p_out == 2.f) ? mg : powf(mg, p_out - 1.f)) : 0.f;
        er *= sc;
        ei *= sc;
    }
    est[o] = er;
    est[o + plane] = ei;
    (void)ns;
}

}  // namespace

void launch_fsn_mean(const float* mag, int B, int n, float denom, float* mu, const int* tlen, hipStream_t st, int la) {
    hipLaunchKernelGGL(fsn_mean_kernel, dim3(B), dim3(256), 0, st, mag, n, denom, mu, tlen, la);
    SE_HIP(hipGetLastError());
}
void launch_fsn_scale(const float* x, float* y, long n, int B, const float* mu, hipStream_t st) {
    hipLaunchKernelGGL(fsn_scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, y, n, B, mu);
    SE_HIP(hipGetLastError());
}
void launch_fsn_build_sb(const float* magT, const float* fbo, float* sb, int B, int steps, hipStream_t st, int sbn, int fbn) {
    SE_CHECK(sbn >= 0 && sbn <= NEIGHBORS_MAX && fbn >= 0 && fbn <= NEIGHBORS_MAX, "launch_fsn_build_sb: neighbour counts are 0..15");
    const int S = NBIN * B;
    hipLaunchKernelGGL(fsn_build_sb_kernel, dim3((S + 255) / 256, sb_width(sbn, fbn), steps), dim3(256), 0, st, magT, fbo, sb, B, sbn, fbn);
    SE_HIP(hipGetLastError());
}
void launch_fsn_colsum(const float* x, long rows, int B, float* part, const int* tlen, hipStream_t st, long frame_rows, int la) {
    SE_CHECK(B >= 1 && B <= 256, "FullSubNet batch per call is limited to 256 utterances");
    hipLaunchKernelGGL(fsn_colsum_kernel, dim3(FSN_SUM_BLOCKS), dim3(256), 0, st, x, rows, B, part, tlen, frame_rows, la);
    SE_HIP(hipGetLastError());
}
void launch_fsn_finish_mean(const float* part, float* mu, float denom, int B, const int* tlen, hipStream_t st, long frame_rows, int la) {
    SE_CHECK(B >= 1 && B <= 256, "FullSubNet batch per call is limited to 256 utterances");
    hipLaunchKernelGGL(fsn_finish_mean_kernel, dim3(1), dim3(256), 0, st, part, mu, denom, B, tlen, frame_rows, la);
    SE_HIP(hipGetLastError());
}
void launch_fsn_mask(const float* maskBT, const float* spec, float* out, int B, int T, float p_out, hipStream_t st, int la) {
    hipLaunchKernelGGL(fsn_mask_kernel, dim3((T + 255) / 256, NBIN, B), dim3(256), 0, st, maskBT, spec, out, B, T, p_out, la);
    SE_HIP(hipGetLastError());
}
void launch_fsn_cum_fb(const float* x, float* y, int n, int B, float* csum, int t_first, hipStream_t st, const int32_t* origin) {
    hipLaunchKernelGGL(fsn_cum_fb_kernel, dim3(B), dim3(256), 0, st, x, y, n, B, csum, t_first, origin);
    SE_HIP(hipGetLastError());
}
void launch_fsn_cum_sb(float* sb, int n, int S, float* csum, int t_first, hipStream_t st, const int32_t* origin, int W) {
    SE_CHECK(!origin || (S >= NBIN && S % NBIN == 0), "launch_fsn_cum_sb: per-row origins need S = 257 * B sequences");
    SE_CHECK(W >= 1 && W <= SBW_MAX, "launch_fsn_cum_sb: the sub-band width is 1..62");
    if (W == SBW)
        hipLaunchKernelGGL(fsn_cum_sb_kernel<SBW>, dim3((S + 255) / 256), dim3(256), 0, st, sb, n, S, csum, t_first, origin, S / NBIN, W);
    else
        hipLaunchKernelGGL(fsn_cum_sb_kernel<0>, dim3((S + 255) / 256), dim3(256), 0, st, sb, n, S, csum, t_first, origin, S / NBIN, W);
    SE_HIP(hipGetLastError());
}
void launch_fsn_moments(const float* x, long rows, int B, double* part, const int* tlen, long frame_rows, hipStream_t st, int la) {
    SE_CHECK(B >= 1 && B <= 256, "FullSubNet batch per call is limited to 256 utterances");
    SE_CHECK(rows >= 1 && frame_rows >= 1 && rows % frame_rows == 0, "launch_fsn_moments: rows is a whole number of frames");
    hipLaunchKernelGGL(fsn_moments_kernel, dim3(FSN_SUM_BLOCKS), dim3(256), 0, st, x, rows, B, part, tlen, frame_rows, la);
    SE_HIP(hipGetLastError());
}
void launch_fsn_finish_gauss(const double* part, float* stat, long rows, int B, const int* tlen, long frame_rows, hipStream_t st, int la) {
    SE_CHECK(B >= 1 && B <= 256, "FullSubNet batch per call is limited to 256 utterances");
    hipLaunchKernelGGL(fsn_finish_gauss_kernel, dim3(1), dim3(256), 0, st, part, stat, rows, B, tlen, frame_rows, la);
    SE_HIP(hipGetLastError());
}
void launch_fsn_gauss_apply(const float* x, float* y, long n, int B, const float* stat, hipStream_t st) {
    hipLaunchKernelGGL(fsn_gauss_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, y, n, B, stat);
    SE_HIP(hipGetLastError());
}
void launch_fsn_cln_fb(const float* x, float* y, int n, int B, float* csum, float* csum2, int t_first, hipStream_t st,
                       const int32_t* origin) {
    SE_CHECK(!csum == !csum2, "launch_fsn_cln_fb: the two running sums come together");
    hipLaunchKernelGGL(fsn_cln_fb_kernel, dim3(B), dim3(256), 0, st, x, y, n, B, csum, csum2, t_first, origin);
    SE_HIP(hipGetLastError());
}
void launch_fsn_cln_sb(float* sb, int n, int S, float* csum, float* csum2, int t_first, hipStream_t st, const int32_t* origin, int W) {
    SE_CHECK(!csum == !csum2, "launch_fsn_cln_sb: the two running sums come together");
    SE_CHECK(!origin || (S >= NBIN && S % NBIN == 0), "launch_fsn_cln_sb: per-row origins need S = 257 * B sequences");
    SE_CHECK(W >= 1 && W <= SBW_MAX, "launch_fsn_cln_sb: the sub-band width is 1..62");
    if (W == SBW)
        hipLaunchKernelGGL(fsn_cln_sb_kernel<SBW>, dim3((S + 255) / 256), dim3(256), 0, st, sb, n, S, csum, csum2, t_first, origin, S / NBIN, W);
    else
        hipLaunchKernelGGL(fsn_cln_sb_kernel<0>, dim3((S + 255) / 256), dim3(256), 0, st, sb, n, S, csum, csum2, t_first, origin, S / NBIN, W);
    SE_HIP(hipGetLastError());
}
void launch_fsn_stream_apply(const float* maskT, const float* spec, float* est, int B, int Tw, int ns, int col0, int gt0,
                             float p_out, hipStream_t st, const int32_t* origin, int la) {
    const int S = NBIN * B;
    hipLaunchKernelGGL(fsn_stream_apply_kernel, dim3((S + 255) / 256, ns), dim3(256), 0, st, maskT, spec, est, B, Tw, ns, col0,
                       gt0, p_out, origin, la);
    SE_HIP(hipGetLastError());
}

}  // namespace se

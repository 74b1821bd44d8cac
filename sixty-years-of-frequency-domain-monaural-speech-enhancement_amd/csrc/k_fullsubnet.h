// Launchers of FullSubNet's private kernels (k_fullsubnet.hip): the utterance-mean and cumulative Laplace norms, the utterance
// Gaussian norm and the cumulative LayerNorm, the sub-band unfold, the mask back end and its frame-online form.
// model_fullsubnet.hip calls them; csrc/tests/model_probe.hip and csrc/tests/fsn_norm_probe.hip call them one at a time.
// Every launcher takes what its kernel takes (the per-row frame counts `tlen` of a ragged batch, the running sums
// `csum` of a stream and the stream's first frame `t_first` included) plus the sizes the grid is cut from.
#pragma once
#include "kernels.h"

namespace se {

namespace fsn {      // (a namespace of their own: other models have an NBIN too)
constexpr int NBIN = 257, LA = 2, SBN = 15, SBW = 2 * SBN + 2;   // 31 noisy + 1 full-band
constexpr int FSN_SUM_BLOCKS = 1024;                      // workgroups of the column sum = rows of its partials
constexpr float FSN_EPS = 1.1920928955078125e-07f;        // np.finfo(np.float32).eps (constant.py:8)
}  // namespace fsn

// mag [B][n] -> mu[b] = sum / denom;  tlen != null: denom = 257 * (tlen[b] + LA)
void launch_fsn_mean(const float* mag, int B, int n, float denom, float* mu, const int* tlen, hipStream_t st);
// y[i] = x[i] / (mu[i % B] + 1e-5), i < n
void launch_fsn_scale(const float* x, float* y, long n, int B, const float* mu, hipStream_t st);
// magT, fbo [steps][257][B] -> sb [steps][32][257 * B]
void launch_fsn_build_sb(const float* magT, const float* fbo, float* sb, int B, int steps, hipStream_t st);
// x [rows][B] -> part [FSN_SUM_BLOCKS][B];  tlen != null: column b stops at row (tlen[b] + LA) * 32 * 257.  B <= 256
void launch_fsn_colsum(const float* x, long rows, int B, float* part, const int* tlen, hipStream_t st);
// part [FSN_SUM_BLOCKS][B] -> mu[b] = sum / denom;  tlen != null: denom = (tlen[b] + LA) * 32 * 257.  B <= 256
void launch_fsn_finish_mean(const float* part, float* mu, float denom, int B, const int* tlen, hipStream_t st);
// maskBT [257 * B][2][T + LA] (sequence s = n * B + b) -> out [B][2][257][T]: the mask itself (spec == null, the forward hook) or
// the decompressed product with spec [B][2][257][T]
void launch_fsn_mask(const float* maskBT, const float* spec, float* out, int B, int T, float p_out, hipStream_t st);
// x -> y [n][257][B]; csum [B] (may be null), read when t_first > 0, written when not null
// origin (optional, [B] int32 on the device: SE_CFG_STREAM_ROW_ORIGINS): row b counts from t_first - origin[b]
void launch_fsn_cum_fb(const float* x, float* y, int n, int B, float* csum, int t_first, hipStream_t st, const int32_t* origin = nullptr);
// sb [n][32][S] in place; csum [S] as above
void launch_fsn_cum_sb(float* sb, int n, int S, float* csum, int t_first, hipStream_t st, const int32_t* origin = nullptr);
// offline_gaussian_norm: x [rows][B] (rows = frames * frame_rows, t-major) -> part [FSN_SUM_BLOCKS][2][B] float64, the partial sums of
// x and x^2;  tlen != null: column b stops at row (tlen[b] + LA) * frame_rows.  B <= 256
void launch_fsn_moments(const float* x, long rows, int B, double* part, const int* tlen, long frame_rows, hipStream_t st);
// part -> stat [2][B]: the mean, and the unbiased std + 1e-5 (N = rows, or the row's own (tlen[b] + LA) * frame_rows).  B <= 256
void launch_fsn_finish_gauss(const double* part, float* stat, long rows, int B, const int* tlen, long frame_rows, hipStream_t st);
// y[i] = (x[i] - stat[i % B]) / stat[B + i % B], i < n  (y may be x)
void launch_fsn_gauss_apply(const float* x, float* y, long n, int B, const float* stat, hipStream_t st);
// cumulative_layer_norm: x -> y [n][257][B]; csum, csum2 [B] (both null or neither): the running sums of x and x^2, read when
// t_first > 0, written when not null;  origin as launch_fsn_cum_fb
void launch_fsn_cln_fb(const float* x, float* y, int n, int B, float* csum, float* csum2, int t_first, hipStream_t st,
                       const int32_t* origin = nullptr);
// sb [n][32][S] in place; csum, csum2 [S] as above
void launch_fsn_cln_sb(float* sb, int n, int S, float* csum, float* csum2, int t_first, hipStream_t st, const int32_t* origin = nullptr);
// maskT [ns][2][257 * B] on columns [col0, col0 + ns) of spec -> est [B][2][257][Tw]; steps with gt0 + tau < LA are skipped
void launch_fsn_stream_apply(const float* maskT, const float* spec, float* est, int B, int Tw, int ns, int col0, int gt0,
                             float p_out, hipStream_t st, const int32_t* origin = nullptr);

}  // namespace se

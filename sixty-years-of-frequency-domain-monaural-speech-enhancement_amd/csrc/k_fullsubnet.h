// Launchers of FullSubNet's private kernels (k_fullsubnet.hip): the utterance-mean and cumulative Laplace norms, the utterance
// Gaussian norm and the cumulative LayerNorm, the sub-band unfold, the mask back end and its frame-online form.
// model_fullsubnet.hip calls them; csrc/tests/model_probe.hip and csrc/tests/fsn_norm_probe.hip call them one at a time.
// Every launcher takes what its kernel takes (the per-row frame counts `tlen` of a ragged batch, the running sums
// `csum` of a stream and the stream's first frame `t_first` included) plus the sizes the grid is cut from.
#pragma once
#include "kernels.h"

namespace se {

namespace fsn {      // (a namespace of their own: other models have an NBIN too)
// The decode script's shape (fullsubnet_sa_decode_vb.py:11-24): look_ahead = 2, sb_num_neighbors = 15, fb_num_neighbors = 0, a sub-band
// input of 31 noisy rows + 1 full-band row.  They are the launchers' defaults; an engine passes its own (model_fullsubnet.hip).
constexpr int NBIN = 257, LA = 2, SBN = 15, SBW = 2 * SBN + 2;
// What an engine accepts: look_ahead 0..6, both neighbour counts 0..15 (include/se_engine.h)
constexpr int LA_MAX = 6, NEIGHBORS_MAX = 15, SBW_MAX = 4 * NEIGHBORS_MAX + 2;
constexpr int sb_width(int sbn, int fbn) { return (2 * sbn + 1) + (2 * fbn + 1); }      // model.py:50
constexpr int FSN_SUM_BLOCKS = 1024;                      // workgroups of the column sum = rows of its partials
constexpr float FSN_EPS = 1.1920928955078125e-07f;        // np.finfo(np.float32).eps (constant.py:8)
}  // namespace fsn

// Trailing arguments la / W / sbn / fbn: the engine's look-ahead, sub-band width and neighbour counts (default: the script's).
// mag [B][n] -> mu[b] = sum / denom;  tlen != null: denom = 257 * (tlen[b] + la)
void launch_fsn_mean(const float* mag, int B, int n, float denom, float* mu, const int* tlen, hipStream_t st, int la = fsn::LA);
// y[i] = x[i] / (mu[i % B] + 1e-5), i < n
void launch_fsn_scale(const float* x, float* y, long n, int B, const float* mu, hipStream_t st);
// magT, fbo [steps][257][B] -> sb [steps][W][257 * B], W = sb_width(sbn, fbn): 2 sbn + 1 rows of magT then 2 fbn + 1 rows of fbo around
// each bin, the frequency axis reflect-padded (BaseModel.unfold)
void launch_fsn_build_sb(const float* magT, const float* fbo, float* sb, int B, int steps, hipStream_t st, int sbn = fsn::SBN,
                         int fbn = 0);
// x [rows][B] -> part [FSN_SUM_BLOCKS][B];  tlen != null: column b stops at row (tlen[b] + la) * frame_rows (= W * 257).  B <= 256
void launch_fsn_colsum(const float* x, long rows, int B, float* part, const int* tlen, hipStream_t st,
                       long frame_rows = (long)fsn::SBW * fsn::NBIN, int la = fsn::LA);
// part [FSN_SUM_BLOCKS][B] -> mu[b] = sum / denom;  tlen != null: denom = (tlen[b] + la) * frame_rows.  B <= 256
void launch_fsn_finish_mean(const float* part, float* mu, float denom, int B, const int* tlen, hipStream_t st,
                            long frame_rows = (long)fsn::SBW * fsn::NBIN, int la = fsn::LA);
// maskBT [257 * B][2][T + la] (sequence s = n * B + b) -> out [B][2][257][T]: the mask itself (spec == null, the forward hook) or
// the decompressed product with spec [B][2][257][T]
void launch_fsn_mask(const float* maskBT, const float* spec, float* out, int B, int T, float p_out, hipStream_t st, int la = fsn::LA);
// x -> y [n][257][B]; csum [B] (may be null), read when t_first > 0, written when not null
// origin (optional, [B] int32 on the device: SE_CFG_STREAM_ROW_ORIGINS): row b counts from t_first - origin[b]
void launch_fsn_cum_fb(const float* x, float* y, int n, int B, float* csum, int t_first, hipStream_t st, const int32_t* origin = nullptr);
// sb [n][W][S] in place; csum [S] as above
void launch_fsn_cum_sb(float* sb, int n, int S, float* csum, int t_first, hipStream_t st, const int32_t* origin = nullptr,
                       int W = fsn::SBW);
// offline_gaussian_norm: x [rows][B] (rows = frames * frame_rows, t-major) -> part [FSN_SUM_BLOCKS][2][B] float64, the partial sums of
// x and x^2;  tlen != null: column b stops at row (tlen[b] + la) * frame_rows.  B <= 256
void launch_fsn_moments(const float* x, long rows, int B, double* part, const int* tlen, long frame_rows, hipStream_t st,
                        int la = fsn::LA);
// part -> stat [2][B]: the mean, and the unbiased std + 1e-5 (N = rows, or the row's own (tlen[b] + la) * frame_rows).  B <= 256
void launch_fsn_finish_gauss(const double* part, float* stat, long rows, int B, const int* tlen, long frame_rows, hipStream_t st,
                             int la = fsn::LA);
// y[i] = (x[i] - stat[i % B]) / stat[B + i % B], i < n  (y may be x)
void launch_fsn_gauss_apply(const float* x, float* y, long n, int B, const float* stat, hipStream_t st);
// cumulative_layer_norm: x -> y [n][257][B]; csum, csum2 [B] (both null or neither): the running sums of x and x^2, read when
// t_first > 0, written when not null;  origin as launch_fsn_cum_fb
void launch_fsn_cln_fb(const float* x, float* y, int n, int B, float* csum, float* csum2, int t_first, hipStream_t st,
                       const int32_t* origin = nullptr);
// sb [n][W][S] in place; csum, csum2 [S] as above
void launch_fsn_cln_sb(float* sb, int n, int S, float* csum, float* csum2, int t_first, hipStream_t st, const int32_t* origin = nullptr,
                       int W = fsn::SBW);
// maskT [ns][2][257 * B] on columns [col0, col0 + ns) of spec -> est [B][2][257][Tw]; steps with gt0 + tau < la are skipped
void launch_fsn_stream_apply(const float* maskT, const float* spec, float* est, int B, int Tw, int ns, int col0, int gt0,
                             float p_out, hipStream_t st, const int32_t* origin = nullptr, int la = fsn::LA);

}  // namespace se

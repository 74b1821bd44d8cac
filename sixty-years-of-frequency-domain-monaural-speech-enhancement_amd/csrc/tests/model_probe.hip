// Test-only probe of the kernels that used to be private to one model file, and of the layout movers no other probe calls:
// FullSubNet's norms, sub-band unfold and mask back end (k_fullsubnet.hip), TaylorSENet's and G2Net's elementwise recurrences, the
// tiled transpose, ELU and fill (k_misc.hip) - one launcher per call on device buffers the caller owns.  Entries whose kernel takes
// the per-row frame counts of a ragged batch publish a Ragged context for the call and hand its tlen to the launcher, as
// model_fullsubnet.hip does.  Plain C entry points for ctypes: tests/test_gpu_model_kernels.py compares every launch with float64.
// Not linked into libse_engine.so.
#include "../kernels.h"
#include "../k_fullsubnet.h"
#include <string>

using namespace se;

namespace {
thread_local std::string g_err;

// rows: device [4][MB] (len | lpad | tlen | olen, as the engine uploads a Ragged) or null; f takes the tlen the model would pass
template <typename F>
int guarded(const int* rows, int MB, F&& f) {
    Ragged rg;
    if (rows) {
        rg.len = rows;
        rg.lpad = rows + MB;
        rg.tlen = rows + 2 * MB;
        rg.olen = rows + 3 * MB;
    }
    try {
        SE_HIP(hipDeviceSynchronize());
        if (rows) set_ragged_ctx(&rg);
        const Ragged* cur = ragged_ctx();
        f(cur ? cur->tlen : nullptr);
        set_ragged_ctx(nullptr);
        SE_HIP(hipGetLastError());
        SE_HIP(hipDeviceSynchronize());
        return 0;
    } catch (const std::exception& e) {
        set_ragged_ctx(nullptr);
        g_err = e.what();
        return -1;
    }
}
template <typename F>
int plain(F&& f) {
    return guarded(nullptr, 0, [&](const int*) { f(); });
}
}  // namespace

extern "C" {

const char* mp_last_error() { return g_err.c_str(); }

// ---- k_misc.hip
int mp_transpose_akt(const float* in, float* out, int A, int K, int T, long in_sa, long in_sk, long out_st, long out_sk) {
    return plain([&] { launch_transpose_akt(in, out, A, K, T, in_sa, in_sk, out_st, out_sk, 0); });
}
int mp_elu(const float* x, float* y, long n) {
    return plain([&] { launch_elu(x, y, n, 0); });
}
int mp_fill(float* p, long n, float v) {
    return plain([&] { launch_fill(p, n, v, 0); });
}
int mp_taylor_zero(const float* gain, const float* spec, float* zero, float* out, long plane, long total) {
    return plain([&] { launch_taylor_zero(gain, spec, zero, out, plane, total, 0); });
}
int mp_taylor_update(const float* hob, float* pre, float* out, long n, float k, float inv_fact) {
    return plain([&] { launch_taylor_update(hob, pre, out, n, k, inv_fact, 0); });
}
int mp_gaf_combine(const float* gain, const float* pre, const float* resi, float* out, long plane, long total) {
    return plain([&] { launch_gaf_combine(gain, pre, resi, out, plane, total, 0); });
}

// ---- k_fullsubnet.hip
int mp_fsn_mean(const float* mag, int B, int n, float denom, float* mu, const int* rows, int MB) {
    return guarded(rows, MB, [&](const int* tlen) { launch_fsn_mean(mag, B, n, denom, mu, tlen, 0); });
}
int mp_fsn_scale(const float* x, float* y, long n, int B, const float* mu) {
    return plain([&] { launch_fsn_scale(x, y, n, B, mu, 0); });
}
int mp_fsn_build_sb(const float* magT, const float* fbo, float* sb, int B, int steps) {
    return plain([&] { launch_fsn_build_sb(magT, fbo, sb, B, steps, 0); });
}
int mp_fsn_colsum(const float* x, long nrows, int B, float* part, const int* rows, int MB) {
    return guarded(rows, MB, [&](const int* tlen) { launch_fsn_colsum(x, nrows, B, part, tlen, 0); });
}
int mp_fsn_finish_mean(const float* part, float* mu, float denom, int B, const int* rows, int MB) {
    return guarded(rows, MB, [&](const int* tlen) { launch_fsn_finish_mean(part, mu, denom, B, tlen, 0); });
}
int mp_fsn_mask(const float* maskBT, const float* spec, float* out, int B, int T, float p_out) {
    return plain([&] { launch_fsn_mask(maskBT, spec, out, B, T, p_out, 0); });
}
int mp_fsn_cum_fb(const float* x, float* y, int n, int B, float* csum, int t_first) {
    return plain([&] { launch_fsn_cum_fb(x, y, n, B, csum, t_first, 0); });
}
int mp_fsn_cum_sb(float* sb, int n, int S, float* csum, int t_first) {
    return plain([&] { launch_fsn_cum_sb(sb, n, S, csum, t_first, 0); });
}
int mp_fsn_stream_apply(const float* maskT, const float* spec, float* est, int B, int Tw, int ns, int col0, int gt0, float p_out) {
    return plain([&] { launch_fsn_stream_apply(maskT, spec, est, B, Tw, ns, col0, gt0, p_out, 0); });
}

}  // extern "C"

// Test-only probe of FullSubNet's Gaussian norm and cumulative LayerNorm (k_fullsubnet.hip: the one-pass float64 moments and their
// finish, the apply, the two-sum cumulative kernels) - one launcher per call on device buffers the caller owns.  Entries whose kernel
// takes the per-row frame counts of a ragged batch publish a Ragged context for the call and hand its tlen to the launcher, as
// model_fullsubnet.hip does (and as model_probe.hip does for the Laplace norms).  Plain C entry points for ctypes:
// tests/test_gpu_fullsubnet_norm_kernels.py compares every launch with float64.  Not linked into libse_engine.so.
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
}  // namespace

extern "C" {

const char* fnp_last_error() { return g_err.c_str(); }

int fnp_moments(const float* x, long nrows, int B, double* part, const int* rows, int MB, long frame_rows) {
    return guarded(rows, MB, [&](const int* tlen) { launch_fsn_moments(x, nrows, B, part, tlen, frame_rows, 0); });
}
int fnp_finish_gauss(const double* part, float* stat, long nrows, int B, const int* rows, int MB, long frame_rows) {
    return guarded(rows, MB, [&](const int* tlen) { launch_fsn_finish_gauss(part, stat, nrows, B, tlen, frame_rows, 0); });
}
int fnp_gauss_apply(const float* x, float* y, long n, int B, const float* stat) {
    return guarded(nullptr, 0, [&](const int*) { launch_fsn_gauss_apply(x, y, n, B, stat, 0); });
}
int fnp_cln_fb(const float* x, float* y, int n, int B, float* csum, float* csum2, int t_first, const int32_t* origin) {
    return guarded(nullptr, 0, [&](const int*) { launch_fsn_cln_fb(x, y, n, B, csum, csum2, t_first, 0, origin); });
}
int fnp_cln_sb(float* sb, int n, int S, float* csum, float* csum2, int t_first, const int32_t* origin) {
    return guarded(nullptr, 0, [&](const int*) { launch_fsn_cln_sb(sb, n, S, csum, csum2, t_first, 0, origin); });
}

}  // extern "C"

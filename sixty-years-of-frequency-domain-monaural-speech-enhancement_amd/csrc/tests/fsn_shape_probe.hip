// Test-only probe of the FullSubNet launchers that take the model's shape at run time (k_fullsubnet.hip): the sub-band unfold with
// its two neighbour counts, the cumulative Laplace norm and cumulative LayerNorm of a sub-band tensor of any width W, and the Gaussian
// norm's moments and finish with a look-ahead other than the decode script's - one launcher per call on device buffers the caller
// owns.  The ragged entries publish a Ragged context and hand its tlen to the launcher, as fsn_norm_probe.hip does.  Plain C entry
// points for ctypes: tests/test_gpu_fullsubnet_shape_kernels.py compares the unfold with a numpy gather for equality and the norms
// with float64.  Not linked into libse_engine.so.
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

const char* fsp_last_error() { return g_err.c_str(); }

// magT, fbo [steps][257][B] -> sb [steps][(2 sbn + 1) + (2 fbn + 1)][257 * B]
int fsp_build_sb(const float* magT, const float* fbo, float* sb, int B, int steps, int sbn, int fbn) {
    return guarded(nullptr, 0, [&](const int*) { launch_fsn_build_sb(magT, fbo, sb, B, steps, 0, sbn, fbn); });
}
int fsp_cum_sb(float* sb, int n, int S, float* csum, int t_first, const int32_t* origin, int W) {
    return guarded(nullptr, 0, [&](const int*) { launch_fsn_cum_sb(sb, n, S, csum, t_first, 0, origin, W); });
}
int fsp_cln_sb(float* sb, int n, int S, float* csum, float* csum2, int t_first, const int32_t* origin, int W) {
    return guarded(nullptr, 0, [&](const int*) { launch_fsn_cln_sb(sb, n, S, csum, csum2, t_first, 0, origin, W); });
}
int fsp_moments(const float* x, long nrows, int B, double* part, const int* rows, int MB, long frame_rows, int la) {
    return guarded(rows, MB, [&](const int* tlen) { launch_fsn_moments(x, nrows, B, part, tlen, frame_rows, 0, la); });
}
int fsp_finish_gauss(const double* part, float* stat, long nrows, int B, const int* rows, int MB, long frame_rows, int la) {
    return guarded(rows, MB, [&](const int* tlen) { launch_fsn_finish_gauss(part, stat, nrows, B, tlen, frame_rows, 0, la); });
}
int fsp_gauss_apply(const float* x, float* y, long n, int B, const float* stat) {
    return guarded(nullptr, 0, [&](const int*) { launch_fsn_gauss_apply(x, y, n, B, stat, 0); });
}

}  // extern "C"

// Test-only probe of Uformer's private kernels (k_uformer.hip: the attentions along time and along frequency, the polar front / back
// end, the interaction of the two branches), one launcher per call on device buffers the caller owns, with a record of every dispatch
// (uf_set_launch_log).  Ragged batches go through set_ragged_ctx, as the engine publishes them.  Plain C entry points for ctypes:
// tests/test_gpu_uformer_kernels.py compares every launch with float64.  Not linked into libse_engine.so.
#include "../k_uformer.h"
#include <string>
#include <vector>

using namespace se;

namespace {
thread_local std::string g_err;
thread_local std::vector<UfLaunchRec> g_log;

// tlen (device [B] or null) published as the engine publishes a ragged batch
template <typename F>
int guarded(const int* tlen, F&& f) {
    Ragged rg;
    rg.tlen = tlen;
    try {
        SE_HIP(hipDeviceSynchronize());
        g_log.clear();
        uf_set_launch_log(&g_log);
        if (tlen) set_ragged_ctx(&rg);
        f();
        set_ragged_ctx(nullptr);
        uf_set_launch_log(nullptr);
        SE_HIP(hipGetLastError());
        SE_HIP(hipDeviceSynchronize());
        return 0;
    } catch (const std::exception& e) {
        set_ragged_ctx(nullptr);
        uf_set_launch_log(nullptr);
        g_err = e.what();
        return -1;
    }
}
}  // namespace

extern "C" {

const char* ap_last_error() { return g_err.c_str(); }

// dispatches of the last call
int ap_launch_count() { return (int)g_log.size(); }
const char* ap_launch_kernel(int i) { return i >= 0 && i < (int)g_log.size() ? g_log[i].kernel : ""; }
// nh, KB, Tk, nblocks, ragged, grid, block, shmem
int ap_launch_get(int i, long long* out, int n) {
    if (i < 0 || i >= (int)g_log.size()) return -1;
    const UfLaunchRec& r = g_log[i];
    const long long v[8] = {r.nh, r.KB, r.Tk, r.nblocks, r.ragged, r.grid, r.block, r.shmem};
    for (int k = 0; k < n && k < 8; ++k) out[k] = v[k];
    return 8;
}

int ap_att_t(const float* pq, float* out, int B, int F, int T, int nh, const int* tlen) {
    return guarded(tlen, [&] { launch_uf_att_t(pq, out, B, F, T, nh, 0); });
}
int ap_att_f(const float* pq, float* out, int B, int F, int T, int nh) {
    return guarded(nullptr, [&] { launch_uf_att_f(pq, out, B, F, T, nh, 0); });
}
int ap_prep(const float* spec, float* mag0, float* ph0, float* xc, float* xm, int B, int T, float p_in) {
    return guarded(nullptr, [&] { launch_uf_prep(spec, mag0, ph0, xc, xm, B, T, p_in, 0); });
}
int ap_fusion(float* cplx, float* mag, int B, long CP) {
    return guarded(nullptr, [&] { launch_uf_fusion(cplx, mag, B, CP, 0); });
}
int ap_post(const float* dc, const float* dm, const float* mag0, const float* ph0, float* est, int B, int T, float p_out) {
    return guarded(nullptr, [&] { launch_uf_post(dc, dm, mag0, ph0, est, B, T, p_out, 0); });
}
int ap_src_cplx(const float* spec, float* out, int B, int T, float p_in) {
    return guarded(nullptr, [&] { launch_uf_src_cplx(spec, out, B, T, p_in, 0); });
}

}  // extern "C"

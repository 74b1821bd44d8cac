// Test-only probe of the window-relative zero tail (window_rows.h, k_rows.hip): the single and the batched launch on device buffers
// the caller owns, and window_cut() as the host compiles it.  Plain C entry points for ctypes: tests/test_gpu_window_zero_tail.py
// compares every launch with a numpy statement for exact equality.  Not linked into libse_engine.so.
#include "../window_rows.h"
#include "../common.h"
#include <string>

using namespace se;

namespace {
thread_local std::string g_err;

template <typename F>
int guarded(F&& f) {
    try {
        SE_HIP(hipDeviceSynchronize());
        f();
        SE_HIP(hipGetLastError());
        SE_HIP(hipDeviceSynchronize());
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}
}  // namespace

extern "C" {

const char* wz_last_error() { return g_err.c_str(); }

int wz_window_cut(int tlen, int t0, int HC, int Tw) { return window_cut(tlen, t0, HC, Tw); }

// x: device [B][rows][Tw]; tlen: device [B]
int wz_zero_tail(float* x, int B, long long rows, int Tw, const int* tlen, int t0, int HC) {
    return guarded([&] { launch_window_zero_tail(x, B, (long)rows, Tw, tlen, t0, HC, 0); });
}

// bufs, rows: HOST arrays of n device pointers / row counts
int wz_zero_tail_batch(float* const* bufs, const long long* rows, int n, int B, int Tw, const int* tlen, int t0, int HC) {
    return guarded([&] {
        SE_CHECK(n >= 0 && n <= ZeroTailBatch::MAX, "wz_zero_tail_batch: 0..8 tensors");
        ZeroTailBatch zb;
        for (int k = 0; k < n; ++k) zb.add(bufs[k], (long)rows[k]);
        launch_window_zero_tail_batch(zb, B, Tw, tlen, t0, HC, 0);
    });
}

}  // extern "C"

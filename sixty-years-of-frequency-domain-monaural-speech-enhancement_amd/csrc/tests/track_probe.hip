// Test-only probe of the tracking unit-RMS scale of frame-online streams (se_stream_begin_tracking): the scale kernel (k_misc.hip:
// launch_stream_track) one push or flush per call, and the forward transform with per-frame scales (k_stft2.hip: stft2_kernel<.., FSC>),
// on device buffers the caller owns.  Plain C entry points for ctypes: tests/test_gpu_stream_tracking_kernels.py compares every launch
// with float64.  Not linked into libse_engine.so.
#include "../kernels.h"
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

const char* tp_last_error() { return g_err.c_str(); }

// one push (fin == 0: the n_new newest of n_total samples) or the flush (fin == 1, n_new == 0) of B rows whose window starts at w0
int tp_stream_track(int n_fft, int hop, const float* wav, long pitch, int B, int n_total, int n_new, int fin, double lam, double* ew,
                    float* c, float* frame_c, float* frame_inv, int ring, int t0, int t1, int w0) {
    return guarded([&] {
        launch_stream_track(StftGeom{n_fft, hop, n_fft}, wav, pitch, B, n_total, n_new, fin != 0, lam, ew, c, frame_c, frame_inv, ring, t0, t1,
                            0, w0);
    });
}

// frames [t_first, T) of B rows under the scales of the ring frame_c (null: under c_scale, the common kernel)
int tp_stft(int n_fft, int hop, const float* wav, long pitch, int B, int L, int Lpad, const float* c_scale, float p_in, float* spec_ri,
            float* mag, int T, int Tp, int t_first, int col0, int w0, const float* frame_c, int ring) {
    return guarded([&] {
        launch_stft(StftGeom{n_fft, hop, n_fft}, wav, pitch, B, L, Lpad, c_scale, p_in, spec_ri, mag, T, Tp, 0, t_first, col0, w0, frame_c, ring);
    });
}

}  // extern "C"

// Test-only probe of the front and back end every model and every stream passes through: the STFT / iSTFT (k_stft2.hip), the unit-RMS
// scales (k_stft.hip, k_misc.hip), the stream helpers, the mask / decompress kernels (k_misc.hip) and the row-size helpers (k_rows.hip),
// one launcher per call on device buffers the caller owns, with a record of the transform instance each launch asks for (fe_launch.h).
// Ragged batches go through set_ragged_ctx, as the engine publishes them.  Plain C entry points for ctypes:
// tests/test_gpu_frontend_kernels.py compares every launch with float64.  Not linked into libse_engine.so.
#include "../kernels.h"
#include "../fe_launch.h"
#include "../window_rows.h"
#include <string>
#include <vector>

using namespace se;

namespace {
thread_local std::string g_err;
thread_local std::vector<FeLaunchRec> g_log;

// rows: device [4][MB] (len | lpad | tlen | olen, as the engine uploads a Ragged) or null
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
        g_log.clear();
        fe_set_launch_log(&g_log);
        if (rows) set_ragged_ctx(&rg);
        f();
        set_ragged_ctx(nullptr);
        fe_set_launch_log(nullptr);
        SE_HIP(hipGetLastError());
        SE_HIP(hipDeviceSynchronize());
        return 0;
    } catch (const std::exception& e) {
        set_ragged_ctx(nullptr);
        fe_set_launch_log(nullptr);
        g_err = e.what();
        return -1;
    }
}
}  // namespace

extern "C" {

const char* fp_last_error() { return g_err.c_str(); }

// transform dispatches of the last call
int fp_launch_count() { return (int)g_log.size(); }
const char* fp_launch_kernel(int i) { return i >= 0 && i < (int)g_log.size() ? g_log[i].kernel : ""; }
// N, MAG, CP, FSC, grid x, grid y, block, shmem, ragged
int fp_launch_get(int i, long long* out, int n) {
    if (i < 0 || i >= (int)g_log.size()) return -1;
    const FeLaunchRec& r = g_log[i];
    const long long v[9] = {r.N, r.MAG, r.CP, r.FSC, r.gx, r.gy, r.block, r.shmem, r.ragged};
    for (int k = 0; k < n && k < 9; ++k) out[k] = v[k];
    return 9;
}

int fp_stft(int n_fft, int hop, int win, const float* wav, long pitch, int B, int L, int Lpad, const float* c_scale, float p_in,
            float* spec_ri, float* mag, int T, int Tp, int t_first, int col0, int w0, const int* rows, int MB) {
    return guarded(rows, MB, [&] {
        launch_stft(StftGeom{n_fft, hop, win}, wav, pitch, B, L, Lpad, c_scale, p_in, spec_ri, mag, T, Tp, 0, t_first, col0, w0);
    });
}
int fp_istft(int n_fft, int hop, int win, const float* spec_ri, int B, int T, int Tp, const float* c_scale, float* wav_out,
             long out_pitch, int Lout, int t_off, int t_lo, int o_lo, const float* frame_inv, int ring, const int* rows, int MB) {
    return guarded(rows, MB, [&] {
        launch_istft(StftGeom{n_fft, hop, win}, spec_ri, B, T, Tp, nullptr, c_scale, wav_out, out_pitch, Lout, 0, t_off, t_lo, o_lo,
                     frame_inv, ring);
    });
}
int fp_rms_scale(const float* wav, int B, int L, long pitch, float* c_out, const int* rows, int MB) {
    return guarded(rows, MB, [&] { launch_rms_scale(wav, B, L, pitch, c_out, 0); });
}
int fp_stream_rms(const float* wav, long pitch, int B, int n_total, int n_new, double* sumsq, float* c, float* frame_inv, int ring,
                  int t0, int t1, int w0) {
    return guarded(nullptr, 0, [&] { launch_stream_rms(wav, pitch, B, n_total, n_new, sumsq, c, frame_inv, ring, t0, t1, 0, w0); });
}
int fp_stream_slide(const float* src, float* dst, long pitch, int B, int shift, int n) {
    return guarded(nullptr, 0, [&] { launch_stream_slide(src, dst, pitch, B, shift, n, 0); });
}
int fp_dccrn_mask(const float* mask, const float* spec, float* est, int B, int F, int T, int Tp, float p_out, int mode) {
    return guarded(nullptr, 0, [&] { launch_dccrn_mask(mask, spec, est, B, F, T, Tp, p_out, 0, mode); });
}
int fp_cmask_apply(const float* mask, const float* spec, float* out, int B, int F, int T, float p_out) {
    return guarded(nullptr, 0, [&] { launch_cmask_apply(mask, spec, out, B, F, T, p_out, 0); });
}
int fp_mag_phase(const float* mag, const float* spec, float* out, int B, int F, int T, float p_out) {
    return guarded(nullptr, 0, [&] { launch_mag_phase(mag, spec, out, B, F, T, p_out, 0); });
}
int fp_polar_pow(const float* x, float* out, int B, int F, int T, float p_out) {
    return guarded(nullptr, 0, [&] { launch_polar_pow(x, out, B, F, T, p_out, 0); });
}
int fp_zero_tail(float* x, int B, long nrows, int T, const int* rows, int MB) {
    return guarded(rows, MB, [&] { launch_zero_tail(x, B, nrows, T, 0); });
}
int fp_fill_rows(int* d, int MB, int B, int len, int lpad, int tlen, int olen) {
    return guarded(nullptr, 0, [&] { launch_fill_rows(d, MB, B, len, lpad, tlen, olen, 0); });
}
int fp_window_rows(const int* src, int* dst, int MB, int B, int t_hi) {
    return guarded(nullptr, 0, [&] { launch_window_rows(src, dst, MB, B, t_hi, 0); });
}

}  // extern "C"

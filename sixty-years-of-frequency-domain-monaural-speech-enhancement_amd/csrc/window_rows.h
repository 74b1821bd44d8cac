// Per-window view of the per-row sizes of a ragged call, for the windowed decode of rows of different lengths
// (se_enhance_long_ragged, engine.hip stream_process), and the window-relative end of a row inside a chunk tensor.
// window_cut() is plain arithmetic and compiles without HIP (csrc/tests/window_cut_check.cpp runs it under the host sanitizers);
// everything else needs the HIP compiler.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SE_WINDOW_HD __host__ __device__
#else
#define SE_WINDOW_HD
#endif

namespace se {

// A chunk tensor holds Tw columns, column c = frame t0 - HC + c (HC history columns, then the new frames from t0 on).  For a row of
// `tlen` frames (0 .. tlen - 1) the columns [0, cut) hold frames of the row and [cut, Tw) frames at or past its end:
//   cut = clamp(tlen - (t0 - HC), 0, Tw)
// 0: the row ended before the window, Tw: it has not ended inside it.  The difference is taken in 64 bits: tlen and t0 run to the
// frame count of the position bound (2^31 - 1 - n_fft - 32 hop samples), and t0 - HC is negative in the first window.
SE_WINDOW_HD inline int window_cut(int tlen, int t0, int HC, int Tw) {
    const long long d = (long long)tlen - ((long long)t0 - HC);
    return d <= 0 ? 0 : d >= Tw ? Tw : (int)d;
}

#ifdef __HIPCC__
// src, dst: device [4][MB] ints laid out as the engine uploads a `Ragged` (len | lpad | tlen | olen, kernels.h), rows 0..B-1.
//   dst.tlen[b] = min(src.tlen[b], t_hi),  the three sample counts copied.
// The STFT and the iSTFT count frames absolutely inside a window too, but a window launch only owns the frames below its own upper
// bound t_hi (the STFT's T = t0 + n, the iSTFT's T = t_fin): with the row's whole-clip frame count they would pair / load frames of
// later windows.  With this view a row that has not ended sees exactly the bound an equal-length launch has (T), a row that ends
// inside or before the window its own last frame.  Runs on the device in stream order: the host walks the windows without waiting.
void launch_window_rows(const int* src, int* dst, int MB, int B, int t_hi, hipStream_t s);

// The rows' whole-clip frame counts for a network that looks AHEAD behind its input layer (the `_vb` DCCRN's decoder, engines made
// with SE_CFG_DCCRN_ROW_ENDS): a context of its own, published by stream_process around stream_chunk of a ragged walk only.  It is
// NOT the ragged context (kernels.h ragged_ctx): no launcher reads it, so the conv / norm / transform launchers inside a chunk go on
// seeing rows of one length; only the model's own zero-tail launches below take it.
struct WindowEnds {
    const int* tlen = nullptr;      // device [B]: whole-clip frame count of row b (the uploaded Ragged's tlen, absolute)
    int t0 = 0;                     // first new frame of the chunk being enqueued
};
const WindowEnds* window_ends_ctx();                // nullptr: rows of one length, or no windowed walk
void set_window_ends_ctx(const WindowEnds* w);      // thread-local, as set_ragged_ctx

// x[b][r][c] = 0 for c in [window_cut(tlen[b], t0, HC, Tw), Tw), for up to MAX tensors [B][rows_k][Tw] of one chunk in one launch
// (blockIdx.z = tensor); everything else stays bit-untouched.  The cut is taken on the device from tlen[b]; a row that has not
// ended inside the window costs its blocks one load and a return.
struct ZeroTailBatch {
    static constexpr int MAX = 8;
    float* buf[MAX];
    long rows[MAX];
    int n = 0;
    void add(float* b, long r) {
        buf[n] = b;
        rows[n] = r;
        ++n;
    }
};
void launch_window_zero_tail_batch(const ZeroTailBatch& zb, int B, int Tw, const int* tlen, int t0, int HC, hipStream_t s);
// one tensor
void launch_window_zero_tail(float* x, int B, long rows, int Tw, const int* tlen, int t0, int HC, hipStream_t s);
#endif

}  // namespace se

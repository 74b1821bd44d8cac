// Per-window view of the per-row sizes of a ragged call, for the windowed decode of rows of different lengths
// (se_enhance_long_ragged, engine.hip stream_process).
#pragma once
#include <hip/hip_runtime.h>

namespace se {

// src, dst: device [4][MB] ints laid out as the engine uploads a `Ragged` (len | lpad | tlen | olen, kernels.h), rows 0..B-1.
//   dst.tlen[b] = min(src.tlen[b], t_hi),  the three sample counts copied.
// The STFT and the iSTFT count frames absolutely inside a window too, but a window launch only owns the frames below its own upper
// bound t_hi (the STFT's T = t0 + n, the iSTFT's T = t_fin): with the row's whole-clip frame count they would pair / load frames of
// later windows.  With this view a row that has not ended sees exactly the bound an equal-length launch has (T), a row that ends
// inside or before the window its own last frame.  Runs on the device in stream order: the host walks the windows without waiting.
void launch_window_rows(const int* src, int* dst, int MB, int B, int t_hi, hipStream_t s);

}  // namespace se

// Sliding input window of frame-online streams (SE_CFG_STREAM_SLIDING): the host arithmetic, nothing else.
//
// A stream's samples live in rows of `pitch` floats; column 0 holds the absolute sample w0 (the window origin), the live
// range is [w0, n_total).  Before a push appends n_new <= max_samples samples that would not fit behind the live range, the
// engine drops everything below stream_keep_from() and moves the rest to column 0 (k_misc.hip: launch_stream_slide).
#pragma once
#include <algorithm>
#include <cstdint>

namespace se {

// floats per row: max_samples (the largest push) + what stays live across a push (< n_fft + hop, see below), rows 16 B aligned
inline long stream_window_pitch(int max_samples, int n_fft, int hop) { return ((long)max_samples + n_fft + hop + 3) & ~3L; }

// the longest stream of a sliding engine, 2^31 - 1 - max_samples samples: every position that crosses calls (n_total, o_done,
// t_done * hop) and every index a kernel forms from them stays an int.  The kernels reach at most half a window + the
// hop-multiple tail pad + one iSTFT block of 32 frames past n_total, so an engine made for clips shorter than that keeps
// that much headroom instead.
inline int64_t stream_sample_limit(int max_samples, int n_fft, int hop) {
    return (int64_t)INT32_MAX - std::max<int64_t>(max_samples, (int64_t)n_fft + 32 * (int64_t)hop);
}

// The first sample any launch AFTER this point can still read, rounded down to a multiple of 4 (the origin stays 16 B aligned
// so that the STFT's wave-uniform loads keep the alignment they have at origin 0), given that frames [0, t_done) are
// transformed and n_total samples have arrived.  Readers of the window:
//   (a) the STFT of a frame t >= t_done (frames below t_done are never transformed again): samples t hop - n_fft/2 ...
//       t hop + n_fft/2 - 1, the lowest of them t_done hop - n_fft/2.  Where that is negative the kernel mirrors (idx -> -idx,
//       the left reflection of the first frames) into [0, n_fft/2]: the bound clamps to 0, so nothing is dropped before every
//       frame that touches the left edge is done.
//   (b) the right-edge reflection at se_stream_flush: idx >= Lpad -> 2 (Lpad - 1) - idx.  The largest idx is the last sample of
//       the last frame, (T - 1) hop + n_fft/2 - 1 <= Lpad + n_fft/2 - 1 (T - 1 = Lpad / hop), whose mirror image is
//       Lpad - n_fft/2 - 1 - and Lpad at the flush >= n_total at the flush >= n_total now.
//   (c) DCCRN's zero tail pad [L, Lpad) is produced by the kernel (idx >= L gives 0): no stored sample.
//   (d) the running RMS reads the n_new newest samples only; they are appended after the slide.
// Both t_done and n_total only grow, so the bound of one call holds for every later one.  With hop <= n_fft/2 (a) is the lower
// of the two after every push (t_done = t_avail, t_avail hop <= n_total - n_fft/2 - 1 + hop), and what stays live is
// n_total - keep <= n_fft + 3 (t_avail hop >= n_total - n_fft/2): a push of max_samples always fits into stream_window_pitch().
inline int stream_keep_from(int n_fft, int hop, int t_done, int n_total) {
    const int64_t a = (int64_t)t_done * hop - n_fft / 2;
    const int64_t b = (int64_t)n_total - n_fft / 2 - 1;
    return (int)(std::max<int64_t>(0, std::min(a, b)) & ~(int64_t)3);
}

}  // namespace se

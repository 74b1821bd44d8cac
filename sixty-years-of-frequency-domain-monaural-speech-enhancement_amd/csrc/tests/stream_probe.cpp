// Test-only: the host arithmetic of sliding stream windows (stream_window.h) behind a C interface, no device code
// (tests/test_sliding_window_logic.py scans it against the STFT kernel's index rules).
#include "../stream_window.h"

extern "C" {
int sp_keep_from(int n_fft, int hop, int t_done, int n_total) { return se::stream_keep_from(n_fft, hop, t_done, n_total); }
long sp_window_pitch(int max_samples, int n_fft, int hop) { return se::stream_window_pitch(max_samples, n_fft, hop); }
long long sp_sample_limit(int max_samples, int n_fft, int hop) { return se::stream_sample_limit(max_samples, n_fft, hop); }
}

// Test-only, host code alone: the cumulative LayerNorm's kernel selection (cln_select.h) behind plain C entry points for ctypes
// (tests/test_cln_select_host.py).  No device code; built with -x c++ like lstm_select_probe.cpp.  The switches are arguments here
// (plane, stream_res), not the environment.
#include "../cln_select.h"

using namespace se;

namespace {
ClnTuning tuning(int plane, int stream_res) {
    ClnTuning t;
    t.plane = plane != 0;
    t.stream_res = stream_res != 0;
    return t;
}
}  // namespace

extern "C" {

// form, n_launch, c0, back, WP, W, VPT, takes_res, scratch
int css_choice_fields() { return 9; }
// kernel, gx, gy, gz, block, lds, res - of each of the three launch entries
int css_launch_fields() { return 7; }
const char* css_form_name(int form) { return cln_form_name(form); }
const char* css_kernel_name(int kernel) { return cln_kernel_name(kernel); }

// cln_select: in = B, C, F, T, K, pre, post, res, parts, ragged, stream, H, n, sB; out = the choice as css_choice_fields() integers,
// then css_launch_fields() per launch entry (all three; those from n_launch on are unused); returns its refusal message ("" when
// the call was accepted)
const char* css_select(const int* in, int plane, int stream_res, long long* out) {
    ClnSelIn s;
    s.B = in[0]; s.C = in[1]; s.F = in[2]; s.T = in[3]; s.K = in[4];
    s.pre = in[5] != 0; s.post = in[6] != 0; s.res = in[7] != 0;
    s.parts = in[8] != 0; s.ragged = in[9] != 0; s.stream = in[10] != 0;
    s.H = in[11]; s.n = in[12]; s.sB = in[13];
    const ClnChoice c = cln_select(s, tuning(plane, stream_res));
    const long long v[9] = {c.form, c.n_launch, c.c0, c.back, c.WP, c.W, c.VPT, c.takes_res, (long long)c.scratch};
    for (int k = 0; k < 9; ++k) out[k] = v[k];
    for (int i = 0; i < 3; ++i) {
        const ClnLaunch& l = c.launch[i];
        const long long w[7] = {l.kernel, l.gx, l.gy, l.gz, l.block, (long long)l.lds, l.res};
        for (int k = 0; k < 7; ++k) out[9 + 7 * i + k] = w[k];
    }
    return c.refusal;
}
// the query behind cln_stream_takes_res for a chunk of H + n columns
int css_chunk_takes_res(int B, int C, int F, int H, int n, int stream_res) { return cln_chunk_takes_res(B, C, F, H, n, tuning(1, stream_res)); }

}  // extern "C"

// Test-only, host code alone: the cooperative LSTM's kernel selection (lstm_select.h) behind plain C entry points for ctypes
// (tests/test_lstm_select_host.py).  No device code; built with -x c++ like gc_select_probe.cpp.  The switches are arguments here
// (coop16, coop4, ...), not the environment.
#include "../lstm_select.h"

using namespace se;

namespace {
LstmTuning tuning(int coop16, int coop4, int coop256, int chunk) {
    LstmTuning t;
    t.coop16 = coop16;
    t.coop4 = coop4;
    t.coop256 = coop256;
    t.chunk = chunk;
    return t;
}
// form, H, NS, TAG, LEAD, NW, L, Z, SS, grid, block, lds, lds_attr, nflag, stale, zero_cell, slabs, chunk
constexpr int CHOICE_FIELDS = 18;
void flatten(const LstmChoice& c, long long* o) {
    const long long v[CHOICE_FIELDS] = {c.form, c.H,  c.NS,    c.TAG,          c.LEAD,     c.NW,    c.L,     c.Z,         c.SS,
                                        c.grid, c.block, (long long)c.lds, c.lds_attr, c.nflag, c.stale, c.zero_cell, c.slabs, c.chunk};
    for (int k = 0; k < CHOICE_FIELDS; ++k) o[k] = v[k];
}
}  // namespace

extern "C" {

int lss_choice_fields() { return CHOICE_FIELDS; }
const char* lss_form_name(int form) { return lstm_form_name(form); }

// lstm_coop_select: out = the choice as CHOICE_FIELDS integers; returns its refusal message ("" when a kernel was chosen)
const char* lss_select(int H, int S, int Z, long gx_row, long out_row, int n_cu, int chunk, int n_layers, int coop16, int coop4, int coop256,
                       long long* out) {
    LstmSelIn in;
    in.H = H; in.S = S; in.Z = Z;
    in.gx_row = gx_row; in.out_row = out_row;
    in.n_cu = n_cu;
    in.chunk = chunk; in.n_layers = n_layers;
    const LstmChoice c = lstm_coop_select(in, tuning(coop16, coop4, coop256, 1));
    flatten(c, out);
    return c.refusal;
}
const char* lss_stack_select(int H, int L, int n_cu, long long* out) {
    const LstmChoice c = lstm_stack_select(H, L, n_cu);
    flatten(c, out);
    return c.refusal;
}

int lss_coop_ok(int H, int S, int Z) { return lstm_coop_ok(H, S, Z); }
int lss_coop256_ok(int S, int n_cu, int coop16, int coop256) { return lstm_coop256_ok(S, n_cu, tuning(coop16, 1, coop256, 1)); }
int lss_chunk_ok(int H, int S, int n_layers, int n_cu, int chunk) { return lstm_coop_chunk_ok(H, S, n_layers, n_cu, tuning(1, 1, 1, chunk)); }
int lss_stack_ok(int H, int L, int n_cu) { return lstm_stack_ok(H, L, n_cu); }
int lss_chunk_steps(int H, int S, int n_layers, int T, int n_cu, int chunk) {
    return lstm_chunk_steps(H, S, n_layers, T, n_cu, tuning(1, 1, 1, chunk));
}
int lss_chunk_launches(int T, int Tc, int L) { return lstm_chunk_launches(T, Tc, L); }
// the ranges of launch s as (layer, t0, len) triples in out[12]; returns their number
int lss_chunk_launch(int T, int Tc, int L, int s, int* out) {
    LstmChunkRange r[4];
    const int n = lstm_chunk_launch(T, Tc, L, s, r);
    for (int i = 0; i < n; ++i) {
        out[3 * i] = r[i].layer;
        out[3 * i + 1] = r[i].t0;
        out[3 * i + 2] = r[i].len;
    }
    return n;
}

}  // extern "C"

// Test-only, host code alone: gc_select (gc_select.h) behind plain C entry points for ctypes (tests/test_gc_select_host.py).
// No device code; built with -x c++ like stream_probe.cpp.
#include "gc_selin_flat.h"
#include <string>

using namespace se;

namespace {
thread_local std::string g_err;

// the launch-log record a dispatch leaves (gc_launch_rec, what gc_log_launch stores), in the order of gc_probe.hip's gcp_launch_get
void record(const GCSelIn& in, const GCDispatch& d, long long* o) {
    const GCLaunchRec r = gc_launch_rec(in, d, 0);
    const long long v[14] = {r.family, r.BM,    r.BN,     r.flat_upr, r.upt,  r.flat_rows,        r.qt2,
                             r.nrm,    r.res,   r.trim,   r.stats,    r.ragged, r.flat_nrm_refused, r.nblk};
    for (int k = 0; k < 14; ++k) o[k] = v[k];
}
}  // namespace

extern "C" {

const char* gcs_last_error() { return g_err.c_str(); }
int gcs_selin_fields() { return GC_SELIN_FIELDS; }

// in: GCSelIn as GC_SELIN_FIELDS integers (gc_selin_flatten's order).  out: the records of the dispatches in launch order (the
// tail launch first), 14 integers each; extra: per dispatch {geom, form, n_ttiles, Qt, lds bytes, nbuf, pw4, t_base}.
// Returns the number of dispatches (1 or 2), -1 when gc_select refuses the launch (gcs_last_error).
int gcs_select(const long long* in, long long* out, long long* extra) {
    try {
        const GCSelIn s = gc_selin_unflatten(in);
        const GCChoice ch = gc_select(s);
        int n = 0;
        for (const GCDispatch* d : {ch.has_tail ? &ch.tail : nullptr, &ch.main}) {
            if (!d) continue;
            record(s, *d, out + 14 * n);
            const long long e[8] = {d->geom, d->form, d->n_ttiles, d->Qt, (long long)d->lds, d->nbuf, d->pw4, d->t_base};
            for (int k = 0; k < 8; ++k) extra[8 * n + k] = e[k];
            ++n;
        }
        return n;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}

int gcs_flat_rows_spanned(int B, int upr, int upt) { return gc_flat_rows_spanned(B, upr, upt); }

// facts of the plan gc_plan_shape gives a layer: BM, BN, CI_C, KCp, nrows, dtmin, causal, lookback, flat_uw, tail_split, qt2_nrows,
// qt2_qoff, then BN and Wp of the GC_G_COUNT geometries
int gcs_plan_shape(int M, int Cin, int ntaps, const int* df, const int* dt, int epi, int si, int tout_hint, int Z, int C0split, int* out) {
    try {
        TapSpec t;
        SE_CHECK(ntaps >= 0 && ntaps <= GC_MAX_TAPS, "tap count");
        t.ntaps = ntaps;
        for (int j = 0; j < ntaps; ++j) {
            t.df[j] = df[j];
            t.dt[j] = dt[j];
        }
        const GCPlanShape s = gc_plan_shape(M, Cin, t, epi, si, tout_hint, Z, C0split);
        int k = 0;
        for (int v : {s.BM, s.BN, s.CI_C, s.KCp, s.nrows, s.dtmin, s.causal, s.lookback, s.flat_uw, (int)s.tail_split, s.qt2_nrows, s.qt2_qoff})
            out[k++] = v;
        for (int g = 0; g < GC_G_COUNT; ++g) {
            out[k++] = s.geom[g].BN;
            out[k++] = s.geom[g].Wp;
        }
        return k;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}

// edge-row classes of a tap set on a plane (gc_edge_classes): out = nclass, cls_lo, cls_hi, then per class (GC_EDGE_MAX of them)
// dead-tap mask, live K rows of a chunk, the same padded, and GC_MAX_KCP entries of the surviving class-0 K rows
int gcs_edge_classes(int ntaps, const int* df, int cic, int si, int Fin, int Q, int* out) {
    TapSpec t;
    if (ntaps < 0 || ntaps > GC_MAX_TAPS) return -1;
    t.ntaps = ntaps;
    for (int j = 0; j < ntaps; ++j) {
        t.df[j] = df[j];
        t.dt[j] = 0;
    }
    const GCEdgeShape e = gc_edge_classes(t, cic, si, Fin, Q);
    int k = 0;
    out[k++] = e.nclass; out[k++] = e.cls_lo; out[k++] = e.cls_hi;
    for (int c = 0; c < GC_EDGE_MAX; ++c) {
        out[k++] = (int)e.dead[c]; out[k++] = e.KC[c]; out[k++] = e.KCp[c];
        for (int i = 0; i < GC_MAX_KCP; ++i) out[k++] = e.live[c][i];
    }
    return k;
}

}  // extern "C"

// Test-only: GCSelIn (gc_select.h) as a flat integer array, for the probes' ctypes entry points (gc_probe.hip gcp_select_get,
// gc_select_probe.cpp gcs_select) and the fixture tests/golden/gc_select_parent.jsonl.gz.  tests/test_gc_select_host.py SELIN names
// the fields in the same order.
#pragma once
#include "../gc_select.h"

namespace se {

constexpr int GC_SELIN_FIELDS = 2 + 2 * GC_G_COUNT + 4 + 4 + 4 + 4 + 17 + 6 + 9 + 2 + 6;
// GCSelIn as integers, in the order of the struct's declaration (g_BN[0..6], then g_Wp[0..6]; tun last: alt_n64, wide_min,
// wide_fill, qt2_min, flat, dbg)
inline void gc_selin_flatten(const GCSelIn& s, long long* o) {
    int k = 0;
    o[k++] = s.BM; o[k++] = s.BN;
    for (int g = 0; g < GC_G_COUNT; ++g) o[k++] = s.g_BN[g];
    for (int g = 0; g < GC_G_COUNT; ++g) o[k++] = s.g_Wp[g];
    for (long long v : {s.flat_uw, s.tail_split, s.qt2_nrows, s.qt2_qoff, s.CI_C, s.nrows, s.KCp, s.causal, s.sm_dfmin, s.sm_dfmax,
                        s.sm_dtmin, s.sm_dtmax, s.pl_C0, s.pl_C1, s.pl_epi, s.pl_Ws, s.epi, s.Z, s.B, s.Q, s.M, s.n_mtiles, s.Tout,
                        s.Tin, s.Fin, s.t_base, s.tb_soft, s.C0, s.C1, s.pad_lo, s.first_step, s.pair, s.si})
        o[k++] = v;
    for (long long v : {s.s0_b, s.s0_c, s.s0_f, s.s1_b, s.s1_c, s.s1_f}) o[k++] = v;
    for (long long v : {s.Ws, s.desc4, s.stats, s.cstats, s.nrm0, s.nrm1, s.fz, s.dst_elu, s.tlen, s.overread0, s.overread1})
        o[k++] = v;
    o[k++] = s.tun.alt_n64; o[k++] = s.tun.wide_min; o[k++] = s.tun.wide_fill; o[k++] = s.tun.qt2_min; o[k++] = s.tun.flat;
    o[k++] = s.tun.dbg;
}
inline GCSelIn gc_selin_unflatten(const long long* o) {
    GCSelIn s{};
    int k = 0;
    s.BM = (int)o[k++]; s.BN = (int)o[k++];
    for (int g = 0; g < GC_G_COUNT; ++g) s.g_BN[g] = (int)o[k++];
    for (int g = 0; g < GC_G_COUNT; ++g) s.g_Wp[g] = (int)o[k++];
    for (int* f : {&s.flat_uw, &s.tail_split, &s.qt2_nrows, &s.qt2_qoff, &s.CI_C, &s.nrows, &s.KCp, &s.causal, &s.sm_dfmin, &s.sm_dfmax,
                   &s.sm_dtmin, &s.sm_dtmax, &s.pl_C0, &s.pl_C1, &s.pl_epi, &s.pl_Ws, &s.epi, &s.Z, &s.B, &s.Q, &s.M, &s.n_mtiles, &s.Tout,
                   &s.Tin, &s.Fin, &s.t_base, &s.tb_soft, &s.C0, &s.C1, &s.pad_lo, &s.first_step, &s.pair, &s.si})
        *f = (int)o[k++];
    for (long* f : {&s.s0_b, &s.s0_c, &s.s0_f, &s.s1_b, &s.s1_c, &s.s1_f}) *f = (long)o[k++];
    for (int* f : {&s.Ws, &s.desc4, &s.stats, &s.cstats, &s.nrm0, &s.nrm1, &s.fz, &s.dst_elu, &s.tlen, &s.overread0, &s.overread1})
        *f = (int)o[k++];
    s.tun.alt_n64 = (int)o[k++]; s.tun.wide_min = (long)o[k++]; s.tun.wide_fill = (int)o[k++]; s.tun.qt2_min = (long)o[k++];
    s.tun.flat = (int)o[k++]; s.tun.dbg = (int)o[k++];
    return s;
}

}  // namespace se

// Stand-alone host program over gc_select.h, meant for `-fsanitize=address,undefined` (make gc_select_check): no device code, not
// loaded into anything.  One hand-written launch per rung of gemmconv's selection ladder - thin (before and after the preamble),
// direct and its LDS-tiled form, 64- and 32-column small launches, resident-K, flattened (narrow, wide, normalising, refused),
// 64 x 256, the LSTM step's 128 x 256, two-row, tail split and the plan's own tile - and the launches the ladder refuses, each of
// which has to be refused with its own message.  Exit status 0 and "ok" when everything holds.
#include "../gc_select.h"
#include <cstdio>
#include <cstring>

using namespace se;

static int failures = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("line %d: %s\n", __LINE__, #c);                  \
            ++failures;                                                  \
        }                                                                \
    } while (0)

static TapSpec taps_of(int nkf, int nkt, int pf, int pt) {
    TapSpec t;
    t.ntaps = nkf * nkt;
    for (int a = 0; a < nkf; ++a)
        for (int b = 0; b < nkt; ++b) {
            t.df[a * nkt + b] = a - pf;
            t.dt[a * nkt + b] = b - pt;
        }
    return t;
}

// a launch of a layer planned by gc_plan_shape: whole rows of T frames, one source inside the arena
static GCSelIn launch_of(int M, int Cin, const TapSpec& t, int epi, int si, int B, int Q, int T, int Z = 1) {
    const GCPlanShape s = gc_plan_shape(M, Cin, t, epi, si, 401, Z, -1);
    GCSelIn in{};
    in.BM = s.BM;
    in.BN = s.BN;
    for (int g = 0; g < GC_G_COUNT; ++g) {
        in.g_BN[g] = s.geom[g].BN;
        in.g_Wp[g] = s.geom[g].Wp;
    }
    in.flat_uw = s.flat_uw;
    in.tail_split = s.tail_split;
    in.qt2_nrows = s.qt2_nrows;
    in.qt2_qoff = s.qt2_qoff;
    in.CI_C = s.CI_C;
    in.nrows = s.nrows;
    in.KCp = s.KCp;
    in.causal = s.causal;
    in.pl_C0 = in.C0 = Cin;
    in.pl_epi = in.epi = epi;
    in.Z = Z;
    in.B = B;
    in.Q = Q;
    in.M = M;
    in.n_mtiles = (M + s.BM - 1) / s.BM;
    in.Tout = in.Tin = T;
    in.Fin = Q * si + 4;
    in.si = si;
    in.s0_f = T;
    in.s0_c = (long)in.Fin * T;
    in.s0_b = in.s0_c * Cin;
    in.desc4 = 1;
    in.overread0 = in.overread1 = T % 4 != 0;
    return in;
}

static bool refused(const GCSelIn& in, const char* word) {
    try {
        (void)gc_select(in);
    } catch (const Error& e) {
        if (std::strstr(e.what(), word)) return true;
        std::printf("refused with \"%s\", expected \"%s\"\n", e.what(), word);
        return false;
    }
    std::printf("not refused, expected \"%s\"\n", word);
    return false;
}

int main() {
    const TapSpec t31 = taps_of(3, 1, 0, 0), t32 = taps_of(3, 2, 0, 1), t52 = taps_of(5, 2, 2, 1), pw = taps_of(1, 1, 0, 0);
    {   // plan shapes: a U^2-Net level (64-row tiles, every geometry but the 32-column one), DCCRN's encoder (128-row tiles)
        const GCPlanShape a = gc_plan_shape(64, 64, t31, EPI_ACT, 2, 401, 1, -1);
        EXPECT(a.BM == 64 && a.BN == 128 && a.flat_uw == 32 && a.causal && a.geom[GC_G_N32].BN == 0);
        EXPECT(a.geom[GC_G_N64].BN == 64 && a.geom[GC_G_N256].BN == 256 && a.geom[GC_G_FLAT128].Wp == 128 && a.geom[GC_G_FLAT256].Wp == 256);
        const GCPlanShape b = gc_plan_shape(128, 64, t52, EPI_ACT, 2, 401, 1, -1);
        EXPECT(b.BM == 128 && b.geom[GC_G_N32].BN == 32 && b.geom[GC_G_N32].Wp == 36 && b.tail_split && b.flat_uw == 0);
        EXPECT(b.lookback == 1 && b.dtmin == -4 && b.geom[GC_G_MAIN].Wp == 132 && b.KCp % 4 == 0);
        EXPECT(b.geom[GC_G_QT2].BN == 64 && b.qt2_nrows == 7 && b.qt2_qoff == 2 * b.geom[GC_G_QT2].Wp);
    }
    {   // edge-row classes of the (5, 2) conv, stride 2, pad 2: two one-row classes from 4 output rows on, none for one row
        const GCEdgeShape e = gc_edge_classes(t52, 2, 2, 8, 4);
        EXPECT(e.nclass == 2 && e.cls_lo == 1 && e.cls_hi == 2 && e.dead[0] == 0x00fu && e.dead[1] == 0x300u);
        EXPECT(e.KC[0] == 12 && e.KCp[0] == 12 && e.KC[1] == 16 && e.KCp[1] == 16 && e.live[0][0] == 4 && e.live[0][6] == 14 && e.live[1][8] == 10);
        EXPECT(gc_edge_classes(t52, 2, 2, 2, 1).nclass == 0 && gc_edge_classes(t52, 2, 2, 4, 2).nclass == 2);
        EXPECT(gc_edge_classes(pw, 8, 1, 4, 4).nclass == 0);
    }
    {   // thin: one frame of a stream, before the preamble (t_base > 0) and after it
        GCSelIn in = launch_of(64, 64, t32, EPI_ACT, 2, 1, 39, 9);
        in.t_base = 8;
        GCChoice c = gc_select(in);
        EXPECT(c.main.family == GC_FAM_THIN && c.main.early && c.main.thin_n == 1 && c.main.nblk == 8 * 39 && !c.has_tail);
        in = launch_of(64, 64, t32, EPI_ACT, 2, 1, 39, 4);
        c = gc_select(in);
        EXPECT(c.main.family == GC_FAM_THIN && !c.main.early && c.main.thin_n == 4 && c.main.pw4 == 1);
        EXPECT(gc_thin_blocks(in, 0) == c.main.nblk);
    }
    {   // direct: plain below 1 024 eight-row workgroups, LDS-tiled from there on
        GCSelIn in = launch_of(2, 32, taps_of(3, 2, 1, 1), EPI_ACT, 1, 4, 64, 401);
        in.Ws = in.pl_Ws = 1;
        in.sm_dfmin = -1, in.sm_dfmax = 1, in.sm_dtmin = -1, in.sm_dtmax = 0;
        GCChoice c = gc_select(in);
        EXPECT(c.main.family == GC_FAM_DIRECT && c.main.nblk == 2L * 64 * 4);
        in.B = 64;
        c = gc_select(in);
        EXPECT(c.main.family == GC_FAM_DIRECT_LDS && c.main.nblk == 2L * 8 * 64 && c.main.NR == 10 && c.main.CC == 2);
        EXPECT(c.main.lds == (size_t)2 * 10 * GC_SMALL_WT * 4);
        in.fz = 1;
        EXPECT(refused(in, "direct (<= 4 channel) path cannot fold"));
    }
    {   // 64-row layer by launch size: 64 x 64 (resident-K on a few frames), flattened narrow / wide, 64 x 256, the plan's own tile
        GCSelIn in = launch_of(64, 64, t31, EPI_ACT, 2, 2, 39, 101);
        GCChoice c = gc_select(in);
        EXPECT(c.main.geom == GC_G_N64 && c.main.BM == 64 && c.main.BN == 64 && c.main.WM == 2 && c.main.form == GC_FORM_PLAIN);
        EXPECT(c.main.n_ttiles == 2 && c.main.nblk == 2L * 39 * 2);
        in = launch_of(64, 64, t31, EPI_ACT, 2, 4, 39, 16);       // (more than GC_THIN_NT frames: not thin)
        c = gc_select(in);
        EXPECT(c.main.form == GC_FORM_RES && c.main.nbuf > 2 && c.main.BN == 64 && c.main.lds <= 158 * 1024);
        in = launch_of(64, 64, t31, EPI_ACT, 2, 30, 39, 61);         // 1 170 workgroups: below alt_n64 -> still 64 columns
        EXPECT(gc_select(in).main.BN == 64);
        in.tun.alt_n64 = 1024;                                          // narrow flattened tiles: 2 units per row, 4 per tile
        c = gc_select(in);
        EXPECT(c.main.geom == GC_G_FLAT128 && c.main.form == GC_FORM_FLAT32 && c.main.flat_upr == 2 && c.main.flat_units == 60 && c.main.n_ttiles == 15);
        EXPECT(c.main.nblk == 39L * 15);
        in = launch_of(64, 64, t31, EPI_ACT, 2, 160, 39, 125);        // wide: 4 units per row, 8 per tile
        in.nrm0 = 1;
        c = gc_select(in);
        EXPECT(c.main.geom == GC_G_FLAT256 && c.main.form == GC_FORM_FLAT32_NRM && c.main.BN == 256 && c.main.WM == 1 && c.main.n_ttiles == 80);
        in = launch_of(64, 64, t31, EPI_ACT, 2, 160, 39, 93);         // 3 units per row: a normalising wide tile would span 4 rows
        in.nrm0 = 1;
        c = gc_select(in);
        EXPECT(c.main.flat_upr == 0 && c.main.flat_nrm_refused == gc_flat_rows_spanned(160, 3, 8) && c.main.flat_nrm_refused == 4);
        EXPECT(c.main.geom == GC_G_MAIN && c.main.form == GC_FORM_NRM && c.main.BN == 128);
        in = launch_of(64, 64, t31, EPI_ACT, 2, 80, 39, 256);         // rows that fill the wide tiles
        c = gc_select(in);
        EXPECT(c.main.geom == GC_G_N256 && c.main.BN == 256 && c.main.flat_upr == 0 && c.main.n_ttiles == 1 && c.main.nblk == 80L * 39);
        in.tun.flat = 0;
        in.tun.wide_min = in.tun.qt2_min = 1 << 20;                     // neither wide nor two-row tiles: the plan's own
        c = gc_select(in);
        EXPECT(c.main.geom == GC_G_MAIN && c.main.BM == 64 && c.main.BN == 128 && c.main.n_ttiles == 2 && !c.has_tail);
    }
    {   // 128-row layer: 32-column tiny launch, 128 x 64, two-row tiles, the tail split (tail first) and trimming
        GCSelIn in = launch_of(128, 64, t52, EPI_ACT, 2, 1, 32, 101);
        GCChoice c = gc_select(in);
        EXPECT(c.main.geom == GC_G_N32 && c.main.BM == 128 && c.main.BN == 32 && c.main.WM == 4 && c.main.n_ttiles == 4);
        in.g_BN[GC_G_N32] = 0;      // (a plan with both narrow geometries never gets here: 64-column tiles at most double the count)
        c = gc_select(in);
        in.g_BN[GC_G_N32] = 32;
        EXPECT(c.main.geom == GC_G_N64 && c.main.BM == 128 && c.main.BN == 64 && c.main.form == GC_FORM_PLAIN);
        in.B = 128;
        in.Tout = in.Tin = 401;
        in.overread0 = in.overread1 = 1;
        c = gc_select(in);
        EXPECT(c.main.geom == GC_G_QT2 && c.main.qt2 == 1 && c.main.Qt == 16 && c.main.nrows == in.qt2_nrows && c.main.n_ttiles == 7);
        in.edge = 1;    // a plan with edge-row classes declines the two-row rung: its own one-row tiles (and the tail split)
        c = gc_select(in);
        EXPECT(c.main.geom == GC_G_MAIN && c.main.qt2 == 0 && c.main.Qt == 32 && c.main.BN == 128 && c.main.form == GC_FORM_PLAIN);
        EXPECT(c.main.n_ttiles == 3 && c.has_tail && c.tail.geom == GC_G_N32 && c.tail.qt2 == 0);
        in.edge = 0;
        in.B = 8;       // 1 024 workgroups: below qt2_min -> three full tiles and the 17-frame tail on 32 columns
        c = gc_select(in);
        EXPECT(c.has_tail && c.tail.geom == GC_G_N32 && c.tail.t_base == 384 && c.tail.n_ttiles == 1 && c.tail.nblk == 8L * 32);
        EXPECT(c.main.geom == GC_G_MAIN && c.main.n_ttiles == 3 && c.main.t_base == 0 && c.main.nblk == 8L * 32 * 3);
        GCSelIn la = launch_of(128, 64, taps_of(3, 3, 1, 1), EPI_ACT, 1, 64, 64, 401);        // a tap looks ahead
        c = gc_select(la);
        EXPECT(!la.causal && c.main.trim == 1 && c.main.pw4 == 1 && c.main.form == GC_FORM_TRIM);
        la.overread0 = 0;       // source outside the arena: single-frame staging
        c = gc_select(la);
        EXPECT(c.main.trim == 0 && c.main.pw4 == 0 && c.main.form == GC_FORM_PLAIN);
    }
    {   // the per-step LSTM GEMM: 128 x 256 from 1 536 workgroups on; h_{-1} = 0 drops the source
        GCSelIn in = launch_of(1024, 256, pw, EPI_LSTM, 1, 4, 1, 512 * 100);
        GCChoice c = gc_select(in);
        EXPECT(c.main.geom == GC_G_N256 && c.main.BM == 128 && c.main.BN == 256 && c.main.WM == 2 && c.main.WN == 2);
        in.first_step = 1;
        EXPECT(gc_select(in).main.C0 == 0);
    }
    // refusals
    GCSelIn in = launch_of(64, 64, t31, EPI_ACT, 2, 80, 39, 256);
    GCSelIn r = in;
    r.C0 = 32;
    EXPECT(refused(r, "source channel split differs from the plan"));
    r = in, r.dst_elu = 1;
    EXPECT(refused(r, "second (ELU) store belongs to the gated epilogue"));
    r = in, r.t_base = 6;
    EXPECT(refused(r, "first output frame must be a multiple of 4 below Tout"));
    r = in, r.t_base = 8, r.stats = 1;
    EXPECT(refused(r, "statistics epilogue needs whole rows"));
    r = in, r.s0_f = 1L << 40;
    EXPECT(refused(r, "source plane too large for 32-bit patch byte offsets"));
    r = in, r.cstats = 1, r.n_mtiles = 2;
    EXPECT(refused(r, "column statistics need a statistics tile configuration and one m-tile (M 64, BM 64, m-tiles 2, epilogue 0, direct 0)"));
    r = in, r.fz = 1, r.stats = 1;
    EXPECT(refused(r, "no trimming / statistics variant of the kernel with the folded interaction"));
    r = in, r.epi = r.pl_epi = EPI_GLU, r.fz = 1;
    EXPECT(refused(r, "cannot fold the branch interaction into its store"));
    r = in, r.epi = r.pl_epi = EPI_GLU, r.nrm0 = 1;
    EXPECT(refused(r, "this kernel variant cannot normalise its sources on the fly"));
    r = in, r.nrm0 = 1, r.causal = 0;
    EXPECT(refused(r, "on-the-fly InstanceNorm needs causal taps, one-row tiles and <= 128 input channels"));
    r = in, r.epi = r.pl_epi = 9;
    EXPECT(refused(r, "unknown epilogue"));
    r = in, r.B = 1 << 20, r.Q = 1 << 12;
    EXPECT(refused(r, "grid size"));
    r = launch_of(128, 64, t52, EPI_ACT, 2, 8, 32, 401), r.stats = 1;
    EXPECT(refused(r, "this tile configuration has no statistics epilogue"));
    r = launch_of(32, 32, t31, EPI_CMB, 2, 80, 39, 256);
    EXPECT(refused(r, "no resident-K / 32-row form of the combine epilogue"));
    r = launch_of(256, 64, pw, EPI_ACT, 1, 64, 4, 401), r.overread0 = 0;
    EXPECT(refused(r, "needs its sources inside the engine arena"));
    {
        TapSpec bad = pw;
        bad.ntaps = 17;
        bool thrown = false;
        try {
            (void)gc_plan_shape(64, 64, bad, EPI_ACT, 1, 401, 1, -1);
        } catch (const Error& e) {
            thrown = std::strstr(e.what(), "tap count") != nullptr;
        }
        EXPECT(thrown);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}

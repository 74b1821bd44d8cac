// Tile selection of the tap-table conv (gemmconv.hip) as pure host functions: what a layer's plan is (gc_plan_shape) and which
// kernel form one launch takes (gc_select).  Plain C++17 without a HIP header, so that both compile and are tested on a CPU
// (tests/gc_select_check.cpp, tests/gc_select_probe.cpp).  gc_make_plan builds the device tables a GCPlanShape lists; gc_launch
// fills a GCSelIn, applies the GCChoice to the kernel's arguments and dispatches it.  A new tile is added here: its geometry in
// gc_plan_shape, its rung in gc_select, and its instantiation in gemmconv.hip's gc_has_variant.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include "se_check.h"

namespace se {

constexpr int GC_MAX_TAPS = 16;
constexpr int GC_MAX_ROWS = 8;
constexpr int GC_MAX_KCP = 48;
constexpr int GC_TAB_KOFF = GC_MAX_ROWS + 2 * GC_MAX_TAPS;   // start of the per-K-row patch offsets in GCParams::tab
// K rows of one staged chunk and patch elements staged per thread, by output-channel tile
constexpr int gc_kcp_max(int BM) { return 32; }
constexpr int gc_bld_max(int BM) { return (BM >= 128 || BM <= 32) ? 9 : 13; }

enum Epi : int {
    EPI_ACT = 0,     // dst = act(acc + bias)
    EPI_LSTM = 1,    // rows are gate-interleaved (4j+{i,f,g,o}); dst = h_t, c updated in place (GCParams::gru: the GRU cell on the same 4-row layout)
    EPI_GLU = 2,     // rows are pair-interleaved (2j, 2j+1): dst[j] = (a+bias) * sigmoid(g+bias)
    EPI_ADD = 3,     // dst = act(acc + bias) + res   (res laid out like dst)
    EPI_MUL = 4,     // dst = act(acc + bias) * aux   (gated TCM branches, CTSNet/Step1_network.py:184)
    EPI_CMB = 5,     // dst = prelu((aux +- acc) * post_scale + post_shift): the last two of Gauss' three products finish the complex
                     // layer in their own store (aux = k1; GCParams::cmb_neg bit z: minus; per-z rows of post_scale / post_shift /
                     // slope at stride ps_z) - gauss.h
};

// launches that produce at most this many frames per row go to the thin kernel (frame-online chunks)
constexpr int GC_THIN_NT = 8;
// most workgroups a launch may have on the thin path
constexpr long GC_THIN_MAX_BLOCKS = 8192;
constexpr int GC_NRM_MAXC = 128;
// batch rows whose InstanceNorm parameters a flattened tile with NRM holds in LDS (gc_kernel: nrmC / nrmK); gc_select only
// sends a normalising launch to the flattened tiles when no tile spans more rows than this
constexpr int GC_FLAT_NRM_ROWS = 2;
// direct (<= 4 output channels) kernel in its LDS-tiled form: output rows per workgroup, LDS row stride of its patch
constexpr int GC_SMALL_QB = 8, GC_SMALL_WT = 264;

struct TapSpec {
    int ntaps = 0;
    int df[GC_MAX_TAPS];
    int dt[GC_MAX_TAPS];
};

enum GCFamily : int { GC_FAM_TILE = 0, GC_FAM_THIN = 1, GC_FAM_THIN_PAIR = 2, GC_FAM_DIRECT = 3, GC_FAM_DIRECT_LDS = 4 };

// Patch geometries of a plan (BN = 0: the plan does not have it)
enum GCGeomId : int {
    GC_G_MAIN = 0,   // the plan's own tile
    GC_G_N32,        // 32 columns: a mostly empty last time tile of a row (own launch), tiny launches of a 128-row layer
    GC_G_N64,        // 64 columns: the whole layer, for launches that would not fill the chip with 128-column tiles
    GC_G_N256,       // 256 columns: big launches of a 64-row layer / of the per-step LSTM GEMM
    GC_G_QT2,        // two-row tiles: 2 output rows x 64 frames, patch rows = union of both rows' input rows
    GC_G_FLAT128,    // unit-flattened (GCParams::flat_upr), 4 units of flat_uw columns
    GC_G_FLAT256,    // unit-flattened, 8 units
    GC_G_COUNT
};

// Environment switches of the ladder, each read once per process (gc_tuning_env)
struct GCTuning {
    int alt_n64 = 4096;      // SE_GC_ALT_N64: 128-column workgroup count below which a 64-row layer uses 64-column tiles
    long wide_min = 6144;    // SE_GC_WIDE_MIN: 128-column workgroup count from which a 64-row layer uses 256-column tiles
    int wide_fill = 75;      // SE_GC_WIDE_FILL: least fill of the plain wide tiles in percent
    long qt2_min = 4096;     // SE_GC_QT2_MIN: workgroup count from which two-row tiles are used
    int flat = 1;            // SE_GC_FLAT: 0 = no unit-flattened tiles (neither their geometries in gc_plan_shape)
    int dbg = 0;             // SE_GC_DBG: GCParams::dbg
};
inline const GCTuning& gc_tuning_env() {
    static const GCTuning t = [] {
        GCTuning v;
        v.alt_n64 = getenv("SE_GC_ALT_N64") ? atoi(getenv("SE_GC_ALT_N64")) : v.alt_n64;
        if (getenv("SE_GC_WIDE_MIN")) v.wide_min = atol(getenv("SE_GC_WIDE_MIN"));
        v.wide_fill = getenv("SE_GC_WIDE_FILL") ? atoi(getenv("SE_GC_WIDE_FILL")) : v.wide_fill;
        if (getenv("SE_GC_QT2_MIN")) v.qt2_min = atol(getenv("SE_GC_QT2_MIN"));
        v.flat = getenv("SE_GC_FLAT") ? atoi(getenv("SE_GC_FLAT")) : v.flat;
        v.dbg = getenv("SE_GC_DBG") ? atoi(getenv("SE_GC_DBG")) : v.dbg;
        return v;
    }();
    return t;
}

// ------------------------------------------------------------------------------------------------ plan shape
struct GCGeomShape {
    int BN = 0, Wp = 0;          // tile columns, LDS row stride of the patch
    int nrows = 0;               // patch rows per input channel
    int rows[GC_MAX_ROWS] = {};  // their frequency offsets, ascending
};
// What a layer gets, decided from its shape alone (no device work)
struct GCPlanShape {
    int BM = 128, BN = 128;
    int C0 = 0;
    int nrows = 0, dtmin = 0, causal = 0, lookback = 0;
    int CI_C = 1, KC = 0, KCp = 0;
    GCGeomShape geom[GC_G_COUNT];
    bool tail_split = false;     // GC_G_N32 may be used as a separate launch for the last time tile
    int flat_uw = 0;             // LDS columns per flattened unit and patch row: 32 (pointwise) or 36 (<= 4 frames of look-back)
    int qt2_nrows = 0, qt2_qoff = 0;
};

inline GCPlanShape gc_plan_shape(int M, int Cin, const TapSpec& taps, int epi, int si, int tout_hint, int Z, int C0split) {
    SE_CHECK(taps.ntaps >= 1 && taps.ntaps <= GC_MAX_TAPS, "tap count");
    GCPlanShape s;
    const int C0 = s.C0 = (C0split < 0 || C0split > Cin) ? Cin : C0split;
    s.BM = M >= 96 ? 128 : (M >= 48 ? 64 : 32);
    {   // memory-bound pointwise layers (<= 128 input channels, <= 384 rows: Uformer's conformer, the TCM blocks' 64 -> 256 layers) on
        // 64-row tiles: twice the workgroups in flight, each small enough to spread its DMAs over the matrix loop
        // (SE_GC_PW_BM64=k: input-channel limit, 0 = 128-row tiles; Uformer + 1.1 %, the others unchanged)
        static const int pw64 = getenv("SE_GC_PW_BM64") ? atoi(getenv("SE_GC_PW_BM64")) : 128;
        if (pw64 > 0 && taps.ntaps == 1 && Cin <= pw64 && M >= 96 && M <= 384 && epi != EPI_LSTM) s.BM = 64;
    }
    s.BN = (tout_hint >= 96 || s.BM == 32) ? 128 : 64;
    // distinct rows / dt span
    int dtmin = taps.dt[0], dtmax = taps.dt[0];
    int rows[GC_MAX_TAPS], nr = 0;
    for (int j = 0; j < taps.ntaps; ++j) {
        dtmin = std::min(dtmin, taps.dt[j]);
        dtmax = std::max(dtmax, taps.dt[j]);
        if (std::find(rows, rows + nr, taps.df[j]) == rows + nr) rows[nr++] = taps.df[j];
        // (the thin kernel reads the taps from its arguments, as shorts)
        SE_CHECK(taps.df[j] >= -32768 && taps.df[j] <= 32767 && taps.dt[j] >= -32768 && taps.dt[j] <= 32767, "tap offset range");
    }
    std::sort(rows, rows + nr);
    SE_CHECK(nr <= GC_MAX_ROWS, "too many distinct frequency rows");
    s.nrows = nr;
    // patch geometry: the staged time window starts a multiple of 4 frames before the tile (origin t0 - pad4) so that it
    // decomposes into 16 B groups that never straddle frame 0 (t0 is a multiple of BN): LDS column w <-> frame t0 + dtmin + w
    s.causal = dtmax <= 0;
    s.lookback = std::max(-dtmin, 0);                      // frames of history the taps reach back (frame-online mode)
    dtmin = -((std::max(-dtmin, 0) + 3) & ~3);
    dtmax = (std::max(dtmax, 0) + 3) & ~3;
    s.dtmin = dtmin;
    const int halo = dtmax - dtmin;
    const int Wp = s.BN + halo;                            // LDS row stride of the patch (multiple of 4)
    SE_CHECK(nr * Wp <= gc_bld_max(s.BM) * 256, "tap span too wide for one staged patch");
    // chunk = CI_C input channels x all taps.  Among the sizes that fit the staging budgets take the one that wastes the
    // fewest K rows on padding to a multiple of 4 (rows of zeros cost full MFMAs), then the largest: measured on the DCCRN
    // bench, 20 exact rows per barrier beat 30 rows padded to 32 (taps = 10), 24 beat 30 / 32 (taps = 6)
    int cic = 1;
    double best = -1.0;
    for (int c = 1; c <= std::max(std::max(C0, Cin - C0), 1); ++c) {
        const int kc = c * taps.ntaps, kcp = (kc + 3) & ~3;
        // pointwise layers stage 16 B groups (4x the slots) and size the chunk by the LDS budget of 3 blocks per CU
        const bool pw = taps.ntaps == 1;
        const int kmax = pw ? (s.BM >= 128 ? 24 : 32) : gc_kcp_max(s.BM);
        const int cap = gc_bld_max(s.BM) * 256 * (pw ? 4 : 1);
        if (kcp > kmax || c * nr * Wp > cap) continue;
        // 64-row layers: keep the chunk small enough for the 64 x 256 tile's patch (3 workgroups per CU) when that still
        // leaves >= 12 K rows per barrier - G2Net's 3-tap convs would stage 8 channels x 3 rows and fall back to 64 x 128
        // tiles (measured: + 4 % for the whole model at batch 256 with 4-channel chunks)
        if (s.BM == 64 && s.BN == 128 && taps.ntaps > 1 && epi != EPI_LSTM && kc > 12 && (long)c * nr * (256 + halo) > 4608) continue;
        const double score = (double)kc / kcp + 1e-4 * kc;       // padding efficiency first, size second
        if (score > best) {
            best = score;
            cic = c;
        }
    }
    s.CI_C = cic;
    s.KC = cic * taps.ntaps;
    s.KCp = (s.KC + 3) & ~3;
    SE_CHECK(s.KCp <= gc_kcp_max(s.BM), "single-channel chunk exceeds K budget");
    const int nbk = gc_bld_max(s.BM);
    auto add = [&](int id, int BN, int wp, const int* rr, int n) {
        GCGeomShape& g = s.geom[id];
        g.BN = BN;
        g.Wp = wp;
        g.nrows = n;
        std::copy(rr, rr + n, g.rows);
    };
    add(GC_G_MAIN, s.BN, Wp, rows, nr);
    // narrower geometries for the last, mostly empty time tile of a row (T = 401 fills 17 of 128 columns of its 4th
    // tile): same weights and chunking, own patch tables; gc_select sends that tile to a 32-column kernel
    // (only where the narrow kernel keeps all four waves busy: 128 rows x 32 columns; a 64-row layer would leave half
    // its waves on padding again - measured slower than the skip logic of the full-width tile)
    // (pointwise layers get the geometry for tiny launches only: as a separate tail launch it doubled the launch count
    // of FullSubNet's per-step LSTM GEMMs)
    s.tail_split = taps.ntaps != 1;
    if (s.BN == 128 && s.BM == 128) add(GC_G_N32, 32, 32 + halo, rows, nr);
    // two-row geometry (gc_kernel: qt2): rows of the patch = union of the input rows of two neighbouring output rows,
    // when that union is an interval and smaller than twice the single-row set
    if (s.BN == 128 && epi != EPI_LSTM && taps.ntaps > 1) {
        int r2[2 * GC_MAX_ROWS], n2 = nr;
        std::copy(rows, rows + nr, r2);
        for (int i = 0; i < nr; ++i)
            if (std::find(r2, r2 + n2, rows[i] + si) == r2 + n2) r2[n2++] = rows[i] + si;
        std::sort(r2, r2 + n2);
        const bool interval = r2[n2 - 1] - r2[0] + 1 == n2;
        const int wp2 = 64 + halo;
        if (interval && n2 <= GC_MAX_ROWS && n2 < 2 * nr && cic * n2 * wp2 <= nbk * 256) {
            add(GC_G_QT2, 64, wp2, r2, n2);
            s.qt2_nrows = n2;
            s.qt2_qoff = si * wp2;
        }
    }
    // 256-column geometry of a 64-row layer: 1 x 4 waves of 64 x 64 do the 128 x 128 tile's matrix work per
    // staged K row (the 64 x 128 tile does half of it), for big launches whose rows fill the wide tiles (T = 501: 98 %)
    if (s.BN == 128 && s.BM == 64 && epi != EPI_LSTM && taps.ntaps > 1) add(GC_G_N256, 256, 256 + halo, rows, nr);
    // 256-column geometry of the per-step LSTM GEMM (FullSubNet's sub-band layers): 2 x 2 waves of 64 x 128 -
    // a staged K row feeds twice the matrix work of the 128 x 128 tile and a weight chunk is fetched once per 256 columns.
    // Measured in round 4 on every 128-row pointwise layer: + 1.7 % on FullSubNet (two streams of step launches fill each
    // other's tails), 1 - 8 % SLOWER on the LSTM input projections, DPCRN's and the conformer's pointwise layers (two
    // workgroups per CU instead of three, coarser tails; with loads and epilogue ablated both tiles run the same
    // 132 - 134 TFLOP/s, so the K loop itself gains nothing) - hence only here
    static const int wide128_env = getenv("SE_GC_WIDE128") ? atoi(getenv("SE_GC_WIDE128")) : 1;
    if (wide128_env && s.BN == 128 && s.BM == 128 && taps.ntaps == 1 && epi == EPI_LSTM && cic * 256 <= 6 * 1024)
        add(GC_G_N256, 256, 256, rows, nr);
    // unit-flattened geometries (GCParams::flat_upr): every 32-frame unit of the tile with its own halo
    if (gc_tuning_env().flat && s.BM == 64 && s.BN == 128 && epi != EPI_LSTM && s.causal && dtmin >= -4 && Z == 1) {
        const int uw = s.flat_uw = 32 - dtmin;      // 32 or 36
        if ((long)cic * nr * 4 * uw <= (long)nbk * 256 * 4) add(GC_G_FLAT128, 128, 4 * uw, rows, nr);
        // (5 x 256 groups, 3 workgroups' LDS - as the plain 64 x 256 tile)
        if ((long)cic * nr * 8 * uw <= 4608) add(GC_G_FLAT256, 256, 8 * uw, rows, nr);
    }
    // 64-column geometry of the whole layer for launches that would not fill the chip with 128-column tiles: the batch is
    // only known at launch time, gc_select picks
    if (s.BN == 128 && (s.BM == 64 || s.BM == 128) && epi != EPI_LSTM) add(GC_G_N64, 64, 64 + halo, rows, nr);
    return s;
}

// ------------------------------------------------------------------------------------------------ edge-row classes
// Output rows whose frequency taps partly lie outside the input plane multiply those taps against the zeros of the padding.  A
// plan that opts in (gc_make_plan: edge_Fin / edge_Q) gives such rows K tables and packed weights of their own that list the
// live K rows only.  Rows with the same dead taps form a class; class 0 has nothing dead.  The kernel's row-to-class rule is
// "row 0, row Q - 1, everything else", so classes are built only when every other row is whole, and at most GC_EDGE_MAX of them.
constexpr int GC_EDGE_MAX = 2;
struct GCEdgeShape {
    int nclass = 0;                           // further classes built (0: the plan behaves as one without)
    int cls_lo = 0, cls_hi = 0;               // class of output row 0 / of row Q - 1
    int Fin = 0, Q = 0;                       // the plane the classes hold for
    unsigned dead[GC_EDGE_MAX] = {};          // bit j: tap j of the class lies outside the plane
    int KC[GC_EDGE_MAX] = {};                 // live K rows of a full chunk
    int KCp[GC_EDGE_MAX] = {};                // ... padded to the K loop's group of two k-pairs
    int live[GC_EDGE_MAX][GC_MAX_KCP] = {};   // class-0 K row (cil * ntaps + j) of surviving row i, ascending
};
// cic: input channels per staged chunk; si: input rows per output row; output row q reads input rows q si + df[j]
inline GCEdgeShape gc_edge_classes(const TapSpec& taps, int cic, int si, int Fin, int Q) {
    GCEdgeShape e;
    if (Fin <= 0 || Q < 2 || taps.ntaps > 31 || cic * taps.ntaps > GC_MAX_KCP) return e;      // (a one-row plane: its row is both edges)
    auto dead_of = [&](int q) {
        unsigned d = 0;
        for (int j = 0; j < taps.ntaps; ++j) {
            const int f = q * si + taps.df[j];
            if (f < 0 || f >= Fin) d |= 1u << j;
        }
        return d;
    };
    for (int q = 1; q + 1 < Q; ++q)
        if (dead_of(q)) return e;              // an inner row with dead taps would need a class the row rule cannot name
    const unsigned all = (1u << taps.ntaps) - 1u, dl = dead_of(0), dh = dead_of(Q - 1);
    if (dl == all || dh == all) return e;
    int n = 0, lo = 0, hi = 0;
    unsigned dd[GC_EDGE_MAX] = {};
    if (dl) {
        dd[n] = dl;
        lo = ++n;
    }
    if (dh) {
        if (dh == dl) hi = lo;
        else {
            dd[n] = dh;
            hi = ++n;
        }
    }
    if (n == 0) return e;
    e.nclass = n;
    e.cls_lo = lo;
    e.cls_hi = hi;
    e.Fin = Fin;
    e.Q = Q;
    for (int c = 0; c < n; ++c) {
        e.dead[c] = dd[c];
        int k = 0;
        for (int cil = 0; cil < cic; ++cil)
            for (int j = 0; j < taps.ntaps; ++j)
                if (!((dd[c] >> j) & 1u)) e.live[c][k++] = cil * taps.ntaps + j;
        e.KC[c] = k;
        e.KCp[c] = (k + 3) & ~3;
    }
    return e;
}

// ------------------------------------------------------------------------------------------------ launch selection
// Everything the ladder reads of a plan and of one launch.  No addresses: a pointer of GCParams is its presence flag here, so
// the same launch gives the same bytes on every run (tests/golden/gc_select_parent.jsonl.gz; as integers: tests/gc_selin_flat.h).
struct GCSelIn {
    // the plan
    int BM, BN;
    int g_BN[GC_G_COUNT], g_Wp[GC_G_COUNT];
    int flat_uw, tail_split, qt2_nrows, qt2_qoff;
    int CI_C, nrows, KCp, causal;
    int sm_dfmin, sm_dfmax, sm_dtmin, sm_dtmax;      // direct path: tap extents
    int pl_C0, pl_C1, pl_epi, pl_Ws;
    // the launch
    int epi, Z, B, Q, M, n_mtiles, Tout, Tin, Fin, t_base, tb_soft, C0, C1, pad_lo, first_step, pair, si;
    long s0_b, s0_c, s0_f, s1_b, s1_c, s1_f;
    int Ws, desc4, stats, cstats, nrm0, nrm1, fz, dst_elu, tlen;
    int overread0, overread1;    // gc_overread_ok(src0), gc_overread_ok(src1)
    GCTuning tun;
    // the plan has edge-row classes this launch can use (GCEdgeShape; gc_launch).  Behind `tun` and outside the flat form of
    // tests/gc_selin_flat.h: a recorded launch has none
    int edge;
};
// kernel variant of a tile launch (template arguments RES / TRIM / FZ / NRM / FLATW of gc_kernel)
enum GCForm : int {
    GC_FORM_PLAIN = 0,
    GC_FORM_RES,         // all chunks of a source resident in LDS
    GC_FORM_TRIM,        // 16 B groups that straddle the end of a row are cut back in LDS
    GC_FORM_FZ,          // branch interaction folded into the store
    GC_FORM_NRM,         // sources normalised on the fly
    GC_FORM_FLAT32, GC_FORM_FLAT36, GC_FORM_FLAT32_NRM, GC_FORM_FLAT36_NRM
};

// One dispatch: the kernel and the per-launch values of its arguments
struct GCDispatch {
    int family = GC_FAM_TILE;
    int geom = GC_G_MAIN;
    int BM = 0, BN = 0, WM = 0, WN = 0, form = GC_FORM_PLAIN;       // GC_FAM_TILE
    bool early = false;      // thin launch taken before the preamble: only C0 is applied to the arguments
    int n_ttiles = 0, Qt = 0, qt2 = 0, qq_off = 0, nrows = 0, pw4 = 0, trim = 0, nbuf = 0, t_base = 0, flat_upr = 0, flat_units = 0;
    int C0 = 0;              // after the first_step rule
    int dbg = 0;
    int thin_n = 0;          // GC_FAM_THIN: frames per row
    int CC = 0, NR = 0;      // GC_FAM_DIRECT_LDS: channels per staged chunk, patch rows
    long nblk = 0;
    size_t lds = 0;
    int flat_nrm_refused = 0;
};
struct GCChoice {
    GCDispatch main;
    bool has_tail = false;   // the last time tile as its own launch, dispatched BEFORE main
    GCDispatch tail;
};

// most batch rows that one flattened tile of `upt` units touches when B rows of `upr` units each are laid end to end
inline int gc_flat_rows_spanned(int B, int upr, int upt) {
    // tile k covers units [k upt, (k + 1) upt); tile k + upr starts exactly upt rows further on, so the first upr tiles show
    // every pattern (a shortened last tile spans no more rows than the full one of its pattern)
    const long units = (long)B * upr, tiles = (units + upt - 1) / upt;
    int most = 0;
    for (long k = 0; k < std::min<long>(tiles, upr); ++k) {
        const long u0 = k * upt, u1 = std::min(u0 + upt, units) - 1;
        most = std::max(most, (int)(u1 / upr - u0 / upr + 1));
    }
    return most;
}

// Geometry of one dispatch, for tests that must know which kernel form a launch reached (gc_set_launch_log;
// csrc/tests/gc_probe.hip, gc_select_probe.cpp).  Host-side only: nothing the kernels compute depends on it.
struct GCLaunchRec {
    int family = GC_FAM_TILE;
    int BM = 0, BN = 0;          // tile (GC_FAM_TILE)
    int flat_upr = 0, upt = 0;   // flattened column tiles: units per batch row, units per tile (0: plain tiles)
    int flat_rows = 0;           // flattened: most batch rows one tile spans
    int qt2 = 0, nrm = 0, res = 0, trim = 0, stats = 0, ragged = 0;
    int flat_nrm_refused = 0;    // the flattened tiles were considered and refused because a normalising tile would span
                                 // more than GC_FLAT_NRM_ROWS rows (value: rows spanned)
    long nblk = 0;               // workgroups
    int epi = 0, gru = 0;        // the launch's epilogue (EPI_LSTM: one recurrent step; gru: its GRU cell)
    int form = GC_FORM_PLAIN;    // GCForm of a GC_FAM_TILE dispatch
    int Z = 1;                   // grouped launches: products per dispatch (blockIdx.z)
};
inline GCLaunchRec gc_launch_rec(const GCSelIn& in, const GCDispatch& d, int gru) {
    GCLaunchRec r;
    r.family = d.family;
    r.BM = d.BM;
    r.BN = d.BN;
    r.flat_upr = d.flat_upr;
    r.upt = d.flat_upr ? d.BN / 32 : 0;
    r.flat_rows = d.flat_upr ? gc_flat_rows_spanned(in.B, d.flat_upr, d.BN / 32) : 0;
    r.qt2 = d.qt2;
    r.nrm = (in.nrm0 || in.nrm1) ? 1 : 0;
    r.res = d.form == GC_FORM_RES ? 1 : 0;
    r.trim = d.trim;
    r.stats = (in.stats || in.cstats) ? 1 : 0;
    r.ragged = in.tlen ? 1 : 0;
    r.flat_nrm_refused = d.flat_nrm_refused;
    r.nblk = d.nblk;
    r.epi = in.epi;
    r.gru = gru;
    r.form = d.form;
    r.Z = in.Z;
    return r;
}

// number of workgroups of the launch on the thin path, 0: not a thin launch
// (C0 / t_base: the launch's values at the point of the ladder that asks)
inline long gc_thin_blocks(const GCSelIn& p, int t_base) {
    const int n = p.Tout - t_base;
    // (layers with <= 4 output channels have the packed matrix too: a one-frame launch of the direct kernel walks its whole K
    // in one thread per output - 20-40 us; the fused parity pair of a transposed conv only exists there)
    if ((p.Ws && p.pair) || n > GC_THIN_NT || p.Z > 1 || p.stats || p.cstats || p.nrm0 || p.nrm1) return 0;
    if (p.epi != EPI_ACT && p.epi != EPI_ADD && p.epi != EPI_MUL && p.epi != EPI_GLU && p.epi != EPI_LSTM) return 0;
    if (p.epi == EPI_LSTM && (p.M & 3)) return 0;
    const long nblk = (long)((p.M + 7) >> 3) * p.Q * p.B;
    // (a few frames per row is not yet a small launch: the LSTM input projections of a batch-1 decode are 1 "frame" wide
    // and 401 rows high with K = 1024 - matrix work)
    if (nblk > GC_THIN_MAX_BLOCKS) return 0;
    // Both paths are latency-bound at these sizes: a thin block walks K / 32 rows with 1 + NT loads each (~0.08 us per row
    // and load, ~2 048 blocks in flight) and re-reads its 8 weight rows from L2 (32 B x K per block: 16 streams x one frame of
    // DCCRN's 256-channel layers = 4 096 blocks x 80 KB - 110 us against 80 us of the MFMA tiles); an MFMA workgroup makes K / 16
    // staged steps of ~0.5 us (~512 in flight).  Measured on the frame-online chunks of CRN / GCRN / DPCRN / DCCRN with 1 and 16
    // streams x 1 and 8 frames: up to 64 columns in all go to the thin kernel unless its weight traffic or its waves say no.
    if (!p.Ws) {
        const int nt = n <= 1 ? 1 : (n <= 2 ? 2 : (n <= 4 ? 4 : 8));
        const double waves_thin = std::ceil((double)nblk / 2048.0);
        const double waves_mfma = std::ceil((double)std::max(p.Z, 1) * p.B * p.Q * std::max(p.n_mtiles, 1) / 512.0);
        if ((long)p.B * n > 64 || nblk > 2800 * waves_mfma || waves_thin * (1 + nt) > 12 * waves_mfma) return 0;
    }
    return nblk;
}

// dynamic LDS of a tile launch
inline size_t gc_lds_bytes(const GCSelIn& in, const GCDispatch& d, int Wp, size_t epi_bytes, int nbuf) {
    const size_t as = (size_t)((in.KCp * (d.BM / 4) + 255) / 256) * 1024, bs = (size_t)((in.CI_C * d.nrows * Wp + 255) / 256) * 256;
    const bool nrmv = in.nrm0 || in.nrm1;
    const size_t nrb = d.flat_upr ? GC_FLAT_NRM_ROWS : 1;      // FLAT: parameters of two batch rows
    const size_t nrm = (nrmv ? (size_t)(nrb * GC_NRM_MAXC + 2 * nrb * gc_kcp_max(d.BM) + 2) * 16 : 0) + (d.flat_upr ? 128 : 0);      // gc_kernel NRM: nrmC + nrmK; FLAT: utab
    const size_t cst = in.cstats ? (size_t)4 * 256 * 2 * 4 : 0;      // GCParams::cstats: cpart [WM][4][BN][2] <= 8 KB, behind the strips inside the staging area
    return std::max((size_t)nbuf * (as + bs) * 4, epi_bytes + cst) + (GC_TAB_KOFF + GC_MAX_KCP + 8) * 4 + (size_t)4 * d.BM * 4 + 64 + nrm;
}
// epilogue: 4*BM row parameters + one transposition strip per wave (rows x (cols + 4))
inline size_t gc_epi_bytes(const GCDispatch& d) { return (size_t)(4 * (d.BM / d.WM) * 36) * sizeof(float); }

// all chunks of a source resident in LDS at once (gc_kernel RES): launches of at most one workgroup per CU whose staging fits;
// returns the staging buffers (0: no)
inline int gc_resident_fits(const GCSelIn& p, const GCDispatch& d) {
    if (d.trim || p.epi == EPI_LSTM || p.epi == EPI_CMB || p.fz || p.nrm0 || p.nrm1 || p.cstats) return 0;
    const long nblk = (long)p.Z * p.B * p.Q * d.n_ttiles * p.n_mtiles;
    const int nch0 = d.C0 > 0 ? (d.C0 + p.CI_C - 1) / p.CI_C : 0, nch1 = p.C1 > 0 ? (p.C1 + p.CI_C - 1) / p.CI_C : 0;
    int nb = std::max(std::max(nch0, nch1), 1);
    // (few frames per row: the chunks of the frame-online mode.  A batch-1 offline decode has as few workgroups, but 64
    // frames of matrix work per chunk to hide the next load under - the double-buffered loop is 1-3 % faster there)
    if (nblk > 256 || nb <= 2 || p.Tout - d.t_base > 64) return 0;
    // as many chunks per round trip as the LDS holds (a longer source goes in groups)
    while (nb > 2 && gc_lds_bytes(p, d, p.g_Wp[d.geom], gc_epi_bytes(d), nb) > 158 * 1024) --nb;
    return nb <= 2 ? 0 : nb;
}

// kernel variants with unit-flattened column tiles (GCParams::flat_upr) that are instantiated: the tiles whose last time tile
// of a T = 401 row is mostly padding, for the epilogues the zoo uses on them
// (64-row tiles only.  Measured in round 6 on one box, batch 256, T = 401, flattened against plain tiles with identical output
// hashes: 64 -> 64 channels at F = 79 on the 64 x 256 tile 3.43 -> 3.17 ms; 32 -> 32 channels on the 32 x 128 tile 1.13 -> 1.26 ms -
// that tile is bound by its staging, not by matrix slots, and a unit's own halo is 9 % more bytes; 64 -> 128 channels on the
// 128 x 128 tile 5.61 -> 5.63 ms against three full tiles + the 32-column tail launch, CTSNet as a whole 3 138 -> 3 017 utt/s)
constexpr bool gc_flat_inst(int BM, int BN, int EPI, int UWv) {
    const bool tile = BM == 64 && (BN == 256 || BN == 128);
    if (!tile) return false;
    if (UWv == 36) return EPI == EPI_ACT || EPI == EPI_GLU || (EPI == EPI_CMB && BN == 256);
    if (UWv == 32) return EPI == EPI_ACT || (EPI == EPI_ADD && BN == 128);
    return false;
}
// (epilogues outside ACT / ADD / GLU / CMB have no flattened variant)
inline bool gc_flat_supported(int BM, int BN, int epi, int uw) {
    return (epi == EPI_ACT || epi == EPI_ADD || epi == EPI_GLU || epi == EPI_CMB) && gc_flat_inst(BM, BN, epi, uw);
}

// the warp grid of a tile
inline void gc_tile_waves(GCDispatch& d) {
    d.WM = d.BN == 32 || (d.BM == 128 && d.BN == 64) ? 4 : (d.BN == 256 && d.BM == 64) || d.BM == 32 ? 1 : 2;
    d.WN = 4 / d.WM;
}

// The variant of the tile kernel for a dispatch whose tile, geometry and per-launch values are set (res: resident-K wanted):
// every refusal of a launch the kernels have no variant for
inline void gc_select_form(const GCSelIn& in, GCDispatch& d, bool res) {
    const bool nrm = in.nrm0 || in.nrm1;
    const int BM = d.BM, BN = d.BN, epi = in.epi;
    gc_tile_waves(d);
    switch (epi) {
        case EPI_ACT: case EPI_ADD: case EPI_MUL: case EPI_GLU: break;
        case EPI_CMB: SE_CHECK(!res && BM >= 64, "no resident-K / 32-row form of the combine epilogue"); break;
        case EPI_LSTM: SE_CHECK(!res, "no resident-K form of the LSTM step"); break;
        default: SE_CHECK(false, "unknown epilogue");
    }
    const int Wp = in.g_Wp[d.geom];
    d.lds = gc_lds_bytes(in, d, Wp, gc_epi_bytes(d), res ? d.nbuf : 2);
    d.nblk = (long)in.Z * (d.flat_upr ? 1 : in.B) * d.Qt * d.n_ttiles * in.n_mtiles;
    SE_CHECK(d.nblk > 0 && d.nblk < (1L << 31), "grid size");
    if (d.flat_upr) {        // unit-flattened column tiles (only the instantiated variants get here)
        const int uw = Wp / (BN / 32);
        SE_CHECK(!res && !in.fz && !d.trim && !d.qt2 && d.pw4 && d.t_base == 0, "gc_launch: flattened tiles on a launch they do not cover");
        for (const int uwv : {36, 32}) {
            if (res || uw != uwv || !gc_flat_supported(BM, BN, epi, uwv)) continue;
            if (epi == EPI_ACT && BM == 64 && nrm) {
                SE_CHECK(in.causal && in.Z == 1 && d.C0 + in.C1 <= GC_NRM_MAXC, "gc_launch: on-the-fly InstanceNorm needs causal taps and <= 128 input channels");
                SE_CHECK(gc_flat_rows_spanned(in.B, d.flat_upr, BN / 32) <= GC_FLAT_NRM_ROWS,
                         "gc_launch: a flattened tile with on-the-fly InstanceNorm would span more batch rows than it holds parameters for");
                d.form = uwv == 36 ? GC_FORM_FLAT36_NRM : GC_FORM_FLAT32_NRM;
                return;
            }
            SE_CHECK(!nrm, "gc_launch: this flattened variant cannot normalise its sources on the fly");
            d.form = uwv == 36 ? GC_FORM_FLAT36 : GC_FORM_FLAT32;
            return;
        }
        SE_CHECK(false, "gc_launch: no flattened variant of this kernel");
    }
    if ((epi == EPI_ACT || epi == EPI_ADD) && !res && in.fz) {          // branch interaction folded into the store (GCParams::fz)
        SE_CHECK(!d.trim && !in.stats, "gc_launch: no trimming / statistics variant of the kernel with the folded interaction");
        d.form = GC_FORM_FZ;
        return;
    }
    SE_CHECK(!in.fz, "gc_launch: this kernel variant cannot fold the branch interaction into its store");
    if (epi == EPI_ACT && BM == 64 && !res && nrm) {      // sources normalised on the fly (GCParams::nrm0 / nrm1)
        SE_CHECK(!d.trim && in.causal && !d.qt2 && in.Z == 1 && d.C0 + in.C1 <= GC_NRM_MAXC,
                 "gc_launch: on-the-fly InstanceNorm needs causal taps, one-row tiles and <= 128 input channels");
        d.form = GC_FORM_NRM;
        return;
    }
    SE_CHECK(!nrm, "gc_launch: this kernel variant cannot normalise its sources on the fly");
    if (epi == EPI_ACT && !res && d.trim) {
        d.form = GC_FORM_TRIM;
        return;
    }
    SE_CHECK(!d.trim, "gc_launch: no trimming variant of this kernel");
    d.form = res ? GC_FORM_RES : GC_FORM_PLAIN;
}

// true when launches of a plan can emit the per-tile statistics of GCParams::stats
inline bool gc_stats_tile(bool Ws, int epi, int BM) { return !Ws && (epi == EPI_GLU || (epi == EPI_ACT && BM == 64)); }

// The direct (<= 4 output channels) path: plain or LDS-tiled form
inline void gc_select_direct(const GCSelIn& p, GCDispatch& d) {
    SE_CHECK(!p.fz, "gc_launch: the direct (<= 4 channel) path cannot fold the branch interaction into its store");
    SE_CHECK(!p.dst_elu, "gc_launch: the direct (<= 4 channel) path has no second (ELU) store");
    SE_CHECK(!p.nrm0 && !p.nrm1, "gc_launch: the direct (<= 4 channel) path cannot normalise its sources on the fly");
    const int MM = p.M <= 1 ? 1 : (p.M <= 2 ? 2 : 4);
    constexpr int SQB = GC_SMALL_QB, SWT = GC_SMALL_WT;
    // LDS-tiled form when the launch still fills the chip with 8-row workgroups and the patch of at least 2 channels fits
    const int NR = (SQB - 1) * p.si + (p.sm_dfmax - p.sm_dfmin) + 1;
    constexpr int small_kb = 24;       // LDS budget of the staged patch (KB): 2-channel chunks, 6-7 workgroups per CU (40 KB: DCCRN -0.4 %, CTSNet -1.7 %)
    // <= 8: s_w holds 8 channels; <= 24 patch rows per chunk: a wave carries 6 rows of the next chunk in registers (gc_small_lds_kernel)
    const int CC = std::min(std::min(8, 24 / std::max(NR, 1)), (int)((size_t)small_kb * 1024 / ((size_t)NR * SWT * sizeof(float))));
    const long nblk8 = (long)((p.Tout + 255) / 256) * ((p.Q + SQB - 1) / SQB) * p.B * p.Z;
    const bool epi_ok = p.epi == EPI_ACT || p.epi == EPI_ADD || p.epi == EPI_MUL || p.epi == EPI_GLU;
    // (worth it from three frequency rows per output row on: with one or two the plain kernel's caches do as well - CRN /
    // DPCRN last layers measured 1-3 % slower here, DCCRN's 5-tap deconv 1 % faster with a third of the fetches)
    if (CC >= 2 && p.Q >= SQB && (p.si == 1 || p.si == 2) && p.sm_dtmax - p.sm_dtmin <= SWT - 256 && nblk8 >= 4 * 256 &&
        (p.sm_dfmax - p.sm_dfmin >= 2 || (p.sm_dfmax - p.sm_dfmin >= 1 && MM >= 2 && d.C0 + p.C1 >= 64))) {
        SE_CHECK(nblk8 < (1L << 31), "grid size");
        SE_CHECK(epi_ok, "direct small-M path: unsupported epilogue");
        d.family = GC_FAM_DIRECT_LDS;
        d.CC = CC;
        d.NR = NR;
        d.lds = (size_t)CC * NR * SWT * sizeof(float);
        d.nblk = nblk8;
        return;
    }
    d.nblk = (long)((p.Tout + 255) / 256) * p.Q * p.B * p.Z;
    SE_CHECK(d.nblk > 0 && d.nblk < (1L << 31), "grid size");
    SE_CHECK(epi_ok, "direct small-M path: unsupported epilogue");
    d.family = GC_FAM_DIRECT;
}

inline GCChoice gc_select(const GCSelIn& in) {
    GCChoice ch;
    GCDispatch& d = ch.main;
    // t_base (default 0): first output frame of the launch - frame-online chunks only produce the frames behind their
    // history columns.  A multiple of 4, so that the 16 B staging groups keep their alignment to frame 0.
    SE_CHECK(in.C0 == in.pl_C0 && in.C1 == in.pl_C1, "gc_launch: source channel split differs from the plan");
    SE_CHECK(!in.dst_elu || (in.epi == EPI_GLU && in.Z == 1), "gc_launch: the second (ELU) store belongs to the gated epilogue");
    d.C0 = (in.epi == EPI_LSTM && in.first_step && in.C1 == 0) ? 0 : in.C0;       // h_{-1} = 0: no matrix work (a step that also projects its input keeps both)
    d.t_base = in.t_base;
    const bool thin_ok = !in.fz && !in.dst_elu;          // (GCParams::fz / dst_elu: MFMA kernel only)
    auto thin = [&]() {
        d.nblk = thin_ok ? gc_thin_blocks(in, d.t_base) : 0;
        if (d.nblk <= 0) return false;
        d.family = GC_FAM_THIN;
        d.thin_n = in.Tout - d.t_base;
        return true;
    };
    if (in.t_base > 0 && thin()) {       // (any first frame)
        d.early = true;
        return ch;
    }
    if (in.tb_soft) d.t_base &= ~3;
    const int tb = d.t_base, Tspan = in.Tout - tb;
    SE_CHECK(tb >= 0 && (tb & 3) == 0 && Tspan > 0, "gc_launch: first output frame must be a multiple of 4 below Tout");
    SE_CHECK(tb == 0 || (!in.stats && !in.cstats), "gc_launch: the statistics epilogue needs whole rows");
    const int BM = in.BM;
    d.n_ttiles = (Tspan + in.BN - 1) / in.BN;
    d.Qt = in.Q;
    d.nrows = in.nrows;
    d.nbuf = 0;
    d.dbg = in.tun.dbg;
    // workgroups of the launch on the plan's own (128-column) tiles: what the thresholds below are in
    const long nblk = (long)in.Z * in.B * in.Q * d.n_ttiles * in.n_mtiles;
    // patch offsets inside one staged chunk are 32-bit (the 64-bit part of an address is the per-block / per-chunk base)
    SE_CHECK((double)in.CI_C * (double)std::max(in.s0_c, in.s1_c) + (double)in.Fin * (double)std::max(in.s0_f, in.s1_f) + in.Tin < 1.0e9,
             "gc_launch: source plane too large for 32-bit patch byte offsets");
    // 16 B staging groups: exact when no group straddles the end of a row (Tin % 4 == 0); for causal tap sets a straddling
    // group only feeds output frames >= Tin, which are never stored - then it merely has to stay inside mapped memory
    // (a tap set that looks ahead would read the straddling group's foreign frames into stored outputs: the kernel trims
    // them in LDS, GC_TRIM_TAIL)
    // the trimming variant exists for the plain epilogue (DCCRN's decoder); it pays from a few thousand workgroups on - small
    // launches are latency-bound and the extra LDS stores per chunk cost them 3 % (batch 1)
    constexpr long trim_min = 8192;
    const bool trim_ok = in.epi == EPI_ACT && nblk >= trim_min;
    d.pw4 = (in.desc4 && (in.Tin % 4 == 0 || ((in.causal || trim_ok) && in.overread0 && in.overread1))) ? 1 : 0;
    d.trim = (d.pw4 && !in.causal && in.Tin % 4 != 0) ? 1 : 0;
    const bool stats_tile = gc_stats_tile(in.pl_Ws, in.pl_epi, BM);
    SE_CHECK(!in.stats || stats_tile, "gc_launch: this tile configuration has no statistics epilogue");
    SE_CHECK(!in.cstats || (stats_tile && in.n_mtiles == 1 && in.Z == 1),
             "gc_launch: column statistics need a statistics tile configuration and one m-tile (M " + std::to_string(in.M) + ", BM " +
                 std::to_string(BM) + ", m-tiles " + std::to_string(in.n_mtiles) + ", epilogue " + std::to_string(in.epi) + ", direct " +
                 std::to_string(in.Ws != 0) + ")");
    SE_CHECK(d.pw4 || in.CI_C * in.nrows * in.g_Wp[GC_G_MAIN] <= gc_bld_max(BM) * 256,
             "pointwise layer with a row length that is not a multiple of 4 needs its sources inside the engine arena");
    if (thin()) return ch;
    if (in.Ws) {
        gc_select_direct(in, d);
        return ch;
    }
    auto tile = [&](GCDispatch& t, int geom, int bm, int bn, int n_ttiles) {
        t.geom = geom;
        t.BM = bm;
        t.BN = bn;
        t.n_ttiles = n_ttiles;
    };
    // small launches: 64-column tiles double the workgroup count (and waste less of the last time tile: T = 401 is
    // 6.3 x 64).  Measured on the TCM models: 64-row layers gain up to ~1 500 workgroups of 128 columns (G2Net + 7 % at
    // B = 64, + 4 % at B = 256, + 16 % at B = 8; DCCRN's big grids lose 1 %), 128-row layers only below one workgroup
    // per CU (B = 8: + 15 %; B = 64: - 3 %)
    if (in.g_BN[GC_G_N64] == 64 && nblk < (BM == 64 ? in.tun.alt_n64 : 256)) {
        constexpr long alt32_max = 512;      // 64-column workgroup count below which a 128-row layer uses 32-column tiles
        const long nblk64 = (long)in.Z * in.B * in.Q * ((Tspan + 63) / 64) * in.n_mtiles;
        if (BM == 128 && in.g_BN[GC_G_N32] == 32 && nblk64 < alt32_max) tile(d, GC_G_N32, 128, 32, (Tspan + 31) / 32);       // tiny launches
        else tile(d, GC_G_N64, BM == 64 ? 64 : 128, 64, (Tspan + 63) / 64);
        gc_tile_waves(d);
        d.nbuf = d.BM == 128 && d.BN == 64 ? 0 : gc_resident_fits(in, d);
        gc_select_form(in, d, d.nbuf > 0);
        return ch;
    }
    // unit-flattened column tiles (GCParams::flat_upr): equal-length offline batches whose rows do not fill their last time tile.
    // T = 401 is 13 units of 32 frames: 2 tiles of 256 / 4 tiles of 128 columns per row hold 16, the flattened batch needs
    // 13 B / 8 (or / 4) tiles - 19 % fewer workgroups for the same stored values
    // (flattened tiles take precedence over the two-row tiles where both apply)
    constexpr long flat_min = 1024;
    if (in.tun.flat && BM == 64 && in.flat_uw && tb == 0 && d.pw4 && !d.trim && !in.fz && in.Z == 1 && nblk >= flat_min && in.B > 1) {
        const int upr = (Tspan + 31) / 32;
        const double sbmax = 4.0 * (double)std::max(in.s0_b, in.s1_b);
        // tile width as the plain path would choose it
        const bool wide = in.g_BN[GC_G_FLAT256] == 256 && nblk >= in.tun.wide_min && gc_flat_supported(64, 256, in.epi, in.flat_uw);
        const int fg = wide ? GC_G_FLAT256 : GC_G_FLAT128;
        const int upt = wide ? 8 : 4;
        const long tiles_plain = (long)in.B * ((Tspan + 32 * upt - 1) / (32 * upt));
        const long tiles_flat = ((long)in.B * upr + upt - 1) / upt;
        // (a unit of a later batch row adds (rows ahead) x batch stride to a 32-bit byte offset)
        const double span = ((double)(upt + upr - 1) / upr + 1.0) * sbmax;
        // a normalising tile holds the InstanceNorm parameters of GC_FLAT_NRM_ROWS batch rows: rows shorter than a tile
        // (wide: upr 1, 2, 3, 5; narrow: upr 1) would put three or more rows into some tiles - those launches keep the plain tiles
        const int nrm_rows = (in.nrm0 || in.nrm1) ? gc_flat_rows_spanned(in.B, upr, upt) : 0;
        const bool nrm_ok = nrm_rows <= GC_FLAT_NRM_ROWS;
        const bool flat_ok = in.g_BN[fg] && gc_flat_supported(BM, in.g_BN[fg], in.epi, in.flat_uw) && tiles_flat * 100 <= tiles_plain * 94 &&
                             span < 3.0e9;
        if (flat_ok && !nrm_ok) d.flat_nrm_refused = nrm_rows;
        if (flat_ok && nrm_ok) {
            d.flat_upr = upr;
            d.flat_units = in.B * upr;
            tile(d, fg, 64, wide ? 256 : 128, (int)tiles_flat);
            gc_select_form(in, d, false);
            return ch;
        }
    }
    const int nt256 = (Tspan + 255) / 256;
    // big launches of a 64-row layer: 64 x 256 tiles when the patch goes in 16 B groups (4 x fewer slots), the rows fill the
    // wide tiles and the staging buffers leave room for 3 workgroups per CU
    if (in.g_BN[GC_G_N256] == 256 && BM == 64 && d.pw4 && nblk >= in.tun.wide_min && Tspan * 100 >= nt256 * 256 * in.tun.wide_fill &&
        (long)in.CI_C * in.nrows * in.g_Wp[GC_G_N256] <= 4608 /* 5 x 256 groups, 3 workgroups' LDS */) {
        tile(d, GC_G_N256, 64, 256, nt256);
        gc_select_form(in, d, false);
        return ch;
    }
    // big launches of the per-step LSTM GEMM: 128 x 256 tiles (two workgroups per CU)
    constexpr long wide128_min = 1536;      // 128-column workgroup count from which the 128 x 256 tile is used
    constexpr int wide128_fill = 75;        // least fill of the wide tiles in percent
    if (in.g_BN[GC_G_N256] == 256 && BM == 128 && in.epi == EPI_LSTM && d.pw4 && !d.trim && !in.stats && nblk >= wide128_min &&
        Tspan * 100L >= (long)nt256 * 256 * wide128_fill) {
        tile(d, GC_G_N256, 128, 256, nt256);
        gc_select_form(in, d, false);
        return ch;
    }
    // big launches of layers whose neighbouring output rows share input rows: two-row tiles (2 x 64 frames)
    // (not with edge-row classes: a two-row tile pairs an edge row with a whole one, and both would run the full K)
    if (!in.edge && in.g_BN[GC_G_QT2] == 64 && in.BN == 128 && in.Q >= 2 && !in.stats && !in.cstats && in.pad_lo == 0 && in.epi != EPI_LSTM &&
        !in.nrm0 && !in.nrm1 && nblk >= in.tun.qt2_min) {
        d.qt2 = 1;
        d.qq_off = in.qt2_qoff;
        d.nrows = in.qt2_nrows;
        d.Qt = (in.Q + 1) / 2;
        tile(d, GC_G_QT2, BM, 128, (Tspan + 63) / 64);
        gc_select_form(in, d, false);
        return ch;
    }
    const bool main_ok = (in.BN == 128 && (BM == 128 || BM == 64 || BM == 32)) || (in.BN == 64 && (BM == 128 || BM == 64));
    // the last time tile of a row, when it is at most half full, goes to a narrower kernel (own launch, same weights)
    const int full = Tspan / in.BN, rem = Tspan - full * in.BN;
    if (in.tail_split && full >= 1 && rem > 0 && in.g_BN[GC_G_N32] && rem <= in.g_BN[GC_G_N32]) {
        SE_CHECK(BM == 128 && in.g_BN[GC_G_N32] == 32, "no gemmconv tail tile config");
        ch.has_tail = true;
        ch.tail = d;
        ch.tail.t_base = tb + full * in.BN;
        tile(ch.tail, GC_G_N32, 128, 32, 1);
        gc_select_form(in, ch.tail, false);
        d.n_ttiles = full;
    }
    SE_CHECK(main_ok, "no gemmconv tile config");
    tile(d, GC_G_MAIN, BM, in.BN, d.n_ttiles);
    gc_select_form(in, d, false);
    return ch;
}

}  // namespace se

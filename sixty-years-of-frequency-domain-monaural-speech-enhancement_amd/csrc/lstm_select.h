// Kernel selection of the cooperative LSTM recurrence (k_lstm_coop.hip) as pure host functions: which kernel form one call takes
// (lstm_coop_select, lstm_stack_select), what the models may ask for (the *_ok support queries) and how a stack is cut into the
// launches of the chunk pipeline (lstm_chunk_steps, lstm_chunk_launch).  Plain C++17 without a HIP header, so that all of it
// compiles and is tested on a CPU (tests/lstm_select_check.cpp, tests/lstm_select_probe.cpp).  k_lstm_coop.hip queries the CU
// count, fills an LstmSelIn and hands the LstmChoice to its one launcher.  A new form is added here: its rung in lstm_coop_select,
// and its instantiation in k_lstm_coop.hip's coop_fn_of.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>

namespace se {

// Environment switches of the ladder, each read once per process (lstm_tuning_env)
struct LstmTuning {
    int coop16 = 1;      // SE_COOP16: 0 = no 16-sequence tiles (lstm_coop16_kernel; neither H = 256 then)
    int coop4 = 1;       // SE_COOP4: 0 = no 4-sequence sub-tiles (lstm_coop8_kernel)
    int coop256 = 1;     // SE_LSTM_COOP256: 0 = H = 256 layers run the per-step GEMM launches of LstmBig
    int chunk = 1;       // SE_LSTM_CHUNK: 0 = no chunk pipeline (a stack runs layer after layer)
    int dbg = 0;         // SE_COOP_DBG: LstmCoopArgs::dbg
};
inline const LstmTuning& lstm_tuning_env() {
    static const LstmTuning t = [] {
        LstmTuning v;
        v.coop16 = getenv("SE_COOP16") ? atoi(getenv("SE_COOP16")) : v.coop16;
        v.coop4 = getenv("SE_COOP4") ? atoi(getenv("SE_COOP4")) : v.coop4;
        v.coop256 = getenv("SE_LSTM_COOP256") ? atoi(getenv("SE_LSTM_COOP256")) : v.coop256;
        v.chunk = getenv("SE_LSTM_CHUNK") ? atoi(getenv("SE_LSTM_CHUNK")) : v.chunk;
        v.dbg = getenv("SE_COOP_DBG") ? atoi(getenv("SE_COOP_DBG")) : v.dbg;
        return v;
    }();
    return t;
}

enum LstmForm : int {
    LSTM_FORM_REFUSED = 0,   // no kernel for the call: LstmChoice::refusal is the launcher's SE_CHECK message
    LSTM_FORM_KS,            // lstm_coop_ks_kernel<H, NS, TAG>: one tile, K split over every CU
    LSTM_FORM_COOP8,         // lstm_coop8_kernel<H, LEAD, NW>: 4-sequence sub-tiles
    LSTM_FORM_COOP16,        // lstm_coop16_kernel<H>: 16-sequence tiles (also every launch of the chunk pipeline)
    LSTM_FORM_COOP,          // lstm_coop_kernel<H>: the flag-barrier form
    LSTM_FORM_STACK,         // lstm_stack_kernel<H, L>: a whole stack on one sequence
};
// the launch log's name of a form (LstmLaunchRec::kernel)
inline const char* lstm_form_name(int form) {
    switch (form) {
        case LSTM_FORM_KS: return "ks";
        case LSTM_FORM_COOP8: return "coop8";
        case LSTM_FORM_COOP16: return "coop16";
        case LSTM_FORM_COOP: return "coop";
        case LSTM_FORM_STACK: return "stack";
        default: return "refused";
    }
}

// What the choice depends on
struct LstmSelIn {
    int H = 0, S = 0, Z = 1;         // units, sequences, LSTMs of the launch (chunk pipeline: layer ranges)
    long gx_row = 0, out_row = 0;    // row pitches of the gate and output tensors (LstmCoopArgs)
    int n_cu = 0;
    int chunk = 0;                   // a launch of the chunk pipeline (launch_lstm_coop_chunk)
    int n_layers = 0;                // ... and the layers of its whole stack
};

// One dispatch: everything the launcher needs and the launch log reports
struct LstmChoice {
    int form = LSTM_FORM_REFUSED;
    const char* refusal = "";
    int H = 0, NS = 0, TAG = 0, LEAD = 0, NW = 0, L = 0;      // template values (0: the kernel does not have it)
    int Z = 0, SS = 0;               // LSTMs per launch, sequence slices
    long grid = 0;
    int block = 256;
    size_t lds = 0;                  // dynamic LDS of the launch
    int lds_attr = 0;                // hipFuncAttributeMaxDynamicSharedMemorySize to set on the function, once per device
    // preparation enqueued before the kernel, in this order: the arrival flags, the exchange slabs (zero: h_{-1} = 0; then slab 1
    // of each LSTM filled with a stale tag so that it does not look like h_0), the cell state
    long nflag = 0;                  // arrival flags to zero (0: the form has none)
    int stale = 0;
    int zero_cell = 0;
    int slabs = 0;                   // slab pairs [2][S][H] of the exchange tensor (Z; chunk pipeline: layers of the stack)
    int chunk = 0;                   // chunk launch: LstmCoopArgs::pz, and only the slabs of layers that start (t0 == 0) are prepared
};

// ------------------------------------------------------------------------------------------------ shared rules
// the per-lane parts of the gate / output addresses are 32-bit offsets inside one LSTM's tensors
inline bool lstm_rows_fit32(int H, long gx_row, long out_row) { return (double)gx_row * 4 * H * 4 < 4.0e9 && (double)out_row * H < 4.0e9; }
// ... and so are the offsets into a slab pair of the exchange tensor
inline bool lstm_slabs_fit32(int H, int S) { return (long)S * H * 8 < (1L << 31); }
// sequence slices: n tiles (or sub-tiles) over the CUs that `wgs` workgroups per slice leave
inline int lstm_slices(int n, int wgs, int n_cu) { return std::max(1, std::min(n, n_cu / wgs)); }
// dynamic LDS of the 16-sequence tiles: two h tiles, the gate staging, the cell state of the ntl tiles a workgroup owns
inline size_t lstm_tile16_lds(int H, int ntl) { return ((size_t)2 * 16 * (H + 4) + (size_t)2 * 4 * 256 + (size_t)4 * ntl * 64) * sizeof(float); }
constexpr size_t LSTM_LDS_MAX = 160 * 1024;      // LDS limit of the tile forms
constexpr size_t LSTM_SUB4_CELL_MAX = 24 * 1024;  // most cell state of a sub-tile slice
constexpr int LSTM_CHUNK_T = 48;                 // steps per chunk of the chunk pipeline

namespace lstm_detail {
inline LstmChoice refuse(const char* msg) {
    LstmChoice c;
    c.refusal = msg;
    return c;
}
inline LstmChoice begin(const LstmSelIn& in, int form) {
    LstmChoice c;
    c.form = form;
    c.H = in.H;
    c.Z = in.Z;
    c.slabs = in.Z;
    return c;
}
// the conditions the two tile forms share (`on`: the form's switch)
inline bool tiles_ok(const LstmSelIn& in, int on) {
    return on && in.S >= 17 && (in.H / 16) * in.Z <= in.n_cu && lstm_slabs_fit32(in.H, in.S) && lstm_rows_fit32(in.H, in.gx_row, in.out_row);
}
// 16-sequence tiles; false: not applicable
inline bool coop16(const LstmSelIn& in, const LstmTuning& tun, LstmChoice& out) {
    if (!tiles_ok(in, tun.coop16)) return false;
    LstmChoice c = begin(in, LSTM_FORM_COOP16);
    const int US = in.H / 16, NT = (in.S + 15) / 16;
    c.SS = lstm_slices(NT, US * in.Z, in.n_cu);
    c.lds = lstm_tile16_lds(in.H, (NT + c.SS - 1) / c.SS);
    if (c.lds > LSTM_LDS_MAX) return false;
    c.lds_attr = (int)LSTM_LDS_MAX;
    c.grid = (long)US * c.SS * in.Z;
    c.stale = 1;
    out = c;
    return true;
}
// 4-sequence sub-tiles, LEAD = slots a fetch runs ahead (at most the sub-tiles a workgroup owns: the padding slots at the end of
// the launch are sub-tiles of step T); false: not applicable
inline bool coop8(const LstmSelIn& in, const LstmTuning& tun, LstmChoice& out) {
    if (!tiles_ok(in, tun.coop4)) return false;
    LstmChoice c = begin(in, LSTM_FORM_COOP8);
    const int H = in.H, US = H / 16, NS4 = (in.S + 3) / 4;
    c.SS = lstm_slices(NS4, US * in.Z, in.n_cu);
    if ((size_t)((NS4 + c.SS - 1) / c.SS) * 256 > LSTM_SUB4_CELL_MAX) return false;       // cell state of the slice must fit LDS
    const int nsub_min = NS4 / c.SS;                          // the fewest sub-tiles a workgroup owns (>= 1)
    int lead = std::min(3, nsub_min);
    if (nsub_min >= 3 && nsub_min < 6) lead = 2;            // a fetch issued 3 slots ahead of a 4-slot cycle would read before h_{t-1} is out
    c.LEAD = std::max(lead, 1);
    c.NW = 4;
    const int nsub_max = (NS4 + c.SS - 1) / c.SS;
    const size_t wl_floats = H == 1024 ? (size_t)c.NW * (H / 64) * 256 : 0;      // one unit's weights per wave (kernel: UL)
    c.lds = ((size_t)(c.LEAD + 1) * 4 * (H + 16) + (size_t)(c.LEAD + 1) * c.NW * 64 + wl_floats + (size_t)64 * nsub_max) * sizeof(float);
    c.lds_attr = (int)LSTM_LDS_MAX;
    c.grid = (long)US * c.SS * in.Z;
    c.block = 64 * c.NW;
    c.stale = 1;
    // (the rung is taken even so: the ladder does not go on to another form)
    out = c.lds <= LSTM_LDS_MAX ? c : refuse("cooperative LSTM (sub-tile form): too many sequences per workgroup for the LDS-resident cell state");
    return true;
}
}  // namespace lstm_detail

// ------------------------------------------------------------------------------------------------ the ladder
// The kernel one launch_lstm_coop / launch_lstm_coop_chunk call reaches
inline LstmChoice lstm_coop_select(const LstmSelIn& in, const LstmTuning& tun) {
    using namespace lstm_detail;
    const int H = in.H, S = in.S, Z = in.Z, n_cu = in.n_cu;
    LstmChoice c;
    if (in.chunk) {      // a launch of the chunk pipeline: 16-sequence tiles, Z layer ranges of an n_layers stack
        if (!(Z >= 1 && Z <= 4 && in.n_layers <= 4 && (H == 512 || H == 1024))) return refuse("launch_lstm_coop_chunk: 1 - 4 layers of 512 / 1024 units");
        if (!lstm_rows_fit32(H, in.gx_row, in.out_row)) return refuse("launch_lstm_coop_chunk: tensor too large for 32-bit lane offsets");
        c = begin(in, LSTM_FORM_COOP16);
        const int US = H / 16, NT = (S + 15) / 16;
        c.SS = lstm_slices(NT, US * Z, n_cu);
        c.lds = lstm_tile16_lds(H, (NT + c.SS - 1) / c.SS);
        if (c.lds > LSTM_LDS_MAX) return refuse("chunked cooperative LSTM: too many tiles per workgroup");
        c.lds_attr = (int)LSTM_LDS_MAX;
        c.grid = (long)US * c.SS * Z;
        c.stale = 1;
        c.slabs = in.n_layers;
        c.chunk = 1;
        return c;
    }
    constexpr const char* widths = "cooperative LSTM kernel is built for H = 512 / 1024";
    if (H < 16 || Z < 1) return refuse(widths);
    if (Z * lstm_slices((S + 15) / 16, (H / 16) * Z, n_cu) > 256) return refuse("cooperative LSTM: too many slices");
    if (H == 256) {      // opt-in width: 16-sequence tiles only, one LSTM of 17 - 4096 sequences
        if (Z == 1 && tun.coop256 && S <= 4096 && coop16(in, tun, c)) return c;
        return refuse("cooperative LSTM at H = 256: one LSTM of 17 - 4096 sequences (lstm_coop256_supported)");
    }
    if (H != 512 && H != 1024) return refuse(widths);
    // one tile: every CU on the K-split form (H = 1024: 7.5 -> 5.1 ... 5.9 us per step for 1 ... 16 sequences; H = 512: 4.4 -> 3.8 at
    // one sequence, nothing from 8 on or with two LSTMs per launch - tools/coopbench.cpp)
    constexpr int ks_z = 2;      // most LSTMs per launch on the K-split form (two, GCRN: 4.4 -> 2.5 ... 3.0 us)
    if (S <= (H == 1024 ? 16 : 4) && (H == 1024 || Z <= ks_z) && (H / 4) * Z <= n_cu && (H / 4) * Z <= 256) {
        c = begin(in, LSTM_FORM_KS);
        // (the tagged exchange pays while a wave's share of h is one or two loads per lane: 4.9 -> 3.1 us per step at one sequence,
        // 5.4 -> 4.2 at four, nothing at sixteen)
        c.NS = S <= 1 ? 1 : S <= 4 ? 4 : 16;
        c.TAG = c.stale = S <= 4;
        c.SS = 1;
        c.grid = (long)(H / 4) * Z;
        c.lds = (size_t)4 * 16 * (H / 4 + 4) * sizeof(float) + (size_t)4 * 64 * 16;
        c.lds_attr = (int)c.lds;
        c.nflag = (long)Z * 256;
        return c;
    }
    // 16-sequence tiles (lstm_coop16_kernel) unless a workgroup would own a single tile per step AND fewer than 16 sequences per
    // unit slice's share of the chip are left to split: there the 4-sequence sub-tiles overlap their own exchange (batch 32,
    // H = 1024: 5.1 us per step against 7.4; batch 64: 8.1 against 7.8)
    const int us_z = (H / 16) * Z, nt16 = (S + 15) / 16;
    const bool sub4 = H == 1024 && us_z <= n_cu && nt16 <= n_cu / us_z && S * us_z < 60 * n_cu / 4;
    if (sub4 && coop8(in, tun, c)) return c;
    if (coop16(in, tun, c)) return c;
    if (coop8(in, tun, c)) return c;
    // the flag-barrier form
    if (us_z > n_cu) return refuse("cooperative LSTM: more unit slices than CUs");
    c = begin(in, LSTM_FORM_COOP);
    c.SS = lstm_slices(nt16, us_z, n_cu);
    c.grid = (long)us_z * c.SS;
    c.lds = (size_t)2 * 16 * (H + 4) * sizeof(float);
    c.lds_attr = (int)c.lds;
    c.nflag = (long)Z * c.SS * 64;       // 64 arrival flags per (z, sequence slice)
    c.zero_cell = 1;                     // h_{-1} = 0 and c_{-1} = 0 are data, not branches in the kernel
    return c;
}

// A stack of L layers on ONE sequence as one launch (lstm_stack_kernel)
inline bool lstm_stack_ok(int H, int L, int n_cu) { return (H == 1024 || H == 512) && (L == 2 || L == 3) && H / 4 <= n_cu; }
inline LstmChoice lstm_stack_select(int H, int L, int n_cu) {
    if (!lstm_stack_ok(H, L, n_cu)) return lstm_detail::refuse("launch_lstm_stack: 2 or 3 layers of 512 / 1024 units on one sequence");
    LstmChoice c;
    c.form = LSTM_FORM_STACK;
    c.H = H;
    c.L = L;
    c.Z = c.SS = 1;
    c.grid = H / 4;
    c.lds = ((size_t)4 * (2 * L - 1) * (H / 4) + (size_t)L * 64) * sizeof(float) + (size_t)(L - 1) * 16 * H * sizeof(float);
    c.lds_attr = (int)c.lds;
    c.stale = 1;
    c.slabs = L;
    return c;
}

// ------------------------------------------------------------------------------------------------ what the models may ask for
// launch_lstm_coop runs Z LSTMs of H units over S sequences
inline bool lstm_coop_ok(int H, int S, int Z) { return (H == 512 || H == 1024) && (H / 16) * Z <= 256 && S <= 4096; }
// ... and an H = 256, Z = 1 time-major layer (opt-in, LstmBig::build(.., coop256 = true))
inline bool lstm_coop256_ok(int S, int n_cu, const LstmTuning& tun) {
    LstmSelIn in;
    in.H = 256;
    in.S = S;
    in.gx_row = in.out_row = S;
    in.n_cu = n_cu;
    const LstmChoice c = lstm_coop_select(in, tun);
    return c.form == LSTM_FORM_COOP16 && c.H == 256;
}
// the chunk pipeline has a kernel for n_layers layers of H units over S sequences
inline bool lstm_coop_chunk_ok(int H, int S, int n_layers, int n_cu, const LstmTuning& tun) {
    if (!tun.chunk || (H != 512 && H != 1024) || n_layers < 2 || n_layers > 4 || S < 17) return false;
    const int US = H / 16, NT = (S + 15) / 16;
    // worth it where one layer alone leaves a workgroup a single tile per step (its exchange is then exposed) and the layers
    // together still fit the chip
    return US * n_layers <= n_cu && NT <= n_cu / US && lstm_slabs_fit32(H, S);
}
// Steps per chunk when a feature-major stack (rows of T * S elements) runs as the chunk pipeline, 0: it does not.  The chunk kernel
// addresses G / out with 32-bit lane offsets over those rows: batches of long clips (H = 1024: T * S >= ~244 k, e.g. 64 clips of
// 3 800 frames) go back to the per-layer path, whose ladder falls back by itself.
inline int lstm_chunk_steps(int H, int S, int n_layers, int T, int n_cu, const LstmTuning& tun) {
    if (!lstm_coop_chunk_ok(H, S, n_layers, n_cu, tun) || !lstm_rows_fit32(H, (long)T * S, (long)T * S)) return 0;
    // the pipeline runs (L - 1) chunks longer than the sequence, every launch costs ~3 steps' worth of launch + fill
    // (measured at batch 64, T = 401: 24 / 36 / 48 / 64 -> CRN 4 907 / 5 022 / 5 281 / 5 204 utt/s)
    const int Tc = std::max(2, std::min(LSTM_CHUNK_T, T)) & ~1;      // even: a chunk keeps the parity of the exchange slabs
    return T < 2 * Tc ? 0 : Tc;
}
// The pipeline of L layers over T steps in chunks of Tc: launch s of lstm_chunk_launches runs layer l on chunk s - l
struct LstmChunkRange {
    int layer, t0, len;
};
inline int lstm_chunk_launches(int T, int Tc, int L) { return (T + Tc - 1) / Tc + L - 1; }
// the ranges of launch s (at most 4), in layer order; returns their number
inline int lstm_chunk_launch(int T, int Tc, int L, int s, LstmChunkRange* out) {
    const int nc = (T + Tc - 1) / Tc;
    int n = 0;
    for (int l = 0; l < L && n < 4; ++l) {
        const int c = s - l;
        if (c < 0 || c >= nc) continue;
        out[n++] = {l, c * Tc, std::min(Tc, T - c * Tc)};
    }
    return n;
}

}  // namespace se

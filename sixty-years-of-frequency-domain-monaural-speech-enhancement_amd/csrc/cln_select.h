// Kernel selection of the cumulative LayerNorm (k_cln.hip) as a pure host function: which of its six forms one launch_cln /
// launch_cln_parts call takes, with the grid and dynamic LDS of every launch, and the calls it refuses.  Plain C++17 without a HIP
// header and without heap allocation, so that it compiles and is tested on a CPU (tests/cln_select_check.cpp,
// tests/cln_select_probe.cpp) and costs a one-frame push nothing (TaylorSENet_new: 75 choices).  k_cln.hip fills a ClnSelIn, checks
// the refusal and executes the ClnChoice's launches in order; the launch log is written from the same entries.  A new form is added
// here: its rung in cln_select, and its kernel's case in k_cln.hip's cln_run.
#pragma once
#include <cstddef>
#include <cstdlib>

namespace se {

// Environment switches of the ladder, each read once per process (cln_tuning_env); 0 = off, unset or anything else = on
struct ClnTuning {
    bool plane = true;        // SE_CLN_PLANE: 0 = the plain 2-D norm without a residual takes the row apply pass (cln_apply_kernel)
    bool stream_res = true;   // SE_CLN_STREAM_RES: 0 = no frame-online form takes the residual (blocks.h adds it with launch_add)
    bool stats = true;        // SE_CLN_STATS: 0 = the U-Net levels run launch_cln, not launch_cln_parts (blocks.h: cln_stats_enabled)
};
inline const ClnTuning& cln_tuning_env() {
    static const ClnTuning t = [] {
        ClnTuning v;
        v.plane = !(getenv("SE_CLN_PLANE") && atoi(getenv("SE_CLN_PLANE")) == 0);
        v.stream_res = !(getenv("SE_CLN_STREAM_RES") && atoi(getenv("SE_CLN_STREAM_RES")) == 0);
        v.stats = !(getenv("SE_CLN_STATS") && atoi(getenv("SE_CLN_STATS")) == 0);
        return v;
    }();
    return t;
}

enum ClnForm : int {
    CLN_FORM_REFUSED = 0,     // no kernel for the call: ClnChoice::refusal is the launcher's SE_CHECK message
    CLN_FORM_PLANE,           // offline: statistics, scan, plane apply (the residual rides on it)
    CLN_FORM_ROWS,            // offline: statistics, scan, row apply (pre-slope / FIR)
    CLN_FORM_PARTS,           // offline, from the producing conv's epilogue sums: scan of the parts, plane apply
    CLN_FORM_STREAM_REG,      // frame-online, one or two new frames: the register kernel
    CLN_FORM_STREAM_WINDOW,   // frame-online, a small window: the three passes in one launch
    CLN_FORM_STREAM_ROWS,     // frame-online: statistics, scan, row apply over the new columns
};
inline const char* cln_form_name(int form) {
    switch (form) {
        case CLN_FORM_PLANE: return "plane";
        case CLN_FORM_ROWS: return "rows";
        case CLN_FORM_PARTS: return "parts";
        case CLN_FORM_STREAM_REG: return "stream_reg";
        case CLN_FORM_STREAM_WINDOW: return "stream_window";
        case CLN_FORM_STREAM_ROWS: return "stream_rows";
        default: return "refused";
    }
}

enum ClnKernel : int { CLN_K_STATS = 0, CLN_K_SCAN, CLN_K_SCAN_PARTS, CLN_K_APPLY, CLN_K_APPLY_PLANE, CLN_K_WINDOW, CLN_K_WINDOW_REG };
// the launch log's name of a kernel (NormLaunchRec::kernel)
inline const char* cln_kernel_name(int kernel) {
    constexpr const char* names[] = {"cln_stats", "cln_scan", "cln_scan_parts", "cln_apply", "cln_apply_plane", "cln_window", "cln_window_reg"};
    return kernel >= 0 && kernel <= CLN_K_WINDOW_REG ? names[kernel] : "";
}

// What the choice depends on
struct ClnSelIn {
    int B = 0, C = 0, F = 1, T = 0;      // x [B][C][F][T]
    int K = 0;                           // taps of the FIR behind the norm (0: none)
    bool pre = false, post = false, res = false;      // a pre-slope, a post-slope, a residual is given
    bool parts = false;                  // the call is launch_cln_parts
    bool ragged = false;                 // a ragged batch is published (ragged_ctx)
    bool stream = false;                 // a frame-online chunk is open (stream_ctx), and its StreamCtx::H, n, B:
    int H = 0, n = 0, sB = 0;
};

struct ClnLaunch {
    int kernel = 0;                      // ClnKernel
    const char* name = "";               // cln_kernel_name(kernel)
    unsigned gx = 1, gy = 1, gz = 1;
    int block = 256;
    size_t lds = 0;                      // dynamic LDS
    bool res = false;                    // the kernel has a residual operand
};

// One dispatch: everything the launcher needs and the launch log reports
struct ClnChoice {
    int form = CLN_FORM_REFUSED;
    const char* refusal = "";
    int n_launch = 0;
    ClnLaunch launch[3];
    int c0 = 0;              // first column summed and scanned (frame-online: H - back)
    int back = 0;            // history columns the FIR reads: brought in by stream_exchange before the launches
    int WP = 0;              // columns per workgroup of cln_stats_kernel (0: the form has no such launch)
    int W = 0, VPT = 0;      // cln_window_reg_kernel<W, VPT> (0: another form)
    bool takes_res = false;  // a residual handed to the call is added by its own launches
    size_t scratch = 0;      // bytes of per-(b, t) statistics: sum, sq (double), mean, rstd (float), [B][T] each
};

constexpr size_t CLN_LDS_MAX = 60000;        // dynamic LDS the scan and window kernels may ask for
constexpr long CLN_REG_ROWS = 256L * 41;     // most rows C * F of the register form (41 values per thread and frame) ...
constexpr int CLN_REG_CH = 256;              // ... and most channels (its per-channel parameters: one per thread)
constexpr long CLN_WINDOW_ELEMS = 32768;     // most elements C * F * (T - c0) of the one-launch window form

namespace cln_detail {
inline ClnChoice refuse(const char* msg) {
    ClnChoice c;
    c.refusal = msg;
    return c;
}
inline void add(ClnChoice& c, int kernel, unsigned gx, unsigned gy, unsigned gz, size_t lds, bool res = false) {
    ClnLaunch& l = c.launch[c.n_launch++];
    l.kernel = kernel;
    l.name = cln_kernel_name(kernel);
    l.gx = gx; l.gy = gy; l.gz = gz;
    l.lds = lds;
    l.res = res;
}
}  // namespace cln_detail

// The form one launch_cln / launch_cln_parts call reaches.  (One refusal is the launcher's own, it needs the pointers: a FIR in place.)
inline ClnChoice cln_select(const ClnSelIn& in, const ClnTuning& tun) {
    using namespace cln_detail;
    const int B = in.B, C = in.C, T = in.T, K = in.K;
    const long R = (long)C * in.F;
    const bool plain = K <= 0 && !in.pre;      // the plain 2-D form: the only one a residual rides on
    if (in.parts && (in.stream || in.ragged)) return refuse("cLN from epilogue statistics: offline equal-length batches only");
    if (in.res && !plain) return refuse("cLN: the residual rides on the plain 2-D form only");
    if ((size_t)T * 16 > CLN_LDS_MAX) return refuse("utterance too long for the LDS-resident cLN scan");
    ClnChoice c;
    c.scratch = (size_t)B * T * (2 * sizeof(double) + 2 * sizeof(float));
    const unsigned row_groups = (unsigned)((R + 7) / 8);      // cln_apply_kernel: eight rows per workgroup
    if (in.parts) {
        c.form = CLN_FORM_PARTS;
        c.takes_res = true;
        add(c, CLN_K_SCAN_PARTS, B, 1, 1, (size_t)T * 16);
        add(c, CLN_K_APPLY_PLANE, B * C, 1, 1, (size_t)T * 8, true);
        return c;
    }
    if (in.stream) {
        // frame-online chunk: the FIR reaches K - 1 frames back into the history columns of x, whose statistics are re-accumulated
        // from the carried totals in the order of the whole-utterance scan
        if (!(T == in.H + in.n && B == in.sB)) return refuse("cLN: tensor is not a window of the current chunk");
        c.back = K > 0 ? K - 1 : 0;
        c.c0 = in.H - c.back;
        if (c.back > in.H) return refuse("cLN FIR longer than the window's history");
        const int Wn = T - c.c0;      // columns summed
        if (plain && in.n <= 2 && R <= CLN_REG_ROWS && C <= CLN_REG_CH) {
            c.form = CLN_FORM_STREAM_REG;
            c.takes_res = tun.stream_res;
            c.W = in.n;
            c.VPT = 41 * in.n;
            add(c, CLN_K_WINDOW_REG, B, 1, 1, 0, true);
        } else if (R * Wn <= CLN_WINDOW_ELEMS && (K <= 0 || (size_t)R * Wn * 4 + (size_t)T * 24 <= CLN_LDS_MAX)) {
            c.form = CLN_FORM_STREAM_WINDOW;
            add(c, CLN_K_WINDOW, B, 1, 1, (size_t)T * 24 + (K > 0 ? (size_t)R * Wn * 4 : 0));
        } else {
            c.form = CLN_FORM_STREAM_ROWS;
            c.WP = 1;
            while (c.WP < Wn && c.WP < 64) c.WP <<= 1;
            add(c, CLN_K_STATS, (Wn + c.WP - 1) / c.WP, B, 1, 0);
            add(c, CLN_K_SCAN, B, 1, 1, (size_t)T * 16);
            add(c, CLN_K_APPLY, (in.n + 255) / 256, row_groups, B, 0);
        }
        if (in.res && !c.takes_res) return refuse("frame-online cLN: the residual rides on the register form only (ask cln_stream_takes_res first)");
        return c;
    }
    c.WP = 64;
    add(c, CLN_K_STATS, (T + 63) / 64, B, 1, 0);
    add(c, CLN_K_SCAN, B, 1, 1, (size_t)T * 16);
    if (plain && (tun.plane || in.res)) {
        c.form = CLN_FORM_PLANE;
        add(c, CLN_K_APPLY_PLANE, B * C, 1, 1, (size_t)T * 8, true);
    } else {
        c.form = CLN_FORM_ROWS;
        add(c, CLN_K_APPLY, (T + 255) / 256, row_groups, B, 0);
    }
    c.takes_res = plain;
    return c;
}

// Does a frame-online chunk of H + n columns, batch B, add the residual of a plain 2-D norm on [C][F] inside the norm's own launch?
inline bool cln_chunk_takes_res(int B, int C, int F, int H, int n, const ClnTuning& tun) {
    ClnSelIn in;
    in.B = in.sB = B; in.C = C; in.F = F;
    in.T = H + n;
    in.post = true;
    in.stream = true;
    in.H = H; in.n = n;
    return cln_select(in, tun).takes_res;
}

}  // namespace se

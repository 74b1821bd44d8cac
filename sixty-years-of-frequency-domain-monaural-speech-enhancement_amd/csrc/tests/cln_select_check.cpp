// Stand-alone host program over cln_select.h, meant for `-fsanitize=address,undefined` (make cln_select_check): no device code,
// not loaded into anything.  One hand-written call per form of the cumulative LayerNorm's ladder - offline plane and row apply, the
// epilogue-sums form, the register form for one and two frames, the window form with and without a FIR, the three-launch form - with
// the grid and LDS of every launch, both sides of each threshold, the switches, and the calls the ladder refuses, each with its own
// message and no launch.  Exit status 0 and "ok" when everything holds.
#include "../cln_select.h"
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

static ClnSelIn offline(int B, int C, int F, int T, int K = 0, bool pre = false, bool res = false) {
    ClnSelIn in;
    in.B = B; in.C = C; in.F = F; in.T = T; in.K = K;
    in.pre = pre; in.post = !pre; in.res = res;
    return in;
}
// a chunk of n new frames behind H history columns
static ClnSelIn chunk(int B, int C, int F, int H, int n, int K = 0, bool pre = false, bool res = false) {
    ClnSelIn in = offline(B, C, F, H + n, K, pre, res);
    in.stream = true;
    in.H = H; in.n = n; in.sB = B;
    return in;
}
static bool launch_is(const ClnLaunch& l, int kernel, const char* name, unsigned gx, unsigned gy, unsigned gz, size_t lds, bool res = false) {
    return l.kernel == kernel && !std::strcmp(l.name, name) && l.gx == gx && l.gy == gy && l.gz == gz && l.block == 256 && l.lds == lds && l.res == res;
}
static bool refused(const ClnChoice& c, const char* word) {
    return c.form == CLN_FORM_REFUSED && c.n_launch == 0 && !c.takes_res && std::strstr(c.refusal, word);
}

int main() {
    const ClnTuning tun;
    ClnTuning noplane, nores;
    noplane.plane = false;
    nores.stream_res = false;

    // ---- offline: statistics (64 columns per workgroup), scan, plane apply; the residual rides on the plane pass
    ClnChoice c = cln_select(offline(2, 5, 7, 401, 0, false, true), tun);
    EXPECT(c.form == CLN_FORM_PLANE && c.n_launch == 3 && !*c.refusal && c.takes_res && c.c0 == 0 && c.back == 0 && c.WP == 64 && c.W == 0 && c.VPT == 0);
    EXPECT(c.scratch == (size_t)2 * 401 * 24);
    EXPECT(launch_is(c.launch[0], CLN_K_STATS, "cln_stats", 7, 2, 1, 0) && launch_is(c.launch[1], CLN_K_SCAN, "cln_scan", 2, 1, 1, 16 * 401));
    EXPECT(launch_is(c.launch[2], CLN_K_APPLY_PLANE, "cln_apply_plane", 10, 1, 1, 8 * 401, true));
    // ---- ... row apply behind a pre-slope or a FIR, or with the plane pass switched off (a residual still takes the plane pass)
    c = cln_select(offline(2, 5, 7, 401, 5, true), tun);
    EXPECT(c.form == CLN_FORM_ROWS && c.n_launch == 3 && !c.takes_res && launch_is(c.launch[2], CLN_K_APPLY, "cln_apply", 2, 5, 2, 0));
    EXPECT(cln_select(offline(2, 5, 7, 401, 0, true), tun).form == CLN_FORM_ROWS);
    EXPECT(cln_select(offline(2, 5, 7, 401), noplane).form == CLN_FORM_ROWS && cln_select(offline(2, 5, 7, 401, 0, false, true), noplane).form == CLN_FORM_PLANE);
    EXPECT(cln_select(offline(1, 1, 1, 3750), tun).form == CLN_FORM_PLANE);
    // ---- the sums of the producing conv's epilogue: scan of the parts, plane apply
    ClnSelIn p = offline(2, 6, 161, 401, 0, false, true);
    p.parts = true;
    c = cln_select(p, noplane);
    EXPECT(c.form == CLN_FORM_PARTS && c.n_launch == 2 && c.takes_res && c.WP == 0 && c.scratch == (size_t)2 * 401 * 24);
    EXPECT(launch_is(c.launch[0], CLN_K_SCAN_PARTS, "cln_scan_parts", 2, 1, 1, 16 * 401) && launch_is(c.launch[1], CLN_K_APPLY_PLANE, "cln_apply_plane", 12, 1, 1, 8 * 401, true));

    // ---- frame-online: one or two new frames of at most 256 x 41 rows and 256 channels from registers
    c = cln_select(chunk(2, 64, 161, 8, 1, 0, false, true), tun);
    EXPECT(c.form == CLN_FORM_STREAM_REG && c.n_launch == 1 && c.takes_res && c.c0 == 8 && c.W == 1 && c.VPT == 41 && c.WP == 0);
    EXPECT(launch_is(c.launch[0], CLN_K_WINDOW_REG, "cln_window_reg", 2, 1, 1, 0, true));
    c = cln_select(chunk(2, 64, 164, 8, 2), tun);
    EXPECT(c.form == CLN_FORM_STREAM_REG && c.W == 2 && c.VPT == 82);
    // (the switch takes the residual off it, not the form)
    c = cln_select(chunk(2, 64, 161, 8, 1), nores);
    EXPECT(c.form == CLN_FORM_STREAM_REG && !c.takes_res && c.n_launch == 1);
    EXPECT(cln_chunk_takes_res(2, 64, 161, 8, 2, tun) && !cln_chunk_takes_res(2, 64, 161, 8, 2, nores) && !cln_chunk_takes_res(2, 64, 161, 8, 3, tun));
    EXPECT(cln_chunk_takes_res(1, 256, 41, 8, 1, tun) && !cln_chunk_takes_res(1, 257, 1, 8, 1, tun) && !cln_chunk_takes_res(1, 64, 165, 8, 1, tun));
    // ---- a small window in one launch: R (T - c0) <= 32768, with a FIR the normalised window in LDS too
    c = cln_select(chunk(2, 66, 161, 8, 1), tun);      // R > 256 * 41
    EXPECT(c.form == CLN_FORM_STREAM_WINDOW && !c.takes_res && c.c0 == 8 && c.W == 0 && launch_is(c.launch[0], CLN_K_WINDOW, "cln_window", 2, 1, 1, 24 * 9));
    EXPECT(cln_select(chunk(2, 8, 20, 8, 3), tun).form == CLN_FORM_STREAM_WINDOW);
    c = cln_select(chunk(2, 64, 1, 62, 16, 63, true), tun);
    EXPECT(c.form == CLN_FORM_STREAM_WINDOW && c.back == 62 && c.c0 == 0 && c.launch[0].lds == (size_t)24 * 78 + 4 * 64 * 78);
    EXPECT(cln_select(chunk(1, 64, 32, 8, 16), tun).form == CLN_FORM_STREAM_WINDOW && cln_select(chunk(1, 64, 32, 8, 17), tun).form == CLN_FORM_STREAM_ROWS);
    // (a FIR window either side of the LDS limit: 4 R W + 24 T = 59948 / 60232)
    EXPECT(cln_select(chunk(1, 205, 1, 8, 64, 8, true), tun).form == CLN_FORM_STREAM_WINDOW && cln_select(chunk(1, 206, 1, 8, 64, 8, true), tun).form == CLN_FORM_STREAM_ROWS);
    // ---- the three launches: statistics over the new columns (WP = their number rounded up to a power of two, at most 64)
    c = cln_select(chunk(2, 64, 33, 8, 64), tun);
    EXPECT(c.form == CLN_FORM_STREAM_ROWS && c.n_launch == 3 && c.c0 == 8 && c.WP == 64 && !c.takes_res);
    EXPECT(launch_is(c.launch[0], CLN_K_STATS, "cln_stats", 1, 2, 1, 0) && launch_is(c.launch[1], CLN_K_SCAN, "cln_scan", 2, 1, 1, 16 * 72));
    EXPECT(launch_is(c.launch[2], CLN_K_APPLY, "cln_apply", 1, 264, 2, 0));
    c = cln_select(chunk(1, 600, 1, 8, 64, 7, true), tun);
    EXPECT(c.form == CLN_FORM_STREAM_ROWS && c.back == 6 && c.c0 == 2 && c.WP == 64 && c.launch[0].gx == 2 && c.launch[2].gy == 75);
    c = cln_select(chunk(1, 256, 42, 8, 5), tun);
    EXPECT(c.form == CLN_FORM_STREAM_ROWS && c.WP == 8 && c.launch[0].gx == 1);

    // ---- the refusals: their messages, no launch
    EXPECT(refused(cln_select(offline(1, 1, 1, 8, 3, false, true), tun), "the residual rides on the plain 2-D form only"));
    EXPECT(refused(cln_select(offline(1, 1, 1, 8, 0, true, true), tun), "the residual rides on the plain 2-D form only"));
    EXPECT(refused(cln_select(offline(1, 1, 1, 3751), tun), "utterance too long for the LDS-resident cLN scan"));
    ClnSelIn w = chunk(2, 4, 7, 8, 1);
    w.T = 10;
    EXPECT(refused(cln_select(w, tun), "tensor is not a window of the current chunk"));
    w = chunk(2, 4, 7, 8, 1);
    w.sB = 3;
    EXPECT(refused(cln_select(w, tun), "tensor is not a window of the current chunk"));
    EXPECT(refused(cln_select(chunk(2, 64, 1, 8, 1, 10, true), tun), "cLN FIR longer than the window's history"));
    EXPECT(cln_select(chunk(2, 64, 1, 8, 1, 9, true), tun).c0 == 0);
    EXPECT(refused(cln_select(chunk(2, 4, 7, 8, 3, 0, false, true), tun), "the residual rides on the register form only"));
    EXPECT(refused(cln_select(chunk(2, 4, 7, 8, 1, 0, false, true), nores), "the residual rides on the register form only"));
    p = offline(2, 6, 7, 40);
    p.parts = true;
    p.ragged = true;
    EXPECT(refused(cln_select(p, tun), "offline equal-length batches only"));
    p = chunk(2, 6, 7, 8, 1);
    p.parts = true;
    EXPECT(refused(cln_select(p, tun), "offline equal-length batches only"));
    p = offline(2, 6, 7, 3751);
    p.parts = true;
    EXPECT(refused(cln_select(p, tun), "utterance too long"));
    EXPECT(!std::strcmp(cln_form_name(CLN_FORM_STREAM_REG), "stream_reg") && !std::strcmp(cln_form_name(CLN_FORM_REFUSED), "refused") &&
           !std::strcmp(cln_kernel_name(CLN_K_WINDOW_REG), "cln_window_reg") && !*cln_kernel_name(7));
    (void)cln_tuning_env();

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}

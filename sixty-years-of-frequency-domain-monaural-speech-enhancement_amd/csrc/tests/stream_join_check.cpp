// Stand-alone host program over stream_join.h, meant for `-fsanitize=address,undefined` (make stream_join_check): no device code, not
// loaded into anything.  Two things:
//   - stream_left_edge_frames() against a brute-force walk: a stream is fed sample by sample (and in pieces of 37) with the counters
//     the engine keeps, and after every push each index expression that tests against position 0 - the STFT's reflection and its
//     fast-path test, stream_keep_from()'s clamp, the lowest frame the iSTFT overlap-adds into a sample still to be written, the first
//     chunk - is evaluated for everything a later launch can reach.  The threshold is one more than the highest t_done at which any of
//     them still fires;
//   - snap_join_plan(): shifts, the joined window and its per-part columns for parts in phase, and every refusal, each for the defect
//     it has, naming the field and both values.
// Exit status 0 and "ok" when everything holds.
#include "../stream_join.h"
#include "../stream_window.h"
#include <cstdio>

using namespace se;

static int failures = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("line %d: %s\n", __LINE__, #c);                  \
            ++failures;                                                  \
        }                                                                \
    } while (0)

static bool has(const std::string& why, const char* word) {
    if (why.find(word) == std::string::npos) std::printf("  got '%s', wanted '%s'\n", why.c_str(), word);
    return why.find(word) != std::string::npos;
}

// ---- the counters of a stream that has received n_total samples (se_stream_push: every frame whose last sample has arrived is
// transformed, every sample below (t_done - lag) hop - n_fft/2 emitted)
struct Pos {
    int n_total = 0, t_done = 0, o_done = 0;
};
static void push(Pos& s, int n_new, int N, int hop, int lag) {
    s.n_total += n_new;
    const int t_avail = s.n_total > N / 2 ? (s.n_total - N / 2 - 1) / hop + 1 : 0;
    s.t_done = std::max(s.t_done, t_avail);
    const int o_hi = std::min(s.n_total, (s.t_done - lag) * hop - N / 2);
    if (o_hi > s.o_done) s.o_done = o_hi;
}

// does anything a launch AFTER this state evaluates test against position 0 and fire?
static bool touches_zero(const Pos& s, int N, int hop) {
    if (s.t_done == 0) return true;                                            // the first chunk is still to come
    for (int t = s.t_done; t < s.t_done + 2 * N / hop + 2; ++t) {              // frames still to be transformed
        if (!(t * hop >= N / 2)) return true;                                  // the fast path's test on the first frame of a pair
        for (int n = 0; n < N; ++n)
            if (t * hop + n - N / 2 < 0) return true;                          // idx < 0: mirrored
    }
    const long a = (long)s.t_done * hop - N / 2, b = (long)s.n_total - N / 2 - 1;
    if (std::min(a, b) < 0) return true;                                       // stream_keep_from clamps
    if (stream_keep_from(N, hop, s.t_done, s.n_total) != (int)(std::min(a, b) & ~3L)) return true;
    for (int o = s.o_done; o < s.o_done + 2 * N; ++o) {                        // samples still to be written
        const int pos = o + N / 2;
        for (int t = pos / hop; pos - t * hop < N; --t)                        // every frame that covers pos
            if (t < 0) return true;                                            // ... one of them lies before frame 0: max(0, .) ends the loop
    }
    return false;
}

static int brute_threshold(int N, int hop, int lag, int piece) {
    Pos s;
    int last_touch = -1;
    bool seen_after[64] = {};
    for (int fed = 0; fed < 40 * hop + 2 * N; fed += piece) {
        push(s, piece, N, hop, lag);
        if (touches_zero(s, N, hop)) last_touch = std::max(last_touch, s.t_done);
        if (s.t_done < 64) seen_after[s.t_done] = true;
    }
    EXPECT(last_touch >= 0 && last_touch < 30 && seen_after[last_touch + 1]);          // the walk went well past it
    return last_touch + 1;
}

// ---- manifests: a group of B rows, n_total samples in, lag 0, as se_stream_save records it
static SnapManifest group(int B, int n_total, int N = 512, int hop = 128, int lag = 0) {
    SnapManifest m;
    m.model = 5; m.flags = 1 << 16; m.n_fft = N; m.hop = hop; m.win = N; m.p_in = 0.5f; m.p_out = 2.f;
    m.batch = B; m.max_chunk = 16; m.first = 0; m.state_B = B;
    Pos s;
    push(s, n_total, N, hop, lag);
    m.n_total = s.n_total; m.t_done = s.t_done; m.o_done = s.o_done;
    m.keep = stream_keep_from(N, hop, s.t_done, s.n_total);
    const int kinds[5] = {SNAP_C, SNAP_HIST, SNAP_H, SNAP_CELL, SNAP_WINDOW};
    const int64_t floats[5] = {1, 7 * 12, 256, 256, (int64_t)m.n_total - m.keep};
    for (int k = 0; k < 5; ++k) {
        SnapSeg sg;
        sg.kind = kinds[k];
        sg.bytes = floats[k] * B * 4;
        m.segs.push_back(sg);
    }
    return m;
}

static std::string plan_of(const std::vector<SnapManifest>& parts, JoinPlan& plan, int lag = 0, const std::string& counts = "") {
    std::vector<const SnapManifest*> p;
    for (const SnapManifest& m : parts) p.push_back(&m);
    return snap_join_plan(p, lag, counts, plan);
}

int main() {
    // ---- the threshold, for the front ends in use: 320 / 160 (CRN, LSTM, GCRN, DPCRN), 512 / 128 (DCCRN; look-ahead 6 with the
    // decoder that looks ahead), and the 400 / 160 front end, whose frames are 512 long (win 400 in n_fft 512) - and as literal 400
    const int fronts[5][2] = {{320, 160}, {512, 128}, {512, 160}, {400, 160}, {512, 256}};
    for (const auto& f : fronts)
        for (int lag : {0, 2, 6})
            for (int piece : {1, 37}) {
                const int want = brute_threshold(f[0], f[1], lag, piece), got = stream_left_edge_frames(f[0], f[1], lag);
                if (want != got) std::printf("  n_fft %d hop %d lag %d piece %d: walk %d, function %d\n", f[0], f[1], lag, piece, want, got);
                EXPECT(want == got);
            }
    EXPECT(stream_left_edge_frames(320, 160, 0) == 1);
    EXPECT(stream_left_edge_frames(512, 128, 0) == 3);
    EXPECT(stream_left_edge_frames(512, 128, 6) == 9);
    EXPECT(stream_left_edge_frames(512, 160, 0) == 3);
    EXPECT(stream_left_edge_frames(400, 160, 0) == 2);

    // ---- parts in phase
    JoinPlan plan;
    {
        const SnapManifest g = group(1, 3701), a = group(2, 3701 - 5 * 128);
        EXPECT(g.t_done - a.t_done == 5 && g.o_done - a.o_done == 640 && g.keep - a.keep == 640);
        EXPECT(plan_of({g, a}, plan).empty());
        EXPECT(plan.shift.size() == 2 && plan.shift[0] == 0 && plan.shift[1] == 640);
        EXPECT(plan.keep == g.keep && plan.live == g.n_total - g.keep && plan.col[0] == 0 && plan.col[1] == 0);
        // ... onto the part that is behind: the shift is negative
        EXPECT(plan_of({a, g}, plan).empty());
        EXPECT(plan.shift[1] == -640 && plan.keep == a.keep && plan.live == a.n_total - a.keep && plan.col[1] == 0);
        // windows of different live lengths: the highest rebased keep wins, the others skip columns
        SnapManifest g8 = g, a12 = a;
        g8.keep -= 8;
        a12.keep -= 12;
        EXPECT(plan_of({g8, a}, plan).empty() && plan.keep == g.keep && plan.col[0] == 8 && plan.col[1] == 0 && plan.live == g.n_total - g.keep);
        EXPECT(plan_of({g8, a12}, plan).empty() && plan.keep == g.keep - 8 && plan.col[0] == 0 && plan.col[1] == 4 &&
               plan.live == g.n_total - g.keep + 8);
        for (size_t p = 0; p < 2; ++p) {          // the columns a part gives lie inside its rows
            const SnapManifest& m = p ? a12 : g8;
            EXPECT(plan.col[p] >= 0 && plan.col[p] + plan.live == m.n_total - m.keep);
        }
        // three parts, two of them with shift 0; one part: a copy
        EXPECT(plan_of({g, group(3, 3701), a}, plan).empty() && plan.shift[1] == 0 && plan.shift[2] == 640);
        EXPECT(plan_of({a}, plan).empty() && plan.shift[0] == 0 && plan.keep == a.keep);
        // equal counters need no left edge: what concat accepts
        EXPECT(plan_of({group(1, 300), group(2, 300)}, plan).empty() && plan.keep == 0 && plan.live == 300);
        // 320 / 160 joins from the first frame on, the look-ahead DCCRN from t_done 9
        EXPECT(plan_of({group(1, 2000, 320, 160), group(1, 2000 - 11 * 160, 320, 160)}, plan).empty() && plan.shift[1] == 1760);
        EXPECT(group(1, 1500, 512, 128, 6).t_done == 10 && group(1, 1500 - 128, 512, 128, 6).t_done == 9);
        EXPECT(plan_of({group(1, 1500, 512, 128, 6), group(1, 1500 - 128, 512, 128, 6)}, plan, 6).empty());
    }

    // ---- refusals
    {
        const SnapManifest g = group(1, 3701), a = group(2, 3701 - 640);
        JoinPlan before;
        EXPECT(plan_of({g, a}, before).empty());
        plan = before;
        EXPECT(has(plan_of({g, group(2, 3701 - 600)}, plan), "n_total 3701 vs 3101, the shift 600 is not a multiple of lcm(hop, 4) = 128"));
        EXPECT(has(plan_of({group(1, 4000, 512, 162), group(1, 4000 - 162, 512, 162)}, plan), "the shift 162 is not a multiple of lcm(hop, 4) = 324"));
        EXPECT(plan.shift == before.shift && plan.keep == before.keep);          // a refusal leaves the plan alone
        SnapManifest m = a;
        m.t_done -= 1;
        EXPECT(has(plan_of({g, m}, plan), "parts[0] and parts[1] are out of phase: n_total - t_done * hop 245 vs 373"));
        m = a;
        m.o_done -= 128;
        EXPECT(has(plan_of({g, m}, plan), "out of phase: n_total - o_done 501 vs 629"));
        // short of the left edge, either side (512 / 128: from t_done 3 on)
        const SnapManifest early = group(1, 512), later = group(1, 512 + 128);
        EXPECT(early.t_done == 2 && later.t_done == 3);
        EXPECT(has(plan_of({later, early}, plan), "parts[1] is short of the left edge: t_done 2, a stream can be rebased from t_done 3 on"));
        EXPECT(has(plan_of({early, later}, plan), "parts[0] is short of the left edge: t_done 2"));
        EXPECT(has(plan_of({group(1, 1500, 512, 128, 6), group(1, 1500 - 256, 512, 128, 6)}, plan, 6), "parts[1] is short of the left edge: t_done 8"));
        EXPECT(plan_of({later, group(2, 512 + 256)}, plan).empty());
        m = a;
        m.first = 1;
        EXPECT(has(plan_of({g, m}, plan), "first 0 vs 1"));
        // absolute time in the state
        m = a;
        m.running = 1;
        EXPECT(has(plan_of({g, m}, plan), "parts[1] is a running-scale stream"));
        EXPECT(has(plan_of({m}, plan), "parts[0] is a running-scale stream"));
        EXPECT(has(plan_of({g, a}, plan, 0, "the norm counts frames"), "cannot be rebased: the norm counts frames"));
        // every other field, named as concat names it
        struct Case { const char* want; void (*mutate)(SnapManifest&); };
        const Case cases[] = {
            {"parts[0] and parts[1] differ: model 5 vs 6", [](SnapManifest& x) { x.model = 6; }},
            {"flags 65536 vs 0", [](SnapManifest& x) { x.flags = 0; }},
            {"n_fft 512 vs 320", [](SnapManifest& x) { x.n_fft = 320; }},
            {"hop 128 vs 160", [](SnapManifest& x) { x.hop = 160; }},
            {"win 512 vs 400", [](SnapManifest& x) { x.win = 400; }},
            {"max_chunk 16 vs 8", [](SnapManifest& x) { x.max_chunk = 8; }},
            {"ring 0 vs 128", [](SnapManifest& x) { x.ring = 128; }},
            {"p_in 0.5", [](SnapManifest& x) { x.p_in = 1.f; }},
            {"p_out 2.0", [](SnapManifest& x) { x.p_out = 1.f; }},
            {"state_B 1 vs 0", [](SnapManifest& x) { x.state_B = 0; }},
            {"segment count 5 vs 4", [](SnapManifest& x) { x.segs.erase(x.segs.begin() + 2); }},
            {"segment 1 hist[0] vs hist[1]", [](SnapManifest& x) { x.segs[1].index = 1; }},
        };
        for (const Case& c : cases) {
            m = a;
            c.mutate(m);
            EXPECT(has(plan_of({g, m}, plan), c.want));
        }
        EXPECT(snap_concat_differs(g, a).find("n_total 3701 vs 3061") == 0);          // concat still refuses what join takes
        EXPECT(snap_concat_differs(g, a, false).empty());
        // a record whose window would start behind its samples (no save writes one)
        plan = before;
        m = a;
        m.keep = m.n_total + 128;
        EXPECT(has(plan_of({g, m}, plan), "the joined window starts behind the samples"));
        std::vector<const SnapManifest*> none;
        EXPECT(has(snap_join_plan(none, 0, "", plan), "n_parts 0"));
        EXPECT(plan.shift == before.shift);
    }
    if (failures == 0) std::printf("ok\n");
    return failures ? 1 : 0;
}

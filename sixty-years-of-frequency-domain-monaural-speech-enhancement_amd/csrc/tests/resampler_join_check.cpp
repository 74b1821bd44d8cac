// Stand-alone host program over resampler_join.h, meant for `-fsanitize=address,undefined` (make resampler_join_check): no device code,
// not loaded into anything.  Four things:
//   - resampler_left_edge() against a brute-force walk: a signal is fed sample by sample (and in pieces of 37) with the counters the
//     StreamResampler keeps, and after every push each index expression that tests against position 0 - the left wing's clamp
//     min(n + 1, .) of resample_taps, the host's max(0, pos - (reach - 2)) - is evaluated for the outputs still to come.  The threshold
//     is one more than the highest next output t at which either still fires;
//   - a rebased signal next to the original: the same pushes release the same counts, the flush computes and emits the same counts,
//     and the history a rebased signal keeps (its origin never moves back) always covers what its next output reads;
//   - the flush identity (int64_t)((double)n * ratio) == n / D and ceil((double)n * ratio) == ceil(n / D) for EVERY n = 0 ... 2^31 - 1,
//     for every D the join accepts (RSJOIN_DECIMATIONS);
//   - rsnap_join_plan(): shifts, the joined history origin and the per-part columns for parts in phase - also parts saved with
//     histories of different lengths - and every refusal, each for the defect it has, with its text.
// Exit status 0 and "ok" when everything holds.
#include "../resampler_join.h"
#include <cstdio>
#include <thread>

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

// ---- the counters of a StreamResampler signal (StreamResampler::push of k_resample.hip, its checks included)
struct Sig {
    int64_t n_total = 0, w0 = 0;
    ResamplePos pos;
};
static int64_t push(const ResamplePlan& p, Sig& s, int64_t n_new) {
    const int64_t n_after = s.n_total + n_new;
    ResamplePos pos = s.pos;
    const int64_t count = resample_advance(p, pos, n_after, INT64_MAX, nullptr, 0);
    // the oldest tap of the first output lies inside the history, and the history fits a buffer row
    EXPECT(count == 0 || std::max<int64_t>(0, (int64_t)resample_pos_of(p, s.pos) - (p.reach - 2)) >= s.w0);
    const int64_t w0_next = std::max<int64_t>(s.w0, n_after - 2 * (int64_t)p.reach);
    EXPECT(w0_next >= s.w0 && n_after - w0_next <= 2 * (int64_t)p.reach && s.n_total - s.w0 <= 2 * (int64_t)p.reach);
    s.w0 = w0_next;
    s.n_total = n_after;
    s.pos = pos;
    return count;
}
// (outputs still to compute, outputs still to emit) of the flush, as StreamResampler::flush forms them
static void flush_counts(const ResamplePlan& p, const Sig& s, int64_t& n_calc, int64_t& n_emit) {
    n_calc = resample_calc_samples(p, s.n_total) - s.pos.t;
    n_emit = (int64_t)std::ceil((double)s.n_total * p.ratio) - s.pos.t;
}

// does anything a launch AFTER this state evaluates test against position 0 and fire?
static bool touches_zero(const ResamplePlan& p, const Sig& s) {
    for (int64_t t = s.pos.t; t < s.pos.t + 4 * p.reach; ++t) {                  // outputs still to be computed
        const double tr = (double)t * p.inc;
        const int n = (int)tr;
        const double frac = p.scale * (tr - n);
        EXPECT(frac == 0.0);                                                     // integer decimation: the table offset is constant
        const int offset = (int)(frac * RS_BITS);
        if (n + 1 < (RS_NWIN - offset) / p.index_step) return true;              // min(n + 1, .): the left wing is cut at sample 0
        if ((int64_t)tr - (p.reach - 2) < 0) return true;                        // max(0, pos - (reach - 2)) clamps
    }
    return false;
}

// fed in pieces of 1 every next output t is visited between two pushes: the threshold is one more than the highest t that still fires.
// Fed in larger pieces only some t are visited; each of them fires exactly when it lies below `edge`.
static int64_t brute_threshold(const ResamplePlan& p, int piece, int64_t edge) {
    Sig s;
    int64_t last_touch = -1, t_max = 0;
    for (int fed = 0; fed < 12 * p.reach; fed += piece) {
        push(p, s, piece);
        const bool fires = touches_zero(p, s);
        EXPECT(fires == (s.pos.t < edge));
        if (fires) last_touch = std::max(last_touch, s.pos.t);
        EXPECT(s.pos.t - t_max <= 1 || piece > 1);
        t_max = s.pos.t;
    }
    EXPECT(last_touch >= 0 && t_max > last_touch + 8);                           // the walk went well past it
    return last_touch + 1;
}

// lengths n in [lo, hi) at which the flush's two double expressions are not n / D and ceil(n / D).  Unsigned counters; ceil(v) of a
// finite v >= 0 below 2^63 as trunc(v) + (v > trunc(v)), which is exact
static uint64_t identity_misses(int D, double ratio, uint64_t lo, uint64_t hi) {
    uint64_t bad = 0, q = lo / (uint64_t)D, r = lo % (uint64_t)D;                     // n = q * D + r
    for (uint64_t n = lo; n < hi; ++n) {
        const double v = (double)(int64_t)n * ratio;
        const uint64_t fl = (uint64_t)(int64_t)v;
        bad += (fl != q) | (fl + (v > (double)(int64_t)fl) != q + (r != 0));
        if (++r == (uint64_t)D) {
            r = 0;
            ++q;
        }
    }
    return bad;
}

// a signal saved after n samples, rebased by s, continued next to the original: the same counts out of every push and the flush
static void rebased_runs_alike(int sr_in, int64_t n_save, int64_t s, int64_t rest) {
    const ResamplePlan p = resample_plan(sr_in, 16000);
    const int64_t D = sr_in / 16000;
    Sig a;
    push(p, a, n_save);
    Sig b = a;
    b.n_total += s; b.w0 += s; b.pos.t += s / D; b.pos.acc = (double)b.pos.t * p.inc;
    const int pieces[6] = {1, 37, 1000, 3, 481, 2000};
    int64_t fed = 0;
    for (int k = 0; fed < rest; ++k) {
        const int64_t m = std::min<int64_t>(pieces[k % 6], rest - fed);
        EXPECT(push(p, a, m) == push(p, b, m));
        EXPECT(b.n_total - a.n_total == s && b.pos.t - a.pos.t == s / D && b.w0 >= a.w0 + s);
        fed += m;
    }
    EXPECT(b.w0 == a.w0 + s);                                                    // ... and the same history once the window has passed the origin
    int64_t ca, ea, cb, eb;
    flush_counts(p, a, ca, ea);
    flush_counts(p, b, cb, eb);
    EXPECT(ca == cb && ea == eb && ca >= 0 && ea >= ca);
}

// ---- records: a group of B rows, n_total samples in, as se_resampler_save writes it
static ResamplerManifest group(int B, int64_t n_total, int sr_in = 48000, int sr_out = 16000) {
    ResamplerManifest m;
    m.sr_in = sr_in; m.sr_out = sr_out; m.batch = B; m.n_total = n_total;
    if (sr_in == sr_out) {
        m.w0 = m.t = n_total;
        m.acc_bits = rsnap_bits_of(0.0);
        return m;
    }
    const ResamplePlan p = resample_plan(sr_in, sr_out);
    Sig s;
    push(p, s, n_total);
    m.w0 = s.w0; m.t = s.pos.t;
    m.acc_bits = rsnap_bits_of(s.pos.acc);
    return m;
}

static std::string plan_of(const std::vector<ResamplerManifest>& parts, ResamplerJoinPlan& plan) {
    std::vector<const ResamplerManifest*> p;
    for (const ResamplerManifest& m : parts) p.push_back(&m);
    return rsnap_join_plan(p, plan);
}

int main() {
    // ---- the threshold, 48 -> 16 and 32 -> 16 kHz
    for (int sr_in : {48000, 32000}) {
        const ResamplePlan p = resample_plan(sr_in, 16000);
        EXPECT(p.exact && p.inc == (double)(sr_in / 16000));
        const int64_t got = resampler_left_edge(p), want = brute_threshold(p, 1, got);
        if (want != got) std::printf("  %d -> 16000 Hz: walk %ld, function %ld\n", sr_in, (long)want, (long)got);
        EXPECT(want == got);
        EXPECT(brute_threshold(p, 37, got) <= got);
    }
    EXPECT(resample_plan(48000, 16000).reach == 193 && resampler_left_edge(resample_plan(48000, 16000)) == 64);
    EXPECT(resample_plan(32000, 16000).reach == 129 && resampler_left_edge(resample_plan(32000, 16000)) == 64);
    // the first n_in at which a signal is past the edge: output 63 is released by sample 63 * D + reach
    EXPECT(group(1, 382).t == 63 && group(1, 383).t == 64 && group(1, 383).w0 == 0 && group(1, 387).w0 == 1);
    EXPECT(group(1, 255, 32000).t == 63 && group(1, 256, 32000).t == 64 && group(1, 256, 32000).w0 == 0);

    // ---- a rebased signal runs like the original: saved right at the edge (history shorter than 2 * reach), and well past it
    for (int64_t n : {383, 385, 386, 700, 5003})
        for (int64_t s : {3, 480, 2400, 480000}) rebased_runs_alike(48000, n, s, 9001);
    for (int64_t n : {256, 257, 258, 4001})
        for (int64_t s : {2, 320, 1600}) rebased_runs_alike(32000, n, s, 6002);

    // ---- the flush identity over every length, for every D the join accepts
    for (int D : RSJOIN_DECIMATIONS) {
        const double ratio = (double)16000 / (16000 * D);
        EXPECT(ratio == (double)8000 / (8000 * D) && ratio == (double)1 / D);          // the correctly rounded 1 / D, whatever the rates
        EXPECT(ratio == resample_plan(16000 * D, 16000).ratio);
        // (eight slices of the range side by side; std::ceil itself on every 4099th length)
        uint64_t bad = 0, part[8] = {};
        std::vector<std::thread> pool;
        const uint64_t end = (uint64_t)RSNAP_MAX_COUNT + 1, step = end / 8;
        for (int k = 0; k < 8; ++k) pool.emplace_back([&, k] { part[k] = identity_misses(D, ratio, k * step, k == 7 ? end : (k + 1) * step); });
        for (auto& t : pool) t.join();
        for (uint64_t v : part) bad += v;
        for (int64_t n = 0; n <= RSNAP_MAX_COUNT; n += 4099)
            bad += (int64_t)std::ceil((double)n * ratio) != (n + D - 1) / D || resample_calc_samples(resample_plan(16000 * D, 16000), n) != n / D;
        if (bad) std::printf("  D = %d: %ld lengths whose flush counts are not n / D and ceil(n / D)\n", D, (long)bad);
        EXPECT(bad == 0);
    }
    EXPECT(rsjoin_walked(1) && rsjoin_walked(2) && rsjoin_walked(3) && !rsjoin_walked(4) && !rsjoin_walked(0) && !rsjoin_walked(6));

    // ---- parts in phase
    ResamplerJoinPlan plan;
    {
        const ResamplerManifest g = group(2, 5003), a = group(1, 5003 - 5 * 480);
        EXPECT(g.t - a.t == 800 && g.w0 - a.w0 == 2400 && g.w0 == 5003 - 386);
        EXPECT(plan_of({g, a}, plan).empty());
        EXPECT(plan.shift.size() == 2 && plan.shift[0] == 0 && plan.shift[1] == 2400);
        EXPECT(plan.w0 == g.w0 && plan.live == 386 && plan.col[0] == 0 && plan.col[1] == 0);
        const ResamplerManifest j = rsnap_joined(g, plan, 3);
        EXPECT(j.batch == 3 && j.n_total == g.n_total && j.t == g.t && j.w0 == g.w0 && j.acc_bits == g.acc_bits && rsnap_check(j).empty());
        // ... onto the part that is behind: the shift is negative
        EXPECT(plan_of({a, g}, plan).empty());
        EXPECT(plan.shift[1] == -2400 && plan.w0 == a.w0 && plan.live == 386 && plan.col[1] == 0);
        // any multiple of D, not only whole hops
        EXPECT(plan_of({g, group(1, 5003 - 3)}, plan).empty() && plan.shift[1] == 3);
        // histories of different lengths: the highest rebased origin wins, the others skip columns
        ResamplerManifest g8 = g, a100 = a;
        g8.w0 += 8;
        a100.w0 += 100;
        EXPECT(plan_of({g8, a}, plan).empty() && plan.w0 == g.w0 + 8 && plan.col[0] == 0 && plan.col[1] == 8 && plan.live == 378);
        EXPECT(plan_of({g8, a100}, plan).empty() && plan.w0 == g.w0 + 100 && plan.col[0] == 92 && plan.col[1] == 0 && plan.live == 286);
        EXPECT(plan_of({a100, g8}, plan).empty() && plan.w0 == a.w0 + 100 && plan.col[0] == 0 && plan.col[1] == 92 && plan.live == 286);
        for (size_t p = 0; p < 2; ++p) {          // the columns a part gives lie inside its rows
            const ResamplerManifest& m = p ? g8 : a100;
            EXPECT(plan.col[p] >= 0 && plan.col[p] + plan.live == rsnap_keep(m));
        }
        // a part saved right at the edge, its history still from sample 0: rebased it starts later than a signal of that length would
        const ResamplerManifest e = group(1, 383), ge = group(2, 383 + 480);
        EXPECT(e.w0 == 0 && ge.w0 == 477);
        EXPECT(plan_of({ge, e}, plan).empty() && plan.w0 == 480 && plan.col[0] == 3 && plan.col[1] == 0 && plan.live == 383);
        // three parts, two of them with shift 0; one part: a copy
        EXPECT(plan_of({g, group(3, 5003), a}, plan).empty() && plan.shift[1] == 0 && plan.shift[2] == 2400);
        EXPECT(plan_of({a}, plan).empty() && plan.shift[0] == 0 && plan.w0 == a.w0 && plan.col[0] == 0 && plan.live == rsnap_keep(a));
        EXPECT(rsnap_joined(a, plan, 1).acc_bits == a.acc_bits);
        // equal counters need no left edge: what concat accepts
        EXPECT(plan_of({group(1, 100), group(2, 100)}, plan).empty() && plan.w0 == 0 && plan.live == 100);
        // 32 -> 16 kHz
        EXPECT(plan_of({group(2, 4001, 32000), group(1, 4001 - 5 * 320, 32000)}, plan).empty() && plan.shift[1] == 1600 && plan.live == 258);
        // pass-through: counters only, any shift
        EXPECT(plan_of({group(2, 900, 16000), group(1, 893, 16000)}, plan).empty() && plan.shift[1] == 7 && plan.live == 0 && plan.w0 == 900);
        EXPECT(plan_of({group(2, 900, 16000), group(1, 0, 16000)}, plan).empty());
    }

    // ---- refusals
    {
        const ResamplerManifest g = group(2, 5003), a = group(1, 5003 - 2400);
        ResamplerJoinPlan before;
        EXPECT(plan_of({g, a}, before).empty());
        plan = before;
        EXPECT(has(plan_of({g, group(1, 5003 - 2399)}, plan),
                   "parts[0] and parts[1] are out of phase: n_in 5003 vs 2604, the shift 2399 is not a multiple of sr_in / sr_out = 3"));
        EXPECT(plan.shift == before.shift && plan.w0 == before.w0);               // a refusal leaves the plan alone
        ResamplerManifest m = a;
        m.t -= 1;
        EXPECT(has(plan_of({g, m}, plan), "parts[0] and parts[1] are out of phase: n_in - n_out * 3 191 vs 194"));
        // short of the left edge, either side (from n_out 64 on)
        const ResamplerManifest early = group(1, 382), later = group(1, 382 + 3);
        EXPECT(early.t == 63 && later.t == 64);
        EXPECT(has(plan_of({later, early}, plan),
                   "parts[1] is short of the left edge: n_out 63, a signal can be rebased from n_out 64 on (48000 -> 16000 Hz)"));
        EXPECT(has(plan_of({early, later}, plan), "parts[0] is short of the left edge: n_out 63"));
        EXPECT(plan_of({later, group(2, 382 + 6)}, plan).empty());
        EXPECT(has(plan_of({group(1, 255, 32000), group(1, 257, 32000)}, plan), "parts[0] is short of the left edge: n_out 63, a signal can be rebased from n_out 64 on (32000 -> 16000 Hz)"));
        // ratios that cannot be rebased
        EXPECT(has(plan_of({group(1, 5000, 44100), group(1, 4000, 44100)}, plan),
                   "44100 -> 16000 Hz cannot be rebased: the read position is a running float64 sum from the signal's start (sr_in % sr_out != 0)"));
        EXPECT(has(plan_of({group(1, 500, 16000, 48000)}, plan), "16000 -> 48000 Hz cannot be rebased: the read position is a running float64 sum"));
        EXPECT(has(plan_of({group(1, 5000, 64000), group(1, 4000, 64000)}, plan), "64000 -> 16000 Hz cannot be rebased: integer decimation by 4 is not among"));
        // rates, named as concat names them
        EXPECT(has(plan_of({g, group(1, 2603, 44100)}, plan), "parts[0] and parts[1] differ: sr_in 48000 vs 44100"));
        EXPECT(has(plan_of({g, a, group(1, 2603, 48000, 8000)}, plan), "parts[0] and parts[2] differ: sr_out 16000 vs 8000"));
        EXPECT(rsnap_concat_differs(g, a).find("n_in 5003 vs 2603") == 0);        // concat still refuses what join takes
        // a record whose history would start behind its samples (no save writes one)
        m = a;
        m.w0 = m.n_total;
        ResamplerManifest gm = g;
        gm.w0 = g.n_total - 10;
        EXPECT(plan_of({gm, m}, plan).empty() && plan.live == 0);
        plan = before;
        m.w0 = m.n_total + 4;
        EXPECT(has(plan_of({g, m}, plan), "the joined history starts behind the samples"));
        std::vector<const ResamplerManifest*> none;
        EXPECT(has(rsnap_join_plan(none, plan), "n_parts 0"));
        EXPECT(plan.shift == before.shift && plan.live == before.live);
    }
    if (failures == 0) std::printf("ok\n");
    return failures ? 1 : 0;
}

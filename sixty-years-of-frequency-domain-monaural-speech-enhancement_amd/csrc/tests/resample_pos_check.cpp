// Stand-alone host program over resample_pos.h, meant for `-fsanitize=address,undefined` (make resample_pos_check): no device
// code, not loaded into anything.  It replays the stateful resampler's host side - the carried read position, the outputs a
// push releases, the history window and the taps the kernel would index in it - for several ratios and push schedules, and
// checks every index against the window, the released counts against the stateless count, and the positions against one
// offline walk.  Exit status 0 and "ok" when everything holds.
#include "../resample_pos.h"
#include <algorithm>
#include <climits>
#include <cstdio>
#include <vector>

using namespace se;

static int failures = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("line %d: %s\n", __LINE__, #c);                  \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// the offline launcher's positions for a signal of n samples
static std::vector<double> offline_positions(const ResamplePlan& p, int64_t n) {
    std::vector<double> tr((size_t)resample_calc_samples(p, n));
    double acc = 0.0;
    for (size_t i = 0; i < tr.size(); ++i) {
        tr[i] = p.exact ? (double)i * p.inc : acc;
        acc += p.inc;
    }
    return tr;
}

// the taps one output indexes: [lo, hi] by absolute position, clamped as the kernel clamps them
static void tap_range(const ResamplePlan& p, double tr, int64_t n_in, int64_t& lo, int64_t& hi) {
    const int64_t n = (int64_t)tr;
    const double frac = p.scale * (tr - (double)n);
    const int offset = (int)(frac * RS_BITS), offset2 = (int)((p.scale - frac) * RS_BITS);
    const int64_t i_max = std::min<int64_t>(n + 1, (RS_NWIN - offset) / p.index_step);
    const int64_t k_max = std::min<int64_t>(n_in - n - 1, (RS_NWIN - offset2) / p.index_step);
    lo = n - (i_max - 1);
    hi = n + std::max<int64_t>(k_max, 0);
}

static void run(int sr_in, int sr_out, int64_t n, const std::vector<int>& schedule) {
    const ResamplePlan p = resample_plan(sr_in, sr_out);
    const std::vector<double> ref = offline_positions(p, n);
    const int64_t hist = 2 * (int64_t)p.reach;
    std::vector<float> window((size_t)hist, 0.f);            // stands for a history buffer: indexed, never valued
    ResamplePos pos;
    int64_t total = 0, w0 = 0, emitted = 0;
    size_t step = 0;
    std::vector<double> tr;
    while (total < n) {
        const int piece = (int)std::min<int64_t>(schedule[std::min(step++, schedule.size() - 1)], n - total);
        const int64_t after = total + piece;
        ResamplePos probe = pos;
        const int64_t count = resample_advance(p, probe, after, INT64_MAX, nullptr, 0);
        tr.assign((size_t)count + 1, -1.0);                  // one spare slot: the walk must not touch it
        const int64_t k = resample_advance(p, pos, after, INT64_MAX, tr.data(), count);
        EXPECT(k == count && tr[(size_t)count] == -1.0);
        EXPECT(count <= (int64_t)((double)piece * p.ratio) + 2);
        EXPECT(resample_ready(p, after) - resample_ready(p, total) == count);
        for (int64_t j = 0; j < count; ++j) {
            EXPECT((size_t)(emitted + j) < ref.size() && tr[(size_t)j] == ref[(size_t)(emitted + j)]);
            int64_t lo, hi;
            tap_range(p, tr[(size_t)j], after, lo, hi);
            EXPECT(lo >= w0 && hi < after);                  // inside [history | new samples]
            if (lo < total) window[(size_t)(lo - w0)] += 1.f;     // the oldest tap lands inside the history buffer
        }
        emitted += count;
        const int64_t w0_next = std::max<int64_t>(0, after - hist);
        EXPECT(w0_next >= w0 && after - w0_next <= hist);
        w0 = w0_next;
        total = after;
    }
    // flush: everything up to floor(n * ratio), right wing cut at n
    const int64_t n_calc = resample_calc_samples(p, n) - emitted;
    EXPECT(n_calc >= 0 && n_calc <= (int64_t)((double)(p.reach + 1) * p.ratio) + 2);
    tr.assign((size_t)std::max<int64_t>(n_calc, 0), 0.0);
    const int64_t k = resample_advance(p, pos, total + p.reach, emitted + n_calc, tr.data(), n_calc);
    EXPECT(k == n_calc);
    for (int64_t j = 0; j < k; ++j) {
        EXPECT(tr[(size_t)j] == ref[(size_t)(emitted + j)]);
        int64_t lo, hi;
        tap_range(p, tr[(size_t)j], total, lo, hi);
        EXPECT(lo >= w0 && hi < total);
        window[(size_t)(lo - w0)] += 1.f;
    }
    EXPECT(emitted + k == (int64_t)ref.size());
}

int main() {
    const int rates[][2] = {{48000, 16000}, {32000, 16000}, {44100, 16000}, {16000, 48000}, {22050, 16000}, {96000, 16000}, {8000, 16000}};
    const std::vector<std::vector<int>> schedules = {{1}, {7}, {480}, {4801}, {1, 191, 2, 1000, 4801}, {193}, {386, 1}};
    for (const auto& r : rates)
        for (const auto& s : schedules)
            for (int64_t n : {1, 100, 192, 193, 194, 579, 4801}) run(r[0], r[1], n, s);
    // the stateless count: monotone, zero below the reach, never above floor(n * ratio), defined up to the int range
    for (const auto& r : rates) {
        const ResamplePlan p = resample_plan(r[0], r[1]);
        int64_t prev = 0;
        for (int64_t n = 0; n < 3000; ++n) {
            const int64_t k = resample_ready(p, n);
            EXPECT(k >= prev && k <= resample_calc_samples(p, n) && (n > p.reach || k == 0));
            prev = k;
        }
        if (p.exact) EXPECT(resample_ready(p, INT_MAX) > 0 && resample_ready(p, INT_MAX) <= resample_calc_samples(p, INT_MAX));
    }
    if (failures) std::printf("%d checks failed\n", failures);
    else std::puts("ok");
    return failures ? 1 : 0;
}

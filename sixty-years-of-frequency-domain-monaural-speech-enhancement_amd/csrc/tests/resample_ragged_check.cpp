// Stand-alone host program over resample_ragged.h, meant for `-fsanitize=address,undefined` (make resample_ragged_check): no device
// code, not loaded into anything.  It checks the row sizes of se_resample_ragged against plain arithmetic for a grid of lengths and
// rates, the split of the rows over launches for batches around the per-launch bound, every refusal with its reason, and that the
// shared position table, however it was grown, holds the doubles one offline walk computes.  With arguments
// `sizes SR_IN SR_OUT N...` it prints "n_calc n_out" per length instead (the caller compares them with se_resample_samples).
// Exit status 0 and "ok" when everything holds.
#include "../resample_ragged.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static RaggedCall call_of(const std::vector<int32_t>& n, int sr_in, int sr_out) {
    RaggedCall c{};
    c.has_in = c.has_out = true;
    c.in_format = RS_SAMPLES_F32;
    c.batch = (int32_t)n.size();
    c.n_in = n.data();
    c.sr_in = sr_in;
    c.sr_out = sr_out;
    c.in_pitch = c.out_pitch = INT32_MAX;
    return c;
}

static bool refused(const RaggedCall& c, const char* reason) {
    RaggedPlan p{};
    p.launches = -7;
    const std::string why = ragged_plan(c, p);
    const bool ok = !why.empty() && why.find(reason) != std::string::npos && p.launches == -7;      // (a refusal leaves the plan alone)
    if (!ok) std::printf("expected a refusal with \"%s\", got \"%s\"\n", reason, why.c_str());
    return ok;
}

int main(int argc, char** argv) {
    if (argc >= 4 && !std::strcmp(argv[1], "sizes")) {
        const int sr_in = std::atoi(argv[2]), sr_out = std::atoi(argv[3]);
        for (int k = 4; k < argc; ++k) {
            const std::vector<int32_t> n = {(int32_t)std::atol(argv[k])};
            RaggedPlan p{};
            const std::string why = ragged_plan(call_of(n, sr_in, sr_out), p);
            if (!why.empty()) {
                std::printf("refused: %s\n", why.c_str());
                return 2;
            }
            const RaggedRow r = ragged_row(p, n[0]);
            std::printf("%d %d\n", r.n_calc, r.n_out);
        }
        return 0;
    }
    const int rates[][2] = {{48000, 16000}, {32000, 16000}, {44100, 16000}, {22050, 16000}, {8000, 16000}, {16000, 16000}, {16000, 48000}, {96000, 16000}};
    // ---- row sizes: floor and ceil of n * sr_out / sr_in in whole numbers, the zero tail 0 or 1 samples, the longest row's sizes
    for (const auto& r : rates) {
        std::vector<int32_t> n;
        for (int32_t v = 1; v <= 1200; ++v) n.push_back(v);
        for (int32_t v : {4799, 4800, 4801, 44100, 48000, 57601, 470400, 470401, 1 << 20}) n.push_back(v);
        RaggedPlan p{};
        EXPECT(ragged_plan(call_of(n, r[0], r[1]), p).empty());
        EXPECT(p.pass == (r[0] == r[1]) && p.launches == ((int)n.size() + RS_RAGGED_ROWS - 1) / RS_RAGGED_ROWS);
        int32_t top_calc = 0, top_out = 0;
        for (int32_t v : n) {
            const RaggedRow row = ragged_row(p, v);
            const int64_t num = (int64_t)v * r[1];
            const int64_t lo = num / r[0], hi = (num + r[0] - 1) / r[0];
            EXPECT(row.n_in == v);
            // (the engine's counts are librosa's: formed in float64, so a whole-number product may land one off the exact quotient -
            // never further, and never with more than one sample of zero tail)
            EXPECT(row.n_calc >= lo - 1 && row.n_calc <= lo && row.n_out >= hi && row.n_out <= hi + 1);
            EXPECT(row.n_out - row.n_calc == 0 || row.n_out - row.n_calc == 1);
            EXPECT(row.n_out == ragged_out_samples(v, r[0], r[1]));
            if (r[0] % r[1] == 0 || r[1] % r[0] == 0) EXPECT(row.n_calc == lo && row.n_out == hi);
            if (r[0] == r[1]) EXPECT(row.n_calc == v && row.n_out == v);
            top_calc = row.n_calc > top_calc ? row.n_calc : top_calc;
            top_out = row.n_out > top_out ? row.n_out : top_out;
        }
        EXPECT(p.n_in_max == 1 << 20 && p.n_calc_max == top_calc && p.n_out_max == top_out);
    }
    // ---- the split over launches: every row in exactly one launch, in order, at most RS_RAGGED_ROWS a launch
    for (int32_t batch : {1, 2, RS_RAGGED_ROWS - 1, RS_RAGGED_ROWS, RS_RAGGED_ROWS + 1, 2 * RS_RAGGED_ROWS, 2 * RS_RAGGED_ROWS + 1, 256, 1000}) {
        int32_t next = 0;
        for (int32_t k = 0; k < ragged_launches(batch); ++k) {
            int32_t row0 = -1, rows = -1;
            ragged_launch_rows(batch, k, row0, rows);
            EXPECT(row0 == next && rows >= 1 && rows <= RS_RAGGED_ROWS);
            next += rows;
        }
        EXPECT(next == batch);
    }
    // ---- the refusals, each with its own reason
    {
        const std::vector<int32_t> n = {100, 4801, 7};
        RaggedCall c = call_of(n, 48000, 16000);
        RaggedPlan p{};
        EXPECT(ragged_plan(c, p).empty() && p.n_in_max == 4801 && p.n_out_max == 1601 && p.n_calc_max == 1600 && p.launches == 1);
        c.in_pitch = 4801;
        c.out_pitch = 1601;
        EXPECT(ragged_plan(c, p).empty());
        RaggedCall d = c;
        d.has_in = false;
        EXPECT(refused(d, "null argument"));
        d = c;
        d.has_out = false;
        EXPECT(refused(d, "null argument"));
        d = c;
        d.n_in = nullptr;
        EXPECT(refused(d, "null argument"));
        d = c;
        d.batch = 0;
        EXPECT(refused(d, "batch 0"));
        d.batch = -3;
        EXPECT(refused(d, "batch -3"));
        d = c;
        d.in_format = 2;
        EXPECT(refused(d, "in_format 2"));
        d.in_format = -1;
        EXPECT(refused(d, "in_format -1"));
        d = c;
        d.sr_in = 0;
        EXPECT(refused(d, "sample rates 0 -> 16000"));
        d = c;
        d.sr_out = -16000;
        EXPECT(refused(d, "sample rates 48000 -> -16000"));
        d = c;
        d.sr_in = 16000 * 513;
        EXPECT(refused(d, "resolution"));
        d = c;
        d.in_pitch = 4800;
        EXPECT(refused(d, "in_pitch 4800 is below the longest row (4801"));
        d = c;
        d.out_pitch = 1600;
        EXPECT(refused(d, "out_pitch 1600 is below the longest row's output (1601"));
        for (int32_t bad : {0, -1, INT32_MIN}) {
            std::vector<int32_t> m = n;
            m[1] = bad;
            RaggedCall e = call_of(m, 48000, 16000);
            EXPECT(refused(e, ("n_in[1] = " + std::to_string(bad)).c_str()));
        }
        // one row alone ignores the pitches, as se_resample's rows of one do
        const std::vector<int32_t> one = {4801};
        RaggedCall e = call_of(one, 48000, 16000);
        e.in_pitch = e.out_pitch = 0;
        EXPECT(ragged_plan(e, p).empty() && p.launches == 1);
        // an output count past 2^31 - 1 (upsampling only), named by row; the largest row that still fits is taken
        const std::vector<int32_t> big = {5, INT32_MAX / 2 + 1};
        EXPECT(refused(call_of(big, 8000, 16000), "n_in[1] = 1073741824: the row's output would pass 2147483647"));
        const std::vector<int32_t> fits = {5, INT32_MAX / 2};
        EXPECT(ragged_plan(call_of(fits, 8000, 16000), p).empty() && p.n_out_max == INT32_MAX - 1);
        const std::vector<int32_t> top = {INT32_MAX};
        EXPECT(ragged_plan(call_of(top, 48000, 16000), p).empty() && p.n_out_max == 715827883);
        EXPECT(ragged_plan(call_of(top, 16000, 16000), p).empty() && p.n_out_max == INT32_MAX);
    }
    // ---- the shared position table: grown in steps, it holds the running sum of one walk, and a row's last position lies in the row
    for (const auto& r : rates) {
        const ResamplePlan plan = resample_plan(r[0], r[1]);
        if (plan.exact || r[0] == r[1]) continue;
        std::vector<double> one, grown;
        double acc_one = 0.0, acc_grown = 0.0;
        ragged_positions_extend(plan, one, acc_one, 5000);
        for (int64_t c : {1, 2, 100, 99, 4096, 5000, 3}) ragged_positions_extend(plan, grown, acc_grown, c);
        EXPECT(one.size() == 5000 && grown.size() == 5000 && std::memcmp(one.data(), grown.data(), 5000 * sizeof(double)) == 0);
        double acc = 0.0;
        for (size_t t = 0; t < one.size(); ++t) {
            EXPECT(one[t] == acc);
            acc += plan.inc;
        }
        RaggedPlan p{};
        p.plan = plan;
        for (int32_t n = 1; n < 2000; ++n) {
            const RaggedRow row = ragged_row(p, n);
            if (row.n_calc > 5000) break;                     // (upsampling: the table built here ends first)
            EXPECT(row.n_calc == 0 || (int64_t)one[(size_t)row.n_calc - 1] < n);
        }
    }
    if (failures) std::printf("%d checks failed\n", failures);
    else std::puts("ok");
    return failures ? 1 : 0;
}

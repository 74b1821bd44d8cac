// Host planning of se_resample_ragged (k_resample.hip): what the call refuses, the sizes of every row and how the rows are dealt
// to launches.  No device code, no HIP types: tests/resample_ragged_check.cpp builds it alone under the host sanitizers.
//
// Row b of a call holds n_in[b] samples and receives, under its own sizes,
//   n_calc = (int)(n_in * ratio)   samples that are computed (resampy: int(shape * sample_ratio)), then
//   n_out  = ceil(n_in * ratio)    - n_calc zeros of librosa's fix_length (0 or 1), then
//   zeros up to n_out of the call's longest row - the row convention of se_enhance_ragged.
// These are the doubles and the truncations of launch_resample / resample_out_samples, so a row alone gets the same counts.
// The row sizes travel to the device as kernel arguments, RS_RAGGED_ROWS rows per launch (three ints a row: 768 bytes of the 4 KB
// an argument block may hold), so a batch of B rows is ceil(B / RS_RAGGED_ROWS) launches and no copy.
#pragma once
#include "resample_pos.h"
#include <climits>
#include <cmath>
#include <cstdint>
#include <string>

namespace se {

constexpr int RS_RAGGED_ROWS = 64;        // rows one launch carries
constexpr int RS_RAGGED_BLOCK = 256;      // outputs one block computes (one per thread)
constexpr int RS_SAMPLES_F32 = 0, RS_SAMPLES_S16 = 1;      // SE_SAMPLES_* of include/se_engine.h

// the arguments of se_resample_ragged as the host sees them (the device pointers only as "given or not")
struct RaggedCall {
    bool has_in, has_out;
    int32_t in_format;
    int64_t in_pitch;
    int32_t batch;
    const int32_t* n_in;      // HOST, batch entries
    int32_t sr_in, sr_out;
    int64_t out_pitch;
};

struct RaggedRow {
    int32_t n_in, n_calc, n_out;
};

struct RaggedPlan {
    bool pass;                // sr_in == sr_out: rows are copied (and converted) through
    ResamplePlan plan;
    int32_t n_in_max;         // the longest row ...
    int32_t n_calc_max;       // ... the outputs it computes: what a shared position table has to cover
    int32_t n_out_max;        // ... and its output: every row is written up to here
    int32_t launches;
};

inline int64_t ragged_out_samples(int32_t n_in, int32_t sr_in, int32_t sr_out) {      // resample_out_samples of k_resample.hip
    if (sr_in == sr_out) return n_in;
    return (int64_t)std::ceil((double)n_in * ((double)sr_out / sr_in));
}

inline RaggedRow ragged_row(const RaggedPlan& p, int32_t n_in) {
    RaggedRow r{};
    r.n_in = n_in;
    r.n_calc = p.pass ? n_in : (int32_t)((double)n_in * p.plan.ratio);
    r.n_out = p.pass ? n_in : (int32_t)std::ceil((double)n_in * p.plan.ratio);
    return r;
}

// launch k of a call of `batch` rows carries rows [row0, row0 + rows)
inline int32_t ragged_launches(int32_t batch) { return (batch + RS_RAGGED_ROWS - 1) / RS_RAGGED_ROWS; }
inline void ragged_launch_rows(int32_t batch, int32_t k, int32_t& row0, int32_t& rows) {
    row0 = k * RS_RAGGED_ROWS;
    rows = batch - row0 < RS_RAGGED_ROWS ? batch - row0 : RS_RAGGED_ROWS;
}

// Every refusal of the call, each with its own reason ("" = accepted, and `p` is filled).  Nothing is touched but `p`.
inline std::string ragged_plan(const RaggedCall& c, RaggedPlan& p) {
    if (!c.has_in || !c.has_out || !c.n_in) return "null argument";
    if (c.batch < 1) return "batch " + std::to_string(c.batch) + ": at least one row has to be given";
    if (c.in_format != RS_SAMPLES_F32 && c.in_format != RS_SAMPLES_S16)
        return "in_format " + std::to_string(c.in_format) + " is neither SE_SAMPLES_F32 (0) nor SE_SAMPLES_S16 (1)";
    if (c.sr_in <= 0 || c.sr_out <= 0)
        return "sample rates " + std::to_string(c.sr_in) + " -> " + std::to_string(c.sr_out) + " Hz: both have to be positive";
    int32_t longest = 0;
    for (int32_t b = 0; b < c.batch; ++b) {
        if (c.n_in[b] < 1) return "n_in[" + std::to_string(b) + "] = " + std::to_string(c.n_in[b]) + ": a row holds at least one sample";
        if (c.n_in[b] > longest) longest = c.n_in[b];
    }
    RaggedPlan q{};
    q.pass = c.sr_in == c.sr_out;
    q.plan = resample_plan(c.sr_in, c.sr_out);
    if (!q.pass && q.plan.index_step < 1)
        return "sample rates " + std::to_string(c.sr_in) + " -> " + std::to_string(c.sr_out) + " Hz: sr_out / sr_in below the filter table's resolution";
    for (int32_t b = 0; b < c.batch; ++b)      // (monotone in n_in, but the reason names the row)
        if (!q.pass && std::ceil((double)c.n_in[b] * q.plan.ratio) > (double)INT_MAX)
            return "n_in[" + std::to_string(b) + "] = " + std::to_string(c.n_in[b]) + ": the row's output would pass " + std::to_string(INT_MAX) +
                   " samples";
    const RaggedRow top = ragged_row(q, longest);
    q.n_in_max = longest;
    q.n_calc_max = top.n_calc;
    q.n_out_max = top.n_out;
    q.launches = ragged_launches(c.batch);
    if (c.batch > 1 && c.in_pitch < longest)
        return "in_pitch " + std::to_string(c.in_pitch) + " is below the longest row (" + std::to_string(longest) + " samples)";
    if (c.batch > 1 && c.out_pitch < top.n_out)
        return "out_pitch " + std::to_string(c.out_pitch) + " is below the longest row's output (" + std::to_string(top.n_out) + " samples)";
    p = q;
    return "";
}

// The shared position table of a ratio that is no integer decimation: resampy's running float64 sum of inc, entry t the read
// position of output t of ANY row (it depends on t and the ratio alone).  Extends `tr` to `count` entries, carrying the sum on.
template <typename Vec>
inline void ragged_positions_extend(const ResamplePlan& plan, Vec& tr, double& acc, int64_t count) {
    while ((int64_t)tr.size() < count) {
        tr.push_back(acc);
        acc += plan.inc;
    }
}

}  // namespace se

// Host arithmetic of the resampler (k_resample.hip): the read position of every output sample and, for the stateful
// resampler, which outputs a prefix of the input makes final.  No device code, no HIP types: tests/resample_pos_check.cpp
// builds it alone under the host sanitizers.
//
// Output t reads the input around position tr(t): the left wing takes x[n], x[n - 1], ... and the right wing x[n + 1], ...
// (n = (int)tr), each at most RS_NWIN / index_step taps long and clamped by the signal's two ends.  tr(t) is
//   t * inc exactly                      when sr_in % sr_out == 0 (integer decimation), or
//   resampy's running float64 sum of inc otherwise - a state (t, acc) that a stream carries from push to push, so that the
//                                        positions are the doubles one offline call computes.
// A wing spans at most RS_NWIN / index_step taps (192 at 48 -> 16 kHz: the filter looks 4 ms ahead).  `reach` rounds that up,
// RS_NWIN / index_step + 1 = ceil(RS_NWIN / index_step) whenever the step does not divide the table (193 at 48 -> 16 kHz), and a
// stream calls output t final once sample n + reach itself has arrived, n + reach < n_in: one sample later than the furthest
// tap any fraction can have, which keeps the rule free of the fraction.
#pragma once
#include <cmath>
#include <cstdint>

namespace se {

constexpr int RS_ZEROS = 64, RS_BITS = 512, RS_NWIN = RS_ZEROS * RS_BITS + 1;

struct ResamplePlan {
    double ratio, inc, scale;
    int index_step, reach;
    bool exact;              // integer decimation: tr(t) = t * inc, no running sum
};

inline ResamplePlan resample_plan(int sr_in, int sr_out) {
    ResamplePlan p{};
    p.ratio = (double)sr_out / sr_in;
    p.inc = 1.0 / p.ratio;
    p.scale = p.ratio < 1.0 ? p.ratio : 1.0;
    p.index_step = (int)(p.scale * RS_BITS);
    p.reach = p.index_step > 0 ? RS_NWIN / p.index_step + 1 : 0;
    p.exact = sr_in % sr_out == 0;
    return p;
}

// the next output sample of a stream and, on the running-sum path, its read position
struct ResamplePos {
    int64_t t = 0;
    double acc = 0.0;
};
inline double resample_pos_of(const ResamplePlan& p, const ResamplePos& s) { return p.exact ? (double)s.t * p.inc : s.acc; }
inline void resample_pos_step(const ResamplePlan& p, ResamplePos& s) {
    ++s.t;
    s.acc += p.inc;
}

// Moves `s` past every output below t_end that the first n_in input samples make final (n + reach < n_in); their read positions go to
// tr[0 .. cap) when tr != nullptr.  Returns how many outputs were passed (it stops at cap when tr is given).
inline int64_t resample_advance(const ResamplePlan& p, ResamplePos& s, int64_t n_in, int64_t t_end, double* tr, int64_t cap) {
    int64_t k = 0;
    while (s.t < t_end && (!tr || k < cap)) {
        const double pos = resample_pos_of(p, s);
        if ((int64_t)pos + p.reach >= n_in) break;
        if (tr) tr[k] = pos;
        ++k;
        resample_pos_step(p, s);
    }
    return k;
}

// floor(n_in * ratio): the samples resampy computes for a signal of n_in samples (the offline launcher's n_calc)
inline int64_t resample_calc_samples(const ResamplePlan& p, int64_t n_in) { return (int64_t)((double)n_in * p.ratio); }

// How many outputs are final once n_in input samples of a signal that has not ended have arrived.  Integer decimation: a
// bisection over t (the position is monotone in t); other ratios walk the running sum from 0, O(outputs).
inline int64_t resample_ready(const ResamplePlan& p, int64_t n_in) {
    if (n_in <= p.reach) return 0;
    if (!p.exact) {
        ResamplePos s;
        return resample_advance(p, s, n_in, INT64_MAX, nullptr, 0);
    }
    int64_t lo = 0, hi = n_in + 1;          // position(lo) is final, position(hi) = hi * inc >= hi is not
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((int64_t)((double)mid * p.inc) + p.reach < n_in) lo = mid;
        else hi = mid;
    }
    return lo + 1;
}

}  // namespace se

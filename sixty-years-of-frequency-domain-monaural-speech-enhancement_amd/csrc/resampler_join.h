// Joining parked source-rate signals that began at different times (se_resampler_state_join, include/se_engine.h): when a parked
// StreamResampler signal is past its left edge, and the plan of a join - the shift of every part onto the counters of parts[0] and
// the one history all rows keep.  Host code alone, no device runtime - k_resample includes it, and so does a stand-alone check program
// (tests/resampler_join_check.cpp).
//
// Integer decimation only (sr_in % sr_out == 0, D = sr_in / sr_out; ResamplePlan::exact).  Output t then reads around input position
// n = t * D exactly: inc = 1 / (sr_out / sr_in) is the double D (checked in the plan), pos_frac is 0, so the table offsets of both
// wings are constants, and resample_pos_of() ignores the running sum `acc`.  Every index resample_taps forms is n plus a constant
// (x(n - i), x(n + k + 1)), WindowAt reads hist[p - w0], and the right wing is clamped by n_total - n - 1: all of them are differences
// of positions, unchanged when n_total, w0 and n move by the same s.  What does depend on position 0, in everything a push or the
// flush evaluates (resample_taps, StreamResampler::push / flush):
//   (1) the left wing's clamp  i_max = min(n + 1, (RS_NWIN - offset) / index_step).  offset is 0 here, so the second term is
//       RS_NWIN / index_step = reach - 1, and the clamp is idle once n + 1 >= reach - 1: for the next output t,
//       t * D >= reach - 2   (191 at 48 -> 16 kHz: t >= 64; 127 at 32 -> 16 kHz: t >= 64).  The same bound idles the host's
//       max(0, pos - (reach - 2)) >= w0 test of push and flush.  Outputs below t are never computed again.
//   (2) the history origin  w0_next = max(w0, n_after - 2 * reach), w0 = 0 at the signal's start.  A signal that is past (1) but has
//       received fewer than 2 * reach samples still has w0 = 0; rebased it holds MORE history than a signal of its new length would,
//       never less, and a push keeps the origin it has until n_after - 2 * reach passes it.  Parts may so have been saved with histories
//       of different lengths.  The join keeps, for every row, the samples from the highest rebased w0 of any part: every part's own w0
//       is at or below what its next output reads (push checks pos - (reach - 2) >= w0), the parts are in phase - after the rebase they
//       share t and n_total - so the highest w0 serves them all.
// resampler_left_edge() is the smallest t that satisfies (1); tests/resampler_join_check.cpp walks a signal sample by sample through
// the index expressions above and finds the same number.
//
// Past that edge a parked signal can be REBASED by any s that is a multiple of D: n_total += s, w0 += s, t += s / D; the stored acc
// becomes (double)t' * inc, which is exact.  Two parked groups whose counters differ by such an s then join into one that advances in
// lockstep.
//
// The flush.  It computes resample_calc_samples = (int64_t)((double)n_total * ratio) outputs and zero-fills up to
// ceil((double)n_total * ratio); a rebased row flushes at a shifted n_total and gets what it would have got alone only if those two
// double expressions equal the integers n_total / D and ceil(n_total / D) at both positions.  ratio = (double)sr_out / sr_in is the
// correctly rounded 1 / D whatever the two rates are, so the identity is a property of D alone; tests/resampler_join_check.cpp walks
// it over n = 0 ... 2^31 - 1 for every D in RSJOIN_DECIMATIONS, and the join accepts those D and no other.  (D = 3: 3k * fl(1/3) =
// k - k 2^-54 exactly, at most half an ulp below k, a tie only where k is a power of two, which rounds to even: k.)
#pragma once
#include "resampler_manifest.h"
#include <algorithm>
#include <vector>

namespace se {

// the integer decimations whose flush arithmetic has been walked (1: pass-through, which computes nothing)
constexpr int RSJOIN_DECIMATIONS[] = {1, 2, 3};

inline bool rsjoin_walked(int64_t D) {
    for (int d : RSJOIN_DECIMATIONS)
        if (d == D) return true;
    return false;
}

// the smallest next output t from which a parked signal of this (integer-decimation) plan can be rebased: t * D >= reach - 2
inline int64_t resampler_left_edge(const ResamplePlan& p) {
    const int64_t D = (int64_t)p.inc;
    return D >= 1 && p.reach > 2 ? ((int64_t)p.reach - 2 + D - 1) / D : 0;
}

// What a join does to its parts, from their records alone.  shift[p] = parts[0].n_total - parts[p].n_total is added to n_total and w0
// of part p (t moves by shift / D).  The result keeps the samples from w0 on: columns [col[p], col[p] + live) of part p's packed rows.
struct ResamplerJoinPlan {
    std::vector<int64_t> shift;
    std::vector<int64_t> col;
    int64_t w0 = 0, live = 0;
};

// "" and the plan, or why the parts cannot be joined (the plan is then left alone)
inline std::string rsnap_join_plan(const std::vector<const ResamplerManifest*>& parts, ResamplerJoinPlan& plan) {
    if (parts.empty()) return "n_parts 0: at least one part has to be given";
    const ResamplerManifest& a = *parts[0];
    auto at = [](size_t p) { return "parts[" + std::to_string(p) + "]"; };
    auto vs = [](int64_t x, int64_t y) { return std::to_string(x) + " vs " + std::to_string(y); };
    const std::string rates = std::to_string(a.sr_in) + " -> " + std::to_string(a.sr_out) + " Hz";
    for (size_t p = 1; p < parts.size(); ++p) {
        if (a.sr_in != parts[p]->sr_in) return "parts[0] and " + at(p) + " differ: sr_in " + vs(a.sr_in, parts[p]->sr_in);
        if (a.sr_out != parts[p]->sr_out) return "parts[0] and " + at(p) + " differ: sr_out " + vs(a.sr_out, parts[p]->sr_out);
    }
    if (a.sr_in <= 0 || a.sr_out <= 0) return "parts[0]: rates out of range";
    if (a.sr_in % a.sr_out != 0)
        return rates + " cannot be rebased: the read position is a running float64 sum from the signal's start (sr_in % sr_out != 0)";
    const int64_t D = a.sr_in / a.sr_out;
    const bool pass = D == 1;
    const ResamplePlan rp = resample_plan(a.sr_in, a.sr_out);
    if (!rsjoin_walked(D) || rp.inc != (double)D || (!pass && rp.index_step <= 0))
        return rates + " cannot be rebased: integer decimation by " + std::to_string(D) +
               " is not among those whose flush arithmetic has been walked over every length (1, 2, 3)";
    ResamplerJoinPlan out;
    bool moved = false;
    for (size_t p = 0; p < parts.size(); ++p) {
        const ResamplerManifest& b = *parts[p];
        const int64_t s = a.n_total - b.n_total;
        if (s % D != 0)
            return "parts[0] and " + at(p) + " are out of phase: n_in " + vs(a.n_total, b.n_total) + ", the shift " + std::to_string(s) +
                   " is not a multiple of sr_in / sr_out = " + std::to_string(D);
        const int64_t fa = a.n_total - a.t * D, fb = b.n_total - b.t * D;
        if (fa != fb) return "parts[0] and " + at(p) + " are out of phase: n_in - n_out * " + std::to_string(D) + " " + vs(fa, fb);
        moved = moved || s != 0;
        out.shift.push_back(s);
    }
    if (moved && !pass) {
        const int64_t need = resampler_left_edge(rp);
        for (size_t p = 0; p < parts.size(); ++p)
            if (parts[p]->t < need)
                return at(p) + " is short of the left edge: n_out " + std::to_string(parts[p]->t) + ", a signal can be rebased from n_out " +
                       std::to_string(need) + " on (" + rates + ")";
    }
    int64_t w0 = 0;
    for (size_t p = 0; p < parts.size(); ++p) w0 = std::max(w0, parts[p]->w0 + out.shift[p]);
    for (size_t p = 0; p < parts.size(); ++p) {
        const int64_t col = w0 - (parts[p]->w0 + out.shift[p]);
        if (w0 > a.n_total || col > rsnap_keep(*parts[p]))
            return at(p) + ": w0 " + vs(w0 - out.shift[p], parts[p]->w0) + ": the joined history starts behind the samples the part holds";
        out.col.push_back(col);
    }
    out.w0 = w0;
    out.live = a.n_total - w0;
    plan = std::move(out);
    return "";
}

// the record of the result: parts[0]'s counters on the joined history, `rows` rows
inline ResamplerManifest rsnap_joined(const ResamplerManifest& first, const ResamplerJoinPlan& plan, int32_t rows) {
    ResamplerManifest m = first;
    m.batch = rows;
    m.w0 = plan.w0;
    if (m.sr_in != m.sr_out) m.acc_bits = rsnap_bits_of((double)m.t * resample_plan(m.sr_in, m.sr_out).inc);
    return m;
}

}  // namespace se

// Joining parked stream groups that began at different times (se_stream_state_join, include/se_engine.h): when a parked stream is
// past its left edge, and the plan of a join - the shift of every part onto the counters of parts[0] and the one input window all
// rows keep.  Host code alone, no HIP - the engine includes it, and so does a stand-alone check program (tests/stream_join_check.cpp).
//
// A decode step of a stream that is past its left edge does not depend on the stream's absolute position, as long as the position
// moves by whole hops: every index the front end forms is a frame index times the hop plus a constant, the grids of the STFT and
// the iSTFT start at the launch's own first frame / first output sample, and the networks that are accepted here take no frame
// index at all (or take it per row from the row's own frame origin: "Per-row frame origins" below).  What does depend on position 0,
// in everything se_stream_push / se_stream_flush launch (the engine's stream_process):
//   (a) the STFT of a frame t reads samples t hop - n_fft/2 ...; where that is negative it mirrors (`idx < 0` in the forward kernel), and its
//       wave-uniform fast path asks `t hop >= n_fft/2` of the first frame of a pair.  Frames below t_done are never transformed
//       again, so neither test can hold once   t_done hop >= n_fft/2.
//   (b) stream_keep_from() clamps t_done hop - n_fft/2 and n_total - n_fft/2 - 1 to 0.  The first is (a); the second is at least
//       (t_done - 1) hop, because frame t_done - 1 was released only when sample (t_done - 1) hop + n_fft/2 had arrived.
//   (c) the iSTFT overlap-adds into output sample o = pos - n_fft/2 every frame t with t hop <= pos < t hop + n_fft and divides by
//       the window energy of exactly those frames.  The engine bounds the frames from below by max(0, t0 - HC); near the start
//       that bound, not `pos - t hop < n_fft`, ends the loop, and the envelope is short of frames that would lie before frame 0.
//       The lowest frame that covers pos is floor((pos - n_fft) / hop) + 1, which is >= 0 from pos >= n_fft - hop on; every
//       sample still to be written has o >= o_done = max(0, (t_done - lag) hop - n_fft/2), so the bound is idle from the start where
//       hop >= n_fft/2 (every pos is at least n_fft/2), and else once   (t_done - lag + 1) hop >= n_fft.   (lag: Model::stream_lag(),
//       the frames a look-ahead model finalises late.)  The frames between t0 - HC and 0 that a rebased stream then LOADS where the
//       original loaded zeros are transformed and never added.
//   (d) the model's first-chunk handling (StreamState::first: an LSTM's first step starts from a zero state) ends with the first
//       chunk:   t_done >= 1.
// stream_left_edge_frames() is the smallest t_done that satisfies all four; tests/stream_join_check.cpp walks a stream sample by
// sample through the index expressions above and finds the same number.  (The window `win` may be shorter than n_fft; frames are
// n_fft long for every index above, so the bound is taken for n_fft.)
// The position independence derived here is exercised at the far end of the counter range too: tests/test_gpu_late_stream.py moves parked
// streams of every streamable network by up to 2^31 - 1 - max(max_samples, n_fft + 32 hop) samples and holds the continuation to bit identity.
#pragma once
#include "stream_rows.h"
#include <algorithm>

namespace se {

inline int stream_left_edge_frames(int n_fft, int hop, int lag) {
    const int stft = (n_fft / 2 + hop - 1) / hop;                  // (a), (b)
    const int istft = hop >= n_fft / 2 ? 0 : (n_fft + hop - 1) / hop - 1 + lag;      // (c)
    return std::max(1, std::max(stft, istft));                     // (d)
}

inline int64_t snap_gcd(int64_t a, int64_t b) { return b == 0 ? a : snap_gcd(b, a % b); }

// What a join does to its parts, from their manifests alone.  shift[p] = parts[0].n_total - parts[p].n_total is added to every
// position of part p (n_total, o_done, keep; t_done moves by shift / hop).  The result keeps, for every row, the input samples from
// `keep` on - the highest rebased keep of any part: each part's keep is at or below what its next launch reads and the parts are in
// phase, so the highest is enough for all - i.e. columns [col[p], col[p] + live) of part p's window rows.
struct JoinPlan {
    std::vector<int64_t> shift;
    std::vector<int32_t> col;
    std::vector<int32_t> rot;      // tracking scale: ring positions part p's per-frame rings move up by, in [0, ring)
    std::vector<int32_t> frames;   // shift[p] / hop: what the join adds to the frame origins of part p's rows (snap_join_origin)
    int32_t keep = 0, live = 0;
};

// Per-row frame origins (SE_CFG_STREAM_ROW_ORIGINS, the SNAP_ORIGIN segment): the models that count frames in a join.
//
// The state of the cLN networks (CTSNet_new, TaylorSENet_new, G2Net_new) and of FullSubNet with the cumulative norm counts frames from
// the start of the stream: the cLN divides its running float64 sums by R (t + 1) and masks FIR / history columns by t >= 0
// (cln_window_reg_kernel, cln_window_kernel, cln_scan_kernel, cln_apply_kernel), the TCM chain kernel divides by 64 (t + 1) and keeps
// its FIR / dilated-conv histories in rings indexed by t & (R - 1) (tcm_chain_kernel), FullSubNet's two cumulative norms divide by
// the frame index (fsn_cum_fb_kernel, fsn_cum_sb_kernel) and its mask stage skips the steps with t < look-ahead
// (fsn_stream_apply_kernel).  None of that state is shared between rows.  With the bit every row b carries an origin o_b (frames,
// int32, zero at se_stream_begin*), and each of these kernels forms t = (group frame) - o_b before it does anything else with it.
// A join moves part p's group frame by f_p = shift[p] / hop and adds f_p to the origins of its rows: t is what it was, so the row
// keeps dividing by its own frame count and reads and writes its rings where it always did.  No ring is rotated, and the carried
// sums are the sums of exactly the frames the divisor counts.  Origins accumulate over joins (o_b + f_p + f'_q ...) and are negative
// for a row of a part older than parts[0].
//
// Every other use of the frame index t0 on these models' paths (Model::stream_chunk and the engine's stream_process), and why none
// of them is model state that a rebase could break:
//   * CTSNet / G2Net / TaylorSENet stream_chunk: t0 goes into StreamScope (-> StreamCtx::t0) and nowhere else.  StreamCtx::t0 is read
//     by launch_cln (tg0 = t0 - H) and launch_tcm_chain (a.t0) alone; both hand StreamCtx::origin to their kernels.  The host
//     branches of those launchers and of the models (the register form for n <= 2, the 32768 switch of the window form, CTSNet's
//     decoder fork for n <= 2) look at the chunk length n and the tensor sizes, never at t0.  The history exchange
//     (stream_exchange, gc_stream_prepare) moves the last columns of a window through per-row slots without an index.
//   * FullSubNet stream_chunk: t0 goes to the three launchers named above, each with the origin pointer.  `ss.first` (an LSTM's first
//     step starts from a zero state) is the one host-side branch on model state; it is group-wide and ends with the first chunk -
//     (d) of the derivation above - and snap_join_plan refuses a moved part that still has it.  `last` (two more steps on zero
//     frames) is the end of the stream, a front-end position common to the group.  A row whose own index is below the look-ahead
//     is not kept out of a join by the left-edge threshold (1 frame for 512 / 256, below the look-ahead of 2) but by the phase check:
//     o_done = (t_done - 2) hop - n_fft / 2 is clamped to 0 below t_done 3, so n_total - o_done of such a part differs from that of any
//     part that is further on.  Parts that are ALL that young join with shift 0 or among themselves, and the kernel skips the steps
//     below the look-ahead per row from the row's own index, so nothing rests on that exclusion.
//   * stream_process: t0 is S.t_done - the STFT's first frame, the iSTFT's frame bounds, the per-frame scale rings, the window
//     origin: all front end, all indexed by the GROUP frame, which is why the tracking-scale rings are still rotated by the join
//     and the running scale is still refused.  Nothing there is per-row model state.
// So the front-end threshold stream_left_edge_frames() suffices for these models too: past it the front end does not depend on the
// absolute position (a) - (d); the model state is per row; zero-initialised slots and ring entries are the causal padding a row's
// kernels find at its own negative indices, rebased or not; and every model-side index is taken from the row's own origin.
//
// the origin of a row of part p after the join (int32 wrap-around would need 2^31 frames: a stream ends long before)
inline int32_t snap_join_origin(int32_t origin, int32_t frames) { return origin + frames; }

// The tracking scale (se_stream_begin_tracking) in a join.  Its state per row is (E, W) and two rings, c_t and 1 / c_t of frame t at
// position t & (ring - 1).  (E, W) are sums over the row's own past, weighted by the distance in blocks from the newest block: no
// absolute position enters, and the shift is a whole number of hops, so the blocks of the rebased row are the blocks it had.  The
// kernel finds the blocks a push completes from n_total alone ([(n_total - n_new) / hop, n_total / hop)), which the manifest rebases.
// The rings ARE indexed by the absolute frame: frame t of the part is frame t + s / hop of the result (s the shift in samples), so
// entry i of a rebased ring row is entry (i - s / hop) mod ring of the part's - a rotation, applied to whole rows by the join
// kernel.  Only some entries are live, i.e. read again: the forward transform reads c_t of frames >= t_done, all of them written
// by a later push before they are read; the inverse reads 1 / c_t of the frames that still cover an output sample to be written,
// o >= o_done: t hop + n_fft > o_done + n_fft / 2, i.e. t >= floor((o_done - n_fft / 2) / hop) + 1 (clamped to 0), up to t_done - 1.
// That is fewer than n_fft / hop + look-ahead + 1 entries of a ring of >= 64, so rotating whole rows moves them all and nothing else
// that matters.
// rotation of a ring of `ring` entries (a power of two) by a shift of s samples, s a multiple of hop of either sign
inline int32_t snap_ring_rot(int64_t s, int32_t hop, int32_t ring) {
    const int64_t f = s / hop;
    return (int32_t)(((f % ring) + ring) % ring);
}
// the source position of entry i of a rotated ring row
inline int32_t snap_ring_src(int32_t i, int32_t rot, int32_t ring) { return (i - rot) & (ring - 1); }
// frames [lo, t_done) of a stream are the ones whose 1 / c_t the inverse transform still reads
inline int64_t snap_ring_live_from(int64_t o_done, int32_t n_fft, int32_t hop) {
    const int64_t x = o_done - n_fft / 2;      // floor division of a value that may be negative
    const int64_t q = x >= 0 ? x / hop : -((-x + hop - 1) / hop);
    return std::max<int64_t>(0, q + 1);
}

// "" and the plan, or why the parts cannot be joined.  lag: the model's stream_lag(); counts_frames: empty, or what in the model's
// state counts frames (such a model is refused: its state cannot be rebased); first_counts: the model keeps a StreamState, whose
// `first` flag SnapManifest::first records (Model::stream_state() != null: the engine says so).  A model that keeps call-order slots
// instead has no such flag and se_stream_save records a constant 1 for it, which says nothing - its first chunk is behind it once
// t_done >= 1, and `need` is at least 1.
inline std::string snap_join_plan(const std::vector<const SnapManifest*>& parts, int lag, const std::string& counts_frames, JoinPlan& plan,
                                  bool first_counts = true) {
    if (parts.empty()) return "n_parts 0: at least one part has to be given";
    const SnapManifest& a = *parts[0];
    auto at = [](size_t p) { return "parts[" + std::to_string(p) + "]"; };
    auto vs = [](int64_t x, int64_t y) { return std::to_string(x) + " vs " + std::to_string(y); };
    if (!counts_frames.empty()) return "this model's stream state cannot be rebased: " + counts_frames;
    if (a.hop < 1 || a.n_fft < 2) return "parts[0]: front end n_fft / hop " + std::to_string(a.n_fft) + " / " + std::to_string(a.hop) + " out of range";
    const int64_t unit = (int64_t)a.hop / snap_gcd(a.hop, 4) * 4;      // lcm(hop, 4): keep is a multiple of 4 and stays one
    JoinPlan out;
    bool moved = false;
    for (size_t p = 0; p < parts.size(); ++p) {
        const SnapManifest& b = *parts[p];
        if (b.running == 1)
            return at(p) + " is a running-scale stream: its ring of 1 / c per frame is indexed by the absolute frame (running 1)";
        if (b.running == 2 && (b.ring < 1 || (b.ring & (b.ring - 1)) != 0))
            return at(p) + " is a tracking-scale stream whose ring length " + std::to_string(b.ring) + " is no power of two";
        if (p > 0) {
            const std::string why = snap_concat_differs(a, b, false);
            if (!why.empty()) return "parts[0] and " + at(p) + " differ: " + why;
        }
        const int64_t s = (int64_t)a.n_total - b.n_total;
        if (s % unit != 0)
            return "parts[0] and " + at(p) + " are out of phase: n_total " + vs(a.n_total, b.n_total) + ", the shift " + std::to_string(s) +
                   " is not a multiple of lcm(hop, 4) = " + std::to_string(unit);
        const int64_t fa = (int64_t)a.n_total - (int64_t)a.t_done * a.hop, fb = (int64_t)b.n_total - (int64_t)b.t_done * b.hop;
        if (fa != fb) return "parts[0] and " + at(p) + " are out of phase: n_total - t_done * hop " + vs(fa, fb);
        const int64_t oa = (int64_t)a.n_total - a.o_done, ob = (int64_t)b.n_total - b.o_done;
        if (oa != ob) return "parts[0] and " + at(p) + " are out of phase: n_total - o_done " + vs(oa, ob);
        moved = moved || s != 0;
        out.shift.push_back(s);
        out.rot.push_back(b.running == 2 ? snap_ring_rot(s, a.hop, b.ring) : 0);
        out.frames.push_back((int32_t)(s / a.hop));      // (s is a multiple of the hop)
    }
    if (moved) {
        const int need = stream_left_edge_frames(a.n_fft, a.hop, lag);
        for (size_t p = 0; p < parts.size(); ++p)
            if (parts[p]->t_done < need || (first_counts && parts[p]->first))
                return at(p) + " is short of the left edge: t_done " + std::to_string(parts[p]->t_done) + ", a stream can be rebased from t_done " +
                       std::to_string(need) + " on (n_fft " + std::to_string(a.n_fft) + ", hop " + std::to_string(a.hop) + ", look-ahead " +
                       std::to_string(lag) + ")";
    }
    int64_t keep = 0;
    for (size_t p = 0; p < parts.size(); ++p) keep = std::max(keep, (int64_t)parts[p]->keep + out.shift[p]);
    for (size_t p = 0; p < parts.size(); ++p) {
        const int64_t col = keep - (parts[p]->keep + out.shift[p]);
        if (keep > a.n_total || col > (int64_t)parts[p]->n_total - parts[p]->keep)
            return at(p) + ": keep " + vs(keep - out.shift[p], parts[p]->keep) + ": the joined window starts behind the samples the part holds";
        out.col.push_back((int32_t)col);
    }
    out.keep = (int32_t)keep;
    out.live = (int32_t)(a.n_total - keep);
    plan = std::move(out);
    return "";
}

}  // namespace se

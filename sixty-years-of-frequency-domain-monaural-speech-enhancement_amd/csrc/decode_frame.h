// The scaffolding every causal network's decode shares: the frame counts of an offline call, the fork / join of a side chain
// onto an auxiliary stream, and the tail of a frame-online chunk of the cLN networks.
#pragma once
#include "model.h"

namespace se {

// Frame counts of one offline enhance() call over B clips of T frames each (model.h has the measurements behind the rule).
//   * causal_all - nothing in the network looks ahead or reduces over the whole clip (the BatchNorm / LSTM networks, the cLN
//     weights of the TCM networks): the rows are zero-extended to Tw = whole 128 B lines (causal_work_frames).  The STFT / iSTFT
//     walk the clip's own Ts = T frames, the caller zeroes its input tensors once (zero_rows) and a recurrent section walks T
//     frames (own_frames).  In a ragged call the rows' own lengths travel in the ragged context and the STFT writes the zeros
//     behind each row's last frame itself: Ts = Tw and nothing is zeroed here.
//   * otherwise (InstanceNorm weights: statistics over the whole clip) the batch runs as ragged rows of ONE length, published
//     by the PadFrames this object owns for the length of the call: Tw = Ts = its frame count.
struct WorkFrames {
    PadFrames pad;
    const bool rag;       // the rows carry their own lengths (a ragged call, or PadFrames' rows of one length)
    const int Tw, Ts;     // row pitch the network runs with; frames the STFT / iSTFT walk
    WorkFrames(EngineCtx& ctx, int B, int L, int Lpad, int T, hipStream_t st, bool causal_all)
        : pad(ctx, B, L, Lpad, T, L, st, causal_all ? 1 : in_pad_multiple()), rag(ragged_ctx() != nullptr),
          Tw(causal_all ? causal_work_frames(T, true) : pad.T), Ts((causal_all && !rag) ? T : Tw), B(B), T(T),
          zext(causal_all && !rag && Tw != T) {}
    ~WorkFrames() {
        if (tl) *tl = 0;
    }
    // x [B][rows][Tw], an input of the network that the STFT fills up to frame T only
    void zero_rows(float* x, long rows, hipStream_t st) const {
        if (zext) SE_HIP(hipMemsetAsync(x, 0, (size_t)B * rows * Tw * sizeof(float), st));
    }
    // `Tl` of a network whose recurrent section walks the clip's own frames: T for the length of the call, then 0 again
    void own_frames(int& Tl) {
        tl = &Tl;
        Tl = T;
    }

  private:
    const int B, T;
    const bool zext;
    int* tl = nullptr;
};

// One fork point on the caller's stream `st`: chains that only depend on what `st` holds now run on auxiliary streams next to
// what `st` is given afterwards.
//     Fork fk(ctx, st, on);
//     chain(fk.to(0), fk.prof(0));  fk.done(0);      // enqueued first, on auxiliary stream 0
//     other(st, &ctx.prof);         fk.join(0);      // st goes on behind both
// The first to() records ev_fork on st, every to(i) makes auxiliary stream i wait for it, done(i) records ev_join[i] behind the
// chain and join(i) makes st wait for that.  With `on` false everything stays on st in the same enqueue order - the order the
// frame-online state slots are taken in - and no event call is made.
struct Fork {
    EngineCtx& ctx;
    const hipStream_t st;
    const bool on;
    bool marked = false;
    Fork(EngineCtx& c, hipStream_t s, bool on_) : ctx(c), st(s), on(on_) {}
    hipStream_t to(int i) {
        if (!on) return st;
        hipStream_t s = ctx.aux_stream(i);
        if (!marked) SE_HIP(hipEventRecord(ctx.ev_fork, st));
        marked = true;
        SE_HIP(hipStreamWaitEvent(s, ctx.ev_fork, 0));
        return s;
    }
    Profiler* prof(int i) const { return on ? &ctx.aux_prof[i] : &ctx.prof; }
    void done(int i) const {
        if (on) SE_HIP(hipEventRecord(ctx.ev_join[i], ctx.aux_stream(i)));
    }
    void join(int i) const {
        if (on) SE_HIP(hipStreamWaitEvent(st, ctx.ev_join[i], 0));
    }
};

// Tail of a frame-online chunk of the cLN networks (CTSNet_new, G2Net_new, TaylorSENet_new): y [B][2][F][T] -> the
// decompressed estimate `est` (may be y), with the previous chunk's last frame in front of the new ones - the iSTFT overlaps
// one frame back.  The chunk tensors of these networks are windows of STREAM_HC = 4 history columns + n new frames that only
// serve the U-Net's one-frame look-back and this overlap: the TCM blocks keep their dilated convs' and FIRs' reach in ring
// state of their own (k_tcm_stream.hip), the shared launch helpers the per-layer history and the cLN sums (kernels.h: StreamCtx).
inline void stream_estimate(const float* y, float* est, int B, int F, int T, float p_out, hipStream_t st) {
    launch_polar_pow(y, est, B, F, T, p_out, st);
    stream_exchange(est, 2L * F * T, (long)F * T, T, B, 2, F, 2, st);
}

}  // namespace se

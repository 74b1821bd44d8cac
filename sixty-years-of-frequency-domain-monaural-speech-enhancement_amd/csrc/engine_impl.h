// What the two units of the entry layer share (engine.hip: the C ABI of the engine; stream_state.hip: parked streams): the handle, the
// call guard, and the few helpers of a frame-online stream both need.
#pragma once
#include "../../include/se_engine.h"
#include "hip_owned.h"
#include "model.h"
#include "rnn.h"
#include "batch_parts.h"
#include <algorithm>
#include <cmath>

using namespace se;

// Every device buffer, pinned buffer, event and stream below is an owner (hip_owned.h): `delete e` releases them, and members are
// destroyed in reverse order of declaration - each model is declared behind the context it refers to
struct se_engine {
    se_config cfg{};
    EngineCtx ctx;
    StateDict sd;
    std::unique_ptr<Model> model;
    bool finalized = false;
    int plan_frames = 0;     // frames the workspace was sized for (>= frames of max_samples; frame-online windows may be longer)
    std::string err;
    // hipGraph replay of se_enhance_batch (SE_CFG_GRAPHS): one instantiated graph per (batch, samples) shape, captured
    // on the second call of a shape (the first, eager call sets kernel attributes and grows the lazy scratch buffers);
    // caller buffers are decoupled from the graph by engine-owned staging rows
    struct GraphEntry {
        int batch, samples;
        hipGraphExec_t exec;     // nullptr: this shape could not be captured, stay eager
    };
    std::vector<GraphEntry> graphs;
    std::vector<std::pair<int, int>> warmed;
    DevBuf<float> stage_in, stage_out;
    DevBuf<float> hook_buf;        // se_backend: the decompressed spectrum between the mask stage and the iSTFT (grows, never shrinks)
    size_t hook_cap = 0;
    // se_enhance_ragged: per-row sizes (len | lpad | tlen | olen, max_batch ints each) go host -> device through a small
    // ring of pinned slots, so back-to-back calls never wait for each other's copy
    static constexpr int RAG_SLOTS = 8;
    PinnedBuf<int> rag_host;       // pinned [RAG_SLOTS][4 * max_batch]
    DevBuf<int> rag_dev;           // device [RAG_SLOTS][4 * max_batch]
    Event rag_ev[RAG_SLOTS];
    int rag_next = 0;
    DevBuf<int> rag_win;           // device [4 * max_batch]: the rows' sizes as the current window launch of se_enhance_long_ragged sees them
    OwnedStream cap_stream;
    // the keys under which work forked onto the process-wide auxiliary streams takes its scratch while a shape is warmed or captured
    // (common.h: ScratchOwner)
    ScratchOwner scratch_own;
    Event ev_fork, ev_join;
    // Two half-batches side by side (round 6: Uformer, DPCRN, CTSNet, TaylorSENet): a second instance of the model with its own context and
    // workspace decodes rows [B / 2, B) of a se_enhance_batch call on a process-wide auxiliary stream while the first decodes
    // rows [0, B / 2) on the caller's - a decode is ~400 launches of very different shapes, two of them in flight fill each
    // other's tails and launch gaps (Uformer + 3 %, DPCRN + 2 %, CTSNet + 2.9 % at batch 256; rows are independent, the results are the
    // rows' own).  Not under the profiler (per-launch durations of concurrent launches are not what a roofline prices), not
    // for graph replay, ragged or frame-online calls.  SE_BATCH_SPLIT=0 / 1: off / on for every model.
    // (Uformer and DPCRN: THREE parts - + 1.5 % over two; CTSNet and TaylorSENet: two - a third loses for TaylorSENet)
    // DCCRN (and its causal-decoder configuration): two equal halves, + 1.8 % at batch 256 (profiles/dccrn_split.md).  Its conv
    // launches drain through a partly filled last round each, and the other half's launches fill it.  The forms meant to put one
    // part's LSTM section under the other part's convs were measured and lost to equal halves: unequal parts (SE_BATCH_LEAD) do hide
    // all of the recurrence (exposed 2.3 -> 0 ms in a kernel trace) but the smaller part ends at 3/4 of the step and the larger one
    // runs the rest alone, without a neighbour to fill its tails; a lower-priority twin stream hid it too and ended level, and still
    // lost 0.3 ms - the recurrence launches stretch from 1.1 to 1.6 ... 2.1 ms beside conv waves and slow those down for as long; three
    // parts lose more.  How a batch is cut is batch_parts.h; SE_BATCH_PARTS=1..3 and SE_BATCH_LEAD=4..12 (8: equal) reach the other cuts.
    static constexpr int MAX_TWINS = BATCH_PARTS_MAX - 1;
    int ntwins = 0;
    int split_lead = BATCH_LEAD_EQUAL;           // batch_parts.h: the first part's share of a split call
    std::unique_ptr<EngineCtx> ctx2[MAX_TWINS];
    std::unique_ptr<Model> twin[MAX_TWINS];      // (behind ctx2: the models go before their contexts)
    Event ev_tfork, ev_tjoin[MAX_TWINS];
    // se_stream_*: the samples received so far ([batch][max_samples]), frames transformed, samples emitted.
    // SE_CFG_STREAM_SLIDING: `wav` is a window [batch][pitch] whose column 0 holds the absolute sample w0 (stream_window.h);
    // a slide copies the live tail into `wav2` and swaps the two
    struct Stream {
        bool active = false;
        int batch = 0, max_chunk = 0, n_total = 0, t_done = 0, o_done = 0;
        int w0 = 0;
        long pitch = 0;          // floats per row of wav (max_samples, or stream_window_pitch())
        DevBuf<float> wav, wav2;
        // se_enhance_long / _ragged: the caller's resident rows (origin 0, not owned), read in place of `wav`; null in a stream
        const float* ext = nullptr;
        long ext_pitch = 0;
        int carve_B = -1, carve_n = -1;      // (batch, chunk frames) the arena was last carved and zero-filled for
        // running unit-RMS scale (se_stream_begin_running): sum of squares so far per stream, 1 / c per frame in a ring
        bool running = false;
        DevBuf<double> sumsq;
        DevBuf<float> frame_inv;
        int ring = 0;
        DevBuf<float> c;
        // SE_CFG_STREAM_ROW_ORIGINS: the rows' frame origins [max_batch] (made at create; EngineCtx::stream_origin points here), zero
        // in a stream that was begun, whatever its snapshot recorded in one that was restored
        DevBuf<int32_t> origin;
        // tracking unit-RMS scale (se_stream_begin_tracking): `sumsq` holds (E, W) per row, every frame has a scale of its own - c_t
        // in the ring frame_c for the forward transform, 1 / c_t in frame_inv for the inverse; lam = exp(-hop / tau) (1: tau == 0)
        bool tracking = false;
        float tau = 0.f;
        double lam = 1.0;
        DevBuf<float> frame_c;
        bool per_frame() const { return running || tracking; }
        int scale_mode() const { return tracking ? 2 : running ? 1 : 0; }      // SnapManifest::running
        // the hipStream the last push / flush / begin of this handle ran on: a new stream that starts on ANOTHER hipStream
        // re-uses (and clears) the parked state buffers, so it must be ordered behind the work still in flight there
        bool has_last = false;
        hipStream_t last_st = nullptr;
        Event ev_order;
        // a stream or a windowed decode starts: nothing received (or a whole clip of n_total_ samples), nothing done, no carve
        void start(int batch_, int n_total_, bool running_, bool tracking_ = false, float tau_ = 0.f, int hop = 1) {
            batch = batch_;
            n_total = n_total_;
            running = running_;
            tracking = tracking_;
            tau = tracking_ ? tau_ : 0.f;
            lam = tracking_ && tau_ > 0.f ? std::exp(-(double)hop / (double)tau_) : 1.0;
            t_done = o_done = w0 = 0;
            carve_B = carve_n = -1;
            ext = nullptr;
        }
    } strm;
};

// what se_last_error(NULL) reads: the error of a call without an engine.  One variable for both units (defined in engine.hip)
extern __attribute__((visibility("hidden"))) std::string g_create_err;

template <typename F>
int guard(se_engine* e, F&& f) {
    // the engine's device is current while the call runs; the caller's current device is restored on the way out
    int prev = -1;
    int rc = 0;
    try {
        if (e) {
            SE_HIP(hipGetDevice(&prev));
            if (prev != e->cfg.device) SE_HIP(hipSetDevice(e->cfg.device));
            else prev = -1;
        }
        f();
    } catch (const std::exception& ex) {
        if (e) e->err = ex.what();
        else g_create_err = ex.what();
        rc = 1;
    }
    if (prev >= 0) (void)hipSetDevice(prev);
    return rc;
}

// the ordering event of the handle's stream: left behind the last launch of every call that enqueues work on the arena, waited for
// by a call on ANOTHER hipStream (engine.hip ArenaCall has the rules)
inline void stream_mark(se_engine::Stream& S, hipStream_t st) {
    SE_HIP(hipEventRecord(S.ev_order.get(), st));
    S.has_last = true;
    S.last_st = st;
}
inline void stream_order_wait(se_engine::Stream& S, hipStream_t st) {
    if (S.has_last && S.last_st != st) SE_HIP(hipStreamWaitEvent(st, S.ev_order.get(), 0));
}

// what a frame-online stream and a windowed decode ask of the model's geometry, and how many frames one window launch takes
inline void check_stream_geometry(const se_engine* e) {
    const StftGeom& g = e->ctx.geom;
    SE_CHECK((g.n_fft + g.hop - 1) / g.hop - 1 + e->model->stream_lag() <= e->model->stream_hc(),
             "front end overlap + look-ahead exceed the history the model keeps");
}
// (the workspace holds `room` frames behind the model's history columns; dflt: the chunk of a call that names none)
inline int window_frames(const se_engine* e, int requested, int dflt) {
    const int room = std::max(1, e->plan_frames - e->model->stream_hc());
    return std::min(requested > 0 ? requested : dflt, room);
}

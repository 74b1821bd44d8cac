// C ABI of the engine (include/se_engine.h): handle, strict state-dict load, stage hooks.
#include "../../include/se_engine.h"
#include "hip_owned.h"
#include "model.h"
#include "resampler.h"
#include "rnn.h"
#include "batch_parts.h"
#include "stream_manifest.h"
#include "k_stream_state.h"
#include "stream_join.h"
#include "stream_rows.h"
#include "stream_window.h"
#include "window_rows.h"
#include <cmath>
#include <algorithm>
#include <climits>
#include <cstring>
#include <mutex>

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

static std::string g_create_err;

template <typename F>
static int guard(se_engine* e, F&& f) {
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

// the stage profiler is visible to the launchers only while a profiled call enqueues work
struct StageProfScope {
    explicit StageProfScope(se_engine* e) { set_stage_prof(e->ctx.prof.on ? &e->ctx.stage_prof : nullptr); }
    ~StageProfScope() { set_stage_prof(nullptr); }
};

extern "C" {

int64_t se_resample_samples(int32_t n_in, int32_t sr_in, int32_t sr_out) {
    if (n_in <= 0 || sr_in <= 0 || sr_out <= 0) return -1;
    return se::resample_out_samples(n_in, sr_in, sr_out);
}

int se_resample(const float* in_dev, int64_t in_pitch, int32_t batch, int32_t n_in, int32_t sr_in, int32_t sr_out,
                float* out_dev, int64_t out_pitch, void* stream) {
    return guard(nullptr, [&] {         // errors are reported through se_last_error(NULL)
        SE_CHECK(in_dev && out_dev, "null argument");
        SE_CHECK(in_pitch >= n_in && out_pitch >= se::resample_out_samples(n_in, sr_in, sr_out), "row pitch too small");
        se::launch_resample(in_dev, in_pitch, batch, n_in, sr_in, sr_out, out_dev, out_pitch, static_cast<hipStream_t>(stream));
    });
}

int se_resample_ragged(const void* in_dev, int32_t in_format, int64_t in_pitch, int32_t batch, const int32_t* n_in, int32_t sr_in,
                       int32_t sr_out, float* out_dev, int64_t out_pitch, void* stream) {
    return guard(nullptr, [&] {         // every refusal is the launcher's (resample_ragged.h), made before anything is enqueued
        se::launch_resample_ragged(in_dev, in_format, in_pitch, batch, n_in, sr_in, sr_out, out_dev, out_pitch, static_cast<hipStream_t>(stream));
    });
}

// the stateful resampler: an object of its own next to the engine (k_resample.hip), errors through se_last_error(NULL)
static se::StreamResampler* rs_of(se_resampler* r) { return reinterpret_cast<se::StreamResampler*>(r); }

int se_resampler_create(int32_t sr_in, int32_t sr_out, int32_t max_batch, int32_t max_push, se_resampler** out) {
    return guard(nullptr, [&] {
        SE_CHECK(out, "null argument");
        *out = reinterpret_cast<se_resampler*>(se::stream_resampler_create(sr_in, sr_out, max_batch, max_push));
    });
}
int se_resampler_destroy(se_resampler* r) {
    return guard(nullptr, [&] { se::stream_resampler_destroy(rs_of(r)); });
}
int se_resampler_begin(se_resampler* r, int32_t batch, void* stream) {
    return guard(nullptr, [&] {
        SE_CHECK(r, "null argument");
        se::stream_resampler_begin(rs_of(r), batch, static_cast<hipStream_t>(stream));
    });
}
int se_resampler_push(se_resampler* r, const float* in_dev, int64_t in_pitch, int32_t n_new, float* out_dev, int64_t out_pitch,
                      int32_t* n_out, void* stream) {
    return guard(nullptr, [&] {
        SE_CHECK(r && n_out, "null argument");
        *n_out = se::stream_resampler_push(rs_of(r), in_dev, in_pitch, n_new, out_dev, out_pitch, static_cast<hipStream_t>(stream));
    });
}
int se_resampler_flush(se_resampler* r, float* out_dev, int64_t out_pitch, int32_t* n_out, void* stream) {
    return guard(nullptr, [&] {
        SE_CHECK(r && n_out, "null argument");
        *n_out = se::stream_resampler_flush(rs_of(r), out_dev, out_pitch, static_cast<hipStream_t>(stream));
    });
}
int64_t se_resampler_ready_samples(int64_t n_in, int32_t sr_in, int32_t sr_out) {
    return se::resample_ready_samples(n_in, sr_in, sr_out);
}

// a parked signal of the stateful resampler (k_resample.hip, resampler_manifest.h)
static se::ResamplerState* rst_of(const se_resampler_state* s) {
    return reinterpret_cast<se::ResamplerState*>(const_cast<se_resampler_state*>(s));      // (the uploaded payload is a cache of the object)
}

int se_resampler_state_create(se_resampler_state** out) {
    return guard(nullptr, [&] {
        SE_CHECK(out, "se_resampler_state_create: null argument");
        *out = reinterpret_cast<se_resampler_state*>(se::resampler_state_create());
    });
}
int se_resampler_state_destroy(se_resampler_state* s) {
    return guard(nullptr, [&] { se::resampler_state_destroy(rst_of(s)); });
}
int64_t se_resampler_state_bytes(const se_resampler_state* s) { return se::resampler_state_bytes(rst_of(s)); }
int se_resampler_state_counts(const se_resampler_state* s, int32_t* sr_in, int32_t* sr_out, int32_t* batch, int64_t* n_in, int64_t* n_out) {
    return guard(nullptr, [&] { se::resampler_state_counts(rst_of(s), sr_in, sr_out, batch, n_in, n_out); });
}
int se_resampler_save(se_resampler* r, se_resampler_state* s, void* stream) {
    return guard(nullptr, [&] {
        SE_CHECK(r && s, "se_resampler_save: null argument");
        se::stream_resampler_save(rs_of(r), rst_of(s), static_cast<hipStream_t>(stream));
    });
}
int se_resampler_restore(se_resampler* r, const se_resampler_state* s, void* stream) {
    return guard(nullptr, [&] {
        SE_CHECK(r && s, "se_resampler_restore: null argument");
        se::stream_resampler_restore(rs_of(r), rst_of(s), static_cast<hipStream_t>(stream));
    });
}
int64_t se_resampler_state_export(const se_resampler_state* s, void* host_buf, int64_t cap) {
    int64_t ret = -1;
    guard(nullptr, [&] { ret = se::resampler_state_export(rst_of(s), host_buf, cap); });
    return ret;
}
int se_resampler_state_import(se_resampler_state* s, const void* host_buf, int64_t bytes) {
    return guard(nullptr, [&] { se::resampler_state_import(rst_of(s), host_buf, bytes); });
}

int se_resampler_state_select(se_resampler_state* dst, const se_resampler_state* src, const int32_t* rows, int32_t n_rows, void* stream) {
    return guard(nullptr, [&] { se::resampler_state_select(rst_of(dst), rst_of(src), rows, n_rows, static_cast<hipStream_t>(stream)); });
}
int se_resampler_state_concat(se_resampler_state* dst, const se_resampler_state* const* parts, int32_t n_parts, void* stream) {
    return guard(nullptr, [&] {
        se::resampler_state_concat(rst_of(dst), reinterpret_cast<se::ResamplerState* const*>(const_cast<se_resampler_state* const*>(parts)), n_parts,
                                   static_cast<hipStream_t>(stream));
    });
}
int se_resampler_state_join(se_resampler_state* dst, const se_resampler_state* const* parts, int32_t n_parts, void* stream) {
    return guard(nullptr, [&] {
        se::resampler_state_join(rst_of(dst), reinterpret_cast<se::ResamplerState* const*>(const_cast<se_resampler_state* const*>(parts)), n_parts,
                                 static_cast<hipStream_t>(stream));
    });
}

int se_pcm16_decode(const int16_t* in_dev, int64_t in_pitch, int32_t batch, int32_t n, float* out_dev, int64_t out_pitch,
                    void* stream) {
    return guard(nullptr, [&] {
        SE_CHECK(in_dev && out_dev, "null argument");
        SE_CHECK(batch == 1 || (in_pitch >= n && out_pitch >= n), "row pitch too small");
        se::launch_pcm16_decode(in_dev, in_pitch, batch, n, out_dev, out_pitch, static_cast<hipStream_t>(stream));
    });
}

int se_pcm16_encode(const float* in_dev, int64_t in_pitch, int32_t batch, int32_t n, int16_t* out_dev, int64_t out_pitch,
                    void* stream) {
    return guard(nullptr, [&] {
        SE_CHECK(in_dev && out_dev, "null argument");
        SE_CHECK(batch == 1 || (in_pitch >= n && out_pitch >= n), "row pitch too small");
        se::launch_pcm16_encode(in_dev, in_pitch, batch, n, out_dev, out_pitch, static_cast<hipStream_t>(stream));
    });
}

int32_t se_abi_version(void) { return 5; }

const char* se_last_error(const se_engine* e) { return e ? e->err.c_str() : g_create_err.c_str(); }

static std::unique_ptr<Model> make_model(int id, EngineCtx& c) {
    switch (id) {
        case SE_MODEL_DCCRN: return make_dccrn(c);
        case SE_MODEL_CRN: return make_crn(c);
        case SE_MODEL_LSTM: return make_lstm(c);
        case SE_MODEL_DPCRN: return make_dpcrn(c);
        case SE_MODEL_GCRN: return make_gcrn(c);
        case SE_MODEL_CTSNET: return make_ctsnet(c);
        case SE_MODEL_TAYLORSENET: return make_taylorsenet(c);
        case SE_MODEL_G2NET: return make_g2net(c);
        case SE_MODEL_UFORMER: return make_uformer(c);
        case SE_MODEL_FULLSUBNET: return make_fullsubnet(c);
        default: SE_CHECK(false, "model id " + std::to_string(id) + " is not built into this engine yet");
    }
    return nullptr;
}
// The stream the second half-batch runs on: the first of the process-wide auxiliary streams (model.h) - the models that split
// do not fork, so it is free during their decodes.  NOT a stream of its own: the runtime maps streams onto four hardware queues
// by default; with a fifth stream in the process (caller's + three auxiliary + this one) two of them shared a queue and G2Net's
// three-stream fork, built later in the same process, ran slower than on one stream (0.448 -> 0.417 in bench.py's zoo).
static hipStream_t twin_stream(int dev, int i = 0) { return EngineCtx::shared_aux(dev, i); }
static std::string why_not_causal(const se_engine* e);

int se_engine_create(const se_config* cfg, se_engine** out) {
    se_engine* e = nullptr;
    int prev_dev = -1;
    (void)hipGetDevice(&prev_dev);
    int rc = guard(nullptr, [&] {
        SE_CHECK(cfg && out, "null argument");
        int ndev = 0;
        SE_HIP(hipGetDeviceCount(&ndev));
        SE_CHECK(ndev > 0, "no HIP device visible: the engine has no CPU fallback");
        SE_CHECK(cfg->device >= 0 && cfg->device < ndev, "device ordinal out of range");
        SE_HIP(hipSetDevice(cfg->device));
        hipDeviceProp_t prop;
        SE_HIP(hipGetDeviceProperties(&prop, cfg->device));
        SE_CHECK(std::string(prop.gcnArchName).rfind("gfx950", 0) == 0,
                 std::string("built for gfx950 (MI355X) only, device is ") + prop.gcnArchName);
        e = new se_engine();
        e->cfg = *cfg;
        e->ctx.max_batch = cfg->max_batch > 0 ? cfg->max_batch : 1;
        e->ctx.max_samples = cfg->max_samples > 0 ? cfg->max_samples : 64000;
        e->ctx.p_in = cfg->p_in > 0.f ? cfg->p_in : 1.f;
        e->ctx.p_out = cfg->p_out > 0.f ? cfg->p_out : 1.f;
        e->ctx.flags = cfg->flags;
        // (the bit names a remedy for DCCRN's look-ahead decoder alone: anywhere else it would be carried along without a meaning)
        SE_CHECK(!(cfg->flags & SE_CFG_DCCRN_ROW_ENDS) || cfg->model == SE_MODEL_DCCRN,
                 "SE_CFG_DCCRN_ROW_ENDS is a bit of SE_MODEL_DCCRN (the per-layer zero tails its look-ahead decoder needs in "
                 "se_enhance_long_ragged): no other model takes it");
        SE_CHECK(!(cfg->flags & SE_CFG_DCCRN_ROW_ENDS) || !(cfg->flags & SE_CFG_DCCRN_CAUSAL_DEC),
                 "SE_CFG_DCCRN_ROW_ENDS does not combine with SE_CFG_DCCRN_CAUSAL_DEC: the causal decoder looks back, not ahead, and "
                 "se_enhance_long_ragged accepts it without the bit");
        // (FullSubNet's norm_type, base_model.py:296-308: offline_laplace_norm is no bit; the other three exclude one another)
        {
            const uint32_t norms = SE_CFG_FSN_GAUSSIAN | SE_CFG_FSN_CUM_LAYERNORM;
            SE_CHECK(!(cfg->flags & norms) || cfg->model == SE_MODEL_FULLSUBNET,
                     "SE_CFG_FSN_GAUSSIAN and SE_CFG_FSN_CUM_LAYERNORM are bits of SE_MODEL_FULLSUBNET (its norm_type, "
                     "offline_gaussian_norm / cumulative_layer_norm): no other model takes them");
            const int nnorm = !!(cfg->flags & SE_CFG_FSN_CUMULATIVE) + !!(cfg->flags & SE_CFG_FSN_GAUSSIAN) + !!(cfg->flags & SE_CFG_FSN_CUM_LAYERNORM);
            SE_CHECK(cfg->model != SE_MODEL_FULLSUBNET || nnorm <= 1,
                     "FullSubNet has one norm_type: at most one of SE_CFG_FSN_CUMULATIVE, SE_CFG_FSN_GAUSSIAN and SE_CFG_FSN_CUM_LAYERNORM");
        }
        // (per-row frame origins are read by the kernels of the models whose state counts frames, and by nothing else)
        if (cfg->flags & SE_CFG_STREAM_ROW_ORIGINS) {
            const bool cln = cfg->model == SE_MODEL_CTSNET || cfg->model == SE_MODEL_G2NET || cfg->model == SE_MODEL_TAYLORSENET;
            const bool fsn = cfg->model == SE_MODEL_FULLSUBNET && (cfg->flags & (SE_CFG_FSN_CUMULATIVE | SE_CFG_FSN_CUM_LAYERNORM)) && !(cfg->flags & SE_CFG_FSN_GRU);
            SE_CHECK(cln || fsn,
                     "SE_CFG_STREAM_ROW_ORIGINS is a bit of the models whose stream state counts frames - SE_MODEL_CTSNET, SE_MODEL_G2NET, "
                     "SE_MODEL_TAYLORSENET, and SE_MODEL_FULLSUBNET with SE_CFG_FSN_CUMULATIVE or SE_CFG_FSN_CUM_LAYERNORM and without SE_CFG_FSN_GRU: no other "
                     "configuration takes it (the others are joined without it)");
            e->strm.origin.alloc((size_t)e->ctx.max_batch);
            SE_HIP(hipMemset(e->strm.origin.get(), 0, (size_t)e->ctx.max_batch * sizeof(int32_t)));
            e->ctx.stream_origin = e->strm.origin.get();
        }
        e->model = make_model(cfg->model, e->ctx);
        e->ctx.geom = e->model->default_geom();
        if (cfg->n_fft > 0) {
            SE_CHECK(cfg->n_fft == e->ctx.geom.n_fft, "n_fft override must match the model's front end");
            e->ctx.geom = StftGeom{cfg->n_fft, cfg->hop > 0 ? cfg->hop : e->ctx.geom.hop, cfg->win > 0 ? cfg->win : cfg->n_fft};
        }
        static const int split_env = getenv("SE_BATCH_SPLIT") ? atoi(getenv("SE_BATCH_SPLIT")) : -1;
        static const int parts_env = getenv("SE_BATCH_PARTS") ? atoi(getenv("SE_BATCH_PARTS")) : 0;
        static const int lead_env = getenv("SE_BATCH_LEAD") ? atoi(getenv("SE_BATCH_LEAD")) : 0;
        const bool split = split_env >= 0 ? split_env != 0
                                          : (cfg->model == SE_MODEL_UFORMER || cfg->model == SE_MODEL_DPCRN || cfg->model == SE_MODEL_CTSNET ||
                                             cfg->model == SE_MODEL_TAYLORSENET || cfg->model == SE_MODEL_DCCRN);
        if (split && e->ctx.max_batch >= BATCH_SPLIT_MIN) {
            const int parts = parts_env >= 1 && parts_env <= BATCH_PARTS_MAX ? parts_env
                              : (cfg->model == SE_MODEL_UFORMER || cfg->model == SE_MODEL_DPCRN) ? 3 : 2;
            e->ntwins = parts - 1;
            e->split_lead = lead_env >= BATCH_LEAD_MIN && lead_env <= BATCH_LEAD_MAX ? lead_env : BATCH_LEAD_EQUAL;
            for (int i = 0; i < e->ntwins; ++i) {
                e->ctx2[i].reset(new EngineCtx());
                // equal parts: the first twin a half (two-part calls), the second a third; unequal: the largest part any call hands it
                e->ctx2[i]->max_batch = e->split_lead == BATCH_LEAD_EQUAL ? (e->ctx.max_batch + i + 1) / (i + 2)
                                                                          : std::max(1, batch_parts_twin_rows(e->ctx.max_batch, e->ntwins, e->split_lead, i));
                e->ctx2[i]->max_samples = e->ctx.max_samples;
                e->ctx2[i]->p_in = e->ctx.p_in;
                e->ctx2[i]->p_out = e->ctx.p_out;
                e->ctx2[i]->flags = e->ctx.flags;
                e->twin[i] = make_model(cfg->model, *e->ctx2[i]);
                e->ctx2[i]->geom = e->ctx.geom;
            }
        }
        *out = e;
        scratch_engine_created(cfg->device);
    });
    if (rc && e) {
        delete e;
    }
    if (prev_dev >= 0) (void)hipSetDevice(prev_dev);
    return rc;
}

int se_engine_destroy(se_engine* e) {
    if (!e) return 0;
    int prev_dev = -1;
    (void)hipGetDevice(&prev_dev);
    (void)hipSetDevice(e->cfg.device);
    (void)hipDeviceSynchronize();
    for (auto& g : e->graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    // (the tile kernels' over-read ranges are dropped before `delete e` releases the arenas they name)
    if (e->ctx.arena.base()) gc_unregister_overread_range(e->ctx.arena.base());
    for (auto& c2 : e->ctx2)
        if (c2 && c2->arena.base()) gc_unregister_overread_range(c2->arena.base());
    const int dev = e->cfg.device;
    delete e;
    scratch_engine_destroyed(dev);      // the device's last engine takes the engine-lifetime scratch slots with it
    if (prev_dev >= 0) (void)hipSetDevice(prev_dev);
    return 0;
}

int se_engine_set_tensor(se_engine* e, const char* key, const void* data, const int64_t* shape, int32_t ndim,
                         int32_t dtype) {
    if (!e) return 1;
    return guard(e, [&] {
        SE_CHECK(!e->finalized, "set_tensor after finalize");
        SE_CHECK(key && (data || ndim == 0) && ndim >= 0 && ndim <= 8, "bad argument");
        HostTensor t;
        int64_t n = 1;
        for (int i = 0; i < ndim; ++i) {
            SE_CHECK(shape[i] >= 0, "negative dim");
            t.shape.push_back(shape[i]);
            n *= shape[i];
        }
        if (dtype == 0) {
            t.data.assign(static_cast<const float*>(data), static_cast<const float*>(data) + n);
        } else if (dtype == 1) {
            t.data.resize(n);
            for (int64_t i = 0; i < n; ++i) t.data[i] = (float)static_cast<const int64_t*>(data)[i];
        } else {
            SE_CHECK(false, "dtype must be 0 (float32) or 1 (int64)");
        }
        e->sd[key] = std::move(t);
    });
}

int se_engine_finalize(se_engine* e) {
    if (!e) return 1;
    return guard(e, [&] {
        SE_CHECK(!e->finalized, "already finalized");
        TrackedSD tsd(e->sd);
        e->model->finalize(tsd);
        tsd.check_all_used();
        // size the workspace for (max_batch, frames of max_samples)
        const int T = e->model->num_frames(e->ctx.max_samples);
        // (a frame-online window is the model's history columns + the chunk: models that keep a long history - CTSNet_new's
        // dilated convs reach 128 frames back - must be able to stream through an engine created for short clips)
        // (models that look ahead run with the frame count rounded up to whole 16 B groups: model.h PadFrames)
        const int fm = pad_frames_mult(e->model->frame_multiple());
        const int Tr = (T + fm - 1) / fm * fm;
        e->plan_frames = e->model->stream_supported() ? std::max(Tr, e->model->stream_hc() + 16) : Tr;
        // a model's layout may depend on the batch (FullSubNet keeps a [T][4H][S] gate tensor below 16 clips and none from 16
        // on, so 15 clips need more than 16...42): the arena covers every batch a call may bring, not only the largest
        // ... and a layout may depend on the window length: FullSubNet's frame-online windows (<= 64 frames) always keep the
        // sub-band gate tensor, at every batch - a stream of 32 rows on an engine made for short clips needs more for a
        // 58-frame chunk than the offline plan at plan_frames holds: the short-window plan is measured too
        size_t need = 0;
        for (int bq : {e->ctx.max_batch, std::min(e->ctx.max_batch, 15)})
            for (int tq : {e->plan_frames, std::min(e->plan_frames, 64)}) {
                if (tq != e->plan_frames && !e->model->stream_supported()) continue;
                e->ctx.arena.measure_begin();
                e->model->plan_buffers(bq, tq);
                need = std::max(need, e->ctx.arena.measure_end());
            }
        e->ctx.arena.reserve(need + (1 << 20));
        gc_register_overread_range(e->ctx.arena.base(), e->ctx.arena.capacity());
        e->model->plan_buffers(e->ctx.max_batch, T);
        for (int i = 0; i < e->ntwins; ++i) {          // the other instances: the same tensors, a workspace for their part of the batch (offline decodes only)
            TrackedSD tsd2(e->sd);
            e->twin[i]->finalize(tsd2);
            size_t need2 = 0;
            for (int bq : {e->ctx2[i]->max_batch, std::min(e->ctx2[i]->max_batch, 15)}) {
                e->ctx2[i]->arena.measure_begin();
                e->twin[i]->plan_buffers(bq, Tr);
                need2 = std::max(need2, e->ctx2[i]->arena.measure_end());
            }
            e->ctx2[i]->arena.reserve(need2 + (1 << 20));
            gc_register_overread_range(e->ctx2[i]->arena.base(), e->ctx2[i]->arena.capacity());
            e->twin[i]->plan_buffers(e->ctx2[i]->max_batch, T);
        }
        e->sd.clear();
        SE_HIP(hipDeviceSynchronize());
        e->finalized = true;
    });
}

// The preamble and the epilogue of every call that enqueues work on the arena, in one scope.
// A call that re-carves the arena (RECARVE: every offline decode; TAKE_OVER: the windowed decodes, which also end a running
// stream) first tells a stream running on this handle to zero-fill its next windows (carve_B), then orders itself behind the
// last call made on ANOTHER hipStream - the event stream_mark() recorded there - so that it cannot overwrite windows that call
// is still reading.  se_stream_push / _flush only mark (MARK_ONLY).
// ... and the other direction: EVERY such call leaves the ordering event behind its last launch, also when it
// throws after enqueueing, so that a se_stream_begin issued on another hipStream right after it cannot re-carve or zero-fill
// the arena under it
static void stream_mark(se_engine::Stream& S, hipStream_t st) {
    SE_HIP(hipEventRecord(S.ev_order.get(), st));
    S.has_last = true;
    S.last_st = st;
}
static void stream_order_wait(se_engine::Stream& S, hipStream_t st) {
    if (S.has_last && S.last_st != st) SE_HIP(hipStreamWaitEvent(st, S.ev_order.get(), 0));
}
struct ArenaCall {
    enum Mode { MARK_ONLY, RECARVE, TAKE_OVER };
    se_engine::Stream& S;
    hipStream_t st;
    ArenaCall(se_engine* e, hipStream_t st_, Mode mode = RECARVE) : S(e->strm), st(st_) {
        if (mode == MARK_ONLY) return;
        if (mode == TAKE_OVER) S.active = false;
        S.carve_B = -1;
        stream_order_wait(S, st);
    }
    ~ArenaCall() {
        try {
            stream_mark(S, st);
        } catch (const std::exception&) {      // (a failed record leaves the previous event in place)
        }
    }
    ArenaCall(const ArenaCall&) = delete;
    ArenaCall& operator=(const ArenaCall&) = delete;
};

int se_forward(se_engine* e, const float* in_dev, const int64_t* in_shape, int32_t in_ndim, float* out_dev,
               void* stream) {
    if (!e) return 1;
    return guard(e, [&] {
        SE_CHECK(e->finalized, "engine not finalized");
        ArenaCall call(e, static_cast<hipStream_t>(stream));
        SE_CHECK(in_dev && out_dev && in_shape, "null argument");
        e->ctx.prof_reset();
        e->model->forward(in_dev, in_shape, in_ndim, out_dev, static_cast<hipStream_t>(stream));
    });
}

int se_uformer_forward(se_engine* e, const float* inputs_dev, const float* src_dev, int32_t batch, int32_t n_samples,
                       float* output_dev, float* src_out_dev, float* output_cplx_dev, float* src_cplx_dev, void* stream) {
    if (!e) return 1;
    return guard(e, [&] {
        SE_CHECK(e->finalized, "engine not finalized");
        ArenaCall call(e, static_cast<hipStream_t>(stream));
        SE_CHECK(inputs_dev && output_dev, "null argument");
        SE_CHECK(batch >= 1 && batch <= e->ctx.max_batch, "batch exceeds max_batch given at create");
        SE_CHECK(n_samples >= e->ctx.geom.n_fft && n_samples <= e->ctx.max_samples, "n_samples outside [n_fft, max_samples]");
        e->ctx.prof_reset();
        e->model->forward_uformer(inputs_dev, src_dev, batch, n_samples, output_dev, src_out_dev, output_cplx_dev, src_cplx_dev,
                                  static_cast<hipStream_t>(stream));
    });
}

int se_enhance_batch(se_engine* e, const float* wav_in_dev, int64_t in_pitch, int32_t batch, int32_t n_samples,
                     float* wav_out_dev, int64_t out_pitch, void* stream) {
    if (!e) return 1;
    return guard(e, [&] {
        SE_CHECK(e->finalized, "engine not finalized");
        ArenaCall call(e, static_cast<hipStream_t>(stream));
        SE_CHECK(wav_in_dev && wav_out_dev, "null argument");
        SE_CHECK(batch >= 1 && batch <= e->ctx.max_batch, "batch exceeds max_batch given at create");
        SE_CHECK(n_samples >= e->ctx.geom.n_fft && n_samples <= e->ctx.max_samples,
                 "n_samples outside [n_fft, max_samples]");
        SE_CHECK(in_pitch >= n_samples && out_pitch >= e->model->output_samples(n_samples), "row pitch too small");
        e->ctx.prof_reset();
        StageProfScope sps(e);
        hipStream_t st = static_cast<hipStream_t>(stream);
        static const int graphs_env = getenv("SE_GRAPH") ? atoi(getenv("SE_GRAPH")) : -1;
        const bool want_graph = (graphs_env >= 0 ? graphs_env != 0 : (e->cfg.flags & SE_CFG_GRAPHS) != 0) && !e->ctx.prof.on &&
                                e->model->graph_capturable();
        if (!want_graph) {
            // (batch_parts.h: three parts from 192 clips on where the model has them, else two; equal or unequal by split_lead)
            const BatchParts bp = e->ctx.prof.on ? BatchParts() : batch_parts_cut(batch, batch_parts_count(batch, e->ntwins), e->split_lead);
            if (bp.n > 1) {
                struct Active {
                    Active() { batch_split_active() = true; }
                    ~Active() { batch_split_active() = false; }
                } active;
                // the caller's stream joins every twin recorded so far, also when a later enhance() throws: their work still
                // reads wav_in and writes wav_out; a failing wait is swallowed, as a failing mark is
                struct TwinJoin {
                    se_engine* e;
                    hipStream_t st;
                    int n = 0;
                    ~TwinJoin() {
                        try {
                            for (int i = 0; i < n; ++i) (void)hipStreamWaitEvent(st, e->ev_tjoin[i].get(), 0);
                        } catch (const std::exception&) {
                        }
                    }
                } join{e, st};
                SE_HIP(hipEventRecord(e->ev_tfork.get(), st));
                for (int i = 0; i < bp.n - 1; ++i) {
                    const int r0 = bp.r0[i + 1], nr = bp.rows[i + 1];
                    SE_CHECK(nr <= e->ctx2[i]->max_batch, "a part of the batch exceeds its instance's workspace");
                    hipStream_t s2 = twin_stream(e->cfg.device, i);
                    SE_HIP(hipStreamWaitEvent(s2, e->ev_tfork.get(), 0));
                    e->twin[i]->enhance(wav_in_dev + (size_t)r0 * in_pitch, in_pitch, nr, n_samples, wav_out_dev + (size_t)r0 * out_pitch,
                                        out_pitch, s2);
                    SE_HIP(hipEventRecord(e->ev_tjoin[i].get(), s2));
                    join.n = i + 1;
                }
                e->model->enhance(wav_in_dev, in_pitch, bp.rows[0], n_samples, wav_out_dev, out_pitch, st);
                return;
            }
            e->model->enhance(wav_in_dev, in_pitch, batch, n_samples, wav_out_dev, out_pitch, st);
            return;
        }
        const int64_t n_out = e->model->output_samples(n_samples);
        se_engine::GraphEntry* ge = nullptr;
        for (auto& g : e->graphs)
            if (g.batch == batch && g.samples == n_samples) ge = &g;
        if (!ge) {
            const std::pair<int, int> key(batch, n_samples);
            // capture on the engine-owned stream: the caller's stream may be the legacy default stream, which cannot capture
            hipStream_t cs = e->cap_stream.get();
            if (std::find(e->warmed.begin(), e->warmed.end(), key) == e->warmed.end()) {
                // first call of a shape: eager, but on the capture stream (fork / join around the caller's stream) so that
                // the lazily grown scratch buffers - keyed by stream - already exist when the shape is captured
                e->warmed.push_back(key);
                SE_HIP(hipEventRecord(e->ev_fork.get(), st));
                SE_HIP(hipStreamWaitEvent(cs, e->ev_fork.get(), 0));
                e->model->enhance(wav_in_dev, in_pitch, batch, n_samples, wav_out_dev, out_pitch, cs);
                SE_HIP(hipEventRecord(e->ev_join.get(), cs));
                SE_HIP(hipStreamWaitEvent(st, e->ev_join.get(), 0));
                return;
            }
            if (!e->stage_in) {
                const int64_t max_out = e->model->output_samples(e->ctx.max_samples);
                e->stage_in.alloc((size_t)e->ctx.max_batch * e->ctx.max_samples);
                e->stage_out.alloc((size_t)e->ctx.max_batch * max_out);
            }
            hipGraph_t graph = nullptr;
            hipGraphExec_t exec = nullptr;
            SE_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
            bool ok = true;
            try {
                e->model->enhance(e->stage_in.get(), n_samples, batch, n_samples, e->stage_out.get(), n_out, cs);
            } catch (const std::exception&) {
                ok = false;
            }
            if (hipStreamEndCapture(cs, &graph) != hipSuccess || !graph) ok = false;
            if (ok && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) ok = false;
            if (graph) (void)hipGraphDestroy(graph);
            (void)hipGetLastError();
            if (getenv("SE_GRAPH_DEBUG"))
                fprintf(stderr, "se_graph: %s (batch %d, samples %d)\n", ok ? "captured" : "capture failed", batch, n_samples);
            e->graphs.push_back({batch, n_samples, ok ? exec : nullptr});
            ge = &e->graphs.back();
        }
        if (!ge->exec) {
            e->model->enhance(wav_in_dev, in_pitch, batch, n_samples, wav_out_dev, out_pitch, st);
            return;
        }
        SE_HIP(hipMemcpy2DAsync(e->stage_in.get(), (size_t)n_samples * sizeof(float), wav_in_dev, (size_t)in_pitch * sizeof(float),
                                (size_t)n_samples * sizeof(float), batch, hipMemcpyDeviceToDevice, st));
        SE_HIP(hipGraphLaunch(ge->exec, st));
        SE_HIP(hipMemcpy2DAsync(wav_out_dev, (size_t)out_pitch * sizeof(float), e->stage_out.get(), (size_t)n_out * sizeof(float),
                                (size_t)n_out * sizeof(float), batch, hipMemcpyDeviceToDevice, st));
    });
}

// the per-row sizes of a ragged call (len | lpad | tlen | olen of rows 0..batch-1), host -> device through the next pinned slot
static Ragged upload_row_sizes(se_engine* e, int batch, const int32_t* lengths, hipStream_t st) {
    const int MB = e->ctx.max_batch;
    if (!e->rag_host) {
        e->rag_host.alloc((size_t)4 * MB * se_engine::RAG_SLOTS);
        e->rag_dev.alloc((size_t)4 * MB * se_engine::RAG_SLOTS);
    }
    const int slot = e->rag_next;
    e->rag_next = (slot + 1) % se_engine::RAG_SLOTS;
    SE_HIP(hipEventSynchronize(e->rag_ev[slot].get()));      // the copy that last used this slot has run (no-op when unused)
    int* h = e->rag_host.get() + (size_t)slot * 4 * MB;
    int* d = e->rag_dev.get() + (size_t)slot * 4 * MB;
    const int hop = e->ctx.geom.hop;
    for (int b = 0; b < batch; ++b) {
        const int L = lengths[b], Lp = e->model->padded_samples(L);
        h[b] = L;
        h[MB + b] = Lp;
        h[2 * MB + b] = 1 + Lp / hop;
        h[3 * MB + b] = (int)e->model->output_samples(L);
    }
    SE_HIP(hipMemcpyAsync(d, h, sizeof(int) * 4 * MB, hipMemcpyHostToDevice, st));
    SE_HIP(hipEventRecord(e->rag_ev[slot].get(), st));
    return Ragged{d, d + MB, d + 2 * MB, d + 3 * MB};
}
// the per-row sizes are visible to the launchers only while this scope enqueues work (null: nothing is published)
struct RaggedScope {
    const bool on;
    explicit RaggedScope(const Ragged* r) : on(r != nullptr) {
        if (on) set_ragged_ctx(r);
    }
    ~RaggedScope() {
        if (on) set_ragged_ctx(nullptr);
    }
    RaggedScope(const RaggedScope&) = delete;
    RaggedScope& operator=(const RaggedScope&) = delete;
};

// the rows' whole-clip frame counts for a model that cuts its own tensors at each row's end (window_rows.h), while this scope enqueues
struct WindowEndsScope {
    const bool on;
    explicit WindowEndsScope(const WindowEnds* w) : on(w != nullptr) {
        if (on) set_window_ends_ctx(w);
    }
    ~WindowEndsScope() {
        if (on) set_window_ends_ctx(nullptr);
    }
    WindowEndsScope(const WindowEndsScope&) = delete;
    WindowEndsScope& operator=(const WindowEndsScope&) = delete;
};

int se_enhance_ragged(se_engine* e, const float* wav_in_dev, int64_t in_pitch, int32_t batch, const int32_t* lengths,
                      float* wav_out_dev, int64_t out_pitch, void* stream) {
    if (!e) return 1;
    return guard(e, [&] {
        SE_CHECK(e->finalized, "engine not finalized");
        ArenaCall call(e, static_cast<hipStream_t>(stream));
        SE_CHECK(wav_in_dev && wav_out_dev && lengths, "null argument");
        SE_CHECK(batch >= 1 && batch <= e->ctx.max_batch, "batch exceeds max_batch given at create");
        SE_CHECK(e->model->ragged_supported(),
                 "this model looks ahead in time (non-causal convolutions / attention): batch only clips of equal length");
        int Lmax = 0;
        for (int b = 0; b < batch; ++b) {
            SE_CHECK(lengths[b] >= e->ctx.geom.n_fft && lengths[b] <= e->ctx.max_samples,
                     "lengths[" + std::to_string(b) + "] outside [n_fft, max_samples]");
            Lmax = std::max(Lmax, (int)lengths[b]);
        }
        SE_CHECK(in_pitch >= Lmax && out_pitch >= e->model->output_samples(Lmax), "row pitch too small");
        hipStream_t st = static_cast<hipStream_t>(stream);
        const Ragged rg = upload_row_sizes(e, batch, lengths, st);
        e->ctx.prof_reset();
        StageProfScope sps(e);
        RaggedScope scope(&rg);
        e->model->enhance(wav_in_dev, in_pitch, batch, Lmax, wav_out_dev, out_pitch, st);
    });
}

// frames [e->strm.t_done, t_end) of the stream through the network, then every output sample they complete (all of them up to
// the end when `last`); the samples are appended to out row b at out_dev[b * out_pitch + *written ...].  The input rows are the
// stream's own window (S.wav, pitch S.pitch, origin S.w0) or, for se_enhance_long, the caller's resident clip (S.ext, origin 0)
// `rows` (se_enhance_long_ragged; null otherwise): the rows' own sizes over their whole clips, absolute.  S.n_total / t_end are then
// those of the LONGEST row.  The STFT and the iSTFT count frames and samples absolutely inside a window too, so a row's sample
// counts (len, lpad, olen) mean in a window what they mean offline: its reflected edge and tail pad fall into whichever window holds
// its end, its samples from olen[b] on are zeros in every window.  Its FRAME count does not carry over as it is: a window launch owns
// the frames below its own bound only (the STFT's t0 + n, the iSTFT's t_fin) - with the whole-clip count the forward transform would
// pair the window's last frame with a frame of the next window, and the inverse would load and transform columns past the window.
// Each of the two launches therefore gets a view with tlen[b] = min(tlen[b], its bound), made on the device in stream order
// (window_rows.h): a row that has not ended sees the bound an equal-length launch has, a row that has ended its own last frame - its
// frames from there on are written as zeros and never overlap-added.  The network is causal and runs as for rows of one length,
// without per-row sizes: past its end a row is fed zero frames.  That is exact for a look-ahead at the network's INPUT (FullSubNet,
// cumulative norm: the zero frames `last` appends are the ones the STFT wrote); a model that looks ahead behind its input layer (the
// `_vb` DCCRN's decoder) needs zeros behind every layer: an engine made with SE_CFG_DCCRN_ROW_ENDS gets the rows' whole-clip frame
// counts and the window origin through a context of its own (window_rows.h WindowEnds), published around stream_chunk only - never
// together with the ragged context - and clears the columns at or past each row's end itself; without the bit the caller refuses it.
static void stream_process(se_engine* e, int t_end, bool last, float* out_dev, int64_t out_pitch, int* written, hipStream_t st,
                           const Ragged* rows = nullptr) {
    se_engine::Stream& S = e->strm;
    const float* wav = S.ext ? S.ext : S.wav.get();
    const long pitch = S.ext ? S.ext_pitch : S.pitch;
    const int w0 = S.w0;
    const StftGeom& g = e->ctx.geom;
    const int HC = e->model->stream_hc(), LAG = e->model->stream_lag(), B = S.batch;
    // a frame that is transformed before the end of the stream never touches the end reflection / the tail padding
    // (se_stream_push only releases frames whose last sample has arrived); at the end the decode script's padded length
    const int Lpad = last ? e->model->padded_samples(S.n_total) : S.n_total;
    const int n_final = last ? (int)e->model->output_samples(S.n_total) : S.n_total;
    const int MB = e->ctx.max_batch;
    if (rows && !e->rag_win) e->rag_win.alloc((size_t)4 * MB);
    // (one buffer: a view, the launch that reads it and the next view follow one another on `st`; rows->len is the base of the
    // uploaded [4][MB] block, upload_row_sizes)
    int* const rw = e->rag_win.get();
    const Ragged win{rw, rw + MB, rw + 2 * MB, rw + 3 * MB};
    const Ragged* view = rows ? &win : nullptr;
    while (S.t_done < t_end) {
        const int t0 = S.t_done, n = std::min(S.max_chunk, t_end - t0), Tw = HC + n;
        float *spec = nullptr, *mag = nullptr, *est = nullptr;
        e->model->stream_bufs(B, n, &spec, &mag, &est);
        // A chunk size that differs from the last one re-carves the arena: the history columns of the new windows would hold
        // whatever the old carve left there.  Layers only look at the columns their taps reach (restored from the state),
        // but zero-weight padding of the matrix operands may touch a neighbouring column - finite values are harmless there,
        // stale bit patterns need not be finite.
        if (S.carve_B != B || S.carve_n != n) {
            SE_HIP(hipMemsetAsync(const_cast<void*>(e->ctx.arena.base()), 0, e->ctx.arena.used(), st));
            S.carve_B = B;
            S.carve_n = n;
        }
        {
            if (rows) launch_window_rows(rows->len, rw, MB, B, t0 + n, st);
            RaggedScope rs(view);
            launch_stft(g, wav, pitch, B, S.n_total, Lpad, S.c.get(), e->ctx.p_in, spec, mag, t0 + n, Tw, st, t0, HC, w0,
                        S.tracking ? S.frame_c.get() : nullptr, S.ring);
        }
        {
            const WindowEnds ends{rows ? rows->tlen : nullptr, t0};
            WindowEndsScope ws(rows && (e->cfg.flags & SE_CFG_DCCRN_ROW_ENDS) ? &ends : nullptr);
            e->model->stream_chunk(B, t0, n, st, last && t0 + n == t_end);
        }
        S.t_done = t0 + n;
        const bool end = last && S.t_done == t_end;
        // estimate frames below t_fin are final (a model that looks ahead finalises LAG frames late); samples whose every
        // covering frame is final: positions below t_fin * hop - and everything once the stream has ended
        const int t_fin = end ? S.t_done : S.t_done - LAG;
        const int o_hi = end ? n_final : std::min(S.n_total, t_fin * g.hop - g.n_fft / 2);
        if (o_hi > S.o_done) {
            if (rows && t_fin != t0 + n) launch_window_rows(rows->len, rw, MB, B, t_fin, st);      // (else the STFT's view holds)
            RaggedScope rs(view);
            launch_istft(g, est, B, t_fin, Tw, nullptr, S.per_frame() ? nullptr : S.c.get(), out_dev + *written, out_pitch, o_hi, st, t0 - HC,
                         std::max(0, t0 - HC), S.o_done, S.per_frame() ? S.frame_inv.get() : nullptr, S.ring);
            *written += o_hi - S.o_done;
            S.o_done = o_hi;
        }
    }
}

// what a frame-online stream and a windowed decode ask of the model's geometry, and how many frames one window launch takes
static void check_stream_geometry(const se_engine* e) {
    const StftGeom& g = e->ctx.geom;
    SE_CHECK((g.n_fft + g.hop - 1) / g.hop - 1 + e->model->stream_lag() <= e->model->stream_hc(),
             "front end overlap + look-ahead exceed the history the model keeps");
}
// (the workspace holds `room` frames behind the model's history columns; dflt: the chunk of a call that names none)
static int window_frames(const se_engine* e, int requested, int dflt) {
    const int room = std::max(1, e->plan_frames - e->model->stream_hc());
    return std::min(requested > 0 ? requested : dflt, room);
}

// the rings and sums of the per-frame scales: made once per handle, for the engine's plan (the running and the tracking scale share them)
static void scale_rings_alloc(se_engine* e, bool tracking) {
    se_engine::Stream& S = e->strm;
    if (!S.sumsq) {
        S.ring = 64;
        while (S.ring < e->plan_frames + 64) S.ring <<= 1;
        S.sumsq.alloc((size_t)2 * e->ctx.max_batch);      // (running: one sum per row; tracking: (E, W) per row)
        S.frame_inv.alloc((size_t)e->ctx.max_batch * S.ring);
    }
    if (tracking && !S.frame_c) S.frame_c.alloc((size_t)e->ctx.max_batch * S.ring);
}

static int stream_begin_impl(se_engine* e, int32_t batch, int32_t max_chunk_frames, const float* c_dev, bool running, void* stream,
                             bool tracking = false, float tau = 0.f) {
    if (!e) return 1;
    return guard(e, [&] {
        SE_CHECK(e->finalized, "engine not finalized");
        e->strm.carve_B = -1;          // (any decode re-carves the arena: a stream running on this handle zero-fills its next windows)
        if (tracking)
            SE_CHECK(std::isfinite(tau) && tau >= 0.f,
                     "se_stream_begin_tracking: tau_samples has to be a finite number >= 0 (0: never forget), got " + std::to_string(tau));
        // (FullSubNet is in the list of those that have one - with a cumulative norm and the LSTM: a refused FullSubNet is told which of
        // the two it lacks)
        SE_CHECK(e->model->stream_supported(),
                 std::string("this model has no frame-online mode (CRN, LSTM, GCRN, DPCRN, DCCRN, FullSubNet with a cumulative norm and "
                             "without the GRU, and the cLN `_new` weights of CTSNet / TaylorSENet / G2Net have)") +
                     (e->cfg.model == SE_MODEL_FULLSUBNET ? ": " + why_not_causal(e) : std::string()));
        SE_CHECK(batch >= 1 && batch <= e->ctx.max_batch, "batch exceeds max_batch given at create");
        check_stream_geometry(e);
        const StftGeom& g = e->ctx.geom;
        if (tracking)
            SE_CHECK(g.n_fft >= 2 * g.hop - 2, "se_stream_begin_tracking: n_fft " + std::to_string(g.n_fft) + " < 2 hop - 2 (hop " + std::to_string(g.hop) +
                                                   "): the stream's input window does not keep the head of an incomplete hop block");
        hipStream_t st = static_cast<hipStream_t>(stream);
        se_engine::Stream& S = e->strm;
        // work of the previous stream on another hipStream: wait for the event that stream_mark() recorded behind ITS last
        // call (the handle itself may have been destroyed since - it is never touched again)
        stream_order_wait(S, st);
        S.max_chunk = window_frames(e, max_chunk_frames, 16);
        if (!S.wav) {
            const bool sliding = (e->cfg.flags & SE_CFG_STREAM_SLIDING) != 0;
            S.pitch = sliding ? stream_window_pitch(e->ctx.max_samples, g.n_fft, g.hop) : e->ctx.max_samples;
            S.wav.alloc((size_t)e->ctx.max_batch * S.pitch);
            if (sliding) S.wav2.alloc((size_t)e->ctx.max_batch * S.pitch);
        }
        if (!S.c) S.c.alloc(e->ctx.max_batch);      // (se_enhance_long may have made it already)
        if (c_dev) SE_HIP(hipMemcpyAsync(S.c.get(), c_dev, (size_t)batch * sizeof(float), hipMemcpyDeviceToDevice, st));
        else launch_fill(S.c.get(), batch, 1.f, st);
        if (running || tracking) {
            scale_rings_alloc(e, tracking);
            SE_HIP(hipMemsetAsync(S.sumsq.get(), 0, (size_t)batch * (tracking ? 2 : 1) * sizeof(double), st));
            launch_fill(S.frame_inv.get(), (long)batch * S.ring, 1.f, st);
            if (tracking) launch_fill(S.frame_c.get(), (long)batch * S.ring, 1.f, st);
        }
        if (S.origin) SE_HIP(hipMemsetAsync(S.origin.get(), 0, (size_t)batch * sizeof(int32_t), st));
        S.start(batch, 0, running, tracking, tau, g.hop);
        e->model->stream_begin(batch, S.max_chunk, st);
        S.active = true;
        stream_mark(S, st);
    });
}

int se_stream_begin(se_engine* e, int32_t batch, int32_t max_chunk_frames, const float* c_dev, void* stream) {
    return stream_begin_impl(e, batch, max_chunk_frames, c_dev, false, stream);
}
int se_stream_begin_running(se_engine* e, int32_t batch, int32_t max_chunk_frames, void* stream) {
    return stream_begin_impl(e, batch, max_chunk_frames, nullptr, true, stream);
}

int se_stream_begin_tracking(se_engine* e, int32_t batch, int32_t max_chunk_frames, float tau_samples, void* stream) {
    return stream_begin_impl(e, batch, max_chunk_frames, nullptr, false, stream, true, tau_samples);
}

int se_stream_scale(se_engine* e, float* c_dev, void* stream) {
    if (!e) return 1;
    return guard(e, [&] {
        se_engine::Stream& S = e->strm;
        SE_CHECK(S.active, "se_stream_scale without se_stream_begin");
        SE_CHECK(c_dev, "se_stream_scale: null argument");
        hipStream_t st = static_cast<hipStream_t>(stream);
        stream_order_wait(S, st);
        SE_HIP(hipMemcpyAsync(c_dev, S.c.get(), (size_t)S.batch * sizeof(float), hipMemcpyDeviceToDevice, st));
        stream_mark(S, st);
    });
}

int se_stream_push(se_engine* e, const float* wav_dev, int64_t pitch, int32_t n_new, float* out_dev, int64_t out_pitch,
                   int32_t* n_out, void* stream) {
    if (!e) return 1;
    return guard(e, [&] {
        se_engine::Stream& S = e->strm;
        SE_CHECK(S.active, "se_stream_push without se_stream_begin");
        SE_CHECK(wav_dev && out_dev && n_out && n_new >= 0, "bad argument");
        SE_CHECK(S.batch == 1 || pitch >= n_new, "se_stream_push: input row pitch smaller than n_new");
        const StftGeom& g = e->ctx.geom;
        const bool sliding = (e->cfg.flags & SE_CFG_STREAM_SLIDING) != 0;
        int keep = S.w0;
        if (sliding) {
            SE_CHECK(n_new <= e->ctx.max_samples, "se_stream_push: a single push may carry at most max_samples samples");
            SE_CHECK((int64_t)S.n_total + n_new <= stream_sample_limit(e->ctx.max_samples, g.n_fft, g.hop),
                     "sliding stream longer than 2^31 - 1 - max_samples samples");
            // the new samples do not fit behind the live tail: drop what no later launch reads (stream_window.h)
            if ((long)(S.n_total - S.w0) + n_new > S.pitch) {
                keep = stream_keep_from(g.n_fft, g.hop, S.t_done, S.n_total);
                SE_CHECK(keep >= S.w0 && keep <= S.n_total && (long)(S.n_total - keep) + n_new <= S.pitch,
                         "se_stream_push: the stream window cannot hold this push behind the samples still to be transformed");
            }
        } else {
            SE_CHECK(S.n_total + n_new <= e->ctx.max_samples, "stream longer than max_samples given at create");
        }
        hipStream_t st = static_cast<hipStream_t>(stream);
        ArenaCall call(e, st, ArenaCall::MARK_ONLY);
        if (keep != S.w0) {
            // [keep, n_total) of every row to column 0 of the other buffer (whole float4s: up to three columns past the tail
            // travel along, inside the row - the append below overwrites them)
            launch_stream_slide(S.wav.get(), S.wav2.get(), S.pitch, S.batch, keep - S.w0, (S.n_total - keep + 3) & ~3, st);
            std::swap(S.wav, S.wav2);
            S.w0 = keep;
        }
        if (n_new > 0)
            SE_HIP(hipMemcpy2DAsync(S.wav.get() + (S.n_total - S.w0), (size_t)S.pitch * sizeof(float), wav_dev,
                                    (size_t)pitch * sizeof(float), (size_t)n_new * sizeof(float), S.batch,
                                    hipMemcpyDeviceToDevice, st));
        S.n_total += n_new;
        // frame t is final once sample t * hop + n_fft / 2 has arrived (its right half is real signal, and frame 0's reflected
        // left half needs sample n_fft / 2 as well)
        const int t_avail = S.n_total > g.n_fft / 2 ? (S.n_total - g.n_fft / 2 - 1) / g.hop + 1 : 0;
        if (S.tracking)     // c_t of the frames this push releases, from the hop blocks it completes
            launch_stream_track(g, S.wav.get(), S.pitch, S.batch, S.n_total, n_new, false, S.lam, S.sumsq.get(), S.c.get(), S.frame_c.get(),
                                S.frame_inv.get(), S.ring, S.t_done, std::max(t_avail, S.t_done), st, S.w0);
        else if (S.running)      // c of the frames this push releases: sqrt(samples so far / their sum of squares)
            launch_stream_rms(S.wav.get(), S.pitch, S.batch, S.n_total, n_new, S.sumsq.get(), S.c.get(), S.frame_inv.get(), S.ring, S.t_done,
                              std::max(t_avail, S.t_done), st, S.w0);
        int written = 0;
        const int will = std::max(0, std::min(S.n_total, (t_avail - e->model->stream_lag()) * g.hop - g.n_fft / 2) - S.o_done);
        SE_CHECK(out_pitch >= will, "output row pitch too small for the samples this push completes");
        e->ctx.prof_reset();
        stream_process(e, std::max(t_avail, S.t_done), false, out_dev, out_pitch, &written, st);
        *n_out = written;
    });
}

int se_stream_flush(se_engine* e, float* out_dev, int64_t out_pitch, int32_t* n_out, void* stream) {
    if (!e) return 1;
    return guard(e, [&] {
        se_engine::Stream& S = e->strm;
        SE_CHECK(S.active, "se_stream_flush without se_stream_begin");
        SE_CHECK(out_dev && n_out, "bad argument");
        SE_CHECK(S.n_total >= e->ctx.geom.n_fft, "stream shorter than one FFT frame");
        SE_CHECK(out_pitch >= e->model->output_samples(S.n_total) - S.o_done, "output row pitch too small for the rest of the stream");
        int written = 0;
        hipStream_t st = static_cast<hipStream_t>(stream);
        ArenaCall call(e, st, ArenaCall::MARK_ONLY);
        e->ctx.prof_reset();
        if (S.tracking)
            launch_stream_track(e->ctx.geom, S.wav.get(), S.pitch, S.batch, S.n_total, 0, true, S.lam, S.sumsq.get(), S.c.get(), S.frame_c.get(),
                                S.frame_inv.get(), S.ring, S.t_done, e->model->num_frames(S.n_total), st, S.w0);
        else if (S.running)
            launch_stream_rms(S.wav.get(), S.pitch, S.batch, S.n_total, 0, S.sumsq.get(), S.c.get(), S.frame_inv.get(), S.ring, S.t_done,
                              e->model->num_frames(S.n_total), st, S.w0);
        stream_process(e, e->model->num_frames(S.n_total), true, out_dev, out_pitch, &written, st);
        *n_out = written;
        S.active = false;
    });
}

// why a model that has no frame-online mode has none: the windowed decode of se_enhance_long is the same walk
static std::string why_not_causal(const se_engine* e) {
    switch (e->cfg.model) {
        case SE_MODEL_UFORMER:
            return "Uformer attends over every frame of the utterance and its dilated convolutions look ahead in time";
        case SE_MODEL_FULLSUBNET:
            if (e->cfg.flags & SE_CFG_FSN_GRU) return "the GRU FullSubNet (SE_CFG_FSN_GRU) has no frame-online mode";
            if (e->cfg.flags & SE_CFG_FSN_GAUSSIAN)
                return "FullSubNet with offline_gaussian_norm (SE_CFG_FSN_GAUSSIAN) subtracts a mean and divides by a standard deviation over "
                       "the whole utterance (cumulative_layer_norm, SE_CFG_FSN_CUM_LAYERNORM, standardises by the frames so far and streams)";
            return "FullSubNet with offline_laplace_norm divides every frame by a mean over the whole utterance "
                   "(cumulative_laplace_norm, SE_CFG_FSN_CUMULATIVE, does not)";
        case SE_MODEL_CTSNET:
        case SE_MODEL_G2NET:
        case SE_MODEL_TAYLORSENET:
            return "the model was loaded with InstanceNorm weights, whose statistics span the whole utterance (the "
                   "cumulative-LayerNorm weights of the `_new` directories do not)";
        default: return "the model has no frame-online mode";
    }
}

// The windowed decode of whole clips behind se_enhance_long (lengths null: every row holds n_samples) and se_enhance_long_ragged
// (rows of their own lengths): the rows' unit-RMS scales over their whole clips first, then the stream's begin step and one walk
// over every frame of the longest row, the last window included (right-edge reflection, hop-multiple tail pad); the STFT reads the
// caller's rows, nothing is copied.  `fn` names the entry point in the refusals
static void enhance_long_impl(se_engine* e, const std::string& fn, const float* wav_in_dev, int64_t in_pitch, int32_t batch,
                              int32_t n_samples, const int32_t* lengths /* null: equal rows */, int32_t max_chunk_frames,
                              float* wav_out_dev, int64_t out_pitch, hipStream_t st) {
    SE_CHECK(e->model->stream_supported(),
             fn + " decodes in windows, which needs a network that is causal end to end: " + why_not_causal(e));
    SE_CHECK(!(lengths && e->cfg.model == SE_MODEL_DCCRN && e->model->stream_lag() > 0 && !(e->cfg.flags & SE_CFG_DCCRN_ROW_ENDS)),
             fn + ": DCCRN's look-ahead decoder reads one frame ahead per layer into tensors that are not zero "
                  "behind a row's own last frame; the per-layer zeroing that rows of different lengths need is not built yet: decode "
                  "them one at a time with se_enhance_long (the causal decoder, SE_CFG_DCCRN_CAUSAL_DEC, is accepted, and so is an "
                  "engine created with SE_CFG_DCCRN_ROW_ENDS)");
    SE_CHECK(batch >= 1 && batch <= e->ctx.max_batch, "batch exceeds max_batch given at create");
    const StftGeom& g = e->ctx.geom;
    int Lmax = 0;
    for (int b = 0; b < (lengths ? batch : 1); ++b) {
        const int n = lengths ? lengths[b] : n_samples;
        const std::string what = fn + (lengths ? ": lengths[" + std::to_string(b) + "]" : ": n_samples");
        SE_CHECK(n >= g.n_fft, what + " shorter than one FFT frame (n_fft)");
        // no push follows, so the headroom of the position counters is the kernels' own reach (stream_window.h), whatever max_samples
        SE_CHECK(n <= stream_sample_limit(0, g.n_fft, g.hop), what + " above the position bound 2^31 - 1 - n_fft - 32 hop");
        Lmax = std::max(Lmax, n);
    }
    SE_CHECK(batch == 1 || in_pitch >= Lmax, fn + ": input row pitch smaller than " + (lengths ? "the longest row" : "n_samples"));
    SE_CHECK(out_pitch >= e->model->output_samples(Lmax),
             fn + ": output row pitch smaller than se_output_samples(" + (lengths ? "longest row" : "n_samples") + ")");
    SE_CHECK(max_chunk_frames >= 0, fn + ": negative max_chunk_frames");
    check_stream_geometry(e);
    // every refusal is above: a refused call leaves a stream running on this handle as it was.  From here the call takes over
    // the stream state, so that stream ends
    ArenaCall call(e, st, ArenaCall::TAKE_OVER);
    se_engine::Stream& S = e->strm;
    S.max_chunk = window_frames(e, max_chunk_frames, INT_MAX);
    if (!S.c) S.c.alloc(e->ctx.max_batch);
    e->ctx.prof_reset();
    // rows of their own lengths: the sizes go up once, for the scales here and for every window of the walk
    const Ragged rg = lengths ? upload_row_sizes(e, batch, lengths, st) : Ragged{};
    const Ragged* rows = lengths ? &rg : nullptr;
    {
        RaggedScope rs(rows);
        launch_rms_scale(wav_in_dev, batch, Lmax, in_pitch, S.c.get(), st);
    }
    if (S.origin) SE_HIP(hipMemsetAsync(S.origin.get(), 0, (size_t)batch * sizeof(int32_t), st));      // (a windowed decode begins at frame 0 in every row)
    S.start(batch, Lmax, false);
    S.ext = wav_in_dev;
    S.ext_pitch = in_pitch;
    e->model->stream_begin(batch, S.max_chunk, st);
    int written = 0;
    stream_process(e, e->model->num_frames(Lmax), true, wav_out_dev, out_pitch, &written, st, rows);
    S.carve_B = -1;
}

int se_enhance_long(se_engine* e, const float* wav_in_dev, int64_t in_pitch, int32_t batch, int32_t n_samples,
                    int32_t max_chunk_frames, float* wav_out_dev, int64_t out_pitch, void* stream) {
    if (!e) return 1;
    return guard(e, [&] {
        SE_CHECK(e->finalized, "engine not finalized");
        SE_CHECK(wav_in_dev && wav_out_dev, "null argument");
        enhance_long_impl(e, "se_enhance_long", wav_in_dev, in_pitch, batch, n_samples, nullptr, max_chunk_frames, wav_out_dev,
                          out_pitch, static_cast<hipStream_t>(stream));
    });
}

int se_enhance_long_ragged(se_engine* e, const float* wav_in_dev, int64_t in_pitch, int32_t batch, const int32_t* lengths,
                           int32_t max_chunk_frames, float* wav_out_dev, int64_t out_pitch, void* stream) {
    if (!e) return 1;
    return guard(e, [&] {
        SE_CHECK(e->finalized, "engine not finalized");
        SE_CHECK(wav_in_dev && wav_out_dev && lengths, "null argument");
        enhance_long_impl(e, "se_enhance_long_ragged", wav_in_dev, in_pitch, batch, 0, lengths, max_chunk_frames, wav_out_dev,
                          out_pitch, static_cast<hipStream_t>(stream));
    });
}

int64_t se_output_samples(const se_engine* e, int32_t n_samples) { return e ? e->model->output_samples(n_samples) : -1; }
int32_t se_num_frames(const se_engine* e, int32_t n_samples) { return e ? e->model->num_frames(n_samples) : -1; }
int32_t se_num_bins(const se_engine* e) { return e ? e->ctx.geom.F() : -1; }

int se_rms_scale(se_engine* e, const float* wav_dev, int64_t pitch, int32_t batch, int32_t n_samples, float* c_dev,
                 void* stream) {
    if (!e) return 1;
    return guard(e, [&] { launch_rms_scale(wav_dev, batch, n_samples, pitch, c_dev, static_cast<hipStream_t>(stream)); });
}

int se_stft(se_engine* e, const float* wav_dev, int64_t pitch, int32_t batch, int32_t n_samples, const float* c_dev,
            float p_in, float* spec_dev, void* stream) {
    if (!e) return 1;
    return guard(e, [&] {
        const int Lpad = e->model->padded_samples(n_samples);
        const int T = 1 + Lpad / e->ctx.geom.hop;
        launch_stft(e->ctx.geom, wav_dev, pitch, batch, n_samples, Lpad, c_dev, p_in, spec_dev, nullptr, T, T,
                    static_cast<hipStream_t>(stream));
    });
}

int se_istft(se_engine* e, const float* spec_dev, int32_t batch, int32_t n_frames, const float* c_dev, float* wav_dev,
             int64_t pitch, int32_t n_out, void* stream) {
    if (!e) return 1;
    return guard(e, [&] {
        launch_istft(e->ctx.geom, spec_dev, batch, n_frames, n_frames, nullptr, c_dev, wav_dev, pitch, n_out,
                     static_cast<hipStream_t>(stream));
    });
}

int se_frontend(se_engine* e, const float* wav_dev, int64_t pitch, int32_t batch, int32_t n_samples, float* c_dev,
                float* spec_dev, void* stream) {
    if (!e) return 1;
    return guard(e, [&] {
        SE_CHECK(wav_dev && c_dev && spec_dev, "null argument");
        SE_CHECK(batch >= 1 && n_samples >= e->ctx.geom.n_fft && pitch >= n_samples, "se_frontend: bad shape");
        hipStream_t st = static_cast<hipStream_t>(stream);
        launch_rms_scale(wav_dev, batch, n_samples, pitch, c_dev, st);
        const int Lpad = e->model->padded_samples(n_samples);
        const int T = 1 + Lpad / e->ctx.geom.hop;
        launch_stft(e->ctx.geom, wav_dev, pitch, batch, n_samples, Lpad, c_dev, e->ctx.p_in, spec_dev, nullptr, T, T, st);
    });
}

int se_backend(se_engine* e, int32_t kind, const float* est_dev, const float* spec_dev, int32_t batch, int32_t n_frames,
               const float* c_dev, float* wav_dev, int64_t pitch, int32_t n_out, void* stream) {
    if (!e) return 1;
    return guard(e, [&] {
        SE_CHECK(est_dev && wav_dev, "null argument");
        SE_CHECK(kind == SE_BACKEND_RI || kind == SE_BACKEND_MAG || kind == SE_BACKEND_CMASK, "se_backend: unknown kind");
        SE_CHECK(kind == SE_BACKEND_RI || spec_dev, "se_backend: this kind needs the front end's spectrum");
        SE_CHECK(batch >= 1 && n_frames >= 1 && n_out >= 1 && pitch >= n_out, "se_backend: bad shape");
        hipStream_t st = static_cast<hipStream_t>(stream);
        const int F = e->ctx.geom.F();
        const size_t need = (size_t)batch * 2 * F * n_frames * sizeof(float);
        if (need > e->hook_cap) {
            SE_HIP(hipStreamSynchronize(st));       // (an earlier call on this stream may still read the old buffer)
            e->hook_cap = 0;
            e->hook_buf.alloc(need / sizeof(float));
            e->hook_cap = need;
        }
        if (kind == SE_BACKEND_RI) launch_polar_pow(est_dev, e->hook_buf.get(), batch, F, n_frames, e->ctx.p_out, st);
        else if (kind == SE_BACKEND_MAG) launch_mag_phase(est_dev, spec_dev, e->hook_buf.get(), batch, F, n_frames, e->ctx.p_out, st);
        else launch_cmask_apply(est_dev, spec_dev, e->hook_buf.get(), batch, F, n_frames, e->ctx.p_out, st);
        launch_istft(e->ctx.geom, e->hook_buf.get(), batch, n_frames, n_frames, nullptr, c_dev, wav_dev, pitch, n_out, st);
    });
}

int se_set_profiling(se_engine* e, int32_t on) {
    if (!e) return 1;
    e->ctx.prof_set(on != 0);
    return 0;
}

int se_get_profile(se_engine* e, double* gemm_ms, int64_t* gemm_launches, double* gemm_flops) {
    if (!e) return 1;
    return guard(e, [&] {
        // launches on the auxiliary streams (FullSubNet's sub-band halves) run concurrently with the main stream's: the sum
        // of their durations is kernel time, not wall time
        double ms = e->ctx.prof.total_ms(), fl = e->ctx.prof.flops;
        int64_t n = e->ctx.prof.launches;
        for (auto& p : e->ctx.aux_prof) {
            ms += p.total_ms();
            fl += p.flops;
            n += p.launches;
        }
        if (gemm_ms) *gemm_ms = ms;
        if (gemm_launches) *gemm_launches = n;
        if (gemm_flops) *gemm_flops = fl;
    });
}

int se_get_stage_profile(se_engine* e, int32_t stage, double* ms, int64_t* launches, double* bytes) {
    if (!e) return 1;
    return guard(e, [&] {
        SE_CHECK(stage >= 0 && stage < STAGE_COUNT, "stage id out of range");
        if (ms) *ms = e->ctx.stage_prof.ms(stage);
        if (launches) *launches = e->ctx.stage_prof.slot[stage].launches;
        if (bytes) *bytes = e->ctx.stage_prof.slot[stage].bytes;
    });
}

// ---- se_stream_save / se_stream_restore: a running stream parked in an object of its own and put back -----------------------
// The object: the manifest (stream_manifest.h, host) + one device payload, every carried buffer at a 16 B aligned offset, the input
// window last.  The payload is sized when a layout is first seen - its window part for the most a stream keeps live between two
// calls - so saving again into the same object allocates nothing.  The two device tables (engine -> payload, payload -> engine) of
// the copy kernel (k_stream_state.hip) are rebuilt on the host at every call, which is a few hundred assignments, and uploaded only
// when they differ from the last upload: through a pinned buffer, so that the call waits for nothing either.
}  // extern "C"

struct se_stream_state {
    SnapManifest man;
    bool filled = false;
    int device = -1;                      // the device the payload, the tables and the event live on
    bool dev_valid = false;               // dev holds the payload of `man` (false after an import, until the first restore)
    std::vector<SnapSeg> dev_layout;      // the segments in front of the window `dev` was laid out for
    int64_t dev_fixed = 0, dev_win_cap = 0;
    std::vector<uint8_t> host;            // payload of an imported image (kept: another device may restore it too)
    struct Table {
        DevBuf<StateSeg> dev;
        PinnedBuf<StateSeg> pin;
        size_t cap = 0;
        std::vector<StateSeg> last;
        Event ev;                         // behind the last upload: the pinned buffer is free again
    };
    struct Side {                         // what belongs to one device (an imported image may be restored on several, one after the other)
        DevBuf<uint8_t> dev;
        Table tab[2];                     // 0: save, 1: restore
        Event ev_use;
        // se_stream_state_select / _concat into this object: the gather kernel's tables (segments, source offsets, part bases, row
        // map) in one block, through a pinned copy of it
        DevBuf<uint8_t> gat_dev;
        PinnedBuf<uint8_t> gat_pin;
        size_t gat_cap = 0;
        Event gat_ev;                     // behind the last upload: the pinned block is free again
    };
    std::unique_ptr<Side> side{new Side()};
    // the hipStream the object was last used on: a call on another one is ordered behind it
    bool has_use = false;
    hipStream_t use_st = nullptr;
};

namespace {

struct DeviceScope {      // a call on the object alone: its device is current while the call runs
    int prev = -1;
    explicit DeviceScope(int dev) {
        if (dev < 0) return;
        int cur = -1;
        SE_HIP(hipGetDevice(&cur));
        if (cur != dev) {
            SE_HIP(hipSetDevice(dev));
            prev = cur;
        }
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

struct EngSeg {
    SnapSeg seg;
    void* ptr;
};

// every buffer chunk k of the stream writes and chunk k + 1 reads, except the input window, in payload order
// (mode: SnapManifest::running - 0 a fixed scale, 1 the running scale, 2 the tracking scale)
std::vector<EngSeg> engine_segments(se_engine* e, int batch, int mode, int ring) {
    se_engine::Stream& S = e->strm;
    std::vector<EngSeg> v;
    auto add = [&](int32_t kind, int32_t index, void* p, int64_t bytes) {
        EngSeg s;
        s.seg.kind = kind;
        s.seg.index = index;
        s.seg.bytes = bytes;
        s.ptr = p;
        v.push_back(s);
    };
    add(SNAP_C, 0, S.c.get(), (int64_t)batch * sizeof(float));
    if (mode) {
        add(SNAP_SUMSQ, 0, S.sumsq.get(), (int64_t)batch * (mode == 2 ? 2 : 1) * sizeof(double));
        add(SNAP_FRAME_INV, 0, S.frame_inv.get(), (int64_t)batch * ring * sizeof(float));
        if (mode == 2) add(SNAP_FRAME_INV, 1, S.frame_c.get(), (int64_t)batch * ring * sizeof(float));
    }
    if (StreamState* ss = e->model->stream_state()) {
        for (size_t i = 0; i < ss->hist.size(); ++i) add(SNAP_HIST, (int32_t)i, ss->hist[i], (int64_t)ss->size_of.at(ss->hist[i]) * sizeof(float));
        for (int l = 0; l < 4; ++l) {
            if (ss->h[l]) add(SNAP_H, l, ss->h[l], (int64_t)ss->size_of.at(ss->h[l]) * sizeof(float));
            if (ss->c[l]) add(SNAP_CELL, l, ss->c[l], (int64_t)ss->size_of.at(ss->c[l]) * sizeof(float));
        }
    }
    if (StreamSlots* sl = e->model->stream_slots())
        for (size_t i = 0; i < sl->v.size(); ++i) add(SNAP_SLOT, (int32_t)i, sl->v[i].first, (int64_t)sl->v[i].second);
    if (S.origin) add(SNAP_ORIGIN, 0, S.origin.get(), (int64_t)batch * sizeof(int32_t));      // (right in front of the window: snap_origin_why)
    return v;
}

bool same_segs(const std::vector<EngSeg>& a, const std::vector<SnapSeg>& b, size_t nb) {
    if (a.size() != nb) return false;
    for (size_t i = 0; i < nb; ++i)
        if (a[i].seg.kind != b[i].kind || a[i].seg.index != b[i].index || a[i].seg.bytes != b[i].bytes) return false;
    return true;
}
bool same_layout(const std::vector<SnapSeg>& a, const std::vector<SnapSeg>& b, size_t nb) {
    if (a.size() != nb) return false;
    for (size_t i = 0; i < nb; ++i)
        if (a[i].kind != b[i].kind || a[i].index != b[i].index || a[i].bytes != b[i].bytes) return false;
    return true;
}

// the most input samples a stream keeps live between two calls: every frame whose samples have all arrived is transformed before
// a push returns, so what a later frame or the flush's reflection still reads is less than a window and a hop (stream_window.h)
int snap_window_cap(const StftGeom& g) { return (g.n_fft + g.hop + 3 + 3) & ~3; }

int64_t fixed_bytes_of(const SnapManifest& m) {
    int64_t n = 0;
    for (const SnapSeg& s : m.segs)
        if (s.kind != SNAP_WINDOW) n += snap_align16(s.bytes);
    return n;
}
size_t fixed_count_of(const SnapManifest& m) {
    return m.segs.empty() || m.segs.back().kind != SNAP_WINDOW ? m.segs.size() : m.segs.size() - 1;
}

void obj_wait(se_stream_state* s, hipStream_t st) {
    if (s->has_use && s->use_st != st) SE_HIP(hipStreamWaitEvent(st, s->side->ev_use.get(), 0));
}
void obj_mark(se_stream_state* s, hipStream_t st) {
    SE_HIP(hipEventRecord(s->side->ev_use.get(), st));
    s->has_use = true;
    s->use_st = st;
}

// a payload buffer on the current device for the layout of m (window part: at least win_cap bytes); the old contents are dropped
void payload_alloc(se_stream_state* s, const SnapManifest& m, int64_t win_cap, int device) {
    const size_t nfix = fixed_count_of(m);
    const int64_t fixed = fixed_bytes_of(m);
    if (s->side->dev && s->device == device && same_layout(s->dev_layout, m.segs, nfix) && s->dev_win_cap >= win_cap) return;
    if (s->side->dev && s->device != device) {          // (payload, tables and event of another device go with that device current)
        DeviceScope ds(s->device);
        s->side.reset();
        s->has_use = false;
    }
    if (!s->side) s->side.reset(new se_stream_state::Side());
    DevBuf<uint8_t> fresh;
    fresh.alloc((size_t)(fixed + win_cap + 16));
    s->side->dev = std::move(fresh);
    s->device = device;
    s->dev_layout.assign(m.segs.begin(), m.segs.begin() + (long)nfix);
    s->dev_fixed = fixed;
    s->dev_win_cap = win_cap;
    s->dev_valid = false;
}

// engine-side segments against payload offsets -> the device table of direction dir (0: engine -> payload); uploaded when it changed
const StateSeg* table_for(se_stream_state* s, int dir, const std::vector<EngSeg>& eng, float* wav, int batch, long* fix_tiles,
                          hipStream_t st) {
    std::vector<StateSeg> v(eng.size() + 1);
    long tiles = 0;
    int64_t off = 0;
    for (size_t i = 0; i <= eng.size(); ++i) {
        StateSeg sg{};
        float* pay = reinterpret_cast<float*>(s->side->dev.get() + (i < eng.size() ? off : s->dev_fixed));
        float* own = i < eng.size() ? static_cast<float*>(eng[i].ptr) : wav;
        sg.src = dir == 0 ? own : pay;
        sg.dst = dir == 0 ? pay : own;
        if (i < eng.size()) {
            SE_CHECK(eng[i].seg.bytes / 4 < INT_MAX, "stream state: segment too large");
            sg.rows = 1;
            sg.len = (int)(eng[i].seg.bytes / 4);
            sg.tile0 = (int)tiles;
            tiles += state_seg_tiles(1, sg.len);
            SE_CHECK(tiles < INT_MAX, "stream state: too many tiles");
            off += snap_align16(eng[i].seg.bytes);
        } else {
            sg.rows = batch;          // the window: extent from the call
            sg.tile0 = (int)tiles;
        }
        v[i] = sg;
    }
    *fix_tiles = tiles;
    auto& T = s->side->tab[dir];
    if (T.dev && T.last.size() == v.size() && std::memcmp(T.last.data(), v.data(), v.size() * sizeof(StateSeg)) == 0) return T.dev.get();
    SE_HIP(hipEventSynchronize(T.ev.get()));
    if (v.size() > T.cap) {
        // (room for the slots a stream of the cLN networks creates on its first chunk: the table of a group that has not produced a
        // frame yet is a handful of rows, the next one well over a hundred)
        const size_t cap = std::max<size_t>(v.size() + 64, 512);
        T.last.clear();
        T.dev.alloc(cap);
        T.pin.alloc(cap);
        T.cap = cap;
    }
    std::memcpy(T.pin.get(), v.data(), v.size() * sizeof(StateSeg));
    SE_HIP(hipMemcpyAsync(T.dev.get(), T.pin.get(), v.size() * sizeof(StateSeg), hipMemcpyHostToDevice, st));
    SE_HIP(hipEventRecord(T.ev.get(), st));
    T.last = v;
    return T.dev.get();
}

std::string hex(int v) {
    char b[16];
    snprintf(b, sizeof b, "0x%x", (unsigned)v);
    return b;
}

// the payload of s is on e's device, or s holds an imported image that can be put there
void check_payload_reachable(const se_engine* e, const se_stream_state* s, const std::string& fn) {
    if (!s->dev_valid || s->device != e->cfg.device)
        SE_CHECK(!s->host.empty(), fn + "the payload lives on device " + std::to_string(s->device) + ", this engine on device " +
                                       std::to_string(e->cfg.device) + " (export the state and import it to move it)");
}
// ... and puts it there (e's device is current): once, until the object is saved into again
void payload_to_device(const se_engine* e, se_stream_state* s, const std::string& fn) {
    if (s->dev_valid && s->device == e->cfg.device) return;
    const SnapManifest& m = s->man;
    if (s->has_use) {
        DeviceScope ds(s->device);
        SE_HIP(hipEventSynchronize(s->side->ev_use.get()));
        s->has_use = false;
    }
    const int64_t win = m.segs.empty() ? 0 : snap_align16(m.segs.back().bytes);
    payload_alloc(s, m, std::max<int64_t>(win, (int64_t)m.batch * snap_window_cap(e->ctx.geom) * sizeof(float)), e->cfg.device);
    SE_CHECK((int64_t)s->host.size() == snap_payload_bytes(m), fn + "host image of the wrong size");
    SE_HIP(hipMemcpy(s->side->dev.get(), s->host.data(), s->host.size(), hipMemcpyHostToDevice));
    s->dev_valid = true;
}

// a snapshot is of this engine's kind: model, flags, front end, exponents (what se_stream_restore and the row operations compare)
void check_snapshot_identity(const se_engine* e, const SnapManifest& m, const std::string& fn) {
    const StftGeom& g = e->ctx.geom;
    SE_CHECK(m.model == e->cfg.model, fn + "the snapshot was taken on model id " + std::to_string(m.model) + ", this engine runs model id " +
                                          std::to_string(e->cfg.model));
    const int free_bits = SE_CFG_GRAPHS | SE_CFG_STREAM_SLIDING;
    SE_CHECK(((m.flags ^ e->cfg.flags) & ~free_bits) == 0,
             fn + "se_config.flags differ (snapshot " + hex(m.flags) + ", engine " + hex(e->cfg.flags) +
                 "; every bit except SE_CFG_GRAPHS and SE_CFG_STREAM_SLIDING has to match)");
    SE_CHECK(m.n_fft == g.n_fft && m.hop == g.hop && m.win == g.win,
             fn + "front end differs (snapshot n_fft / hop / win " + std::to_string(m.n_fft) + " / " + std::to_string(m.hop) + " / " +
                 std::to_string(m.win) + ", engine " + std::to_string(g.n_fft) + " / " + std::to_string(g.hop) + " / " + std::to_string(g.win) + ")");
    SE_CHECK(m.p_in == e->ctx.p_in && m.p_out == e->ctx.p_out, fn + "magnitude exponents p_in / p_out differ");
    const std::string org = snap_origin_why(m);
    SE_CHECK(org.empty(), fn + org);
    SE_CHECK(e->model->stream_supported(), fn + "this engine's model has no frame-online mode");
}

}  // namespace

extern "C" {

int se_stream_state_create(se_stream_state** out) {
    return guard(nullptr, [&] {
        SE_CHECK(out, "se_stream_state_create: null argument");
        *out = new se_stream_state();
    });
}

int se_stream_state_destroy(se_stream_state* s) {
    if (!s) return 0;
    return guard(nullptr, [&] {
        std::unique_ptr<se_stream_state> own(s);
        if (s->device >= 0) {
            DeviceScope ds(s->device);
            if (s->has_use) (void)hipEventSynchronize(s->side->ev_use.get());
            own.reset();
        }
    });
}

int64_t se_stream_state_bytes(const se_stream_state* s) {
    if (!s || !s->filled) return 0;
    return s->side->dev ? s->dev_fixed + s->dev_win_cap : snap_payload_bytes(s->man);
}

int se_stream_save(se_engine* e, se_stream_state* s, void* stream) {
    if (!e) return 1;
    return guard(e, [&] {
        SE_CHECK(s, "se_stream_save: null argument");
        se_engine::Stream& S = e->strm;
        SE_CHECK(S.active, "se_stream_save without se_stream_begin");
        hipStream_t st = static_cast<hipStream_t>(stream);
        const StftGeom& g = e->ctx.geom;
        SnapManifest m;
        m.model = e->cfg.model;
        m.flags = e->cfg.flags;
        m.n_fft = g.n_fft;
        m.hop = g.hop;
        m.win = g.win;
        m.p_in = e->ctx.p_in;
        m.p_out = e->ctx.p_out;
        m.batch = S.batch;
        m.max_chunk = S.max_chunk;
        m.n_total = S.n_total;
        m.t_done = S.t_done;
        m.o_done = S.o_done;
        // only what a later launch can still read (stream_window.h): rows stored back to back, not at this engine's pitch
        m.keep = std::max(S.w0, stream_keep_from(g.n_fft, g.hop, S.t_done, S.n_total));
        m.running = S.scale_mode();
        m.ring = S.per_frame() ? S.ring : 0;
        if (S.tracking) std::memcpy(&m.reserved[0], &S.tau, sizeof(float));
        const StreamState* ss = e->model->stream_state();
        const StreamSlots* sl = e->model->stream_slots();
        m.first = ss ? (ss->first ? 1 : 0) : 1;
        m.state_B = ss ? ss->B : sl ? sl->B : 0;
        const int live = m.n_total - m.keep;
        const int wcap = snap_window_cap(g);
        SE_CHECK(live >= 0 && live <= wcap, "se_stream_save: " + std::to_string(live) + " live input samples, more than a window and a hop");
        const std::vector<EngSeg> eng = engine_segments(e, S.batch, S.scale_mode(), S.ring);
        for (const EngSeg& sg : eng) {
            SE_CHECK(sg.ptr && sg.seg.bytes >= 0 && (sg.seg.bytes & 3) == 0, "se_stream_save: a carried buffer is missing or of an odd size");
            m.segs.push_back(sg.seg);
        }
        SnapSeg wseg;
        wseg.kind = SNAP_WINDOW;
        wseg.bytes = (int64_t)S.batch * live * sizeof(float);
        m.segs.push_back(wseg);
        // nothing of the object or the stream has changed up to here
        payload_alloc(s, m, (int64_t)S.batch * wcap * sizeof(float), e->cfg.device);
        stream_order_wait(S, st);
        obj_wait(s, st);
        long fix_tiles = 0;
        const StateSeg* tab = table_for(s, 0, eng, S.wav.get(), S.batch, &fix_tiles, st);
        StateWindow w;
        w.src_off = m.keep - S.w0;
        w.src_pitch = S.pitch;
        w.dst_pitch = live;
        w.rows = S.batch;
        w.len = live;
        launch_stream_state_copy(tab, (int)eng.size(), fix_tiles, (int)eng.size(), w, st);
        s->man = std::move(m);
        s->filled = true;
        s->dev_valid = true;
        s->host.clear();
        s->host.shrink_to_fit();
        stream_mark(S, st);
        obj_mark(s, st);
    });
}

int se_stream_restore(se_engine* e, const se_stream_state* cs, void* stream) {
    if (!e) return 1;
    return guard(e, [&] {
        se_stream_state* s = const_cast<se_stream_state*>(cs);      // (the tables and the uploaded payload are caches of the object)
        SE_CHECK(s, "se_stream_restore: null argument");
        SE_CHECK(e->finalized, "engine not finalized");
        SE_CHECK(s->filled, "se_stream_restore: the stream state object is empty");
        const SnapManifest& m = s->man;
        const StftGeom& g = e->ctx.geom;
        const std::string fn = "se_stream_restore: ";
        check_snapshot_identity(e, m, fn);
        SE_CHECK(m.batch <= e->ctx.max_batch, fn + "snapshot of " + std::to_string(m.batch) + " rows exceeds max_batch " +
                                                  std::to_string(e->ctx.max_batch) + " given at create");
        check_stream_geometry(e);
        SE_CHECK(window_frames(e, m.max_chunk, 16) == m.max_chunk,
                 fn + "the workspace is not planned for the snapshot's max_chunk_frames (" + std::to_string(m.max_chunk) + ")");
        const bool sliding = (e->cfg.flags & SE_CFG_STREAM_SLIDING) != 0;
        const int live = m.n_total - m.keep;
        const long pitch = sliding ? stream_window_pitch(e->ctx.max_samples, g.n_fft, g.hop) : e->ctx.max_samples;
        if (sliding) SE_CHECK(live <= pitch, fn + "the stream window of this engine cannot hold the " + std::to_string(live) + " live samples of the snapshot");
        else
            SE_CHECK(m.n_total <= e->ctx.max_samples, fn + "the stream has received " + std::to_string(m.n_total) +
                                                          " samples, more than max_samples given at create (and the engine has no SE_CFG_STREAM_SLIDING)");
        SE_CHECK(live <= snap_window_cap(g), fn + "more live input samples than a window and a hop");
        se_engine::Stream& S = e->strm;
        int ring = 0;
        SE_CHECK(m.running >= 0 && m.running <= 2, fn + "unknown scale mode " + std::to_string(m.running) + " in the snapshot");
        float tau = 0.f;
        if (m.running == 2) {
            std::memcpy(&tau, &m.reserved[0], sizeof(float));
            SE_CHECK(std::isfinite(tau) && tau >= 0.f, fn + "the snapshot of a tracking-scale stream records a tau_samples that is not a finite number >= 0");
            SE_CHECK(g.n_fft >= 2 * g.hop - 2, fn + "n_fft < 2 hop - 2: this front end cannot run a tracking scale");
        }
        if (m.running) {
            int need = S.sumsq ? S.ring : 64;
            if (!S.sumsq)
                while (need < e->plan_frames + 64) need <<= 1;
            SE_CHECK(m.ring >= need && (m.ring & (m.ring - 1)) == 0,
                     fn + "the snapshot of a " + (m.running == 2 ? "tracking" : "running") + "-scale stream keeps 1 / c of " + std::to_string(m.ring) + " frames per row, this engine needs " +
                         std::to_string(need) + " (planned for a larger max_samples)");
            ring = m.ring;
        }
        const size_t nfix = fixed_count_of(m);
        SE_CHECK(nfix + 1 == m.segs.size(), fn + "snapshot without an input window segment");
        const bool has_ss = e->model->stream_state() != nullptr;
        std::vector<std::pair<void*, size_t>> want_slots;
        for (size_t i = 0; i < nfix; ++i) {
            const SnapSeg& sg = m.segs[i];
            const bool rec = sg.kind == SNAP_HIST || sg.kind == SNAP_H || sg.kind == SNAP_CELL;
            SE_CHECK(!(rec && !has_ss) && !(sg.kind == SNAP_SLOT && has_ss), fn + "the snapshot's state is not of this model's kind");
            if (sg.kind == SNAP_SLOT) {
                SE_CHECK(sg.index == (int32_t)want_slots.size() && sg.bytes > 0, fn + "state slots out of order");
                want_slots.emplace_back(nullptr, (size_t)sg.bytes);
            }
        }
        check_payload_reachable(e, s, fn);
        // ---- every refusal is above: from here the call takes the handle's stream over, as se_stream_begin does
        hipStream_t st = static_cast<hipStream_t>(stream);
        S.active = false;
        payload_to_device(e, s, fn);
        stream_order_wait(S, st);
        obj_wait(s, st);
        S.max_chunk = m.max_chunk;
        if (!S.wav) {
            S.pitch = pitch;
            S.wav.alloc((size_t)e->ctx.max_batch * S.pitch);
            if (sliding) S.wav2.alloc((size_t)e->ctx.max_batch * S.pitch);
        }
        if (!S.c) S.c.alloc(e->ctx.max_batch);
        if (m.running && (!S.sumsq || S.ring != ring)) {
            if (!S.sumsq) S.sumsq.alloc((size_t)2 * e->ctx.max_batch);
            S.frame_inv.alloc((size_t)e->ctx.max_batch * ring);
            if (S.frame_c) S.frame_c.alloc((size_t)e->ctx.max_batch * ring);
            S.ring = ring;
        }
        if (m.running == 2 && !S.frame_c) S.frame_c.alloc((size_t)e->ctx.max_batch * S.ring);
        // the model's state buffers: left where they are when they already have the snapshot's layout (two groups that alternate
        // on one engine), else made as a new stream makes them - the slots of the cLN networks in the recorded order and sizes,
        // which a stream creates lazily on its first chunk and checks on every later one
        if (StreamState* ss = e->model->stream_state()) {
            if (ss->B != m.batch || !same_segs(engine_segments(e, m.batch, m.running, ring), m.segs, nfix))
                e->model->stream_begin(m.batch, m.max_chunk, st);
            ss->first = m.first != 0;
        } else if (StreamSlots* sl = e->model->stream_slots()) {
            bool same = sl->B == m.batch && sl->v.size() == want_slots.size() && !want_slots.empty();
            for (size_t i = 0; same && i < want_slots.size(); ++i) same = sl->v[i].second == want_slots[i].second;
            if (want_slots.empty()) {
                e->model->stream_begin(m.batch, m.max_chunk, st);
                // (slots an earlier stream of the same batch left are zero now: what a snapshot from before the first chunk means)
            } else if (!same) {
                sl->clear();
                for (auto& w : want_slots) {
                    void* d = nullptr;
                    SE_HIP(hipMalloc(&d, w.second));
                    sl->v.emplace_back(d, w.second);
                }
                sl->B = m.batch;
            }
        }
        const std::vector<EngSeg> eng = engine_segments(e, m.batch, m.running, ring);
        // (a snapshot from before the first chunk into an engine whose slots exist: they were zeroed above and stay out of the copy)
        std::vector<EngSeg> dst;
        for (const EngSeg& sg : eng)
            if (!(sg.seg.kind == SNAP_SLOT && want_slots.empty())) dst.push_back(sg);
        SE_CHECK(same_segs(dst, m.segs, nfix),
                 fn + "the snapshot's state buffers do not have the sizes this engine's model keeps (weights of other shapes?); the handle's stream has ended");
        S.start(m.batch, m.n_total, m.running == 1, m.running == 2, tau, g.hop);
        S.t_done = m.t_done;
        S.o_done = m.o_done;
        S.w0 = sliding ? m.keep : 0;
        long fix_tiles = 0;
        const StateSeg* tab = table_for(s, 1, dst, S.wav.get(), m.batch, &fix_tiles, st);
        StateWindow w;
        w.dst_off = m.keep - S.w0;
        w.src_pitch = live;
        w.dst_pitch = S.pitch;
        w.rows = m.batch;
        w.len = live;
        launch_stream_state_copy(tab, (int)dst.size(), fix_tiles, (int)dst.size(), w, st);
        S.active = true;
        stream_mark(S, st);
        obj_mark(s, st);
    });
}

}  // extern "C"

// ---- se_stream_state_select / se_stream_state_concat: a snapshot made of rows of others ---------------------------------------
// Only the model knows where the batch index sits in its carried buffers, so an engine of the snapshots' kind supplies the layouts
// (stream_rows.h): the engine's own segments follow from the manifest, the recurrent models declare theirs (Model::stream_layout,
// the declaration their buffers are allocated from), a call-order slot is [B][row bytes] by construction (StreamCtx::slot).  The
// manifest arithmetic is host code (stream_rows.h); the rows move in one launch (k_stream_state.hip, stream_state_gather_kernel).
// Neither call touches the stream running on the engine or its workspace.
//
// se_stream_state_join is concat for parts whose position counters differ by whole hops (stream_join.h: when a parked stream can be
// rebased, and the plan - shifts, the one window every row keeps): the same gather with a per-part column offset into the window
// (stream_state_join_kernel), the result on the counters of parts[0].  Nothing in a payload holds a position - the accepted models
// carry conv history and LSTM (h, c), the engine the scale c - so rebasing a part is a matter of the manifest alone.
namespace {

std::vector<RowLayout> snapshot_layouts(se_engine* e, const SnapManifest& m, const std::string& fn) {
    std::vector<RowLayout> lay(m.segs.size());
    StateLayout sl;
    const bool rec = e->model->stream_state() != nullptr;
    if (rec) sl = e->model->stream_layout();
    for (size_t k = 0; k < m.segs.size(); ++k) {
        const SnapSeg& sg = m.segs[k];
        if (snap_engine_layout(m, sg, lay[k])) continue;
        const std::string name = snap_seg_name(sg);
        SE_CHECK(m.state_B >= 1, fn + "segment " + name + " of a snapshot without model state");
        if (sg.kind == SNAP_SLOT) {
            SE_CHECK(!rec && e->model->stream_slots(), fn + "the snapshot's state is not of this model's kind");
            SE_CHECK(sg.bytes > 0 && sg.bytes % ((int64_t)m.state_B * 4) == 0,
                     fn + "state slot " + name + " of " + std::to_string(sg.bytes) + " bytes is not " + std::to_string(m.state_B) + " rows of whole floats");
            lay[k] = {1, sg.bytes / ((int64_t)m.state_B * 4)};
            continue;
        }
        SE_CHECK(rec, fn + "the snapshot's state is not of this model's kind");
        RowLayout l;
        if (sg.kind == SNAP_HIST && (size_t)sg.index < sl.hist.size()) l = sl.hist[(size_t)sg.index];
        else if (sg.kind == SNAP_H && sg.index < 4) l = sl.h[sg.index];
        else if (sg.kind == SNAP_CELL && sg.index < 4) l = sl.c[sg.index];
        SE_CHECK(l.outer >= 1, fn + "this engine's model keeps no state buffer " + name);
        lay[k] = l;
    }
    const std::string why = snap_layout_check(m, lay);
    SE_CHECK(why.empty(), fn + why + " (weights of other shapes?)");
    return lay;
}

struct RowSource {
    se_stream_state* part;
    int32_t row;
};

// "", or what in the state a stream of this engine's model carries counts frames from the start of the stream: such a state cannot be
// moved to another position.  The models that are left ignore stream_chunk()'s t0 ((void)t0 in CRN, LSTM, GCRN, DPCRN, DCCRN)
// With SE_CFG_STREAM_ROW_ORIGINS every row counts from its own origin, which the join moves along (stream_join.h): "" for every model
std::string join_counts_frames(const se_engine* e) {
    if (e->cfg.flags & SE_CFG_STREAM_ROW_ORIGINS) return "";
    const char* hint = " (an engine created with SE_CFG_STREAM_ROW_ORIGINS keeps a frame origin per row and joins this model)";
    switch (e->cfg.model) {
        case SE_MODEL_CTSNET:
        case SE_MODEL_G2NET:
        case SE_MODEL_TAYLORSENET:
            return std::string("the cumulative LayerNorm divides its running sums by the number of frames so far, and the TCM rings are indexed by the "
                               "absolute frame (StreamCtx::t0, k_tcm_stream.hip)") + hint;
        case SE_MODEL_FULLSUBNET:
            if (e->cfg.flags & SE_CFG_FSN_CUM_LAYERNORM)
                return std::string("the cumulative LayerNorm of FullSubNet divides its running sums by the absolute frame index (launch_fsn_cln_fb / "
                                   "launch_fsn_cln_sb), and the look-ahead skips the steps before frame 2 by it") + hint;
            return std::string("the cumulative Laplace norm divides its running sums by the absolute frame index (launch_fsn_cum_fb / launch_fsn_cum_sb), "
                               "and the look-ahead skips the steps before frame 2 by it") + hint;
        default:
            return "";
    }
}
static_assert(SNAP_FLAG_ROW_ORIGINS == SE_CFG_STREAM_ROW_ORIGINS, "stream_manifest.h names the bit of include/se_engine.h");

// dst <- the rows `src` names, in order; parts: the distinct source objects, every one checked against e and of one layout `lay`.
// jp (se_stream_state_join): the parts' windows differ in length - `lay` then describes the RESULT, whose window starts at jp->keep,
// and row bd of it is columns [jp->col[p], jp->col[p] + jp->live) of its part's window row; the counters are those of parts[0]
void gather_rows(se_engine* e, se_stream_state* dst, const std::vector<se_stream_state*>& parts, const std::vector<int2>& rowmap,
                 const std::vector<RowLayout>& lay, const std::string& fn, hipStream_t st, const JoinPlan* jp = nullptr) {
    const int Bd = (int)rowmap.size(), np = (int)parts.size();
    SnapManifest m = snap_rows_manifest(parts[0]->man, lay, Bd);
    if (jp) {
        SE_CHECK(!m.segs.empty() && m.segs.back().kind == SNAP_WINDOW && (int)jp->col.size() == np, fn + "snapshot without an input window segment");
        m.keep = jp->keep;
    }
    const int nseg = (int)m.segs.size();
    SE_CHECK(nseg >= 1, fn + "snapshot without segments");
    long tiles = 0;
    std::vector<GatherSeg> tab((size_t)nseg);
    for (int k = 0; k < nseg; ++k) {
        SE_CHECK(m.segs[(size_t)k].bytes / 4 < INT_MAX && lay[(size_t)k].outer < INT_MAX && lay[(size_t)k].inner < INT_MAX, fn + "segment too large");
        tab[(size_t)k].outer = (int)lay[(size_t)k].outer;
        tab[(size_t)k].inner = (int)lay[(size_t)k].inner;
        tab[(size_t)k].n = (int)(m.segs[(size_t)k].bytes / 4);
        tab[(size_t)k].tile0 = (int)tiles;
        tiles += state_gather_tiles(tab[(size_t)k].n);
        SE_CHECK(tiles < INT_MAX, fn + "too many tiles");
    }
    for (se_stream_state* p : parts) check_payload_reachable(e, p, fn);
    // ---- every refusal is above
    for (se_stream_state* p : parts) payload_to_device(e, p, fn);
    const StftGeom& g = e->ctx.geom;
    const int64_t win = m.segs.back().kind == SNAP_WINDOW ? snap_align16(m.segs.back().bytes) : 0;
    if (dst->has_use && dst->device != e->cfg.device) {
        DeviceScope ds(dst->device);
        SE_HIP(hipEventSynchronize(dst->side->ev_use.get()));
        dst->has_use = false;
    }
    payload_alloc(dst, m, std::max<int64_t>(win, (int64_t)Bd * snap_window_cap(g) * sizeof(float)), e->cfg.device);
    SE_CHECK(snap_payload_bytes(m) <= dst->dev_fixed + dst->dev_win_cap, fn + "payload smaller than its manifest");
    for (se_stream_state* p : parts) obj_wait(p, st);
    obj_wait(dst, st);
    // one block: GatherSeg[nseg] | long src_off[np][nseg] | const float* base[np] | int2 rowmap[Bd] | int part_B[np]
    // (join: | int window row length[np] | int window column[np] | int ring rotation[np] | int shift in frames[np])
    const size_t o_off = (size_t)nseg * sizeof(GatherSeg), o_base = o_off + (size_t)np * nseg * sizeof(long),
                 o_map = o_base + (size_t)np * sizeof(float*), o_pb = o_map + (size_t)Bd * sizeof(int2), o_win = o_pb + (size_t)np * sizeof(int),
                 total = o_win + (jp ? 4 * (size_t)np * sizeof(int) : 0);
    auto& sd = *dst->side;
    SE_HIP(hipEventSynchronize(sd.gat_ev.get()));
    if (total > sd.gat_cap) {
        const size_t cap = std::max<size_t>(total + 4096, 32768);
        sd.gat_cap = 0;
        sd.gat_dev.alloc(cap);
        sd.gat_pin.alloc(cap);
        sd.gat_cap = cap;
    }
    uint8_t* pin = sd.gat_pin.get();
    const std::vector<int64_t> doff = snap_offsets(m);
    for (int k = 0; k < nseg; ++k) tab[(size_t)k].dst = reinterpret_cast<float*>(dst->side->dev.get() + doff[(size_t)k]);
    std::memcpy(pin, tab.data(), o_off);
    long* soff = reinterpret_cast<long*>(pin + o_off);
    const float** base = reinterpret_cast<const float**>(pin + o_base);
    int* pb = reinterpret_cast<int*>(pin + o_pb);
    for (int p = 0; p < np; ++p) {
        const std::vector<int64_t> off = snap_offsets(parts[(size_t)p]->man);
        for (int k = 0; k < nseg; ++k) soff[(size_t)p * nseg + k] = (long)(off[(size_t)k] / 4);
        base[p] = reinterpret_cast<const float*>(parts[(size_t)p]->side->dev.get());
        pb[p] = parts[(size_t)p]->man.batch;
        if (jp) {
            int* wi = reinterpret_cast<int*>(pin + o_win);
            wi[p] = parts[(size_t)p]->man.n_total - parts[(size_t)p]->man.keep;
            wi[np + p] = jp->col[(size_t)p];
            wi[2 * np + p] = jp->rot[(size_t)p];
            wi[3 * np + p] = jp->frames[(size_t)p];
        }
    }
    std::memcpy(pin + o_map, rowmap.data(), (size_t)Bd * sizeof(int2));
    uint8_t* dev = sd.gat_dev.get();
    SE_HIP(hipMemcpyAsync(dev, pin, total, hipMemcpyHostToDevice, st));
    SE_HIP(hipEventRecord(sd.gat_ev.get(), st));
    GatherArgs a{};
    a.tab = reinterpret_cast<const GatherSeg*>(dev);
    a.src_off = reinterpret_cast<const long*>(dev + o_off);
    a.part_base = reinterpret_cast<const float* const*>(dev + o_base);
    a.rowmap = reinterpret_cast<const int2*>(dev + o_map);
    a.part_B = reinterpret_cast<const int*>(dev + o_pb);
    a.nseg = nseg;
    a.Bd = Bd;
    if (jp) {
        JoinWindow w;
        w.seg = nseg - 1;
        w.part_inner = reinterpret_cast<const int*>(dev + o_win);
        w.part_col = w.part_inner + np;
        w.part_rot = w.part_inner + 2 * np;
        // the rows' frame origins move with the frames too (stream_join.h): + shift / hop on the way through the same launch
        w.part_frames = w.part_inner + 3 * np;
        for (int k = 0; k < nseg; ++k)
            if (m.segs[(size_t)k].kind == SNAP_ORIGIN) {
                SE_CHECK(w.origin_seg < 0 && tab[(size_t)k].outer == 1 && tab[(size_t)k].inner == 1 && tab[(size_t)k].n == Bd && (int)jp->frames.size() == np,
                         fn + "frame origin segment of an odd layout");
                w.origin_seg = k;
            }
        // the per-frame rings of a tracking-scale group move with the frames (stream_join.h): the SNAP_FRAME_INV segments, side by side
        for (int k = 0; k < nseg; ++k)
            if (m.segs[(size_t)k].kind == SNAP_FRAME_INV && m.running == 2) {
                SE_CHECK(tab[(size_t)k].inner == m.ring && (m.ring & (m.ring - 1)) == 0, fn + "per-frame ring of an odd length");
                if (w.ring_hi == w.ring_lo) w.ring_lo = k, w.ring_hi = k + 1;
                else if (k == w.ring_hi) w.ring_hi = k + 1;
                else SE_CHECK(false, fn + "per-frame rings are not adjacent segments");
            }
        launch_stream_state_join(a, w, tiles, st);
    } else {
        launch_stream_state_gather(a, tiles, st);
    }
    dst->man = m;
    dst->filled = true;
    dst->dev_valid = true;
    dst->host.clear();
    dst->host.shrink_to_fit();
    obj_mark(dst, st);
    for (se_stream_state* p : parts) obj_mark(p, st);
}

}  // namespace

extern "C" {

int se_stream_state_select(se_engine* e, se_stream_state* dst, const se_stream_state* csrc, const int32_t* rows, int32_t n_rows,
                           void* stream) {
    if (!e) return 1;
    return guard(e, [&] {
        const std::string fn = "se_stream_state_select: ";
        se_stream_state* src = const_cast<se_stream_state*>(csrc);      // (the uploaded payload is a cache of the object)
        SE_CHECK(dst && src, fn + "null argument");
        SE_CHECK(e->finalized, "engine not finalized");
        SE_CHECK(dst != src, fn + "dst == src: the rows are read while they are written");
        SE_CHECK(src->filled, fn + "the stream state object is empty");
        check_snapshot_identity(e, src->man, fn);
        const std::string bad = snap_rows_check(rows, n_rows, src->man.batch);
        SE_CHECK(bad.empty(), fn + bad);
        const std::vector<RowLayout> lay = snapshot_layouts(e, src->man, fn);
        std::vector<int2> map((size_t)n_rows);
        for (int32_t j = 0; j < n_rows; ++j) map[(size_t)j] = make_int2(0, rows[j]);
        gather_rows(e, dst, {src}, map, lay, fn, static_cast<hipStream_t>(stream));
    });
}

int se_stream_state_concat(se_engine* e, se_stream_state* dst, const se_stream_state* const* cparts, int32_t n_parts, void* stream) {
    if (!e) return 1;
    return guard(e, [&] {
        const std::string fn = "se_stream_state_concat: ";
        SE_CHECK(dst && cparts, fn + "null argument");
        SE_CHECK(e->finalized, "engine not finalized");
        SE_CHECK(n_parts >= 1, fn + "n_parts " + std::to_string(n_parts) + ": at least one part has to be given");
        std::vector<se_stream_state*> parts;
        std::vector<int2> map;
        int64_t total = 0;
        for (int32_t p = 0; p < n_parts; ++p) {
            se_stream_state* s = const_cast<se_stream_state*>(cparts[p]);
            SE_CHECK(s, fn + "parts[" + std::to_string(p) + "] is null");
            SE_CHECK(s != dst, fn + "dst == parts[" + std::to_string(p) + "]: the rows are read while they are written");
            SE_CHECK(s->filled, fn + "parts[" + std::to_string(p) + "]: the stream state object is empty");
            if (p > 0) {
                const std::string why = snap_concat_differs(cparts[0]->man, s->man);
                SE_CHECK(why.empty(), fn + "parts[0] and parts[" + std::to_string(p) + "] differ: " + why);
            }
            total += s->man.batch;
            SE_CHECK(total < (1 << 24), fn + "too many rows");
            parts.push_back(s);
        }
        check_snapshot_identity(e, parts[0]->man, fn);
        const std::vector<RowLayout> lay = snapshot_layouts(e, parts[0]->man, fn);
        for (int32_t p = 0; p < n_parts; ++p) {
            if (p > 0) {      // the same layouts hold part p's sizes (a slot's row size is read off part 0)
                const std::string why = snap_layout_check(parts[(size_t)p]->man, lay);
                SE_CHECK(why.empty(), fn + "parts[" + std::to_string(p) + "]: " + why);
            }
            for (int32_t r = 0; r < parts[(size_t)p]->man.batch; ++r) map.push_back(make_int2(p, r));
        }
        gather_rows(e, dst, parts, map, lay, fn, static_cast<hipStream_t>(stream));
    });
}

int se_stream_state_join(se_engine* e, se_stream_state* dst, const se_stream_state* const* cparts, int32_t n_parts, void* stream) {
    if (!e) return 1;
    return guard(e, [&] {
        const std::string fn = "se_stream_state_join: ";
        SE_CHECK(dst && cparts, fn + "null argument");
        SE_CHECK(e->finalized, "engine not finalized");
        SE_CHECK(n_parts >= 1, fn + "n_parts " + std::to_string(n_parts) + ": at least one part has to be given");
        std::vector<se_stream_state*> parts;
        std::vector<const SnapManifest*> mans;
        int64_t total = 0;
        for (int32_t p = 0; p < n_parts; ++p) {
            se_stream_state* s = const_cast<se_stream_state*>(cparts[p]);
            SE_CHECK(s, fn + "parts[" + std::to_string(p) + "] is null");
            SE_CHECK(s != dst, fn + "dst == parts[" + std::to_string(p) + "]: the rows are read while they are written");
            SE_CHECK(s->filled, fn + "parts[" + std::to_string(p) + "]: the stream state object is empty");
            total += s->man.batch;
            SE_CHECK(total < (1 << 24), fn + "too many rows");
            parts.push_back(s);
            mans.push_back(&s->man);
        }
        check_snapshot_identity(e, parts[0]->man, fn);
        JoinPlan plan;
        const std::string why = snap_join_plan(mans, e->model->stream_lag(), join_counts_frames(e), plan, e->model->stream_state() != nullptr);
        SE_CHECK(why.empty(), fn + why);
        // every part against the layouts of this engine's model, its window at its own length; the result's at the joined length
        std::vector<RowLayout> lay = snapshot_layouts(e, parts[0]->man, fn);
        SE_CHECK(!lay.empty() && parts[0]->man.segs.back().kind == SNAP_WINDOW, fn + "snapshot without an input window segment");
        std::vector<int2> map;
        for (int32_t p = 0; p < n_parts; ++p) {
            const SnapManifest& pm = parts[(size_t)p]->man;
            if (p > 0) {
                lay.back().inner = (int64_t)pm.n_total - pm.keep;
                const std::string bad = snap_layout_check(pm, lay);
                SE_CHECK(bad.empty(), fn + "parts[" + std::to_string(p) + "]: " + bad);
            }
            for (int32_t r = 0; r < pm.batch; ++r) map.push_back(make_int2(p, r));
        }
        lay.back().inner = plan.live;
        gather_rows(e, dst, parts, map, lay, fn, static_cast<hipStream_t>(stream), &plan);
    });
}

int se_stream_state_counts(const se_stream_state* s, int32_t* batch, int64_t* n_total, int64_t* t_done, int64_t* o_done, int32_t* hop) {
    return guard(nullptr, [&] {
        SE_CHECK(s, "se_stream_state_counts: null argument");
        SE_CHECK(s->filled, "se_stream_state_counts: the stream state object is empty");
        if (batch) *batch = s->man.batch;
        if (n_total) *n_total = s->man.n_total;
        if (t_done) *t_done = s->man.t_done;
        if (o_done) *o_done = s->man.o_done;
        if (hop) *hop = s->man.hop;
    });
}

int64_t se_stream_state_export(const se_stream_state* s, void* host_buf, int64_t cap) {
    int64_t ret = -1;
    guard(nullptr, [&] {
        SE_CHECK(s, "se_stream_state_export: null argument");
        SE_CHECK(s->filled, "se_stream_state_export: the stream state object is empty");
        const int64_t size = snap_image_bytes(s->man), table = snap_table_bytes(s->man), pay = snap_payload_bytes(s->man);
        if (cap == 0) {
            ret = size;
            return;
        }
        SE_CHECK(host_buf && cap >= size, "se_stream_state_export: the buffer holds " + std::to_string(cap) + " bytes, the image needs " + std::to_string(size));
        uint8_t* out = static_cast<uint8_t*>(host_buf);
        snap_write_table(s->man, out);
        if (!s->host.empty()) {
            SE_CHECK((int64_t)s->host.size() == pay, "se_stream_state_export: host image of the wrong size");
            std::memcpy(out + table, s->host.data(), (size_t)pay);
        } else {
            SE_CHECK(s->side->dev && s->dev_valid, "se_stream_state_export: no payload");
            DeviceScope ds(s->device);
            se_stream_state* ms = const_cast<se_stream_state*>(s);
            if (s->has_use) SE_HIP(hipEventSynchronize(ms->side->ev_use.get()));
            if (pay > 0) SE_HIP(hipMemcpy(out + table, s->side->dev.get(), (size_t)pay, hipMemcpyDeviceToHost));
            int64_t off = 0;
            for (const SnapSeg& sg : s->man.segs) {      // the bytes between two segments are nobody's: zeros in the image
                std::memset(out + table + off + sg.bytes, 0, (size_t)(snap_align16(sg.bytes) - sg.bytes));
                off += snap_align16(sg.bytes);
            }
        }
        ret = size;
    });
    return ret;
}

int se_stream_state_import(se_stream_state* s, const void* host_buf, int64_t bytes) {
    return guard(nullptr, [&] {
        SE_CHECK(s && host_buf, "se_stream_state_import: null argument");
        SnapManifest m;
        int64_t off = 0;
        const std::string why = snap_parse(host_buf, bytes, m, off);
        SE_CHECK(why.empty(), "se_stream_state_import: " + why);
        std::vector<uint8_t> pay(static_cast<const uint8_t*>(host_buf) + off, static_cast<const uint8_t*>(host_buf) + bytes);
        // nothing of the object has changed up to here
        s->man = std::move(m);
        s->host = std::move(pay);
        s->filled = true;
        s->dev_valid = false;
    });
}

}  // extern "C"

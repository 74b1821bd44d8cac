// C ABI of the engine (include/se_engine.h): handle, strict state-dict load, stage hooks.
// (parked streams - se_stream_save / _restore and the se_stream_state_* calls - are stream_state.hip; what the two units share is
// engine_impl.h)
#include "engine_impl.h"
#include "resampler.h"
#include "stream_window.h"
#include "window_rows.h"
#include <algorithm>
#include <climits>

std::string g_create_err;

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
        // (SE_CFG_FSN_LOOK_AHEAD(2) spells the script's look_ahead, which an empty field means too: one engine, one set of flags - the
        // parked-stream calls compare them - so the field is stored empty)
        if (cfg->model == SE_MODEL_FULLSUBNET && ((cfg->flags >> 22) & 7u) == 3u) e->cfg.flags &= ~(7u << 22);
        e->ctx.flags = e->cfg.flags;
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
        // (FullSubNet's look_ahead and fb_num_neighbors: bits 22-24 hold look_ahead + 1 with 0 = the script's 2, bits 25-28 the count)
        {
            const uint32_t shape = (7u << 22) | (15u << 25);
            SE_CHECK(!(cfg->flags & shape) || cfg->model == SE_MODEL_FULLSUBNET,
                     "SE_CFG_FSN_LOOK_AHEAD and SE_CFG_FSN_FB_NEIGHBORS are fields of SE_MODEL_FULLSUBNET (its look_ahead and "
                     "fb_num_neighbors): no other model takes them");
            // (every value of the three-bit field is a look_ahead the engine builds: 1..7 = 0..6 frames)
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
    scratch_owner_release(dev, e->scratch_own);      // (the device is idle and the graphs that named these buffers are gone)
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
            // warm-up and capture take the scratch of forked work under this engine's own keys (common.h: ScratchOwner): the
            // warm-up grows the very slots whose addresses the capture bakes in
            static_assert(ScratchOwner::N == EngineCtx::MAX_AUX, "one scratch key per auxiliary stream");
            e->scratch_own.from = e->ctx.aux;
            struct OwnScratch {
                explicit OwnScratch(ScratchOwner* o) { scratch_owner_set(o); }
                ~OwnScratch() { scratch_owner_set(nullptr); }
            } own(&e->scratch_own);
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

}  // extern "C"

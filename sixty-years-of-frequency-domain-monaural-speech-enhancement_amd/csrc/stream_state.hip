// Parked frame-online streams (se_stream_save / se_stream_restore and the se_stream_state_* calls of include/se_engine.h): a running
// stream put into an object of its own and put back, and snapshots made of rows of others.
// The object: the manifest (stream_manifest.h, host) + one device payload, every carried buffer at a 16 B aligned offset, the input
// window last; what it shares with every parked object - ordering, release, upload, export, import - is parked.h.  The payload is
// sized when a layout is first seen - its window part for the most a stream keeps live between two calls - so saving again into the
// same object allocates nothing.  The two device tables (engine -> payload, payload -> engine) of the copy kernel
// (k_stream_state.hip) are rebuilt on the host at every call, which is a few hundred assignments, and uploaded only when they differ
// from the last upload: through a pinned buffer, so that the call waits for nothing either.
// (the calls below are declared extern "C" by include/se_engine.h and keep that linkage)
#include "engine_impl.h"
#include "parked.h"
#include "stream_manifest.h"
#include "k_stream_state.h"
#include "stream_join.h"
#include "stream_rows.h"
#include "stream_window.h"
#include <climits>
#include <cstring>

struct se_stream_state : Parked {
    SnapManifest man;
    std::vector<SnapSeg> dev_layout;      // the segments in front of the window the payload was laid out for
    int64_t dev_fixed = 0, dev_win_cap = 0;
    struct Table {
        DevBuf<StateSeg> dev;
        PinnedBuf<StateSeg> pin;
        size_t cap = 0;
        std::vector<StateSeg> last;
        Event ev;                         // behind the last upload: the pinned buffer is free again
    };
    struct StreamSide : Side {            // (an imported image may be restored on several devices, one after the other)
        Table tab[2];                     // 0: save, 1: restore
        // se_stream_state_select / _concat into this object: the gather kernel's tables (segments, source offsets, part bases, row
        // map) in one block, through a pinned copy of it
        DevBuf<uint8_t> gat_dev;
        PinnedBuf<uint8_t> gat_pin;
        size_t gat_cap = 0;
        Event gat_ev;                     // behind the last upload: the pinned block is free again
    };
    std::unique_ptr<Side> make_side() const override { return std::unique_ptr<Side>(new StreamSide()); }
    StreamSide& sd() { return static_cast<StreamSide&>(*side); }
};

namespace {

struct EngSeg : SnapSeg {
    void* ptr;
};

// every buffer chunk k of the stream writes and chunk k + 1 reads, except the input window, in payload order
// (mode: SnapManifest::running - 0 a fixed scale, 1 the running scale, 2 the tracking scale)
std::vector<EngSeg> engine_segments(se_engine* e, int batch, int mode, int ring) {
    se_engine::Stream& S = e->strm;
    std::vector<EngSeg> v;
    auto add = [&](int32_t kind, int32_t index, void* p, int64_t bytes) {
        EngSeg s;
        s.kind = kind;
        s.index = index;
        s.bytes = bytes;
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

// a (engine segments, or a layout) is the first nb segments of b
template <typename Seg>
bool same_segs(const std::vector<Seg>& a, const std::vector<SnapSeg>& b, size_t nb) {
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

// a payload buffer on the current device for the layout of m (window part: at least win_cap bytes); the old contents are dropped
void payload_alloc(se_stream_state* s, const SnapManifest& m, int64_t win_cap, int device) {
    const size_t nfix = fixed_count_of(m);
    const int64_t fixed = fixed_bytes_of(m);
    if (s->has_payload() && s->device == device && same_segs(s->dev_layout, m.segs, nfix) && s->dev_win_cap >= win_cap) return;
    s->fresh_payload((size_t)(fixed + win_cap + 16), device);
    s->dev_layout.assign(m.segs.begin(), m.segs.begin() + (long)nfix);
    s->dev_fixed = fixed;
    s->dev_win_cap = win_cap;
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
            SE_CHECK(eng[i].bytes / 4 < INT_MAX, "stream state: segment too large");
            sg.rows = 1;
            sg.len = (int)(eng[i].bytes / 4);
            sg.tile0 = (int)tiles;
            tiles += state_seg_tiles(1, sg.len);
            SE_CHECK(tiles < INT_MAX, "stream state: too many tiles");
            off += snap_align16(eng[i].bytes);
        } else {
            sg.rows = batch;          // the window: extent from the call
            sg.tile0 = (int)tiles;
        }
        v[i] = sg;
    }
    *fix_tiles = tiles;
    auto& T = s->sd().tab[dir];
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
    if (!s->on_device(e->cfg.device))
        SE_CHECK(!s->host.empty(), fn + "the payload lives on device " + std::to_string(s->device) + ", this engine on device " +
                                       std::to_string(e->cfg.device) + " (export the state and import it to move it)");
}
// ... and puts it there (e's device is current): once, until the object is saved into again
void payload_to_device(const se_engine* e, se_stream_state* s, const std::string& fn) {
    if (s->on_device(e->cfg.device)) return;
    const SnapManifest& m = s->man;
    const int64_t win = m.segs.empty() ? 0 : snap_align16(m.segs.back().bytes);
    payload_alloc(s, m, std::max<int64_t>(win, (int64_t)m.batch * snap_window_cap(e->ctx.geom) * sizeof(float)), e->cfg.device);
    SE_CHECK((int64_t)s->host.size() == snap_payload_bytes(m), fn + "host image of the wrong size");
    s->upload_host();
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
        s->drop_side();
    });
}

int64_t se_stream_state_bytes(const se_stream_state* s) {
    if (!s || !s->filled) return 0;
    return s->has_payload() ? s->dev_fixed + s->dev_win_cap : snap_payload_bytes(s->man);
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
            SE_CHECK(sg.ptr && sg.bytes >= 0 && (sg.bytes & 3) == 0, "se_stream_save: a carried buffer is missing or of an odd size");
            m.segs.push_back(sg);
        }
        SnapSeg wseg;
        wseg.kind = SNAP_WINDOW;
        wseg.bytes = (int64_t)S.batch * live * sizeof(float);
        m.segs.push_back(wseg);
        // nothing of the object or the stream has changed up to here
        payload_alloc(s, m, (int64_t)S.batch * wcap * sizeof(float), e->cfg.device);
        stream_order_wait(S, st);
        s->wait(st);
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
        s->set_saved();
        stream_mark(S, st);
        s->mark(st);
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
        s->wait(st);
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
            if (!(sg.kind == SNAP_SLOT && want_slots.empty())) dst.push_back(sg);
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
        s->mark(st);
    });
}

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
    if (dst->device != e->cfg.device) dst->sync_use();
    payload_alloc(dst, m, std::max<int64_t>(win, (int64_t)Bd * snap_window_cap(g) * sizeof(float)), e->cfg.device);
    SE_CHECK(snap_payload_bytes(m) <= dst->dev_fixed + dst->dev_win_cap, fn + "payload smaller than its manifest");
    for (se_stream_state* p : parts) p->wait(st);
    dst->wait(st);
    // one block: GatherSeg[nseg] | long src_off[np][nseg] | const float* base[np] | int2 rowmap[Bd] | int part_B[np]
    // (join: | int window row length[np] | int window column[np] | int ring rotation[np] | int shift in frames[np])
    const size_t o_off = (size_t)nseg * sizeof(GatherSeg), o_base = o_off + (size_t)np * nseg * sizeof(long),
                 o_map = o_base + (size_t)np * sizeof(float*), o_pb = o_map + (size_t)Bd * sizeof(int2), o_win = o_pb + (size_t)np * sizeof(int),
                 total = o_win + (jp ? 4 * (size_t)np * sizeof(int) : 0);
    auto& sd = dst->sd();
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
    dst->set_saved();
    dst->mark(st);
    for (se_stream_state* p : parts) p->mark(st);
}

}  // namespace

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
        const std::vector<se_stream_state*> parts = collect_parts(dst, cparts, n_parts, fn, "stream state", [&](int32_t p, const se_stream_state* s) {
            const std::string why = p > 0 ? snap_concat_differs(cparts[0]->man, s->man) : "";
            SE_CHECK(why.empty(), fn + "parts[0] and parts[" + std::to_string(p) + "] differ: " + why);
        });
        check_snapshot_identity(e, parts[0]->man, fn);
        const std::vector<RowLayout> lay = snapshot_layouts(e, parts[0]->man, fn);
        for (int32_t p = 1; p < n_parts; ++p) {      // the same layouts hold part p's sizes (a slot's row size is read off part 0)
            const std::string why = snap_layout_check(parts[(size_t)p]->man, lay);
            SE_CHECK(why.empty(), fn + "parts[" + std::to_string(p) + "]: " + why);
        }
        gather_rows(e, dst, parts, part_rows(parts), lay, fn, static_cast<hipStream_t>(stream));
    });
}

int se_stream_state_join(se_engine* e, se_stream_state* dst, const se_stream_state* const* cparts, int32_t n_parts, void* stream) {
    if (!e) return 1;
    return guard(e, [&] {
        const std::string fn = "se_stream_state_join: ";
        SE_CHECK(dst && cparts, fn + "null argument");
        SE_CHECK(e->finalized, "engine not finalized");
        std::vector<const SnapManifest*> mans;
        const std::vector<se_stream_state*> parts =
            collect_parts(dst, cparts, n_parts, fn, "stream state", [&](int32_t, const se_stream_state* s) { mans.push_back(&s->man); });
        check_snapshot_identity(e, parts[0]->man, fn);
        JoinPlan plan;
        const std::string why = snap_join_plan(mans, e->model->stream_lag(), join_counts_frames(e), plan, e->model->stream_state() != nullptr);
        SE_CHECK(why.empty(), fn + why);
        // every part against the layouts of this engine's model, its window at its own length; the result's at the joined length
        std::vector<RowLayout> lay = snapshot_layouts(e, parts[0]->man, fn);
        SE_CHECK(!lay.empty() && parts[0]->man.segs.back().kind == SNAP_WINDOW, fn + "snapshot without an input window segment");
        for (int32_t p = 1; p < n_parts; ++p) {
            const SnapManifest& pm = parts[(size_t)p]->man;
            lay.back().inner = (int64_t)pm.n_total - pm.keep;
            const std::string bad = snap_layout_check(pm, lay);
            SE_CHECK(bad.empty(), fn + "parts[" + std::to_string(p) + "]: " + bad);
        }
        lay.back().inner = plan.live;
        gather_rows(e, dst, parts, part_rows(parts), lay, fn, static_cast<hipStream_t>(stream), &plan);
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
        const bool from_host = !s->host.empty();
        if (from_host) SE_CHECK((int64_t)s->host.size() == pay, "se_stream_state_export: host image of the wrong size");
        else SE_CHECK(s->resident(), "se_stream_state_export: no payload");
        const_cast<se_stream_state*>(s)->export_payload(out + table, (size_t)pay);      // (the event is a cache of the object)
        if (!from_host) {
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
        s->adopt_image(std::move(pay));
    });
}

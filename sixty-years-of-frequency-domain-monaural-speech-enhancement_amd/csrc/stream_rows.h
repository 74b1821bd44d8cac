// Rows of a parked stream group (se_stream_state_select / se_stream_state_concat, include/se_engine.h): where the batch index sits in
// every carried buffer, and the manifest arithmetic of a snapshot made from some rows of others.  Host code alone, no HIP - the
// engine includes it, and so does a stand-alone check program (tests/stream_select_check.cpp).
//
// A carried buffer made for Bs rows is [outer][Bs][inner] floats: element (o, b, i) lives at (o * Bs + b) * inner + i.
//   conv history [B][rows][HC]              (1, rows * HC)         LSTM state [H][B]                 (H, 1)
//   DCCRN's complex LSTM [2][128][2 B]      (2 * 128 * 2, 1)       a per-sequence state [H][F][B]    (H * F, 1)
//   a call-order slot [B][row bytes]        (1, row bytes / 4)     sumsq [B] doubles                 (1, 2)
//   (E, W) [B][2] doubles (tracking scale)  (1, 4)
//   frame_inv, frame_c [B][ring]            (1, ring)              the window [B][n_total - keep]    (1, n_total - keep)
//   frame origins [B] int32                 (1, 1)
// The layouts are not part of a snapshot: the model declares them where it allocates the buffers (rnn.h StreamState::begin,
// kernels.h StreamCtx::slot), and an engine of the snapshot's kind is asked for them when rows are selected or joined.
#pragma once
#include "stream_manifest.h"

namespace se {

struct RowLayout {
    int64_t outer = 0, inner = 0;      // floats; outer == 0: no such buffer
};

// the layouts a model with recurrent state declares (rnn.h StreamState): history tensors in order, (h, c) of up to four layers
struct StateLayout {
    std::vector<RowLayout> hist;
    RowLayout h[4], c[4];
};

// the segments whose layout follows from the manifest alone (the engine's own buffers); false: a buffer of the model
inline bool snap_engine_layout(const SnapManifest& m, const SnapSeg& s, RowLayout& l) {
    switch (s.kind) {
        case SNAP_C: l = {1, 1}; return true;
        case SNAP_SUMSQ: l = {1, m.running == 2 ? 4 : 2}; return true;      // (tracking scale: (E, W) per row)
        case SNAP_FRAME_INV: l = {1, m.ring}; return true;
        case SNAP_WINDOW: l = {1, (int64_t)m.n_total - m.keep}; return true;
        case SNAP_ORIGIN: l = {1, 1}; return true;      // (int32, moved like floats: select and concat cut it by rows, the join adds to it)
        default: return false;
    }
}

inline const char* snap_kind_name(int32_t kind) {
    static const char* const names[] = {"?", "c", "sumsq", "frame_inv", "hist", "h", "cell", "slot", "window", "origin"};
    return kind >= SNAP_C && kind <= SNAP_KIND_MAX ? names[kind] : names[0];
}
inline std::string snap_seg_name(const SnapSeg& s) { return std::string(snap_kind_name(s.kind)) + "[" + std::to_string(s.index) + "]"; }

// "" or why `rows` cannot pick rows of a snapshot of `batch` rows
inline std::string snap_rows_check(const int32_t* rows, int32_t n_rows, int32_t batch) {
    if (n_rows < 1) return "n_rows " + std::to_string(n_rows) + ": at least one row has to be selected";
    if (!rows) return "null row list";
    for (int32_t j = 0; j < n_rows; ++j)
        if (rows[j] < 0 || rows[j] >= batch)
            return "rows[" + std::to_string(j) + "] = " + std::to_string(rows[j]) + " outside 0 .. " + std::to_string(batch - 1);
    return "";
}

// Every segment of m against its layout: lay[k] describes m.segs[k] for m.batch rows.  "" or the segment that does not fit
inline std::string snap_layout_check(const SnapManifest& m, const std::vector<RowLayout>& lay) {
    if (lay.size() != m.segs.size()) return "layouts for " + std::to_string(lay.size()) + " segments, the snapshot has " + std::to_string(m.segs.size());
    if (m.state_B != 0 && m.state_B != m.batch)
        return "the model state was made for " + std::to_string(m.state_B) + " rows, the group has " + std::to_string(m.batch);
    for (size_t k = 0; k < lay.size(); ++k) {
        const RowLayout& l = lay[k];
        if (l.outer < 1 || l.inner < 0 || l.outer > SNAP_MAX_BYTES || l.inner > SNAP_MAX_BYTES)
            return "segment " + snap_seg_name(m.segs[k]) + " has no row layout";
        if (l.outer * (int64_t)m.batch * l.inner * 4 != m.segs[k].bytes)
            return "segment " + snap_seg_name(m.segs[k]) + " holds " + std::to_string(m.segs[k].bytes) + " bytes, its layout [" + std::to_string(l.outer) +
                   "][" + std::to_string(m.batch) + "][" + std::to_string(l.inner) + "] floats describes " +
                   std::to_string(l.outer * (int64_t)m.batch * l.inner * 4);
    }
    return "";
}

// the manifest of n_rows rows with the counters, modes and layouts of src: batch and state_B, and the segment sizes they scale
inline SnapManifest snap_rows_manifest(const SnapManifest& src, const std::vector<RowLayout>& lay, int32_t n_rows) {
    SnapManifest d = src;
    d.batch = n_rows;
    d.state_B = src.state_B ? n_rows : 0;
    for (size_t k = 0; k < d.segs.size(); ++k) d.segs[k].bytes = lay[k].outer * (int64_t)n_rows * lay[k].inner * 4;
    return d;
}

// payload offset (bytes) of every segment
inline std::vector<int64_t> snap_offsets(const SnapManifest& m) {
    std::vector<int64_t> off(m.segs.size());
    int64_t o = 0;
    for (size_t k = 0; k < m.segs.size(); ++k) {
        off[k] = o;
        o += snap_align16(m.segs[k].bytes);
    }
    return off;
}

// "" or the first field in which part b differs from part a (index ib / ia in the reason): everything except batch, state_B and
// the segment sizes has to agree for the two to be rows of one group.  positions == false leaves out n_total, t_done, o_done and keep
// (se_stream_state_join, stream_join.h: parts whose positions differ by whole hops)
inline std::string snap_concat_differs(const SnapManifest& a, const SnapManifest& b, bool positions = true) {
    auto ne = [](const char* name, int64_t x, int64_t y) { return std::string(name) + " " + std::to_string(x) + " vs " + std::to_string(y); };
#define SE_SNAP_SAME(f) \
    if (a.f != b.f) return ne(#f, a.f, b.f);
    SE_SNAP_SAME(model) SE_SNAP_SAME(flags) SE_SNAP_SAME(n_fft) SE_SNAP_SAME(hop) SE_SNAP_SAME(win)
    SE_SNAP_SAME(max_chunk)
    if (positions) {
        SE_SNAP_SAME(n_total) SE_SNAP_SAME(t_done) SE_SNAP_SAME(o_done) SE_SNAP_SAME(keep)
    }
    SE_SNAP_SAME(running) SE_SNAP_SAME(ring) SE_SNAP_SAME(first)
#undef SE_SNAP_SAME
    if (a.running == 2 && a.reserved[0] != b.reserved[0]) {      // the float bits of se_stream_begin_tracking's time constant
        float ta, tb;
        std::memcpy(&ta, &a.reserved[0], sizeof(float));
        std::memcpy(&tb, &b.reserved[0], sizeof(float));
        return "tau_samples " + std::to_string(ta) + " vs " + std::to_string(tb);
    }
    if (a.p_in != b.p_in) return "p_in " + std::to_string(a.p_in) + " vs " + std::to_string(b.p_in);
    if (a.p_out != b.p_out) return "p_out " + std::to_string(a.p_out) + " vs " + std::to_string(b.p_out);
    if ((a.state_B != 0) != (b.state_B != 0)) return ne("state_B", a.state_B, b.state_B);
    if (a.segs.size() != b.segs.size()) return ne("segment count", (int64_t)a.segs.size(), (int64_t)b.segs.size());
    for (size_t k = 0; k < a.segs.size(); ++k)
        if (a.segs[k].kind != b.segs[k].kind || a.segs[k].index != b.segs[k].index)
            return "segment " + std::to_string(k) + " " + snap_seg_name(a.segs[k]) + " vs " + snap_seg_name(b.segs[k]);
    return "";
}

}  // namespace se

// The manifest of a parked frame-online stream (se_stream_save / se_stream_restore, include/se_engine.h) and its host image: host
// code alone, no HIP - the engine includes it, and so does a stand-alone check program (tests/stream_manifest_check.cpp).
//
// A snapshot is this record + one payload: the carried device buffers back to back, each at a 16 B aligned offset, in the order of
// `segs`.  The input window goes last: it is the one segment whose size changes from save to save (the live samples), so every
// other offset stays where the first save of a layout put it.
//
// Host image (se_stream_state_export / _import), little endian as the hosts this runs on:
//   u32 magic 'SEST' | u32 version | i32 x 18 engine + stream fields | f32 p_in | f32 p_out | i32 nseg | i32 0 | i64 payload bytes
//   nseg x { i32 kind | i32 index | i64 bytes }
//   payload: segment k at the sum of the 16 B rounded sizes before it, `payload bytes` in all
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace se {

enum SnapKind : int32_t {
    SNAP_C = 1,          // Stream::c          [batch] float
    SNAP_SUMSQ = 2,      // Stream::sumsq      [batch] double            (running scale only)
    SNAP_FRAME_INV = 3,  // Stream::frame_inv  [batch][ring] float       (running scale only)
    SNAP_HIST = 4,       // StreamState::hist[index]
    SNAP_H = 5,          // StreamState::h[index]
    SNAP_CELL = 6,       // StreamState::c[index]
    SNAP_SLOT = 7,       // StreamSlots::v[index], in call order
    SNAP_WINDOW = 8,     // input samples [keep, n_total) of every row, rows back to back: [batch][n_total - keep] float
    SNAP_ORIGIN = 9      // the rows' frame origins [batch] int32: in every snapshot of an engine with SE_CFG_STREAM_ROW_ORIGINS, the
                         // last segment in front of the window, and in no other
};
constexpr int32_t SNAP_KIND_MAX = SNAP_ORIGIN;
constexpr int32_t SNAP_FLAG_ROW_ORIGINS = 1 << 19;      // SE_CFG_STREAM_ROW_ORIGINS (include/se_engine.h; the engine asserts the two agree)

struct SnapSeg {
    int32_t kind = 0, index = 0;
    int64_t bytes = 0;
};

struct SnapManifest {
    // the engine the stream ran on: what a restore compares
    int32_t model = 0, flags = 0, n_fft = 0, hop = 0, win = 0;
    float p_in = 1.f, p_out = 1.f;
    // Stream's counters and modes; keep = the absolute sample the saved window starts at (a multiple of 4)
    int32_t batch = 0, max_chunk = 0, n_total = 0, t_done = 0, o_done = 0, keep = 0, running = 0, ring = 0;
    int32_t first = 1;       // StreamState::first
    int32_t state_B = 0;     // rows the model's state was made for (0: none yet)
    int32_t reserved[4] = {0, 0, 0, 0};
    std::vector<SnapSeg> segs;
};

constexpr uint32_t SNAP_MAGIC = 0x54534553u;      // "SEST"
constexpr uint32_t SNAP_VERSION = 1;
constexpr int64_t SNAP_HEAD_BYTES = 8 + 18 * 4 + 8 + 8 + 8;
constexpr int64_t SNAP_SEG_BYTES = 16;
constexpr int32_t SNAP_MAX_SEGS = 1 << 16;
constexpr int64_t SNAP_MAX_BYTES = (int64_t)1 << 40;

inline int64_t snap_align16(int64_t n) { return (n + 15) & ~(int64_t)15; }
inline int64_t snap_payload_bytes(const SnapManifest& m) {
    int64_t n = 0;
    for (const SnapSeg& s : m.segs) n += snap_align16(s.bytes);
    return n;
}
// "" or why the origin segment of m is not where the flags of m put it: one segment [batch] int32 right in front of the window
// with SNAP_FLAG_ROW_ORIGINS, none without
inline std::string snap_origin_why(const SnapManifest& m) {
    const bool want = (m.flags & SNAP_FLAG_ROW_ORIGINS) != 0;
    int n = 0;
    for (size_t k = 0; k < m.segs.size(); ++k) {
        if (m.segs[k].kind != SNAP_ORIGIN) continue;
        ++n;
        if (!want) return "a frame origin segment in a snapshot of an engine without SE_CFG_STREAM_ROW_ORIGINS";
        if (m.segs[k].index != 0 || m.segs[k].bytes != (int64_t)m.batch * 4)
            return "frame origin segment of " + std::to_string(m.segs[k].bytes) + " bytes, " + std::to_string(m.batch) + " rows keep " +
                   std::to_string((int64_t)m.batch * 4);
        if (k + 2 != m.segs.size() || m.segs.back().kind != SNAP_WINDOW) return "frame origin segment misplaced (it goes right in front of the input window)";
    }
    if (n > 1) return "more than one frame origin segment";
    if (want && n == 0) return "no frame origin segment in a snapshot of an engine with SE_CFG_STREAM_ROW_ORIGINS";
    return "";
}

inline int64_t snap_table_bytes(const SnapManifest& m) { return SNAP_HEAD_BYTES + SNAP_SEG_BYTES * (int64_t)m.segs.size(); }
inline int64_t snap_image_bytes(const SnapManifest& m) { return snap_table_bytes(m) + snap_payload_bytes(m); }

namespace snap_detail {
template <typename T>
inline void put(uint8_t*& p, T v) {
    std::memcpy(p, &v, sizeof(T));
    p += sizeof(T);
}
template <typename T>
inline T get(const uint8_t*& p) {
    T v;
    std::memcpy(&v, p, sizeof(T));
    p += sizeof(T);
    return v;
}
}  // namespace snap_detail

// header + segment table into out[0, snap_table_bytes(m)); the payload follows it
inline void snap_write_table(const SnapManifest& m, uint8_t* out) {
    using snap_detail::put;
    uint8_t* p = out;
    put<uint32_t>(p, SNAP_MAGIC);
    put<uint32_t>(p, SNAP_VERSION);
    const int32_t f[18] = {m.model,  m.flags,  m.n_fft, m.hop,     m.win,  m.batch, m.max_chunk,   m.n_total,     m.t_done,
                           m.o_done, m.keep,   m.running, m.ring,  m.first, m.state_B, m.reserved[0], m.reserved[1], m.reserved[2]};
    for (int32_t v : f) put<int32_t>(p, v);
    put<float>(p, m.p_in);
    put<float>(p, m.p_out);
    put<int32_t>(p, (int32_t)m.segs.size());
    put<int32_t>(p, 0);
    put<int64_t>(p, snap_payload_bytes(m));
    for (const SnapSeg& s : m.segs) {
        put<int32_t>(p, s.kind);
        put<int32_t>(p, s.index);
        put<int64_t>(p, s.bytes);
    }
}

// Parses and validates an image of `bytes` bytes.  Returns "" and fills m / payload_off, or the reason the image is refused (m is
// then unspecified; the caller parses into a scratch record).
inline std::string snap_parse(const void* buf, int64_t bytes, SnapManifest& m, int64_t& payload_off) {
    using snap_detail::get;
    if (!buf || bytes < 8) return "stream state image: truncated (shorter than its magic and version)";
    const uint8_t* p = static_cast<const uint8_t*>(buf);
    if (get<uint32_t>(p) != SNAP_MAGIC) return "stream state image: bad magic (not written by se_stream_state_export)";
    const uint32_t ver = get<uint32_t>(p);
    if (ver != SNAP_VERSION) return "stream state image: version " + std::to_string(ver) + ", this library reads version " + std::to_string(SNAP_VERSION);
    if (bytes < SNAP_HEAD_BYTES) return "stream state image: truncated (header cut short)";
    int32_t f[18];
    for (int32_t& v : f) v = get<int32_t>(p);
    m = SnapManifest();
    m.model = f[0]; m.flags = f[1]; m.n_fft = f[2]; m.hop = f[3]; m.win = f[4]; m.batch = f[5]; m.max_chunk = f[6];
    m.n_total = f[7]; m.t_done = f[8]; m.o_done = f[9]; m.keep = f[10]; m.running = f[11]; m.ring = f[12]; m.first = f[13];
    m.state_B = f[14]; m.reserved[0] = f[15]; m.reserved[1] = f[16]; m.reserved[2] = f[17];
    m.p_in = get<float>(p);
    m.p_out = get<float>(p);
    const int32_t nseg = get<int32_t>(p);
    (void)get<int32_t>(p);
    const int64_t total = get<int64_t>(p);
    if (nseg < 0 || nseg > SNAP_MAX_SEGS) return "stream state image: segment count " + std::to_string(nseg) + " out of range";
    if (total < 0 || total > SNAP_MAX_BYTES) return "stream state image: payload size negative or overflowing";
    const int64_t table = SNAP_HEAD_BYTES + SNAP_SEG_BYTES * (int64_t)nseg;
    if (bytes < table) return "stream state image: truncated (segment table cut short)";
    int64_t sum = 0;
    m.segs.resize((size_t)nseg);
    for (int32_t k = 0; k < nseg; ++k) {
        SnapSeg& s = m.segs[(size_t)k];
        s.kind = get<int32_t>(p);
        s.index = get<int32_t>(p);
        s.bytes = get<int64_t>(p);
        if (s.kind < SNAP_C || s.kind > SNAP_KIND_MAX || s.index < 0)
            return "stream state image: segment " + std::to_string(k) + " of unknown kind";
        if (s.bytes < 0 || s.bytes > SNAP_MAX_BYTES || (s.bytes & 3))
            return "stream state image: segment " + std::to_string(k) + " has a negative, overflowing or odd size";
        sum += snap_align16(s.bytes);
        if (sum > SNAP_MAX_BYTES) return "stream state image: segment sizes overflow";
    }
    if (sum != total)
        return "stream state image: segment table sizes add up to " + std::to_string(sum) + " bytes, the payload is recorded as " +
               std::to_string(total);
    if (bytes < table + total)
        return "stream state image: truncated (" + std::to_string(bytes) + " bytes, the manifest describes " + std::to_string(table + total) + ")";
    if (bytes > table + total)
        return "stream state image: " + std::to_string(bytes - table - total) + " trailing bytes behind the payload";
    if (m.batch < 1 || m.max_chunk < 1 || m.n_total < 0 || m.t_done < 0 || m.o_done < 0 || m.keep < 0 || m.keep > m.n_total ||
        (m.keep & 3) || m.ring < 0 || m.state_B < 0)
        return "stream state image: stream counters out of range";
    for (int32_t k = 0; k < nseg; ++k)
        if (m.segs[(size_t)k].kind == SNAP_WINDOW && (k != nseg - 1 || m.segs[(size_t)k].bytes != (int64_t)m.batch * (m.n_total - m.keep) * 4))
            return "stream state image: input window segment misplaced or of the wrong size";
    const std::string org = snap_origin_why(m);
    if (!org.empty()) return "stream state image: " + org;
    payload_off = table;
    return "";
}

}  // namespace se

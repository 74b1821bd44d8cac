// The host record of a parked StreamResampler signal (se_resampler_save / se_resampler_restore, include/se_engine.h) and its host
// image: host code alone, no device runtime - k_resample includes it, and so does a stand-alone check program
// (tests/resampler_manifest_check.cpp).
//
// A snapshot is this record + one payload: the live history, samples [w0, n_total) of every row, rows back to back - at most
// 2 * reach floats per row (resample_pos.h).  Which of the object's two history buffers was current, the pinned position ring and
// the filter table are not part of it: a push's read positions are re-derived from (t, acc), the table from the rates.  A
// pass-through object (sr_in == sr_out) keeps no history: its record has w0 == n_total and no payload.
//
// Host image (se_resampler_state_export / _import), little endian as the hosts this runs on, RSNAP_HEAD_BYTES + payload:
//   u32 magic 'SERS' | u32 version | i32 sr_in | i32 sr_out | i32 batch | i32 0
//   i64 n_total | i64 w0 | i64 t | 8 bytes: the double acc as it lies in memory | i64 payload bytes
//   payload: batch rows of n_total - w0 floats
#pragma once
#include "resample_pos.h"
#include <cstdint>
#include <cstring>
#include <string>

namespace se {

struct ResamplerManifest {
    int32_t sr_in = 0, sr_out = 0, batch = 0;
    int64_t n_total = 0;     // input samples arrived
    int64_t w0 = 0;          // first sample of the history
    int64_t t = 0;           // next output sample
    uint64_t acc_bits = 0;   // the running read position (ResamplePos::acc), bit for bit
};

constexpr uint32_t RSNAP_MAGIC = 0x53524553u;     // "SERS"
constexpr uint32_t RSNAP_VERSION = 1;
constexpr int64_t RSNAP_HEAD_BYTES = 8 + 4 * 4 + 5 * 8;
constexpr int64_t RSNAP_MAX_COUNT = 2147483647;   // the samples, in or out, se_resample accepts
constexpr int64_t RSNAP_MAX_BYTES = (int64_t)1 << 40;

inline uint64_t rsnap_bits_of(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}
inline double rsnap_double_of(uint64_t b) {
    double v;
    std::memcpy(&v, &b, 8);
    return v;
}

inline int64_t rsnap_keep(const ResamplerManifest& m) { return m.n_total - m.w0; }
inline int64_t rsnap_payload_bytes(const ResamplerManifest& m) { return (int64_t)m.batch * rsnap_keep(m) * 4; }
inline int64_t rsnap_image_bytes(const ResamplerManifest& m) { return RSNAP_HEAD_BYTES + rsnap_payload_bytes(m); }

namespace rsnap_detail {
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
}  // namespace rsnap_detail

// Why a record cannot be one a save wrote ("" when it can): the counters alone, no image around them
inline std::string rsnap_check(const ResamplerManifest& m) {
    const std::string pre = "resampler state image: ";
    if (m.sr_in <= 0 || m.sr_out <= 0 || m.batch < 1) return pre + "rates or batch out of range";
    const double acc = rsnap_double_of(m.acc_bits);
    if (m.n_total < 0 || m.w0 < 0 || m.t < 0 || !(acc >= 0.0))
        return pre + "negative counters";
    if (m.n_total > RSNAP_MAX_COUNT || m.t > RSNAP_MAX_COUNT || !(acc <= (double)RSNAP_MAX_COUNT))
        return pre + "overflowing counters";
    if (m.w0 > m.n_total)
        return pre + "the history starts at sample " + std::to_string(m.w0) + ", behind the " + std::to_string(m.n_total) + " samples that have arrived";
    const int64_t keep = rsnap_keep(m);
    if (m.sr_in == m.sr_out) {
        if (keep != 0) return pre + "a pass-through signal (sr_in == sr_out) with a history";
        return "";
    }
    const ResamplePlan p = resample_plan(m.sr_in, m.sr_out);
    if (p.index_step <= 0) return pre + "sr_out / sr_in below the table's resolution";
    if (keep > 2 * (int64_t)p.reach)
        return pre + "a history of " + std::to_string(keep) + " samples per row, more than 2 * reach = " + std::to_string(2 * (int64_t)p.reach) +
               " of " + std::to_string(m.sr_in) + " -> " + std::to_string(m.sr_out) + " Hz";
    return "";
}

// ---- rows of parked signals (se_resampler_state_select / _concat): the payload is [batch][n_total - w0] floats
// "" or why `rows` cannot pick rows of a state of `batch` rows
inline std::string rsnap_rows_check(const int32_t* rows, int32_t n_rows, int32_t batch) {
    if (n_rows < 1) return "n_rows " + std::to_string(n_rows) + ": at least one row has to be selected";
    if (!rows) return "null row list";
    for (int32_t j = 0; j < n_rows; ++j)
        if (rows[j] < 0 || rows[j] >= batch)
            return "rows[" + std::to_string(j) + "] = " + std::to_string(rows[j]) + " outside 0 .. " + std::to_string(batch - 1);
    return "";
}
// "" or the first field in which two parts of a concat differ: everything except the batch has to agree
inline std::string rsnap_concat_differs(const ResamplerManifest& a, const ResamplerManifest& b) {
    auto ne = [](const char* name, int64_t x, int64_t y) { return std::string(name) + " " + std::to_string(x) + " vs " + std::to_string(y); };
    if (a.sr_in != b.sr_in) return ne("sr_in", a.sr_in, b.sr_in);
    if (a.sr_out != b.sr_out) return ne("sr_out", a.sr_out, b.sr_out);
    if (a.n_total != b.n_total) return ne("n_in", a.n_total, b.n_total);
    if (a.t != b.t) return ne("n_out", a.t, b.t);
    if (a.w0 != b.w0) return ne("w0", a.w0, b.w0);
    if (a.acc_bits != b.acc_bits)
        return "read position " + std::to_string(rsnap_double_of(a.acc_bits)) + " vs " + std::to_string(rsnap_double_of(b.acc_bits)) + " (bits differ)";
    return "";
}

// the header into out[0, RSNAP_HEAD_BYTES); the payload follows it
inline void rsnap_write_head(const ResamplerManifest& m, uint8_t* out) {
    using rsnap_detail::put;
    uint8_t* p = out;
    put<uint32_t>(p, RSNAP_MAGIC);
    put<uint32_t>(p, RSNAP_VERSION);
    put<int32_t>(p, m.sr_in);
    put<int32_t>(p, m.sr_out);
    put<int32_t>(p, m.batch);
    put<int32_t>(p, 0);
    put<int64_t>(p, m.n_total);
    put<int64_t>(p, m.w0);
    put<int64_t>(p, m.t);
    put<uint64_t>(p, m.acc_bits);
    put<int64_t>(p, rsnap_payload_bytes(m));
}

// Parses and validates an image of `bytes` bytes.  Returns "" and fills m / payload_off, or the reason the image is refused (m is
// then unspecified; the caller parses into a scratch record).
inline std::string rsnap_parse(const void* buf, int64_t bytes, ResamplerManifest& m, int64_t& payload_off) {
    using rsnap_detail::get;
    const std::string pre = "resampler state image: ";
    if (!buf || bytes < 8) return pre + "truncated (shorter than its magic and version)";
    const uint8_t* p = static_cast<const uint8_t*>(buf);
    if (get<uint32_t>(p) != RSNAP_MAGIC) return pre + "bad magic (not written by se_resampler_state_export)";
    const uint32_t ver = get<uint32_t>(p);
    if (ver != RSNAP_VERSION) return pre + "version " + std::to_string(ver) + ", this library reads version " + std::to_string(RSNAP_VERSION);
    if (bytes < RSNAP_HEAD_BYTES) return pre + "truncated (header cut short)";
    m = ResamplerManifest();
    m.sr_in = get<int32_t>(p);
    m.sr_out = get<int32_t>(p);
    m.batch = get<int32_t>(p);
    (void)get<int32_t>(p);
    m.n_total = get<int64_t>(p);
    m.w0 = get<int64_t>(p);
    m.t = get<int64_t>(p);
    m.acc_bits = get<uint64_t>(p);
    const int64_t total = get<int64_t>(p);
    if (total < 0 || total > RSNAP_MAX_BYTES) return pre + "payload size negative or overflowing";
    const std::string why = rsnap_check(m);
    if (!why.empty()) return why;
    if (total != rsnap_payload_bytes(m))
        return pre + "the payload is recorded as " + std::to_string(total) + " bytes, batch * (n_total - w0) * 4 is " +
               std::to_string(rsnap_payload_bytes(m));
    if (bytes < RSNAP_HEAD_BYTES + total)
        return pre + "truncated (" + std::to_string(bytes) + " bytes, the header describes " + std::to_string(RSNAP_HEAD_BYTES + total) + ")";
    if (bytes > RSNAP_HEAD_BYTES + total)
        return pre + std::to_string(bytes - RSNAP_HEAD_BYTES - total) + " trailing bytes behind the payload";
    payload_off = RSNAP_HEAD_BYTES;
    return "";
}

}  // namespace se

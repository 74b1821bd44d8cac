// Stand-alone host program over stream_manifest.h, meant for `-fsanitize=address,undefined` (make stream_manifest_check): no
// device code, not loaded into anything.  It writes the host image of snapshots with 0, 1 and 300 segments into buffers of exactly
// the image's size (so that a write or a read past either end is the sanitizer's to report), parses them back and compares every
// field, and feeds the parser the malformed images se_stream_state_import has to refuse - each has to be refused for the defect
// it has.  Exit status 0 and "ok" when everything holds.
#include "../stream_manifest.h"
#include <algorithm>
#include <climits>
#include <cstdio>
#include <memory>

using namespace se;

static int failures = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("line %d: %s\n", __LINE__, #c);                  \
            ++failures;                                                  \
        }                                                                \
    } while (0)

static SnapManifest make(int nseg) {
    SnapManifest m;
    m.model = 5; m.flags = 1 << 16; m.n_fft = 512; m.hop = 128; m.win = 512; m.p_in = 0.5f; m.p_out = 2.f;
    m.batch = 2; m.max_chunk = 16; m.n_total = 3700; m.t_done = 26; m.o_done = 3000; m.keep = 3072; m.running = 1; m.ring = 128;
    m.first = 0; m.state_B = 2;
    for (int k = 0; k < nseg; ++k) {
        SnapSeg s;
        const bool last = k == nseg - 1;
        s.kind = last ? SNAP_WINDOW : (k % 2 ? SNAP_SLOT : SNAP_HIST);
        s.index = last ? 0 : k;
        s.bytes = last ? (int64_t)m.batch * (m.n_total - m.keep) * 4 : 4 * (int64_t)((k * 37) % 19);      // sizes 0, 4, ... no multiple of 16
        m.segs.push_back(s);
    }
    return m;
}

// a heap buffer of exactly n bytes
static std::unique_ptr<uint8_t[]> image_of(const SnapManifest& m, int64_t& n) {
    n = snap_image_bytes(m);
    std::unique_ptr<uint8_t[]> buf(new uint8_t[(size_t)n]);
    snap_write_table(m, buf.get());
    for (int64_t i = snap_table_bytes(m); i < n; ++i) buf[(size_t)i] = (uint8_t)(i * 7);
    return buf;
}

static bool refused(const uint8_t* p, int64_t n, const char* word) {
    SnapManifest m;
    int64_t off = -1;
    const std::string why = snap_parse(p, n, m, off);
    if (why.find(word) == std::string::npos) std::printf("  got '%s', wanted '%s'\n", why.c_str(), word);
    return !why.empty() && why.find(word) != std::string::npos;
}

int main() {
    for (int nseg : {0, 1, 300}) {
        const SnapManifest m = make(nseg);
        int64_t n = 0;
        const auto buf = image_of(m, n);
        EXPECT(n == SNAP_HEAD_BYTES + 16 * (int64_t)nseg + snap_payload_bytes(m));
        SnapManifest r;
        int64_t off = -1;
        const std::string why = snap_parse(buf.get(), n, r, off);
        EXPECT(why.empty());
        EXPECT(off == snap_table_bytes(m));
        EXPECT(r.model == m.model && r.flags == m.flags && r.n_fft == m.n_fft && r.hop == m.hop && r.win == m.win);
        EXPECT(r.p_in == m.p_in && r.p_out == m.p_out && r.batch == m.batch && r.max_chunk == m.max_chunk);
        EXPECT(r.n_total == m.n_total && r.t_done == m.t_done && r.o_done == m.o_done && r.keep == m.keep);
        EXPECT(r.running == m.running && r.ring == m.ring && r.first == m.first && r.state_B == m.state_B);
        EXPECT(r.segs.size() == m.segs.size());
        for (size_t k = 0; k < r.segs.size() && k < m.segs.size(); ++k)
            EXPECT(r.segs[k].kind == m.segs[k].kind && r.segs[k].index == m.segs[k].index && r.segs[k].bytes == m.segs[k].bytes);
        // 16 B aligned offsets
        int64_t o = 0;
        for (const SnapSeg& s : m.segs) {
            EXPECT((o & 15) == 0);
            o += snap_align16(s.bytes);
        }
        EXPECT(o == snap_payload_bytes(m));

        // cut short at every length below the whole: each in a buffer of its own exact size
        for (int64_t cut : {(int64_t)0, (int64_t)3, (int64_t)8, SNAP_HEAD_BYTES - 1, SNAP_HEAD_BYTES, snap_table_bytes(m) - 1, n - 1}) {
            if (cut < 0 || cut >= n) continue;
            std::unique_ptr<uint8_t[]> part(new uint8_t[(size_t)std::max<int64_t>(cut, 1)]);
            std::memcpy(part.get(), buf.get(), (size_t)cut);
            EXPECT(refused(part.get(), cut, "truncated"));
        }
        // trailing bytes
        {
            std::unique_ptr<uint8_t[]> more(new uint8_t[(size_t)n + 5]);
            std::memcpy(more.get(), buf.get(), (size_t)n);
            std::memset(more.get() + n, 0, 5);
            EXPECT(refused(more.get(), n + 5, "trailing"));
        }
        // garbage, wrong version
        {
            std::unique_ptr<uint8_t[]> g(new uint8_t[(size_t)n]);
            for (int64_t i = 0; i < n; ++i) g[(size_t)i] = (uint8_t)(0xA5 ^ i);
            EXPECT(refused(g.get(), n, "magic"));
            std::memcpy(g.get(), buf.get(), (size_t)n);
            g[4] = 9;
            EXPECT(refused(g.get(), n, "version"));
        }
        if (nseg > 0) {
            auto with = [&](int64_t pos, int64_t value) {
                std::unique_ptr<uint8_t[]> g(new uint8_t[(size_t)n]);
                std::memcpy(g.get(), buf.get(), (size_t)n);
                std::memcpy(g.get() + pos, &value, 8);
                return g;
            };
            const int64_t size0 = SNAP_HEAD_BYTES + 8;      // the first segment's size field
            EXPECT(refused(with(size0, m.segs[0].bytes + 64).get(), n, "add up"));             // one size enlarged
            EXPECT(refused(with(size0, -16).get(), n, "negative"));
            EXPECT(refused(with(size0, INT64_MAX - 7).get(), n, "overflowing"));
            EXPECT(refused(with(SNAP_HEAD_BYTES - 8, -1).get(), n, "negative or overflowing"));  // the payload total
            // a segment count that would run the table past the image
            std::unique_ptr<uint8_t[]> g(new uint8_t[(size_t)n]);
            std::memcpy(g.get(), buf.get(), (size_t)n);
            const int32_t many = 60000;
            std::memcpy(g.get() + SNAP_HEAD_BYTES - 16, &many, 4);
            EXPECT(refused(g.get(), n, nseg * 16 + SNAP_HEAD_BYTES + snap_payload_bytes(m) < SNAP_HEAD_BYTES + 16 * (int64_t)many ? "truncated" : "add up"));
            const int32_t neg = -1;
            std::memcpy(g.get() + SNAP_HEAD_BYTES - 16, &neg, 4);
            EXPECT(refused(g.get(), n, "segment count"));
        }
    }
    EXPECT(refused(nullptr, 100, "truncated"));
    if (failures == 0) std::printf("ok\n");
    return failures ? 1 : 0;
}

// Stand-alone host program over stream_rows.h and the row functions of resampler_manifest.h, meant for
// `-fsanitize=address,undefined` (make stream_select_check): no device code, not loaded into anything.  The layout arithmetic of
// se_stream_state_select / _concat as pure functions: the scaled segment sizes and payload offsets of a result, for a hand-written
// manifest with all eight segment kinds, a reference gather over host buffers written out index by index, and every refusal that
// needs no device - each has to be refused for the defect it has.  Exit status 0 and "ok" when everything holds.
#include "../resampler_manifest.h"
#include "../stream_rows.h"
#include <cstdio>

using namespace se;

static int failures = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("line %d: %s\n", __LINE__, #c);                  \
            ++failures;                                                  \
        }                                                                \
    } while (0)

static bool has(const std::string& why, const char* word) {
    if (why.find(word) == std::string::npos) std::printf("  got '%s', wanted '%s'\n", why.c_str(), word);
    return why.find(word) != std::string::npos;
}

// a group of B rows of a running-scale stream: c, sumsq, frame_inv, two histories, (h, c) of one layer, a slot, the window
static SnapManifest make(int B, std::vector<RowLayout>& lay) {
    SnapManifest m;
    m.model = 5; m.flags = 1 << 16; m.n_fft = 512; m.hop = 128; m.win = 512; m.p_in = 0.5f; m.p_out = 2.f;
    m.batch = B; m.max_chunk = 16; m.n_total = 3701; m.t_done = 26; m.o_done = 3000; m.keep = 3072; m.running = 1; m.ring = 128;
    m.first = 0; m.state_B = B;
    const int kinds[9] = {SNAP_C, SNAP_SUMSQ, SNAP_FRAME_INV, SNAP_HIST, SNAP_HIST, SNAP_H, SNAP_CELL, SNAP_SLOT, SNAP_WINDOW};
    const int index[9] = {0, 0, 0, 0, 1, 0, 0, 0, 0};
    const RowLayout model_lay[9] = {{}, {}, {}, {1, 7 * 12}, {1, 5}, {2 * 128 * 2, 1}, {256, 1}, {1, 4}, {}};
    lay.clear();
    for (int k = 0; k < 9; ++k) {
        SnapSeg s;
        s.kind = kinds[k];
        s.index = index[k];
        RowLayout l;
        if (!snap_engine_layout(m, s, l)) l = model_lay[k];
        s.bytes = l.outer * B * l.inner * 4;
        m.segs.push_back(s);
        lay.push_back(l);
    }
    return m;
}

// payload of m whose float at (segment k, o, b, i) encodes (k, o, tag of row b, i); exactly snap_payload_bytes(m) long, padding = -1
static std::vector<float> fill(const SnapManifest& m, const std::vector<RowLayout>& lay, const std::vector<int>& tags) {
    std::vector<float> pay((size_t)(snap_payload_bytes(m) / 4), -1.f);
    const std::vector<int64_t> off = snap_offsets(m);
    for (size_t k = 0; k < m.segs.size(); ++k)
        for (int64_t o = 0; o < lay[k].outer; ++o)
            for (int b = 0; b < m.batch; ++b)
                for (int64_t i = 0; i < lay[k].inner; ++i)
                    pay[(size_t)(off[k] / 4 + (o * m.batch + b) * lay[k].inner + i)] = (float)(((k * 37 + o) * 11 + tags[(size_t)b]) * 13 + i % 13);
    return pay;
}

int main() {
    std::vector<RowLayout> lay;
    const SnapManifest src = make(4, lay);
    EXPECT(snap_layout_check(src, lay).empty());
    // the window's layout follows the counters: 3701 - 3072 = 629 live samples, no multiple of 4
    EXPECT(lay.back().outer == 1 && lay.back().inner == 629 && src.segs.back().bytes == 4 * 629 * 4);
    EXPECT(lay[1].inner == 2 && src.segs[1].bytes == 4 * 8);           // sumsq: doubles as two floats per row
    EXPECT(lay[2].inner == 128);

    // ---- select: sizes scale with the rows, everything else is copied, offsets stay 16 B aligned
    for (int n : {1, 2, 3, 4, 7}) {
        const SnapManifest d = snap_rows_manifest(src, lay, n);
        EXPECT(d.batch == n && d.state_B == n);
        EXPECT(d.n_total == src.n_total && d.t_done == src.t_done && d.o_done == src.o_done && d.keep == src.keep && d.running == src.running &&
               d.ring == src.ring && d.first == src.first && d.max_chunk == src.max_chunk && d.model == src.model && d.flags == src.flags);
        EXPECT(d.segs.size() == src.segs.size());
        int64_t sum = 0;
        const std::vector<int64_t> off = snap_offsets(d);
        for (size_t k = 0; k < d.segs.size(); ++k) {
            EXPECT(d.segs[k].kind == src.segs[k].kind && d.segs[k].index == src.segs[k].index);
            EXPECT(d.segs[k].bytes * 4 == src.segs[k].bytes * n);
            EXPECT(off[k] == sum && (off[k] & 15) == 0);
            sum += snap_align16(d.segs[k].bytes);
        }
        EXPECT(sum == snap_payload_bytes(d));
        EXPECT(snap_layout_check(d, lay).empty());
        EXPECT(snap_concat_differs(src, d).empty());                   // rows of one group: a select and its source may be joined
        // the manifest survives the host image
        std::vector<uint8_t> img((size_t)snap_image_bytes(d), 0);
        snap_write_table(d, img.data());
        SnapManifest r;
        int64_t po = -1;
        EXPECT(snap_parse(img.data(), (int64_t)img.size(), r, po).empty() && po == snap_table_bytes(d) && r.batch == n);
    }
    {   // a snapshot from before the first frame: engine-level segments only
        SnapManifest e0 = src;
        std::vector<RowLayout> l0;
        e0.state_B = 0;
        e0.segs.clear();
        for (size_t k = 0; k < src.segs.size(); ++k)
            if (src.segs[k].kind < SNAP_HIST || src.segs[k].kind == SNAP_WINDOW) {
                e0.segs.push_back(src.segs[k]);
                l0.push_back(lay[k]);
            }
        EXPECT(snap_layout_check(e0, l0).empty());
        const SnapManifest d = snap_rows_manifest(e0, l0, 1);
        EXPECT(d.state_B == 0 && d.batch == 1 && d.segs.size() == 4 && d.segs.back().bytes == 629 * 4);
        EXPECT(has(snap_concat_differs(src, e0), "state_B"));
    }

    // ---- the gather the kernel performs, written out index by index on host payloads: select [3, 1, 1] of rows tagged 0..3
    {
        const std::vector<int> tags = {0, 1, 2, 3}, pick = {3, 1, 1};
        const std::vector<float> sp = fill(src, lay, tags);
        const SnapManifest d = snap_rows_manifest(src, lay, 3);
        std::vector<float> dp((size_t)(snap_payload_bytes(d) / 4), -1.f);
        const std::vector<int64_t> so = snap_offsets(src), dof = snap_offsets(d);
        for (size_t k = 0; k < d.segs.size(); ++k)
            for (int64_t o = 0; o < lay[k].outer; ++o)
                for (int b = 0; b < 3; ++b)
                    for (int64_t i = 0; i < lay[k].inner; ++i)
                        dp[(size_t)(dof[k] / 4 + (o * 3 + b) * lay[k].inner + i)] = sp[(size_t)(so[k] / 4 + (o * 4 + pick[(size_t)b]) * lay[k].inner + i)];
        EXPECT(dp == fill(d, lay, pick));          // the payload of a group whose rows ARE 3, 1, 1 - padding untouched
    }

    // ---- refusals
    const int32_t ok_rows[3] = {3, 0, 3}, bad_hi[2] = {0, 4}, bad_lo[2] = {-1, 0};
    EXPECT(snap_rows_check(ok_rows, 3, 4).empty());
    EXPECT(has(snap_rows_check(bad_hi, 2, 4), "rows[1] = 4 outside 0 .. 3"));
    EXPECT(has(snap_rows_check(bad_lo, 2, 4), "rows[0] = -1 outside 0 .. 3"));
    EXPECT(has(snap_rows_check(ok_rows, 0, 4), "n_rows 0"));
    EXPECT(has(snap_rows_check(ok_rows, -2, 4), "n_rows -2"));
    EXPECT(has(snap_rows_check(nullptr, 1, 4), "null"));
    {   // a segment that does not have the size its layout describes; a buffer without a layout; a state made for other rows
        SnapManifest m = src;
        m.segs[3].bytes += 16;
        EXPECT(has(snap_layout_check(m, lay), "segment hist[0]"));
        std::vector<RowLayout> l2 = lay;
        l2[5] = RowLayout();
        EXPECT(has(snap_layout_check(src, l2), "segment h[0] has no row layout"));
        l2.pop_back();
        EXPECT(has(snap_layout_check(src, l2), "layouts for 8 segments"));
        m = src;
        m.state_B = 3;
        EXPECT(has(snap_layout_check(m, lay), "made for 3 rows"));
    }
    {   // parts that differ in each single field, named
        std::vector<RowLayout> l2;
        const SnapManifest other = make(2, l2);
        EXPECT(snap_concat_differs(src, other).empty());
        struct Case { const char* want; void (*mutate)(SnapManifest&); };
        const Case cases[] = {
            {"model 5 vs 6", [](SnapManifest& m) { m.model = 6; }},
            {"flags 65536 vs 0", [](SnapManifest& m) { m.flags = 0; }},
            {"n_fft 512 vs 320", [](SnapManifest& m) { m.n_fft = 320; }},
            {"hop 128 vs 160", [](SnapManifest& m) { m.hop = 160; }},
            {"win 512 vs 400", [](SnapManifest& m) { m.win = 400; }},
            {"max_chunk 16 vs 8", [](SnapManifest& m) { m.max_chunk = 8; }},
            {"n_total 3701 vs 3541", [](SnapManifest& m) { m.n_total = 3541; }},
            {"t_done 26 vs 25", [](SnapManifest& m) { m.t_done = 25; }},
            {"o_done 3000 vs 2872", [](SnapManifest& m) { m.o_done = 2872; }},
            {"keep 3072 vs 2944", [](SnapManifest& m) { m.keep = 2944; }},
            {"running 1 vs 0", [](SnapManifest& m) { m.running = 0; }},
            {"ring 128 vs 256", [](SnapManifest& m) { m.ring = 256; }},
            {"first 0 vs 1", [](SnapManifest& m) { m.first = 1; }},
            {"p_in 0.5", [](SnapManifest& m) { m.p_in = 1.f; }},
            {"p_out 2.0", [](SnapManifest& m) { m.p_out = 1.f; }},
            {"segment count 9 vs 8", [](SnapManifest& m) { m.segs.erase(m.segs.begin() + 4); }},
            {"segment 7 slot[0] vs slot[1]", [](SnapManifest& m) { m.segs[7].index = 1; }},
        };
        for (const Case& c : cases) {
            SnapManifest m = other;
            c.mutate(m);
            EXPECT(has(snap_concat_differs(src, m), c.want));
        }
    }

    // ---- the resampler's half: [batch][n_total - w0] floats
    {
        ResamplerManifest a;
        a.sr_in = 48000; a.sr_out = 16000; a.batch = 3; a.n_total = 5000; a.w0 = 4700; a.t = 1500; a.acc_bits = rsnap_bits_of(4500.25);
        ResamplerManifest b = a;
        b.batch = 1;
        EXPECT(rsnap_concat_differs(a, b).empty());
        b = a; b.sr_in = 44100; EXPECT(has(rsnap_concat_differs(a, b), "sr_in 48000 vs 44100"));
        b = a; b.sr_out = 8000; EXPECT(has(rsnap_concat_differs(a, b), "sr_out 16000 vs 8000"));
        b = a; b.n_total = 5001; EXPECT(has(rsnap_concat_differs(a, b), "n_in 5000 vs 5001"));
        b = a; b.t = 1501; EXPECT(has(rsnap_concat_differs(a, b), "n_out 1500 vs 1501"));
        b = a; b.w0 = 4699; EXPECT(has(rsnap_concat_differs(a, b), "w0 4700 vs 4699"));
        b = a; b.acc_bits ^= 1; EXPECT(has(rsnap_concat_differs(a, b), "read position"));
        EXPECT(has(rsnap_rows_check(bad_hi, 2, 3), "rows[1] = 4 outside 0 .. 2"));
        EXPECT(has(rsnap_rows_check(ok_rows, 0, 3), "n_rows 0"));
        EXPECT(rsnap_rows_check(ok_rows + 1, 1, 3).empty());
    }
    if (failures == 0) std::printf("ok\n");
    return failures ? 1 : 0;
}

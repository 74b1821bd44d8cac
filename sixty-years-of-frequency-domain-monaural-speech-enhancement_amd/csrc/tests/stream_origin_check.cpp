// Stand-alone check of the host side of per-row frame origins (SE_CFG_STREAM_ROW_ORIGINS): the SNAP_ORIGIN segment in a manifest and
// its host image (stream_manifest.h), its row arithmetic in select, concat and join (stream_rows.h, stream_join.h), and the join plan of
// the models whose state counts frames.  Built with the host sanitizers (Makefile: stream_origin_check), run on a CPU; prints "ok" and
// returns 0, or the first failures and 1.
#include "../stream_join.h"
#include <cstdio>
#include <cstdlib>

using namespace se;

static int fails = 0;
#define EXPECT(cond, ...)                       \
    do {                                        \
        if (!(cond)) {                          \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);           \
            std::printf("\n");                  \
            if (++fails > 20) std::exit(1);     \
        }                                       \
    } while (0)

constexpr int BIT = SNAP_FLAG_ROW_ORIGINS;
// include/se_engine.h: SE_MODEL_FULLSUBNET, _CTSNET, _G2NET, _TAYLORSENET and SE_CFG_FSN_CUMULATIVE; the plan only compares them
constexpr int MODEL_FSN = 6, MODEL_CTS = 7, MODEL_G2 = 8, MODEL_TAYLOR = 9, FSN_CUM = 16;

// a stream of `model` after n_total samples: c, the model's state - two call-order slots for the cLN networks (none before the first
// chunk), history tensors and LSTM (h, c) for FullSubNet - the origins with the bit, the window
static SnapManifest stream(int model, int flags, int n_fft, int hop, int lag, int n_total, int batch) {
    SnapManifest m;
    m.model = model; m.flags = flags; m.n_fft = n_fft; m.hop = hop; m.win = n_fft;
    m.batch = batch; m.max_chunk = 16; m.n_total = n_total;
    m.t_done = n_total > n_fft / 2 ? (n_total - n_fft / 2 - 1) / hop + 1 : 0;
    m.o_done = std::max(0, std::min(n_total, (m.t_done - lag) * hop - n_fft / 2));
    m.keep = (int)(std::max<int64_t>(0, std::min<int64_t>((int64_t)m.t_done * hop - n_fft / 2, (int64_t)n_total - n_fft / 2 - 1)) & ~(int64_t)3);
    m.first = m.t_done > 0 ? 0 : 1;
    m.state_B = batch;
    auto seg = [&](int kind, int index, int64_t bytes) {
        SnapSeg s; s.kind = kind; s.index = index; s.bytes = bytes;
        m.segs.push_back(s);
    };
    seg(SNAP_C, 0, (int64_t)batch * 4);
    if (model == MODEL_FSN) {
        for (int i = 0; i < 4; ++i) seg(SNAP_HIST, i, (int64_t)batch * 4 * (i < 2 ? 2 * 257 * 8 : i == 2 ? 1 : 257));
        for (int l = 0; l < 4; ++l) {
            seg(SNAP_H, l, (int64_t)batch * 4 * (l < 2 ? 512 : 384 * 257));
            seg(SNAP_CELL, l, (int64_t)batch * 4 * (l < 2 ? 512 : 384 * 257));
        }
    } else if (m.t_done > 0) {
        seg(SNAP_SLOT, 0, (int64_t)batch * 16);
        seg(SNAP_SLOT, 1, (int64_t)batch * 4 * 1000);
    }
    if (flags & BIT) seg(SNAP_ORIGIN, 0, (int64_t)batch * 4);
    seg(SNAP_WINDOW, 0, (int64_t)batch * (n_total - m.keep) * 4);
    return m;
}

static std::vector<uint8_t> image(const SnapManifest& m) {
    std::vector<uint8_t> img((size_t)snap_image_bytes(m), 0);
    snap_write_table(m, img.data());
    return img;
}
static std::string parse(const SnapManifest& m, SnapManifest* out = nullptr) {
    const std::vector<uint8_t> img = image(m);
    SnapManifest got;
    int64_t off = -1;
    const std::string why = snap_parse(img.data(), (int64_t)img.size(), got, off);
    if (why.empty()) EXPECT(off == snap_table_bytes(m), "payload offset %lld", (long long)off);
    if (out) *out = got;
    return why;
}
static std::vector<RowLayout> layouts(const SnapManifest& m) {
    std::vector<RowLayout> lay(m.segs.size());
    for (size_t k = 0; k < m.segs.size(); ++k)
        if (!snap_engine_layout(m, m.segs[k], lay[k])) lay[k] = {1, m.segs[k].bytes / ((int64_t)m.state_B * 4)};      // a slot: [B][row]
    return lay;
}
static size_t origin_seg(const SnapManifest& m) {
    for (size_t k = 0; k < m.segs.size(); ++k)
        if (m.segs[k].kind == SNAP_ORIGIN) return k;
    return m.segs.size();
}

// what the gather does to the origin segment of the result: row bd <- row rowmap[bd].second of part rowmap[bd].first, + frames[part]
static std::vector<int32_t> gather(const std::vector<std::vector<int32_t>>& parts, const std::vector<std::pair<int, int>>& rowmap,
                                   const std::vector<int32_t>& frames) {
    std::vector<int32_t> out;
    for (const auto& r : rowmap) out.push_back(snap_join_origin(parts[(size_t)r.first][(size_t)r.second], frames[(size_t)r.first]));
    return out;
}

int main() {
    const int F = BIT | FSN_CUM;
    // ---- a manifest with the segment survives the host image, field by field
    {
        const SnapManifest m = stream(MODEL_CTS, BIT, 320, 160, 0, 4000, 3);
        SnapManifest got;
        const std::string why = parse(m, &got);
        EXPECT(why.empty(), "round trip refused: %s", why.c_str());
        EXPECT(got.flags == BIT && got.batch == 3 && got.segs.size() == m.segs.size(), "round trip: flags %d batch %d", got.flags, got.batch);
        const size_t k = origin_seg(got);
        EXPECT(k + 2 == got.segs.size() && got.segs[k].bytes == 12 && got.segs[k].index == 0, "origin segment at %zu of %zu", k, got.segs.size());
        EXPECT(std::string(snap_kind_name(SNAP_ORIGIN)) == "origin" && snap_seg_name(got.segs[k]) == "origin[0]", "segment name %s", snap_seg_name(got.segs[k]).c_str());
        EXPECT(snap_origin_why(m).empty(), "a well-formed manifest: %s", snap_origin_why(m).c_str());
        // before the first chunk: no slots yet, the origins are there all the same
        const SnapManifest early = stream(MODEL_G2, BIT, 320, 160, 0, 100, 2);
        EXPECT(early.t_done == 0 && early.segs.size() == 3 && parse(early).empty(), "a stream before its first chunk: %s", parse(early).c_str());
        // and without the bit nothing is new: the segment list of the parent's snapshots
        const SnapManifest plain = stream(MODEL_CTS, 0, 320, 160, 0, 4000, 3);
        EXPECT(origin_seg(plain) == plain.segs.size() && parse(plain).empty() && snap_image_bytes(plain) + 16 + 16 == snap_image_bytes(m),
               "a snapshot without the bit: %s", parse(plain).c_str());
    }
    // ---- refusals, each for the defect it has
    {
        SnapManifest m = stream(MODEL_TAYLOR, BIT, 320, 160, 0, 4000, 3);
        const size_t k = origin_seg(m);
        SnapManifest bad = m;
        bad.segs[k].bytes = 16;                                   // four rows' worth in a group of three
        EXPECT(parse(bad).find("frame origin segment of 16 bytes, 3 rows keep 12") != std::string::npos, "wrong size: %s", parse(bad).c_str());
        bad = m;
        bad.segs[k].bytes = 8;
        EXPECT(parse(bad).find("frame origin segment of 8 bytes") != std::string::npos, "short: %s", parse(bad).c_str());
        bad = m;
        std::swap(bad.segs[k], bad.segs[k + 1]);                  // behind the window
        EXPECT(!parse(bad).empty() && parse(bad).find("misplaced") != std::string::npos, "behind the window: %s", parse(bad).c_str());
        bad = m;
        std::swap(bad.segs[k], bad.segs[k - 1]);                  // in front of a slot
        EXPECT(parse(bad).find("frame origin segment misplaced") != std::string::npos, "in front of a slot: %s", parse(bad).c_str());
        bad = m;
        bad.segs.erase(bad.segs.begin() + (long)k);               // the bit without the segment
        EXPECT(parse(bad).find("no frame origin segment in a snapshot of an engine with SE_CFG_STREAM_ROW_ORIGINS") != std::string::npos, "lacking: %s",
               parse(bad).c_str());
        bad = m;
        bad.flags = 0;                                            // the segment without the bit
        EXPECT(parse(bad).find("a frame origin segment in a snapshot of an engine without SE_CFG_STREAM_ROW_ORIGINS") != std::string::npos, "carrying: %s",
               parse(bad).c_str());
        bad = m;
        bad.segs.insert(bad.segs.begin() + (long)k, bad.segs[k]);      // twice
        EXPECT(!parse(bad).empty(), "two origin segments accepted");
        bad = m;
        bad.segs[k].index = 1;
        EXPECT(!parse(bad).empty(), "origin[1] accepted");
    }
    // ---- rows: select and concat cut the segment like any [B][1] buffer
    {
        const SnapManifest m = stream(MODEL_CTS, BIT, 320, 160, 0, 4000, 3);
        const std::vector<RowLayout> lay = layouts(m);
        const size_t k = origin_seg(m);
        EXPECT(lay[k].outer == 1 && lay[k].inner == 1, "origin layout [%lld][B][%lld]", (long long)lay[k].outer, (long long)lay[k].inner);
        EXPECT(snap_layout_check(m, lay).empty(), "layouts: %s", snap_layout_check(m, lay).c_str());
        const SnapManifest one = snap_rows_manifest(m, lay, 1), five = snap_rows_manifest(m, lay, 5);
        EXPECT(one.segs[k].bytes == 4 && five.segs[k].bytes == 20 && snap_origin_why(one).empty() && snap_origin_why(five).empty(), "rows manifest: %lld %lld",
               (long long)one.segs[k].bytes, (long long)five.segs[k].bytes);
        EXPECT(parse(one).empty() && parse(five).empty(), "rows manifests do not parse: %s / %s", parse(one).c_str(), parse(five).c_str());
        const std::vector<int32_t> org = {0, 5, -3};
        // select rows 2, 0 (frames 0: no shift), concat of two groups
        EXPECT(gather({org}, {{0, 2}, {0, 0}}, {0}) == (std::vector<int32_t>{-3, 0}), "select");
        EXPECT(gather({org, {7}}, {{0, 0}, {0, 1}, {0, 2}, {1, 0}}, {0, 0}) == (std::vector<int32_t>{0, 5, -3, 7}), "concat");
        // a snapshot with the bit and one without are not rows of one group: the flags differ, and so do the segment lists
        const SnapManifest plain = stream(MODEL_CTS, 0, 320, 160, 0, 4000, 1);
        EXPECT(snap_concat_differs(m, plain).find("flags") != std::string::npos, "concat with and without the bit: %s", snap_concat_differs(m, plain).c_str());
        SnapManifest lied = plain;
        lied.flags = BIT;
        EXPECT(snap_concat_differs(m, lied).find("segment") != std::string::npos, "segment lists: %s", snap_concat_differs(m, lied).c_str());
    }
    // ---- the join: shift / hop on the origins of every part, of either sign, accumulating
    {
        const int hop = 160;
        const SnapManifest g = stream(MODEL_CTS, BIT, 320, hop, 0, 20000 + 7, 2), a = stream(MODEL_CTS, BIT, 320, hop, 0, 20000 + 7 - 5 * hop, 1),
                           old = stream(MODEL_CTS, BIT, 320, hop, 0, 20000 + 7 + 40 * hop, 1);
        JoinPlan plan;
        std::string why = snap_join_plan({&g, &a, &old}, 0, "", plan);
        EXPECT(why.empty(), "join refused: %s", why.c_str());
        EXPECT(plan.frames == (std::vector<int32_t>{0, 5, -40}), "frames %d %d %d", plan.frames.size() == 3 ? plan.frames[0] : -1,
               plan.frames.size() == 3 ? plan.frames[1] : -1, plan.frames.size() == 3 ? plan.frames[2] : -1);
        for (size_t p = 0; p < 3; ++p) EXPECT(plan.shift[p] == (int64_t)plan.frames[p] * hop, "part %zu: shift %lld", p, (long long)plan.shift[p]);
        std::vector<int32_t> j = gather({{0, 0}, {0}, {0}}, {{0, 0}, {0, 1}, {1, 0}, {2, 0}}, plan.frames);
        EXPECT(j == (std::vector<int32_t>{0, 0, 5, -40}), "first join");
        // row b's own frame index of group frame t: what it was before the join, for every row
        const int tg = g.t_done;
        EXPECT(tg - j[2] == a.t_done && tg - j[3] == old.t_done && tg - j[0] == g.t_done, "own indices %d %d %d", tg - j[0], tg - j[2], tg - j[3]);
        // the result joined again, 12 hops later, onto a younger group that goes first: every origin moves by the same shift
        SnapManifest res = stream(MODEL_CTS, BIT, 320, hop, 0, 20000 + 7 + 12 * hop, 4);
        const SnapManifest late = stream(MODEL_CTS, BIT, 320, hop, 0, 20000 + 7 - 100 * hop, 1);
        why = snap_join_plan({&late, &res}, 0, "", plan);
        EXPECT(why.empty() && plan.frames == (std::vector<int32_t>{0, -112}), "second join: %s", why.c_str());
        const std::vector<int32_t> j2 = gather({{0}, j}, {{0, 0}, {1, 0}, {1, 1}, {1, 2}, {1, 3}}, plan.frames);
        EXPECT(j2 == (std::vector<int32_t>{0, -112, -112, -107, -152}), "accumulated origins %d %d %d %d %d", j2[0], j2[1], j2[2], j2[3], j2[4]);
        EXPECT(late.t_done - j2[3] == a.t_done + 12 && late.t_done - j2[4] == old.t_done + 12, "own indices after two joins");
        // the models that keep call-order slots record a constant `first` = 1, and the engine tells the plan that it says nothing
        // (first_counts = false: Model::stream_state() is null): it does not hold a moved part back once a chunk is behind it
        SnapManifest g1 = g, a1 = a;
        g1.first = a1.first = 1;
        why = snap_join_plan({&g1, &a1}, 0, "", plan, false);
        EXPECT(why.empty() && plan.frames == (std::vector<int32_t>{0, 5}), "first = 1 on slot models: %s", why.c_str());
        // ... while for a model whose `first` is a real flag the same manifests are short of the left edge
        why = snap_join_plan({&g1, &a1}, 0, "", plan, true);
        EXPECT(why == "parts[0] is short of the left edge: t_done " + std::to_string(g1.t_done) +
                          ", a stream can be rebased from t_done 1 on (n_fft 320, hop 160, look-ahead 0)",
               "first = 1 where it counts: %s", why.c_str());
        // one part: a copy
        why = snap_join_plan({&a}, 0, "", plan);
        EXPECT(why.empty() && plan.frames == (std::vector<int32_t>{0}), "one part: %s", why.c_str());
        // the result's manifest keeps the segment where it belongs
        std::vector<RowLayout> lay = layouts(g);
        lay.back().inner = plan.live;
        EXPECT(snap_origin_why(snap_rows_manifest(g, lay, 4)).empty(), "joined manifest");
    }
    // ---- the plan accepts each of the four configurations with the bit (the engine hands it no counts_frames reason) ...
    {
        struct Cfg { int model, flags, n_fft, hop, lag; };
        for (const Cfg& c : {Cfg{MODEL_CTS, BIT, 320, 160, 0}, Cfg{MODEL_TAYLOR, BIT, 320, 160, 0}, Cfg{MODEL_G2, BIT, 320, 160, 0}, Cfg{MODEL_FSN, F, 512, 256, 2}}) {
            const SnapManifest g = stream(c.model, c.flags, c.n_fft, c.hop, c.lag, 9000 + 5 * c.hop, 2), a = stream(c.model, c.flags, c.n_fft, c.hop, c.lag, 9000, 1);
            JoinPlan plan;
            // what the engine passes: FullSubNet keeps a StreamState (its `first` is a flag), the cLN networks keep slots
            const bool fc = c.model == MODEL_FSN;
            const std::string why = snap_join_plan({&g, &a}, c.lag, "", plan, fc);
            EXPECT(why.empty() && plan.frames.size() == 2 && plan.frames[1] == 5, "model %d with the bit: %s", c.model, why.c_str());
            // everything else holds: phase, the left edge, the running scale
            const SnapManifest off = stream(c.model, c.flags, c.n_fft, c.hop, c.lag, 9000 + 50, 1);
            EXPECT(snap_join_plan({&g, &off}, c.lag, "", plan).find("out of phase") != std::string::npos, "model %d: out of phase", c.model);
            // The left edge.  All four configurations can be rebased from their first frame on, and a real stream that has transformed
            // nothing has emitted nothing either, so it is out of phase in o_done before the plan asks for the edge.  The refusal is the
            // plan's all the same and is held to its words on manifests no stream produces: a part with in-phase counters and t_done 0
            // (o_done is then what the phase check wants, negative), with the segments of a stream that has run ...
            const int need = stream_left_edge_frames(c.n_fft, c.hop, c.lag);
            EXPECT(need == 1, "model %d: left-edge threshold %d", c.model, need);
            const std::string edge = " on (n_fft " + std::to_string(c.n_fft) + ", hop " + std::to_string(c.hop) + ", look-ahead " + std::to_string(c.lag) + ")";
            SnapManifest young = a;
            young.t_done = 0;
            young.n_total = g.n_total - g.t_done * c.hop;
            young.o_done = young.n_total - (g.n_total - g.o_done);
            young.keep = 0;
            young.segs.back().bytes = (int64_t)young.batch * young.n_total * 4;
            EXPECT((g.n_total - young.n_total) % c.hop == 0 && young.first == g.first, "model %d: the young part is not in phase", c.model);
            std::string w = snap_join_plan({&g, &young}, c.lag, "", plan, fc);
            EXPECT(w == "parts[1] is short of the left edge: t_done 0, a stream can be rebased from t_done 1" + edge, "model %d, t_done 0: %s", c.model, w.c_str());
            w = snap_join_plan({&young, &g}, c.lag, "", plan, fc);
            EXPECT(w == "parts[0] is short of the left edge: t_done 0, a stream can be rebased from t_done 1" + edge, "model %d, t_done 0 first: %s", c.model, w.c_str());
            // ... and parts past the edge by their counters whose `first` is still set: refused where the model keeps the flag
            // (FullSubNet: its LSTMs would start from a zero state again), accepted where the field is the constant of a slot model
            SnapManifest gf = g, af = a;
            gf.first = af.first = 1;
            w = snap_join_plan({&gf, &af}, c.lag, "", plan, fc);
            if (fc)
                EXPECT(w == "parts[0] is short of the left edge: t_done " + std::to_string(g.t_done) + ", a stream can be rebased from t_done 1" + edge,
                       "model %d, first = 1: %s", c.model, w.c_str());
            else
                EXPECT(w.empty() && plan.frames[1] == 5, "model %d, first = 1: %s", c.model, w.c_str());
            // (shift 0: nothing moves, nothing is asked of the edge)
            EXPECT(snap_join_plan({&gf, &gf}, c.lag, "", plan, fc).empty(), "model %d: equal counters", c.model);
            SnapManifest run = a;
            run.running = 1;
            EXPECT(snap_join_plan({&g, &run}, c.lag, "", plan).find("is a running-scale stream") != std::string::npos, "model %d: running scale", c.model);
            // ... and refuses a manifest without it with the wording of an engine without it
            const SnapManifest p0 = stream(c.model, c.flags & ~BIT, c.n_fft, c.hop, c.lag, 9000, 1);
            w = snap_join_plan({&p0}, c.lag, "the cumulative LayerNorm divides its running sums by the number of frames so far", plan);
            EXPECT(w == "this model's stream state cannot be rebased: the cumulative LayerNorm divides its running sums by the number of frames so far",
                   "model %d without the bit: %s", c.model, w.c_str());
            // the two kinds do not mix
            EXPECT(snap_join_plan({&g, &p0}, c.lag, "", plan).find("differ: flags") != std::string::npos, "model %d: mixed parts", c.model);
        }
    }
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}

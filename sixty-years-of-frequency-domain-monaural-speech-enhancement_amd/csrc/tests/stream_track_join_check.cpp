// Stand-alone check of the host arithmetic a tracking-scale stream adds to se_stream_state_join (stream_join.h): the rotation of the
// per-frame rings, which entries are live, and the plan's acceptance.  Built with the host sanitizers (Makefile:
// stream_track_join_check), run on a CPU; prints "ok" and returns 0, or the first failure and 1.
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

static SnapManifest tracking(int n_fft, int hop, int lag, int n_total, int ring, float tau, int batch) {
    SnapManifest m;
    m.model = 2; m.n_fft = n_fft; m.hop = hop; m.win = n_fft;
    m.batch = batch; m.max_chunk = 8; m.n_total = n_total;
    m.t_done = n_total > n_fft / 2 ? (n_total - n_fft / 2 - 1) / hop + 1 : 0;
    m.o_done = std::max(0, std::min(n_total, (m.t_done - lag) * hop - n_fft / 2));
    m.keep = (int)(std::max<int64_t>(0, std::min<int64_t>((int64_t)m.t_done * hop - n_fft / 2, (int64_t)n_total - n_fft / 2 - 1)) & ~(int64_t)3);
    m.running = 2; m.ring = ring; m.first = m.t_done > 0 ? 0 : 1; m.state_B = batch;
    std::memcpy(&m.reserved[0], &tau, sizeof(float));
    auto seg = [&](int kind, int index, int64_t bytes) {
        SnapSeg s; s.kind = kind; s.index = index; s.bytes = bytes;
        m.segs.push_back(s);
    };
    seg(SNAP_C, 0, (int64_t)batch * 4);
    seg(SNAP_SUMSQ, 0, (int64_t)batch * 16);
    seg(SNAP_FRAME_INV, 0, (int64_t)batch * ring * 4);
    seg(SNAP_FRAME_INV, 1, (int64_t)batch * ring * 4);
    seg(SNAP_WINDOW, 0, (int64_t)batch * (n_total - m.keep) * 4);
    return m;
}

int main() {
    // ---- the rotation: frame t of a part is frame t + s / hop of the result, for shifts of either sign and beyond one ring
    for (int ring : {64, 128, 1024})
        for (int hop : {128, 160})
            for (int64_t f : {0L, 1L, 5L, 63L, 64L, 65L, 1000L, 123456L, -1L, -64L, -777L}) {
                const int64_t s = f * hop;
                const int rot = snap_ring_rot(s, hop, ring);
                EXPECT(rot >= 0 && rot < ring, "rot %d outside [0, %d)", rot, ring);
                std::vector<int64_t> src((size_t)ring), dst((size_t)ring);
                const int64_t t_lo = 5000;      // the ring holds frames [t_lo, t_lo + ring) of the part
                for (int64_t t = t_lo; t < t_lo + ring; ++t) src[(size_t)(t & (ring - 1))] = t;
                for (int i = 0; i < ring; ++i) dst[(size_t)i] = src[(size_t)snap_ring_src(i, rot, ring)];
                for (int64_t t = t_lo; t < t_lo + ring; ++t)
                    EXPECT(dst[(size_t)((t + f) & (ring - 1))] == t, "ring %d hop %d shift %lld frames: frame %lld misplaced", ring, hop, (long long)f,
                           (long long)t);
            }
    // ---- the live entries: the lowest frame whose 1 / c_t the inverse still reads, against a walk over the overlap-add's own test
    for (auto g : {std::pair<int, int>{320, 160}, {512, 128}, {512, 256}, {320, 161}})
        for (int o_done = 0; o_done < 3000; o_done += 7) {
            const int n_fft = g.first, hop = g.second;
            // frame t covers output sample o (pos = o + n_fft / 2) when t hop <= pos < t hop + n_fft; every sample >= o_done is still to be written
            int64_t lo = -1;
            for (int64_t t = 0; lo < 0; ++t)
                if (t * hop + n_fft > o_done + n_fft / 2) lo = t;
            EXPECT(snap_ring_live_from(o_done, n_fft, hop) == lo, "n_fft %d hop %d o_done %d: live from %lld, walk finds %lld", n_fft, hop, o_done,
                   (long long)snap_ring_live_from(o_done, n_fft, hop), (long long)lo);
        }
    // ... and they fit the shortest ring with room to spare, for every front end and look-ahead in the project
    for (auto g : {std::pair<int, int>{320, 160}, {512, 128}, {512, 256}, {320, 100}})
        for (int lag : {0, 2, 6})
            for (int n_total = 4000; n_total < 4700; n_total += 13) {
                const SnapManifest m = tracking(g.first, g.second, lag, n_total, 64, 8000.f, 1);
                const int64_t live = m.t_done - snap_ring_live_from(m.o_done, m.n_fft, m.hop);
                EXPECT(live >= 0 && live < 32, "n_fft %d hop %d lag %d n_total %d: %lld live ring entries", g.first, g.second, lag, n_total, (long long)live);
            }
    // ---- the plan: tracking parts in phase are accepted with the rotation of their shift; the refusals keep their wording
    {
        const int hop = 160, unit = 160;
        SnapManifest a = tracking(320, hop, 0, 48000 + 40, 512, 8000.f, 2), b = tracking(320, hop, 0, 8000 + 40, 512, 8000.f, 1);
        JoinPlan plan;
        std::string why = snap_join_plan({&a, &b}, 0, "", plan);
        EXPECT(why.empty(), "in-phase tracking parts refused: %s", why.c_str());
        EXPECT(plan.rot.size() == 2 && plan.rot[0] == 0 && plan.rot[1] == ((48000 - 8000) / hop) % 512, "rotation %d", plan.rot.size() == 2 ? plan.rot[1] : -1);
        EXPECT(plan.shift[1] == 40000 && plan.shift[1] % unit == 0, "shift %lld", (long long)plan.shift[1]);
        // the later stream first: a negative shift
        why = snap_join_plan({&b, &a}, 0, "", plan);
        EXPECT(why.empty() && plan.rot[1] == (512 - (40000 / hop) % 512) % 512, "negative shift: %s rot %d", why.c_str(), plan.rot.empty() ? -1 : plan.rot[1]);
        // another time constant
        SnapManifest c = tracking(320, hop, 0, 8000 + 40, 512, 1600.f, 1);
        why = snap_join_plan({&a, &c}, 0, "", plan);
        EXPECT(why.find("tau_samples") != std::string::npos, "differing tau not named: %s", why.c_str());
        EXPECT(snap_concat_differs(b, c).find("tau_samples") != std::string::npos, "concat: differing tau not named");
        // a fixed-scale part
        SnapManifest d = b;
        d.running = 0; d.ring = 0; d.reserved[0] = 0;
        d.segs.erase(d.segs.begin() + 1, d.segs.begin() + 4);
        why = snap_join_plan({&a, &d}, 0, "", plan);
        EXPECT(why.find("running 2 vs 0") != std::string::npos, "tracking with fixed scale: %s", why.c_str());
        // the running scale is refused as before
        SnapManifest r = b;
        r.running = 1;
        why = snap_join_plan({&a, &r}, 0, "", plan);
        EXPECT(why.find("is a running-scale stream") != std::string::npos, "running part: %s", why.c_str());
        // short of the left edge
        // (512 / 128 with six frames of look-ahead: rebased from t_done 9 on; this part has transformed 8)
        SnapManifest s = tracking(512, 128, 6, 1173, 512, 8000.f, 1), a2 = tracking(512, 128, 6, 1173 + 128 * 50, 512, 8000.f, 1);
        EXPECT(s.t_done == 8, "t_done %d", s.t_done);
        why = snap_join_plan({&a2, &s}, 6, "", plan);
        EXPECT(why.find("short of the left edge") != std::string::npos, "left edge: %s", why.c_str());
        // a ring that is no power of two
        SnapManifest q = b;
        q.ring = 500;
        why = snap_join_plan({&q}, 0, "", plan);
        EXPECT(why.find("no power of two") != std::string::npos, "odd ring: %s", why.c_str());
    }
    // ---- the row layouts of the engine-level segments of a tracking snapshot
    {
        const SnapManifest m = tracking(512, 128, 6, 9000, 256, 0.f, 3);
        std::vector<RowLayout> lay(m.segs.size());
        for (size_t k = 0; k < m.segs.size(); ++k) EXPECT(snap_engine_layout(m, m.segs[k], lay[k]), "segment %zu has no engine layout", k);
        const std::string why = snap_layout_check(m, lay);
        EXPECT(why.empty(), "layouts: %s", why.c_str());
        const SnapManifest one = snap_rows_manifest(m, lay, 1);
        EXPECT(one.segs[1].bytes == 16 && one.segs[2].bytes == 256 * 4 && one.segs[3].bytes == 256 * 4, "one row: %lld %lld", (long long)one.segs[1].bytes,
               (long long)one.segs[2].bytes);
    }
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}

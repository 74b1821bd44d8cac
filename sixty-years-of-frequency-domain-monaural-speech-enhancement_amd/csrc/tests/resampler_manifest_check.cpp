// Stand-alone host program over resampler_manifest.h, meant for `-fsanitize=address,undefined` (make resampler_manifest_check): no
// device code, not loaded into anything.  It writes the host image of snapshots taken before the first push, mid-signal at every
// rate pair the tests use and of a pass-through signal into buffers of exactly the image's size (so that a write or a read past
// either end is the sanitizer's to report), parses them back and compares every field, and feeds the parser the malformed images
// se_resampler_state_import has to refuse - each has to be refused for the defect it has.  Exit status 0 and "ok" when everything
// holds.
#include "../resampler_manifest.h"
#include <algorithm>
#include <climits>
#include <cstdio>
#include <limits>
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

// the record a save leaves after n_total samples of a signal at sr_in -> sr_out: the counters a push keeps
static ResamplerManifest make(int sr_in, int sr_out, int batch, int64_t n_total) {
    ResamplerManifest m;
    m.sr_in = sr_in;
    m.sr_out = sr_out;
    m.batch = batch;
    m.n_total = n_total;
    if (sr_in == sr_out) {
        m.w0 = m.t = n_total;
        return m;
    }
    const ResamplePlan p = resample_plan(sr_in, sr_out);
    m.w0 = std::max<int64_t>(0, n_total - 2L * p.reach);
    ResamplePos pos;
    (void)resample_advance(p, pos, n_total, INT64_MAX, nullptr, 0);
    m.t = pos.t;
    m.acc_bits = rsnap_bits_of(pos.acc);
    return m;
}

// a heap buffer of exactly n bytes
static std::unique_ptr<uint8_t[]> image_of(const ResamplerManifest& m, int64_t& n) {
    n = rsnap_image_bytes(m);
    std::unique_ptr<uint8_t[]> buf(new uint8_t[(size_t)n]);
    rsnap_write_head(m, buf.get());
    for (int64_t i = RSNAP_HEAD_BYTES; i < n; ++i) buf[(size_t)i] = (uint8_t)(i * 7);
    return buf;
}

static bool refused(const uint8_t* p, int64_t n, const char* word) {
    ResamplerManifest m;
    int64_t off = -1;
    const std::string why = rsnap_parse(p, n, m, off);
    if (why.find(word) == std::string::npos) std::printf("  got '%s', wanted '%s'\n", why.c_str(), word);
    return !why.empty() && why.find(word) != std::string::npos;
}

// header field offsets (resampler_manifest.h)
constexpr int64_t OFF_SR_IN = 8, OFF_BATCH = 16, OFF_N_TOTAL = 24, OFF_W0 = 32, OFF_T = 40, OFF_ACC = 48, OFF_PAYLOAD = 56;

int main() {
    EXPECT(RSNAP_HEAD_BYTES == 64 && OFF_PAYLOAD + 8 == RSNAP_HEAD_BYTES);
    const double third = 1.0 / 3.0;
    EXPECT(rsnap_double_of(rsnap_bits_of(third)) == third);

    const ResamplerManifest cases[] = {
        make(48000, 16000, 2, 0),          // before the first push: no payload
        make(48000, 16000, 2, 100),        // shorter than reach: nothing released, the history is the whole signal
        make(48000, 16000, 2, 5003),       // a full history of 2 * reach
        make(32000, 16000, 1, 777),
        make(44100, 16000, 3, 1681),       // the running sum: acc has a fraction
        make(16000, 48000, 2, 131),        // upsampling, reach 65
        make(16000, 16000, 2, 900),        // pass-through: counters only
    };
    for (const ResamplerManifest& m : cases) {
        EXPECT(rsnap_check(m).empty());
        int64_t n = 0;
        const auto buf = image_of(m, n);
        EXPECT(n == RSNAP_HEAD_BYTES + (int64_t)m.batch * (m.n_total - m.w0) * 4);
        ResamplerManifest r;
        int64_t off = -1;
        const std::string why = rsnap_parse(buf.get(), n, r, off);
        EXPECT(why.empty());
        EXPECT(off == RSNAP_HEAD_BYTES);
        EXPECT(r.sr_in == m.sr_in && r.sr_out == m.sr_out && r.batch == m.batch);
        EXPECT(r.n_total == m.n_total && r.w0 == m.w0 && r.t == m.t && r.acc_bits == m.acc_bits);

        // cut short at every length below the whole: each in a buffer of its own exact size
        for (int64_t cut : {(int64_t)0, (int64_t)3, (int64_t)8, RSNAP_HEAD_BYTES - 1, RSNAP_HEAD_BYTES, n - 1}) {
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
            EXPECT(refused(more.get(), n + 1, "trailing"));
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
        auto with64 = [&](int64_t pos, int64_t value) {
            std::unique_ptr<uint8_t[]> g(new uint8_t[(size_t)n]);
            std::memcpy(g.get(), buf.get(), (size_t)n);
            std::memcpy(g.get() + pos, &value, 8);
            return g;
        };
        auto with32 = [&](int64_t pos, int32_t value) {
            std::unique_ptr<uint8_t[]> g(new uint8_t[(size_t)n]);
            std::memcpy(g.get(), buf.get(), (size_t)n);
            std::memcpy(g.get() + pos, &value, 4);
            return g;
        };
        const int64_t pay = rsnap_payload_bytes(m);
        // a payload size that is not batch * (n_total - w0) * 4
        EXPECT(refused(with64(OFF_PAYLOAD, pay + 4).get(), n, "batch * (n_total - w0) * 4"));
        EXPECT(refused(with64(OFF_PAYLOAD, -4).get(), n, "negative or overflowing"));
        EXPECT(refused(with64(OFF_PAYLOAD, INT64_MAX - 3).get(), n, "negative or overflowing"));
        // negative or overflowing counters
        EXPECT(refused(with64(OFF_N_TOTAL, -1).get(), n, "negative"));
        EXPECT(refused(with64(OFF_W0, -1).get(), n, "negative"));
        EXPECT(refused(with64(OFF_T, -1).get(), n, "negative"));
        EXPECT(refused(with64(OFF_ACC, (int64_t)rsnap_bits_of(-1.5)).get(), n, "negative"));
        EXPECT(refused(with64(OFF_ACC, (int64_t)rsnap_bits_of(std::numeric_limits<double>::quiet_NaN())).get(), n, "negative"));
        EXPECT(refused(with64(OFF_N_TOTAL, (int64_t)1 << 31).get(), n, "overflowing"));
        EXPECT(refused(with64(OFF_N_TOTAL, INT64_MAX).get(), n, "overflowing"));
        EXPECT(refused(with64(OFF_T, (int64_t)1 << 31).get(), n, "overflowing"));
        EXPECT(refused(with64(OFF_ACC, (int64_t)rsnap_bits_of(1e300)).get(), n, "overflowing"));
        EXPECT(refused(with64(OFF_ACC, (int64_t)rsnap_bits_of(std::numeric_limits<double>::infinity())).get(), n, "overflowing"));
        EXPECT(refused(with32(OFF_BATCH, 0).get(), n, "rates or batch"));
        EXPECT(refused(with32(OFF_SR_IN, -48000).get(), n, "rates or batch"));
        // w0 > n_total
        EXPECT(refused(with64(OFF_W0, m.n_total + 1).get(), n, "behind the"));
        // more history than 2 * reach of the recorded rates (a pass-through signal: any history at all)
        if (m.sr_in != m.sr_out) {
            const int64_t reach = resample_plan(m.sr_in, m.sr_out).reach;
            EXPECT(refused(with64(OFF_N_TOTAL, m.w0 + 2 * reach + 1).get(), n, "2 * reach"));
            if (m.n_total - m.w0 == 2 * reach) EXPECT(refused(with64(OFF_W0, m.w0 - 1).get(), n, "2 * reach"));
        } else {
            EXPECT(refused(with64(OFF_W0, m.n_total - 1).get(), n, "pass-through"));
        }
        // a batch that no longer matches the payload
        if (pay) EXPECT(refused(with32(OFF_BATCH, m.batch + 1).get(), n, "batch * (n_total - w0) * 4"));
    }
    // rates whose ratio the table cannot resolve
    {
        ResamplerManifest m = make(48000, 16000, 1, 10);
        m.sr_out = 1;
        EXPECT(rsnap_check(m).find("resolution") != std::string::npos);
    }
    EXPECT(refused(nullptr, 100, "truncated"));
    if (failures == 0) std::printf("ok\n");
    return failures ? 1 : 0;
}

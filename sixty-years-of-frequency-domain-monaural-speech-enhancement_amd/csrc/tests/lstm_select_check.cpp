// Stand-alone host program over lstm_select.h, meant for `-fsanitize=address,undefined` (make lstm_select_check): no device code,
// not loaded into anything.  One hand-written call per rung of the cooperative LSTM's ladder - the H = 256 opt-in, the K-split
// form by NS / TAG, sub-tiles by LEAD (before and after the 16-sequence tiles), 16-sequence tiles, the flag-barrier form, a chunk
// launch, the one-sequence stack - and the calls the ladder refuses, each with its own message; then the support queries and the
// chunk plan.  256 CUs unless a line says otherwise.  Exit status 0 and "ok" when everything holds.
#include "../lstm_select.h"
#include <cstdio>
#include <cstring>

using namespace se;

static int failures = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("line %d: %s\n", __LINE__, #c);                  \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// a time-major call (rows of S sequences)
static LstmSelIn call(int H, int S, int Z = 1, int n_cu = 256) {
    LstmSelIn in;
    in.H = H; in.S = S; in.Z = Z;
    in.gx_row = in.out_row = S;
    in.n_cu = n_cu;
    return in;
}
static bool is(const LstmChoice& c, int form, int H, int v = 0) {
    const int cv = form == LSTM_FORM_KS ? c.NS : form == LSTM_FORM_COOP8 ? c.LEAD : form == LSTM_FORM_STACK ? c.L : 0;
    return c.form == form && c.H == H && cv == v;
}
static bool refused(const LstmChoice& c, const char* word) { return c.form == LSTM_FORM_REFUSED && std::strstr(c.refusal, word); }

int main() {
    const LstmTuning tun;
    LstmTuning no16, no4, no256, nochunk;
    no16.coop16 = 0;
    no4.coop4 = 0;
    no256.coop256 = 0;
    nochunk.chunk = 0;

    // ---- K-split form: NS / TAG by S, one exchange slab pair per LSTM, 256 flags each
    LstmChoice c = lstm_coop_select(call(1024, 1), tun);
    EXPECT(is(c, LSTM_FORM_KS, 1024, 1) && c.TAG == 1 && c.stale == 1 && c.nflag == 256 && c.grid == 256 && c.SS == 1 && !c.zero_cell);
    EXPECT(c.lds == (size_t)4 * 16 * 260 * 4 + 4096 && c.lds_attr == (int)c.lds && c.block == 256);
    c = lstm_coop_select(call(1024, 4), tun);
    EXPECT(is(c, LSTM_FORM_KS, 1024, 4) && c.TAG == 1);
    c = lstm_coop_select(call(1024, 16), tun);
    EXPECT(is(c, LSTM_FORM_KS, 1024, 16) && c.TAG == 0 && c.stale == 0);
    c = lstm_coop_select(call(512, 4, 2), tun);
    EXPECT(is(c, LSTM_FORM_KS, 512, 4) && c.grid == 256 && c.nflag == 512 && c.slabs == 2);
    EXPECT(is(lstm_coop_select(call(512, 5), tun), LSTM_FORM_COOP, 512));                 // H = 512: up to 4 sequences only
    EXPECT(!is(lstm_coop_select(call(1024, 16, 1, 128), tun), LSTM_FORM_KS, 1024, 16));   // H / 4 workgroups need as many CUs

    // ---- sub-tiles ahead of the 16-sequence tiles (H = 1024, a single tile per workgroup and S us_z < 15 n_cu): LEAD by sub-tiles owned
    c = lstm_coop_select(call(1024, 17), tun);
    EXPECT(is(c, LSTM_FORM_COOP8, 1024, 1) && c.NW == 4 && c.SS == 4 && c.grid == 256 && c.stale == 1 && c.nflag == 0 && c.lds_attr == 160 * 1024);
    EXPECT(c.lds == ((size_t)2 * 4 * 1040 + 2 * 4 * 64 + 4 * 16 * 256 + 64 * 2) * 4);
    EXPECT(is(lstm_coop_select(call(1024, 29), tun), LSTM_FORM_COOP8, 1024, 2));
    EXPECT(is(lstm_coop_select(call(1024, 59), tun), LSTM_FORM_COOP8, 1024, 2));
    // ---- 16-sequence tiles
    c = lstm_coop_select(call(1024, 60), tun);
    EXPECT(is(c, LSTM_FORM_COOP16, 1024) && c.SS == 4 && c.grid == 256 && c.lds == lstm_tile16_lds(1024, 1) && c.lds_attr == 160 * 1024 && c.stale == 1);
    EXPECT(is(lstm_coop_select(call(1024, 1472), tun), LSTM_FORM_COOP16, 1024));
    c = lstm_coop_select(call(512, 100, 2), tun);
    EXPECT(is(c, LSTM_FORM_COOP16, 512) && c.Z == 2 && c.SS == 4 && c.grid == 256 && c.slabs == 2);
    // ---- sub-tiles behind them (the tiles' cell states no longer fit LDS), LEAD = 3
    c = lstm_coop_select(call(1024, 1473), tun);
    EXPECT(is(c, LSTM_FORM_COOP8, 1024, 3) && c.lds <= LSTM_LDS_MAX);
    EXPECT(is(lstm_coop_select(call(1024, 1536), tun), LSTM_FORM_COOP8, 1024, 3));
    // ---- the flag-barrier form: flags per (z, slice), the cell state zeroed, no stale fill
    c = lstm_coop_select(call(1024, 1537), tun);
    EXPECT(is(c, LSTM_FORM_COOP, 1024) && c.SS == 4 && c.nflag == 4 * 64 && c.zero_cell == 1 && c.stale == 0 && c.lds == (size_t)2 * 16 * 1028 * 4 &&
           c.lds_attr == (int)c.lds);
    // ---- the switches
    EXPECT(is(lstm_coop_select(call(512, 17), no16), LSTM_FORM_COOP8, 512, 1));
    EXPECT(is(lstm_coop_select(call(512, 100), no16), LSTM_FORM_COOP8, 512, 2));
    EXPECT(is(lstm_coop_select(call(512, 200), no16), LSTM_FORM_COOP8, 512, 3));
    EXPECT(is(lstm_coop_select(call(512, 3073), no16), LSTM_FORM_COOP, 512));
    EXPECT(is(lstm_coop_select(call(1024, 17), no4), LSTM_FORM_COOP16, 1024));
    EXPECT(is(lstm_coop_select(call(1024, 1473), no4), LSTM_FORM_COOP, 1024));
    // ---- 32-bit lane offsets: feature-major rows either side of 4 GB fall from the tiles to the flag-barrier form
    LstmSelIn fm = call(1024, 992);
    fm.gx_row = fm.out_row = 992L * 246;
    EXPECT(is(lstm_coop_select(fm, tun), LSTM_FORM_COOP16, 1024));
    fm.gx_row = fm.out_row = 992L * 247;
    EXPECT(is(lstm_coop_select(fm, tun), LSTM_FORM_COOP, 1024));
    EXPECT(lstm_rows_fit32(1024, 244140, 244140) && !lstm_rows_fit32(1024, 244141, 1) && !lstm_rows_fit32(1024, 1, 3906250));
    EXPECT(lstm_slabs_fit32(1024, 262143) && !lstm_slabs_fit32(1024, 262144));
    // ---- H = 256: opt-in, one LSTM of 17 - 4096 sequences on 16-sequence tiles
    c = lstm_coop_select(call(256, 17), tun);
    EXPECT(is(c, LSTM_FORM_COOP16, 256) && c.SS == 2 && c.grid == 32);
    EXPECT(is(lstm_coop_select(call(256, 4096), tun), LSTM_FORM_COOP16, 256));
    EXPECT(refused(lstm_coop_select(call(256, 16), tun), "H = 256"));
    EXPECT(refused(lstm_coop_select(call(256, 4097), tun), "H = 256"));
    EXPECT(refused(lstm_coop_select(call(256, 17, 2), tun), "H = 256"));
    EXPECT(refused(lstm_coop_select(call(256, 17), no256), "H = 256"));
    EXPECT(refused(lstm_coop_select(call(256, 17), no16), "H = 256"));
    // ---- the other refusals
    EXPECT(refused(lstm_coop_select(call(384, 17), tun), "built for H = 512 / 1024"));
    EXPECT(refused(lstm_coop_select(call(384, 2), tun), "built for H = 512 / 1024"));
    EXPECT(refused(lstm_coop_select(call(8, 2), tun), "built for H = 512 / 1024"));
    EXPECT(refused(lstm_coop_select(call(1024, 100, 2, 64), tun), "more unit slices than CUs"));
    EXPECT(refused(lstm_coop_select(call(512, 4096, 2, 16384), tun), "too many slices"));      // 2 x 256 slices
    // ---- a launch of the chunk pipeline: 16-sequence tiles whatever the switches, slabs for the whole stack
    LstmSelIn ch = call(1024, 64, 2);
    ch.gx_row = ch.out_row = 64L * 401;
    ch.chunk = 1;
    ch.n_layers = 3;
    c = lstm_coop_select(ch, no16);
    EXPECT(is(c, LSTM_FORM_COOP16, 1024) && c.chunk == 1 && c.slabs == 3 && c.Z == 2 && c.SS == 2 && c.grid == 256 && c.lds == lstm_tile16_lds(1024, 2));
    ch.n_layers = 5;
    EXPECT(refused(lstm_coop_select(ch, tun), "1 - 4 layers"));
    ch.n_layers = 2;
    ch.H = 256;
    EXPECT(refused(lstm_coop_select(ch, tun), "1 - 4 layers"));
    ch.H = 1024;
    ch.gx_row = 992L * 247;
    EXPECT(refused(lstm_coop_select(ch, tun), "32-bit lane offsets"));
    ch = call(1024, 4096, 1, 64);
    ch.chunk = 1;
    ch.n_layers = 2;
    EXPECT(refused(lstm_coop_select(ch, tun), "too many tiles per workgroup"));
    // ---- the one-sequence stack
    c = lstm_stack_select(1024, 3, 256);
    EXPECT(is(c, LSTM_FORM_STACK, 1024, 3) && c.grid == 256 && c.slabs == 3 && c.stale == 1 && c.Z == 1 && c.SS == 1 &&
           c.lds == ((size_t)4 * 5 * 256 + 3 * 64) * 4 + (size_t)2 * 16 * 1024 * 4);
    EXPECT(is(lstm_stack_select(512, 2, 128), LSTM_FORM_STACK, 512, 2));
    EXPECT(refused(lstm_stack_select(1024, 4, 256), "2 or 3 layers"));
    EXPECT(refused(lstm_stack_select(1024, 2, 255), "2 or 3 layers"));
    EXPECT(refused(lstm_stack_select(256, 2, 256), "2 or 3 layers"));

    // ---- the support queries
    EXPECT(lstm_coop_ok(1024, 4096, 4) && !lstm_coop_ok(1024, 4097, 1) && !lstm_coop_ok(1024, 1, 5) && lstm_coop_ok(512, 1, 8) && !lstm_coop_ok(256, 17, 1));
    EXPECT(!lstm_coop256_ok(16, 256, tun) && lstm_coop256_ok(17, 256, tun) && lstm_coop256_ok(4096, 256, tun) && !lstm_coop256_ok(4097, 256, tun));
    EXPECT(!lstm_coop256_ok(17, 15, tun) && !lstm_coop256_ok(17, 256, no256) && !lstm_coop256_ok(17, 256, no16));
    EXPECT(!lstm_coop_chunk_ok(1024, 16, 2, 256, tun) && lstm_coop_chunk_ok(1024, 17, 2, 256, tun) && lstm_coop_chunk_ok(1024, 64, 4, 256, tun));
    EXPECT(!lstm_coop_chunk_ok(1024, 65, 2, 256, tun) && !lstm_coop_chunk_ok(1024, 17, 5, 256, tun) && !lstm_coop_chunk_ok(1024, 17, 1, 256, tun));
    EXPECT(lstm_coop_chunk_ok(512, 128, 2, 256, tun) && !lstm_coop_chunk_ok(512, 129, 2, 256, tun) && !lstm_coop_chunk_ok(1024, 17, 2, 256, nochunk));
    EXPECT(!lstm_coop_chunk_ok(1024, 17, 3, 128, tun) && !lstm_coop_chunk_ok(256, 17, 2, 256, tun));
    // ---- the chunk plan
    EXPECT(lstm_chunk_steps(1024, 17, 2, 95, 256, tun) == 0 && lstm_chunk_steps(1024, 17, 2, 96, 256, tun) == 48);
    EXPECT(lstm_chunk_steps(1024, 17, 2, 1, 256, tun) == 0 && lstm_chunk_steps(1024, 17, 2, 3, 256, tun) == 0 && lstm_chunk_steps(1024, 17, 2, 4, 256, tun) == 0);
    EXPECT(lstm_chunk_steps(1024, 64, 2, 3814, 256, tun) == 48 && lstm_chunk_steps(1024, 64, 2, 3815, 256, tun) == 0);      // T S 16 KB = 4 GB
    EXPECT(lstm_chunk_steps(1024, 17, 2, 96, 256, nochunk) == 0);
    EXPECT(lstm_chunk_launches(97, 48, 2) == 4);
    const int want[4][2][3] = {{{0, 0, 48}, {-1}}, {{0, 48, 48}, {1, 0, 48}}, {{0, 96, 1}, {1, 48, 48}}, {{1, 96, 1}, {-1}}};
    for (int s = 0; s < 4; ++s) {
        LstmChunkRange r[4];
        const int n = lstm_chunk_launch(97, 48, 2, s, r);
        EXPECT(n == (want[s][1][0] < 0 ? 1 : 2));
        for (int i = 0; i < n; ++i) EXPECT(r[i].layer == want[s][i][0] && r[i].t0 == want[s][i][1] && r[i].len == want[s][i][2]);
    }
    LstmChunkRange r4[4];
    EXPECT(lstm_chunk_launch(401, 48, 4, 5, r4) == 4 && r4[3].layer == 3 && r4[3].t0 == 96 && r4[0].t0 == 240);
    EXPECT(lstm_chunk_launch(401, 48, 4, 11, r4) == 1 && r4[0].layer == 3 && r4[0].t0 == 384 && r4[0].len == 17);
    EXPECT(std::strcmp(lstm_form_name(LSTM_FORM_COOP8), "coop8") == 0 && std::strcmp(lstm_form_name(c.form), "stack") == 0);

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}

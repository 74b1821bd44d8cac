// Stand-alone host program over window_cut() of window_rows.h, meant for `-fsanitize=address,undefined` (make window_cut_check): no
// device code, not loaded into anything.  It walks the windows of a decode as stream_process does (t0 = 0, n, 2n, ... with HC = 12
// history columns, chunk sizes 1, 7 and 16) for every row length 1 .. 80 while a longer row keeps the walk going, and holds the cut of
// every window against the brute-force statement: column c of the window holds frame t0 - HC + c, and it is kept if and only if that
// frame lies below the row's frame count.  Then the ends of the range: the frame count and window origin of a clip at the position
// bound 2^31 - 1 - n_fft - 32 hop samples, and INT_MAX itself, where a 32-bit difference would overflow.  Exit status 0 and "ok".
#include "../window_rows.h"
#include <climits>
#include <cstdio>
#include <initializer_list>

using namespace se;

static int failures = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            if (failures < 20) std::printf("line %d: %s\n", __LINE__, #c); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// columns [0, cut) kept, [cut, Tw) cleared  <=>  column c kept iff frame t0 - HC + c < tlen
static void check(int tlen, int t0, int HC, int Tw) {
    const int cut = window_cut(tlen, t0, HC, Tw);
    EXPECT(cut >= 0 && cut <= Tw);
    for (int c = 0; c < Tw; ++c) {
        const bool kept = (long long)t0 - HC + c < (long long)tlen;
        EXPECT(kept == (c < cut));
    }
}

int main() {
    const int HC = 12;
    long long cases = 0;
    for (int n : {1, 7, 16})
        for (int tlen = 1; tlen <= 80; ++tlen)
            for (int t0 = 0; t0 < 80 + 2 * HC + 2 * n; t0 += n) {      // the walk of a longer row goes on behind this one's end
                check(tlen, t0, HC, HC + n);
                ++cases;
            }
    // a shorter last window at every origin (n < max_chunk) and the causal decoder's four history columns
    for (int tlen = 1; tlen <= 80; ++tlen)
        for (int t0 = 0; t0 <= 100; ++t0)
            for (int n = 1; n <= 16; ++n) {
                check(tlen, t0, HC, HC + n);
                check(tlen, t0, 4, 4 + n);
                cases += 2;
            }
    // named cases: before the window, at column 0, inside, at Tw - 1, at Tw, beyond
    EXPECT(window_cut(5, 40, 12, 19) == 0);
    EXPECT(window_cut(28, 40, 12, 19) == 0);
    EXPECT(window_cut(29, 40, 12, 19) == 1);
    EXPECT(window_cut(40, 40, 12, 19) == 12);
    EXPECT(window_cut(46, 40, 12, 19) == 18);
    EXPECT(window_cut(47, 40, 12, 19) == 19);
    EXPECT(window_cut(1000, 40, 12, 19) == 19);
    EXPECT(window_cut(1, 0, 12, 13) == 13);      // the first window: t0 - HC is negative, columns 0 .. HC - 1 are frames below 0
    // the position bound of se_enhance_long_ragged: n_fft 512, hop 128 (DCCRN's front end; frames = 1 + padded samples / hop)
    const long long bound = 2147483647LL - 512 - 32 * 128;
    const int tmax = (int)(1 + (bound + 127) / 128);
    for (int n : {1, 7, 16, 500})
        for (int d = -40; d <= 40; ++d) {
            check(tmax, tmax + d - n, HC, HC + n);      // the longest row's last windows
            check(1, tmax + d - n, HC, HC + n);         // against a row that ended at the start
            check(tmax + d, 0, HC, HC + n);             // and the first window of the longest
            cases += 3;
        }
    // the ends of int: no 32-bit difference is formed
    EXPECT(window_cut(INT_MAX, 0, 12, 28) == 28);
    EXPECT(window_cut(INT_MAX, INT_MAX, 12, 28) == 12);
    EXPECT(window_cut(0, INT_MAX, 12, 28) == 0);
    EXPECT(window_cut(INT_MAX, INT_MIN + 12, 12, 28) == 28);
    EXPECT(window_cut(INT_MIN, INT_MAX, 0, 28) == 0);
    check(INT_MAX, INT_MAX - 5, HC, HC + 16);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("%lld windows\nok\n", cases);
    return 0;
}

// Stand-alone host program over batch_parts.h, meant for `-fsanitize=address,undefined` (make batch_parts_check): no device code, not
// loaded into anything.  Every batch from 0 to 4 100 and a few near INT_MAX, one to three parts, every lead: the parts tile the
// batch in order, equal parts are the ceil(batch / parts) rule, unequal parts keep whole 4-row groups in every part but the last
// and do not grow from part to part for a lead above equal, and a twin's workspace holds every part it is ever given.  Exit status 0 and "ok".
// With arguments `cut <parts> <lead> <batch>...` it prints the rows of each batch's parts, one line per batch.
#include "../batch_parts.h"
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static void check_cut(int batch, int parts, int lead) {
    const BatchParts p = batch_parts_cut(batch, parts, lead);
    EXPECT(p.n >= 1 && p.n <= BATCH_PARTS_MAX && p.n <= (parts < 1 ? 1 : parts));
    if (parts > BATCH_PARTS_MAX) parts = BATCH_PARTS_MAX;      // (more parts than streams: as many as there are)
    long long sum = 0;
    for (int i = 0; i < p.n; ++i) {
        EXPECT(p.r0[i] == sum);
        EXPECT(p.rows[i] > 0 || batch <= 0);
        sum += p.rows[i];
    }
    EXPECT(sum == (batch > 0 ? batch : 0));
    if (parts <= 1 || batch <= 0) {
        EXPECT(p.n == 1);
        return;
    }
    if (lead == BATCH_LEAD_EQUAL) {
        const int Bp = (int)(((long long)batch + parts - 1) / parts);
        for (int i = 0; i + 1 < p.n; ++i) EXPECT(p.rows[i] == Bp);
        EXPECT(p.rows[p.n - 1] <= Bp);
        return;
    }
    if (batch < 4 * parts) {
        EXPECT(p.n == 1);
        return;
    }
    EXPECT(p.n == parts);
    for (int i = 0; i + 1 < p.n; ++i) EXPECT(p.rows[i] % 4 == 0 && p.rows[i] >= 4);
    EXPECT(p.rows[p.n - 1] >= 4);
    const int l = lead < BATCH_LEAD_MIN ? BATCH_LEAD_MIN : lead > BATCH_LEAD_MAX ? BATCH_LEAD_MAX : lead;
    // the first part is the nearest whole group to its share wherever the later parts' 4 rows leave room for it
    const double want = (double)batch * l / (8.0 * parts);
    if (want >= 4 && want <= batch - 4.0 * parts) EXPECT(p.rows[0] >= want - 2.0 - 1e-6 && p.rows[0] <= want + 2.0 + 1e-6);
    if (l > BATCH_LEAD_EQUAL && batch >= BATCH_SPLIT_MIN)
        for (int i = 0; i + 1 < p.n; ++i) EXPECT(p.rows[i] >= p.rows[i + 1]);
}

int main(int argc, char** argv) {
    if (argc >= 4 && !std::strcmp(argv[1], "cut")) {
        const int parts = std::atoi(argv[2]), lead = std::atoi(argv[3]);
        for (int a = 4; a < argc; ++a) {
            const BatchParts p = batch_parts_cut(std::atoi(argv[a]), parts, lead);
            for (int i = 0; i < p.n; ++i) std::printf(i ? " %d" : "%d", p.rows[i]);
            std::printf("\n");
        }
        return 0;
    }
    for (int parts = 0; parts <= 4; ++parts)
        for (int lead = 0; lead <= 16; ++lead) {
            for (int b = -1; b <= 4100; ++b) check_cut(b, parts, lead);
            for (int b : {INT_MAX, INT_MAX - 1, INT_MAX - 3, INT_MAX / 2, 1 << 30}) check_cut(b, parts, lead);
        }
    // the cases the documents name
    BatchParts p = batch_parts_cut(256, 2, 10);
    EXPECT(p.n == 2 && p.rows[0] == 160 && p.rows[1] == 96);
    p = batch_parts_cut(256, 2, 9);
    EXPECT(p.n == 2 && p.rows[0] == 144 && p.rows[1] == 112);
    p = batch_parts_cut(67, 2, 10);
    EXPECT(p.n == 2 && p.rows[0] == 40 && p.rows[1] == 27);      // (the last part: 24 rows + a group of 3)
    p = batch_parts_cut(256, 3, 10);
    EXPECT(p.n == 3 && p.rows[0] == 108 && p.rows[1] == 92 && p.rows[2] == 56);
    p = batch_parts_cut(65, 2, BATCH_LEAD_EQUAL);
    EXPECT(p.n == 2 && p.rows[0] == 33 && p.rows[1] == 32);
    p = batch_parts_cut(200, 3, BATCH_LEAD_EQUAL);
    EXPECT(p.n == 3 && p.rows[0] == 67 && p.rows[1] == 67 && p.rows[2] == 66);
    // parts per call
    EXPECT(batch_parts_count(63, 2) == 1 && batch_parts_count(64, 0) == 1 && batch_parts_count(64, 1) == 2 && batch_parts_count(256, 1) == 2);
    EXPECT(batch_parts_count(191, 2) == 2 && batch_parts_count(192, 2) == 3 && batch_parts_count(INT_MAX, 5) == 3);
    // a twin's rows cover every call, and no more than the largest part it is given
    for (int ntwins = 1; ntwins <= 2; ++ntwins)
        for (int lead = BATCH_LEAD_MIN; lead <= BATCH_LEAD_MAX; ++lead)
            for (int mb : {64, 65, 100, 191, 192, 193, 256, 300}) {
                for (int t = 0; t < ntwins; ++t) {
                    const int cap = batch_parts_twin_rows(mb, ntwins, lead, t);
                    bool reached = false;
                    for (int b = BATCH_SPLIT_MIN; b <= mb; ++b) {
                        const BatchParts q = batch_parts_cut(b, batch_parts_count(b, ntwins), lead);
                        if (t + 1 < q.n) {
                            EXPECT(q.rows[t + 1] <= cap);
                            reached = reached || q.rows[t + 1] == cap;
                        }
                    }
                    EXPECT(reached || cap == 0);
                }
            }
    EXPECT(batch_parts_twin_rows(63, 1, 10, 0) == 0);
    EXPECT(batch_parts_twin_rows(256, 1, 10, 0) == 96 && batch_parts_twin_rows(256, 1, BATCH_LEAD_EQUAL, 0) == 128);
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}

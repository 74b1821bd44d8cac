// How se_enhance_batch cuts an equal-length batch into the parts that decode side by side (engine.hip).
// Host arithmetic only, no HIP: csrc/tests/batch_parts_check.cpp runs it under the host sanitizers.
#pragma once

namespace se {

constexpr int BATCH_PARTS_MAX = 3;          // the caller's stream + two pooled auxiliary streams
constexpr int BATCH_SPLIT_MIN = 64;         // calls of fewer clips stay one decode
constexpr int BATCH_LEAD_EQUAL = 8;         // `lead` of equal parts
constexpr int BATCH_LEAD_MIN = 4, BATCH_LEAD_MAX = 12;

struct BatchParts {
    int n = 1;                              // parts that have rows (1: the call stays one decode)
    int r0[BATCH_PARTS_MAX] = {};           // first row of part i
    int rows[BATCH_PARTS_MAX] = {};         // its rows; part 0 runs on the caller's stream, part i > 0 on twin i - 1
};

// parts of a call of `batch` clips on an engine that owns `ntwins` further instances: one below BATCH_SPLIT_MIN, three from 192 clips
// on where there are two twins (at 64 clips a third part loses: DPCRN - 3 %), else two
inline int batch_parts_count(int batch, int ntwins) {
    if (ntwins <= 0 || batch < BATCH_SPLIT_MIN) return 1;
    const int have = ntwins + 1 < BATCH_PARTS_MAX ? ntwins + 1 : BATCH_PARTS_MAX;
    return have >= 3 && batch >= 192 ? 3 : 2;
}

// `lead` is the share of the first of k parts still to cut, in eighths of an equal share: it takes lead / (8 k) of the rows left.
// BATCH_LEAD_EQUAL: ceil(batch / parts) rows per part, the last part shorter - any row count.
// Any other lead (clamped to BATCH_LEAD_MIN ... BATCH_LEAD_MAX): unequal parts that reach the same layer at different times.  Every
// part but the last is a whole number of 4-row groups (the recurrent kernels walk 4 sequences per workgroup: only the last part
// may carry a group that is not full) and every part keeps at least 4 rows; batches too small for that stay one decode.
inline BatchParts batch_parts_cut(int batch, int parts, int lead) {
    BatchParts p;
    p.rows[0] = batch > 0 ? batch : 0;
    if (parts > BATCH_PARTS_MAX) parts = BATCH_PARTS_MAX;
    if (batch <= 0 || parts <= 1) return p;
    if (lead == BATCH_LEAD_EQUAL) {
        const int Bp = (int)(((long long)batch + parts - 1) / parts);
        p.n = 0;
        for (int i = 0; i < parts && (long long)i * Bp < batch; ++i) {
            p.r0[i] = i * Bp;
            p.rows[i] = batch - i * Bp < Bp ? batch - i * Bp : Bp;
            p.n = i + 1;
        }
        return p;
    }
    if (batch < 4 * parts) return p;
    lead = lead < BATCH_LEAD_MIN ? BATCH_LEAD_MIN : lead > BATCH_LEAD_MAX ? BATCH_LEAD_MAX : lead;
    int r = 0;
    for (int i = 0; i < parts; ++i) {
        const int k = parts - i, left = batch - r;
        int take = left;
        if (k > 1) {
            // nearest multiple of 4 to left * lead / (8 k), in 64 bits (batch is any int)
            const long long num = (long long)left * lead, den = 8LL * k;
            take = (int)((2 * num + 4 * den) / (8 * den)) * 4;
            const int hi = (left - 4 * (k - 1)) & ~3;      // the later parts keep 4 rows each
            take = take < 4 ? 4 : take > hi ? hi : take;
        }
        p.r0[i] = r;
        p.rows[i] = take;
        r += take;
    }
    p.n = parts;
    return p;
}

// rows twin `twin` (part twin + 1) must hold on an engine created for calls of up to max_batch clips: the largest part it is
// given by any call the engine splits
inline int batch_parts_twin_rows(int max_batch, int ntwins, int lead, int twin) {
    int m = 0;
    for (int b = BATCH_SPLIT_MIN; b <= max_batch; ++b) {
        const BatchParts p = batch_parts_cut(b, batch_parts_count(b, ntwins), lead);
        if (twin + 1 < p.n && p.rows[twin + 1] > m) m = p.rows[twin + 1];
    }
    return m;
}

}  // namespace se

// kta_fold.h — the fold of the scan's partial rows into the persistent vectors, once: the body of
// kta_fold_partials (kta_kernels.hip).
// Layout of vec: u64[P*7] (reference field order) followed by KTA_NGLOBALS globals (include/kta_hip.h).  A thread sums one
// column of the workspace over the rows it is given (consecutive threads read consecutive words), then one device-scope
// integer atomic per (thread, output).  Integer atomics commute => exact, whoever folds which rows and when.
// The rows are read kFoldLoads at a time: the loads are issued together and then combined, so that a thread has that
// many in flight instead of one dependent-looking load after another.
#pragma once

#include <limits.h>

#include "kta_fold_groups.h"
#include "kta_kernels.h"

#ifndef KTA_FOLD_LOADS
#define KTA_FOLD_LOADS 32
#endif

namespace kta {

constexpr uint32_t kFoldLoads = KTA_FOLD_LOADS;   // a thread's loads in flight (profiles/fold_wide_groups.jsonl)
enum FoldOp : int { FOLD_SUM = 0, FOLD_MIN = 1, FOLD_MAX = 2 };   // (the extrema are signed)

// Column `col` of the rows [r0, r1), combined by OP.
template <int OP>
__device__ __forceinline__ unsigned long long fold_column(const uint64_t *partials, uint32_t r0, uint32_t r1, uint32_t row_len,
                                                          uint32_t col)
{
    const unsigned long long none = OP == FOLD_SUM ? 0ull : OP == FOLD_MIN ? (unsigned long long)LLONG_MAX : (unsigned long long)LLONG_MIN;
    unsigned long long acc = none;
    for (uint32_t r = r0; r < r1; r += kFoldLoads) {
        unsigned long long x[kFoldLoads];
#pragma unroll
        for (uint32_t k = 0; k < kFoldLoads; k++) x[k] = r + k < r1 ? partials[(uint64_t)(r + k) * row_len + col] : none;
#pragma unroll
        for (uint32_t k = 0; k < kFoldLoads; k++) {
            if (OP == FOLD_SUM) acc += x[k];
            else if (OP == FOLD_MIN) acc = (long long)x[k] < (long long)acc ? x[k] : acc;
            else acc = (long long)x[k] > (long long)acc ? x[k] : acc;
        }
    }
    return acc;
}

// Column `col` (below row_len) of the rows [r0, r1) (r0 < r1) of `partials` into vec / avec (null: no analytics tail in
// the rows).
__device__ __forceinline__ void fold_rows(const uint64_t *partials, uint32_t r0, uint32_t r1, uint32_t P, uint64_t *vec,
                                          uint32_t row_len, uint64_t *avec, uint32_t col)
{
    const uint32_t base_len = P * kScanCols + kScanGlobals;
    unsigned long long *v = reinterpret_cast<unsigned long long *>(vec);
    unsigned long long *g = v + (uint64_t)P * 7;
    if (col >= base_len) {
        // analytics tail of the row: [P][4] signed-max extrema, then 2 x 34 histogram sums.
        // avec layout: [2 x 34 histogram][P][4 extrema]
        const uint32_t a = col - base_len;
        if (a < 4u * P) {
            const long long m = (long long)fold_column<FOLD_MAX>(partials, r0, r1, row_len, col);
            atomicMax(reinterpret_cast<long long *>(avec) + kAnalyticsHist + a, m);
        } else {
            const unsigned long long t = fold_column<FOLD_SUM>(partials, r0, r1, row_len, col);
            if (t) atomicAdd(reinterpret_cast<unsigned long long *>(avec) + (a - 4u * P), t);
        }
        return;
    }
    if (col < P * kScanCols) {
        const uint32_t p = col / kScanCols, f = col % kScanCols;
        const unsigned long long s = fold_column<FOLD_SUM>(partials, r0, r1, row_len, col);
        if (s == 0) return;
        unsigned long long *o = v + (uint64_t)p * 7;
        switch (f) {
        case 0: // record count: total += s, alive += s, key_non_null += s, records += s
            atomicAdd(&o[0], s);
            atomicAdd(&o[2], s);
            atomicAdd(&o[4], s);
            atomicAdd(&g[2], s);
            break;
        case 1: // tombstones: tombstones += s, alive -= s   (alive = total - tombstones)
            atomicAdd(&o[1], s);
            atomicAdd(&o[2], 0ull - s);
            break;
        case 2: // key None: key_null += s, key_non_null -= s
            atomicAdd(&o[3], s);
            atomicAdd(&o[4], 0ull - s);
            break;
        case 3: atomicAdd(&o[5], s); break; // key_size_sum
        default: atomicAdd(&o[6], s); break; // value_size_sum
        }
        return;
    }
    // the row's globals; the three list words (kta_kernels.hip: kScanListA ...) are read by no fold
    const uint32_t gi = col - P * kScanCols;
    long long *gs = reinterpret_cast<long long *>(g);
    if (gi == SG_TMIN || gi == SG_SMIN) { // minima are kept bit-complemented: all four are MAX
        const long long m = (long long)fold_column<FOLD_MIN>(partials, r0, r1, row_len, col);
        atomicMax(&gs[gi == SG_TMIN ? 4 : 6], ~m);
    } else if (gi == SG_TMAX || gi == SG_SMAX) {
        const long long m = (long long)fold_column<FOLD_MAX>(partials, r0, r1, row_len, col);
        atomicMax(&gs[gi == SG_TMAX ? 5 : 7], m);
    } else if (gi == SG_BAD) {
        const unsigned long long s = fold_column<FOLD_SUM>(partials, r0, r1, row_len, col);
        if (s) atomicAdd(&g[0], s);
    }
}

}   // namespace kta

// kta_fold_groups.h — the group rule of the fold of the scan's partial rows (kta_fold.h), once.
// The `rows` rows of a partial workspace are folded in groups of kFoldGroupRows consecutive rows; the last group may be
// short.  A group is what one workgroup of kta_fold_partials folds of its columns: launch_fold_partials makes a row slice
// of every group.
// Plain C++ as well as HIP, host and device (tests/native/fold_groups_check.cpp): no HIP runtime call, no LDS.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define KTA_FOLD_HD __host__ __device__
#else
#define KTA_FOLD_HD
#endif

#ifndef KTA_FOLD_GROUP_ROWS
#define KTA_FOLD_GROUP_ROWS 64
#endif

namespace kta {

// Rows of a group.  The fold's time on one MI355X is about 0.056 us per workgroup of its grid plus the chain of a thread's
// load blocks (kta_fold.h: kFoldLoads rows each), not the 13 MB it reads: 64 rows — 20 groups x 6 column blocks for the
// flagship's 1280 rows — are the best of 8, 32, 64, 128 and 256 (profiles/fold_wide_groups.jsonl).
constexpr uint32_t kFoldGroupRows = KTA_FOLD_GROUP_ROWS;
static_assert(kFoldGroupRows >= 1, "a group has rows");

// The number of groups of `rows` rows.
KTA_FOLD_HD inline uint32_t fold_groups(uint32_t rows) { return rows / kFoldGroupRows + (rows % kFoldGroupRows != 0u ? 1u : 0u); }

// The group of row `row`.
KTA_FOLD_HD inline uint32_t fold_group_of(uint32_t row) { return row / kFoldGroupRows; }

// The rows [r0, r1) of group `group` of `rows` rows (group < fold_groups(rows)).
KTA_FOLD_HD inline void fold_group_rows(uint32_t group, uint32_t rows, uint32_t &r0, uint32_t &r1)
{
    r0 = group * kFoldGroupRows;
    r1 = rows - r0 < kFoldGroupRows ? rows : r0 + kFoldGroupRows;
}

}   // namespace kta

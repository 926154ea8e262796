// kta_filter.h — the rules of the record filter (kta_set_filter, include/kta_hip.h states them; this is their code), once:
// which record passes, what a tile's header and summary decide without reading a record, and the order-preserving rank of
// a passing record inside its tile.  Plain C++ for host and device: the kernels of kta_filter.hip, the host helper
// kta_filter_host and tests/native/filter_check.cpp all call this text.  No HIP runtime call, no LDS.
#pragma once

#include <stdint.h>

#include "kta_hip.h"
#include "kta_tile.h"

namespace kta {

// from_ms == INT64_MIN / to_ms == INT64_MAX: no bound on that side.  parts: a partition set is given (the bitmap has
// ceil(P / 32) words, bit p of word p / 32 for partition p).
struct FilterSpec {
    int64_t from_ms, to_ms;
    uint32_t P;
    uint32_t parts;
};

KTA_TILE_HD inline bool filter_timed(const FilterSpec &f) { return f.from_ms != INT64_MIN || f.to_ms != INT64_MAX; }
KTA_TILE_HD inline uint32_t filter_bitmap_words(uint32_t P) { return (P + 31u) / 32u; }

// The time test alone, on the raw i64 milliseconds.  A record without a timestamp (-1) fails as soon as a bound is set.
KTA_TILE_HD inline bool filter_time_passes(const FilterSpec &f, int64_t ts_ms)
{
    if (!filter_timed(f)) return true;
    if (ts_ms == -1) return false;
    return ts_ms >= f.from_ms && (f.to_ms == INT64_MAX || ts_ms < f.to_ms);
}

// The record predicate.  bitmap is read only when f.parts: a partition outside [0, P) is in no set.
KTA_TILE_HD inline bool filter_record_passes(const FilterSpec &f, const uint32_t *bitmap, int32_t partition, int64_t ts_ms)
{
    if (f.parts) {
        if ((uint32_t)partition >= f.P) return false;
        if (!((bitmap[(uint32_t)partition >> 5] >> ((uint32_t)partition & 31u)) & 1u)) return false;
    }
    return filter_time_passes(f, ts_ms);
}

// What a tile's header and summary decide for all of its 1024 records at once.
enum FilterTile : uint32_t {
    FILTER_TILE_READ = 0,   // nothing: the records are read
    FILTER_TILE_NONE = 1,   // no record of the tile passes
    FILTER_TILE_ALL = 2     // every record of the tile passes
};

// whole: the tile's 1024 records all belong to the slice.  The conditions under which a summary is looked at are the
// packed scan's: a COMPACT header, a VALID summary, a whole tile.  Then
//   NONE  a time bound is set and the tile has no timestamp other than -1, or its timed span [ts_base, ts_base + ts_span]
//         lies wholly outside the window (its records of -1 fail anyway);
//   ALL   a time bound is set, the span lies wholly inside the window, the tile has no record of -1, no partition set is
//         given and every stored partition is a real one (part_max < min(P, 0xFFFF)).
// With a partition set only NONE is ever answered.
KTA_TILE_HD inline FilterTile filter_tile_decide(const FilterSpec &f, const kta_tile_hdr &h, const kta_tile_sum &s, bool whole)
{
    if (!whole || h.mode != KTA_TILE_COMPACT || !(s.flags & KTA_TILE_SUM_VALID) || !filter_timed(f)) return FILTER_TILE_READ;
    if (!(s.flags & KTA_TILE_SUM_TIMED)) return FILTER_TILE_NONE;
    const int64_t lo = h.ts_base, hi = (int64_t)((uint64_t)h.ts_base + (uint64_t)s.ts_span);
    if (hi < f.from_ms || (f.to_ms != INT64_MAX && lo >= f.to_ms)) return FILTER_TILE_NONE;
    const bool inside = lo >= f.from_ms && (f.to_ms == INT64_MAX || hi < f.to_ms);
    const uint32_t part_lim = f.P < KTA_COMPACT_PART_NONE ? f.P : KTA_COMPACT_PART_NONE;
    if (inside && !(s.flags & KTA_TILE_SUM_UNTIMED) && !f.parts && (uint32_t)s.part_max < part_lim) return FILTER_TILE_ALL;
    return FILTER_TILE_READ;
}

// The tiles of a slice: records [a0, a0 + n) of an allocation (a0 = 0 for the raw layout) lie in the layout tiles
// T0 .. T0 + tiles - 1, and tile t of the slice is the part of layout tile T0 + t inside the slice — so a view that
// starts inside a tile cuts its first and last tile, and the ones between keep their summaries.
KTA_TILE_HD inline uint64_t filter_slice_tiles(uint64_t a0, uint64_t n)
{
    return n == 0 ? 0 : (a0 + n - 1) / KTA_TILE_RECORDS - a0 / KTA_TILE_RECORDS + 1;
}

// The rank of a wave's lane among the passing lanes of one 64-record instruction: the passing lanes below it
// (v_mbcnt_lo / _hi on the device).  ballot: the instruction's passing lanes.
KTA_TILE_HD inline uint32_t filter_lane_rank(uint64_t ballot, uint32_t lane)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)lane;
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
#else
    return (uint32_t)__builtin_popcountll(ballot & ((1ull << lane) - 1ull));
#endif
}

// A tile is taken by four waves: wave w holds the tile's records [256 w, 256 w + 256) in four instructions of 64, record
// 256 w + 64 k + lane in instruction k.  With the four ballots of a wave and the totals of the waves below it, the rank
// of the record of (k, lane) among the tile's passing records, in record order:
KTA_TILE_HD inline uint32_t filter_tile_rank(uint32_t wave_base, const uint64_t (&ballot)[4], uint32_t k, uint32_t lane)
{
    uint32_t r = wave_base;
    for (uint32_t q = 0; q < k; q++) r += (uint32_t)__builtin_popcountll(ballot[q]);
    return r + filter_lane_rank(ballot[k], lane);
}

} // namespace kta

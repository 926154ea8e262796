// kta_plane_pack.h — the words the plane loop of the lean scan kernel adds to the front level (kta_kernels.hip:
// lean_quad(PlaneSlot), PackedWg::front_flush(raw)), once: the fields, their bounds, the interval that keeps them, pack
// and unpack.
// A plane record is pt | ku << 8 | vu << 16 (kta_tile.h): ku <= 0xFF with 0xFF for a key of -1, vu <= 0xFFFF with 0xFFFF
// for a value of -1.  The lengths are added RAW, markers included; the flush takes them out by the flag counts.
//   main word   ONE 64-bit add per record into W1[slot]:   1 | ku << 14 | (u64)vu << 35
//               as dwords: low = 1 | ku << 14, high = vu << 3 (no 64-bit shift).  Fields: count (14 bits), raw key sum
//               (21 bits), raw value sum (29 bits) — 64 bits in all.
//   flag word   ONE 32-bit add into the low dword of W2[slot], by the lanes where it is not zero:   knull | tomb << 16
// A uniform quad (a lane's four records of one partition) adds the sums of its four records' words in one add each.
// The bound.  Slot (p, r) takes records only from the kWG / R threads of replica r (rep = tid & (R - 1)): at most
// 1024 / R records per tile.  A plane interval is min(kFrontFlushTiles, 8 R) taken tiles, so a slot takes at most 8192
// records between two flushes — the asserts below — and the flush unpacks EVERY replica before it sums: the replicas'
// sum obeys no field's bound.
// Plain C++ as well as HIP, host and device (tests/native/plane_pack_check.cpp): no HIP runtime call, no LDS.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define KTA_PLANE_HD __host__ __device__
#else
#define KTA_PLANE_HD
#endif

namespace kta {

constexpr uint32_t kPlaneTileRecords = 1024;      // KTA_TILE_RECORDS: 256 threads x 4 records
constexpr uint32_t kPlaneKeyNone = 0xFFu;         // KTA_PLANE_KEY_NONE
constexpr uint32_t kPlaneValNone = 0xFFFFu;       // KTA_COMPACT_LEN_NONE
constexpr uint32_t kPlaneCountBits = 14, kPlaneKeyBits = 21, kPlaneValBits = 29;
constexpr uint32_t kPlaneKeyShift = kPlaneCountBits;                    // 14, in the low dword
constexpr uint32_t kPlaneValShift = kPlaneCountBits + kPlaneKeyBits;    // 35: 3 in the high dword
constexpr uint32_t kPlaneTombShift = 16;                                // in the flag word
constexpr uint64_t kPlaneSlotRecords = 8192;      // what a slot takes in one plane interval, at most

// The tiles a workgroup takes between two flushes of the plane form (uniform): min(front_flush_tiles, 8 R).
KTA_PLANE_HD constexpr uint32_t plane_interval_tiles(uint32_t rep_log2, uint32_t front_flush_tiles)
{
    return rep_log2 >= 2u ? front_flush_tiles : (8u << rep_log2 < front_flush_tiles ? 8u << rep_log2 : front_flush_tiles);
}
// The records slot (p, r) can take in such an interval: the interval's tiles x the records of replica r's threads.
KTA_PLANE_HD constexpr uint64_t plane_slot_records(uint32_t rep_log2, uint32_t front_flush_tiles)
{
    return (uint64_t)plane_interval_tiles(rep_log2, front_flush_tiles) * (kPlaneTileRecords >> rep_log2);
}

static_assert(kPlaneCountBits + kPlaneKeyBits + kPlaneValBits == 64, "the main word's three fields fill 64 bits");
static_assert(kPlaneValShift - 32u == 3u && kPlaneKeyShift + kPlaneKeyBits > 32u, "the value sum begins at bit 3 of the high dword");
static_assert(plane_slot_records(0, 32) == kPlaneSlotRecords && plane_slot_records(1, 32) == kPlaneSlotRecords &&
              plane_slot_records(2, 32) == kPlaneSlotRecords && plane_slot_records(3, 32) <= kPlaneSlotRecords &&
              plane_slot_records(6, 32) <= kPlaneSlotRecords, "a slot takes at most 8192 records per plane interval");
static_assert(plane_interval_tiles(0, 32) == 8 && plane_interval_tiles(1, 32) == 16 && plane_interval_tiles(2, 32) == 32 &&
              plane_interval_tiles(6, 32) == 32, "8, 16, then 32 tiles");
static_assert(kPlaneSlotRecords < (1ull << kPlaneCountBits), "the count of a plane interval fits 14 bits");
static_assert(kPlaneSlotRecords * kPlaneKeyNone < (1ull << kPlaneKeyBits), "its raw key sum (2 088 960) fits 21 bits");
static_assert(kPlaneSlotRecords * kPlaneValNone < (1ull << kPlaneValBits), "its raw value sum (536 862 720) fits 29 bits");
static_assert(kPlaneSlotRecords < (1ull << kPlaneTombShift), "null keys and tombstones fit 16 bits each");

// What one add carries: the main word as its two dwords, and the flag word (0: the add is left out).
struct PlaneAdd {
    uint32_t lo, hi, flags;
};
KTA_PLANE_HD inline uint64_t plane_word(const PlaneAdd &a)
{
    return ((uint64_t)a.hi << 32) | a.lo;
}
// n records of one slot whose stored lengths sum to ku and vu, knulls of them without a key, tombs without a value
// (a record: n = 1; a uniform quad: n = 4).
KTA_PLANE_HD inline PlaneAdd plane_pack(uint32_t n, uint32_t ku, uint32_t vu, uint32_t knulls, uint32_t tombs)
{
    return PlaneAdd{n | (ku << kPlaneKeyShift), vu << (kPlaneValShift - 32u), knulls | (tombs << kPlaneTombShift)};
}
KTA_PLANE_HD inline PlaneAdd plane_pack_record(uint32_t ku, uint32_t vu)
{
    return plane_pack(1u, ku, vu, ku == kPlaneKeyNone, vu == kPlaneValNone);
}

// The five sums of an interval, per partition: what the flush adds to the back level.
struct PlaneSums {
    uint64_t cnt = 0, tb = 0, kn = 0, ks = 0, vs = 0;   // ks, vs: raw until plane_corrected
};
// One replica's two words into the sums (each replica on its own: only a single slot's fields are bounded).
KTA_PLANE_HD inline void plane_unpack(PlaneSums &s, uint64_t w, uint64_t f)
{
    s.cnt += w & ((1ull << kPlaneCountBits) - 1ull);
    s.ks += (w >> kPlaneKeyShift) & ((1ull << kPlaneKeyBits) - 1ull);
    s.vs += w >> kPlaneValShift;
    s.kn += f & ((1ull << kPlaneTombShift) - 1ull);
    s.tb += (f >> kPlaneTombShift) & 0xFFFFull;
}
// The markers out of the raw sums: every null key added 0xFF, every tombstone 0xFFFF.
KTA_PLANE_HD inline void plane_corrected(PlaneSums &s)
{
    s.ks -= (uint64_t)kPlaneKeyNone * s.kn;
    s.vs -= (uint64_t)kPlaneValNone * s.tb;
}

}   // namespace kta

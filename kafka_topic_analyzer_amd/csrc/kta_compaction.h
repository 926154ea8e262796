// kta_compaction.h — the compaction what-if (KTA_FLAG_COMPACTION, include/kta_hip.h): the one statement of which replayed
// record log compaction would keep, the layout of the result vector and the packing of the pass's LDS words.  Shared by
// the kernel (kta_compaction.hip), the host code that reads the vector and the stand-alone check
// (tests/native/compaction_check.cpp): plain C++, no HIP header.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KTA_COMPACTION_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define KTA_COMPACTION_HD inline
#endif

namespace kta {

// What a replayed record is to the cleaner.
enum CompactionClass : uint32_t {
    kCompactionUnkeyed = 0,           // key None: compaction goes by key
    kCompactionSuperseded,            // a later record of the slot was seen by the first pass: adds nothing
    kCompactionUnknown,               // the table never saw this record: the replay does not match the first pass
    kCompactionLive,                  // survives, value Some, partition in [0, P)
    kCompactionTombstone,             // survives, value None, partition in [0, P): kept until delete.retention.ms
    kCompactionLiveOutside,           // survives, value Some, partition outside [0, P)
    kCompactionTombstoneOutside,      // survives, value None, partition outside [0, P)
    kCompactionClasses
};

// The value the alive-key pass writes for a record of sequence number s (kta_alive.hip): ((s + 1) << 1) | alive.
KTA_COMPACTION_HD uint64_t compaction_value(uint64_t s, int32_t val_len) { return ((s + 1u) << 1) | (val_len >= 0 ? 1u : 0u); }

// THE RULE.  entry: the record's slot table[fnv1a(key)] after the first pass.  A record survives exactly when the value it
// would write is the value its slot holds.
KTA_COMPACTION_HD CompactionClass compaction_classify(uint64_t entry, uint64_t s, int32_t key_len, int32_t val_len, int32_t partition,
                                                      uint32_t P)
{
    if (key_len < 0) return kCompactionUnkeyed;
    const uint64_t v = compaction_value(s, val_len);
    if (entry > v) return kCompactionSuperseded;
    if (entry < v) return kCompactionUnknown;
    const bool inside = (uint32_t)partition < P;   // (a negative partition is a large unsigned one)
    if (val_len >= 0) return inside ? kCompactionLive : kCompactionLiveOutside;
    return inside ? kCompactionTombstone : kCompactionTombstoneOutside;
}

// The result vector u64[5 P + 6]: word 5 p + k of partition p, then the globals.
enum : uint32_t {
    kCompactionLiveRecords = 0, kCompactionLiveKeyBytes = 1, kCompactionLiveValueBytes = 2, kCompactionTombstoneRecords = 3,
    kCompactionTombstoneKeyBytes = 4, kCompactionWords = 5
};
enum : uint32_t {
    kCompactionReplayed = 0, kCompactionUnkeyedRecords = 1, kCompactionUnknownRecords = 2, kCompactionLiveOutsideRecords = 3,
    kCompactionTombstonesOutsideRecords = 4, kCompactionReserved = 5, kCompactionGlobals = 6
};
KTA_COMPACTION_HD size_t compaction_len(uint32_t P) { return (size_t)kCompactionWords * P + kCompactionGlobals; }

// The pass's LDS words of a partition, 32 B: W0 = live_records | tombstone_records << 32 (a launch takes at most 2^30
// records: no half overflows), W1 = live_key_bytes, W2 = live_value_bytes, W3 = tombstone_key_bytes.
enum : uint32_t { kCompactionLdsWords = 4 };
constexpr uint64_t kCompactionLaunchMax = 1ull << 30;
KTA_COMPACTION_HD uint64_t compaction_w0(bool live) { return live ? 1ull : 1ull << 32; }
KTA_COMPACTION_HD uint64_t compaction_w0_live(uint64_t w0) { return w0 & 0xFFFFFFFFull; }
KTA_COMPACTION_HD uint64_t compaction_w0_tombstones(uint64_t w0) { return w0 >> 32; }

} // namespace kta

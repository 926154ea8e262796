// kta_compact_delete.h — the compact,delete what-if (kta_set_compact_delete, include/kta_hip.h): the one statement of the
// kept state a replayed record advances, the kept vector's layout and its identities with the segment vector and the
// compaction vector of the same records, and the what-if walk.  A record's size, its segment and the record that closes a
// row are kta_segments.h's, its class kta_compaction.h's: nothing of either is said again here.  Shared by the kernels
// (kta_compaction.hip writes the class byte, kta_segments.hip the kept rows), the host code that reads the vectors and the
// stand-alone check (tests/native/compact_delete_check.cpp): plain C++, no HIP header.
#pragma once

#include "kta_compaction.h"
#include "kta_segments.h"

namespace kta {

// ---- the kept vector u64[(P*M + P) * 4 + 8] ------------------------------------------------------------------------
// The segment vector's shape and helpers (segments_row_at, segments_total_at, segments_globals_at, segments_len).  A row
// and a total are {L, B, T, K} in the places of {C, B, T, H + 1}: the live records and the tombstones compaction keeps,
// and their bytes K, of the partition's log up to position B.  The globals are the segment vector's.
enum : uint32_t { kKeptL = kSegC, kKeptB = kSegB, kKeptT = kSegT, kKeptK = kSegH1 };

// The class byte of a replayed record, as the compaction kernel stores it for the kept-row kernels.
enum : uint8_t { kKeptClassNone = 0, kKeptClassLive = 1, kKeptClassTombstone = 2 };
KTA_SEGMENTS_HD uint8_t kept_class_byte(CompactionClass k)
{
    return k == kCompactionLive ? kKeptClassLive : k == kCompactionTombstone ? kKeptClassTombstone : kKeptClassNone;
}

constexpr uint32_t kCompactDeleteMaxPartitions = 2048;     // the smaller of the two passes' bounds (kta_kernels.h)
constexpr uint64_t kCompactDeleteScratchBytes = 128ull << 20;   // the class column: a byte per record of a replay slice

// ---- THE RULE -----------------------------------------------------------------------------------------------------
// The definition as the sequential loop it is (the stand-alone check runs this; the kernels reach the same words with
// prefix sums).  vec: segments_len(P, M) words, made by segments_init.  cls: the record's kept_class_byte.
inline void kept_apply_record(uint64_t *vec, uint32_t P, uint32_t M, int32_t partition, int32_t key_len, int32_t val_len, uint8_t cls)
{
    uint64_t *g = vec + segments_globals_at(P, M);
    const uint64_t S = g[kSegGlobalS];
    if ((uint32_t)partition >= P) {
        g[kSegGlobalBadPartition]++;
        return;
    }
    g[kSegGlobalRecords]++;
    uint64_t *t = vec + segments_total_at(P, M, (uint32_t)partition);
    const uint64_t before = t[kKeptB], z = segments_record_size((uint32_t)g[kSegGlobalOverhead], key_len, val_len);
    t[kKeptB] += z;
    if (cls == kKeptClassLive) t[kKeptL] += 1, t[kKeptK] += z;
    if (cls == kKeptClassTombstone) t[kKeptT] += 1, t[kKeptK] += z;
    uint32_t row;
    if (segments_closes(before, t[kKeptB], S, M, &row)) {
        uint64_t *r = vec + segments_row_at((uint32_t)partition, M, row);
        for (uint32_t k = 0; k < kSegWords; k++) r[k] = t[k];
        g[kSegGlobalClosed]++;
    }
}

// ---- identities ---------------------------------------------------------------------------------------------------
// seg: the first pass's segment vector; kept: the replay's kept vector; comp: the replay's compaction vector
// u64[compaction_len(P)].  All hold exactly when the replay was handed the records of the first pass, in its order.
inline bool compact_delete_identities_hold(const uint64_t *seg, const uint64_t *kept, const uint64_t *comp, uint32_t P, uint32_t M)
{
    const uint64_t *gs = seg + segments_globals_at(P, M), *gk = kept + segments_globals_at(P, M);
    bool ok = comp[(size_t)kCompactionWords * P + kCompactionUnknownRecords] == 0;
    for (uint32_t k = kSegGlobalRecords; k <= kSegGlobalOverhead; k++) ok = ok && gs[k] == gk[k];
    const uint64_t overhead = gs[kSegGlobalOverhead];
    for (uint32_t p = 0; p < P && ok; p++) {
        const uint64_t *ts = seg + segments_total_at(P, M, p), *tk = kept + segments_total_at(P, M, p), *c = comp + (size_t)kCompactionWords * p;
        ok = ok && tk[kKeptB] == ts[kSegB] && tk[kKeptL] == c[kCompactionLiveRecords] && tk[kKeptT] == c[kCompactionTombstoneRecords];
        ok = ok && tk[kKeptK] == overhead * (tk[kKeptL] + tk[kKeptT]) + c[kCompactionLiveKeyBytes] + c[kCompactionLiveValueBytes] +
                                     c[kCompactionTombstoneKeyBytes];
        uint64_t l = 0, t = 0, kk = 0;
        for (uint32_t s = 0; s < M && ok; s++) {
            const uint64_t *rs = seg + segments_row_at(p, M, s), *rk = kept + segments_row_at(p, M, s);
            const bool closed = rs[kSegC] != 0;                  // (a record closed it: at least that one is counted)
            ok = ok && closed == (rk[kKeptB] != 0) && rk[kKeptB] == rs[kSegB];
            if (!closed) continue;
            ok = ok && rk[kKeptL] >= l && rk[kKeptT] >= t && rk[kKeptK] >= kk;
            l = rk[kKeptL], t = rk[kKeptT], kk = rk[kKeptK];
        }
        ok = ok && tk[kKeptL] >= l && tk[kKeptT] >= t && tk[kKeptK] >= kk;
    }
    return ok;
}

// ---- the what-if --------------------------------------------------------------------------------------------------
// out[(P + 1)][kCdWords]: a row per partition and one for the topic (the sums; its rule word is the OR of the partitions'
// and its clamped word their count).
enum : uint32_t {
    kCdRecords = 0, kCdBytes,                    // now
    kCdCompactedRecords, kCdCompactedBytes,      // after compaction alone: the cleaned prefix plus the active segment whole
    kCdKeptRecords, kCdKeptBytes,                // under compact,delete
    kCdKeptTombstones,
    kCdSegmentsDeleted,
    kCdRule,                                     // as kRetRule
    kCdClamped,                                  // as kRetClamped
    kCdWords
};
// The size rule on compacted sizes: what the log holds after cleaning, less the kept bytes up to and including row k.
KTA_SEGMENTS_HD bool compact_delete_size_takes(const uint64_t *kept_row, uint64_t compacted_bytes, int64_t retention_bytes)
{
    return retention_bytes >= 0 && compacted_bytes - kept_row[kKeptK] >= (uint64_t)retention_bytes;
}
inline void compact_delete_whatif(const uint64_t *seg, const uint64_t *kept, uint32_t P, uint32_t M, int64_t now_ms, int64_t retention_ms,
                                  int64_t retention_bytes, uint64_t *out)
{
    static const uint64_t kZero[kSegWords] = {0, 0, 0, 0};
    const uint64_t S = seg[segments_globals_at(P, M) + kSegGlobalS];
    uint64_t *all = out + (size_t)P * kCdWords;
    for (uint32_t k = 0; k < kCdWords; k++) all[k] = 0;
    for (uint32_t p = 0; p < P; p++) {
        const uint64_t *t = seg + segments_total_at(P, M, p);
        uint64_t *o = out + (size_t)p * kCdWords;
        const uint64_t *last = kZero, *klast = kZero;            // the last closed row, of both vectors
        for (uint32_t s = 0; s + 1 < M; s++)
            if (seg[segments_row_at(p, M, s) + kSegC] != 0) last = seg + segments_row_at(p, M, s), klast = kept + segments_row_at(p, M, s);
        // the active segment: never cleaned, never deleted
        const uint64_t a_records = t[kSegC] - last[kSegC], a_bytes = t[kSegB] - last[kSegB], a_tombstones = t[kSegT] - last[kSegT];
        const uint64_t compacted_bytes = klast[kKeptK] + a_bytes;
        const uint64_t *kcut = kZero;                            // the kept row of the last deleted one
        uint64_t deleted = 0, by_time = 0, by_size = 0;
        bool walking = true, timing = true, sizing = true;
        for (uint32_t s = 0; s + 1 < M; s++) {
            const uint64_t *r = seg + segments_row_at(p, M, s), *rk = kept + segments_row_at(p, M, s);
            if (r[kSegC] == 0) continue;
            timing = timing && retention_time_takes(r, now_ms, retention_ms);
            sizing = sizing && compact_delete_size_takes(rk, compacted_bytes, retention_bytes);
            by_time += timing, by_size += sizing;
            walking = walking && (timing || sizing);             // (each rule's rows are a prefix: H and K only grow)
            if (walking) deleted++, kcut = rk;
        }
        o[kCdRecords] = t[kSegC], o[kCdBytes] = t[kSegB];
        o[kCdCompactedRecords] = klast[kKeptL] + klast[kKeptT] + a_records;
        o[kCdCompactedBytes] = compacted_bytes;
        o[kCdKeptRecords] = o[kCdCompactedRecords] - (kcut[kKeptL] + kcut[kKeptT]);
        o[kCdKeptBytes] = compacted_bytes - kcut[kKeptK];
        o[kCdKeptTombstones] = klast[kKeptT] - kcut[kKeptT] + a_tombstones;
        o[kCdSegmentsDeleted] = deleted;
        o[kCdRule] = deleted == 0 ? 0u : by_time >= by_size ? 1u : 2u;
        o[kCdClamped] = t[kSegB] / S >= (uint64_t)(M - 1u) ? 1u : 0u;
        for (uint32_t k = 0; k < kCdWords; k++) {
            if (k == kCdRule) all[k] |= o[k];
            else all[k] += o[k];
        }
    }
}

} // namespace kta

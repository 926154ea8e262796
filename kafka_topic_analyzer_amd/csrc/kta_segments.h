// kta_segments.h — the retention what-if (kta_set_segments, include/kta_hip.h): the one statement of a record's model
// size, of the segment a byte offset falls into and of the record that closes a row, the layout of the result vector, its
// identities with the counter vector, the merge and the what-if walk.  Shared by the kernels (kta_segments.hip, through
// kta_segments_wave.h), the host code that reads the vector and the stand-alone check (tests/native/segments_check.cpp):
// plain C++, no HIP header.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KTA_SEGMENTS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define KTA_SEGMENTS_HD inline
#endif

namespace kta {

// ---- configuration ------------------------------------------------------------------------------------------------
constexpr uint64_t kSegmentsMaxBytes = 1ull << 40;     // S at most
constexpr uint64_t kSegmentsMaxRows = 1ull << 20;      // P * M at most
KTA_SEGMENTS_HD bool segments_config_ok(uint64_t S, uint64_t M, uint64_t P)
{
    return S >= 1 && S <= kSegmentsMaxBytes && M >= 2 && P >= 1 && P <= kSegmentsMaxRows && M <= kSegmentsMaxRows && P * M <= kSegmentsMaxRows;
}

// ---- the vector u64[(P*M + P) * 4 + 8] ----------------------------------------------------------------------------
// rows [p*M + s][4] | totals [P][4] | 8 globals.  A row and a total are {C, B, T, H + 1}: records, bytes, tombstones and
// the largest timestamp (0: none) of the partition up to and including the record that wrote the row / the last record.
enum : uint32_t { kSegC = 0, kSegB = 1, kSegT = 2, kSegH1 = 3, kSegWords = 4 };
enum : uint32_t {
    kSegGlobalRecords = 0, kSegGlobalBadPartition = 1, kSegGlobalClosed = 2, kSegGlobalS = 3, kSegGlobalM = 4, kSegGlobalOverhead = 5,
    kSegGlobals = 8
};
KTA_SEGMENTS_HD size_t segments_row_at(uint32_t p, uint32_t M, uint32_t s) { return ((size_t)p * M + s) * kSegWords; }
KTA_SEGMENTS_HD size_t segments_total_at(uint32_t P, uint32_t M, uint32_t p) { return ((size_t)P * M + p) * kSegWords; }
KTA_SEGMENTS_HD size_t segments_globals_at(uint32_t P, uint32_t M) { return ((size_t)P * M + P) * kSegWords; }
KTA_SEGMENTS_HD size_t segments_len(uint32_t P, uint32_t M) { return segments_globals_at(P, M) + kSegGlobals; }

// ---- THE RULE -----------------------------------------------------------------------------------------------------
// a record's model size
KTA_SEGMENTS_HD uint64_t segments_record_size(uint32_t overhead, int32_t key_len, int32_t val_len)
{
    return (uint64_t)overhead + (uint64_t)(key_len > 0 ? key_len : 0) + (uint64_t)(val_len > 0 ? val_len : 0);
}
// a timestamp's word: ts + 1, 0 for "not available" (every negative one)
KTA_SEGMENTS_HD uint64_t segments_ts_word(int64_t ts_ms) { return ts_ms >= 0 ? (uint64_t)ts_ms + 1u : 0u; }
// the segment (row) the byte at offset b of a partition's log falls into
KTA_SEGMENTS_HD uint32_t segments_index(uint64_t b, uint64_t S, uint32_t M)
{
    const uint64_t s = b / S;
    return s < (uint64_t)(M - 1u) ? (uint32_t)s : M - 1u;
}
// the least offset behind b whose segment is another one (UINT64_MAX: none, b lies in the last row)
KTA_SEGMENTS_HD uint64_t segments_next_boundary(uint64_t b, uint64_t S, uint32_t M)
{
    const uint64_t s = b / S;
    return s < (uint64_t)(M - 1u) ? (s + 1u) * S : UINT64_MAX;
}
// A record whose partition held b_before bytes before it and b_after behind it closes row *row exactly when this holds.
KTA_SEGMENTS_HD bool segments_closes(uint64_t b_before, uint64_t b_after, uint64_t S, uint32_t M, uint32_t *row)
{
    *row = segments_index(b_before, S, M);
    return segments_index(b_after, S, M) > *row;
}

// The definition as the sequential loop it is, one record at a time (the stand-alone check runs this; the kernels reach the
// same words with prefix sums).  vec: segments_len(P, M) words.
inline void segments_init(uint64_t *vec, uint32_t P, uint64_t S, uint32_t M, uint32_t overhead)
{
    for (size_t i = 0; i < segments_len(P, M); i++) vec[i] = 0;
    uint64_t *g = vec + segments_globals_at(P, M);
    g[kSegGlobalS] = S, g[kSegGlobalM] = M, g[kSegGlobalOverhead] = overhead;
}
inline void segments_apply_record(uint64_t *vec, uint32_t P, uint32_t M, int32_t partition, int32_t key_len, int32_t val_len, int64_t ts_ms)
{
    uint64_t *g = vec + segments_globals_at(P, M);
    const uint64_t S = g[kSegGlobalS];
    const uint32_t overhead = (uint32_t)g[kSegGlobalOverhead];
    if ((uint32_t)partition >= P) {    // (a negative partition is a large unsigned one)
        g[kSegGlobalBadPartition]++;
        return;
    }
    g[kSegGlobalRecords]++;
    uint64_t *t = vec + segments_total_at(P, M, (uint32_t)partition);
    const uint64_t before = t[kSegB], h = segments_ts_word(ts_ms);
    t[kSegC] += 1, t[kSegB] += segments_record_size(overhead, key_len, val_len), t[kSegT] += val_len < 0 ? 1u : 0u;
    if (h > t[kSegH1]) t[kSegH1] = h;
    uint32_t row;
    if (segments_closes(before, t[kSegB], S, M, &row)) {
        uint64_t *r = vec + segments_row_at((uint32_t)partition, M, row);
        for (uint32_t k = 0; k < kSegWords; k++) r[k] = t[k];
        g[kSegGlobalClosed]++;
    }
}

// ---- identities with the counter vector of the same records (include/kta_hip.h: u64[P*7 + KTA_NGLOBALS]) ------------
// counters: [P][7] = total, tombstones, alive, key_null, key_non_null, key_size_sum, value_size_sum | the globals, of
// which g_records and g_bad are the words KTA_G_RECORDS and KTA_G_BAD_PARTITION.
inline bool segments_identities_hold(const uint64_t *vec, uint32_t P, uint32_t M, const uint64_t *counters, uint64_t g_records, uint64_t g_bad)
{
    const uint64_t *g = vec + segments_globals_at(P, M);
    const uint64_t overhead = g[kSegGlobalOverhead];
    bool ok = g[kSegGlobalRecords] == g_records && g[kSegGlobalBadPartition] == g_bad;   // (KTA_G_RECORDS: the records inside [0, P))
    for (uint32_t p = 0; p < P; p++) {
        const uint64_t *t = vec + segments_total_at(P, M, p), *c = counters + (size_t)p * 7;
        ok = ok && t[kSegC] == c[0] && t[kSegT] == c[1] && t[kSegB] - overhead * t[kSegC] == c[5] + c[6];
    }
    return ok;
}

// ---- merge --------------------------------------------------------------------------------------------------------
// acc += other: every word a sum but the three configuration globals, which must agree (false: they do not, acc is as it
// was).  Exact when every partition's records went through ONE context in order (the others hold zeros).
inline bool segments_merge(uint64_t *acc, const uint64_t *other, uint32_t P, uint32_t M)
{
    const size_t ga = segments_globals_at(P, M);
    for (uint32_t k = kSegGlobalS; k <= kSegGlobalOverhead; k++)
        if (acc[ga + k] != other[ga + k]) return false;
    for (size_t i = 0; i < ga + kSegGlobalS; i++) acc[i] += other[i];
    return true;
}

// ---- the what-if --------------------------------------------------------------------------------------------------
// out[(P + 1)][kRetWords]: a row per partition and one for the topic (the sums; its rule word is the OR of the
// partitions' and its clamped word their count).
enum : uint32_t {
    kRetSegments = 0,        // closed non-empty rows + 1 if the open tail holds a record
    kRetRecords, kRetBytes, kRetTombstones,                  // now
    kRetRecordsKept, kRetBytesKept, kRetTombstonesKept,      // under the policy
    kRetSegmentsDeleted,
    kRetRule,                // 0: nothing deleted; 1: the time rule reached at least as far as the size rule; 2: the size rule further
    kRetClamped,             // the partition outgrew its M rows: the last row holds the rest and counts as active
    kRetWords
};
// row k of a partition is deleted by the time rule / the size rule (retention -1: the rule is off)
KTA_SEGMENTS_HD bool retention_time_takes(const uint64_t *row, int64_t now_ms, int64_t retention_ms)
{
    if (retention_ms < 0 || row[kSegH1] == 0) return false;
    const uint64_t h = row[kSegH1] - 1u;                 // 0 .. 2^63 - 1
    if (now_ms < 0 || (uint64_t)now_ms < h) return false;
    return (uint64_t)now_ms - h > (uint64_t)retention_ms;
}
KTA_SEGMENTS_HD bool retention_size_takes(const uint64_t *row, const uint64_t *total, int64_t retention_bytes)
{
    return retention_bytes >= 0 && total[kSegB] - row[kSegB] >= (uint64_t)retention_bytes;
}
inline void retention_whatif(const uint64_t *vec, uint32_t P, uint32_t M, int64_t now_ms, int64_t retention_ms, int64_t retention_bytes,
                             uint64_t *out)
{
    const uint64_t S = vec[segments_globals_at(P, M) + kSegGlobalS];
    uint64_t *all = out + (size_t)P * kRetWords;
    for (uint32_t k = 0; k < kRetWords; k++) all[k] = 0;
    for (uint32_t p = 0; p < P; p++) {
        const uint64_t *t = vec + segments_total_at(P, M, p);
        uint64_t *o = out + (size_t)p * kRetWords;
        const uint64_t *last = nullptr, *cut = nullptr;  // the last closed row; the last deleted one
        uint64_t closed = 0, deleted = 0, by_time = 0, by_size = 0;
        bool walking = true, timing = true, sizing = true;
        for (uint32_t s = 0; s + 1 < M; s++) {
            const uint64_t *r = vec + segments_row_at(p, M, s);
            if (r[kSegC] == 0) continue;                 // never closed: skipped by a large record, or not reached
            closed++, last = r;
            timing = timing && retention_time_takes(r, now_ms, retention_ms);
            sizing = sizing && retention_size_takes(r, t, retention_bytes);
            by_time += timing, by_size += sizing;
            walking = walking && (timing || sizing);     // (each rule's rows are a prefix: H and B only grow)
            if (walking) deleted++, cut = r;
        }
        o[kRetSegments] = closed + (t[kSegC] > (last ? last[kSegC] : 0u) ? 1u : 0u);
        o[kRetRecords] = t[kSegC], o[kRetBytes] = t[kSegB], o[kRetTombstones] = t[kSegT];
        o[kRetRecordsKept] = t[kSegC] - (cut ? cut[kSegC] : 0u);
        o[kRetBytesKept] = t[kSegB] - (cut ? cut[kSegB] : 0u);
        o[kRetTombstonesKept] = t[kSegT] - (cut ? cut[kSegT] : 0u);
        o[kRetSegmentsDeleted] = deleted;
        o[kRetRule] = deleted == 0 ? 0u : by_time >= by_size ? 1u : 2u;
        o[kRetClamped] = t[kSegB] / S >= (uint64_t)(M - 1u) ? 1u : 0u;
        for (uint32_t k = 0; k < kRetWords; k++) {
            if (k == kRetRule) all[k] |= o[k];
            else all[k] += o[k];
        }
    }
}

} // namespace kta

// kta_kernels.h — internal launch interface between the C-ABI layer (kta_api.hip) and the
// gfx950 kernels: the metrics scan and its fold (kta_kernels.hip) and the single-kernel alive-table family
// (kta_alive_table.hip).  Not part of the public ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kta_hip.h"
#include "kta_tile.h"
#include "kta_filter.h"

namespace kta {

constexpr int kWG = 256;                    // threads per workgroup (4 wave64)
constexpr uint32_t kScanCols = 5;           // per-partition partial columns written by the scan:
                                            //   count, tombstones, key_null, key_size_sum, value_size_sum
constexpr uint32_t kScanGlobals = 8;        // per-workgroup partial globals (see ScanGlobal)
constexpr uint64_t kAliveSlots = 1ull << 32; // the reference hashes into a usize from a u32 (metric.rs:259)

enum ScanGlobal : uint32_t {
    SG_TMIN = 0, SG_TMAX = 1, SG_SMIN = 2, SG_SMAX = 3, SG_BAD = 4, SG_NREC = 5
};

// hdr == null: the raw layout, the pointers address record 0 of the batch.  Otherwise the tile-compact layout
// (kta_hip.h): the pointers — all four — address record 0 of the ALLOCATION (tile 0) and the batch is its records
// [rec0, rec0 + n); a tile's header says how its bytes of the four columns are used.
struct ScanColumns {
    const int32_t *partition;
    const int32_t *key_len;
    const int32_t *val_len;
    const int64_t *ts_ms;
    const kta_tile_hdr *hdr;
    uint64_t rec0;
    const kta_tile_sum *sum;   // the tiles' summaries beside hdr (kta_tile.h), or null: none.  Read by kta_metrics_scan_packed only.
    const uint32_t *mark;      // the tiles' plane marks beside sum (kta_tile.h), or null: none, or ignored (scan_variant bit 64)
    const uint32_t *size;      // the tiles' size extrema, two words per tile (kta_tile.h); null wherever mark is
};

struct AliveColumns {
    const int32_t *key_len;
    const int32_t *val_len;
    const uint32_t *key_off;
    const uint8_t *key_bytes;
    const uint64_t *seq; // may be null
};

// Table state: the slots this context ever wrote, in the order they were first written — what a rank exports in the
// exchange instead of sweeping its 32 GiB table.  Every kernel that writes the table appends a slot when it finds the
// entry 0 (never written).  n counts past cap when the list overflows (the exchange then sweeps the table).
struct WrittenList {
    uint32_t *slots;            // null: not tracked
    unsigned long long *n;      // device counter
    uint64_t cap;
};

#ifdef __HIPCC__
// wave-aggregated append (works under divergence: the ballot covers the active lanes)
__device__ __forceinline__ void note_new_slot(const WrittenList &wl, bool is_new, uint32_t slot)
{
    if (!wl.slots) return;
    const unsigned long long m = __ballot(is_new);
    if (m == 0ull) return;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    unsigned long long base = 0;
    if (is_new && rank == 0u) base = atomicAdd(wl.n, (unsigned long long)__popcll(m));
    base = __shfl(base, __ffsll((long long)m) - 1);
    if (is_new && base + rank < wl.cap) wl.slots[base + rank] = slot;
}
#endif

struct ScanPlan {
    uint32_t workgroups;   // grid size
    uint32_t rep_log2;     // LDS replication of each partition's slots
    uint32_t lds_bytes;    // dynamic LDS per workgroup
    uint32_t variant;      // 0 = accumulate (three 64-bit LDS atomics per record or quad), 9 = loads only (diagnostic)
    bool summaries;        // packed: take a summarised tile's timestamp extrema from its summary (req_variant bit 32 clears it)
    bool planes;           // packed: take a marked tile through its plane (req_variant bit 64 clears it)
    bool packed;           // tile-compact, accumulating, no additive outputs: kta_metrics_scan_packed (two atomics, two
                           // levels of partials in LDS: lds_bytes = 16 P R + 40 P)
    bool nontemporal;      // stream the columns with non-temporal loads
    bool analytics;        // additive outputs: size histograms + per-partition extrema
    uint32_t row_len;      // u64 words per workgroup row of the partial workspace
    uint32_t timeline_rows; // TIMELINE: n_buckets + 3 rows of {packed count, bytes} in LDS after the other arrays; 0 = none
};

// Timeline (kta_set_timeline): vector u64[(n_buckets + 3) * 3], rows [no timestamp, before, bucket 0..n-1, after] of
// [records, tombstones, bytes].  The scan places a counted record with the host-side reciprocal of the width and an
// exact +-1 correction (no 64-bit division per record).
constexpr uint32_t kTimelineCols = KTA_TIMELINE_COLS;
inline uint32_t timeline_len(uint32_t n_buckets) { return (n_buckets + 3u) * kTimelineCols; }
struct TimelineArgs {
    long long origin;           // origin_ms >= 0
    unsigned long long width;   // bucket_ms >= 1
    unsigned long long span;    // n_buckets * bucket_ms (no int64 overflow with origin)
    float inv_width;            // 1 / bucket_ms, rounded: an estimate the kernel corrects
    uint32_t n_buckets;         // 1 .. KTA_TIMELINE_MAX_BUCKETS
    uint64_t *vec;              // the live accumulator (device-scope atomicAdd of the non-zero rows at every flush)
};

constexpr uint32_t kAnalyticsHist = 2 * 34; // key-size and value-size log2 histograms
// analytics vector: u64[2*34 + 4*P] = histograms, then per partition [~min ts, max ts, ~smallest, largest]
inline uint32_t analytics_len(uint32_t P) { return kAnalyticsHist + 4 * P; }

// u64 words one workgroup writes into the partial workspace
inline uint32_t scan_row_len(uint32_t P, bool analytics)
{
    return P * kScanCols + kScanGlobals + (analytics ? 4 * P + 2 * 34 : 0);
}

// tiled: the batch is tile-compact (ScanColumns.hdr): more workgroups per CU (see plan_scan)
// timeline_buckets: 0 = no timeline (the plan of before); else the timeline's rows come out of the same LDS budget
ScanPlan plan_scan(uint32_t P, uint64_t n, int cu_count, int req_workgroups, int req_variant, bool analytics,
                   bool tiled = false, uint32_t timeline_buckets = 0);

// K1: per-record metric accumulation (metric.rs:207-252) over one struct-of-arrays batch.
// tl: the timeline (plan.timeline_rows != 0), else null.
hipError_t launch_metrics_scan(const ScanPlan &plan, const ScanColumns &c, uint64_t n, uint32_t P,
                               uint64_t *partials, hipStream_t s, const TimelineArgs *tl = nullptr);
// K5: fold the per-workgroup partial rows into the persistent counter vector.
hipError_t launch_fold_partials(const uint64_t *partials, uint32_t rows, uint32_t P, uint64_t *vec,
                                uint32_t row_len, uint64_t *analytics_vec, hipStream_t s);
// Tile-compact batches (kta_hip.h): make every tile that overlaps the allocation's records [lo, hi) raw (what bit 0:
// partition and ts_ms; bit 1: the lengths, u16 -> i32), expanded in place, so records outside the range keep their values:
// before a producer that writes the raw layout stores into the range (what 3), or, with keep — the tiles inside the range
// are expanded as well —, before a pass that reads plain i32 lengths next to keys runs over it (what 2).
hipError_t launch_tiles_to_raw(int32_t *partition, int64_t *ts_ms, int32_t *key_len, int32_t *val_len, kta_tile_hdr *hdr,
                               uint64_t lo, uint64_t hi, uint32_t what, bool keep, hipStream_t s);
// reset the counter vector to the MessageMetrics::new state (metric.rs:30-46)
hipError_t launch_init_vector(uint64_t *vec, uint32_t P, uint64_t *analytics_vec, hipStream_t s);

// K2+K3: FNV (fnv32.rs:92-101) + last-writer-wins table update (metric.rs:289-304)
// variant 0 = fused; 1 = fused + running alive count (returning atomics, default); 8 / 9 = ablation halves
// (hash -> scratch, scratch -> table)
hipError_t launch_alive_update(const AliveColumns &c, uint64_t n, uint64_t base_seq, uint64_t *table,
                               int workgroups, int variant, uint32_t *scratch, int64_t *running, hipStream_t s,
                               const uint32_t *only_if /* variant 2: device word, run only when non-zero; may be null */,
                               const WrittenList &written);
// K2'+K3' (kta_alive.hip): the same update as two kernels — hash + partition the batch's (hash, index, alive)
// pairs by the hash's top bits into workgroup-private segments, then one workgroup per bucket merges its
// pairs in LDS and applies the survivors to the region of the persistent state it alone writes.  The state is
// either the reference's bit set (batches applied in submission order) or the u64 last-writer table (global
// sequence numbers).  A seq column must ascend inside a batch (checked on the device: alive_order_flag).
constexpr uint64_t kAlivePartitionMin = 1ull << 21;   // table state: below this the single-kernel update is used
constexpr uint64_t kAlivePartitionMax = 1ull << 28;   // records per launch pair: larger batches are sliced
struct AlivePartitionPlan {
    bool pair32;            // bit set state: 4-byte pairs with implicit order (kta_alive.hip); table state: 8-byte pairs
    uint32_t bucket_log2;   // buckets = state regions = apply workgroups
    uint32_t segment_wgs;   // partition workgroups = segments per bucket
    uint32_t tiles_per_wg;  // 256-record tiles each partition workgroup takes (a contiguous range)
    uint32_t cap;           // pairs per segment
    uint64_t max_records;   // records one launch pair takes (larger batches are sliced)
    uint64_t pair_words;    // u64 words of the pair workspace
    uint64_t count_words;   // u32 words of the segment-count workspace
    uint64_t pool_pairs;    // pairs the pool takes (whose segment was full); bit set state: in blocks of 16, their tags behind them
    uint64_t pool_words;    // u64 words of the pool's allocation
    uint64_t ctl_bytes;     // pool control words + pool histogram + order flag
};
struct AliveState {
    uint64_t *table;        // u64[2^32], or null
    uint32_t *bitmap;       // u32[2^27] = 2^32 bits, or null (exactly one of the two)
    int64_t *running;       // running alive count
    WrittenList written;    // table state: the slots ever written
};
struct AliveWorkspace {
    uint64_t *pairs;
    uint32_t *counts;
    uint64_t *pool;
    void *pool_ctl;         // ctl_bytes
    uint32_t *fail_from;    // u32[3 x buckets] (bit set state): per bucket the first segment pass 2 left to kta_alive_fallback
                            // (or none), then the list of the buckets it gave up, then the list of the buckets whose slots
                            // did not fit pass 2's table in one piece (applied in slot-range passes)
    uint64_t *failed_total; // bit set state: += the buckets a launch pair handed to kta_alive_fallback (device word; may be null)
};
AlivePartitionPlan plan_alive_partition(uint64_t n, int req_wgs, int cu_count, bool pair32);
// Both handlers in one pass (bit set state): pass 1 also reads partition and ts_ms and writes one row of the scan's partial
// workspace per partition workgroup (plan.segment_wgs rows of row_len words), to be folded by launch_fold_partials —
// MessageMetrics::handle_message (metric.rs:207-252) without a second reading of key_len and val_len.
struct AliveFuse {
    const int32_t *partition;   // as ScanColumns: with hdr, the allocation's record 0 and the batch's first record rec0
    const int64_t *ts_ms;
    const kta_tile_hdr *hdr;
    uint64_t rec0;
    uint32_t P;
    uint64_t *partials;
    uint32_t row_len;
};
bool alive_fuse_possible(const AlivePartitionPlan &plan, uint32_t P);   // P <= 256, and less than 2^21 records per workgroup
hipError_t launch_alive_partitioned(const AliveColumns &c, uint64_t n, uint64_t base_seq, const AliveState &st,
                                    const AlivePartitionPlan &plan, const AliveWorkspace &ws,
                                    uint64_t *stats /* [pairs, claims] += ; may be null */, hipStream_t s,
                                    const AliveFuse *fuse = nullptr /* null: the alive-key pass only */);
// device word that the launch pair sets when the batch's seq column does not ascend (the pair then did nothing)
const uint32_t *alive_order_flag(const AliveWorkspace &ws, int bucket_log2);
// popcount of the bit set -> *out += (u64)
hipError_t launch_bitmap_count(const uint32_t *bitmap, uint64_t *out, hipStream_t s);
// K4: sum_all_alive (metric.rs:282-284): count table entries whose low bit is set -> *out (u64)
hipError_t launch_alive_count(const uint64_t *table, uint64_t n_slots, uint64_t *out, hipStream_t s);
// compact (slot, value) export / import of the entries ever written: what sharded GPUs exchange
hipError_t launch_alive_count_span(const uint64_t *table, uint64_t lo, uint64_t hi, uint64_t *out, hipStream_t s);
hipError_t launch_alive_count_written(const uint64_t *table, uint64_t n_slots, uint64_t *out, hipStream_t s);
hipError_t launch_alive_export(const uint64_t *table, uint64_t n_slots, uint32_t *out_slots, uint64_t *out_vals,
                               uint64_t *counter, uint64_t cap, hipStream_t s);
hipError_t launch_alive_export_span(const uint64_t *table, uint64_t lo, uint64_t hi, uint32_t *out_slots,
                                    uint64_t *out_vals, uint64_t *counter, uint64_t cap, hipStream_t s);
hipError_t launch_alive_count_written_span(const uint64_t *table, uint64_t lo, uint64_t hi, uint64_t *out, hipStream_t s);
hipError_t launch_alive_import(const uint32_t *slots, const uint64_t *vals, uint64_t n, uint64_t *table,
                               int64_t *running, const WrittenList &written, hipStream_t s);
// the exchange over the written list: entries per owner rank (owner(slot) = (slot * R) >> 32), their export as
// one contiguous (slot, value) list per owner, and the alive count of one owner's range
// (the list's length is read on the device; *overflow = 1 when it exceeds the list's capacity)
hipError_t launch_written_count(const WrittenList &wl, int nranks, uint64_t *counts /* [nranks] += */, uint64_t *overflow, hipStream_t s);
hipError_t launch_written_export(const WrittenList &wl, const uint64_t *table, int nranks, int skip_rank,
                                 const uint64_t *owner_at /* device [nranks] */, uint64_t *cursors /* device [nranks], zero */,
                                 uint32_t *out_slots, uint64_t *out_vals, hipStream_t s);
hipError_t launch_written_alive_count(const WrittenList &wl, const uint64_t *table, uint64_t lo, uint64_t hi,
                                      uint64_t *out /* = */, hipStream_t s);
// table -> 2^32-bit bitmap (u32 words)
hipError_t launch_alive_bitmap(const uint64_t *table, uint64_t n_slots, uint32_t *bitmap, hipStream_t s);
// hash only (tests)
hipError_t launch_fnv32(const uint8_t *key_bytes, const uint32_t *key_off, const int32_t *key_len,
                        uint64_t n, uint32_t *out, hipStream_t s);

// Key sketch (KTA_FLAG_KEY_SKETCH, kta_sketch.hip): u32 registers [P][4096], the live accumulator, raised with atomicMax by
// the records that get past two filters — a per-(partition, register group) floor in LDS (the least register of the
// group, refreshed by launch_key_sketch_floor before every launch) and a read of the register itself.  Registers only
// grow, so a filter that reads a stale (smaller) value costs an atomic, never an update.
constexpr uint32_t kSketchRegs = 1u << KTA_SKETCH_LOG2;
constexpr uint32_t kSketchFloorBytes = 16384;   // LDS of the floors: P * groups <= this, groups = 4096 >> group_shift
inline uint32_t sketch_group_shift(uint32_t P)  // log2 of registers per floor group
{
    uint32_t s = 0;
    while (((uint64_t)P * (kSketchRegs >> s)) > kSketchFloorBytes) s++;
    return s;
}
struct SketchColumns {
    const int32_t *partition;   // as ScanColumns: with hdr, the allocation's record 0 and the batch's first record rec0
    const kta_tile_hdr *hdr;
    uint64_t rec0;
    const int32_t *key_len;     // the batch's record 0 (both layouts)
    const uint32_t *key_off;
    const uint8_t *key_bytes;   // readable 16 bytes past the last key
};
// stats: u64[3] += keyed records, records that read their register, records that reached an atomic (device words)
hipError_t launch_key_sketch(const SketchColumns &c, uint64_t n, uint32_t P, uint32_t *regs, const uint8_t *floors,
                             uint64_t *stats, int cu_count, hipStream_t s);
// floors[p << (12 - group_shift) | g] = min of partition p's registers of group g (u8)
hipError_t launch_key_sketch_floor(const uint32_t *regs, uint32_t P, uint8_t *floors, hipStream_t s);
// out[i] = regs[i] (u32 -> u64): the snapshot kta_finish_device takes
hipError_t launch_key_sketch_widen(const uint32_t *regs, uint64_t n, uint64_t *out, hipStream_t s);

// Hot keys (KTA_FLAG_HOT_KEYS, kta_hot.hip): the live accumulator u64[2][1024][23] that the workgroups of launch_hot_keys
// add their LDS counters to, the exemplar table and the three per-slot words of its claiming (kta_hot_candidates writes
// them before every launch: the cell's candidate x, a mark bit when the slot does not hold it, a zeroed claim).
constexpr uint32_t kHotFlushRoundsMax = 511;    // rounds of 4096 records between two flushes: below 2^21 records
constexpr uint32_t kHotLdsBytes = KTA_HOT_ROWS * KTA_HOT_CELLS * (8 * 8 + 4) + KTA_HOT_ROWS * KTA_HOT_CELLS / 8;
struct HotState {
    uint64_t *acc;              // u64[KTA_HOT_VECTOR_WORDS]
    kta_hot_exemplar *slots;    // [2][1024]
    uint32_t *want;             // u32[2048]
    uint32_t *mark;             // u32[64]: a bit per slot
    uint32_t *claim;            // u32[2048]
    uint64_t *stats;            // u64[4] += keyed records, add groups, mid-stream flushes, exemplars captured
};
// the candidates, then the pass over records [0, n) of c; *workgroups = the pass's grid.  flush_rounds 0: the most.
hipError_t launch_hot_keys(const SketchColumns &c, uint64_t n, uint32_t P, const HotState &st, uint32_t flush_rounds, int cu_count,
                           uint32_t *workgroups, hipStream_t s);

// Timestamp order (KTA_FLAG_TS_ORDER, kta_ts_order.hip): the live vector u64[3 P + 64] = [P][2] late records and their
// lateness | hist[63] | timed | the largest lateness [P], the running maximum hi i64[P] (-1: none) that carries over from
// batch to batch, and the workspace i64[chunks][P] of one launch triple.
constexpr uint32_t kTsOrderMaxPartitions = 4096;            // the apply kernel's LDS plan: one wave per workgroup up there
constexpr size_t kTsOrderWorkspaceWords = (size_t)1 << 22;  // 32 MiB: chunks per launch triple = this / P
constexpr uint64_t kTsOrderChunkMin = 1024;                 // default chunk: the slice over kTsOrderChunks, at least this
constexpr uint64_t kTsOrderChunks = 8192;
inline size_t ts_order_len(uint32_t P) { return 3 * (size_t)P + 64; }
struct TsOrderState {
    uint64_t *vec;              // u64[3 P + 64]
    int64_t *hi;                // i64[P]
    int64_t *ws;                // i64[kTsOrderWorkspaceWords]
    uint64_t *stats;            // u64[3] += instructions with a timestamped record, of them one partition, colliding groups
};
// Records [0, n) of c in chunks of `chunk` records (a multiple of 64; ceil(n / chunk) * P <= kTsOrderWorkspaceWords):
// chunk maxima, prefix, apply.
hipError_t launch_ts_order(const ScanColumns &c, uint64_t n, uint64_t chunk, uint32_t P, const TsOrderState &st, hipStream_t s);

// Segments (kta_set_segments, kta_segments.hip; the rule and the vector's layout are kta_segments.h's): the live vector
// u64[(P M + P) 4 + 8], whose totals [P][4] are the running state that carries over from batch to batch, the workspace
// u64[chunks][P][4] of one launch triple and a flag word per chunk.
constexpr uint32_t kSegmentsMaxPartitions = 2048;           // the apply kernel's LDS plan: 41 B per partition and wave, one wave up there
constexpr size_t kSegmentsWorkspaceWords = (size_t)1 << 23; // 64 MiB: chunks per launch triple = this / (4 P)
constexpr uint64_t kSegmentsChunkMin = 1024;                // default chunk: the slice over kSegmentsChunks, at least this
constexpr uint64_t kSegmentsChunks = 8192;
struct SegmentsState {
    uint64_t *vec;              // u64[segments_len(P, M)]
    uint64_t *ws;               // u64[kSegmentsWorkspaceWords]
    uint32_t *flags;            // u32[kSegmentsWorkspaceWords / 4]
    uint64_t *stats;            // u64[4] += chunks applied, chunks skipped, instructions of one partition, colliding groups
    uint64_t S;
    uint32_t M, overhead;
};
// Records [0, n) of c in chunks of `chunk` records (a multiple of 64, at most 2^31; ceil(n / chunk) * 4 P <=
// kSegmentsWorkspaceWords): chunk sums, prefix, apply.
hipError_t launch_segments(const ScanColumns &c, uint64_t n, uint64_t chunk, uint32_t P, const SegmentsState &st, hipStream_t s);
// The kept rows of the compact,delete what-if (kta_set_compact_delete; the rule and the vector's layout are
// kta_compact_delete.h's): the same triple over st.vec = the kept vector, with cls u8[n] the records' class bytes, which
// launch_compaction wrote.  The timestamp column is not read.  st.stats: u64[4] as above.
hipError_t launch_kept_rows(const ScanColumns &c, const uint8_t *cls, uint64_t n, uint64_t chunk, uint32_t P, const SegmentsState &st, hipStream_t s);

// Partitioner (KTA_FLAG_PARTITIONER, kta_partitioner.hip): the live vector u64[2 P + 2 Q] = [P][2] checked, placed |
// [Q][2] target_records, target_bytes, every word a sum that the workgroups of launch_partitioner add their LDS counters to.
constexpr uint32_t kPartitionerMaxPartitions = 4096;        // P and Q each: 8 P + 12 Q bytes of LDS, 80 KiB up there
constexpr uint64_t kPartitionerLaunchMax = 1ull << 30;      // records per launch: the u32 fields in LDS cannot overflow
inline size_t partitioner_len(uint32_t P, uint32_t Q) { return 2 * (size_t)P + 2 * (size_t)Q; }
struct PartitionerColumns {
    SketchColumns k;            // what the key sketch reads
    const int32_t *val_len;     // the batch's record 0, plain i32 (both layouts), as k.key_len
};
// the pass over records [0, n) of c, n <= kPartitionerLaunchMax; stats: u64[3] += keyed records, LDS adds to the partition
// words, LDS adds to the target words (after combining); *workgroups = the grid
hipError_t launch_partitioner(const PartitionerColumns &c, uint64_t n, uint32_t P, uint32_t Q, uint64_t *acc, uint64_t *stats,
                              int cu_count, uint32_t *workgroups, hipStream_t s);
// out = {dynamic LDS bytes, threads, workgroups per CU} of the launch for P and Q (kta_partitioner_info)
void partitioner_lds_plan(uint32_t P, uint32_t Q, uint32_t out[3]);

// Compaction what-if (KTA_FLAG_COMPACTION, kta_compaction.hip; the rule and the vector's layout are kta_compaction.h's): the
// live vector u64[5 P + 6], every word a sum that the workgroups of launch_compaction add their LDS words to.
constexpr uint32_t kCompactionMaxPartitions = 4096;         // 32 P bytes of LDS, 128 KiB up there
struct CompactionColumns {
    SketchColumns k;            // what the key sketch reads
    const int32_t *val_len;     // the batch's record 0, plain i32 (both layouts), as k.key_len
    const uint64_t *seq;        // null: record i has the sequence number base_seq + i
};
// the replay of records [0, n) of c against the last-writer table, n <= kCompactionLaunchMax; stats: u64[3] += keyed
// records looked at, LDS adds, reserved; *workgroups = the grid.  cls (null: none): u8[n], gets every record's class byte
// (kta_compact_delete.h) — another instantiation of the kernel.
hipError_t launch_compaction(const CompactionColumns &c, uint64_t n, uint64_t base_seq, uint32_t P, const uint64_t *table, uint64_t *acc,
                             uint64_t *stats, int cu_count, uint32_t *workgroups, hipStream_t s, uint8_t *cls = nullptr);
// out = {dynamic LDS bytes, threads, workgroups per CU} of the launch for P (kta_compaction_info)
void compaction_lds_plan(uint32_t P, uint32_t out[3]);

// Size percentiles (KTA_FLAG_SIZE_QUANTILES, kta_size_quantiles.hip; the bin rule and the vector's layout are
// kta_size_bins.h's): the live vector u64[P * 3 * 464 + 8], every word a sum that the workgroups of launch_size_quantiles add
// their LDS counters to.
constexpr uint32_t kSizeQuantilesMaxSlice = 28;             // partitions of a slice at most: 28 * 5568 B = 152.25 KiB of LDS
constexpr uint32_t kSizeQuantilesMaxPartitions = 1024;      // 37 slices, each of which streams the batch; an 11 MiB vector
constexpr uint64_t kSizeQuantilesLaunchMax = 1ull << 30;    // records per launch: the u32 counters in LDS cannot overflow
// the pass over records [0, n) of c (partition, key_len, val_len in the tiles' own forms; ts_ms is not read),
// n <= kSizeQuantilesLaunchMax.  forced_slice: the tests' S (0: the plan's).  variant 0: the slices are the grid's second
// dimension; 1: one launch per slice; 9: the loads alone (both diagnostics).  stats: u64[8], word 0 += LDS adds issued
// (after combining); *workgroups = the workgroups launched
hipError_t launch_size_quantiles(const ScanColumns &c, uint64_t n, uint32_t P, uint32_t forced_slice, int variant, uint64_t *acc, uint64_t *stats,
                                 int cu_count, uint32_t *workgroups, hipStream_t s);
// out = {S, slices, dynamic LDS bytes, threads, workgroups per CU} of the launch for P (kta_size_quantiles_info)
void size_quantiles_plan(uint32_t P, uint32_t forced_slice, uint32_t out[5]);

// Record filter (kta_set_filter, kta_filter.hip; the rules are kta_filter.h's): one slice of a device batch, compacted in
// record order into a raw-layout scratch batch by three launches (count per tile, prefix of the counts, scatter).
constexpr uint64_t kFilterSlice = 1ull << 26;                                   // records per slice, at most
constexpr uint64_t kFilterMaxTiles = kFilterSlice / KTA_TILE_RECORDS + 1;       // (+ 1: a view that starts inside a tile)
constexpr uint64_t kFilterCountWords = 256 * 260;                                // the prefix kernel's 256 stretches of whole 16-byte words
constexpr uint32_t kFilterBitmapBytes = 65536;                                  // the partition set in LDS: P <= 2^19
struct FilterSource {
    const int32_t *partition;   // as ScanColumns: with hdr, the allocation's record 0, and the slice's first record is a0;
    const int32_t *key_len;     // without, the slice's own record 0 and a0 == 0
    const int32_t *val_len;
    const int64_t *ts_ms;
    const kta_tile_hdr *hdr;
    const kta_tile_sum *sum;    // null: no summaries, every tile is read
    uint64_t a0;
    const uint32_t *key_off;    // the slice's record 0 (plain in both layouts); null: no key columns
    const uint64_t *seq;        // likewise; null: base_seq + i
    uint64_t base_seq;          // of the slice's record 0
};
struct FilterDest {             // the scratch batch, raw layout
    int32_t *partition, *key_len, *val_len;
    int64_t *ts_ms;
    uint32_t *key_off;          // null: not kept
    uint64_t *seq;              // null: not kept
    uint64_t capacity;          // records: no store goes at or past it
};
struct FilterWorkspace {
    uint32_t *count;            // u32[kFilterCountWords]: a tile's count, and how it was decided in the high half
    uint64_t *offset;           // u64[kFilterMaxTiles + 1]: the exclusive prefix, then the slice's total
    uint64_t *stats;            // u64[3] += tiles decided "none" by summary, decided "all" by summary, read
    uint64_t *total_host;       // one word of pinned host memory, as the device addresses it: the slice's total, written by
                                // the prefix kernel itself (no copy command between the kernel and the host's wait)
};
// records [0, n) of c, n <= kFilterSlice.  launch_filter_count: the counts and their prefix; the total is
// *ws.total_host (and ws.offset[filter_slice_tiles(c.a0, n)]) once the stream got there.  launch_filter_scatter: the passing records to `out`,
// behind it on the same stream (a slice whose total is 0 or n does not need it).
hipError_t launch_filter_count(const FilterSource &c, uint64_t n, const FilterSpec &f, const uint32_t *bitmap, const FilterWorkspace &ws, hipStream_t s);
hipError_t launch_filter_scatter(const FilterSource &c, uint64_t n, const FilterSpec &f, const uint32_t *bitmap, const FilterWorkspace &ws,
                                 const FilterDest &out, hipStream_t s);

} // namespace kta

// kta_api.hip — the extern "C" boundary of libkta_hip.so (include/kta_hip.h): context,
// pinned struct-of-arrays staging ring, H2D/compute streams, result decode.
// Host code only; the kernels are in the other .hip files (the scan: kta_kernels.hip; the alive table's single-kernel
// family: kta_alive_table.hip), behind the launchers of kta_kernels.h.  There is no CPU fallback: every
// entry point that computes anything needs a gfx950 device.
#include "../../include/kta_hip.h"
#include "kta_compact_delete.h"
#include "kta_compaction.h"
#include "kta_header_names.h"
#include "kta_internal.h"
#include "kta_kernels.h"
#include "kta_murmur2.h"
#include "kta_payload.h"
#include "kta_record_batches.h"
#include "kta_segments.h"
#include "kta_size_bins.h"
#include "kta_value_bytes.h"
#include "kta_lz4_model.h"

#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <cstdlib>
#include <string>
#include <time.h>
#include <vector>

namespace {

thread_local std::string g_create_error = "";

// One staging batch = ONE pinned slab and ONE device slab with the same layout: the columns at 16-byte
// aligned offsets in the order [partition | key_len | val_len | ts_ms | key_off | seq | key_bytes], sized for
// the batch capacity, the variable part (key bytes) last.  A submit is then a single H2D copy of the slab's
// used prefix (a copy per column — up to seven DMA launches per batch — was 19 % of the GPU time of a
// host-fed run, profiles/r01).
struct Stage {
    kta_batch host{};  // column pointers into host_slab (pinned)
    kta_batch dev{};   // column pointers into dev_slab
    PinnedBuf<uint8_t> host_slab;
    DeviceBuf<uint8_t> dev_slab;
    size_t metric_bytes = 0;      // [partition .. ts_ms]
    size_t key_bytes_off = 0;     // where key_bytes starts (0 without -c, the key sketch or the hot keys)
    size_t slab_bytes = 0;
    Event done;
    bool busy = false;
};

constexpr size_t kMaxTimedPairs = 2048;

} // namespace

struct kta_ctx {
    // kta_destroy releases what the context owns by deleting it: members go in the reverse of this order, so the streams
    // come first here (destroyed last, after every buffer and event), and nothing below may outlive them.
    Stream s_own;                   // the context's own compute stream (s_compute may be caller-owned)
    Stream s_copy;
    int device = 0;
    uint32_t P = 0;
    bool alive = false;
    int cu_count = 256;
    hipStream_t s_compute = nullptr;
    Event ev_copied;
    bool analytics = false;
    bool stage_seq = false;         // KTA_FLAG_SEQ_COLUMN
    DeviceBuf<uint64_t> d_avec;     // analytics vector u64[2*34 + 4*P] (KTA_FLAG_ANALYTICS)
    DeviceBuf<uint64_t> d_avec_out; // its snapshot (kta_finish_device), reduced by the exchange like d_vec_out
    // timeline (kta_set_timeline): d_tvec u64[(n_buckets + 3) * 3] the live accumulator, d_tvec_out its snapshot
    bool timeline = false;
    kta::TimelineArgs tl{};
    DeviceBuf<uint64_t> d_tvec, d_tvec_out;
    bool handed_records = false;    // a record reached the context since kta_create / kta_reset (kta_set_timeline refuses)
    // key sketch (KTA_FLAG_KEY_SKETCH): d_sketch u32[P * 4096] the live registers, d_sketch_out the u64 snapshot, d_sketch_floor
    // the floors of the sketch kernel's filter, d_sketch_stats its work counters (kta_key_sketch_info)
    bool sketch = false;
    DeviceBuf<uint32_t> d_sketch;
    DeviceBuf<uint64_t> d_sketch_out, d_sketch_stats;
    DeviceBuf<uint8_t> d_sketch_floor;
    uint64_t sketch_launches = 0;
    // hot keys (KTA_FLAG_HOT_KEYS): d_hot u64[2 * 1024 * 23] the live accumulator, d_hot_out its snapshot, d_hot_slots the
    // exemplar table, d_hot_ctl the words of its claiming [want 2048 | claim 2048 | mark 64], d_hot_stats the pass's counters
    bool hot = false;
    DeviceBuf<uint64_t> d_hot, d_hot_out, d_hot_stats;
    DeviceBuf<kta_hot_exemplar> d_hot_slots;
    DeviceBuf<uint32_t> d_hot_ctl;
    uint64_t hot_launches = 0, hot_workgroups = 0;
    uint32_t hot_flush_rounds = 0;   // kta_set_hot_flush_rounds (tests); 0: the most the fields admit
    // timestamp order (KTA_FLAG_TS_ORDER): d_tso u64[3 P + 64] the live vector, d_tso_out its snapshot, d_tso_hi i64[P] the
    // running maximum per partition (-1: none) that carries over from batch to batch, d_tso_ws the workspace of a launch
    // triple (allocated once), d_tso_stats the apply kernel's work counters (kta_ts_order_info)
    bool tso = false;
    DeviceBuf<uint64_t> d_tso, d_tso_out, d_tso_stats;
    DeviceBuf<int64_t> d_tso_hi, d_tso_ws;
    uint64_t tso_launches = 0, tso_chunks = 0, tso_last_chunk = 0;
    uint64_t tso_chunk = 0;          // kta_set_ts_order_chunk (tests); 0: by the slice's length
    // segments (kta_set_segments): d_seg u64[(P M + P) 4 + 8] the live vector, whose totals are the running state that carries
    // over from batch to batch, d_seg_ws / d_seg_flags the workspace of a launch triple (allocated once), d_seg_stats the
    // apply kernel's work counters (kta_segments_info)
    bool seg = false;
    uint64_t seg_S = 0;
    uint32_t seg_M = 0, seg_overhead = 0;
    DeviceBuf<uint64_t> d_seg, d_seg_out, d_seg_ws, d_seg_stats;   // (d_seg_out: the snapshot)
    DeviceBuf<uint32_t> d_seg_flags;
    uint64_t seg_launches = 0, seg_chunks = 0, seg_last_chunk = 0;
    uint64_t seg_chunk = 0;          // kta_set_segments_chunk (tests); 0: by the slice's length
    // partitioner (KTA_FLAG_PARTITIONER): d_part u64[2 P + 2 Q] the live vector, d_part_out its snapshot, d_part_stats the
    // kernel's work counters (kta_partitioner_info); part_q the what-if partition count (kta_set_repartition; P at first)
    bool part = false;
    uint32_t part_q = 0;
    DeviceBuf<uint64_t> d_part, d_part_out, d_part_stats;
    uint64_t part_launches = 0, part_workgroups = 0;
    // compaction what-if (KTA_FLAG_COMPACTION): d_comp u64[5 P + 6] the live vector, d_comp_stats the kernel's work counters
    // (kta_compaction_info); comp_replay the mode (kta_compaction_replay), comp_saved_seq the first pass's next_seq while it is on
    bool comp = false, comp_replay = false;
    uint64_t comp_saved_seq = 0;
    DeviceBuf<uint64_t> d_comp, d_comp_stats;
    uint64_t comp_launches = 0, comp_workgroups = 0;
    // compact,delete what-if (kta_set_compact_delete): d_kept u64[(P M + P) 4 + 8] the kept vector the replay writes, whose totals
    // are its running state, d_cd_cls the class column of one replay slice (a byte per record; grows to the largest slice
    // seen, at most 128 MiB), d_cd_stats the kept-apply kernel's work counters (kta_compact_delete_info).  The workspace and
    // the flags of the launch triple are the segment pass's: the two never run at the same time.
    bool cd = false;
    DeviceBuf<uint64_t> d_kept, d_cd_stats;
    DeviceBuf<uint8_t> d_cd_cls;
    uint64_t cd_launches = 0, cd_chunks = 0;
    // size percentiles (KTA_FLAG_SIZE_QUANTILES): d_sizeq u64[P * 3 * 464 + 8] the live vector, d_sizeq_out its snapshot,
    // d_sizeq_stats the kernel's work counters (kta_size_quantiles_info); sizeq_slice the tests' S (kta_set_size_quantiles_slice;
    // 0: the plan's), sizeq_variant the launch form (KTA_SIZEQ_VARIANT: 0, or the diagnostics 1 and 9 of tools/bench_size_quantiles.py)
    bool sizeq = false;
    DeviceBuf<uint64_t> d_sizeq, d_sizeq_out, d_sizeq_stats;
    uint32_t sizeq_slice = 0, sizeq_last_workgroups = 0;
    int sizeq_variant = 0;
    // record batches (KTA_FLAG_RECORD_BATCHES): d_rb u64[20 P + 1524] the live vector that kta_kafka.hip's decode call adds to
    // (kta_internal_blob_pass), d_rb_out its snapshot
    bool rb = false;
    DeviceBuf<uint64_t> d_rb, d_rb_out;
    // payload (KTA_FLAG_PAYLOAD): d_pl u64[24 P + 69648] the live vector that the decode call adds to (kta_internal_blob_pass),
    // d_pl_out its snapshot
    bool pl = false;
    DeviceBuf<uint64_t> d_pl, d_pl_out;
    // header names (KTA_FLAG_HEADER_NAMES): d_hn u64[73736] the live vector that the decode call adds to
    // (kta_internal_blob_pass), d_hn_out its snapshot, d_hn_names the name table beside it (not snapshotted, not exchanged),
    // d_hn_info the pass's work counters
    bool hn = false;
    DeviceBuf<uint64_t> d_hn, d_hn_out, d_hn_info;
    DeviceBuf<kta_header_name> d_hn_names;
    // value bytes (KTA_FLAG_VALUE_BYTES): d_vb u64[264 P] the live vector that the decode call adds to (kta_internal_blob_pass),
    // d_vb_out its snapshot, d_vb_info the pass's work counters, vb_variant the launch form (KTA_VALUE_BYTES_VARIANT: 0, or 1
    // of tools/bench_value_bytes.py)
    bool vb = false;
    int vb_variant = 0;
    DeviceBuf<uint64_t> d_vb, d_vb_out, d_vb_info;
    // compression what-if (KTA_FLAG_COMPRESS_WHATIF): d_cw u64[8 P + 20] the live vector that the decode call adds to
    // (kta_internal_blob_pass), d_cw_out its snapshot
    bool cw = false;
    DeviceBuf<uint64_t> d_cw, d_cw_out;
    // record filter (kta_set_filter): the window and the set, d_filter_bitmap the set's ceil(P / 32) words, the workspace of a
    // slice's three launches (allocated at the first filtered batch), h_filter_total the slice's total as the host reads
    // it, and the scratch batch the passing records go to (raw layout; grows to the largest slice seen)
    bool filter = false;
    kta::FilterSpec filter_spec{INT64_MIN, INT64_MAX, 0, 0};
    uint64_t filter_slice = kta::kFilterSlice;
    DeviceBuf<uint32_t> d_filter_bitmap, d_filter_count;
    DeviceBuf<uint64_t> d_filter_offset, d_filter_stats;
    PinnedBuf<uint64_t> h_filter_total;
    uint64_t *d_filter_total = nullptr;   // h_filter_total as the device addresses it
    DeviceBuf<uint8_t> d_filter_scratch;
    kta_batch filter_scratch{};      // column pointers into d_filter_scratch
    uint64_t filter_seen = 0, filter_passed = 0, filter_slices = 0;
    DeviceBuf<uint64_t> d_vec;      // u64[P*7 + KTA_NGLOBALS]: the live accumulator
    DeviceBuf<uint64_t> d_vec_out;  // its snapshot (kta_finish_device): what kta_result_vector hands out and the
                                    // exchange reduces in place — the accumulator itself is never reduced
    DeviceBuf<uint64_t> d_partials; // scan workspace: max_rows x row_len
    uint32_t max_rows = 0;
    // -c: the persistent state is ONE of
    //   d_bitmap  the reference's bit set, u32[2^27] (default: batches are applied in submission order), or
    //   d_table   u64[2^32] last-writer table (KTA_FLAG_ALIVE_TABLE / KTA_FLAG_SEQ_COLUMN: global sequence numbers)
    bool alive_table = false;
    DeviceBuf<uint32_t> d_bitmap;
    DeviceBuf<uint64_t> d_table;
    DeviceBuf<int64_t> d_alive_running; // running alive count
    bool running_valid = true;          // false once an update ran without counting
    // table state: the slots ever written (what the exchange exports); invalid once somebody else wrote the table
    DeviceBuf<uint32_t> d_written;  // (its size is the list's capacity)
    DeviceBuf<unsigned long long> d_written_n;
    bool written_valid = true;
    DeviceBuf<uint32_t> d_exp_slots;    // kta_alive_export_entries buffers
    DeviceBuf<uint64_t> d_exp_vals, d_exp_count;
    DeviceBuf<uint32_t> d_hash_scratch; // ablation variants only
    DeviceBuf<uint64_t> d_pairs;        // partitioned alive pass: (hash, local seq, alive) pairs by [workgroup][bucket]
    DeviceBuf<uint32_t> d_pair_counts;  //   and the fill of every segment, [bucket][workgroup]
    DeviceBuf<uint64_t> d_pool;         //   pairs whose segment was full (8 words more than the plan's pool_words)
    DeviceBuf<uint8_t> d_pool_ctl;      //   pool cursor, histogram, order flag
    DeviceBuf<uint32_t> d_fail_from;    //   buckets handed to the fallback kernel (bit set state)
    // Feedback for the automatic choice (alive_variant 3 / 4): the partitioned pass pays when records die in
    // LDS (a compacted topic repeats its keys inside a batch); a batch of mostly unique keys is cheaper in
    // the single-kernel update.  Every partitioned batch reports [pairs, entries claimed]; a batch that
    // claimed more than kAliveUniqueNum / kAliveUniqueDen of its pairs sends the next kAliveBackoff batches
    // down the single-kernel path before the partitioned pass is tried again.
    DeviceBuf<uint64_t> d_alive_stats;
    PinnedBuf<uint64_t> h_alive_stats;
    Event ev_alive_stats;
    bool alive_stats_pending = false;
    bool fuse_handlers = true;      // both handlers of a batch in one pass where that is possible (KTA_NO_FUSE=1: never)
    DeviceBuf<uint64_t> d_failed_total; // buckets handed to kta_alive_fallback since create / reset (kta_alive_pass_info)
    int alive_backoff = 0;
    // what the partitioned pass did since kta_create / kta_reset (kta_alive_pass_info): launch pairs, of them with both
    // handlers in the one pass, of them with the metrics handler through the scan although the batch began fused, and the
    // buckets that the sampled launches (the last one of every batch of 2^24 records and more, bit set state) handed to
    // kta_alive_fallback; the word comes back with the stream and is never waited for
    uint64_t info_slices = 0, info_fused = 0, info_scanned = 0, info_failed_buckets = 0;
    std::vector<Stage> stages;
    // the tile-compact batches kta_device_batch_alloc handed out (as allocated): a raw-layout kta_batch whose columns point
    // inside one of them is a view of it at a record offset (kta_internal_resolve)
    std::vector<kta_batch> compact_batches;
    uint64_t batch_capacity = 0, key_bytes_capacity = 0;
    int cur = 0;
    bool acquired = false;
    uint64_t fill_n = 0, fill_kb = 0; // kta_handle_message fill state
    uint64_t msg_count = 0, msg_flushes = 0, msg_flush_ns = 0, msg_wait_ns = 0;   // kta_handle_message_stats
    uint64_t next_seq = 0;
    // tuning / profiling
    int scan_wgs = 0, scan_variant = 16, alive_wgs = 0, alive_variant = 3; // 16: non-temporal loads; 3: partitioned pass for large batches
    bool timing = false;
    // HIP-event pairs recorded around each kernel on the compute stream (no host sync while
    // recording); drained by kta_kernel_time_stats.  kind: 0 scan, 1 fold, 2 alive update.
    TimerPool<3> timers{2 * kMaxTimedPairs};
    // extension state owned by another translation unit of the library (kta_kafka.hip)
    void *ext_state = nullptr;
    void (*ext_free)(void *) = nullptr;
    void *comm_state = nullptr;     // kta_comm.hip
    void (*comm_free)(void *) = nullptr;
    std::string err;
};

int kta_internal_fail(kta_ctx *ctx, int code, const std::string &msg)
{
    if (ctx) ctx->err = msg; else g_create_error = msg;
    return code;
}

namespace {

uint64_t now_ns()
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }

uint64_t tiles_of(uint64_t n) { return (n + KTA_TILE_RECORDS - 1) / KTA_TILE_RECORDS; }

// Tile-compact (kta_hip.h): the columns cover whole tiles, so that a kernel may read any record of a tile the batch touches.
int alloc_device_batch(kta_ctx *ctx, uint64_t cap, uint64_t kcap, bool keys, bool seq, kta_batch *b)
{
    memset(b, 0, sizeof(*b));
    b->capacity = cap;
    b->key_bytes_capacity = keys ? kcap : 0;
    b->layout = KTA_LAYOUT_TILE_COMPACT;
    const uint64_t ntiles = tiles_of(cap) ? tiles_of(cap) : 1;
    const uint64_t rows = ntiles * KTA_TILE_RECORDS;
    const size_t c4 = pad16(rows * 4 + 16), c8 = pad16(rows * 8 + 16);
    // (the tiles' summaries behind the headers, their plane marks behind those, the size extrema last: kta::tile_sums_behind,
    // tile_marks_behind, tile_sizes_behind)
    KTA_HIP(ctx, hipMalloc((void **)&b->tile_hdr, ntiles * kta::kTileSideBytes));
    KTA_HIP(ctx, hipMemset(b->tile_hdr, 0, ntiles * kta::kTileSideBytes));   // every tile raw, no summary, no plane
    KTA_HIP(ctx, hipMalloc((void **)&b->partition, c4));
    KTA_HIP(ctx, hipMalloc((void **)&b->key_len, c4));
    KTA_HIP(ctx, hipMalloc((void **)&b->val_len, c4));
    KTA_HIP(ctx, hipMalloc((void **)&b->ts_ms, c8));
    if (keys) {
        KTA_HIP(ctx, hipMalloc((void **)&b->key_off, c4));
        KTA_HIP(ctx, hipMalloc((void **)&b->key_bytes, pad16(kcap + 16)));
    }
    if (seq) KTA_HIP(ctx, hipMalloc((void **)&b->seq, c8));
    return KTA_OK;
}

void free_device_batch(kta_batch *b)
{
    if (b->partition) (void)hipFree(b->partition);
    if (b->key_len) (void)hipFree(b->key_len);
    if (b->val_len) (void)hipFree(b->val_len);
    if (b->ts_ms) (void)hipFree(b->ts_ms);
    if (b->key_off) (void)hipFree(b->key_off);
    if (b->key_bytes) (void)hipFree(b->key_bytes);
    if (b->seq) (void)hipFree(b->seq);
    if (b->tile_hdr) (void)hipFree(b->tile_hdr);
    memset(b, 0, sizeof(*b));
}

// A device batch as the kernels take it is a kta_internal_columns (kta_internal.h).  hdr == null: the raw layout, the
// pointers are the caller's.  Otherwise a tile-compact allocation: the pointers address its record 0 and the batch starts
// at its record rec0 — the allocation itself (rec0 0), or a raw-layout kta_batch whose columns point inside one of the
// context's tile-compact allocations (a view built by pointer arithmetic, rec0 = the offset).

uint64_t allocation_rows(const kta_batch &e) { return (tiles_of(e.capacity) ? tiles_of(e.capacity) : 1) * KTA_TILE_RECORDS; }

// The tile-compact allocation of the context whose column `col` (partition or key_len) holds the address p, and the
// record of it that p lies in; null: none does.
kta_batch *find_allocation(kta_ctx *ctx, const int32_t *p, int32_t *kta_batch::*col, uint64_t *rec0)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    for (kta_batch &e : ctx->compact_batches) {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(e.*col);
        if (!p || a < lo || a >= lo + allocation_rows(e) * 4) continue;
        *rec0 = (a - lo) / 4;
        return &e;
    }
    return nullptr;
}

// The columns of records [at, ...) of a resolved batch, in either layout: a raw batch's pointers move, a tile-compact
// batch keeps the allocation's record 0 and its first record moves.
kta_internal_columns columns_at(const kta_internal_columns &rb, uint64_t at)
{
    kta_internal_columns r = rb;
    r.rec0 += at;
    if (!rb.hdr) r.partition += at, r.key_len += at, r.val_len += at, r.ts_ms += at;
    return r;
}
kta::ScanColumns scan_columns(const kta_internal_columns &rb, uint64_t at)
{
    const kta_internal_columns r = columns_at(rb, at);
    return kta::ScanColumns{r.partition, r.key_len, r.val_len, r.ts_ms, r.hdr, r.rec0, r.sum, r.mark, r.size};
}
// (the key-reading passes take the lengths and the keys from the batch's own columns: plain i32 in both layouts)
kta::SketchColumns sketch_columns(const kta_internal_columns &rb, const kta_batch *c, uint64_t at)
{
    const kta_internal_columns r = columns_at(rb, at);
    return kta::SketchColumns{r.partition, r.hdr, r.rec0, c->key_len + at, c->key_off + at, c->key_bytes};
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Before a pass that reads plain i32 lengths next to keys (the alive-key pass, the key sketch, the hot keys, the partitioner) runs over
// records [0, n) of c: when c's length columns lie in a keyless allocation — a view of it handed over with key columns
// of the caller's own —, the u16 tiles the range touches are widened in place (exact; one small pass, and none when the
// lengths are the caller's own or a keyed allocation's).
int widen_lens_for_keys(kta_ctx *ctx, const kta_batch *c, uint64_t n)
{
    uint64_t rec0 = 0;
    const kta_batch *e = find_allocation(ctx, c->key_len, &kta_batch::key_len, &rec0);
    if (!e || e->key_bytes) return KTA_OK;
    const uint64_t rows = allocation_rows(*e), hi = rec0 + n < rows ? rec0 + n : rows;
    KTA_HIP(ctx, kta::launch_tiles_to_raw(e->partition, e->ts_ms, e->key_len, e->val_len, e->tile_hdr, rec0, hi, 2u, true, ctx->s_compute));
    return KTA_OK;
}

constexpr uint64_t kAliveUniqueNum = 2, kAliveUniqueDen = 5;   // > 40 % of a batch's pairs claimed an entry: mostly unique keys
constexpr int kAliveBackoff = 7;

kta::WrittenList written_list(kta_ctx *ctx) { return kta::WrittenList{ctx->d_written.get(), ctx->d_written_n.get(), ctx->d_written.size()}; }

// A pass that takes a batch in slices that double from lo records to hi: launch(at, take) per slice.
template <class F> int for_doubling_slices(uint64_t n, uint64_t lo, uint64_t hi, F launch)
{
    for (uint64_t at = 0, slice = lo; at < n; slice = slice < hi ? slice * 2 : slice) {
        const uint64_t take = n - at < slice ? n - at : slice;
        int rc = launch(at, take);
        if (rc != KTA_OK) return rc;
        at += take;
    }
    return KTA_OK;
}

// The key sketch over a batch whose metric columns were resolved to rb.  A launch takes a slice, and the floors of its
// filter are refreshed from the registers before each: the slices double from 2^20 records to 2^26, so that the floors
// of a fresh sketch rise within the first large batch.
constexpr uint64_t kSketchSliceMin = 1ull << 20, kSketchSliceMax = 1ull << 26;
int run_key_sketch(kta_ctx *ctx, const kta_batch *c, const kta_internal_columns &rb, uint64_t n)
{
    return for_doubling_slices(n, kSketchSliceMin, kSketchSliceMax, [&](uint64_t at, uint64_t take) -> int {
        KTA_HIP(ctx, kta::launch_key_sketch_floor(ctx->d_sketch.get(), ctx->P, ctx->d_sketch_floor.get(), ctx->s_compute));
        KTA_HIP(ctx, kta::launch_key_sketch(sketch_columns(rb, c, at), take, ctx->P, ctx->d_sketch.get(), ctx->d_sketch_floor.get(),
                                            ctx->d_sketch_stats.get(), ctx->cu_count, ctx->s_compute));
        ctx->sketch_launches++;
        return KTA_OK;
    });
}

// The hot-key pass over a batch whose metric columns were resolved to rb.  A launch takes a slice, and the candidates its
// exemplars go by are computed from the accumulator before each: the slices double from 2^16 records to 2^26, so that the
// heavy keys of a topic's first batch get their exemplars within it.
constexpr uint64_t kHotSliceMin = 1ull << 16, kHotSliceMax = 1ull << 26;
constexpr size_t kHotSlotsN = (size_t)KTA_HOT_ROWS * KTA_HOT_CELLS;
kta::HotState hot_state(kta_ctx *ctx)
{
    uint32_t *ctl = ctx->d_hot_ctl.get();
    return kta::HotState{ctx->d_hot.get(), ctx->d_hot_slots.get(), ctl, ctl + 2 * kHotSlotsN, ctl + kHotSlotsN, ctx->d_hot_stats.get()};
}
int run_hot_keys(kta_ctx *ctx, const kta_batch *c, const kta_internal_columns &rb, uint64_t n)
{
    const kta::HotState st = hot_state(ctx);
    return for_doubling_slices(n, kHotSliceMin, kHotSliceMax, [&](uint64_t at, uint64_t take) -> int {
        uint32_t wgs = 0;
        KTA_HIP(ctx, kta::launch_hot_keys(sketch_columns(rb, c, at), take, ctx->P, st, ctx->hot_flush_rounds, ctx->cu_count, &wgs, ctx->s_compute));
        ctx->hot_launches++;
        ctx->hot_workgroups += wgs;
        return KTA_OK;
    });
}

// The partitioner pass over a batch whose metric columns were resolved to rb, in launches of at most 2^30 records (the
// u32 fields of its LDS counters).
int run_partitioner(kta_ctx *ctx, const kta_batch *c, const kta_internal_columns &rb, uint64_t n)
{
    for (uint64_t at = 0; at < n;) {
        const uint64_t take = n - at < kta::kPartitionerLaunchMax ? n - at : kta::kPartitionerLaunchMax;
        uint32_t wgs = 0;
        KTA_HIP(ctx, kta::launch_partitioner(kta::PartitionerColumns{sketch_columns(rb, c, at), c->val_len + at}, take, ctx->P, ctx->part_q,
                                             ctx->d_part.get(), ctx->d_part_stats.get(), ctx->cu_count, &wgs, ctx->s_compute));
        ctx->part_launches++;
        ctx->part_workgroups += wgs;
        at += take;
    }
    return KTA_OK;
}

// The size-percentile pass over a batch whose metric columns were resolved to rb, in launches of at most 2^30 records (the
// u32 counters of its LDS slices).  It reads the tiles' own forms: nothing is widened for it.
constexpr size_t kSizeqStatWords = 8;
int run_size_quantiles(kta_ctx *ctx, const kta_internal_columns &rb, uint64_t n)
{
    for (uint64_t at = 0; at < n;) {
        const uint64_t take = n - at < kta::kSizeQuantilesLaunchMax ? n - at : kta::kSizeQuantilesLaunchMax;
        uint32_t wgs = 0;
        KTA_HIP(ctx, kta::launch_size_quantiles(scan_columns(rb, at), take, ctx->P, ctx->sizeq_slice, ctx->sizeq_variant, ctx->d_sizeq.get(),
                                                ctx->d_sizeq_stats.get(), ctx->cu_count, &wgs, ctx->s_compute));
        ctx->sizeq_last_workgroups = wgs;
        at += take;
    }
    return KTA_OK;
}

// The compaction pass over a batch whose metric columns were resolved to rb, in launches of at most 2^30 records (the
// halves of its LDS word W0).
int run_compaction(kta_ctx *ctx, const kta_batch *c, const kta_internal_columns &rb, uint64_t n, uint64_t base_seq)
{
    for (uint64_t at = 0; at < n;) {
        const uint64_t take = n - at < kta::kCompactionLaunchMax ? n - at : kta::kCompactionLaunchMax;
        uint32_t wgs = 0;
        KTA_HIP(ctx, kta::launch_compaction(kta::CompactionColumns{sketch_columns(rb, c, at), c->val_len + at, c->seq ? c->seq + at : nullptr}, take,
                                            base_seq + at, ctx->P, ctx->d_table.get(), ctx->d_comp.get(), ctx->d_comp_stats.get(), ctx->cu_count,
                                            &wgs, ctx->s_compute));
        ctx->comp_launches++;
        ctx->comp_workgroups += wgs;
        at += take;
    }
    return KTA_OK;
}

// The replay of a context with kta_set_compact_delete on: per slice the compaction launch, which also writes the slice's class
// column, then the kept-row triple over the same records.  The chunk is run_segments' (kta_set_segments_chunk included);
// a slice is as many chunks as the workspace has rows for, and no more records than the class column's 128 MiB hold.
int run_compact_delete(kta_ctx *ctx, const kta_batch *c, const kta_internal_columns &rb, uint64_t n, uint64_t base_seq)
{
    const kta::SegmentsState st{ctx->d_kept.get(), ctx->d_seg_ws.get(), ctx->d_seg_flags.get(), ctx->d_cd_stats.get(), ctx->seg_S, ctx->seg_M,
                                ctx->seg_overhead};
    const uint64_t max_rows = kta::kSegmentsWorkspaceWords / ((uint64_t)ctx->P * kta::kSegWords);
    for (uint64_t at = 0; at < n;) {
        const uint64_t left = n - at;
        uint64_t chunk = ctx->seg_chunk;
        if (chunk == 0) {
            chunk = ((left + kta::kSegmentsChunks - 1) / kta::kSegmentsChunks + 255) / 256 * 256;
            if (chunk < kta::kSegmentsChunkMin) chunk = kta::kSegmentsChunkMin;
        }
        uint64_t take = left / chunk >= max_rows ? max_rows * chunk : left;
        if (take > kta::kCompactDeleteScratchBytes)
            take = chunk <= kta::kCompactDeleteScratchBytes ? kta::kCompactDeleteScratchBytes / chunk * chunk : kta::kCompactDeleteScratchBytes;
        if (ctx->d_cd_cls.size() < take) {
            KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));   // (an earlier slice may still read the old column)
            KTA_HIP(ctx, ctx->d_cd_cls.alloc(take));
        }
        uint32_t wgs = 0;
        KTA_HIP(ctx, kta::launch_compaction(kta::CompactionColumns{sketch_columns(rb, c, at), c->val_len + at, c->seq ? c->seq + at : nullptr}, take,
                                            base_seq + at, ctx->P, ctx->d_table.get(), ctx->d_comp.get(), ctx->d_comp_stats.get(), ctx->cu_count,
                                            &wgs, ctx->s_compute, ctx->d_cd_cls.get()));
        ctx->comp_launches++;
        ctx->comp_workgroups += wgs;
        KTA_HIP(ctx, kta::launch_kept_rows(scan_columns(rb, at), ctx->d_cd_cls.get(), take, chunk, ctx->P, st, ctx->s_compute));
        ctx->cd_launches += 3;
        ctx->cd_chunks += (take + chunk - 1) / chunk;
        at += take;
    }
    return KTA_OK;
}

// A batch of the replay (kta_compaction_replay): the compaction pass — with kta_set_compact_delete, the kept rows behind it —
// and nothing else, whatever `which` says.
int run_replayed_batch(kta_ctx *ctx, const kta_batch *c, uint64_t n, uint64_t base_seq)
{
    // every refusal comes before the first launch
    if (!c->partition || !c->key_len || !c->val_len) return fail(ctx, KTA_ERR_INVALID, "metric columns missing");
    if (!c->key_off || !c->key_bytes) return fail(ctx, KTA_ERR_INVALID, "key columns missing (KTA_FLAG_COMPACTION)");
    kta_internal_columns rb{};
    int rc = kta_internal_resolve(ctx, c, &rb);
    if (rc != KTA_OK) return rc;
    rc = widen_lens_for_keys(ctx, c, n);
    if (rc != KTA_OK) return rc;
    if (ctx->cd) return run_compact_delete(ctx, c, rb, n, base_seq);
    return run_compaction(ctx, c, rb, n, base_seq);
}

// The timestamp-order pass over a batch whose metric columns were resolved to rb: chunk maxima, prefix, apply per slice,
// in order.  A slice is as many chunks as the workspace has rows for P partitions; the chunk is the slice over
// kTsOrderChunks (enough waves to fill the device a few times over), a multiple of 256 records, or the tests' own.
int run_ts_order(kta_ctx *ctx, const kta_internal_columns &rb, uint64_t n)
{
    const kta::TsOrderState st{ctx->d_tso.get(), ctx->d_tso_hi.get(), ctx->d_tso_ws.get(), ctx->d_tso_stats.get()};
    const uint64_t max_rows = kta::kTsOrderWorkspaceWords / ctx->P;
    for (uint64_t at = 0; at < n;) {
        const uint64_t left = n - at;
        uint64_t chunk = ctx->tso_chunk;
        if (chunk == 0) {
            chunk = ((left + kta::kTsOrderChunks - 1) / kta::kTsOrderChunks + 255) / 256 * 256;
            if (chunk < kta::kTsOrderChunkMin) chunk = kta::kTsOrderChunkMin;
        }
        const uint64_t take = left / chunk >= max_rows ? max_rows * chunk : left;
        KTA_HIP(ctx, kta::launch_ts_order(scan_columns(rb, at), take, chunk, ctx->P, st, ctx->s_compute));
        ctx->tso_launches++;
        ctx->tso_chunks += (take + chunk - 1) / chunk;
        ctx->tso_last_chunk = chunk;
        at += take;
    }
    return KTA_OK;
}

// The segment pass over a batch whose metric columns were resolved to rb, as run_ts_order: chunk sums, prefix, apply per
// slice, in order.  A slice is as many chunks as the workspace has rows for P partitions.
int run_segments(kta_ctx *ctx, const kta_internal_columns &rb, uint64_t n)
{
    const kta::SegmentsState st{ctx->d_seg.get(), ctx->d_seg_ws.get(), ctx->d_seg_flags.get(), ctx->d_seg_stats.get(), ctx->seg_S, ctx->seg_M,
                                ctx->seg_overhead};
    const uint64_t max_rows = kta::kSegmentsWorkspaceWords / ((uint64_t)ctx->P * kta::kSegWords);
    for (uint64_t at = 0; at < n;) {
        const uint64_t left = n - at;
        uint64_t chunk = ctx->seg_chunk;
        if (chunk == 0) {
            chunk = ((left + kta::kSegmentsChunks - 1) / kta::kSegmentsChunks + 255) / 256 * 256;
            if (chunk < kta::kSegmentsChunkMin) chunk = kta::kSegmentsChunkMin;
        }
        const uint64_t take = left / chunk >= max_rows ? max_rows * chunk : left;
        KTA_HIP(ctx, kta::launch_segments(scan_columns(rb, at), take, chunk, ctx->P, st, ctx->s_compute));
        ctx->seg_launches++;
        ctx->seg_chunks += (take + chunk - 1) / chunk;
        ctx->seg_last_chunk = chunk;
        at += take;
    }
    return KTA_OK;
}

// The workspace of the partitioned alive pass, large enough for plan pl: the pairs, their counts and the pool grow
// together (all three released, after the compute stream has drained, before any is allocated again); the pool's control
// words and the fail lists are allocated once.
int grow_alive_workspace(kta_ctx *ctx, const kta::AlivePartitionPlan &pl)
{
    if (ctx->d_pairs.size() < pl.pair_words || ctx->d_pair_counts.size() < pl.count_words ||
        ctx->d_pool.size() < pl.pool_words + 8) {
        KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));
        ctx->d_pairs.reset();
        ctx->d_pair_counts.reset();
        ctx->d_pool.reset();
        KTA_HIP(ctx, ctx->d_pairs.alloc(pl.pair_words));
        KTA_HIP(ctx, ctx->d_pair_counts.alloc(pl.count_words));
        KTA_HIP(ctx, ctx->d_pool.alloc(pl.pool_words + 8));
    }
    if (!ctx->d_pool_ctl) KTA_HIP(ctx, ctx->d_pool_ctl.alloc(pl.ctl_bytes));
    // (per bucket + the list of given-up buckets + the list for the slot-range passes)
    if (!ctx->d_fail_from) KTA_HIP(ctx, ctx->d_fail_from.alloc((size_t)3 << pl.bucket_log2));
    return KTA_OK;
}

// Launch the handlers over device-resident columns on the compute stream.
int run_handlers(kta_ctx *ctx, const kta_batch *c, uint64_t n, uint64_t base_seq, int which)
{
    if (n == 0) return KTA_OK;
    if (ctx->comp_replay) return run_replayed_batch(ctx, c, n, base_seq);   // behind the filter: the passing records, the numbers they kept
    const kta::TimelineArgs *tl = ctx->timeline ? &ctx->tl : nullptr;
    const uint32_t tl_buckets = ctx->timeline ? ctx->tl.n_buckets : 0u;
    hipEvent_t a = nullptr, b = nullptr;
    // every refusal comes before the first launch: a batch is counted by both handlers or by neither
    if ((which & 2) && ctx->alive && (!c->key_len || !c->val_len || !c->key_off || !c->key_bytes))
        return fail(ctx, KTA_ERR_INVALID, "key columns missing (count_alive_keys)");
    if ((which & 1) && ctx->sketch && (!c->key_off || !c->key_bytes))
        return fail(ctx, KTA_ERR_INVALID, "key columns missing (KTA_FLAG_KEY_SKETCH)");
    if ((which & 1) && ctx->hot && (!c->key_off || !c->key_bytes))
        return fail(ctx, KTA_ERR_INVALID, "key columns missing (KTA_FLAG_HOT_KEYS)");
    if ((which & 1) && ctx->part && (!c->key_off || !c->key_bytes))
        return fail(ctx, KTA_ERR_INVALID, "key columns missing (KTA_FLAG_PARTITIONER)");
    // Table state: which kernels take the batch is decided before anything is launched (the fused pass below depends on it).
    // 3 = the partitioned pass for batches of >= 2^21 records (13: for batches of any size — tests), with the automatic
    // fall-back to the single-kernel filtered update (2) for batches of mostly unique keys; 1 / 2 / 8 / 9 = the
    // single-kernel variants.  Bit set state: every batch takes the partitioned pass.
    const bool part_kind = ctx->alive_variant == 3 || ctx->alive_variant == 13 || ctx->alive_variant == 4 || ctx->alive_variant == 14;
    const bool partitioned = !ctx->alive_table || (part_kind && (n >= kta::kAlivePartitionMin || ctx->alive_variant >= 13));
    bool use_partitioned = partitioned;
    if ((which & 2) && ctx->alive && partitioned && ctx->alive_table && ctx->alive_variant < 13) {   // automatic choice only (13 forces it)
        if (ctx->alive_stats_pending && hipEventQuery(ctx->ev_alive_stats.get()) == hipSuccess) {
            ctx->alive_stats_pending = false;
            const uint64_t pairs = ctx->h_alive_stats.get()[0], claims = ctx->h_alive_stats.get()[1];
            if (pairs && claims * kAliveUniqueDen > pairs * kAliveUniqueNum) ctx->alive_backoff = kAliveBackoff;
        }
        if (ctx->alive_backoff > 0) {
            ctx->alive_backoff--;
            use_partitioned = false;
        }
    }
    // Both handlers over one batch (what kafka.rs:107-109 does with every message): with at most 256 partitions, pass 1 of
    // the partitioned alive-key pass does the metrics handler's work as well (kta_alive.hip, FuseArgs) — the batch is read
    // once: 40 B + key per record instead of 20 + 28 in the bit set state, 48 B + key instead of 20 + 36 for a sharded
    // rank's batch with its seq column (table state).  The fused pass has no LDS room for the analytics or the timeline.
    bool fuse = false;
    if (which == 3 && ctx->alive && use_partitioned && !ctx->analytics && !ctx->timeline && ctx->fuse_handlers) {
        const uint64_t first = n > kta::kAlivePartitionMax ? kta::kAlivePartitionMax : n;
        const kta::AlivePartitionPlan pl0 = kta::plan_alive_partition(first, ctx->alive_wgs, ctx->cu_count, !ctx->alive_table);
        fuse = kta::alive_fuse_possible(pl0, ctx->P) && pl0.segment_wgs <= ctx->max_rows;
    }
    if (which & 1) {
        if (!c->partition || !c->key_len || !c->val_len || !c->ts_ms)
            return fail(ctx, KTA_ERR_INVALID, "metric columns missing");
        if (!aligned16(c->partition) || !aligned16(c->key_len) || !aligned16(c->val_len) ||
            !aligned16(c->ts_ms))
            return fail(ctx, KTA_ERR_INVALID, "device columns must be 16-byte aligned");
    }
    kta_internal_columns rb{};
    if (which & 1) {
        int rc = kta_internal_resolve(ctx, c, &rb);
        if (rc != KTA_OK) return rc;
        // (the size-percentile pass loads whole 16-byte groups of an allocation's tiles)
        if (ctx->sizeq && rb.rows && rb.rec0 + n > rb.rows) return fail(ctx, KTA_ERR_INVALID, "the batch ends behind its allocation (KTA_FLAG_SIZE_QUANTILES)");
    }
    if (((which & 2) && ctx->alive) || ((which & 1) && (ctx->sketch || ctx->hot || ctx->part))) {
        int rc = widen_lens_for_keys(ctx, c, n);
        if (rc != KTA_OK) return rc;
    }
    // The metrics handler over records [at, at + m): plan the scan, clamp it to the partial workspace, launch it and
    // fold its rows.  timed: with the event pairs of kinds 0 (scan) and 1 (fold) around the two launches.
    auto scan_and_fold = [&](uint64_t at, uint64_t m, bool timed) -> int {
        const kta::ScanColumns sc = scan_columns(rb, at);
        kta::ScanPlan pl = kta::plan_scan(ctx->P, m, ctx->cu_count, ctx->scan_wgs, ctx->scan_variant, ctx->analytics,
                                          sc.hdr != nullptr, tl_buckets);
        if (pl.workgroups > ctx->max_rows) pl.workgroups = ctx->max_rows;
        if (timed) {
            int rc = ctx->timers.pair(ctx, ctx->s_compute, 0, &a, &b);
            if (rc != KTA_OK) return rc;
            KTA_HIP(ctx, hipEventRecord(a, ctx->s_compute));
        }
        KTA_HIP(ctx, kta::launch_metrics_scan(pl, sc, m, ctx->P, ctx->d_partials.get(), ctx->s_compute, tl));
        if (timed) {
            KTA_HIP(ctx, hipEventRecord(b, ctx->s_compute));
            int rc = ctx->timers.pair(ctx, ctx->s_compute, 1, &a, &b);
            if (rc != KTA_OK) return rc;
            KTA_HIP(ctx, hipEventRecord(a, ctx->s_compute));
        }
        KTA_HIP(ctx, kta::launch_fold_partials(ctx->d_partials.get(), pl.workgroups, ctx->P, ctx->d_vec.get(), pl.row_len, ctx->d_avec.get(),
                                               ctx->s_compute));
        if (timed) KTA_HIP(ctx, hipEventRecord(b, ctx->s_compute));
        return KTA_OK;
    };
    if ((which & 1) && !fuse) {
        ctx->handed_records = true;
        int rc = scan_and_fold(0, n, ctx->timing);
        if (rc != KTA_OK) return rc;
    }
    if ((which & 2) && ctx->alive) {
        kta::AliveColumns ac{c->key_len, c->val_len, c->key_off, c->key_bytes, c->seq};
        if (ctx->timing) {
            int rc = ctx->timers.pair(ctx, ctx->s_compute, 2, &a, &b);
            if (rc != KTA_OK) return rc;
            KTA_HIP(ctx, hipEventRecord(a, ctx->s_compute));
        }
        if (ctx->alive_table && (ctx->alive_variant == 8 || ctx->alive_variant == 9) && ctx->d_hash_scratch.size() < n) {
            KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));
            KTA_HIP(ctx, ctx->d_hash_scratch.alloc(n));
        }
        // Bit set state: every batch takes the partitioned pass (hash + partition, per-bucket merge in LDS, the
        // bucket's bitmap region streamed through LDS); batches are applied in submission order, base_seq and a
        // seq column are not looked at.
        // Table state: the choice made above.  A seq column has to ascend inside a batch for the partitioned pass (the
        // merge orders a batch's records by their index): checked on the device, and a batch that fails the check runs
        // the filtered update instead, conditionally, without a host round trip.  (Both partition kernels read their
        // columns 4 bytes per lane: any alignment will do.)
        if (ctx->alive_table && ctx->alive_variant != 1 && ctx->alive_variant != 2 && !part_kind) ctx->running_valid = false;   // non-counting kernels
        if (use_partitioned) {
            if (!ctx->d_alive_stats) {   // (four words: builds with KTA_ALIVE_PHASES add instalments and side-table entries)
                KTA_HIP(ctx, ctx->d_alive_stats.alloc(4));
                KTA_HIP(ctx, ctx->h_alive_stats.alloc(4));
                KTA_HIP(ctx, hipEventCreateWithFlags(ctx->ev_alive_stats.put(), hipEventDisableTiming));
            }
            const bool report = ctx->alive_table && !ctx->alive_stats_pending;       // one report in flight at a time
            // Bit set state: a bucket with more distinct slots than pass 2's LDS table takes is applied in instalments (careful
            // mode, groups of segments sized to fit the table: kta_alive.hip); what defeats that too — hot keys that overflow
            // their segments into the pool, one group's segments all in one set — goes to kta_alive_fallback, exact and slow.
            // The number of such buckets is sampled for kta_alive_pass_info.  (Round 4 applied the batches that followed one
            // with such buckets in slices of 2^26 records; with the groups sized from the fills a whole batch of config 5's
            // law takes 8.2 ms where four slices took 10.1, and the slicing went.)
            if (!ctx->d_failed_total) {
                KTA_HIP(ctx, ctx->d_failed_total.alloc(1));
                KTA_HIP(ctx, hipMemsetAsync(ctx->d_failed_total.get(), 0, sizeof(uint64_t), ctx->s_compute));
            }
            if (report) KTA_HIP(ctx, hipMemsetAsync(ctx->d_alive_stats.get(), 0, 4 * sizeof(uint64_t), ctx->s_compute));
            for (uint64_t at = 0; at < n;) {
                const uint64_t left = n - at;
                kta::AlivePartitionPlan pl = kta::plan_alive_partition(left, ctx->alive_wgs, ctx->cu_count, !ctx->alive_table);
                const uint64_t take = left < pl.max_records ? left : pl.max_records;
                int rc = grow_alive_workspace(ctx, pl);
                if (rc != KTA_OK) return rc;
                kta::AliveColumns sl{c->key_len + at, c->val_len + at, c->key_off + at, c->key_bytes,
                                     ctx->alive_table && c->seq ? c->seq + at : nullptr};
                kta::AliveState st{ctx->alive_table ? ctx->d_table.get() : nullptr, ctx->alive_table ? nullptr : ctx->d_bitmap.get(),
                                   ctx->d_alive_running.get(), written_list(ctx)};
                kta::AliveWorkspace ws{ctx->d_pairs.get(), ctx->d_pair_counts.get(), ctx->d_pool.get(), ctx->d_pool_ctl.get(), ctx->d_fail_from.get(), ctx->d_failed_total.get()};
                ctx->info_slices++;
                if (fuse && kta::alive_fuse_possible(pl, ctx->P) && pl.segment_wgs <= ctx->max_rows) {
                    ctx->info_fused++;
                    ctx->handed_records = true;
                    const uint32_t row_len = kta::scan_row_len(ctx->P, false);
                    const kta::ScanColumns sc = scan_columns(rb, at);
                    const kta::AliveFuse fz{sc.partition, sc.ts_ms, sc.hdr, sc.rec0, ctx->P, ctx->d_partials.get(), row_len};
                    KTA_HIP(ctx, kta::launch_alive_partitioned(sl, take, base_seq + at, st, pl, ws, report ? ctx->d_alive_stats.get() : nullptr,
                                                               ctx->s_compute, &fz));
                    KTA_HIP(ctx, kta::launch_fold_partials(ctx->d_partials.get(), pl.segment_wgs, ctx->P, ctx->d_vec.get(), row_len, ctx->d_avec.get(),
                                                           ctx->s_compute));
                } else {
                    if (fuse) {      // (a slice the fused pass does not take: its records go through the scan)
                        ctx->info_scanned++;
                        int rc = scan_and_fold(at, take, false);
                        if (rc != KTA_OK) return rc;
                    }
                    KTA_HIP(ctx, kta::launch_alive_partitioned(sl, take, base_seq + at, st, pl, ws,
                                                               report ? ctx->d_alive_stats.get() : nullptr, ctx->s_compute));
                }
                if (sl.seq)   // the batch's seq column did not ascend: the pair did nothing, this runs instead
                    KTA_HIP(ctx, kta::launch_alive_update(sl, take, base_seq + at, ctx->d_table.get(), 0, 2, nullptr,
                                                          ctx->d_alive_running.get(), ctx->s_compute,
                                                          kta::alive_order_flag(ws, (int)pl.bucket_log2), written_list(ctx)));
                at += take;
            }
            if (report) {
                KTA_HIP(ctx, hipMemcpyAsync(ctx->h_alive_stats.get(), ctx->d_alive_stats.get(), 2 * sizeof(uint64_t),
                                            hipMemcpyDeviceToHost, ctx->s_compute));
                KTA_HIP(ctx, hipEventRecord(ctx->ev_alive_stats.get(), ctx->s_compute));
                ctx->alive_stats_pending = true;
            }
        } else {
            const int v = part_kind ? 2 : ctx->alive_variant;
            KTA_HIP(ctx, kta::launch_alive_update(ac, n, base_seq, ctx->d_table.get(), ctx->alive_wgs > 2048 ? 0 : ctx->alive_wgs,
                                                  v, ctx->d_hash_scratch.get(), ctx->d_alive_running.get(), ctx->s_compute, nullptr,
                                                  written_list(ctx)));
        }
        if (ctx->timing) KTA_HIP(ctx, hipEventRecord(b, ctx->s_compute));
    }
    if ((which & 1) && ctx->sketch) {   // after the scan or the fused pass, which it leaves as they are
        int rc = run_key_sketch(ctx, c, rb, n);
        if (rc != KTA_OK) return rc;
    }
    if ((which & 1) && ctx->tso) {      // likewise; it reads partition and ts_ms only
        int rc = run_ts_order(ctx, rb, n);
        if (rc != KTA_OK) return rc;
    }
    if ((which & 1) && ctx->seg) {      // likewise; partition, ts_ms and the lengths in the tiles' own forms, no keys
        int rc = run_segments(ctx, rb, n);
        if (rc != KTA_OK) return rc;
    }
    if ((which & 1) && ctx->hot) {      // a pass of its own, likewise
        int rc = run_hot_keys(ctx, c, rb, n);
        if (rc != KTA_OK) return rc;
    }
    if ((which & 1) && ctx->part) {     // likewise
        int rc = run_partitioner(ctx, c, rb, n);
        if (rc != KTA_OK) return rc;
    }
    if ((which & 1) && ctx->sizeq) {    // likewise; partition and the lengths in the tiles' own forms, no keys
        int rc = run_size_quantiles(ctx, rb, n);
        if (rc != KTA_OK) return rc;
    }
    return KTA_OK;
}

// The scratch batch of the filter, large enough for `cap` records: partition, key_len, val_len, ts_ms, and key_off / seq
// where the context reads them (released, after the compute stream has drained, before it is allocated again).
int grow_filter_scratch(kta_ctx *ctx, uint64_t cap, bool keys, bool seq)
{
    kta_batch &b = ctx->filter_scratch;
    if (b.capacity >= cap && (!keys || b.key_off) && (!seq || b.seq)) return KTA_OK;
    KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));
    cap = (cap + KTA_TILE_RECORDS - 1) / KTA_TILE_RECORDS * KTA_TILE_RECORDS;
    memset(&b, 0, sizeof b);
    const size_t c4 = pad16(cap * 4), c8 = pad16(cap * 8);
    KTA_HIP(ctx, ctx->d_filter_scratch.alloc(3 * c4 + c8 + (keys ? c4 : 0) + (seq ? c8 : 0)));
    uint8_t *base = ctx->d_filter_scratch.get();
    b.ts_ms = reinterpret_cast<int64_t *>(base), base += c8;
    if (seq) b.seq = reinterpret_cast<uint64_t *>(base), base += c8;
    b.partition = reinterpret_cast<int32_t *>(base), base += c4;
    b.key_len = reinterpret_cast<int32_t *>(base), base += c4;
    b.val_len = reinterpret_cast<int32_t *>(base), base += c4;
    if (keys) b.key_off = reinterpret_cast<uint32_t *>(base);
    b.capacity = cap;
    return KTA_OK;
}

// A filtered context's batch (kta_set_filter): slice by slice, the passing records are compacted in order into the scratch
// batch — count per tile, prefix, ONE host wait for the slice's total, because the plans of the passes behind need the
// record count on the host, then the scatter — and the handlers get the scratch batch.  A slice nothing of which passes
// launches nothing more; a slice all of which passes is handed on as it is, as a view at its record offset, unscattered.
int run_filtered_batch(kta_ctx *ctx, const kta_batch *c, uint64_t n, uint64_t base_seq, int which)
{
    if (!c->partition || !c->key_len || !c->val_len || !c->ts_ms) return fail(ctx, KTA_ERR_INVALID, "metric columns missing (the filter reads them)");
    if (!aligned16(c->partition) || !aligned16(c->key_len) || !aligned16(c->val_len) || !aligned16(c->ts_ms))
        return fail(ctx, KTA_ERR_INVALID, "device columns must be 16-byte aligned");
    const bool keys = c->key_off && c->key_bytes;
    const bool seq = ctx->alive && ctx->alive_table;
    kta_internal_columns rb{};
    int rc = kta_internal_resolve(ctx, c, &rb);
    if (rc != KTA_OK) return rc;
    if (rb.rows && rb.rec0 + n > rb.rows) return fail(ctx, KTA_ERR_INVALID, "the batch ends behind its allocation");
    if (!ctx->d_filter_count) {
        KTA_HIP(ctx, ctx->d_filter_count.alloc(kta::kFilterCountWords));
        KTA_HIP(ctx, ctx->d_filter_offset.alloc(kta::kFilterMaxTiles + 1));
        KTA_HIP(ctx, ctx->h_filter_total.alloc(1));
        KTA_HIP(ctx, hipHostGetDevicePointer(reinterpret_cast<void **>(&ctx->d_filter_total), ctx->h_filter_total.get(), 0));
    }
    // a hand-built tile-compact batch (its own tile_hdr) has no views: only its first slice can be handed on as it is
    const bool viewable = !rb.hdr || rb.rows != 0;
    ctx->handed_records = true;
    for (uint64_t at = 0; at < n;) {
        const uint64_t take = n - at < ctx->filter_slice ? n - at : ctx->filter_slice;
        rc = grow_filter_scratch(ctx, take, keys, seq);
        if (rc != KTA_OK) return rc;
        const kta_internal_columns r = columns_at(rb, at);
        const kta_batch &sb = ctx->filter_scratch;
        const kta::FilterSource src{r.partition, r.key_len, r.val_len, r.ts_ms, r.hdr, r.sum, r.hdr ? r.rec0 : 0,
                                    keys ? c->key_off + at : nullptr, c->seq ? c->seq + at : nullptr, base_seq + at};
        const kta::FilterDest dst{sb.partition, sb.key_len, sb.val_len, sb.ts_ms, keys ? sb.key_off : nullptr, seq ? sb.seq : nullptr, sb.capacity};
        const kta::FilterWorkspace ws{ctx->d_filter_count.get(), ctx->d_filter_offset.get(), ctx->d_filter_stats.get(), ctx->d_filter_total};
        KTA_HIP(ctx, kta::launch_filter_count(src, take, ctx->filter_spec, ctx->d_filter_bitmap.get(), ws, ctx->s_compute));
        KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));   // the one wait of the slice: the prefix kernel wrote the total to pinned memory
        const uint64_t m = *static_cast<volatile uint64_t *>(ctx->h_filter_total.get());
        if (m > take || m > sb.capacity) return fail(ctx, KTA_ERR_CAPACITY, "filter: a slice's total exceeds the scratch batch");
        ctx->filter_seen += take, ctx->filter_passed += m, ctx->filter_slices++;
        const bool hand_on = m == take && (viewable || at == 0);
        if (m && !hand_on)
            KTA_HIP(ctx, kta::launch_filter_scatter(src, take, ctx->filter_spec, ctx->d_filter_bitmap.get(), ws, dst, ctx->s_compute));
        if (hand_on) {
            kta_batch v = *c;
            if (at) {
                v.partition += at, v.key_len += at, v.val_len += at, v.ts_ms += at;
                if (v.key_off) v.key_off += at;
                if (v.seq) v.seq += at;
                v.capacity = c->capacity > at ? c->capacity - at : 0;
            }
            rc = run_handlers(ctx, &v, take, base_seq + at, which);
        } else if (m) {
            kta_batch v = sb;
            v.key_bytes = keys ? c->key_bytes : nullptr;
            v.key_bytes_capacity = c->key_bytes_capacity;
            rc = run_handlers(ctx, &v, m, base_seq + at, which);
        }
        if (rc != KTA_OK) return rc;
        at += take;
    }
    return KTA_OK;
}

// Every submission path ends here: the staging ring (kta_batch_submit, and through it kta_handle_message, kta_flush and
// kta_replay_messages), kta_submit_device[_ex] and, through that, the Kafka decode.  Without a filter nothing is added.
int run_device_batch(kta_ctx *ctx, const kta_batch *c, uint64_t n, uint64_t base_seq, int which)
{
    if (n == 0) return KTA_OK;
    if (!ctx->filter) return run_handlers(ctx, c, n, base_seq, which);
    return run_filtered_batch(ctx, c, n, base_seq, which);
}

// ---- result sections ------------------------------------------------------------------------------------------------
// The shape of a section's vector (kta_internal.h has the table): its length and the SUM prefix of its merge rule, as
// functions of the section's own shape.  The context's table below and the context-free kta_merge_* both read them here.
struct Shape {
    size_t words, sum_words;
    bool max_signed;
};
Shape all_sum(size_t words) { return Shape{words, words, false}; }
Shape counters_shape(uint32_t P)
{
    const size_t nc = (size_t)P * KTA_NCOUNTERS;
    return Shape{nc + KTA_NGLOBALS, nc + KTA_NSUM_GLOBALS, true};
}
Shape analytics_shape(uint32_t P) { return Shape{kta::analytics_len(P), kta::kAnalyticsHist, true}; }
Shape timeline_shape(uint32_t n_buckets) { return all_sum(kta::timeline_len(n_buckets)); }
Shape key_sketch_shape(uint32_t P) { return Shape{(size_t)P * kta::kSketchRegs, 0, false}; }
Shape hot_keys_shape() { return all_sum(KTA_HOT_VECTOR_WORDS); }
Shape ts_order_shape(uint32_t P) { return Shape{kta::ts_order_len(P), 2 * (size_t)P + 64, true}; }
Shape partitioner_shape(uint32_t P, uint32_t Q) { return all_sum(kta::partitioner_len(P, Q)); }
Shape size_quantiles_shape(uint32_t P) { return all_sum(kta::size_quantiles_len(P)); }
// (the MAX suffix is S, M, overhead and the two zero words: equal on every rank, so the maximum is each rank's own; the
// kept vector has the segments' shape)
Shape segments_shape(uint32_t P, uint32_t M)
{
    const size_t words = kta::segments_len(P, M);
    return Shape{words, words - kta::kSegGlobals + kta::kSegGlobalS, false};
}
Shape record_batches_shape(uint32_t P) { return Shape{kta::rb_len(P), kta::rb_sum_words(P), false}; }
Shape payload_shape(uint32_t P) { return all_sum(kta::payload_len(P)); }
Shape header_names_shape() { return all_sum(kta::kHnWords); }
Shape value_bytes_shape(uint32_t P) { return all_sum(kta::value_bytes_len(P)); }
Shape compress_whatif_shape(uint32_t P) { return all_sum(kta::compress_whatif_len(P)); }
Shape compaction_shape(uint32_t P) { return all_sum(kta::compaction_len(P)); }   // (live only: nothing reduces it)

// what include/kta_hip.h says of these shapes in macros, for the callers that size their buffers by them
static_assert(kta::kAnalyticsHist == 2 * KTA_HIST_BUCKETS, "the two histograms: kta_kernels.h and kta_hip.h");
static_assert(kta::kTimelineCols == KTA_TIMELINE_COLS && kta::kSketchRegs == KTA_SKETCH_REGISTERS, "kta_kernels.h and kta_hip.h");
static_assert(KTA_HOT_VECTOR_WORDS == 2 * 1024 * 23, "the hot-key vector: kta_internal.h's table and kta_hip.h");
static_assert(KTA_TS_ORDER_HIST + 1 == 64, "the 64 words between a timestamp-order vector's sums and its maxima: hist[63] and timed");
static_assert(kta::kSizePartitionWords == KTA_SIZE_QUANTITIES * KTA_SIZE_BINS && kta::kSizeGlobals == KTA_SIZE_GLOBALS, "kta_size_bins.h and kta_hip.h");
static_assert(kta::kCompactionWords == KTA_COMPACTION_WORDS && kta::kCompactionGlobals == KTA_COMPACTION_GLOBALS, "kta_compaction.h and kta_hip.h");
static_assert(kta::kRetWords == KTA_RETENTION_WORDS, "the what-if's row is said twice: kta_segments.h and kta_hip.h");
static_assert(kta::kCdWords == KTA_COMPACT_DELETE_WORDS, "the what-if's row is said twice: kta_compact_delete.h and kta_hip.h");
static_assert(kta::kRbPartitionWords == KTA_RB_PARTITION_WORDS && kta::kRbCodecs == KTA_RB_CODECS && kta::kRbCodecWords == KTA_RB_CODEC_WORDS &&
                  kta::kRbHistBins == KTA_RB_HIST_BINS && kta::kRbMaxWords == KTA_RB_MAX_WORDS && kta::kRbSketchRegs == KTA_RB_SKETCH_REGISTERS,
              "kta_record_batches.h and kta_hip.h");
static_assert(KTA_RB_WORDS(7) == 20 * 7 + 1524 && KTA_RB_SUM_WORDS(7) == 16 * 7 + 500 &&
                  kta::kRbPartitionWords * 7 + kta::kRbCodecTable == KTA_RB_SUM_WORDS(7) &&
                  KTA_RB_SUM_WORDS(7) + kta::kRbMaxWords * 7 + kta::kRbSketchRegs == KTA_RB_WORDS(7),
              "the record-batch vector's length: kta_record_batches.h and kta_hip.h");
static_assert(kta::kPlPartitionWords == KTA_PAYLOAD_PARTITION_WORDS && kta::kPlHistBins == KTA_PAYLOAD_HIST_BINS && kta::kPlRows == KTA_PAYLOAD_ROWS &&
                  kta::kPlCells == KTA_PAYLOAD_CELLS && kta::kPlCellWords == KTA_PAYLOAD_CELL_WORDS && kta::kPlClasses == KTA_PAYLOAD_CLASSES,
              "kta_payload.h and kta_hip.h");
static_assert(KTA_PAYLOAD_WORDS(7) == 24 * 7 + 16 + 2 * 1024 * 34 && kta::kPlPartitionWords * 7 + kta::kPlHistBins + kta::kPlTableWords == KTA_PAYLOAD_WORDS(7),
              "the payload vector's length: kta_payload.h and kta_hip.h");
static_assert(KTA_HEADER_NAMES_WORDS == kta::kHnWords && KTA_HEADER_NAMES_GLOBALS == kta::kHnGlobals && KTA_HEADER_NAMES_CELL_WORDS == kta::kHnCellWords &&
                  KTA_HEADER_NAMES_SLOTS == kta::kHnSlots && KTA_HEADER_NAME_BYTES == kta::kHnExemplarBytes && KTA_HEADER_NAMES_ROWS == kta::kPlRows &&
                  KTA_HEADER_NAMES_CELLS == kta::kPlCells,
              "kta_header_names.h and kta_hip.h");
static_assert(sizeof(kta_header_name) == sizeof(kta::HnSlot) && offsetof(kta_header_name, hash) == offsetof(kta::HnSlot, hash) &&
                  offsetof(kta_header_name, name_len) == offsetof(kta::HnSlot, name_len) && offsetof(kta_header_name, state) == offsetof(kta::HnSlot, state) &&
                  offsetof(kta_header_name, bytes) == offsetof(kta::HnSlot, bytes) && KTA_HEADER_NAME_PUBLISHED == kta::kHnPublished,
              "a slot of the name table: kta_header_names.h and kta_hip.h");
static_assert(KTA_VALUE_BYTES_PARTITION_WORDS == kta::kVbPartitionWords && KTA_VALUE_BYTES_BINS == kta::kVbBins && KTA_VALUE_BYTES_WORDS(7) == 264 * 7,
              "kta_value_bytes.h and kta_hip.h");
static_assert(KTA_VALUE_BYTES_NONE == kta::kVbNone && KTA_VALUE_BYTES_TEXT == kta::kVbText && KTA_VALUE_BYTES_DENSE == kta::kVbDense &&
                  KTA_VALUE_BYTES_BINARY == kta::kVbBinary,
              "the classes: kta_value_bytes.h and kta_hip.h");
static_assert(KTA_COMPRESS_WHATIF_PARTITION_WORDS == kta::kCwPartitionWords && KTA_COMPRESS_WHATIF_CODECS == kta::kCwCodecs &&
                  KTA_COMPRESS_WHATIF_CODEC_WORDS == kta::kCwCodecWords && KTA_COMPRESS_WHATIF_WORDS(7) == 8 * 7 + 20 &&
                  kta::kCwBatchHeader == KTA_KAFKA_BATCH_HEADER,
              "kta_lz4_model.h, kta_hip.h and kta_kafka.h");

// One section of the result as the host layer handles it: a row of sections_of, which states every section once.  live
// and out point at the context's owners, allocated or not.
struct Section {
    bool on;
    DeviceBuf<uint64_t> *live;   // the live accumulator; null: it is no u64 vector (the key sketch's u32 registers)
    DeviceBuf<uint64_t> *out;    // the snapshot kta_finish_device takes; null: the section is live only
    Shape shape;                 // as the section is configured now
    bool zero_is_empty;          // reset_state clears the live vector with zeros; false: by a line of its own there
    const char *noun;            // check_words: "the <noun> has N u64 words, not M"
    const char *off;             // kta_last_error of every entry point of the section while it is off
};

void sections_of(kta_ctx *ctx, Section s[KTA_SEC_KINDS])
{
    const uint32_t P = ctx->P;
    s[KTA_RV_COUNTERS] = Section{true, &ctx->d_vec, &ctx->d_vec_out, counters_shape(P), false, "counter vector", ""};
    s[KTA_RV_ANALYTICS] = Section{ctx->analytics, &ctx->d_avec, &ctx->d_avec_out, analytics_shape(P), false, "analytics vector",
                                  "context was created without KTA_FLAG_ANALYTICS"};
    s[KTA_RV_TIMELINE] = Section{ctx->timeline, &ctx->d_tvec, &ctx->d_tvec_out, timeline_shape(ctx->tl.n_buckets), true, "timeline",
                                 "the context has no timeline (kta_set_timeline)"};
    s[KTA_RV_KEY_SKETCH] = Section{ctx->sketch, nullptr, &ctx->d_sketch_out, key_sketch_shape(P), false, "key sketch",
                                   "context was created without KTA_FLAG_KEY_SKETCH"};
    s[KTA_RV_HOT_KEYS] = Section{ctx->hot, &ctx->d_hot, &ctx->d_hot_out, hot_keys_shape(), true, "hot-key vector",
                                 "context was created without KTA_FLAG_HOT_KEYS"};
    s[KTA_RV_TS_ORDER] = Section{ctx->tso, &ctx->d_tso, &ctx->d_tso_out, ts_order_shape(P), true, "timestamp-order vector",
                                 "context was created without KTA_FLAG_TS_ORDER"};
    s[KTA_RV_PARTITIONER] = Section{ctx->part, &ctx->d_part, &ctx->d_part_out, partitioner_shape(P, ctx->part_q), true, "partitioner vector",
                                    "context was created without KTA_FLAG_PARTITIONER"};
    s[KTA_RV_SIZE_QUANTILES] = Section{ctx->sizeq, &ctx->d_sizeq, &ctx->d_sizeq_out, size_quantiles_shape(P), true, "size-percentile vector",
                                       "context was created without KTA_FLAG_SIZE_QUANTILES"};
    s[KTA_RV_SEGMENTS] = Section{ctx->seg, &ctx->d_seg, &ctx->d_seg_out, segments_shape(P, ctx->seg_M), false, "segment vector",
                                 "the context has no segments (kta_set_segments)"};
    s[KTA_RV_RECORD_BATCHES] = Section{ctx->rb, &ctx->d_rb, &ctx->d_rb_out, record_batches_shape(P), true, "record-batch vector",
                                       "context was created without KTA_FLAG_RECORD_BATCHES"};
    s[KTA_RV_PAYLOAD] = Section{ctx->pl, &ctx->d_pl, &ctx->d_pl_out, payload_shape(P), true, "payload vector", "context was created without KTA_FLAG_PAYLOAD"};
    s[KTA_RV_HEADER_NAMES] = Section{ctx->hn, &ctx->d_hn, &ctx->d_hn_out, header_names_shape(), true, "header-name vector",
                                      "context was created without KTA_FLAG_HEADER_NAMES"};
    s[KTA_RV_VALUE_BYTES] = Section{ctx->vb, &ctx->d_vb, &ctx->d_vb_out, value_bytes_shape(P), true, "value-byte vector",
                                     "context was created without KTA_FLAG_VALUE_BYTES"};
    s[KTA_RV_COMPRESS_WHATIF] = Section{ctx->cw, &ctx->d_cw, &ctx->d_cw_out, compress_whatif_shape(P), true, "compression what-if vector",
                                         "context was created without KTA_FLAG_COMPRESS_WHATIF"};
    s[KTA_SEC_COMPACTION] = Section{ctx->comp, &ctx->d_comp, nullptr, compaction_shape(P), true, "compaction vector",
                                    "context was created without KTA_FLAG_COMPACTION"};
    s[KTA_SEC_KEPT] = Section{ctx->cd, &ctx->d_kept, nullptr, segments_shape(P, ctx->seg_M), false, "kept vector",
                              "the context has no compact,delete what-if (kta_set_compact_delete)"};
}

Section section(kta_ctx *ctx, int kind)
{
    Section s[KTA_SEC_KINDS];
    sections_of(ctx, s);
    return s[kind];
}

// the refusal of an entry point whose section is off
int section_off(kta_ctx *ctx, int kind) { return fail(ctx, KTA_ERR_INVALID, section(ctx, kind).off); }

// `words` u64 words of a vector on the device (a live accumulator or a snapshot), once the compute stream has reached them.
int read_words(kta_ctx *ctx, const uint64_t *d_src, uint64_t *host, size_t words)
{
    KTA_HIP(ctx, hipMemcpyAsync(host, d_src, words * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->s_compute));
    KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));
    return KTA_OK;
}

// the caller's buffer for the vector called `name` has its length
int check_words(kta_ctx *ctx, const char *name, size_t words, size_t n_u64)
{
    if (n_u64 == words) return KTA_OK;
    return fail(ctx, KTA_ERR_INVALID, std::string("the ") + name + " has " + std::to_string(words) + " u64 words, not " + std::to_string(n_u64));
}

// How every read-back of a section into the caller's u64[n_u64] begins: the arguments, the section on, the buffer's
// length, the device.  *s: the section's row.
int begin_read(kta_ctx *ctx, int kind, const uint64_t *out, size_t n_u64, Section *s)
{
    if (!ctx || !out) return KTA_ERR_INVALID;
    *s = section(ctx, kind);
    if (!s->on) return fail(ctx, KTA_ERR_INVALID, s->off);
    int rc = check_words(ctx, s->noun, s->shape.words, n_u64);
    if (rc != KTA_OK) return rc;
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    return KTA_OK;
}

// kta_get_<section>: the live vector, staged messages flushed first
int get_section(kta_ctx *ctx, int kind, uint64_t *out, size_t n_u64)
{
    Section s;
    int rc = begin_read(ctx, kind, out, n_u64, &s);
    if (rc != KTA_OK) return rc;
    rc = kta_flush(ctx);
    if (rc != KTA_OK) return rc;
    return read_words(ctx, s.live->get(), out, n_u64);
}

// kta_exchange_<section>: the snapshot as it is (nothing is flushed)
int exchange_section(kta_ctx *ctx, int kind, uint64_t *out, size_t n_u64)
{
    Section s;
    int rc = begin_read(ctx, kind, out, n_u64, &s);
    return rc != KTA_OK ? rc : read_words(ctx, s.out->get(), out, n_u64);
}

// kta_<section>_result_vector (snapshot) and kta_<section>_vector (the live vector): the device pointer and the length
int section_vector(kta_ctx *ctx, int kind, bool snapshot, void **device_ptr, size_t *n_u64)
{
    if (!ctx || !device_ptr || !n_u64) return KTA_ERR_INVALID;
    const Section s = section(ctx, kind);
    if (!s.on) return fail(ctx, KTA_ERR_INVALID, s.off);
    *device_ptr = (snapshot ? s.out : s.live)->get();
    *n_u64 = s.shape.words;
    return KTA_OK;
}

// kta_merge_<section>: acc = acc (+) other by the rule of the result vectors, SUM over [0, sum_words), MAX over the rest
int merge_section(uint64_t *acc, const uint64_t *other, bool bounds_ok, const Shape &sh)
{
    if (!acc || !other || !bounds_ok) return KTA_ERR_INVALID;
    for (size_t i = 0; i < sh.sum_words; i++) acc[i] += other[i];
    for (size_t i = sh.sum_words; i < sh.words; i++)
        if (sh.max_signed ? (int64_t)other[i] > (int64_t)acc[i] : other[i] > acc[i]) acc[i] = other[i];
    return KTA_OK;
}

// Both vectors of a section cleared, and (alloc_section) allocated at `words` first: what kta_create does for every
// section that is on and a configuration call for the one it gives another shape.  Each owner is released before either
// is allocated again, after the compute stream has drained.
int clear_section(kta_ctx *ctx, const Section &s, size_t words)
{
    if (s.live) KTA_HIP(ctx, hipMemsetAsync(s.live->get(), 0, words * sizeof(uint64_t), ctx->s_compute));
    if (s.out) KTA_HIP(ctx, hipMemsetAsync(s.out->get(), 0, words * sizeof(uint64_t), ctx->s_compute));
    return KTA_OK;
}
int alloc_section(kta_ctx *ctx, const Section &s, size_t words)
{
    KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));
    if (s.live) s.live->reset();
    if (s.out) s.out->reset();
    const std::string what = std::string("allocating the ") + s.noun;   // (a failure names the section, as its own lines once did)
    if (s.live) KTA_HIP_AS(ctx, s.live->alloc(words), what.c_str());
    if (s.out) KTA_HIP_AS(ctx, s.out->alloc(words), (what + "'s snapshot").c_str());
    return clear_section(ctx, s, words);
}

// A live vector of the segments' shape (the segment vector, the kept vector) as its configuration call, kta_reset and,
// for the kept vector, kta_compaction_replay(ctx, 1) leave it: zero but for the configuration globals; its pass's four
// work counters zero.
int clear_segment_vector(kta_ctx *ctx, uint64_t *vec, uint64_t *stats)
{
    const uint64_t cfg[3] = {ctx->seg_S, ctx->seg_M, ctx->seg_overhead};
    KTA_HIP(ctx, hipMemsetAsync(vec, 0, kta::segments_len(ctx->P, ctx->seg_M) * sizeof(uint64_t), ctx->s_compute));
    KTA_HIP(ctx, hipMemcpyAsync(vec + kta::segments_globals_at(ctx->P, ctx->seg_M) + kta::kSegGlobalS, cfg, sizeof cfg, hipMemcpyHostToDevice,
                                ctx->s_compute));
    KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));   // (cfg is this frame's)
    KTA_HIP(ctx, hipMemsetAsync(stats, 0, 4 * sizeof(uint64_t), ctx->s_compute));
    return KTA_OK;
}
int clear_segments(kta_ctx *ctx)
{
    ctx->seg_launches = ctx->seg_chunks = ctx->seg_last_chunk = 0;
    return clear_segment_vector(ctx, ctx->d_seg.get(), ctx->d_seg_stats.get());
}
int clear_kept(kta_ctx *ctx)
{
    ctx->cd_launches = ctx->cd_chunks = 0;
    return clear_segment_vector(ctx, ctx->d_kept.get(), ctx->d_cd_stats.get());
}

int reset_state(kta_ctx *ctx)
{
    // Every live vector whose empty value is zeros; the configurations (timeline, Q, segments, forced slices) stay.  Below:
    // the vectors with another empty value, and what a section keeps beside its vector.
    Section sec[KTA_SEC_KINDS];
    sections_of(ctx, sec);
    for (const Section &s : sec)
        if (s.on && s.live && s.zero_is_empty)
            KTA_HIP(ctx, hipMemsetAsync(s.live->get(), 0, s.shape.words * sizeof(uint64_t), ctx->s_compute));
    KTA_HIP(ctx, kta::launch_init_vector(ctx->d_vec.get(), ctx->P, ctx->d_avec.get(), ctx->s_compute));   // counters, analytics: the extrema
    if (ctx->sketch) {                  // (the live registers are u32)
        KTA_HIP(ctx, hipMemsetAsync(ctx->d_sketch.get(), 0, (size_t)ctx->P * kta::kSketchRegs * sizeof(uint32_t), ctx->s_compute));
        KTA_HIP(ctx, hipMemsetAsync(ctx->d_sketch_stats.get(), 0, 3 * sizeof(uint64_t), ctx->s_compute));
        ctx->sketch_launches = 0;
    }
    if (ctx->hot) {
        KTA_HIP(ctx, hipMemsetAsync(ctx->d_hot_slots.get(), 0, kHotSlotsN * sizeof(kta_hot_exemplar), ctx->s_compute));
        KTA_HIP(ctx, hipMemsetAsync(ctx->d_hot_stats.get(), 0, 4 * sizeof(uint64_t), ctx->s_compute));
        ctx->hot_launches = ctx->hot_workgroups = 0;
    }
    if (ctx->tso) {                     // (hi: every byte 0xFF is -1, none)
        KTA_HIP(ctx, hipMemsetAsync(ctx->d_tso_hi.get(), 0xFF, (size_t)ctx->P * sizeof(int64_t), ctx->s_compute));
        KTA_HIP(ctx, hipMemsetAsync(ctx->d_tso_stats.get(), 0, 3 * sizeof(uint64_t), ctx->s_compute));
        ctx->tso_launches = ctx->tso_chunks = ctx->tso_last_chunk = 0;
    }
    if (ctx->seg) {                     // (its globals hold the configuration)
        int rc = clear_segments(ctx);
        if (rc != KTA_OK) return rc;
    }
    if (ctx->hn) {                      // (the name table is cleared with the vector; the work counters as well)
        KTA_HIP(ctx, hipMemsetAsync(ctx->d_hn_names.get(), 0, kta::kHnSlots * sizeof(kta_header_name), ctx->s_compute));
        KTA_HIP(ctx, hipMemsetAsync(ctx->d_hn_info.get(), 0, 4 * sizeof(uint64_t), ctx->s_compute));
    }
    if (ctx->vb) KTA_HIP(ctx, hipMemsetAsync(ctx->d_vb_info.get(), 0, 4 * sizeof(uint64_t), ctx->s_compute));   // (the work counters)
    if (ctx->part) {
        KTA_HIP(ctx, hipMemsetAsync(ctx->d_part_stats.get(), 0, 3 * sizeof(uint64_t), ctx->s_compute));
        ctx->part_launches = ctx->part_workgroups = 0;
    }
    if (ctx->comp) {
        KTA_HIP(ctx, hipMemsetAsync(ctx->d_comp_stats.get(), 0, 3 * sizeof(uint64_t), ctx->s_compute));
        ctx->comp_launches = ctx->comp_workgroups = 0;
        ctx->comp_replay = false;
        ctx->comp_saved_seq = 0;
    }
    if (ctx->cd) {                      // (the switch stays; likewise)
        int rc = clear_kept(ctx);
        if (rc != KTA_OK) return rc;
    }
    if (ctx->sizeq) {
        KTA_HIP(ctx, hipMemsetAsync(ctx->d_sizeq_stats.get(), 0, kSizeqStatWords * sizeof(uint64_t), ctx->s_compute));
        ctx->sizeq_last_workgroups = 0;
    }
    ctx->handed_records = false;
    if (ctx->d_filter_stats) KTA_HIP(ctx, hipMemsetAsync(ctx->d_filter_stats.get(), 0, 3 * sizeof(uint64_t), ctx->s_compute));
    ctx->filter_seen = ctx->filter_passed = ctx->filter_slices = 0;   // (the filter itself stays)
    if (ctx->alive) {
        if (ctx->alive_table) {
            KTA_HIP(ctx, hipMemsetAsync(ctx->d_table.get(), 0, kta::kAliveSlots * sizeof(uint64_t), ctx->s_compute));
            KTA_HIP(ctx, hipMemsetAsync(ctx->d_written_n.get(), 0, sizeof(unsigned long long), ctx->s_compute));
            ctx->written_valid = true;
        } else {
            KTA_HIP(ctx, hipMemsetAsync(ctx->d_bitmap.get(), 0, (size_t)(kta::kAliveSlots / 8), ctx->s_compute));
        }
        KTA_HIP(ctx, hipMemsetAsync(ctx->d_alive_running.get(), 0, sizeof(int64_t), ctx->s_compute));
        ctx->running_valid = true;
        // a new topic: what the old one's batches taught about backing off does not carry over (a word still on its way
        // lands in h_alive_stats before any later copy — same stream — and is never looked at)
        if (ctx->d_failed_total) KTA_HIP(ctx, hipMemsetAsync(ctx->d_failed_total.get(), 0, sizeof(uint64_t), ctx->s_compute));
        ctx->alive_stats_pending = false;
        ctx->alive_backoff = 0;
        ctx->info_slices = ctx->info_fused = ctx->info_scanned = ctx->info_failed_buckets = 0;
    }
    ctx->next_seq = 0;
    ctx->msg_count = ctx->msg_flushes = ctx->msg_flush_ns = ctx->msg_wait_ns = 0;
    return KTA_OK;
}

} // namespace

void kta_internal_result_vectors(kta_ctx *ctx, ResultVector rv[KTA_RV_KINDS])
{
    Section sec[KTA_SEC_KINDS];
    sections_of(ctx, sec);
    for (int k = 0; k < KTA_RV_KINDS; k++) {
        const Section &s = sec[k];
        rv[k] = s.on ? ResultVector{s.out->get(), s.shape.words, s.shape.sum_words, s.shape.max_signed} : ResultVector{nullptr, 0, 0, false};
    }
}

// The batches of bytes[0, len) that count on the host, as kta_kafka_index_host finds them, compressed ones inflated:
// batch(descriptor, record bytes, their length) for each.  A stream that does not inflate is a failed batch: skipped.
template <class OnBatch>
static int host_batches_described(const uint8_t *bytes, uint64_t len, int32_t partition, OnBatch batch)
{
    kta_kafka_index_stats st;
    int rc = kta_kafka_index_host(bytes, len, partition, 0, 0, (len + 127) & ~63ull, nullptr, 0, &st);
    if (rc != KTA_OK && rc != KTA_ERR_CAPACITY) return rc;
    std::vector<kta_kafka_batch_desc> descs(st.n_batches);
    rc = kta_kafka_index_host(bytes, len, partition, 0, 0, (len + 127) & ~63ull, descs.data(), descs.size(), &st);
    if (rc != KTA_OK) return rc;
    std::vector<uint8_t> inflated;
    for (const kta_kafka_batch_desc &d : descs) {
        if (d.status != 0 || d.n_records <= 0 || d.byte_off > len || len - d.byte_off < d.batch_bytes || d.batch_bytes < KTA_KAFKA_BATCH_HEADER) continue;
        const uint8_t *src = bytes + d.byte_off + KTA_KAFKA_BATCH_HEADER;
        const uint64_t n = d.batch_bytes - KTA_KAFKA_BATCH_HEADER;
        if (!(d.flags & (KTA_KB_SNAPPY | KTA_KB_LZ4 | KTA_KB_GZIP | KTA_KB_ZSTD))) {
            batch(d, src, n);
            continue;
        }
        const uint64_t cap = d.payload_end > d.payload_off ? d.payload_end - d.payload_off : 0;   // the index's bound (exact for gzip and Snappy)
        inflated.assign(cap + 64, 0);
        const int64_t got = (d.flags & KTA_KB_SNAPPY) ? kta_snappy_inflate_host(src, n, inflated.data(), cap)
                            : (d.flags & KTA_KB_LZ4)  ? kta_lz4_inflate_host(src, n, inflated.data(), cap)
                            : (d.flags & KTA_KB_GZIP) ? kta_gzip_inflate_host(src, n, inflated.data(), cap)
                                                      : kta_zstd_inflate_host(src, n, inflated.data(), cap);
        if (got < 0) continue;
        batch(d, inflated.data(), (uint64_t)got);
    }
    return KTA_OK;
}

// The same for a caller that needs the records alone: batch(record bytes, their length, n_records).
template <class OnBatch>
static int host_batches(const uint8_t *bytes, uint64_t len, int32_t partition, OnBatch batch)
{
    return host_batches_described(bytes, len, partition,
                                  [&](const kta_kafka_batch_desc &d, const uint8_t *recs, uint64_t n) { batch(recs, n, (uint64_t)d.n_records); });
}

extern "C" {

int kta_abi_version(void) { return KTA_ABI_VERSION; }

int kta_device_count(int *n)
{
    if (!n) return KTA_ERR_INVALID;
    *n = 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return KTA_ERR_NO_DEVICE;
    *n = ndev;
    return KTA_OK;
}

const char *kta_last_error(const kta_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int kta_create(const kta_config *cfg, kta_ctx **out)
{
    if (!cfg || !out) return fail(nullptr, KTA_ERR_INVALID, "kta_create: null argument");
    *out = nullptr;
    // What a flag asks of the configuration, in the order it is checked: the partitions it admits and, where the pass
    // reads the alive-key state, count_alive_keys (checked first).  Refusals carry the flag's name and the reason.
    struct FlagBound {
        uint32_t flag;
        const char *name;
        int (*most)(void);
        const char *reason;
        const char *needs_alive;   // null: the flag works without count_alive_keys
    };
    // (before the general bound, which is the same number today for some: the message names the pass that sets this one)
    static const FlagBound kBeforeGeneral[] = {
        {KTA_FLAG_PARTITIONER, "KTA_FLAG_PARTITIONER", kta_partitioner_max_partitions, "the pass keeps its counters in LDS", nullptr},
        {KTA_FLAG_SIZE_QUANTILES, "KTA_FLAG_SIZE_QUANTILES", kta_size_quantiles_max_partitions, "every slice of 28 partitions streams the batch again",
         nullptr},
        {KTA_FLAG_COMPACTION, "KTA_FLAG_COMPACTION", kta_compaction_max_partitions, "the pass keeps 32 B per partition in LDS",
         "the pass reads the last-writer table"},
    };
    static const FlagBound kAfterGeneral[] = {
        {KTA_FLAG_ANALYTICS, "KTA_FLAG_ANALYTICS", kta_analytics_max_partitions, "the analytics scan keeps 4 extrema per partition in LDS", nullptr},
        {KTA_FLAG_KEY_SKETCH, "KTA_FLAG_KEY_SKETCH", [] { return KTA_SKETCH_MAX_PARTITIONS; }, "a u64 snapshot of 4096 registers per partition", nullptr},
        {KTA_FLAG_TS_ORDER, "KTA_FLAG_TS_ORDER", kta_ts_order_max_partitions, "a wave of the apply kernel keeps its running maxima in LDS", nullptr},
    };
    // the refusal of a flag's row, "" when the configuration meets it
    auto refusal = [cfg](const FlagBound &b) -> std::string {
        if (!(cfg->flags & b.flag)) return "";
        if (b.needs_alive && !cfg->count_alive_keys) return std::string(b.name) + " needs count_alive_keys (" + b.needs_alive + ")";
        if (cfg->n_partitions <= b.most()) return "";
        return std::string(b.name) + " admits at most " + std::to_string(b.most()) + " partitions (" + b.reason + ")";
    };
    for (const FlagBound &b : kBeforeGeneral)
        if (const std::string why = refusal(b); !why.empty()) return fail(nullptr, KTA_ERR_INVALID, why);
    if (cfg->n_partitions <= 0 || cfg->n_partitions > 4096) return fail(nullptr, KTA_ERR_INVALID, "n_partitions must be in [1, 4096]");
    for (const FlagBound &b : kAfterGeneral)
        if (const std::string why = refusal(b); !why.empty()) return fail(nullptr, KTA_ERR_INVALID, why);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, KTA_ERR_NO_DEVICE, "no HIP device visible (libkta_hip has no CPU fallback)");
    if (cfg->device_id < 0 || cfg->device_id >= ndev)
        return fail(nullptr, KTA_ERR_INVALID, "device_id out of range");
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, cfg->device_id);
    if (e != hipSuccess) return hip_fail(nullptr, e, "hipGetDeviceProperties");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, KTA_ERR_NO_DEVICE,
                    std::string("device is ") + prop.gcnArchName + ", libkta_hip is built for gfx950 only");
    e = hipSetDevice(cfg->device_id);
    if (e != hipSuccess) return hip_fail(nullptr, e, "hipSetDevice");

    kta_ctx *ctx = new (std::nothrow) kta_ctx();
    if (!ctx) return fail(nullptr, KTA_ERR_NOMEM, "out of host memory");
    ctx->device = cfg->device_id;
    ctx->P = (uint32_t)cfg->n_partitions;
    ctx->alive = cfg->count_alive_keys != 0;
    ctx->analytics = (cfg->flags & KTA_FLAG_ANALYTICS) != 0;
    ctx->sketch = (cfg->flags & KTA_FLAG_KEY_SKETCH) != 0;
    ctx->hot = (cfg->flags & KTA_FLAG_HOT_KEYS) != 0;
    ctx->tso = (cfg->flags & KTA_FLAG_TS_ORDER) != 0;
    ctx->part = (cfg->flags & KTA_FLAG_PARTITIONER) != 0;
    ctx->part_q = ctx->part ? ctx->P : 0u;
    ctx->comp = (cfg->flags & KTA_FLAG_COMPACTION) != 0;
    ctx->sizeq = (cfg->flags & KTA_FLAG_SIZE_QUANTILES) != 0;
    ctx->rb = (cfg->flags & KTA_FLAG_RECORD_BATCHES) != 0;
    ctx->pl = (cfg->flags & KTA_FLAG_PAYLOAD) != 0;
    ctx->hn = (cfg->flags & KTA_FLAG_HEADER_NAMES) != 0;
    ctx->vb = (cfg->flags & KTA_FLAG_VALUE_BYTES) != 0;
    ctx->cw = (cfg->flags & KTA_FLAG_COMPRESS_WHATIF) != 0;
    {
        const char *bv = getenv("KTA_VALUE_BYTES_VARIANT");   // A/B switch of tools/bench_value_bytes.py: 1 every byte its own LDS add, 2 all pairs
        ctx->vb_variant = bv && (bv[0] == '1' || bv[0] == '2') && !bv[1] ? bv[0] - '0' : 0;
    }
    {
        const char *qv = getenv("KTA_SIZEQ_VARIANT");   // A/B switch of tools/bench_size_quantiles.py: 1 a launch per slice, 9 loads only
        ctx->sizeq_variant = qv && (qv[0] == '1' || qv[0] == '9') && !qv[1] ? qv[0] - '0' : 0;
    }
    {
        const char *nf = getenv("KTA_NO_FUSE");      // A/B switch of bench.py and the tests: the two handlers as two passes
        ctx->fuse_handlers = !(nf && nf[0] == '1');
    }
    ctx->stage_seq = (cfg->flags & KTA_FLAG_SEQ_COLUMN) != 0;
    ctx->alive_table = ctx->alive && (cfg->flags & (KTA_FLAG_SEQ_COLUMN | KTA_FLAG_ALIVE_TABLE | KTA_FLAG_COMPACTION)) != 0;
    ctx->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    ctx->batch_capacity = cfg->batch_capacity ? cfg->batch_capacity : (1ull << 22);
    ctx->key_bytes_capacity = cfg->key_bytes_capacity ? cfg->key_bytes_capacity : 64ull * ctx->batch_capacity;
    int rc = KTA_OK;
    auto bail = [&](int code) {
        g_create_error = ctx->err;
        kta_destroy(ctx);
        return code;
    };
    if (ctx->key_bytes_capacity >= (1ull << 32)) {
        ctx->err = "key_bytes_capacity must be < 4 GiB (key_off is a batch-local u32)";
        return bail(KTA_ERR_INVALID);
    }
#define KTA_TRY(call)                                                     \
    do {                                                                  \
        hipError_t e__ = (call);                                          \
        if (e__ != hipSuccess) return bail(hip_fail(ctx, e__, #call));    \
    } while (0)
    KTA_TRY(hipStreamCreateWithFlags(ctx->s_own.put(), hipStreamNonBlocking));
    ctx->s_compute = ctx->s_own.get();
    KTA_TRY(hipStreamCreateWithFlags(ctx->s_copy.put(), hipStreamNonBlocking));
    KTA_TRY(hipEventCreateWithFlags(ctx->ev_copied.put(), hipEventDisableTiming));
    // every section that is on: its live vector and its snapshot, both zero (kta_reset below gives the live ones their empty values)
    Section sec[KTA_SEC_KINDS];
    sections_of(ctx, sec);
    for (const Section &s : sec) {
        if (s.on) rc = alloc_section(ctx, s, s.shape.words);
        if (rc != KTA_OK) return bail(rc);
    }
    // what a section keeps beside the two
    ctx->max_rows = (uint32_t)ctx->cu_count * 8u;
    KTA_TRY(ctx->d_partials.alloc((size_t)ctx->max_rows * kta::scan_row_len(ctx->P, ctx->analytics)));
    if (ctx->sketch) {
        KTA_TRY(ctx->d_sketch.alloc((size_t)ctx->P * kta::kSketchRegs));
        KTA_TRY(ctx->d_sketch_floor.alloc(kta::kSketchFloorBytes));
        KTA_TRY(ctx->d_sketch_stats.alloc(3));
    }
    if (ctx->hot) {
        KTA_TRY(ctx->d_hot_slots.alloc(kHotSlotsN));
        KTA_TRY(ctx->d_hot_ctl.alloc(2 * kHotSlotsN + kHotSlotsN / 32));
        KTA_TRY(ctx->d_hot_stats.alloc(4));
    }
    if (ctx->tso) {
        KTA_TRY(ctx->d_tso_hi.alloc(ctx->P));
        KTA_TRY(ctx->d_tso_ws.alloc(kta::kTsOrderWorkspaceWords));
        KTA_TRY(ctx->d_tso_stats.alloc(3));
    }
    if (ctx->part) KTA_TRY(ctx->d_part_stats.alloc(3));
    if (ctx->hn) {
        KTA_TRY(ctx->d_hn_names.alloc(kta::kHnSlots));
        KTA_TRY(ctx->d_hn_info.alloc(4));
    }
    if (ctx->vb) KTA_TRY(ctx->d_vb_info.alloc(4));
    if (ctx->comp) KTA_TRY(ctx->d_comp_stats.alloc(3));
    if (ctx->sizeq) KTA_TRY(ctx->d_sizeq_stats.alloc(kSizeqStatWords));
    if (ctx->alive) {
        if (ctx->alive_table) {
            KTA_TRY(ctx->d_table.alloc(kta::kAliveSlots));
            KTA_TRY(ctx->d_written.alloc((size_t)1 << 28));   // 1 GiB of slot numbers; beyond that the exchange sweeps the table
            KTA_TRY(ctx->d_written_n.alloc(1));
        } else {
            KTA_TRY(ctx->d_bitmap.alloc((size_t)(kta::kAliveSlots / 32)));
        }
        KTA_TRY(ctx->d_alive_running.alloc(1));
    }
#undef KTA_TRY
    rc = reset_state(ctx);
    if (rc != KTA_OK) return bail(rc);
    // staging ring is allocated lazily (first kta_batch_acquire / kta_handle_message)
    ctx->stages.resize(cfg->n_staging > 0 ? (size_t)cfg->n_staging : 2);
    *out = ctx;
    return KTA_OK;
}

void kta_destroy(kta_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->s_compute) (void)hipStreamSynchronize(ctx->s_compute);
    if (ctx->s_copy) (void)hipStreamSynchronize(ctx->s_copy.get());
    if (ctx->ext_state && ctx->ext_free) ctx->ext_free(ctx->ext_state);
    if (ctx->comm_state && ctx->comm_free) ctx->comm_free(ctx->comm_state);
    // the context's memory and events, the streams last (the member order of kta_ctx)
    delete ctx;
}

int kta_reset(kta_ctx *ctx)
{
    if (!ctx) return KTA_ERR_INVALID;
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    ctx->fill_n = ctx->fill_kb = 0;
    return reset_state(ctx);
}

static int ensure_stage(kta_ctx *ctx, Stage &st)
{
    if (st.host_slab) return KTA_OK;
    const uint64_t cap = ctx->batch_capacity, kcap = ctx->key_bytes_capacity;
    const bool keys = ctx->alive || ctx->sketch || ctx->hot || ctx->part, seq = ctx->alive && ctx->stage_seq;
    size_t off = 0, o_part, o_klen, o_vlen, o_ts, o_koff = 0, o_seq = 0, o_kb = 0;
    o_part = off; off += pad16(cap * 4);
    o_klen = off; off += pad16(cap * 4);
    o_vlen = off; off += pad16(cap * 4);
    o_ts = off; off += pad16(cap * 8);
    st.metric_bytes = off;
    if (keys) {
        o_koff = off; off += pad16(cap * 4);
        if (seq) { o_seq = off; off += pad16(cap * 8); }
        o_kb = off; off += pad16(kcap + 16);
    }
    st.key_bytes_off = o_kb;
    st.slab_bytes = off;
    KTA_HIP(ctx, st.host_slab.alloc(off));
    KTA_HIP(ctx, st.dev_slab.alloc(off));
    auto point = [&](kta_batch &b, uint8_t *base) {
        memset(&b, 0, sizeof b);
        b.capacity = cap;
        b.key_bytes_capacity = keys ? kcap : 0;
        b.partition = reinterpret_cast<int32_t *>(base + o_part);
        b.key_len = reinterpret_cast<int32_t *>(base + o_klen);
        b.val_len = reinterpret_cast<int32_t *>(base + o_vlen);
        b.ts_ms = reinterpret_cast<int64_t *>(base + o_ts);
        if (keys) {
            b.key_off = reinterpret_cast<uint32_t *>(base + o_koff);
            b.key_bytes = base + o_kb;
            if (seq) b.seq = reinterpret_cast<uint64_t *>(base + o_seq);
        }
    };
    point(st.host, st.host_slab.get());
    point(st.dev, st.dev_slab.get());
    KTA_HIP(ctx, hipEventCreateWithFlags(st.done.put(), hipEventDisableTiming));
    return KTA_OK;
}

int kta_batch_acquire(kta_ctx *ctx, kta_batch *out)
{
    if (!ctx || !out) return KTA_ERR_INVALID;
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    Stage &st = ctx->stages[ctx->cur];
    int rc = ensure_stage(ctx, st);
    if (rc != KTA_OK) return rc;
    if (st.busy) { // the ring wrapped: wait until the kernels that read this stage are done
        KTA_HIP(ctx, hipEventSynchronize(st.done.get()));
        st.busy = false;
    }
    *out = st.host;
    ctx->acquired = true;
    return KTA_OK;
}

int kta_batch_submit(kta_ctx *ctx, uint64_t n, uint64_t n_key_bytes, uint64_t base_seq)
{
    if (!ctx) return KTA_ERR_INVALID;
    if (!ctx->acquired) return fail(ctx, KTA_ERR_INVALID, "kta_batch_submit without kta_batch_acquire");
    const bool keys = ctx->alive || ctx->sketch || ctx->hot || ctx->part;
    if (n > ctx->batch_capacity || (keys && n_key_bytes > ctx->key_bytes_capacity))
        return fail(ctx, KTA_ERR_CAPACITY, "batch larger than the staging capacity");
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    Stage &st = ctx->stages[ctx->cur];
    ctx->acquired = false;
    if (n == 0) return KTA_OK;
    hipStream_t cs = ctx->s_copy.get();
    const size_t used = keys ? st.key_bytes_off + n_key_bytes : st.metric_bytes;
    if (n * 2 >= ctx->batch_capacity) {
        // a batch that is at least half full (every batch of a stream but its last): ONE copy of the slab's
        // used prefix — the unused tails of the columns travel along, the launches do not multiply
        KTA_HIP(ctx, hipMemcpyAsync(st.dev_slab.get(), st.host_slab.get(), used, hipMemcpyHostToDevice, cs));
    } else {
        KTA_HIP(ctx, hipMemcpyAsync(st.dev.partition, st.host.partition, n * 4, hipMemcpyHostToDevice, cs));
        KTA_HIP(ctx, hipMemcpyAsync(st.dev.key_len, st.host.key_len, n * 4, hipMemcpyHostToDevice, cs));
        KTA_HIP(ctx, hipMemcpyAsync(st.dev.val_len, st.host.val_len, n * 4, hipMemcpyHostToDevice, cs));
        KTA_HIP(ctx, hipMemcpyAsync(st.dev.ts_ms, st.host.ts_ms, n * 8, hipMemcpyHostToDevice, cs));
        if (keys) {
            KTA_HIP(ctx, hipMemcpyAsync(st.dev.key_off, st.host.key_off, n * 4, hipMemcpyHostToDevice, cs));
            if (n_key_bytes)
                KTA_HIP(ctx, hipMemcpyAsync(st.dev.key_bytes, st.host.key_bytes, n_key_bytes, hipMemcpyHostToDevice, cs));
            if (st.host.seq)   // KTA_FLAG_SEQ_COLUMN: the producer wrote every record's global sequence number
                KTA_HIP(ctx, hipMemcpyAsync(st.dev.seq, st.host.seq, n * 8, hipMemcpyHostToDevice, cs));
        }
    }
    KTA_HIP(ctx, hipEventRecord(ctx->ev_copied.get(), cs));
    KTA_HIP(ctx, hipStreamWaitEvent(ctx->s_compute, ctx->ev_copied.get(), 0));
    int rc = run_device_batch(ctx, &st.dev, n, base_seq, 3);
    if (rc != KTA_OK) return rc;
    KTA_HIP(ctx, hipEventRecord(st.done.get(), ctx->s_compute));
    st.busy = true;
    ctx->cur = (ctx->cur + 1) % (int)ctx->stages.size();
    return KTA_OK;
}

int kta_flush(kta_ctx *ctx)
{
    if (!ctx) return KTA_ERR_INVALID;
    if (ctx->fill_n == 0) return KTA_OK;
    const uint64_t n = ctx->fill_n, kb = ctx->fill_kb;
    const uint64_t base = ctx->next_seq;
    ctx->fill_n = ctx->fill_kb = 0;
    ctx->next_seq += n;
    return kta_batch_submit(ctx, n, kb, base);
}

int kta_seek_seq(kta_ctx *ctx, uint64_t next_seq)
{
    if (!ctx) return KTA_ERR_INVALID;
    int rc = kta_flush(ctx);   // records already staged keep the numbers they were given
    if (rc != KTA_OK) return rc;
    ctx->next_seq = next_seq;
    return KTA_OK;
}

int kta_handle_message(kta_ctx *ctx, int32_t partition, int64_t ts_ms, const void *key, int64_t key_len,
                       int64_t val_len)
{
    if (!ctx) return KTA_ERR_INVALID;
    if (key_len > INT32_MAX || val_len > INT32_MAX)
        return fail(ctx, KTA_ERR_INVALID, "key/value length above i32 range");
    if (!key) key_len = -1; // m.key() is None iff librdkafka's key pointer is null
    const bool keys = ctx->alive || ctx->sketch || ctx->hot || ctx->part;
    const uint64_t kb = (keys && key_len > 0) ? (uint64_t)key_len : 0;
    if (kb > ctx->key_bytes_capacity) return fail(ctx, KTA_ERR_CAPACITY, "key larger than key_bytes_capacity");
    if (ctx->fill_n > 0 && (ctx->fill_n == ctx->batch_capacity || ctx->fill_kb + kb > ctx->key_bytes_capacity)) {
        const uint64_t t0 = now_ns();
        int rc = kta_flush(ctx);
        ctx->msg_flush_ns += now_ns() - t0;
        ctx->msg_flushes++;
        if (rc != KTA_OK) return rc;
    }
    if (ctx->fill_n == 0) {
        kta_batch tmp;
        const uint64_t t0 = now_ns();
        int rc = kta_batch_acquire(ctx, &tmp);
        ctx->msg_wait_ns += now_ns() - t0;
        if (rc != KTA_OK) return rc;
    }
    kta_batch &h = ctx->stages[ctx->cur].host;
    const uint64_t i = ctx->fill_n;
    ctx->handed_records = true;
    h.partition[i] = partition;
    h.ts_ms[i] = ts_ms;
    h.key_len[i] = key_len < 0 ? -1 : (int32_t)key_len;
    h.val_len[i] = val_len < 0 ? -1 : (int32_t)val_len;
    if (keys) {
        if (h.seq) h.seq[i] = ctx->next_seq + i;
        h.key_off[i] = (uint32_t)ctx->fill_kb;
        if (kb) {
            memcpy(h.key_bytes + ctx->fill_kb, key, kb);
            ctx->fill_kb += kb;
        }
    }
    ctx->fill_n = i + 1;
    ctx->msg_count++;
    return KTA_OK;
}

int kta_replay_messages(kta_ctx *ctx, const kta_batch *c, uint64_t n)
{
    if (!ctx || !c) return KTA_ERR_INVALID;
    if (!c->partition || !c->key_len || !c->val_len || !c->ts_ms) return fail(ctx, KTA_ERR_INVALID, "metric columns missing");
    if (ctx->alive && (!c->key_off || !c->key_bytes)) return fail(ctx, KTA_ERR_INVALID, "key columns missing (count_alive_keys)");
    if (ctx->sketch && (!c->key_off || !c->key_bytes)) return fail(ctx, KTA_ERR_INVALID, "key columns missing (KTA_FLAG_KEY_SKETCH)");
    if (ctx->hot && (!c->key_off || !c->key_bytes)) return fail(ctx, KTA_ERR_INVALID, "key columns missing (KTA_FLAG_HOT_KEYS)");
    if (ctx->part && (!c->key_off || !c->key_bytes)) return fail(ctx, KTA_ERR_INVALID, "key columns missing (KTA_FLAG_PARTITIONER)");
    // through a pointer the compiler cannot see through: the loop pays the call a foreign caller pays per message
    static int (*volatile entry)(kta_ctx *, int32_t, int64_t, const void *, int64_t, int64_t) = kta_handle_message;
    static const uint8_t no_bytes[1] = {0};
    for (uint64_t i = 0; i < n; i++) {
        const int32_t kl = c->key_len[i];
        const void *key = kl < 0 ? nullptr : (c->key_bytes && c->key_off ? (const void *)(c->key_bytes + c->key_off[i]) : (const void *)no_bytes);
        int rc = entry(ctx, c->partition[i], c->ts_ms[i], key, kl, c->val_len[i]);
        if (rc != KTA_OK) return rc;
    }
    return KTA_OK;
}

int kta_handle_message_stats(kta_ctx *ctx, uint64_t out[4])
{
    if (!ctx || !out) return KTA_ERR_INVALID;
    out[0] = ctx->msg_count, out[1] = ctx->msg_flushes, out[2] = ctx->msg_flush_ns, out[3] = ctx->msg_wait_ns;
    return KTA_OK;
}

int kta_submit_device_ex(kta_ctx *ctx, const kta_batch *cols, uint64_t n, uint64_t base_seq, int which)
{
    if (!ctx || !cols) return KTA_ERR_INVALID;
    if (which < 1 || which > 3) return fail(ctx, KTA_ERR_INVALID, "which must be 1, 2 or 3");
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    return run_device_batch(ctx, cols, n, base_seq, which);
}

int kta_submit_device(kta_ctx *ctx, const kta_batch *cols, uint64_t n, uint64_t base_seq)
{
    return kta_submit_device_ex(ctx, cols, n, base_seq, 3);
}

int kta_device_batch_alloc(kta_ctx *ctx, uint64_t capacity, uint64_t key_bytes_capacity, int with_seq,
                           kta_batch *out)
{
    if (!ctx || !out) return KTA_ERR_INVALID;
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    if (key_bytes_capacity >= (1ull << 32))
        return fail(ctx, KTA_ERR_INVALID, "key_bytes_capacity must be < 4 GiB per batch");
    int rc = alloc_device_batch(ctx, capacity, key_bytes_capacity, key_bytes_capacity > 0, with_seq != 0, out);
    if (rc != KTA_OK) free_device_batch(out);
    else ctx->compact_batches.push_back(*out);
    return rc;
}

int kta_device_batch_free(kta_ctx *ctx, kta_batch *cols)
{
    if (!ctx || !cols) return KTA_ERR_INVALID;
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));
    uint64_t rec0 = 0;
    const kta_batch *e = find_allocation(ctx, cols->partition, &kta_batch::partition, &rec0);
    if (e && e->partition == cols->partition) ctx->compact_batches.erase(ctx->compact_batches.begin() + (e - ctx->compact_batches.data()));
    free_device_batch(cols);
    return KTA_OK;
}

int kta_batch_from_raw(kta_ctx *ctx, const kta_batch *h, uint64_t n, const kta_batch *d)
{
    if (!ctx || !h || !d) return KTA_ERR_INVALID;
    if (n == 0) return KTA_OK;
    if (!h->partition || !h->key_len || !h->val_len || !h->ts_ms || !d->partition || !d->key_len || !d->val_len || !d->ts_ms)
        return fail(ctx, KTA_ERR_INVALID, "metric columns missing");
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    kta_internal_columns r{};
    int rc = kta_internal_resolve(ctx, d, &r);
    if (rc != KTA_OK) return rc;
    KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));
    if (!r.hdr || !r.keyless) {   // (a keyless tile-compact allocation takes the lengths tile by tile, below)
        KTA_HIP(ctx, hipMemcpy(d->key_len, h->key_len, n * 4, hipMemcpyHostToDevice));
        KTA_HIP(ctx, hipMemcpy(d->val_len, h->val_len, n * 4, hipMemcpyHostToDevice));
    }
    if (!r.hdr) {
        KTA_HIP(ctx, hipMemcpy(d->partition, h->partition, n * 4, hipMemcpyHostToDevice));
        KTA_HIP(ctx, hipMemcpy(d->ts_ms, h->ts_ms, n * 8, hipMemcpyHostToDevice));
        return KTA_OK;
    }
    if (r.rec0 % KTA_TILE_RECORDS)
        return fail(ctx, KTA_ERR_INVALID, "a tile-compact batch is written from a tile boundary");
    // the tiles' images, then one copy per column and one of the headers
    const uint64_t nt = tiles_of(n);
    std::vector<int32_t> part(nt * KTA_TILE_RECORDS, 0);
    std::vector<int64_t> ts(nt * KTA_TILE_RECORDS, 0);
    std::vector<kta_tile_hdr> hdr(nt);
    std::vector<kta_tile_sum> sum(nt);
    std::vector<uint32_t> mark(nt, 0u), size(2 * nt, 0u);
    std::vector<int32_t> klen, vlen;
    if (r.keyless) {
        klen.assign(nt * KTA_TILE_RECORDS, 0);
        vlen.assign(nt * KTA_TILE_RECORDS, 0);
    }
    for (uint64_t T = 0; T < nt; T++) {
        const uint64_t a = T * KTA_TILE_RECORDS, m = n - a < KTA_TILE_RECORDS ? n - a : KTA_TILE_RECORDS;
        hdr[T] = kta::tile_pack_host(h->partition + a, h->ts_ms + a, h->key_len + a, h->val_len + a, m, r.keyless, part.data() + a, ts.data() + a,
                                     r.keyless ? klen.data() + a : nullptr, r.keyless ? vlen.data() + a : nullptr, &sum[T]);
        // (the plane rides in the ts image that is uploaded whole anyway)
        if (r.mark) mark[T] = kta::tile_plane_host(hdr[T], h->partition + a, h->key_len + a, h->val_len + a, m, ts.data() + a, &size[2 * T]);
    }
    if (r.keyless) {
        KTA_HIP(ctx, hipMemcpy(r.key_len + r.rec0, klen.data(), klen.size() * 4, hipMemcpyHostToDevice));
        KTA_HIP(ctx, hipMemcpy(r.val_len + r.rec0, vlen.data(), vlen.size() * 4, hipMemcpyHostToDevice));
    }
    KTA_HIP(ctx, hipMemcpy(r.partition + r.rec0, part.data(), part.size() * 4, hipMemcpyHostToDevice));
    KTA_HIP(ctx, hipMemcpy(r.ts_ms + r.rec0, ts.data(), ts.size() * 8, hipMemcpyHostToDevice));
    KTA_HIP(ctx, hipMemcpy(r.hdr + r.rec0 / KTA_TILE_RECORDS, hdr.data(), nt * sizeof(kta_tile_hdr), hipMemcpyHostToDevice));
    if (r.sum) KTA_HIP(ctx, hipMemcpy(r.sum + r.rec0 / KTA_TILE_RECORDS, sum.data(), nt * sizeof(kta_tile_sum), hipMemcpyHostToDevice));
    // (the size extrema before the marks that vouch for them)
    if (r.mark) KTA_HIP(ctx, hipMemcpy(r.size + 2 * (r.rec0 / KTA_TILE_RECORDS), size.data(), 2 * nt * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (r.mark) KTA_HIP(ctx, hipMemcpy(r.mark + r.rec0 / KTA_TILE_RECORDS, mark.data(), nt * sizeof(uint32_t), hipMemcpyHostToDevice));
    return KTA_OK;
}

int kta_batch_tile_summaries(kta_ctx *ctx, const kta_batch *d, uint64_t n, kta_tile_sum *out)
{
    if (!ctx || !d || !out) return KTA_ERR_INVALID;
    if (!d->partition) return fail(ctx, KTA_ERR_INVALID, "metric columns missing");
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    kta_internal_columns r{};
    int rc = kta_internal_resolve(ctx, d, &r);
    if (rc != KTA_OK) return rc;
    if (!r.sum) return fail(ctx, KTA_ERR_INVALID, "the batch has no tile summaries (not an allocation of kta_device_batch_alloc)");
    if (r.rec0 % KTA_TILE_RECORDS) return fail(ctx, KTA_ERR_INVALID, "tile summaries are read from a tile boundary");
    if (r.rec0 + n > r.rows) return fail(ctx, KTA_ERR_CAPACITY, "more records than the allocation holds");
    if (n == 0) return KTA_OK;
    KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));
    KTA_HIP(ctx, hipMemcpy(out, r.sum + r.rec0 / KTA_TILE_RECORDS, tiles_of(n) * sizeof(kta_tile_sum), hipMemcpyDeviceToHost));
    return KTA_OK;
}

int kta_batch_tile_planes(kta_ctx *ctx, const kta_batch *d, uint64_t n, uint32_t *out)
{
    if (!ctx || !d || !out) return KTA_ERR_INVALID;
    if (!d->partition) return fail(ctx, KTA_ERR_INVALID, "metric columns missing");
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    kta_internal_columns r{};
    int rc = kta_internal_resolve(ctx, d, &r);
    if (rc != KTA_OK) return rc;
    if (!r.mark) return fail(ctx, KTA_ERR_INVALID, "the batch has no plane marks (not an allocation of kta_device_batch_alloc)");
    if (r.rec0 % KTA_TILE_RECORDS) return fail(ctx, KTA_ERR_INVALID, "plane marks are read from a tile boundary");
    if (r.rec0 + n > r.rows) return fail(ctx, KTA_ERR_CAPACITY, "more records than the allocation holds");
    if (n == 0) return KTA_OK;
    KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));
    KTA_HIP(ctx, hipMemcpy(out, r.mark + r.rec0 / KTA_TILE_RECORDS, tiles_of(n) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return KTA_OK;
}

int kta_batch_to_raw(kta_ctx *ctx, const kta_batch *d, uint64_t n, const kta_batch *h)
{
    if (!ctx || !h || !d) return KTA_ERR_INVALID;
    if (n == 0) return KTA_OK;
    if (!h->partition || !h->key_len || !h->val_len || !h->ts_ms || !d->partition || !d->key_len || !d->val_len || !d->ts_ms)
        return fail(ctx, KTA_ERR_INVALID, "metric columns missing");
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    kta_internal_columns r{};
    int rc = kta_internal_resolve(ctx, d, &r);
    if (rc != KTA_OK) return rc;
    KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));
    KTA_HIP(ctx, hipMemcpy(h->key_len, d->key_len, n * 4, hipMemcpyDeviceToHost));   // (the records of u16 tiles: replaced below)
    KTA_HIP(ctx, hipMemcpy(h->val_len, d->val_len, n * 4, hipMemcpyDeviceToHost));
    if (!r.hdr) {
        KTA_HIP(ctx, hipMemcpy(h->partition, d->partition, n * 4, hipMemcpyDeviceToHost));
        KTA_HIP(ctx, hipMemcpy(h->ts_ms, d->ts_ms, n * 8, hipMemcpyDeviceToHost));
        return KTA_OK;
    }
    const uint64_t t0 = r.rec0 / KTA_TILE_RECORDS, nt = tiles_of(r.rec0 + n) - t0;
    std::vector<int32_t> part(nt * KTA_TILE_RECORDS);
    std::vector<int64_t> ts(nt * KTA_TILE_RECORDS);
    std::vector<kta_tile_hdr> hdr(nt);
    KTA_HIP(ctx, hipMemcpy(part.data(), r.partition + t0 * KTA_TILE_RECORDS, part.size() * 4, hipMemcpyDeviceToHost));
    KTA_HIP(ctx, hipMemcpy(ts.data(), r.ts_ms + t0 * KTA_TILE_RECORDS, ts.size() * 8, hipMemcpyDeviceToHost));
    KTA_HIP(ctx, hipMemcpy(hdr.data(), r.hdr + t0, nt * sizeof(kta_tile_hdr), hipMemcpyDeviceToHost));
    // tile by tile, the batch's records of it; a u16 tile (keyless allocations) brings its groups
    std::vector<int32_t> g16(KTA_TILE_RECORDS);
    for (uint64_t T = 0; T < nt; T++) {
        const uint64_t a = (t0 + T) * KTA_TILE_RECORDS;   // the tile's first record in the allocation
        const uint64_t j0 = a < r.rec0 ? r.rec0 - a : 0, j1 = r.rec0 + n - a < KTA_TILE_RECORDS ? r.rec0 + n - a : KTA_TILE_RECORDS;
        const bool u16 = hdr[T].lens == KTA_TILE_LENS_U16;
        if (u16) KTA_HIP(ctx, hipMemcpy(g16.data(), r.key_len + a, g16.size() * 4, hipMemcpyDeviceToHost));
        const uint64_t o = a + j0 - r.rec0;               // the batch's record
        kta::tile_unpack_host(hdr[T], part.data() + T * KTA_TILE_RECORDS, ts.data() + T * KTA_TILE_RECORDS, u16 ? g16.data() : nullptr, nullptr,
                              j0, j1, h->partition + o, h->ts_ms + o, h->key_len + o, h->val_len + o);
    }
    return KTA_OK;
}


int kta_copy_to_device(kta_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (!ctx) return KTA_ERR_INVALID;
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));
    KTA_HIP(ctx, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return KTA_OK;
}

int kta_copy_to_host(kta_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (!ctx) return KTA_ERR_INVALID;
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));
    KTA_HIP(ctx, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return KTA_OK;
}

int kta_set_compute_stream(kta_ctx *ctx, void *hip_stream)
{
    if (!ctx) return KTA_ERR_INVALID;
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));   // nothing of ours may still be in flight on the old stream
    ctx->s_compute = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->s_own.get();
    return KTA_OK;
}

int kta_sync(kta_ctx *ctx)
{
    if (!ctx) return KTA_ERR_INVALID;
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    KTA_HIP(ctx, hipStreamSynchronize(ctx->s_copy.get()));
    KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));
    return KTA_OK;
}

int kta_finish_device(kta_ctx *ctx)
{
    if (!ctx) return KTA_ERR_INVALID;
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    int rc = kta_flush(ctx);
    if (rc != KTA_OK) return rc;
    // every snapshot is a copy of its live vector ...
    Section sec[KTA_SEC_KINDS];
    sections_of(ctx, sec);
    for (const Section &s : sec)
        if (s.on && s.live && s.out)
            KTA_HIP(ctx, hipMemcpyAsync(s.out->get(), s.live->get(), s.shape.words * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->s_compute));
    // ... but the key sketch's: its live registers are u32, and a kernel widens them
    if (ctx->sketch)
        KTA_HIP(ctx, kta::launch_key_sketch_widen(ctx->d_sketch.get(), sec[KTA_RV_KEY_SKETCH].shape.words, ctx->d_sketch_out.get(), ctx->s_compute));
    if (ctx->alive) {
        uint64_t *dst = ctx->d_vec_out.get() + (size_t)ctx->P * KTA_NCOUNTERS + KTA_G_ALIVE_KEYS;
        if (ctx->running_valid)  // exact running count (every update so far ran a counting kernel): no table scan
            KTA_HIP(ctx, hipMemcpyAsync(dst, ctx->d_alive_running.get(), sizeof(uint64_t), hipMemcpyDeviceToDevice,
                                        ctx->s_compute));
        else if (ctx->alive_table)
            KTA_HIP(ctx, kta::launch_alive_count(ctx->d_table.get(), kta::kAliveSlots, dst, ctx->s_compute));
        else {
            KTA_HIP(ctx, hipMemsetAsync(dst, 0, sizeof(uint64_t), ctx->s_compute));
            KTA_HIP(ctx, kta::launch_bitmap_count(ctx->d_bitmap.get(), dst, ctx->s_compute));
        }
    }
    return KTA_OK;
}

int kta_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64)
{
    return section_vector(ctx, KTA_RV_COUNTERS, true, device_ptr, n_u64);
}

int kta_decode_vector(const uint64_t *vec, uint32_t P, int count_alive_keys, kta_result *out,
                      uint64_t *counters_out)
{
    if (!vec || !out || P == 0) return KTA_ERR_INVALID;
    const uint64_t *g = vec + (size_t)P * KTA_NCOUNTERS;
    memset(out, 0, sizeof(*out));
    out->n_partitions = P;
    uint64_t total = 0, live = 0, size = 0;
    for (uint32_t p = 0; p < P; p++) {
        const uint64_t *c = vec + (size_t)p * KTA_NCOUNTERS;
        total += c[KTA_C_TOTAL];
        live += c[KTA_C_ALIVE];
        size += c[KTA_C_KEY_SIZE_SUM] + c[KTA_C_VALUE_SIZE_SUM];
    }
    if (counters_out) memcpy(counters_out, vec, (size_t)P * KTA_NCOUNTERS * sizeof(uint64_t));
    out->any_records = total > 0;
    out->any_live = live > 0;
    out->count_alive_keys = count_alive_keys ? 1u : 0u;
    // metric.rs:210: timestamp / 1000 truncates toward zero, and is monotone, so applying it
    // to the extrema of the millisecond values equals the extrema of the per-record seconds.
    out->min_ts_sec = out->any_records ? (int64_t)~g[KTA_G_NOT_MIN_TS_MS] / 1000 : 0;
    out->max_ts_sec = out->any_records ? (int64_t)g[KTA_G_MAX_TS_MS] / 1000 : 0;
    out->smallest_message = out->any_live ? ~g[KTA_G_NOT_SMALLEST] : UINT64_MAX; // metric.rs:42
    out->largest_message = g[KTA_G_LARGEST];
    out->overall_count = total;
    out->overall_size = size;
    out->alive_keys = count_alive_keys ? g[KTA_G_ALIVE_KEYS] : 0;
    out->bad_partition_records = g[KTA_G_BAD_PARTITION];
    // metric.rs:210 / kafka.rs:104: NaiveDateTime::from_timestamp panics outside chrono's range, on the first
    // such record; one such record among those counted puts an extremum outside the range
    if (out->any_records && (out->min_ts_sec < KTA_CHRONO_MIN_SEC || out->max_ts_sec > KTA_CHRONO_MAX_SEC))
        return KTA_ERR_TIMESTAMP_RANGE;
    return out->bad_partition_records ? KTA_ERR_BAD_PARTITION : KTA_OK;
}

int kta_merge_vectors(uint64_t *acc, const uint64_t *other, uint32_t P)
{
    return merge_section(acc, other, P != 0, counters_shape(P));
}

int kta_finish(kta_ctx *ctx, kta_result *out, uint64_t *counters_out)
{
    if (!ctx || !out) return KTA_ERR_INVALID;
    int rc = kta_finish_device(ctx);
    if (rc != KTA_OK) return rc;
    return kta_exchange_result(ctx, out, counters_out);
}

int kta_exchange_result(kta_ctx *ctx, kta_result *out, uint64_t *counters_out)
{
    if (!ctx || !out) return KTA_ERR_INVALID;
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    const Section s = section(ctx, KTA_RV_COUNTERS);
    std::vector<uint64_t> host(s.shape.words);
    int rc = read_words(ctx, s.out->get(), host.data(), host.size());
    if (rc != KTA_OK) return rc;
    rc = kta_decode_vector(host.data(), ctx->P, ctx->alive ? 1 : 0, out, counters_out);
    if (rc == KTA_ERR_BAD_PARTITION) {
        char buf[128];
        snprintf(buf, sizeof buf, "%llu record(s) had a partition id outside [0, %u)",
                 (unsigned long long)out->bad_partition_records, ctx->P);
        ctx->err = buf;
    } else if (rc == KTA_ERR_TIMESTAMP_RANGE) {
        ctx->err = "a record's timestamp / 1000 is outside chrono's NaiveDateTime range: the reference panics on it "
                   "('invalid or out-of-range datetime', metric.rs:210)";
    }
    return rc;
}

int kta_analytics_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64)
{
    return section_vector(ctx, KTA_RV_ANALYTICS, false, device_ptr, n_u64);
}

int kta_decode_analytics(const uint64_t *vec, uint32_t P, kta_analytics *out, int64_t *part_min_ts_sec,
                         int64_t *part_max_ts_sec, uint64_t *part_smallest, uint64_t *part_largest)
{
    if (!vec || !out || P == 0) return KTA_ERR_INVALID;
    for (int b = 0; b < KTA_HIST_BUCKETS; b++) {
        out->key_size_hist[b] = vec[b];
        out->value_size_hist[b] = vec[KTA_HIST_BUCKETS + b];
    }
    for (uint32_t p = 0; p < P; p++) {
        const int64_t *x = reinterpret_cast<const int64_t *>(vec) + kta::kAnalyticsHist + 4 * (size_t)p;
        const bool seen = x[1] != INT64_MIN;     // max ts never written => no record in this partition
        const bool live = x[3] != INT64_MIN;     // largest never written => no non-tombstone
        if (part_min_ts_sec) part_min_ts_sec[p] = seen ? (~x[0]) / 1000 : INT64_MAX;  // metric.rs:210 (monotone)
        if (part_max_ts_sec) part_max_ts_sec[p] = seen ? x[1] / 1000 : INT64_MIN;
        if (part_smallest) part_smallest[p] = live ? (uint64_t)~x[2] : UINT64_MAX;
        if (part_largest) part_largest[p] = live ? (uint64_t)x[3] : 0;
    }
    return KTA_OK;
}

int kta_merge_analytics(uint64_t *acc, const uint64_t *other, uint32_t P)
{
    return merge_section(acc, other, P != 0, analytics_shape(P));
}

// The analytics read-back is struct-shaped: the section's live vector (staged messages flushed first) or its snapshot,
// copied to the host and decoded.  The buffers and the guard are its row's.
static int read_analytics(kta_ctx *ctx, bool snapshot, kta_analytics *out, int64_t *part_min_ts_sec, int64_t *part_max_ts_sec,
                          uint64_t *part_smallest, uint64_t *part_largest)
{
    if (!ctx || !out) return KTA_ERR_INVALID;
    const Section s = section(ctx, KTA_RV_ANALYTICS);
    if (!s.on) return fail(ctx, KTA_ERR_INVALID, s.off);
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    int rc = snapshot ? KTA_OK : kta_flush(ctx);
    if (rc != KTA_OK) return rc;
    std::vector<uint64_t> host(s.shape.words);
    rc = read_words(ctx, (snapshot ? s.out : s.live)->get(), host.data(), host.size());
    if (rc != KTA_OK) return rc;
    return kta_decode_analytics(host.data(), ctx->P, out, part_min_ts_sec, part_max_ts_sec, part_smallest, part_largest);
}

int kta_get_analytics(kta_ctx *ctx, kta_analytics *out, int64_t *part_min_ts_sec, int64_t *part_max_ts_sec,
                      uint64_t *part_smallest, uint64_t *part_largest)
{
    return read_analytics(ctx, false, out, part_min_ts_sec, part_max_ts_sec, part_smallest, part_largest);
}

int kta_exchange_analytics(kta_ctx *ctx, kta_analytics *out, int64_t *part_min_ts_sec, int64_t *part_max_ts_sec,
                           uint64_t *part_smallest, uint64_t *part_largest)
{
    return read_analytics(ctx, true, out, part_min_ts_sec, part_max_ts_sec, part_smallest, part_largest);
}

int kta_analytics_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64)
{
    return section_vector(ctx, KTA_RV_ANALYTICS, true, device_ptr, n_u64);
}

// The largest P whose scan plan (raw and tile-compact) with `timeline_buckets` (0: none) fits one workgroup's LDS on
// gfx950, its static reduction arrays (kta_metrics_scan's s_red) included.
static uint32_t max_partitions_for(bool analytics, uint32_t timeline_buckets)
{
    const uint32_t lds_limit = 160u * 1024u, static_lds = (kta::kWG / 64u) * 6u * 8u;
    uint32_t lo = 0, hi = 4096;
    while (lo < hi) {   // lds_bytes grows with P: the largest P that fits
        const uint32_t mid = (lo + hi + 1) / 2;
        const uint32_t lds = std::max(kta::plan_scan(mid, 1, 1, 1, 0, analytics, false, timeline_buckets).lds_bytes,
                                      kta::plan_scan(mid, 1, 1, 1, 0, analytics, true, timeline_buckets).lds_bytes);
        if (lds + static_lds <= lds_limit) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

int kta_analytics_max_partitions(void) { return (int)max_partitions_for(true, 0); }

int kta_timeline_max_partitions(uint32_t flags, uint32_t n_buckets)
{
    if (n_buckets < 1 || n_buckets > KTA_TIMELINE_MAX_BUCKETS) return 0;
    return (int)max_partitions_for((flags & KTA_FLAG_ANALYTICS) != 0, n_buckets);
}

int kta_set_timeline(kta_ctx *ctx, int64_t origin_ms, int64_t bucket_ms, uint32_t n_buckets)
{
    if (!ctx) return KTA_ERR_INVALID;
    if (origin_ms < 0) return fail(ctx, KTA_ERR_INVALID, "kta_set_timeline: origin_ms must be >= 0");
    if (bucket_ms < 1) return fail(ctx, KTA_ERR_INVALID, "kta_set_timeline: bucket_ms must be >= 1");
    if (n_buckets < 1 || n_buckets > KTA_TIMELINE_MAX_BUCKETS)
        return fail(ctx, KTA_ERR_INVALID, "kta_set_timeline: n_buckets must be in [1, " +
                                              std::to_string(KTA_TIMELINE_MAX_BUCKETS) + "]");
    if (bucket_ms > (INT64_MAX - origin_ms) / (int64_t)n_buckets)
        return fail(ctx, KTA_ERR_INVALID, "kta_set_timeline: origin_ms + n_buckets * bucket_ms overflows int64");
    if (ctx->handed_records || ctx->fill_n)
        return fail(ctx, KTA_ERR_INVALID, "kta_set_timeline: the context has been handed records since kta_create / kta_reset");
    const uint32_t pmax = max_partitions_for(ctx->analytics, n_buckets);
    if (ctx->P > pmax)
        return fail(ctx, KTA_ERR_INVALID, "kta_set_timeline: the scan's LDS plan with " + std::to_string(n_buckets) +
                                              " buckets admits at most " + std::to_string(pmax) + " partitions" +
                                              (ctx->analytics ? " with KTA_FLAG_ANALYTICS" : ""));
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    const Section s = section(ctx, KTA_RV_TIMELINE);
    const size_t words = timeline_shape(n_buckets).words;
    const bool fits = ctx->timeline && ctx->tl.n_buckets == n_buckets;
    if (!fits) ctx->timeline = false;   // (until both vectors have the new length)
    int rc = fits ? clear_section(ctx, s, words) : alloc_section(ctx, s, words);
    if (rc != KTA_OK) return rc;
    ctx->tl.origin = origin_ms;
    ctx->tl.width = (unsigned long long)bucket_ms;
    ctx->tl.span = (unsigned long long)bucket_ms * n_buckets;
    ctx->tl.inv_width = (float)(1.0 / (double)bucket_ms);
    ctx->tl.n_buckets = n_buckets;
    ctx->tl.vec = ctx->d_tvec.get();
    ctx->timeline = true;
    return KTA_OK;
}

int kta_get_timeline(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return get_section(ctx, KTA_RV_TIMELINE, out, n_u64); }
int kta_exchange_timeline(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return exchange_section(ctx, KTA_RV_TIMELINE, out, n_u64); }
int kta_timeline_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64) { return section_vector(ctx, KTA_RV_TIMELINE, false, device_ptr, n_u64); }
int kta_timeline_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64)
{
    return section_vector(ctx, KTA_RV_TIMELINE, true, device_ptr, n_u64);
}

// The key sketch is the section table's one exception: its live registers are u32, so the live read-back widens them on
// the host (and kta_finish_device launches a kernel that widens them into the snapshot).
int kta_get_key_sketch(kta_ctx *ctx, uint64_t *out, size_t n_u64)
{
    Section s;
    int rc = begin_read(ctx, KTA_RV_KEY_SKETCH, out, n_u64, &s);
    if (rc != KTA_OK) return rc;
    rc = kta_flush(ctx);
    if (rc != KTA_OK) return rc;
    std::vector<uint32_t> host(n_u64);
    KTA_HIP(ctx, hipMemcpyAsync(host.data(), ctx->d_sketch.get(), n_u64 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->s_compute));
    KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));
    for (size_t i = 0; i < n_u64; i++) out[i] = host[i];
    return KTA_OK;
}

int kta_exchange_key_sketch(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return exchange_section(ctx, KTA_RV_KEY_SKETCH, out, n_u64); }
int kta_key_sketch_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64)
{
    return section_vector(ctx, KTA_RV_KEY_SKETCH, true, device_ptr, n_u64);
}

int kta_key_sketch_info(kta_ctx *ctx, uint64_t out[4])
{
    if (!ctx || !out) return KTA_ERR_INVALID;
    if (!ctx->sketch) return section_off(ctx, KTA_RV_KEY_SKETCH);
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    int rc = read_words(ctx, ctx->d_sketch_stats.get(), out, 3);
    out[3] = ctx->sketch_launches;
    return rc;
}

int kta_merge_key_sketch(uint64_t *acc, const uint64_t *other, uint32_t P)
{
    return merge_section(acc, other, P != 0 && P <= KTA_SKETCH_MAX_PARTITIONS, key_sketch_shape(P));
}

int kta_get_hot_keys(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return get_section(ctx, KTA_RV_HOT_KEYS, out, n_u64); }
int kta_exchange_hot_keys(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return exchange_section(ctx, KTA_RV_HOT_KEYS, out, n_u64); }
int kta_hot_keys_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64)
{
    return section_vector(ctx, KTA_RV_HOT_KEYS, true, device_ptr, n_u64);
}

int kta_get_hot_key_exemplars(kta_ctx *ctx, kta_hot_exemplar *out, size_t n_slots)
{
    if (!ctx || !out) return KTA_ERR_INVALID;
    if (!ctx->hot) return section_off(ctx, KTA_RV_HOT_KEYS);
    if (n_slots != kHotSlotsN)
        return fail(ctx, KTA_ERR_INVALID, "the exemplar table has " + std::to_string(kHotSlotsN) + " slots, not " + std::to_string(n_slots));
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    int rc = kta_flush(ctx);
    if (rc != KTA_OK) return rc;
    KTA_HIP(ctx, hipMemcpyAsync(out, ctx->d_hot_slots.get(), kHotSlotsN * sizeof(kta_hot_exemplar), hipMemcpyDeviceToHost, ctx->s_compute));
    KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));
    return KTA_OK;
}

int kta_hot_keys_info(kta_ctx *ctx, uint64_t out[6])
{
    if (!ctx || !out) return KTA_ERR_INVALID;
    if (!ctx->hot) return section_off(ctx, KTA_RV_HOT_KEYS);
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    uint64_t st[4];
    int rc = read_words(ctx, ctx->d_hot_stats.get(), st, 4);
    out[0] = st[0], out[1] = st[1], out[2] = st[2], out[3] = ctx->hot_launches, out[4] = st[3], out[5] = ctx->hot_workgroups;
    return rc;
}

int kta_set_hot_flush_rounds(kta_ctx *ctx, uint32_t rounds)
{
    if (!ctx) return KTA_ERR_INVALID;
    if (!ctx->hot) return section_off(ctx, KTA_RV_HOT_KEYS);
    if (rounds > kta::kHotFlushRoundsMax)
        return fail(ctx, KTA_ERR_INVALID, "a workgroup flushes after at most " + std::to_string(kta::kHotFlushRoundsMax) + " rounds");
    ctx->hot_flush_rounds = rounds;
    return KTA_OK;
}

int kta_merge_hot_keys(uint64_t *acc, const uint64_t *other) { return merge_section(acc, other, true, hot_keys_shape()); }

int kta_ts_order_max_partitions(void) { return (int)kta::kTsOrderMaxPartitions; }

int kta_get_ts_order(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return get_section(ctx, KTA_RV_TS_ORDER, out, n_u64); }
int kta_exchange_ts_order(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return exchange_section(ctx, KTA_RV_TS_ORDER, out, n_u64); }
int kta_ts_order_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64)
{
    return section_vector(ctx, KTA_RV_TS_ORDER, true, device_ptr, n_u64);
}

int kta_merge_ts_order(uint64_t *acc, const uint64_t *other, uint32_t P)
{
    return merge_section(acc, other, P != 0 && P <= kta::kTsOrderMaxPartitions, ts_order_shape(P));
}

int kta_ts_order_info(kta_ctx *ctx, uint64_t out[6])
{
    if (!ctx || !out) return KTA_ERR_INVALID;
    if (!ctx->tso) return section_off(ctx, KTA_RV_TS_ORDER);
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    uint64_t st[3];
    int rc = read_words(ctx, ctx->d_tso_stats.get(), st, 3);
    out[0] = ctx->tso_launches, out[1] = ctx->tso_chunks, out[2] = st[0], out[3] = st[1], out[4] = st[2], out[5] = ctx->tso_last_chunk;
    return rc;
}

int kta_set_ts_order_chunk(kta_ctx *ctx, uint64_t records)
{
    if (!ctx) return KTA_ERR_INVALID;
    if (!ctx->tso) return section_off(ctx, KTA_RV_TS_ORDER);
    if (records % 64 != 0 || records > (1ull << 32))
        return fail(ctx, KTA_ERR_INVALID, "a chunk is a multiple of 64 records, at most 2^32 (0: the default)");
    ctx->tso_chunk = records;
    return KTA_OK;
}

int kta_segments_max_partitions(void) { return (int)kta::kSegmentsMaxPartitions; }

uint32_t kta_segments_words(uint32_t P, uint32_t M) { return kta::segments_config_ok(1, M, P) ? (uint32_t)kta::segments_len(P, M) : 0u; }

int kta_set_segments(kta_ctx *ctx, uint64_t segment_bytes, uint32_t rows_per_partition, uint32_t record_overhead)
{
    if (!ctx) return KTA_ERR_INVALID;
    if (segment_bytes < 1 || segment_bytes > kta::kSegmentsMaxBytes)
        return fail(ctx, KTA_ERR_INVALID, "kta_set_segments: segment_bytes must be in [1, 2^40]");
    if (rows_per_partition < 2 || (uint64_t)rows_per_partition * ctx->P > kta::kSegmentsMaxRows)
        return fail(ctx, KTA_ERR_INVALID, "kta_set_segments: rows_per_partition must be at least 2 and P * rows_per_partition at most 2^20");
    if (ctx->P > kta::kSegmentsMaxPartitions)
        return fail(ctx, KTA_ERR_INVALID, "kta_set_segments admits at most " + std::to_string(kta::kSegmentsMaxPartitions) + " partitions");
    if (ctx->handed_records || ctx->fill_n)
        return fail(ctx, KTA_ERR_INVALID, "kta_set_segments: the context has been handed records since kta_create / kta_reset");
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    const size_t words = segments_shape(ctx->P, rows_per_partition).words;
    if (!ctx->seg || ctx->seg_M != rows_per_partition) {
        ctx->seg = false;               // (until both vectors have the new length)
        int rc = alloc_section(ctx, section(ctx, KTA_RV_SEGMENTS), words);
        if (rc != KTA_OK) return rc;
    }
    if (!ctx->d_seg_ws) {
        KTA_HIP(ctx, ctx->d_seg_ws.alloc(kta::kSegmentsWorkspaceWords));
        KTA_HIP(ctx, ctx->d_seg_flags.alloc(kta::kSegmentsWorkspaceWords / kta::kSegWords));
        KTA_HIP(ctx, ctx->d_seg_stats.alloc(4));
    }
    ctx->seg_S = segment_bytes, ctx->seg_M = rows_per_partition, ctx->seg_overhead = record_overhead;
    ctx->cd = false;                    // (the kept vector has the old configuration's shape: kta_set_compact_delete comes after this)
    int rc = clear_segments(ctx);
    if (rc != KTA_OK) return rc;
    KTA_HIP(ctx, hipMemcpyAsync(ctx->d_seg_out.get(), ctx->d_seg.get(), words * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->s_compute));
    ctx->seg = true;
    return KTA_OK;
}

int kta_get_segments(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return get_section(ctx, KTA_RV_SEGMENTS, out, n_u64); }
int kta_exchange_segments(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return exchange_section(ctx, KTA_RV_SEGMENTS, out, n_u64); }
int kta_segments_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64)
{
    return section_vector(ctx, KTA_RV_SEGMENTS, true, device_ptr, n_u64);
}

int kta_segments_info(kta_ctx *ctx, uint64_t out[6])
{
    if (!ctx || !out) return KTA_ERR_INVALID;
    if (!ctx->seg) return section_off(ctx, KTA_RV_SEGMENTS);
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    int rc = kta_flush(ctx);
    if (rc != KTA_OK) return rc;
    uint64_t st[4];
    rc = read_words(ctx, ctx->d_seg_stats.get(), st, 4);
    out[0] = ctx->seg_chunks, out[1] = ctx->seg_last_chunk, out[2] = ctx->seg_launches, out[3] = st[0], out[4] = st[1], out[5] = st[3];
    return rc;
}

int kta_set_segments_chunk(kta_ctx *ctx, uint64_t records)
{
    if (!ctx) return KTA_ERR_INVALID;
    if (!ctx->seg) return section_off(ctx, KTA_RV_SEGMENTS);
    if (records % 64 != 0 || records > (1ull << 31))
        return fail(ctx, KTA_ERR_INVALID, "a chunk is a multiple of 64 records, at most 2^31 (0: the default)");
    ctx->seg_chunk = records;
    return KTA_OK;
}

int kta_merge_segments(uint64_t *acc, const uint64_t *other, uint32_t P, uint32_t M)
{
    if (!acc || !other || !kta::segments_config_ok(1, M, P)) return KTA_ERR_INVALID;
    return kta::segments_merge(acc, other, P, M) ? KTA_OK : KTA_ERR_INVALID;
}

int kta_retention_whatif(const uint64_t *vec, uint32_t P, uint32_t M, int64_t now_ms, int64_t retention_ms, int64_t retention_bytes, uint64_t *out,
                         size_t n_u64)
{
    if (!vec || !out || !kta::segments_config_ok(1, M, P) || n_u64 != ((size_t)P + 1) * KTA_RETENTION_WORDS) return KTA_ERR_INVALID;
    if (retention_ms < -1 || retention_bytes < -1) return KTA_ERR_INVALID;
    const uint64_t *g = vec + kta::segments_globals_at(P, M);
    if (g[kta::kSegGlobalM] != M || !kta::segments_config_ok(g[kta::kSegGlobalS], M, P)) return KTA_ERR_INVALID;   // not a vector of this shape
    kta::retention_whatif(vec, P, M, now_ms, retention_ms, retention_bytes, out);
    return KTA_OK;
}

int kta_partitioner_max_partitions(void) { return (int)kta::kPartitionerMaxPartitions; }

uint32_t kta_murmur2(const void *key, size_t len)
{
    // the words in place, the tail bytes from a copy (the device's tail word may end 3 bytes past the key)
    const uint8_t *k = static_cast<const uint8_t *>(key);
    uint32_t h = kta::kMurmur2Seed ^ (uint32_t)len;
    const size_t words = len >> 2;
    for (size_t d = 0; d < words; d++) h = kta::murmur2_word(h, kta::murmur2_load32(k + 4 * d));
    uint8_t tail[4] = {0};
    if (len & 3u) memcpy(tail, k + 4 * words, len & 3u);
    return kta::murmur2_finish(h, kta::murmur2_load32(tail), (uint32_t)len);
}

int kta_set_repartition(kta_ctx *ctx, uint32_t q)
{
    if (!ctx) return KTA_ERR_INVALID;
    if (!ctx->part) return section_off(ctx, KTA_RV_PARTITIONER);
    if (q < 1 || q > kta::kPartitionerMaxPartitions)
        return fail(ctx, KTA_ERR_INVALID, "kta_set_repartition: Q must be in [1, " + std::to_string(kta::kPartitionerMaxPartitions) + "]");
    if (ctx->handed_records || ctx->fill_n)
        return fail(ctx, KTA_ERR_INVALID, "kta_set_repartition: the context has been handed records since kta_create / kta_reset");
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    const Section s = section(ctx, KTA_RV_PARTITIONER);
    const size_t words = partitioner_shape(ctx->P, q).words;
    if (q == ctx->part_q) return clear_section(ctx, s, words);
    int rc = alloc_section(ctx, s, words);
    if (rc != KTA_OK) return rc;
    ctx->part_q = q;
    return KTA_OK;
}

int kta_get_partitioner(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return get_section(ctx, KTA_RV_PARTITIONER, out, n_u64); }
int kta_exchange_partitioner(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return exchange_section(ctx, KTA_RV_PARTITIONER, out, n_u64); }
int kta_partitioner_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64)
{
    return section_vector(ctx, KTA_RV_PARTITIONER, true, device_ptr, n_u64);
}

int kta_merge_partitioner(uint64_t *acc, const uint64_t *other, uint32_t P, uint32_t q)
{
    const uint32_t most = kta::kPartitionerMaxPartitions;
    return merge_section(acc, other, P != 0 && P <= most && q != 0 && q <= most, partitioner_shape(P, q));
}

int kta_partitioner_info(kta_ctx *ctx, uint64_t out[6])
{
    if (!ctx || !out) return KTA_ERR_INVALID;
    if (!ctx->part) return section_off(ctx, KTA_RV_PARTITIONER);
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    uint64_t st[3];
    int rc = read_words(ctx, ctx->d_part_stats.get(), st, 3);
    uint32_t plan[3];
    kta::partitioner_lds_plan(ctx->P, ctx->part_q, plan);
    out[0] = st[0], out[1] = ctx->part_launches, out[2] = st[1], out[3] = st[2], out[4] = ctx->part_workgroups, out[5] = plan[0];
    return rc;
}

// ---- size percentiles (kta_size_bins.h holds the rule, kta_size_quantiles.hip the kernel) -------------------------------

int kta_size_quantiles_max_partitions(void) { return (int)kta::kSizeQuantilesMaxPartitions; }

uint32_t kta_size_bin(uint32_t size) { return kta::size_bin(size); }

int kta_size_bin_bounds(uint32_t bin, uint64_t *lo, uint64_t *hi)
{
    if (bin >= kta::kSizeBins || !lo || !hi) return KTA_ERR_INVALID;
    *lo = kta::size_bin_lo(bin), *hi = kta::size_bin_hi(bin);
    return KTA_OK;
}

int kta_size_quantile(const uint64_t *hist, uint64_t num, uint64_t den, uint64_t *lo, uint64_t *hi)
{
    if (!hist || !lo || !hi || den == 0 || num > den) return KTA_ERR_INVALID;
    uint32_t bin = 0;
    if (!kta::size_quantile(hist, num, den, &bin)) return 0;
    *lo = kta::size_bin_lo(bin), *hi = kta::size_bin_hi(bin);
    return 1;
}

int kta_get_size_quantiles(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return get_section(ctx, KTA_RV_SIZE_QUANTILES, out, n_u64); }
int kta_exchange_size_quantiles(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return exchange_section(ctx, KTA_RV_SIZE_QUANTILES, out, n_u64); }
int kta_size_quantiles_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64)
{
    return section_vector(ctx, KTA_RV_SIZE_QUANTILES, true, device_ptr, n_u64);
}

int kta_merge_size_quantiles(uint64_t *acc, const uint64_t *other, uint32_t P)
{
    return merge_section(acc, other, P != 0 && P <= kta::kSizeQuantilesMaxPartitions, size_quantiles_shape(P));
}

int kta_set_size_quantiles_slice(kta_ctx *ctx, uint32_t partitions)
{
    if (!ctx) return KTA_ERR_INVALID;
    if (!ctx->sizeq) return section_off(ctx, KTA_RV_SIZE_QUANTILES);
    if (partitions > kta::kSizeQuantilesMaxSlice)
        return fail(ctx, KTA_ERR_INVALID, "kta_set_size_quantiles_slice: at most " + std::to_string(kta::kSizeQuantilesMaxSlice) + " partitions (0: the default)");
    ctx->sizeq_slice = partitions;
    return KTA_OK;
}

int kta_size_quantiles_info(kta_ctx *ctx, uint64_t out[6])
{
    if (!ctx || !out) return KTA_ERR_INVALID;
    if (!ctx->sizeq) return section_off(ctx, KTA_RV_SIZE_QUANTILES);
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    int rc = kta_flush(ctx);
    if (rc != KTA_OK) return rc;
    uint64_t adds = 0;
    rc = read_words(ctx, ctx->d_sizeq_stats.get(), &adds, 1);
    uint32_t plan[5];
    kta::size_quantiles_plan(ctx->P, ctx->sizeq_slice, plan);
    out[0] = plan[0], out[1] = plan[1], out[2] = plan[2], out[3] = plan[3], out[4] = ctx->sizeq_last_workgroups, out[5] = adds;
    return rc;
}

// ---- record batches (kta_record_batches.h holds the rule, kta_record_batches.hip the kernel, kta_kafka.hip the launch) ----

int kta_get_record_batches(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return get_section(ctx, KTA_RV_RECORD_BATCHES, out, n_u64); }
int kta_exchange_record_batches(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return exchange_section(ctx, KTA_RV_RECORD_BATCHES, out, n_u64); }
int kta_record_batches_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64)
{
    return section_vector(ctx, KTA_RV_RECORD_BATCHES, true, device_ptr, n_u64);
}
int kta_record_batches_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64)
{
    return section_vector(ctx, KTA_RV_RECORD_BATCHES, false, device_ptr, n_u64);
}

int kta_merge_record_batches(uint64_t *acc, const uint64_t *other, uint32_t P)
{
    return merge_section(acc, other, P != 0 && P <= 4096, record_batches_shape(P));
}

int kta_record_batches_estimate_producers(const uint64_t *vec, uint32_t P, double *out)
{
    if (!vec || !out || P == 0 || P > 4096) return KTA_ERR_INVALID;
    *out = kta::rb_estimate(vec + kta::rb_sketch_at(P));
    return KTA_OK;
}

int kta_record_batches_identities(const uint64_t *vec, uint32_t P)
{
    if (!vec || P == 0 || P > 4096) return KTA_ERR_INVALID;
    return kta::rb_identities_hold(vec, P) ? 1 : 0;
}

int kta_record_batches_host(const uint8_t *bytes, uint64_t len, int32_t partition, const uint64_t *inflated, uint64_t *vec, uint32_t P)
{
    if (!bytes || !vec || P == 0 || P > 4096) return KTA_ERR_INVALID;
    kta_kafka_index_stats st;
    int rc = kta_kafka_index_host(bytes, len, partition, 0, 0, (len + 127) & ~63ull, nullptr, 0, &st);
    if (rc != KTA_OK && rc != KTA_ERR_CAPACITY) return rc;
    std::vector<kta_kafka_batch_desc> descs(st.n_batches);
    rc = kta_kafka_index_host(bytes, len, partition, 0, 0, (len + 127) & ~63ull, descs.data(), descs.size(), &st);
    if (rc != KTA_OK) return rc;
    for (size_t i = 0; i < descs.size(); i++) {
        kta_kafka_batch_desc d = descs[i];
        if (inflated && (d.flags & (KTA_KB_SNAPPY | KTA_KB_LZ4 | KTA_KB_GZIP | KTA_KB_ZSTD))) d.payload_end = d.payload_off + inflated[i];
        if (!kta::rb_counted(kta::rb_no_filter(), P, d.partition, d.base_ts_ms, d.max_ts_ms)) continue;
        const bool inside = kta::rb_header_inside(d.byte_off, len);
        kta::rb_accumulate(vec, P, (uint32_t)d.partition, inside && d.status == 0 ? kta::rb_batch(d, kta::rb_fields(bytes + d.byte_off)) : kta::rb_failed_batch());
    }
    return KTA_OK;
}

// ---- payload (kta_payload.h holds the rule, kta_payload.hip the kernel, kta_kafka.hip the launch) -------------------------

int kta_get_payload(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return get_section(ctx, KTA_RV_PAYLOAD, out, n_u64); }
int kta_exchange_payload(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return exchange_section(ctx, KTA_RV_PAYLOAD, out, n_u64); }
int kta_payload_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64) { return section_vector(ctx, KTA_RV_PAYLOAD, true, device_ptr, n_u64); }
int kta_payload_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64) { return section_vector(ctx, KTA_RV_PAYLOAD, false, device_ptr, n_u64); }
int kta_merge_payload(uint64_t *acc, const uint64_t *other, uint32_t P) { return merge_section(acc, other, P != 0 && P <= 4096, payload_shape(P)); }

int kta_payload_identities(const uint64_t *vec, const uint64_t *counter_vec, uint32_t P)
{
    if (!vec || P == 0 || P > 4096) return KTA_ERR_INVALID;
    return kta::payload_identities_hold(vec, P, counter_vec, KTA_NCOUNTERS) ? 1 : 0;
}

int kta_payload_schema_ids(const uint64_t *vec, uint32_t P, uint32_t *ids, uint64_t *records, uint64_t *bytes, size_t cap, size_t *n,
                           uint64_t *unresolved_records, uint64_t *unresolved_bytes)
{
    if (!vec || !n || P == 0 || P > 4096 || (cap && (!ids || !records || !bytes))) return KTA_ERR_INVALID;
    const std::vector<kta::PayloadSchemaId> found = kta::payload_schema_ids(vec, P, unresolved_records, unresolved_bytes);
    *n = found.size();
    for (size_t i = 0; i < found.size() && i < cap; i++) ids[i] = found[i].id, records[i] = found[i].records, bytes[i] = found[i].bytes;
    return KTA_OK;
}

int kta_payload_host(const uint8_t *bytes, uint64_t len, int32_t partition, uint64_t *vec, uint32_t P)
{
    if (!bytes || !vec || P == 0 || P > 4096) return KTA_ERR_INVALID;
    if (partition < 0 || (uint32_t)partition >= P) return KTA_OK;             // outside [0, P): adds nothing
    auto passes = [](long long) { return true; };                               // (no context, no filter)
    return host_batches(bytes, len, partition, [&](const uint8_t *recs, uint64_t n, uint64_t n_records) {
        kta::payload_batch_host(vec, P, (uint32_t)partition, recs, 0, n, n_records, passes);
    });
}

// ---- header names (kta_header_names.h holds the rule, kta_header_names.hip the kernel, kta_kafka.hip the launch) ---------

int kta_get_header_names(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return get_section(ctx, KTA_RV_HEADER_NAMES, out, n_u64); }
int kta_exchange_header_names(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return exchange_section(ctx, KTA_RV_HEADER_NAMES, out, n_u64); }
int kta_header_names_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64)
{
    return section_vector(ctx, KTA_RV_HEADER_NAMES, true, device_ptr, n_u64);
}
int kta_header_names_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64) { return section_vector(ctx, KTA_RV_HEADER_NAMES, false, device_ptr, n_u64); }
int kta_merge_header_names(uint64_t *acc, const uint64_t *other) { return merge_section(acc, other, true, header_names_shape()); }

int kta_get_header_name_table(kta_ctx *ctx, kta_header_name *out, size_t n_slots)
{
    if (!ctx || !out) return KTA_ERR_INVALID;
    if (!ctx->hn) return section_off(ctx, KTA_RV_HEADER_NAMES);
    if (n_slots != kta::kHnSlots)
        return fail(ctx, KTA_ERR_INVALID, "the name table has " + std::to_string(kta::kHnSlots) + " slots, not " + std::to_string(n_slots));
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    int rc = kta_flush(ctx);
    if (rc != KTA_OK) return rc;
    KTA_HIP(ctx, hipMemcpyAsync(out, ctx->d_hn_names.get(), kta::kHnSlots * sizeof(kta_header_name), hipMemcpyDeviceToHost, ctx->s_compute));
    KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));
    for (size_t i = 0; i < n_slots; i++)                                        // only published slots leave the library
        if (out[i].state != KTA_HEADER_NAME_PUBLISHED) memset(&out[i], 0, sizeof out[i]);
    return KTA_OK;
}

int kta_header_names_identities(const uint64_t *vec, const uint64_t *payload_vec, uint32_t P)
{
    if (!vec || (payload_vec && (P == 0 || P > 4096))) return KTA_ERR_INVALID;
    return kta::hn_identities_hold(vec, payload_vec, P) ? 1 : 0;
}

int kta_header_names_list(const uint64_t *vec, const kta_header_name *table, kta_header_name_row *rows, size_t cap, size_t *n,
                          uint64_t *unresolved_occurrences, uint64_t *unresolved_value_bytes)
{
    if (!vec || !n || (cap && !rows)) return KTA_ERR_INVALID;
    const std::vector<kta::HnListed> found =
        kta::hn_list(vec, reinterpret_cast<const kta::HnSlot *>(table), unresolved_occurrences, unresolved_value_bytes);
    *n = found.size();
    for (size_t i = 0; i < found.size() && i < cap; i++) {
        kta_header_name_row &r = rows[i];
        memset(&r, 0, sizeof r);
        r.hash = found[i].hash, r.occurrences = found[i].occurrences, r.name_len = found[i].name_len, r.value_bytes = found[i].value_bytes;
        r.null_values = found[i].null_values;
        if (found[i].name) r.has_name = 1, memcpy(r.name, found[i].name->bytes, sizeof r.name);
    }
    return KTA_OK;
}

int kta_header_names_host(const uint8_t *bytes, uint64_t len, int32_t partition, uint64_t *vec, kta_header_name *table, uint32_t P)
{
    if (!bytes || !vec || P == 0 || P > 4096) return KTA_ERR_INVALID;
    if (partition < 0 || (uint32_t)partition >= P) return KTA_OK;             // outside [0, P): adds nothing
    auto passes = [](long long) { return true; };                               // (no context, no filter)
    return host_batches(bytes, len, partition, [&](const uint8_t *recs, uint64_t n, uint64_t n_records) {
        kta::hn_batch_host(vec, reinterpret_cast<kta::HnSlot *>(table), recs, 0, n, n_records, passes);
    });
}

// ---- value bytes (kta_value_bytes.h holds the rule, kta_value_bytes.hip the kernel, kta_kafka.hip the launch) --------------

int kta_get_value_bytes(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return get_section(ctx, KTA_RV_VALUE_BYTES, out, n_u64); }
int kta_exchange_value_bytes(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return exchange_section(ctx, KTA_RV_VALUE_BYTES, out, n_u64); }
int kta_value_bytes_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64)
{
    return section_vector(ctx, KTA_RV_VALUE_BYTES, true, device_ptr, n_u64);
}
int kta_value_bytes_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64) { return section_vector(ctx, KTA_RV_VALUE_BYTES, false, device_ptr, n_u64); }
int kta_merge_value_bytes(uint64_t *acc, const uint64_t *other, uint32_t P)
{
    return merge_section(acc, other, P != 0, value_bytes_shape(P));
}

int kta_value_bytes_identities(const uint64_t *vec, uint32_t P, const uint64_t *payload_vec, const uint64_t *counter_vec)
{
    if (!vec || P == 0 || (payload_vec && P > 4096)) return KTA_ERR_INVALID;   // (a payload vector has 4096 partitions at most)
    return kta::value_bytes_identities_hold(vec, P, payload_vec, counter_vec, KTA_NCOUNTERS) ? 1 : 0;
}

int kta_value_bytes_summary(const uint64_t *words, kta_value_bytes_summary_t *out)
{
    if (!words || !out) return KTA_ERR_INVALID;
    const kta::ValueBytesSummary s = kta::value_bytes_summary(words);
    memset(out, 0, sizeof *out);
    out->records = s.records, out->values = s.values, out->bytes = s.bytes, out->repeats = s.repeats, out->distinct = s.distinct;
    out->floor_bytes = s.floor_bytes, out->printable = s.printable, out->zero = s.zero, out->high = s.high, out->top_count = s.top_count;
    out->entropy_bits = s.entropy_bits, out->top_byte = s.top_byte, out->cls = s.cls;
    return KTA_OK;
}

int kta_value_bytes_host(const uint8_t *bytes, uint64_t len, int32_t partition, uint64_t *vec, uint32_t P)
{
    if (!bytes || !vec || P == 0) return KTA_ERR_INVALID;
    if (partition < 0 || (uint32_t)partition >= P) return KTA_OK;             // outside [0, P): adds nothing
    auto passes = [](long long) { return true; };                               // (no context, no filter)
    return host_batches(bytes, len, partition, [&](const uint8_t *recs, uint64_t n, uint64_t n_records) {
        kta::value_bytes_batch_host(vec, (uint32_t)partition, recs, 0, n, n_records, passes);
    });
}

// ---- compression what-if (kta_lz4_model.h holds the model and the rule, kta_lz4_model.hip the kernel, kta_kafka.hip the launch)

int kta_get_compress_whatif(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return get_section(ctx, KTA_RV_COMPRESS_WHATIF, out, n_u64); }
int kta_exchange_compress_whatif(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return exchange_section(ctx, KTA_RV_COMPRESS_WHATIF, out, n_u64); }
int kta_compress_whatif_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64)
{
    return section_vector(ctx, KTA_RV_COMPRESS_WHATIF, true, device_ptr, n_u64);
}
int kta_compress_whatif_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64)
{
    return section_vector(ctx, KTA_RV_COMPRESS_WHATIF, false, device_ptr, n_u64);
}
int kta_merge_compress_whatif(uint64_t *acc, const uint64_t *other, uint32_t P)
{
    return merge_section(acc, other, P != 0, compress_whatif_shape(P));
}

int kta_compress_whatif_identities(const uint64_t *vec, uint32_t P)
{
    if (!vec || P == 0) return KTA_ERR_INVALID;
    return kta::compress_whatif_identities_hold(vec, P) ? 1 : 0;
}

int64_t kta_lz4_model_host(const uint8_t *src, uint64_t n, uint8_t *dst, uint64_t cap)
{
    if (!src && n) return -1;
    std::vector<uint32_t> table(kta::kLz4mTable);
    if (!dst) {
        kta::Lz4mCount out;
        return (int64_t)kta::lz4m_frame(src, n, table.data(), out).frame_bytes;
    }
    kta::Lz4mEmit out{dst, cap};
    return (int64_t)kta::lz4m_frame(src, n, table.data(), out).frame_bytes;
}

int kta_compress_whatif_host(const uint8_t *bytes, uint64_t len, int32_t partition, uint64_t *vec, uint32_t P)
{
    if (!bytes || !vec || P == 0) return KTA_ERR_INVALID;
    if (partition < 0 || (uint32_t)partition >= P) return KTA_OK;             // outside [0, P): adds nothing
    return host_batches_described(bytes, len, partition, [&](const kta_kafka_batch_desc &d, const uint8_t *recs, uint64_t n) {
        kta::compress_whatif_add(vec, P, (uint32_t)partition, kta::compress_whatif_codec(d.flags), d.batch_bytes, recs, n);
    });
}

// ---- compaction what-if (kta_compaction.h holds the rule, kta_compaction.hip the kernel) --------------------------------

int kta_compaction_max_partitions(void) { return (int)kta::kCompactionMaxPartitions; }

int kta_compaction_replay(kta_ctx *ctx, int on)
{
    if (!ctx) return KTA_ERR_INVALID;
    if (!ctx->comp) return section_off(ctx, KTA_SEC_COMPACTION);
    const bool want = on != 0;
    if (want == ctx->comp_replay) return KTA_OK;
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    int rc = kta_flush(ctx);   // what was staged goes where it was staged for
    if (rc != KTA_OK) return rc;
    if (want) {
        rc = clear_section(ctx, section(ctx, KTA_SEC_COMPACTION), compaction_shape(ctx->P).words);
        if (rc != KTA_OK) return rc;
        if (ctx->cd) {
            rc = clear_kept(ctx);
            if (rc != KTA_OK) return rc;
        }
        ctx->comp_saved_seq = ctx->next_seq;
        ctx->next_seq = 0;
    } else {
        ctx->next_seq = ctx->comp_saved_seq;
    }
    ctx->comp_replay = want;
    return KTA_OK;
}

int kta_get_compaction(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return get_section(ctx, KTA_SEC_COMPACTION, out, n_u64); }

int kta_compaction_info(kta_ctx *ctx, uint64_t out[6])
{
    if (!ctx || !out) return KTA_ERR_INVALID;
    if (!ctx->comp) return section_off(ctx, KTA_SEC_COMPACTION);
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    uint64_t st[3];
    int rc = read_words(ctx, ctx->d_comp_stats.get(), st, 3);
    uint32_t plan[3];
    kta::compaction_lds_plan(ctx->P, plan);
    out[0] = st[0], out[1] = ctx->comp_launches, out[2] = ctx->comp_workgroups, out[3] = st[1], out[4] = plan[0], out[5] = 0;
    return rc;
}

// ---- compact,delete what-if (kta_compact_delete.h holds the rule; the kernels are kta_compaction.hip's and kta_segments.hip's) ----

static_assert(kta::kCompactDeleteMaxPartitions == (kta::kSegmentsMaxPartitions < kta::kCompactionMaxPartitions ? kta::kSegmentsMaxPartitions
                                                                                                               : kta::kCompactionMaxPartitions),
              "the smaller of the two passes' bounds");

int kta_compact_delete_max_partitions(void) { return (int)kta::kCompactDeleteMaxPartitions; }

int kta_set_compact_delete(kta_ctx *ctx, int on)
{
    if (!ctx) return KTA_ERR_INVALID;
    if (!ctx->comp) return section_off(ctx, KTA_SEC_COMPACTION);
    if (!ctx->seg) return section_off(ctx, KTA_RV_SEGMENTS);
    if (ctx->handed_records || ctx->fill_n || ctx->comp_replay)
        return fail(ctx, KTA_ERR_INVALID, "kta_set_compact_delete: the context has been handed records since kta_create / kta_reset");
    if (ctx->P > kta::kCompactDeleteMaxPartitions)
        return fail(ctx, KTA_ERR_INVALID, "kta_set_compact_delete admits at most " + std::to_string(kta::kCompactDeleteMaxPartitions) + " partitions");
    if (!on) {
        ctx->cd = false;
        return KTA_OK;
    }
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    const Section s = section(ctx, KTA_SEC_KEPT);   // (live only: the one vector)
    int rc = ctx->d_kept.size() != s.shape.words ? alloc_section(ctx, s, s.shape.words) : KTA_OK;
    if (rc != KTA_OK) return rc;
    if (!ctx->d_cd_stats) KTA_HIP(ctx, ctx->d_cd_stats.alloc(4));
    rc = clear_kept(ctx);
    if (rc != KTA_OK) return rc;
    ctx->cd = true;
    return KTA_OK;
}

int kta_get_compact_delete(kta_ctx *ctx, uint64_t *out, size_t n_u64) { return get_section(ctx, KTA_SEC_KEPT, out, n_u64); }

int kta_compact_delete_info(kta_ctx *ctx, uint64_t out[4])
{
    if (!ctx || !out) return KTA_ERR_INVALID;
    if (!ctx->cd) return section_off(ctx, KTA_SEC_KEPT);
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    int rc = kta_flush(ctx);
    if (rc != KTA_OK) return rc;
    uint64_t st[4];
    rc = read_words(ctx, ctx->d_cd_stats.get(), st, 4);
    out[0] = ctx->cd_launches, out[1] = ctx->cd_chunks, out[2] = st[0], out[3] = ctx->d_cd_cls.size();
    return rc;
}

int kta_compact_delete_whatif(const uint64_t *seg_vec, const uint64_t *kept_vec, const uint64_t *comp_vec, uint32_t P, uint32_t M, int64_t now_ms,
                              int64_t retention_ms, int64_t retention_bytes, uint64_t *out, size_t n_u64)
{
    if (!seg_vec || !kept_vec || !comp_vec || !out || !kta::segments_config_ok(1, M, P) || P > kta::kCompactDeleteMaxPartitions ||
        n_u64 != ((size_t)P + 1) * KTA_COMPACT_DELETE_WORDS)
        return KTA_ERR_INVALID;
    if (retention_ms < -1 || retention_bytes < -1) return KTA_ERR_INVALID;
    const uint64_t *g = seg_vec + kta::segments_globals_at(P, M);
    if (g[kta::kSegGlobalM] != M || !kta::segments_config_ok(g[kta::kSegGlobalS], M, P)) return KTA_ERR_INVALID;   // not a vector of this shape
    if (!kta::compact_delete_identities_hold(seg_vec, kept_vec, comp_vec, P, M)) return KTA_ERR_INVALID;   // the replay did not match the first pass
    kta::compact_delete_whatif(seg_vec, kept_vec, P, M, now_ms, retention_ms, retention_bytes, out);
    return KTA_OK;
}

// ---- record filter (kta_filter.h holds the rules, kta_filter.hip the kernels) ------------------------------------------

int kta_set_filter(kta_ctx *ctx, int64_t from_ms, int64_t to_ms, const uint32_t *partition_bitmap, uint32_t n_words)
{
    if (!ctx) return KTA_ERR_INVALID;
    if (from_ms >= to_ms) return fail(ctx, KTA_ERR_INVALID, "kta_set_filter: from_ms must be below to_ms");
    if (partition_bitmap && n_words == 0) return fail(ctx, KTA_ERR_INVALID, "kta_set_filter: a partition bitmap of no words");
    if (ctx->handed_records || ctx->fill_n)
        return fail(ctx, KTA_ERR_INVALID, "kta_set_filter: the context has been handed records since kta_create / kta_reset");
    const uint32_t words = kta::filter_bitmap_words(ctx->P);
    std::vector<uint32_t> set(words, 0u);
    if (partition_bitmap) {
        if ((size_t)words * 4 > kta::kFilterBitmapBytes)
            return fail(ctx, KTA_ERR_INVALID, "kta_set_filter: a partition set needs P <= " + std::to_string(kta::kFilterBitmapBytes * 8u));
        for (uint32_t w = 0; w < n_words; w++) {
            const uint32_t valid = w >= words ? 0u : (w + 1 == words && (ctx->P & 31u)) ? (1u << (ctx->P & 31u)) - 1u : 0xFFFFFFFFu;
            if (partition_bitmap[w] & ~valid) return fail(ctx, KTA_ERR_INVALID, "kta_set_filter: the bitmap names a partition at or beyond P");
            if (w < words) set[w] = partition_bitmap[w];
        }
    }
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));
    if (!ctx->d_filter_stats) {
        KTA_HIP(ctx, ctx->d_filter_stats.alloc(3));
        KTA_HIP(ctx, hipMemset(ctx->d_filter_stats.get(), 0, 3 * sizeof(uint64_t)));
    }
    if (partition_bitmap) {
        if (!ctx->d_filter_bitmap) KTA_HIP(ctx, ctx->d_filter_bitmap.alloc(words));
        KTA_HIP(ctx, hipMemcpy(ctx->d_filter_bitmap.get(), set.data(), (size_t)words * 4, hipMemcpyHostToDevice));
    }
    ctx->filter_spec = kta::FilterSpec{from_ms, to_ms, ctx->P, partition_bitmap ? 1u : 0u};
    ctx->filter = partition_bitmap || kta::filter_timed(ctx->filter_spec);   // no bound and no set: no filter
    return KTA_OK;
}

int kta_set_filter_slice(kta_ctx *ctx, uint64_t records)
{
    if (!ctx) return KTA_ERR_INVALID;
    if (records == 0) records = kta::kFilterSlice;
    if (records % KTA_TILE_RECORDS || records > kta::kFilterSlice)
        return fail(ctx, KTA_ERR_INVALID, "kta_set_filter_slice: a multiple of 1024 records, at most 2^26");
    ctx->filter_slice = records;
    return KTA_OK;
}

int kta_filter_info(kta_ctx *ctx, uint64_t out[6])
{
    if (!ctx || !out) return KTA_ERR_INVALID;
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    int rc = kta_flush(ctx);
    if (rc != KTA_OK) return rc;
    uint64_t st[3] = {0, 0, 0};
    if (ctx->d_filter_stats) rc = read_words(ctx, ctx->d_filter_stats.get(), st, 3);
    out[0] = ctx->filter_seen, out[1] = ctx->filter_passed, out[2] = st[0], out[3] = st[1], out[4] = st[2], out[5] = ctx->filter_slices;
    return rc;
}

int kta_filter_host(const int32_t *partition, const int64_t *ts_ms, uint64_t n, uint32_t n_partitions, int64_t from_ms, int64_t to_ms,
                    const uint32_t *partition_bitmap, uint32_t n_words, uint64_t *indices_out, uint64_t *n_out)
{
    if ((n && (!partition || !ts_ms)) || !n_out || from_ms >= to_ms) return KTA_ERR_INVALID;
    if (partition_bitmap && n_words < kta::filter_bitmap_words(n_partitions)) return KTA_ERR_INVALID;
    const kta::FilterSpec f{from_ms, to_ms, n_partitions, partition_bitmap ? 1u : 0u};
    uint64_t m = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (!kta::filter_record_passes(f, partition_bitmap, partition[i], ts_ms[i])) continue;
        if (indices_out) indices_out[m] = i;
        m++;
    }
    *n_out = m;
    return KTA_OK;
}

int kta_filter_tile_host(uint32_t n_partitions, int64_t from_ms, int64_t to_ms, int has_partition_set, const kta_tile_hdr *hdr,
                         const kta_tile_sum *sum, int whole)
{
    if (!hdr || !sum || from_ms >= to_ms) return KTA_ERR_INVALID;
    const kta::FilterSpec f{from_ms, to_ms, n_partitions, has_partition_set ? 1u : 0u};
    return (int)kta::filter_tile_decide(f, *hdr, *sum, whole != 0);
}

namespace {

// a^-1 mod 2^32 of an odd a, by Newton's iteration (each step doubles the correct low bits: 3, 6, 12, 24, 48)
constexpr uint32_t inverse_mod_2_32(uint32_t a)
{
    uint32_t v = a;
    for (int i = 0; i < 5; i++) v *= 2u - a * v;
    return v;
}
constexpr uint32_t kFmixInv1 = inverse_mod_2_32(0x85ebca6bu), kFmixInv2 = inverse_mod_2_32(0xc2b2ae35u);
static_assert(kFmixInv1 * 0x85ebca6bu == 1u && kFmixInv2 * 0xc2b2ae35u == 1u, "the inverses of fmix32's multipliers");

uint32_t fmix32_inverse(uint32_t x)
{
    x ^= x >> 16;
    x *= kFmixInv2;
    x ^= (x >> 13) ^ (x >> 26);
    x *= kFmixInv1;
    x ^= x >> 16;
    return x;
}

// the cell of x in `row` and the 22 bits the cell index leaves
void hot_cell_of(uint32_t x, int row, uint32_t *cell, uint32_t *y)
{
    if (row == 0) *cell = x & 1023u, *y = x >> 10;
    else *cell = (x >> 10) & 1023u, *y = (x & 1023u) | ((x >> 20) << 10);
}

} // namespace

int kta_hot_keys_recover(const uint64_t *vec, uint32_t max_out, kta_hot_key *entries, uint32_t *n_out, uint64_t *keyed_out)
{
    if (!vec || !n_out || (max_out && !entries) || max_out > KTA_HOT_ROWS * KTA_HOT_CELLS) return KTA_ERR_INVALID;
    *n_out = 0;
    uint64_t keyed = 0;
    for (uint32_t i = 0; i < KTA_HOT_ROWS * KTA_HOT_CELLS; i++) {
        const uint64_t *a = vec + (size_t)i * KTA_HOT_WORDS;
        if (a[0] >= (1ull << 54)) return KTA_ERR_INVALID;
        for (uint32_t b = 1; b < KTA_HOT_WORDS; b++)
            if (a[b] > a[0]) return KTA_ERR_INVALID;
        if (i < KTA_HOT_CELLS) keyed += a[0];
    }
    if (keyed_out) *keyed_out = keyed;
    struct Cand { uint32_t x, hash; uint64_t upper, lower; };
    std::vector<Cand> found;
    for (uint32_t i = 0; i < KTA_HOT_ROWS * KTA_HOT_CELLS; i++) {
        const uint64_t *a = vec + (size_t)i * KTA_HOT_WORDS;
        const uint64_t T = a[0];
        if (T == 0) continue;
        uint32_t y = 0;
        for (uint32_t b = 0; b < KTA_HOT_WORDS - 1; b++)
            if (2 * a[1 + b] > T) y |= 1u << b;
        const uint32_t cell = i % KTA_HOT_CELLS;
        const uint32_t x = i < KTA_HOT_CELLS ? (cell | (y << 10)) : ((y & 1023u) | (cell << 10) | ((y >> 10) << 20));
        uint64_t upper = UINT64_MAX, lower = 0;
        for (int row = 0; row < KTA_HOT_ROWS; row++) {
            uint32_t rc, ry;
            hot_cell_of(x, row, &rc, &ry);
            const uint64_t *r = vec + ((size_t)row * KTA_HOT_CELLS + rc) * KTA_HOT_WORDS;
            const uint64_t Tr = r[0];
            uint64_t least = Tr, deficit = 0;
            for (uint32_t b = 0; b < KTA_HOT_WORDS - 1; b++) {
                const uint64_t agree = ((ry >> b) & 1u) ? r[1 + b] : Tr - r[1 + b];
                least = std::min(least, agree);
                deficit += Tr - agree;
            }
            upper = std::min(upper, least);
            lower = std::max(lower, deficit >= Tr ? 0 : Tr - deficit);
        }
        if (upper * 512 < keyed) continue;
        found.push_back(Cand{x, fmix32_inverse(x), upper, lower});
    }
    std::sort(found.begin(), found.end(), [](const Cand &p, const Cand &q) {
        return p.upper != q.upper ? p.upper > q.upper : p.hash < q.hash;
    });
    found.erase(std::unique(found.begin(), found.end(), [](const Cand &p, const Cand &q) { return p.x == q.x; }), found.end());
    const uint32_t n = (uint32_t)std::min<size_t>(found.size(), max_out);
    for (uint32_t k = 0; k < n; k++) entries[k] = kta_hot_key{found[k].hash, 0u, found[k].upper, found[k].lower};
    *n_out = n;
    return KTA_OK;
}

namespace {

// Ertl 2017, Algorithm 6 (the improved raw estimator) for m = 4096 registers and q = 32 - 12 = 20 hash bits below the
// register index, from the register histogram C[0 .. q + 1].
constexpr int kSketchQ = 32 - KTA_SKETCH_LOG2;

double hll_sigma(double x)
{
    if (x == 1.0) return INFINITY;
    double y = 1.0, z = x, zp;
    do {
        x *= x;
        zp = z;
        z += x * y;
        y += y;
    } while (z != zp);
    return z;
}

double hll_tau(double x)
{
    if (x == 0.0 || x == 1.0) return 0.0;
    double y = 1.0, z = 1.0 - x, zp;
    do {
        x = sqrt(x);
        zp = z;
        y *= 0.5;
        z -= (1.0 - x) * (1.0 - x) * y;
    } while (z != zp);
    return z / 3.0;
}

double hll_estimate(const uint64_t (&C)[kSketchQ + 2])
{
    const double m = (double)KTA_SKETCH_REGISTERS;
    double z = m * hll_tau(1.0 - (double)C[kSketchQ + 1] / m);
    for (int k = kSketchQ; k >= 1; k--) z = 0.5 * (z + (double)C[k]);
    z += m * hll_sigma((double)C[0] / m);
    return m * m / (2.0 * log(2.0)) / z;
}

} // namespace

int kta_key_sketch_estimate(const uint64_t *vec, uint32_t P, double *per_partition, double *topic)
{
    if (!vec || P == 0 || P > KTA_SKETCH_MAX_PARTITIONS) return KTA_ERR_INVALID;
    const size_t words = (size_t)P * KTA_SKETCH_REGISTERS;
    for (size_t i = 0; i < words; i++)
        if (vec[i] > (uint64_t)kSketchQ + 1) return KTA_ERR_INVALID;
    std::vector<uint64_t> all(KTA_SKETCH_REGISTERS, 0);
    for (uint32_t p = 0; p < P; p++) {
        const uint64_t *r = vec + (size_t)p * KTA_SKETCH_REGISTERS;
        uint64_t C[kSketchQ + 2] = {};
        for (uint32_t j = 0; j < KTA_SKETCH_REGISTERS; j++) {
            C[r[j]]++;
            all[j] = std::max(all[j], r[j]);
        }
        if (per_partition) per_partition[p] = hll_estimate(C);
    }
    if (topic) {
        uint64_t C[kSketchQ + 2] = {};
        for (uint32_t j = 0; j < KTA_SKETCH_REGISTERS; j++) C[all[j]]++;
        *topic = hll_estimate(C);
    }
    return KTA_OK;
}

static const char *const kNeedsTable =
    "the context keeps the alive set as a bit set: create it with KTA_FLAG_ALIVE_TABLE for sequence-numbered entries";

int kta_export_alive_bitmap(kta_ctx *ctx, void *dst)
{
    if (!ctx || !dst) return KTA_ERR_INVALID;
    if (!ctx->alive) return fail(ctx, KTA_ERR_INVALID, "context was created without count_alive_keys");
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    int rc = kta_flush(ctx);
    if (rc != KTA_OK) return rc;
    const size_t bytes = (size_t)(kta::kAliveSlots / 8);
    if (!ctx->alive_table) {       // the state IS the reference's bit set
        KTA_HIP(ctx, hipMemcpyAsync(dst, ctx->d_bitmap.get(), bytes, hipMemcpyDeviceToHost, ctx->s_compute));
        KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));
        return KTA_OK;
    }
    DeviceBuf<uint32_t> d_bm;   // (released on every return; hipFree waits for the device first)
    KTA_HIP(ctx, d_bm.alloc(bytes / sizeof(uint32_t)));
    const char *const what = "alive bitmap export";
    KTA_HIP_AS(ctx, kta::launch_alive_bitmap(ctx->d_table.get(), kta::kAliveSlots, d_bm.get(), ctx->s_compute), what);
    KTA_HIP_AS(ctx, hipMemcpyAsync(dst, d_bm.get(), bytes, hipMemcpyDeviceToHost, ctx->s_compute), what);
    KTA_HIP_AS(ctx, hipStreamSynchronize(ctx->s_compute), what);
    return KTA_OK;
}

int kta_alive_table(kta_ctx *ctx, void **device_ptr, size_t *n_u64)
{
    if (!ctx || !device_ptr || !n_u64) return KTA_ERR_INVALID;
    if (!ctx->alive) return fail(ctx, KTA_ERR_INVALID, "context was created without count_alive_keys");
    if (!ctx->alive_table) return fail(ctx, KTA_ERR_INVALID, kNeedsTable);
    *device_ptr = ctx->d_table.get();
    *n_u64 = (size_t)kta::kAliveSlots;
    return KTA_OK;
}

int kta_alive_export_entries(kta_ctx *ctx, void **d_slots, void **d_vals, uint64_t *n)
{
    if (!ctx || !d_slots || !d_vals || !n) return KTA_ERR_INVALID;
    if (!ctx->alive) return fail(ctx, KTA_ERR_INVALID, "context was created without count_alive_keys");
    if (!ctx->alive_table) return fail(ctx, KTA_ERR_INVALID, kNeedsTable);
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    int rc = kta_flush(ctx);
    if (rc != KTA_OK) return rc;
    hipStream_t s = ctx->s_compute;
    if (!ctx->d_exp_count) KTA_HIP(ctx, ctx->d_exp_count.alloc(1));
    uint64_t written = 0;
    KTA_HIP(ctx, kta::launch_alive_count_written(ctx->d_table.get(), kta::kAliveSlots, ctx->d_exp_count.get(), s));
    KTA_HIP(ctx, hipMemcpyAsync(&written, ctx->d_exp_count.get(), sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    KTA_HIP(ctx, hipStreamSynchronize(s));
    if (ctx->d_exp_vals.size() < written) {   // (the stream is idle: both lists go before either comes back)
        const size_t cap = written + written / 8 + 1024;
        ctx->d_exp_slots.reset();
        ctx->d_exp_vals.reset();
        KTA_HIP(ctx, ctx->d_exp_slots.alloc(cap));
        KTA_HIP(ctx, ctx->d_exp_vals.alloc(cap));
    }
    if (written)
        KTA_HIP(ctx, kta::launch_alive_export(ctx->d_table.get(), kta::kAliveSlots, ctx->d_exp_slots.get(), ctx->d_exp_vals.get(),
                                              ctx->d_exp_count.get(), ctx->d_exp_vals.size(), s));
    KTA_HIP(ctx, hipStreamSynchronize(s));
    *d_slots = ctx->d_exp_slots.get();
    *d_vals = ctx->d_exp_vals.get();
    *n = written;
    return KTA_OK;
}

int kta_alive_import_entries(kta_ctx *ctx, const void *d_slots, const void *d_vals, uint64_t n)
{
    if (!ctx || (n && (!d_slots || !d_vals))) return KTA_ERR_INVALID;
    if (!ctx->alive) return fail(ctx, KTA_ERR_INVALID, "context was created without count_alive_keys");
    if (!ctx->alive_table) return fail(ctx, KTA_ERR_INVALID, kNeedsTable);
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    int rc = kta_flush(ctx);
    if (rc != KTA_OK) return rc;
    KTA_HIP(ctx, kta::launch_alive_import(static_cast<const uint32_t *>(d_slots), static_cast<const uint64_t *>(d_vals),
                                          n, ctx->d_table.get(), ctx->d_alive_running.get(), written_list(ctx), ctx->s_compute));
    return KTA_OK;
}

int kta_alive_count_range(kta_ctx *ctx, uint64_t slot_lo, uint64_t slot_hi, uint64_t *count)
{
    if (!ctx || !count || slot_lo > slot_hi || slot_hi > kta::kAliveSlots) return KTA_ERR_INVALID;
    if (!ctx->alive) return fail(ctx, KTA_ERR_INVALID, "context was created without count_alive_keys");
    if (!ctx->alive_table) return fail(ctx, KTA_ERR_INVALID, kNeedsTable);
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    int rc = kta_flush(ctx);
    if (rc != KTA_OK) return rc;
    hipStream_t s = ctx->s_compute;
    if (!ctx->d_exp_count) KTA_HIP(ctx, ctx->d_exp_count.alloc(1));
    KTA_HIP(ctx, kta::launch_alive_count_span(ctx->d_table.get(), slot_lo, slot_hi, ctx->d_exp_count.get(), s));
    KTA_HIP(ctx, hipMemcpyAsync(count, ctx->d_exp_count.get(), sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    KTA_HIP(ctx, hipStreamSynchronize(s));
    return KTA_OK;
}

int kta_alive_table_modified(kta_ctx *ctx)
{
    if (!ctx) return KTA_ERR_INVALID;
    if (!ctx->alive) return fail(ctx, KTA_ERR_INVALID, "context was created without count_alive_keys");
    ctx->running_valid = false;  // the next kta_finish recounts from the table
    ctx->written_valid = false;  // and the exchange sweeps it: somebody else wrote entries
    return KTA_OK;
}

int kta_fnv32_device(kta_ctx *ctx, const uint8_t *key_bytes, const uint32_t *key_off, const int32_t *key_len,
                     uint64_t n, uint64_t n_key_bytes, uint32_t *hash_out)
{
    if (!ctx || !key_off || !key_len || !hash_out) return KTA_ERR_INVALID;
    if (n == 0) return KTA_OK;
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    DeviceBuf<uint8_t> d_kb;
    DeviceBuf<uint32_t> d_off, d_out;
    DeviceBuf<int32_t> d_len;
    const char *const what = "kta_fnv32_device";
    hipStream_t s = ctx->s_compute;
    KTA_HIP_AS(ctx, d_kb.alloc(pad16(n_key_bytes + 16)), what);
    KTA_HIP_AS(ctx, d_off.alloc(n), what);
    KTA_HIP_AS(ctx, d_len.alloc(n), what);
    KTA_HIP_AS(ctx, d_out.alloc(n), what);
    if (n_key_bytes) KTA_HIP_AS(ctx, hipMemcpyAsync(d_kb.get(), key_bytes, n_key_bytes, hipMemcpyHostToDevice, s), what);
    KTA_HIP_AS(ctx, hipMemcpyAsync(d_off.get(), key_off, n * 4, hipMemcpyHostToDevice, s), what);
    KTA_HIP_AS(ctx, hipMemcpyAsync(d_len.get(), key_len, n * 4, hipMemcpyHostToDevice, s), what);
    KTA_HIP_AS(ctx, kta::launch_fnv32(d_kb.get(), d_off.get(), d_len.get(), n, d_out.get(), s), what);
    KTA_HIP_AS(ctx, hipMemcpyAsync(hash_out, d_out.get(), n * 4, hipMemcpyDeviceToHost, s), what);
    KTA_HIP_AS(ctx, hipStreamSynchronize(s), what);
    return KTA_OK;
}

int kta_set_timing(kta_ctx *ctx, int enable)
{
    if (!ctx) return KTA_ERR_INVALID;
    ctx->timing = enable != 0;
    return KTA_OK;
}

int kta_kernel_time_stats(kta_ctx *ctx, float avg_ms[3], uint64_t launches[3])
{
    if (!ctx || !avg_ms || !launches) return KTA_ERR_INVALID;
    KTA_HIP(ctx, hipSetDevice(ctx->device));
    return ctx->timers.stats(ctx, ctx->s_compute, avg_ms, launches);
}

int kta_set_tuning(kta_ctx *ctx, int scan_workgroups, int scan_variant, int alive_workgroups, int alive_variant)
{
    if (!ctx) return KTA_ERR_INVALID;
    if (scan_workgroups < 0 || alive_workgroups < 0) return fail(ctx, KTA_ERR_INVALID, "negative workgroup count");
    ctx->scan_wgs = scan_workgroups;
    ctx->scan_variant = scan_variant;
    ctx->alive_wgs = alive_workgroups;
    ctx->alive_variant = alive_variant;
    return KTA_OK;
}

int kta_set_fuse(kta_ctx *ctx, int enable)
{
    if (!ctx) return KTA_ERR_INVALID;
    ctx->fuse_handlers = enable != 0;
    return KTA_OK;
}

int kta_alive_pass_info(kta_ctx *ctx, uint64_t out[6])
{
    if (!ctx || !out) return KTA_ERR_INVALID;
    // the device's own count (every launch pair's fallback kernel adds what pass 2 handed it): waits for the compute stream
    ctx->info_failed_buckets = 0;
    if (ctx->d_failed_total) {
        KTA_HIP(ctx, hipSetDevice(ctx->device));
        KTA_HIP(ctx, hipMemcpyAsync(&ctx->info_failed_buckets, ctx->d_failed_total.get(), sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->s_compute));
        KTA_HIP(ctx, hipStreamSynchronize(ctx->s_compute));
    }
    out[0] = kta::kAlivePartitionMax;
    out[1] = ctx->info_slices;
    out[2] = ctx->info_fused;
    out[3] = ctx->info_scanned;
    out[4] = ctx->info_failed_buckets;
    out[5] = ctx->fuse_handlers ? 1 : 0;
    return KTA_OK;
}

} // extern "C"

// what kta_internal.h declares for the other translation units of the library
void **kta_internal_ext_slot(kta_ctx *ctx, void (*free_fn)(void *))
{
    ctx->ext_free = free_fn;
    return &ctx->ext_state;
}
void **kta_internal_comm_slot(kta_ctx *ctx, void (*free_fn)(void *))
{
    ctx->comm_free = free_fn;
    return &ctx->comm_state;
}
bool kta_internal_want_keys(kta_ctx *ctx) { return ctx->alive || ctx->sketch || ctx->hot || ctx->part; }
uint32_t kta_internal_partitions(kta_ctx *ctx) { return ctx->P; }
uint64_t *kta_internal_table(kta_ctx *ctx) { return ctx->d_table.get(); }
bool kta_internal_alive_table(kta_ctx *ctx) { return ctx->alive_table; }
bool kta_internal_compaction(kta_ctx *ctx) { return ctx->comp; }
bool kta_internal_blob_pass(kta_ctx *ctx, int kind, kta_internal_pass *out)
{
    switch (kind) {
    case KTA_PASS_RECORD_BATCHES: *out = kta_internal_pass{ctx->rb, ctx->d_rb.get(), nullptr, nullptr, 0}; break;
    case KTA_PASS_PAYLOAD: *out = kta_internal_pass{ctx->pl, ctx->d_pl.get(), nullptr, nullptr, 0}; break;
    case KTA_PASS_HEADER_NAMES: *out = kta_internal_pass{ctx->hn, ctx->d_hn.get(), ctx->d_hn_info.get(), ctx->d_hn_names.get(), 0}; break;
    case KTA_PASS_VALUE_BYTES: *out = kta_internal_pass{ctx->vb, ctx->d_vb.get(), ctx->d_vb_info.get(), nullptr, ctx->vb_variant}; break;
    case KTA_PASS_COMPRESS_WHATIF: *out = kta_internal_pass{ctx->cw, ctx->d_cw.get(), nullptr, nullptr, 0}; break;
    default: *out = kta_internal_pass{false, nullptr, nullptr, nullptr, 0}; break;
    }
    return out->on && !ctx->comp_replay;
}
kta_internal_pass_env kta_internal_blob_pass_env(kta_ctx *ctx)
{
    const bool f = ctx->filter;
    return kta_internal_pass_env{f ? ctx->filter_spec.from_ms : INT64_MIN, f ? ctx->filter_spec.to_ms : INT64_MAX,
                                 f && ctx->filter_spec.parts ? ctx->d_filter_bitmap.get() : nullptr, ctx->cu_count};
}
int kta_internal_section_off(kta_ctx *ctx, int kind) { return section_off(ctx, kind); }
bool kta_internal_written(kta_ctx *ctx, kta::WrittenList *out)
{
    *out = kta::WrittenList{ctx->d_written.get(), ctx->d_written_n.get(), ctx->d_written.size()};
    return ctx->written_valid && ctx->d_written.get();
}
int64_t *kta_internal_running(kta_ctx *ctx) { return ctx->d_alive_running.get(); }
uint64_t kta_internal_take_seq(kta_ctx *ctx, uint64_t n)
{
    const uint64_t base = ctx->next_seq;
    ctx->next_seq += n;
    return base;
}
bool kta_internal_timing(kta_ctx *ctx) { return ctx->timing; }
hipStream_t kta_internal_copy_stream(kta_ctx *ctx) { return ctx->s_copy.get(); }
bool kta_internal_count_alive(kta_ctx *ctx) { return ctx->alive; }
hipStream_t kta_internal_stream(kta_ctx *ctx) { return ctx->s_compute; }
int kta_internal_device(kta_ctx *ctx) { return ctx->device; }
void kta_internal_set_error(kta_ctx *ctx, const char *msg) { ctx->err = msg; }

int kta_internal_prepare_raw(kta_ctx *ctx, const kta_batch *d, uint64_t n)
{
    kta_internal_columns r{};
    int rc = kta_internal_resolve(ctx, d, &r);
    if (rc != KTA_OK || !r.hdr || n == 0) return rc;
    KTA_HIP(ctx, kta::launch_tiles_to_raw(r.partition, r.ts_ms, r.key_len, r.val_len, r.hdr, r.rec0, r.rec0 + n,
                                          r.keyless ? 3u : 1u, false, ctx->s_compute));
    return KTA_OK;
}

int kta_internal_resolve(kta_ctx *ctx, const kta_batch *c, kta_internal_columns *r)
{
    *r = kta_internal_columns{c->partition, c->key_len, c->val_len, c->ts_ms, nullptr, 0, false, 0, nullptr, nullptr, nullptr};
    uint64_t rec0 = 0;
    if (const kta_batch *e = find_allocation(ctx, c->partition, &kta_batch::partition, &rec0)) {
        if (e->partition + rec0 != c->partition) return fail(ctx, KTA_ERR_INVALID, "a view of a tile-compact batch must start at a record");
        if ((c->ts_ms && c->ts_ms != e->ts_ms + rec0) || (c->key_len && c->key_len != e->key_len + rec0) ||
            (c->val_len && c->val_len != e->val_len + rec0))
            return fail(ctx, KTA_ERR_INVALID, "the columns of a view of a tile-compact batch start at different records");
        *r = kta_internal_columns{e->partition, e->key_len, e->val_len, e->ts_ms, e->tile_hdr, rec0, e->key_bytes == nullptr, allocation_rows(*e),
                                  kta::tile_sums_behind(e->tile_hdr, allocation_rows(*e) / KTA_TILE_RECORDS),
                                  kta::tile_marks_behind(e->tile_hdr, allocation_rows(*e) / KTA_TILE_RECORDS),
                                  kta::tile_sizes_behind(e->tile_hdr, allocation_rows(*e) / KTA_TILE_RECORDS)};
        return KTA_OK;
    }
    if (c->layout == KTA_LAYOUT_TILE_COMPACT) {
        if (!c->tile_hdr) return fail(ctx, KTA_ERR_INVALID, "a tile-compact batch needs its tile headers");
        r->hdr = c->tile_hdr;
    } else if (c->layout != KTA_LAYOUT_RAW) {
        return fail(ctx, KTA_ERR_INVALID, "unknown batch layout");
    }
    return KTA_OK;
}

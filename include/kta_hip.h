/*
 * kta_hip.h — C ABI of libkta_hip.so: the MI355X (gfx950) implementation of the
 * per-record metric-accumulation hot path of xenji/kafka-topic-analyzer.
 *
 * This is the drop-in boundary.  Reference interface being replaced (paths under
 * /root/reference):
 *
 *   src/kafka.rs:18-20    trait MetricHandler { fn handle_message(&mut self, m: &BorrowedMessage) }
 *   src/kafka.rs:107-109  dispatch: every handler, every polled message, registration order
 *   src/metric.rs:206-253 impl MetricHandler for MessageMetrics
 *   src/metric.rs:288-305 impl MetricHandler for LogCompactionInMemoryMetrics (-c)
 *   src/metric.rs:104-195 accessors the report reads (main.rs:130-170)
 *   src/metric.rs:282-284 sum_all_alive()
 *
 * A Rust `MetricHandler` shim binds these entry points over FFI (INTEGRATION.md shows
 * the `extern "C"` block): `handle_message` becomes `kta_handle_message` (copies what
 * the borrowed message exposes into pinned struct-of-arrays staging and launches the
 * HIP kernels whenever a batch fills), and the accessors read a `kta_result` obtained
 * from `kta_finish`.  Plain pointers and sizes only; every function returns a status
 * (0 = OK, negative = error) and never throws or aborts across the boundary.
 * There is NO CPU fallback: without a usable gfx950 device `kta_create` fails.
 *
 * Threading: one producer thread per context (the reference's poll loop is single
 * threaded, kafka.rs:92-135).  Internally the context owns two HIP streams (H2D copy,
 * compute) and a ring of pinned staging batches.
 */
#ifndef KTA_HIP_H
#define KTA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KTA_ABI_VERSION 7   /* 7: the opt-in size percentiles (KTA_FLAG_SIZE_QUANTILES, kta_get_size_quantiles, kta_exchange_size_quantiles, kta_size_quantiles_result_vector, kta_merge_size_quantiles, kta_size_quantiles_max_partitions, kta_size_quantiles_info, kta_set_size_quantiles_slice, kta_size_bin, kta_size_bin_bounds, kta_size_quantile, kta_render_size_percentiles; kta_exchange reduces its snapshot), only added entry points and a flag bit; the record filter (kta_set_filter, kta_filter_info, kta_set_filter_slice, kta_filter_host, kta_filter_tile_host, kta_render_filter), only added entry points; the compaction what-if (KTA_FLAG_COMPACTION, kta_compaction_replay, kta_get_compaction, kta_compaction_max_partitions, kta_compaction_info, kta_render_compaction), only added entry points and one flag bit; the opt-in partitioner pass (KTA_FLAG_PARTITIONER, kta_set_repartition, kta_get_partitioner, kta_exchange_partitioner, kta_partitioner_result_vector, kta_merge_partitioner, kta_partitioner_max_partitions, kta_partitioner_info, kta_render_partitioner, kta_murmur2; kta_exchange reduces its snapshot), only added entry points and a flag bit; tile summaries beside the tile headers (kta_tile_sum, kta_batch_tile_summaries, bit 32 of kta_set_tuning's scan_variant), only an added entry point and library-owned storage: kta_tile_hdr and kta_batch are unchanged; the opt-in timestamp order (KTA_FLAG_TS_ORDER, kta_get_ts_order, kta_exchange_ts_order, kta_ts_order_result_vector, kta_merge_ts_order, kta_ts_order_max_partitions, kta_ts_order_info, kta_set_ts_order_chunk, kta_render_ts_order; kta_exchange reduces its snapshot), only added entry points and a flag bit; the opt-in hot keys (KTA_FLAG_HOT_KEYS, kta_get_hot_keys, kta_exchange_hot_keys, kta_hot_keys_result_vector, kta_merge_hot_keys, kta_hot_keys_recover, kta_get_hot_key_exemplars, kta_hot_keys_info, kta_set_hot_flush_rounds, kta_render_hot_keys; kta_exchange reduces its snapshot), only added entry points and a flag bit; the opt-in key sketch (KTA_FLAG_KEY_SKETCH, kta_get_key_sketch, kta_exchange_key_sketch, kta_key_sketch_result_vector, kta_merge_key_sketch, kta_key_sketch_estimate, kta_key_sketch_info, kta_render_distinct_keys; kta_exchange reduces its snapshot), only added entry points and a flag bit; the opt-in timeline (kta_set_timeline, kta_timeline_max_partitions, kta_get_timeline, kta_timeline_vector, kta_exchange_timeline, kta_timeline_result_vector, kta_render_timeline; kta_exchange reduces its snapshot), only added entry points (the version stays 7: no existing layout or call changed); kta_batch.tile_hdr / layout appended to the struct (the tile-compact device layout, kta_tile_hdr: a zero-initialised kta_batch is the raw layout of before), kta_batch_from_raw, kta_batch_to_raw; the analytics vector has a snapshot that kta_exchange reduces (kta_exchange_analytics, kta_analytics_result_vector), kta_decode_analytics, kta_merge_analytics, kta_render_analytics, kta_analytics_max_partitions; a KTA_FLAG_ANALYTICS context with more partitions than the scan's LDS plan admits is refused by kta_create; 6: kta_replay_messages, kta_handle_message_stats, kta_zstd_inflate_host_small (kta_kafka.h); the table state takes the fused pass; kta_kafka_set_variant takes 0, 1, 2, 10, 11 only (the other geometries went in round 5); 5: kta_set_fuse, kta_alive_pass_info; 4: KTA_FLAG_ALIVE_TABLE, the default -c state is the bit set (submission order); 3: kta_comm_* / kta_exchange*, kta_result_vector is a snapshot; 2: kta_kafka_batch_desc.scratch_end */

/* status codes */
#define KTA_OK 0
#define KTA_ERR_INVALID (-1)       /* bad argument / misuse                         */
#define KTA_ERR_HIP (-2)           /* a HIP runtime call failed (see kta_last_error) */
#define KTA_ERR_NOMEM (-3)         /* host or device allocation failed              */
#define KTA_ERR_NO_DEVICE (-4)     /* no usable gfx950 device                        */
#define KTA_ERR_BAD_PARTITION (-5) /* a record's partition id was outside [0, P)     */
#define KTA_ERR_CAPACITY (-6)      /* batch / key-byte capacity exceeded             */
#define KTA_ERR_DIV_BY_ZERO (-7)   /* where the reference panics (metric.rs:135,144,153) */
#define KTA_ERR_COMM (-8)          /* RCCL missing or a collective failed (see kta_last_error) */
#define KTA_ERR_TIMESTAMP_RANGE (-9) /* where the reference panics: a record's ts / 1000 outside chrono's range (metric.rs:210, kafka.rs:104) */

/* chrono 0.4.19 (Cargo.lock:84-85) NaiveDateTime::from_timestamp(secs, 0) — metric.rs:210, kafka.rs:104 —
 * .expect()s a date inside NaiveDate's years [i32::MIN >> 13, i32::MAX >> 13] = [-262144, 262143]:
 * -262144-01-01 00:00:00 .. 262143-12-31 23:59:59 in seconds since the epoch.  A record outside ends the
 * reference ("invalid or out-of-range datetime"); this library counts it like any other and says so at
 * kta_finish / kta_decode_vector (the extrema of the scan tell: one such record moves one of them out). */
#define KTA_CHRONO_MIN_SEC (-8334632851200LL)
#define KTA_CHRONO_MAX_SEC (8210298412799LL)

/* Per-partition counters, in the field order of `struct MessageMetrics`
 * (metric.rs:13-19). */
enum {
    KTA_C_TOTAL = 0,          /* total_messages  metric.rs:13 */
    KTA_C_TOMBSTONES = 1,     /* tombstones      metric.rs:14 */
    KTA_C_ALIVE = 2,          /* alive           metric.rs:15 */
    KTA_C_KEY_NULL = 3,       /* key_null        metric.rs:16 */
    KTA_C_KEY_NON_NULL = 4,   /* key_non_null    metric.rs:17 */
    KTA_C_KEY_SIZE_SUM = 5,   /* key_size_sum    metric.rs:18 */
    KTA_C_VALUE_SIZE_SUM = 6, /* value_size_sum  metric.rs:19 */
    KTA_NCOUNTERS = 7
};

/* The device result vector ("counter vector") is u64[P*7 + KTA_NGLOBALS]:
 * counters[p*7 + c], then KTA_NSUM_GLOBALS SUM-type globals, then four MAX-type
 * globals.  It is the unit that is reduced across GPUs when partitions are sharded:
 * ONE all-reduce SUM over the first P*7 + KTA_NSUM_GLOBALS words (u64 wrap-around ==
 * i64 wrap-around) and ONE all-reduce MAX (signed i64) over the last four.  Minima are
 * stored bit-complemented (~x is an order-reversing bijection on i64 without overflow),
 * so that every extremum is a MAX. */
enum {
    KTA_G_BAD_PARTITION = 0, /* SUM: records whose partition id was out of range (ignored)      */
    KTA_G_ALIVE_KEYS = 1,    /* SUM: alive keys of this context's table (kta_finish); in an exchange, of the
                                hash range this rank owns — disjoint ranges, so the SUM is the job's count */
    KTA_G_RECORDS = 2,       /* SUM: records scanned (== overall_count, metric.rs:25)            */
    KTA_G_RESERVED = 3,      /* SUM: reserved, zero                                              */
    KTA_NSUM_GLOBALS = 4,
    KTA_G_NOT_MIN_TS_MS = 4, /* MAX: ~min(ts_ms) (i64); ~INT64_MAX when no record seen; a raw
                                timestamp of -1 (not available) was mapped to 0 first          */
    KTA_G_MAX_TS_MS = 5,     /* MAX: max(ts_ms), INT64_MIN when no record seen                   */
    KTA_G_NOT_SMALLEST = 6,  /* MAX: ~(size of the smallest non-tombstone); ~INT64_MAX if none   */
    KTA_G_LARGEST = 7,       /* MAX: size of the largest non-tombstone, 0 if none (metric.rs:41) */
    KTA_NGLOBALS = 8
};

typedef struct kta_ctx kta_ctx;

typedef struct kta_config {
    int32_t device_id;           /* HIP device ordinal                                        */
    int32_t n_partitions;        /* P: partition ids are dense in [0, P) (Kafka's are)         */
    int32_t count_alive_keys;    /* 1 == the reference's -c/--count-alive-keys (main.rs:77-80) */
    int32_t n_staging;           /* pinned staging batches in the ring; 0 -> 2                */
    uint64_t batch_capacity;     /* records per staging batch; 0 -> 1<<22                     */
    uint64_t key_bytes_capacity; /* key bytes per staging batch; 0 -> 64 * batch_capacity;
                                    must be < 4 GiB (key_off is u32, batch-local)             */
    uint32_t flags;              /* KTA_FLAG_*                                                */
    uint32_t reserved;           /* 0                                                         */
} kta_config;

/* Additive analytics (NOT in the reference, never printed by the reference report): log2
 * histograms of key and value sizes and per-partition timestamp / message-size extrema,
 * accumulated by the same scan kernel in extra LDS arrays.  Opt-in: costs LDS, not bandwidth.
 * The scan keeps [P][4] extrema in LDS, so P is bounded (kta_analytics_max_partitions); with -c the
 * batch takes two passes (scan, then the alive-key pass): the fused pass has no LDS room for them. */
#define KTA_FLAG_ANALYTICS 1u
/* The staging batches of kta_batch_acquire carry a `seq` column (with count_alive_keys): the producer writes
 * every record's GLOBAL consumption index, kta_batch_submit's base_seq is ignored.  For a rank of a
 * partition-sharded run, whose records are not consecutive in the topic's consumption order. */
#define KTA_FLAG_SEQ_COLUMN 2u
/* How a -c context keeps the alive set (the reference: one BitSet, metric.rs:262-264):
 *   default               the reference's own bit set, 2^32 bits = 512 MiB.  Batches are applied IN SUBMISSION
 *                         ORDER (what the reference does with the messages it polls); base_seq is not looked at.
 *   KTA_FLAG_ALIVE_TABLE  a last-writer table u64[2^32] = 32 GiB of ((seq + 1) << 1 | alive): batches, shards and
 *                         ranks may arrive in any order, the largest GLOBAL sequence number of a slot wins.  What a
 *                         rank of a sharded run needs (kta_comm_create with nranks > 1, kta_alive_table,
 *                         kta_alive_export_entries / import_entries / count_range).  Implied by KTA_FLAG_SEQ_COLUMN.
 *                         A seq column has to ascend inside each batch to take the fast path (checked on the device;
 *                         other batches are still exact, through the single-kernel update). */
#define KTA_FLAG_ALIVE_TABLE 4u
#define KTA_HIST_BUCKETS 34 /* [0] None, [1] length 0, [2+k] 2^k <= length < 2^(k+1), k = 0..31 */

typedef struct kta_analytics {
    uint64_t key_size_hist[KTA_HIST_BUCKETS];
    uint64_t value_size_hist[KTA_HIST_BUCKETS];
} kta_analytics;

/* Timeline (NOT in the reference, never printed by the reference report; kta_set_timeline): records, tombstones
 * and bytes per time bucket, accumulated by the same scan in LDS.  Configured by origin_ms >= 0, bucket_ms >= 1
 * and 1 <= n_buckets <= KTA_TIMELINE_MAX_BUCKETS, with origin_ms + n_buckets * bucket_ms within int64.  Every
 * record the scan counts (partition in [0, P); the others only go to bad_partition_records) falls into exactly
 * one row:
 *   row 0             "no timestamp"  ts_ms < 0 (a raw -1)
 *   row 1             "before"        0 <= ts_ms < origin_ms
 *   row 2 + k         bucket k        origin_ms + k * bucket_ms <= ts_ms < origin_ms + (k + 1) * bucket_ms
 *   row n_buckets + 2 "after"         ts_ms >= origin_ms + n_buckets * bucket_ms
 * Each row holds KTA_TIMELINE_COLS u64 columns: records, tombstones (val_len == -1), bytes (max(key_len, 0) +
 * max(val_len, 0), the report's P-Bytes summand).  The vector is u64[(n_buckets + 3) * KTA_TIMELINE_COLS],
 * row-major; every word is a SUM, so the vectors of disjoint record sets add element-wise. */
#define KTA_TIMELINE_MAX_BUCKETS 1024
#define KTA_TIMELINE_COLS 3

/* Key sketch (NOT in the reference, never printed by the reference report): one HyperLogLog sketch per partition over
 * the keys, to estimate the distinct keys each partition holds.  Opt-in at kta_create.  For every record the metrics
 * handler counts (partition in [0, P)) whose key is Some (key_len >= 0: the empty key and tombstones included):
 *   h = fnv1a(key)                     the reference's variant, init = mul = 0x811c9dc5 (fnv32.rs:76-101), as -c hashes
 *   x = fmix32(h)                      x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13; x *= 0xc2b2ae35; x ^= x >> 16
 *   j = x >> 20                        the register, 0 .. 4095
 *   w = x << 12                        the other 20 bits, left-aligned
 *   rho = w == 0 ? 21 : clz32(w) + 1   1 .. 21
 *   M[p][j] = max(M[p][j], rho)        0: no key seen
 * Null keys, partitions outside [0, P) and records handed only to the alive-key handler (which == 2) are skipped.  The
 * registers are maxima: exact, independent of order and batching, and they reduce across GPUs with MAX.
 * The host-side vector is u64[P * KTA_SKETCH_REGISTERS], word p * 4096 + j, one register per word (the collectives
 * reduce 8-byte words).  It counts distinct 32-bit key HASHES, as -c counts alive keys by hash slot: at 10^8 keys
 * visibly fewer than the distinct keys (about 1.2 % fewer).  The estimate (kta_key_sketch_estimate) has a standard
 * error of 1.04 / sqrt(4096), about 1.6 %.  kta_create refuses the flag above KTA_SKETCH_MAX_PARTITIONS partitions. */
#define KTA_FLAG_KEY_SKETCH 8u
#define KTA_SKETCH_LOG2 12
#define KTA_SKETCH_REGISTERS (1u << KTA_SKETCH_LOG2)
#define KTA_SKETCH_MAX_PARTITIONS 16384   /* 512 MiB of u64 snapshot */

/* Hot keys (NOT in the reference, never printed by the reference report): a topic-wide sketch that names the keys
 * holding the largest shares of the keyed records.  Opt-in at kta_create.  The vector is
 * u64[KTA_HOT_ROWS][KTA_HOT_CELLS][KTA_HOT_WORDS] (47 104 words, 368 KiB), every word a SUM, so the vectors of disjoint
 * record sets add word by word and the sketch depends on no order, batching or sharding.  For every record the metrics
 * handler counts (partition in [0, P)) whose key is Some (key_len >= 0: the empty key and tombstones included; the key
 * sketch's records), with h = fnv1a(key) and x = fmix32(h) as above KTA_FLAG_KEY_SKETCH:
 *   row 0: cell c0 = x & 1023,          rest y0 = x >> 10
 *   row 1: cell c1 = (x >> 10) & 1023,  rest y1 = (x & 1023) | ((x >> 20) << 10)
 * and in each row r the record adds 1 to word 0 of cell c_r (the cell's total T) and, for every set bit b of the 22-bit
 * y_r, 1 to word 1 + b.  The cell index supplies ten bits of x and the 22 bit counters the others; fmix32 is a bijection,
 * so x names h.
 * Readout (kta_hot_keys_recover: host only, deterministic).  For every cell with T > 0 the candidate is the x put
 * together from the cell index and the bits b with 2 * count_b > T.  For a candidate, in each of its two rows,
 * agree_b = count_b where its bit b is set, else T - count_b.  Then
 *   upper U = min over both rows of min(T, min_b agree_b)
 *   lower L = max(0, max over both rows of T - sum_b (T - agree_b))
 * and L <= (records of the hash) <= U whatever the data: every record of the hash agrees in every bit, every other
 * record of the cell disagrees in at least one.  A candidate is reported when U * 512 >= keyed, keyed = the sum of row
 * 0's totals; candidates are de-duplicated by x, ordered by U descending, then hash ascending, and cut at the caller's
 * maximum.  The reported hash is h = the inverse of fmix32 at x.  A key below 1/512 of the keyed records is not
 * promised; two keys of one 32-bit hash are one key here, as for -c.
 * Exemplars: a table of [KTA_HOT_ROWS][KTA_HOT_CELLS] kta_hot_exemplar slots on the device keeps, best effort, the bytes
 * (at most KTA_HOT_EXEMPLAR_BYTES) of one record's key per cell whose hash was the cell's candidate when a launch began.
 * A valid slot always holds one record's key whose hash is the slot's `hash`.  Counts never depend on exemplars, and
 * collectives do not move them. */
#define KTA_FLAG_HOT_KEYS 16u
#define KTA_HOT_ROWS 2
#define KTA_HOT_CELLS 1024
#define KTA_HOT_WORDS 23
#define KTA_HOT_VECTOR_WORDS (KTA_HOT_ROWS * KTA_HOT_CELLS * KTA_HOT_WORDS)
#define KTA_HOT_EXEMPLAR_BYTES 32
#define KTA_HOT_MAX_REPORTED 64
typedef struct kta_hot_exemplar {
    uint32_t hash;      /* fnv1a of the key */
    uint32_t key_len;   /* the key's own length; bytes holds its first min(key_len, 32) */
    uint32_t valid;     /* 0: the slot is empty */
    uint32_t pad;
    uint8_t bytes[KTA_HOT_EXEMPLAR_BYTES];
} kta_hot_exemplar;
typedef struct kta_hot_key {
    uint32_t hash;      /* fnv1a of the key(s) */
    uint32_t pad;
    uint64_t upper;     /* records of the hash, at most */
    uint64_t lower;     /* records of the hash, at least */
} kta_hot_key;

/* Timestamp order (NOT in the reference, never printed by the reference report): how out of order a topic's timestamps
 * are, per partition — exact, every word an integer.  Opt-in at kta_create.  A context created with KTA_FLAG_TS_ORDER
 * keeps a running maximum hi[p] per partition, initially "none".  Records are taken in consumption order:
 *   - batches in the order they were submitted to the context;
 *   - records by their index inside a batch.
 * A seq column and base_seq are not looked at.  A record that the metrics handler counts (which & 1, partition in
 * [0, P)) and whose ts_ms >= 0 is TIMESTAMPED.  Any negative timestamp counts as "not available", as the timeline
 * treats it.  A timestamped record of partition p is handled like this:
 *   timed += 1
 *   if hi[p] is set and hi[p] > ts:            late: older than something its partition delivered before it
 *       d = hi[p] - ts                         1 <= d < 2^63
 *       late[p] += 1;  late_ms_sum[p] += d     the sum wraps modulo 2^64
 *       max_late_ms[p] = max(max_late_ms[p], d)
 *       hist[63 - clz64(d)] += 1               floor(log2 d), 0..62
 *   else:
 *       hi[p] = ts                             an equal timestamp is in order
 * Records with a negative timestamp, records with a partition outside [0, P) and records handed only to the alive-key
 * handler (which == 2) touch nothing.
 * The result vector is u64[3 P + 64]: [P][2] = late, late_ms_sum; then hist[63]; then timed — all of these SUM words —;
 * then max_late_ms[P], MAX words that are never negative.  That is a SUM prefix of 2 P + 64 words and a MAX suffix of P
 * words.  hi[p] is device state of the context and not part of the vector; kta_reset clears the vector and hi.
 * Two such vectors merge exactly (SUM / MAX) when every partition's records went through ONE context in order: how
 * kta.gpus=N and bench.py --gpus N shard (p on rank p % N).  kta_create refuses the flag above
 * kta_ts_order_max_partitions() partitions. */
#define KTA_FLAG_TS_ORDER 32u
#define KTA_TS_ORDER_HIST 63   /* hist[k]: late by 2^k <= d < 2^(k+1) ms */

/* Partitioner (NOT in the reference, never printed by the reference report): is the topic keyed the way Kafka's default
 * partitioner keys it, and how would its keyed records and bytes spread over Q partitions — exact, every word an
 * integer.  Opt-in at kta_create.  The pass looks at every record that the metrics handler counts (which & 1, partition
 * in [0, P)) and whose key is Some (key_len >= 0): the empty key and tombstones included — the key sketch's records.
 * For each such record of partition p:
 *   h = murmur2(key)          Kafka's org.apache.kafka.common.utils.Utils.murmur2: seed 0x9747b28c, m = 0x5bd1e995, r = 24,
 *                             little-endian 4-byte words, the 1..3 tail bytes as there, final h ^= h>>13; h *= m; h ^= h>>15
 *   t = h & 0x7fffffff        Utils.toPositive (NOT abs)
 *   checked[p] += 1
 *   placed[p]  += (t % P == p)                     the record lies where the Java default partitioner puts its key
 *   target_records[t % Q] += 1
 *   target_bytes[t % Q]   += key_len + max(val_len, 0)
 * Q is the what-if partition count: P unless kta_set_repartition set another; kta_reset keeps it.
 * Records with a null key, records with a partition outside [0, P) and records handed only to the alive-key handler
 * (which == 2) touch nothing.
 * The result vector is u64[2 P + 2 Q]: word 2p is checked[p], word 2p + 1 placed[p]; word 2P + 2q is target_records[q],
 * word 2P + 2q + 1 target_bytes[q].  Every word is a SUM: the vectors of disjoint record sets add word by word, so the
 * result is exact and independent of order, batching and sharding.  checked[p] equals the counter vector's
 * key_non_null[p].  murmur2 of "21" is -973932308, of "foobar" -790332482, of "abc" 479470107, of the empty key 275646681
 * (Kafka's UtilsTest).  kta_create refuses the flag above kta_partitioner_max_partitions() partitions, and
 * kta_set_repartition a Q above it. */
#define KTA_FLAG_PARTITIONER 0x40u   /* 64: bit 6 */

/* Compaction what-if (NOT in the reference, never printed by the reference report): the records and bytes that log
 * compaction would keep, per partition — exact, every word an integer.  Opt-in at kta_create.  The flag needs
 * count_alive_keys (KTA_ERR_INVALID with a message naming the flag otherwise) and implies KTA_FLAG_ALIVE_TABLE, as
 * KTA_FLAG_SEQ_COLUMN does; kta_create refuses it above kta_compaction_max_partitions() partitions (at least 4096: the
 * pass keeps 32 B per partition in LDS), and kta_comm_create with nranks > 1 refuses such a context (after kta_exchange
 * only the owner of a hash range holds the merged entries).
 * The FIRST PASS is unchanged: the context is an ordinary -c context in the table state, every hash slot of which holds
 * ((seq + 1) << 1) | alive of its last writer.  A record survives compaction exactly when the value it would write is the
 * value its slot holds, so one more pass over the same batches answers the question.
 * REPLAY MODE (kta_compaction_replay).  Turning it on flushes the staged messages in the mode they were staged in, zeroes
 * the compaction vector, saves the context's next sequence number and sets it to 0, and sets the mode; turning it off
 * flushes what the replay staged and restores the sequence number.  While it is on, EVERY submission path — the staging
 * ring behind kta_batch_submit / kta_handle_message / kta_replay_messages, kta_submit_device[_ex] whatever `which` says,
 * the Kafka decode — hands its batches to the compaction pass and to nothing else, behind the record filter: a filtered
 * context replays the passing records with the sequence numbers they kept.  The replay does not touch the counter vector,
 * the alive table and its running count, or any other opt-in vector.  kta_reset zeroes the vector and turns the mode off.
 * The caller replays the same records with the same sequence numbers it submitted the first time: same base_seq, same seq
 * column, or the same order through the paths that number records themselves.
 * For every record shown during replay, with s its sequence number (seq[i] if the batch has the column, else
 * base_seq + i), h = fnv1a(key) (the -c hash) and v = ((s + 1) << 1) | (val_len >= 0):
 *   key_len < 0       unkeyed += 1, nothing else (compaction goes by key)
 *   table[h] == v     the record SURVIVES:
 *                       partition p in [0, P), val_len >= 0:  live_records[p] += 1, live_key_bytes[p] += key_len,
 *                                                             live_value_bytes[p] += val_len
 *                       partition p in [0, P), val_len < 0:   tombstone_records[p] += 1, tombstone_key_bytes[p] += key_len
 *                                                             (a tombstone the cleaner keeps until delete.retention.ms)
 *                       partition outside [0, P):             live_outside += 1 if val_len >= 0, else tombstones_outside += 1
 *   table[h] >  v     superseded: adds nothing
 *   table[h] <  v     (0 included) unknown += 1: the table never saw this record, the replay does not match the first pass
 * and every record shown adds 1 to replayed.
 * The result vector is u64[5 P + 6], every word a SUM: word 5p + k is live_records, live_key_bytes, live_value_bytes,
 * tombstone_records, tombstone_key_bytes of partition p; then replayed, unkeyed, unknown, live_outside,
 * tombstones_outside and one reserved word that is 0.
 * After a replay of everything the first pass was handed:
 *   sum of live_records[p] + live_outside == alive keys (the context's running count, what kta_finish reports);
 *   unknown == 0;
 *   live_records[p] + tombstone_records[p] <= key_non_null[p].
 * Caveats.  As with -c, two keys of one 32-bit hash are one key.  The slot is topic-wide, as in the reference: a key
 * written to several partitions survives once here and once per partition in Kafka — exact for a topic in which every key
 * lives in one partition, which the partitioner pass checks.  Two records with one sequence number and one hash are a
 * caller's error: both survive. */
#define KTA_FLAG_COMPACTION (0x80u)  /* 128: bit 7 */
#define KTA_COMPACTION_WORDS 5       /* per partition */
#define KTA_COMPACTION_GLOBALS 6

/* Size percentiles (NOT in the reference, never printed by the reference report): per partition a histogram fine enough
 * to read percentiles of the key, value and message sizes from — exact counts, every word an integer.  Opt-in at
 * kta_create.  For every record that the metrics handler counts (which & 1, partition in [0, P)) three quantities are
 * binned:
 *   K = key_len                      if key_len >= 0
 *   V = val_len                      if val_len >= 0
 *   M = max(key_len, 0) + val_len    if val_len >= 0, as u32: the reference's message_size of a non-tombstone
 *                                    (metric.rs:212-251), the quantity whose smallest and largest the report prints
 * The bin of a u32 v, KTA_SIZE_BINS = 464 of them (csrc/kta_size_bins.h is the code):
 *   v < 32:     bin(v) = v
 *   otherwise:  e = 31 - clz(v),  bin(v) = 32 + 16 (e - 5) + ((v >> (e - 4)) & 15)
 *   lo(b) = b for b < 32, else (16 + (b - 32) % 16) << ((b - 32) / 16 + 1);  hi(b) = lo(b + 1) - 1, hi(463) = 2^32 - 1
 * Sizes below 32 are exact; above that a bin is at most 1/16 of its lower bound wide.
 * The vector is u64[P * 3 * 464 + 8], every word a SUM, so the vectors of disjoint record sets add word by word and the
 * result is exact and independent of order, batching and sharding.  Word (p * 3 + q) * 464 + b holds partition p, quantity
 * q (K = 0, V = 1, M = 2), bin b.  The eight globals behind them: records counted; records with a partition outside
 * [0, P) (they touch nothing else); keyed records; non-tombstones; four words that are zero.
 * Identities with the counter vector of the same records:
 *   sum_b K[p][b] == key_non_null[p];   sum_b V[p][b] == sum_b M[p][b] == alive[p];
 *   global 1 == KTA_G_RECORDS;          global 2 == KTA_G_BAD_PARTITION.
 * Read-off (kta_size_quantile): nearest rank, r = max(1, ceil(num * N / den)) with the product in 128 bits and N the
 * histogram's count; the answer is the first bin whose running count reaches r, as its lo and hi.  The printed value is
 * hi: an upper bound that is exact below 32 and at most 6.25 % high above.
 * Records handed only to the alive-key handler (which == 2) and the batches of a compaction replay touch nothing; a
 * filtered context bins the passing records.  kta_create refuses the flag above kta_size_quantiles_max_partitions()
 * partitions. */
#define KTA_FLAG_SIZE_QUANTILES 0x100U   /* 256: bit 8 */
#define KTA_SIZE_BINS 464
#define KTA_SIZE_QUANTITIES 3            /* K, V, M */
#define KTA_SIZE_GLOBALS 8

/* Record batches (NOT in the reference, which never sees a batch): what the headers of the Kafka v2 record batches say that
 * the raw-log decode delivers (kta_kafka.h: kta_kafka_decode_device, and through it kta_kafka_blob_submit and
 * kta_kafka_consume) — does the producer batch, what does compression buy, what wrote the log and what has the cleaner
 * already removed.  Opt-in at kta_create.  Every word is exact; only the number of producers READ OFF the sketch's registers
 * is an estimate (HyperLogLog, 2^10 registers, standard error 1.04 / sqrt(1024) = 3.25 %).  csrc/kta_record_batches.h is the
 * code of everything below.
 * Per batch, from its descriptor (read after the call's inflate and decode kernels: status is final, payload_end -
 * payload_off the exact inflated size) and from the header bytes partitionLeaderEpoch (12), attributes (21),
 * lastOffsetDelta (23) and producerId (43), big endian at any alignment:
 *   codec 0..4 (none, gzip, Snappy, LZ4, zstd); wire = batch_bytes; recbytes = batch_bytes - 61;
 *   payload = payload_end - payload_off (= recbytes for codec 0); span_ms = clamp(max_ts_ms - base_ts_ms, 0, 2^31 - 1);
 *   extent = max(lastOffsetDelta + 1, n_records); bin(x) = 0 for x == 0, else min(31, 1 + floor(log2 x)).
 * The vector is u64[20 P + 1524]: words [0, 16 P + 500) are SUMS, the rest unsigned MAXIMA.
 *   partition p, 16 words at 16 p: batches, records, wire, payload, compressed batches, recbytes and payload of the
 *     compressed batches, extent, transactional, idempotent (producerId >= 0), LogAppendTime, span_ms, failed, three zeros;
 *   codec c, 100 words at 16 P + 100 c: batches, records, recbytes, payload, then three histograms of 32 bins by
 *     bin(n_records), bin(wire), bin(span_ms);
 *   partition p, 4 maxima at 16 P + 500 + 4 p: the largest n_records, wire, partitionLeaderEpoch + 1 (0: none seen, or
 *     epoch -1) and span_ms;
 *   the producer sketch, 1024 words at 20 P + 500: over the idempotent batches, h = splitmix64(producerId), register
 *     h >> 54, rank 1 + clz(h << 10 | 1 << 9), kept by MAX.
 * A FAILED batch (status != 0: a bad CRC under check.crcs, bad framing, a stream that does not inflate) adds 1 to its
 * partition's `failed` and nothing else anywhere.  A batch whose partition is outside [0, P) is left out entirely (its
 * records land in KTA_G_BAD_PARTITION).  Control batches, batches without records, unknown codecs (5..7) and magic 0/1
 * message sets get no descriptor and are not in these numbers: kta_kafka_index_stats counts them.
 * Identities: the sums over the codecs of batches, records and payload equal the sums over the partitions of words 0, 1
 * and 3; words 4, 5 and 6 summed over the partitions equal batches, recbytes and payload summed over codecs 1..4; each
 * histogram of a codec sums to its batches; and, in a run with no failed batch and no filter, the records summed over the
 * partitions equal the counter vector's total_messages (tombstones included) over the partitions.
 * Composition.  During a compaction replay (kta_compaction_replay) the source is read a second time and the pass is
 * skipped: batches are counted once.  With a filter (kta_set_filter) a batch is counted iff its partition is selected and
 * its [base_ts_ms, max_ts_ms] overlaps the window, base_ts_ms < to_ms && max_ts_ms >= from_ms with an absent bound open:
 * the batches that overlap the window, not the records that pass.
 * With the flag off no kernel is launched and nothing is allocated. */
#define KTA_FLAG_RECORD_BATCHES 0x200U   /* 512: bit 9 (the suffix in capitals, as bit 8 has it) */
#define KTA_RB_PARTITION_WORDS 16
#define KTA_RB_CODECS 5
#define KTA_RB_CODEC_WORDS 100
#define KTA_RB_HIST_BINS 32
#define KTA_RB_MAX_WORDS 4
#define KTA_RB_SKETCH_REGISTERS 1024
#define KTA_RB_WORDS(P) (20u * (size_t)(P) + 1524u)
#define KTA_RB_SUM_WORDS(P) (16u * (size_t)(P) + 500u)

/* Payload (NOT in the reference, which never looks inside a value): what lies inside the records that the raw-log decode
 * delivers (kta_kafka.h: kta_kafka_decode_device, and through it kta_kafka_blob_submit and kta_kafka_consume) — the class of
 * every value, the schema-registry ids of the values in Confluent's wire format, and the record headers.  Opt-in at
 * kta_create.  Every word is exact and a SUM.  csrc/kta_payload.h is the code of everything below.
 * A record COUNTS when its batch's descriptor has status 0 after the call's inflate and decode kernels, its framing and that
 * of every record in front of it in the batch is good, its partition lies in [0, P) and, under kta_set_filter, it passes the
 * filter (its timestamp as the decode gives it: base_ts_ms + delta, or max_ts_ms under LogAppendTime).
 * Value class, exactly one: null (length -1); empty (0); framed (length >= 5 and byte 0 == 0x00: the id is bytes 1..4, big
 * endian); json (byte 0 is `{` or `[`); other.
 * Headers: headersCount varint, then per header keyLen varint | key | valueLen varint (-1: null) | value, up to the record's
 * end as its length prefix gives it.  BAD when the count or a key length is negative, a value length is below -1, a varint
 * runs on past ten bytes, a field overruns the record or the walk does not end exactly at the record's end (so also when
 * the section is absent).  A record with bad headers adds 1 to bad_headers and nothing to another header word or to the
 * histogram; its value counts all the same.
 * The vector is u64[24 P + 16 + 2 * 1024 * 34]:
 *   partition p, 24 words at 24 p: records; null, empty, framed, json, other records; the value bytes of the five classes;
 *     with_headers, headers, header_key_bytes, header_value_bytes, header_null_values, bad_headers, header_wire_bytes (the
 *     bytes from the headersCount varint to the record's end); six zeros;
 *   16 words at 24 P: records by their number of headers, 0 .. 14 and >= 15, over the topic;
 *   the schema-id table at 24 P + 16: two rows of 1024 cells of 34 words — T records, B value bytes, 32 bit counters.  A
 *     framed record with id x adds 1 to T, its value length to B and 1 to the counter of every set bit of x, in cell
 *     x & 1023 of row 0 and in cell fmix32(x) & 1023 of row 1 (murmur3's finaliser).
 * kta_payload_schema_ids reads the ids off the table; kta_payload_identities states the identities between the words.
 * Composition.  During a compaction replay (kta_compaction_replay) the source is read a second time and the pass is skipped:
 * records are counted once.  Failed batches (status != 0) add nothing; the record-batch section counts them.
 * With the flag off no kernel is launched and nothing is allocated. */
#define KTA_FLAG_PAYLOAD 0x400U          /* 1024: bit 10 */
#define KTA_PAYLOAD_PARTITION_WORDS 24
#define KTA_PAYLOAD_CLASSES 5            /* null, empty, framed, json, other */
#define KTA_PAYLOAD_HIST_BINS 16
#define KTA_PAYLOAD_ROWS 2
#define KTA_PAYLOAD_CELLS 1024
#define KTA_PAYLOAD_CELL_WORDS 34
#define KTA_PAYLOAD_WORDS(P) (24u * (size_t)(P) + 16u + 2u * 1024u * 34u)

/* Header names (NOT in the reference): a census of the names of the record headers that the raw-log decode delivers
 * (kta_kafka.h: kta_kafka_decode_device, and through it kta_kafka_blob_submit and kta_kafka_consume).  Opt-in at kta_create,
 * independent of KTA_FLAG_PAYLOAD.  Every word is exact and a SUM.  csrc/kta_header_names.h is the code of everything below.
 * A record COUNTS under the payload section's rule (above KTA_FLAG_PAYLOAD: status 0, framing, partition in [0, P), the
 * filter with LogAppendTime handled alike).  A counted record whose header section is BAD — the payload section's
 * definition, csrc/kta_payload.h's payload_walk_headers — adds nothing here; a counted record whose section is good is
 * LOOKED AT.  During a compaction replay the pass is skipped; failed batches add nothing.
 * Every header occurrence of a record looked at: h = the FNV-32 of the name's bytes as -c hashes keys (fnv32.rs:76-101; two
 * names of one hash are one name; an empty name is a name, of hash 0x811c9dc5).  The occurrence adds T += 1, L += name
 * length, V += value length (0 for a null value), Z += 1 for a null value and 1 to the bit counter of every set bit of h,
 * in cell h & 1023 of row 0 and in cell fmix32(h) & 1023 of row 1 (the payload table's cell rule).
 * The vector is u64[KTA_HEADER_NAMES_WORDS], independent of P:
 *   8 globals: occurrences, name bytes, value bytes, null values, records with at least one header, records looked at, two
 *     zero words;
 *   two rows of 1024 cells of 36 words at word 8: T, L, V, Z, 32 bit counters.
 * The NAME TABLE beside it, kta_header_name[2][1024], slot 1024 r + c for cell c of row r: a slot whose state is
 * KTA_HEADER_NAME_PUBLISHED holds the first min(name_len, 48) bytes of ONE occurrence's name whose hash is `hash` and maps
 * to that cell in that row.  The first writer wins.  Best effort: no count depends on it, it is not snapshotted and not
 * exchanged (it stays on its rank), kta_reset clears it.
 * kta_header_names_list reads the names off the table; kta_header_names_identities states the identities.
 * With the flag off no kernel is launched and nothing is allocated. */
#define KTA_FLAG_HEADER_NAMES 0x800U     /* 2048: bit 11 */
#define KTA_HEADER_NAMES_GLOBALS 8
#define KTA_HEADER_NAMES_ROWS 2
#define KTA_HEADER_NAMES_CELLS 1024
#define KTA_HEADER_NAMES_CELL_WORDS 36
#define KTA_HEADER_NAMES_WORDS (8u + 2u * 1024u * 36u)
#define KTA_HEADER_NAMES_SLOTS (2u * 1024u)
#define KTA_HEADER_NAME_BYTES 48
#define KTA_HEADER_NAME_PUBLISHED 2u
typedef struct kta_header_name {
    uint32_t hash;
    uint32_t name_len;       /* the name's whole length, also beyond 48 */
    uint32_t state;          /* KTA_HEADER_NAME_PUBLISHED, or the slot says nothing */
    uint32_t reserved;
    uint8_t bytes[KTA_HEADER_NAME_BYTES];
} kta_header_name;
/* A row of kta_header_names_list: a recovered hash with its exact sums; name[0 .. min(name_len, 48)) when has_name. */
typedef struct kta_header_name_row {
    uint32_t hash;
    uint32_t has_name;
    uint64_t occurrences;
    uint64_t name_len;       /* L / T */
    uint64_t value_bytes;
    uint64_t null_values;
    uint8_t name[KTA_HEADER_NAME_BYTES];
} kta_header_name_row;

/* Value bytes (NOT in the reference): a histogram of the bytes of the VALUES of the records that the raw-log decode delivers
 * (kta_kafka.h: kta_kafka_decode_device, and through it kta_kafka_blob_submit and kta_kafka_consume), per partition: would the
 * topic compress, is it text or binary, zero-padded, or compressed or encrypted by its producer already?  Opt-in at
 * kta_create, independent of every other flag.  Every word is exact and a SUM.  csrc/kta_value_bytes.h is the code of
 * everything below.
 * A record COUNTS under the payload section's rule (above KTA_FLAG_PAYLOAD: status 0, framing, partition in [0, P), the
 * filter with LogAppendTime handled alike).  During a compaction replay the pass is skipped; failed batches add nothing;
 * compressed batches are read in their inflated form: the section describes the uncompressed values.
 * Every byte b at position i of a counted record's value (val_len > 0) adds 1 to bin b of its partition, and 1 to `repeats`
 * when i > 0 and it equals the byte at i - 1 of the same value — never the byte in front of the value: not the length varint,
 * not the key, not the record before it.
 * The vector is u64[KTA_VALUE_BYTES_WORDS(P)], 264 words per partition: words 0 .. 255 the bins, 256 records (counted), 257
 * values (those with val_len > 0), 258 bytes, 259 repeats, 260 .. 263 zero.  There are no P-independent words and no cap on P
 * beyond what the vector costs.
 * kta_value_bytes_summary reads one partition's words, or their sum over the topic, off: H0, the order-0 floor, the shares
 * and a class.  The class is a HEURISTIC, the first that holds: none (no bytes), text (printable >= 95 % of the bytes), dense
 * (at least 65 536 bytes and H0 >= 7.5 bits: compressed, encrypted or random already), binary.
 * kta_value_bytes_identities states the identities.  With the flag off no kernel is launched and nothing is allocated. */
#define KTA_FLAG_VALUE_BYTES 0x1000U     /* 4096: bit 12 */
#define KTA_VALUE_BYTES_BINS 256
#define KTA_VALUE_BYTES_PARTITION_WORDS 264
#define KTA_VALUE_BYTES_WORDS(P) (264u * (size_t)(P))
#define KTA_VALUE_BYTES_NONE 0u
#define KTA_VALUE_BYTES_TEXT 1u
#define KTA_VALUE_BYTES_DENSE 2u
#define KTA_VALUE_BYTES_BINARY 3u
/* What kta_value_bytes_summary reads off 264 words.  entropy_bits: H0 = - sum (c / B) log2(c / B) over the non-zero bins in
 * ascending byte order, in double; 0 when B = 0.  floor_bytes: ceil(B H0 / 8), what an order-0 entropy coder alone could not
 * go below.  printable: bins 0x20 .. 0x7E plus \t \n \r.  zero: bin 0.  high: bins >= 0x80.  top_byte / top_count: the most
 * common byte (the lowest on a tie) and its count.  cls: KTA_VALUE_BYTES_NONE .. KTA_VALUE_BYTES_BINARY. */
typedef struct kta_value_bytes_summary_t {
    uint64_t records, values, bytes, repeats;
    uint64_t distinct, floor_bytes, printable, zero, high, top_count;
    double entropy_bits;
    uint32_t top_byte, cls;
} kta_value_bytes_summary_t;

/* Compression what-if (NOT in the reference): the bytes a defined LZ4 compressor, the MODEL, would leave of the records
 * section of every batch that the raw-log decode delivers (kta_kafka.h: kta_kafka_decode_device, and through it
 * kta_kafka_blob_submit and kta_kafka_consume), per partition and by the batch's current codec: what would
 * `compression.type=lz4` save on this topic, at its present batching?  Opt-in at kta_create, independent of every other flag.
 * Every word is exact and a SUM.  csrc/kta_lz4_model.h is the code of everything below and states the model once.
 * A batch COUNTS when its descriptor has status 0 and a partition in [0, P); with a filter (kta_set_filter) its partition is
 * in the set and its [base_ts_ms, max_ts_ms] overlaps the window, the record-batch section's rule: the section is about
 * whole batches.  During a compaction replay the pass is skipped; failed batches add nothing; compressed batches are read in
 * their inflated form.
 * The unit is a batch's inflated records section, cut into independent blocks of at most 65536 bytes.  Its frame is 7 bytes
 * (magic, FLG 0x60, BD 0x40, HC), per block 4 bytes and min(model(block), block length) bytes — a block that does not shrink is
 * stored —, and an end mark of 4 bytes; no checksums, no content size.  model(block): the LZ4 block grammar with a match
 * finder of a 4096-entry table that is looked up 64 positions at a time (kta_lz4_model.h).  The model is a FLOOR of what
 * compression wins: liblz4 itself finds candidates the model does not, gzip and zstd do better still.
 * The vector is u64[KTA_COMPRESS_WHATIF_WORDS(P)]: 8 words per partition — batches, blocks, stored_blocks, raw_bytes (the
 * records sections inflated), now_bytes (sum of batch_bytes - 61: the records sections as they lie on disk), model_bytes (the
 * frames), sequences (matches), match_bytes (the bytes matches cover) — and behind them 5 codecs x 4 words by the batch's
 * current codec (0 none, 1 gzip, 2 snappy, 3 lz4, 4 zstd): batches, raw_bytes, now_bytes, model_bytes.  The 61 bytes of a
 * batch's header are on neither side.  With the flag off no kernel is launched and nothing is allocated. */
#define KTA_FLAG_COMPRESS_WHATIF 0x2000U /* 8192: bit 13 */
#define KTA_COMPRESS_WHATIF_PARTITION_WORDS 8
#define KTA_COMPRESS_WHATIF_CODECS 5
#define KTA_COMPRESS_WHATIF_CODEC_WORDS 4
#define KTA_COMPRESS_WHATIF_WORDS(P) (8u * (size_t)(P) + 20u)

/* Record filter (NOT in the reference, which always consumes the whole topic): analyse a time window and a subset of
 * partitions.  kta_set_filter gives a context a window [from_ms, to_ms) and / or a set of partitions.  A record PASSES iff
 * both hold:
 *   - its partition is in the set, when a set is given; a partition outside [0, P) is in no set;
 *   - from_ms <= ts_ms < to_ms, when a bound is given (INT64_MIN / INT64_MAX: no bound on that side): the comparison is on
 *     the raw i64 milliseconds, before any / 1000.  A record with ts_ms == -1 (not available) fails as soon as either
 *     bound is set; without bounds it passes.
 * Without a set, a record whose partition is outside [0, P) passes the partition test, and is counted and reported as a
 * bad partition exactly as without a filter.
 * THE CONTRACT: for every handler and every opt-in pass, a filtered context is left in exactly the state of an unfiltered
 * context that was handed only the passing records — in the same order, with the same sequence numbers (a record keeps
 * the seq it had: its seq column's, or base_seq + its index in the batch it came in).  That covers the counter vector and
 * the alive set in both states, KTA_G_RECORDS and the extrema included, every opt-in result vector, and
 * KTA_ERR_TIMESTAMP_RANGE / KTA_ERR_BAD_PARTITION: a record that is filtered out can cause neither.
 * How: every submission path (the staging ring behind kta_batch_submit, kta_handle_message and kta_replay_messages;
 * kta_submit_device[_ex]; the Kafka decode) ends in one function, and there a filtered context compacts the batch in
 * record order into a scratch batch of its own (raw layout, keys zero-copy) before the existing passes, which are
 * unchanged, see a shorter batch.  The batch is taken in slices of at most 2^26 records; a slice costs three launches
 * (count per 1024-record tile, prefix of the counts, scatter) and ONE HOST WAIT on the compute stream, for the prefix's
 * total: the plans of the passes behind need the record count on the host.  A filtered submit is therefore not
 * asynchronous.  A tile of a kta_device_batch_alloc allocation is decided from its 24 bytes of header and summary
 * (kta_tile_sum) where they say that none or all of its records pass; a slice of which nothing passes launches nothing
 * more, and one of which everything passes is handed on as it is (neither is scattered).  The scratch batch grows to the largest slice seen (20 B per record, 24 with
 * key columns, 8 more in the table state).  Without a filter nothing is launched, allocated or waited for. */

/* One batch of decoded records as struct-of-arrays columns.  What the reference's
 * handlers read from a BorrowedMessage (metric.rs:208-209, 218, 233, 291-293):
 *   partition[i]  m.partition()                                          i32
 *   ts_ms[i]      raw rdkafka timestamp in ms; -1 == not available       i64
 *   key_len[i]    m.key():  -1 == None, >= 0 == Some(k).len()            i32
 *   val_len[i]    m.payload(): -1 == None (tombstone), >= 0 == len       i32
 *   key_off[i]    offset of the key's bytes in key_bytes (if key_len>0)  u32  (-c, KTA_FLAG_KEY_SKETCH or KTA_FLAG_HOT_KEYS only)
 *   key_bytes     concatenated key bytes; device buffers must be readable  u8   (-c, KTA_FLAG_KEY_SKETCH or KTA_FLAG_HOT_KEYS only)
 *                 for 16 bytes past the last key (kta_device_batch_alloc pads)
 *   seq[i]        optional global consumption index; NULL => base_seq+i  u64  (-c only)
 * Value bytes are never read by the reference path (only their length). */
/* Device batch layouts (kta_batch.layout).
 *   KTA_LAYOUT_RAW (0)           the columns as above, one element per record.  What a zero-initialised kta_batch
 *                                means, what host batches and the staging ring always are.
 *   KTA_LAYOUT_TILE_COMPACT (1)  what kta_device_batch_alloc returns.  Records are grouped in tiles of
 *                                KTA_TILE_RECORDS; tile t owns the same bytes of each column as in the raw layout
 *                                (records [t*1024, t*1024+1024)), and tile_hdr[t].mode says how partition and ts_ms use them:
 *     KTA_TILE_RAW      the raw layout (a zero header: what a fresh allocation holds)
 *     KTA_TILE_COMPACT  partition as u16 in the first half of the tile's partition bytes (KTA_COMPACT_PART_NONE == -1),
 *                       ts_ms as an i32 offset from ts_base in the first half of the tile's ts_ms bytes
 *                       (KTA_COMPACT_TS_NONE == -1, not available): 6 B per record instead of 12.  Taken when every
 *                       partition id lies in [-1, 65535) and the tile's timestamps other than -1 span less than 2^31 ms.
 *   tile_hdr[t].lens, independent of mode, says how key_len and val_len use the tile's bytes:
 *     KTA_TILE_LENS_I32  i32 per record in both columns, as in the raw layout (a zero header)
 *     KTA_TILE_LENS_U16  the tile's own 4 KiB of the key_len column hold 256 groups of 16 B: group g has the four u16
 *                        key lengths of the tile's records 4g .. 4g+3, then their four u16 value lengths
 *                        (KTA_COMPACT_LEN_NONE == -1, None); the tile's bytes of the val_len column are unused: 4 B per
 *                        record instead of 8.  Taken when every key_len and val_len of the tile lies in [-1, 65535).
 *                        ONLY in allocations without key columns (kta_device_batch_alloc with key_bytes_capacity == 0):
 *                        a keyed allocation never has lens != 0, so the kernels that read lengths next to keys always
 *                        see plain i32 columns.  When a view into a keyless allocation is handed to a key-reading pass
 *                        together with key columns of the caller's own, the lengths of the tiles it touches are widened
 *                        in place first.
 *   Tile summaries (kta_tile_sum): every allocation of kta_device_batch_alloc keeps one summary per tile BESIDE the
 *   headers (not in them: kta_tile_hdr is unchanged).  A summary is trusted only next to a KTA_TILE_COMPACT header;
 *   whoever writes a COMPACT header writes that tile's summary in the same step, and the summary is VALID only if that
 *   step wrote all KTA_TILE_RECORDS records of the tile (the partial last tile of a fill gets a zero summary; all zero
 *   means "no summary").  It holds what the writer knew anyway: the span of the tile's timestamps other than -1 (the
 *   latest is ts_base + ts_span, modulo 2^64), its largest stored u16 partition, and whether it has timed and untimed
 *   records.  The packed metrics scan takes a summarised tile's earliest and latest timestamp from it and does not
 *   load the tile's timestamp offsets (6 B per record instead of 10).  A hand-built tile-compact kta_batch with its
 *   own tile_hdr has no summaries.  kta_batch_tile_summaries reads them back.
 *   Scan planes: a KTA_TILE_COMPACT tile uses only the first 4 KiB of its 8 KiB of the ts_ms column.  Bytes
 *   [4096, 8192) may hold the tile's scan plane: record j of the tile as the u32 at byte 4096 + 4 j,
 *   partition | key << 8 | val << 16 — partition in [0, 256) (no marker: a tile with an id of -1 or >= 256 has no plane),
 *   key the key length in [0, 255) or 0xFF for -1, val the value length in [0, 65535) or KTA_COMPACT_LEN_NONE for -1.
 *   The plane REPEATS what the u16 / i32 forms of the tile hold — those are written exactly as without it, and every
 *   reader but the packed metrics scan reads them —; the scan reads 4 B per record of a tile with a plane instead of 6,
 *   in one stream.  A tile has a plane exactly when its mark is 1: the marks are a u32 per tile that the allocation
 *   keeps beside the summaries.  A mark is trusted only next to a KTA_TILE_COMPACT header and a VALID summary; whoever
 *   writes a tile's summary writes its mark, 0 or 1, in the same step, and the plane before it; the mark is 1 only for a
 *   compact tile of all 1024 records in which every record fits.  A header that turns raw needs nothing more, and
 *   widening the lengths touches neither the ts_ms bytes nor the values.  The plane does not depend on `lens`: tiles
 *   of keyed allocations have planes too.  kta_batch_tile_planes reads the marks back.  Beside the marks the
 *   allocation keeps two more u32 per tile, trusted only where the mark is 1 and written with it: the least and the
 *   largest key_len + val_len of the tile's records that have a value (a key of -1 counts as 0; 0xFFFFFFFF / 0 when it
 *   has none).  The scan takes a marked tile's size extrema from them and adds the plane's lengths as stored, markers
 *   included; the counts of null keys and tombstones correct the two size sums when they leave the workgroup's LDS.
 *   key_off, key_bytes and seq are the same in both layouts.  The columns of a tile-compact batch are
 *   written by kta_synth_fill_device (compact tiles), kta_kafka_decode_device (raw tiles) and kta_batch_from_raw, and
 *   read back by kta_batch_to_raw; a raw-layout kta_batch whose column pointers lie inside a tile-compact allocation of
 *   the same context (a view at a record offset) is resolved to it by every entry point.  Reading key_len / val_len of a
 *   keyless tile-compact allocation with a plain copy gives the tiles' stored form: use kta_batch_to_raw. */
#define KTA_LAYOUT_RAW 0u
#define KTA_LAYOUT_TILE_COMPACT 1u
#define KTA_TILE_RECORDS 1024u
#define KTA_TILE_RAW 0u
#define KTA_TILE_COMPACT 1u
#define KTA_COMPACT_PART_NONE 0xFFFFu        /* compact partition of a record whose id is -1 */
#define KTA_COMPACT_TS_NONE INT32_MIN        /* compact timestamp of a record whose ts_ms is -1 */
#define KTA_TILE_LENS_I32 0u
#define KTA_TILE_LENS_U16 1u
#define KTA_COMPACT_LEN_NONE 0xFFFFu         /* u16 length of a record whose key_len / val_len is -1 */

typedef struct kta_tile_hdr {
    int64_t ts_base;   /* KTA_TILE_COMPACT: ts_ms = ts_base + offset */
    uint32_t mode;     /* KTA_TILE_RAW / KTA_TILE_COMPACT: partition and ts_ms */
    uint32_t lens;     /* KTA_TILE_LENS_I32 / KTA_TILE_LENS_U16: key_len and val_len */
} kta_tile_hdr;

#define KTA_TILE_SUM_VALID 1u     /* the summary describes all 1024 records of the tile */
#define KTA_TILE_SUM_TIMED 2u     /* the tile has a timestamp other than -1 */
#define KTA_TILE_SUM_UNTIMED 4u   /* the tile has a timestamp of -1 */
typedef struct kta_tile_sum {   /* of a KTA_TILE_COMPACT tile whose 1024 records one producer call wrote; all zero: none */
    uint32_t ts_span;           /* hi - lo of the timestamps other than -1 (lo is tile_hdr.ts_base); < 2^31 */
    uint16_t part_max;          /* the largest stored u16 partition (a record with id -1 makes it KTA_COMPACT_PART_NONE) */
    uint16_t flags;             /* KTA_TILE_SUM_VALID | _TIMED | _UNTIMED */
} kta_tile_sum;

typedef struct kta_batch {
    int32_t *partition;
    int32_t *key_len;
    int32_t *val_len;
    int64_t *ts_ms;
    uint32_t *key_off;
    uint8_t *key_bytes;
    uint64_t *seq;
    uint64_t capacity;           /* records the columns can hold   */
    uint64_t key_bytes_capacity; /* bytes key_bytes can hold       */
    kta_tile_hdr *tile_hdr;      /* KTA_LAYOUT_TILE_COMPACT: one header per tile of the capacity */
    uint32_t layout;             /* KTA_LAYOUT_*                   */
    uint32_t reserved;           /* 0                              */
} kta_batch;

/* Decoded results: everything the reference's report reads (main.rs:130-170). */
typedef struct kta_result {
    uint32_t n_partitions;
    uint32_t any_records;      /* 1 if at least one record was scanned                 */
    uint32_t any_live;         /* 1 if at least one non-tombstone was scanned           */
    uint32_t count_alive_keys; /* 1 if alive_keys is valid                              */
    int64_t min_ts_sec;        /* min over records of trunc(ts_ms/1000) (metric.rs:210) */
    int64_t max_ts_sec;
    uint64_t smallest_message; /* raw state: u64::MAX if no non-tombstone (metric.rs:42) */
    uint64_t largest_message;  /* raw state: 0 if none (metric.rs:41)                   */
    uint64_t overall_count;    /* metric.rs:25 */
    uint64_t overall_size;     /* metric.rs:24 */
    uint64_t alive_keys;       /* sum_all_alive(), metric.rs:282-284                    */
    uint64_t bad_partition_records;
} kta_result;

/* ---- lifecycle ---------------------------------------------------------------- */
/* MessageMetrics::new + LogCompactionInMemoryMetrics::new (metric.rs:30-46, 267-271):
 * allocates the device counter vector, the scan workspace and — with
 * count_alive_keys — the 2^32-slot last-writer table (32 GiB of HBM). */
int kta_create(const kta_config *cfg, kta_ctx **out);
void kta_destroy(kta_ctx *ctx);
/* Message of the last failure on this context (ctx may be NULL: last kta_create failure
 * on the calling thread).  Never NULL. */
const char *kta_last_error(const kta_ctx *ctx);
int kta_abi_version(void);
/* HIP devices visible to the process (a sharded run places rank r on device r). */
int kta_device_count(int *n);
/* Zero all accumulated state (counters, extrema, alive table). */
int kta_reset(kta_ctx *ctx);

/* ---- per-message entry: what MetricHandler::handle_message binds to ----------- */
/* kafka.rs:107-109 / metric.rs:207-252 / metric.rs:289-304.  key == NULL or
 * key_len < 0 is key None; val_len < 0 is payload None.  The call copies lengths,
 * timestamp, partition and (with -c) the key bytes into the current pinned staging
 * batch and submits it when full.  Records get consecutive sequence numbers. */
int kta_handle_message(kta_ctx *ctx, int32_t partition, int64_t ts_ms, const void *key,
                       int64_t key_len, int64_t val_len);
/* Submit the partially filled staging batch, if any. */
int kta_flush(kta_ctx *ctx);
/* kta_handle_message for each of the n records of HOST columns, in order — what the reference's consume loop
 * (kafka.rs:92-135) does with the messages it polls, as a native loop: a host in a language with an expensive foreign
 * call (the ctypes mirror, a JVM) replays decoded records through the per-message entry without paying that call per
 * message, and bench.py times the entry itself with it (`boundary_per_message`).  cols: partition, key_len, val_len,
 * ts_ms; with -c also key_off and key_bytes (a key of length >= 0 is passed as a non-null pointer, -1 as key None). */
int kta_replay_messages(kta_ctx *ctx, const kta_batch *host_cols, uint64_t n);
/* Host-side cost of the per-message entry since kta_create / kta_reset: out[0] messages taken, out[1] staging batches
 * submitted by it, out[2] nanoseconds spent submitting them (the copy's and the kernels' launches), out[3] nanoseconds
 * blocked because the staging ring had wrapped onto a batch still in flight (the GPU, or the link, was the slower side). */
int kta_handle_message_stats(kta_ctx *ctx, uint64_t out[4]);
/* The next record of kta_handle_message / kta_kafka_consume gets this global sequence number (a rank of a
 * sharded run positions itself at the first record of each of its partitions' stretches). */
int kta_seek_seq(kta_ctx *ctx, uint64_t next_seq);

/* ---- batch entry: a decoder that already produces columns --------------------- */
/* Borrow the current pinned staging batch (blocks until the ring has a free one). */
int kta_batch_acquire(kta_ctx *ctx, kta_batch *out);
/* Submit the first n_records of the acquired batch: async H2D copy + kernels.
 * base_seq = global consumption index of record 0 (ignored without -c). */
int kta_batch_submit(kta_ctx *ctx, uint64_t n_records, uint64_t n_key_bytes, uint64_t base_seq);

/* ---- device-resident batches (HBM-resident topic shards, benchmarks) ----------- */
/* Column pointers in `cols` are device pointers (16-byte aligned).  Asynchronous on
 * the context's compute stream. */
int kta_submit_device(kta_ctx *ctx, const kta_batch *cols, uint64_t n_records, uint64_t base_seq);
/* Run only one of the two handlers over a device batch (profiling / benchmarks):
 * which = 1 MessageMetrics, 2 LogCompactionInMemoryMetrics, 3 both.  With both, -c, the bit set state and at most 256
 * partitions the batch is read ONCE: the first kernel of the alive-key pass also does the metrics handler's work
 * (src/kafka.rs:107-109 hands every message to every handler; same results bit for bit; kta_set_fuse(ctx, 0)
 * keeps the two passes).  kta_batch_submit and kta_handle_message submit with which = 3. */
int kta_submit_device_ex(kta_ctx *ctx, const kta_batch *cols, uint64_t n_records,
                         uint64_t base_seq, int which);
int kta_device_batch_alloc(kta_ctx *ctx, uint64_t capacity, uint64_t key_bytes_capacity,
                           int with_seq, kta_batch *out);
int kta_device_batch_free(kta_ctx *ctx, kta_batch *cols);
/* The four metric columns (partition, key_len, val_len, ts_ms) of records [0, n) between HOST columns in the raw layout
 * and a device batch of either layout (synchronous).  from_raw packs every tile that the compact form holds losslessly
 * (partition and ts_ms; in an allocation without key columns also the lengths, as u16) and stores the others raw, so any i32 / i64 values round-trip exactly; into a tile-compact batch it writes from a
 * tile boundary (record 0 of the allocation or of a view at a multiple of KTA_TILE_RECORDS) and may overwrite the rest
 * of the last tile it touches.  to_raw unpacks. */
int kta_batch_from_raw(kta_ctx *ctx, const kta_batch *host_cols, uint64_t n, const kta_batch *device_cols);
int kta_batch_to_raw(kta_ctx *ctx, const kta_batch *device_cols, uint64_t n, const kta_batch *host_cols);
/* The tile summaries (kta_tile_sum, above) of the tiles of records [0, n) of a device batch: tiles_of(n) = ceil(n / 1024)
 * entries to `out` (synchronous).  device_cols is an allocation of kta_device_batch_alloc or a view of one that starts on
 * a tile boundary; KTA_ERR_INVALID for anything else (a batch without summaries).  An entry is meaningful only where
 * the tile's header is KTA_TILE_COMPACT. */
int kta_batch_tile_summaries(kta_ctx *ctx, const kta_batch *device_cols, uint64_t n, kta_tile_sum *out);
/* Its twin for the plane marks (scan planes, above): tiles_of(n) u32 to `out`, 1 where the tile has a plane.  The same
 * batches, the same errors; an entry is meaningful only where the tile's header is KTA_TILE_COMPACT and its summary VALID. */
int kta_batch_tile_planes(kta_ctx *ctx, const kta_batch *device_cols, uint64_t n, uint32_t *out);
/* Plain copies.  NOT a way to write the partition, ts_ms, key_len or val_len column of a tile-compact allocation
 * (kta_device_batch_alloc): its tiles' headers and summaries describe the bytes their producer stored, and the scan trusts
 * them — a summarised tile's stored partitions are not compared with P again, so partition bytes written behind a
 * summary's back index the scan's LDS out of bounds.  Write such a batch with kta_batch_from_raw, kta_synth_fill_device or
 * kta_kafka_decode_device only.  key_off, key_bytes and seq are plain in both layouts. */
int kta_copy_to_device(kta_ctx *ctx, void *dst_device, const void *src_host, size_t bytes);
int kta_copy_to_host(kta_ctx *ctx, void *dst_host, const void *src_device, size_t bytes);

/* ---- record filter (definition above kta_batch) ---------------------------------------------------------------- */
/* from_ms == INT64_MIN / to_ms == INT64_MAX: no bound on that side.  partition_bitmap == NULL: all partitions; else bit
 * p & 31 of word p / 32 is partition p, n_words >= 1 words are read, and a bit at or beyond P is KTA_ERR_INVALID, as is
 * from_ms >= to_ms and a set on a context of more than 2^19 partitions.  Neither bound and no set: the context has no
 * filter (again).  Accepted only while the context has been handed no record since kta_create / kta_reset, as
 * kta_set_timeline is; kta_reset keeps the filter and zeroes kta_filter_info's counts. */
int kta_set_filter(kta_ctx *ctx, int64_t from_ms, int64_t to_ms, const uint32_t *partition_bitmap, uint32_t n_words);
/* Since kta_create / kta_reset (staged messages are flushed first): out[0] records seen, out[1] records passed, out[2]
 * tiles decided by their summary as "none passes", out[3] tiles decided by their summary as "all pass", out[4] tiles
 * read record by record, out[5] slices.  All zero on a context without a filter. */
int kta_filter_info(kta_ctx *ctx, uint64_t out[6]);
/* Tuning and tests: the records of a slice, a multiple of 1024, at most 2^26 (0: the default, 2^26). */
int kta_set_filter_slice(kta_ctx *ctx, uint64_t records);
/* The same predicate over HOST columns (host only, no context, no device): the indices of the passing records of
 * [0, n), ascending, to indices_out (may be NULL: count only) and their number to *n_out.  A bitmap has at least
 * ceil(n_partitions / 32) words. */
int kta_filter_host(const int32_t *partition, const int64_t *ts_ms, uint64_t n, uint32_t n_partitions, int64_t from_ms, int64_t to_ms,
                    const uint32_t *partition_bitmap, uint32_t n_words, uint64_t *indices_out, uint64_t *n_out);
/* What one tile's header and summary decide (host only): 0 the tile's records are read, 1 none passes, 2 all pass; negative:
 * an error.  whole: the tile's 1024 records all belong to the slice. */
int kta_filter_tile_host(uint32_t n_partitions, int64_t from_ms, int64_t to_ms, int has_partition_set, const kta_tile_hdr *hdr,
                         const kta_tile_sum *sum, int whole);

/* Run the context's kernels on a caller-owned HIP stream (e.g. the stream RCCL collectives are issued
 * on), so that submit -> collective -> next submit needs no host synchronisation.  NULL restores the
 * context's own compute stream — so the null (default) stream, whose handle is 0, cannot be selected:
 * pass a created stream (PyTorch: a torch.cuda.Stream, not the default stream).  The stream must belong to
 * the context's device and outlive its use. */
int kta_set_compute_stream(kta_ctx *ctx, void *hip_stream);

/* ---- results --------------------------------------------------------------------- */
/* Wait for everything submitted so far. */
int kta_sync(kta_ctx *ctx);
/* Fold everything submitted so far, count alive keys (with -c), copy the counter vector
 * to the host and decode it.  counters_out (may be NULL) receives P*7 u64.  Returns
 * KTA_ERR_BAD_PARTITION (results still filled in) if any record was out of range, and
 * KTA_ERR_TIMESTAMP_RANGE (results filled in as well, and taking precedence) if the reference would not
 * have got this far: some record's ts / 1000 lies outside [KTA_CHRONO_MIN_SEC, KTA_CHRONO_MAX_SEC].
 * Non-destructive: more batches may follow and kta_finish may be called again. */
int kta_finish(kta_ctx *ctx, kta_result *out, uint64_t *counters_out);
/* Device pointer and length (in u64) of the SNAPSHOT of the counter vector that kta_finish_device
 * takes: collectives may reduce it in place, the live accumulator is never touched, so the counters of
 * kta_finish and of further batches after an exchange stay correct.  One exception, -c after an exchange with
 * nranks > 1: the exchange merges other ranks' entries of this rank's hash range INTO this rank's table, so the
 * `alive_keys` of a later kta_finish on this context is neither the rank's own count nor the job's — read the
 * job's count from kta_exchange_result (every exchange recomputes it). */
int kta_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
/* As kta_finish but leaves the snapshot on the device (no D2H, asynchronous). */
int kta_finish_device(kta_ctx *ctx);

/* ---- multi-GPU exchange: one context = one rank = one GPU, RCCL over xGMI --------------------------- */
/* The reference is one process, one MessageMetrics, one BitSet (main.rs:77-82).  Kafka partitions shard
 * across GPUs with no data-path collective (every per-partition counter depends on its own partition's
 * records only, metric.rs:74-100); what replaces "the report reads the handlers" (main.rs:121-179) is ONE
 * exchange step.  Records of a sharded -c run carry GLOBAL sequence numbers (kta_batch.seq / base_seq).
 *   kta_comm_unique_id  on one rank; hand the 128 bytes to the others out of band
 *   kta_comm_create     every rank, collectively (ncclCommInitRank); nranks == 1 needs no id and no RCCL
 *   kta_exchange        kta_finish_device, then on the compute stream: (-c) every rank sends the table
 *                       entries it ever wrote to the owner of their hash range (rank r owns the slots
 *                       [ceil(r 2^32 / R), ceil((r+1) 2^32 / R)); one grouped ncclSend / ncclRecv), the
 *                       owner merges by last writer and counts its range; then ONE grouped launch of
 *                       all-reduce SUM over vec[0 : P*7+4] and all-reduce MAX over vec[P*7+4 : P*7+8]
 *                       What a rank sends is found through the list of slots the context wrote for the first
 *                       time (4 bytes per distinct key hash), not by sweeping the 32 GiB table; the one host
 *                       synchronisation of the step is for the sizes of the sends.  A rank that fails locally
 *                       aborts its communicator (ncclCommAbort), so that its peers get an error instead of
 *                       waiting in their collectives; the context's communicator is unusable afterwards.
 *                       With KTA_FLAG_ANALYTICS the same grouped launch also reduces the analytics snapshot:
 *                       all-reduce SUM (u64) over its 2 x 34 histogram words and all-reduce MAX (i64) over its
 *                       4 * P extrema words (neutral element INT64_MIN: a partition's owner wins).
 *                       With a timeline (kta_set_timeline) the same grouped launch also reduces the timeline
 *                       snapshot: all-reduce SUM (u64) over all of its words.
 *                       With KTA_FLAG_KEY_SKETCH the same grouped launch also reduces the key sketch's snapshot:
 *                       all-reduce MAX (u64) over all of its P * 4096 words.
 *                       With KTA_FLAG_HOT_KEYS the same grouped launch also reduces the hot-key snapshot:
 *                       all-reduce SUM (u64) over all of its 47 104 words (exemplars stay on their rank).
 *                       With KTA_FLAG_TS_ORDER the same grouped launch also reduces the timestamp-order snapshot:
 *                       all-reduce SUM (u64) over its first 2 P + 64 words and all-reduce MAX (i64) over its last P.
 *                       With KTA_FLAG_PARTITIONER the same grouped launch also reduces the partitioner snapshot:
 *                       all-reduce SUM (u64) over all of its 2 P + 2 Q words.
 *                       With KTA_FLAG_SIZE_QUANTILES the same grouped launch also reduces the size-percentile snapshot:
 *                       all-reduce SUM (u64) over all of its P * 3 * 464 + 8 words (every rank needs the flag).
 *   kta_exchange_result the decoded snapshot: after kta_exchange the whole job's result on every rank
 *                       (kta_exchange_analytics, kta_exchange_timeline, kta_exchange_key_sketch, kta_exchange_hot_keys:
 *                       the same for the analytics, the timeline, the key sketch, the hot keys)
 * Every rank of a job must be created with the same P AND the same KTA_FLAG_ANALYTICS, KTA_FLAG_KEY_SKETCH,
 * KTA_FLAG_HOT_KEYS, KTA_FLAG_TS_ORDER and KTA_FLAG_PARTITIONER bits (and, for the timestamp order to be the topic's, every
 * partition's records must have gone through ONE rank in order: partition p on rank p % N; with the partitioner pass,
 * the same Q: kta_set_repartition), and
 * be given the same timeline configuration (or none on every rank): the collectives of a rank with analytics, a key
 * sketch or a timeline do not match those of a rank without, and nothing checks that the configurations agree.
 * RCCL is bound at run time (KTA_RCCL_LIBRARY, /opt/rocm/lib/librccl.so.1). */
#define KTA_COMM_ID_BYTES 128
int kta_comm_unique_id(uint8_t id[KTA_COMM_ID_BYTES]);
int kta_comm_create(kta_ctx *ctx, int nranks, int rank, const uint8_t id[KTA_COMM_ID_BYTES]);
int kta_comm_destroy(kta_ctx *ctx);
int kta_exchange(kta_ctx *ctx);
int kta_exchange_result(kta_ctx *ctx, kta_result *out, uint64_t *counters_out);
/* Small host-side vectors of the same job (per-partition start / end offsets of the report,
 * main.rs:155-157): all-reduce SUM (op_max 0) or MAX (1), in place, synchronous. */
int kta_comm_allreduce_i64(kta_ctx *ctx, int64_t *host_values, size_t n, int op_max);
/* Communicator facts and the alive entries the last kta_exchange sent / received (profiling). */
int kta_comm_info(kta_ctx *ctx, int *nranks, int *rank, uint64_t *entries_sent, uint64_t *entries_received);
/* Host-side decode of a (possibly all-reduced) counter vector. */
int kta_decode_vector(const uint64_t *vec, uint32_t n_partitions, int count_alive_keys,
                      kta_result *out, uint64_t *counters_out);
/* Host-side merge of two counter vectors (acc <- acc (+) other) with the per-field
 * reduction operator (SUM over the prefix, signed MAX over the last four words) — exactly
 * the reduction the two collectives implement. */
int kta_merge_vectors(uint64_t *acc, const uint64_t *other, uint32_t n_partitions);

/* Analytics of everything submitted so far (context created with KTA_FLAG_ANALYTICS).  The four
 * per-partition arrays (length P, any may be NULL) use the reference's conventions: seconds =
 * trunc(ms / 1000) with a raw timestamp of -1 counted as 0; a partition without records reports
 * min_ts_sec = INT64_MAX / max_ts_sec = INT64_MIN; without non-tombstones smallest = UINT64_MAX,
 * largest = 0. */
int kta_get_analytics(kta_ctx *ctx, kta_analytics *out, int64_t *part_min_ts_sec, int64_t *part_max_ts_sec,
                      uint64_t *part_smallest, uint64_t *part_largest);
/* Device pointer / length (u64) of the analytics vector: [2 x 34 histogram (SUM)] then per
 * partition [~min ts_ms, max ts_ms, ~smallest, largest] (signed MAX) — reducible across GPUs like
 * the counter vector. */
int kta_analytics_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
/* The analytics of the SNAPSHOT that kta_finish_device (kta_finish, kta_exchange) takes of the analytics vector,
 * decoded like kta_get_analytics: after kta_exchange the whole job's analytics on every rank.  The live accumulator
 * (kta_get_analytics, kta_analytics_vector) is never reduced, so further batches and a second exchange do not count
 * anything twice. */
int kta_exchange_analytics(kta_ctx *ctx, kta_analytics *out, int64_t *part_min_ts_sec, int64_t *part_max_ts_sec,
                           uint64_t *part_smallest, uint64_t *part_largest);
/* Device pointer / length (u64) of that snapshot: what collectives (distributed.py) reduce in place. */
int kta_analytics_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
/* Host-side decode of a (possibly all-reduced) analytics vector u64[2*34 + 4*P], conventions as kta_get_analytics. */
int kta_decode_analytics(const uint64_t *vec, uint32_t n_partitions, kta_analytics *out, int64_t *part_min_ts_sec,
                         int64_t *part_max_ts_sec, uint64_t *part_smallest, uint64_t *part_largest);
/* Host-side merge of two analytics vectors (acc <- acc (+) other): SUM over the histograms, signed MAX over
 * the extrema — exactly the reduction the two collectives of the exchange implement. */
int kta_merge_analytics(uint64_t *acc, const uint64_t *other, uint32_t n_partitions);
/* The largest P a KTA_FLAG_ANALYTICS context may have: the analytics scan's LDS plan (7 u64 per partition slot plus
 * the histograms) must fit one workgroup's 160 KiB of LDS on gfx950.  kta_create refuses more. */
int kta_analytics_max_partitions(void);

/* Give the context a timeline (definition above KTA_TIMELINE_MAX_BUCKETS), zeroed.  Accepted only while the context
 * has been handed no record since kta_create / kta_reset (kta_reset zeroes the timeline and keeps its
 * configuration); may be called again then to change it.  KTA_ERR_INVALID, with a kta_last_error message and
 * nothing launched, for a value out of range, after a batch, or when the scan's LDS plan with the timeline does not
 * fit one workgroup (with KTA_FLAG_ANALYTICS and a large P: kta_timeline_max_partitions).  With -c, a batch of a
 * context with a timeline takes two passes (scan, then the alive-key pass), as with analytics.
 * Every timeline call below on a context without a timeline returns KTA_ERR_INVALID. */
int kta_set_timeline(kta_ctx *ctx, int64_t origin_ms, int64_t bucket_ms, uint32_t n_buckets);
/* The largest P a context created with `flags` may have for a timeline of n_buckets buckets (host only; 0 for an
 * n_buckets out of range).  Never more than kta_analytics_max_partitions() with KTA_FLAG_ANALYTICS. */
int kta_timeline_max_partitions(uint32_t flags, uint32_t n_buckets);
/* The live accumulator, copied to out[n_u64] (n_u64 = (n_buckets + 3) * KTA_TIMELINE_COLS; staged messages are
 * flushed first). */
int kta_get_timeline(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* Device pointer / length (u64) of the live accumulator. */
int kta_timeline_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
/* The SNAPSHOT that kta_finish_device (kta_finish, kta_exchange) takes of the timeline, copied to out[n_u64]: after
 * kta_exchange the whole job's timeline on every rank.  The live accumulator is never reduced, so further batches
 * and a second exchange do not count anything twice. */
int kta_exchange_timeline(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* Device pointer / length (u64) of that snapshot: what collectives (distributed.py) reduce in place. */
int kta_timeline_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);

/* Key sketch (context created with KTA_FLAG_KEY_SKETCH; definition above KTA_FLAG_KEY_SKETCH).  With the flag the staging
 * batches carry key_off and key_bytes without -c as well (kta_handle_message, kta_batch_submit, kta_replay_messages, the
 * Kafka decode), and a device batch handed to the metrics handler (which & 1) without key columns is refused with
 * KTA_ERR_INVALID before anything is launched.  kta_reset zeroes the registers; kta_finish_device snapshots them.  Every
 * call below on a context without the flag returns KTA_ERR_INVALID.
 * The live accumulator, copied to out[n_u64] (n_u64 = P * 4096; staged messages are flushed first). */
int kta_get_key_sketch(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* The SNAPSHOT that kta_finish_device (kta_finish, kta_exchange) takes, copied to out[n_u64]: after kta_exchange the
 * whole job's sketch on every rank.  The live accumulator is never reduced. */
int kta_exchange_key_sketch(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* Device pointer / length (u64) of that snapshot: what collectives (distributed.py) reduce in place. */
int kta_key_sketch_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
/* Host-side merge of two sketch vectors u64[P * 4096] (acc <- max(acc, other), word by word): what the exchange's
 * all-reduce MAX implements. */
int kta_merge_key_sketch(uint64_t *acc, const uint64_t *other, uint32_t n_partitions);
/* Host-side estimate of a sketch vector (no device): per_partition[P] (may be NULL) the estimated distinct keys of each
 * partition, *topic (may be NULL) the estimate of the register-wise max over all partitions — a key hash seen in two
 * partitions counts once, as for -c.  Ertl's improved raw estimator (Ertl 2017, "New cardinality estimation algorithms
 * for HyperLogLog sketches", Algorithm 6), q = 20: exactly 0 for an empty sketch, +inf when every register is 21.
 * KTA_ERR_INVALID for a register above 21. */
int kta_key_sketch_estimate(const uint64_t *vec, uint32_t n_partitions, double *per_partition, double *topic);
/* Work counters of the sketch kernel since kta_create / kta_reset (profiling; waits for the compute stream): out[0]
 * keyed records it looked at, out[1] of them past the floor filter (a read of their register), out[2] atomics issued,
 * out[3] launches. */
int kta_key_sketch_info(kta_ctx *ctx, uint64_t out[4]);

/* Hot keys (context created with KTA_FLAG_HOT_KEYS; definition above KTA_FLAG_HOT_KEYS).  With the flag the staging
 * batches carry key_off and key_bytes without -c as well, and a device batch handed to the metrics handler (which & 1)
 * without key columns is refused with KTA_ERR_INVALID before anything is launched.  kta_reset zeroes the vector and the
 * exemplars; kta_finish_device snapshots the vector.  Every call below that takes a context fails on one without the flag
 * with KTA_ERR_INVALID and a message naming KTA_FLAG_HOT_KEYS.
 * The live accumulator, copied to out[n_u64] (n_u64 = KTA_HOT_VECTOR_WORDS; staged messages are flushed first). */
int kta_get_hot_keys(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* The SNAPSHOT that kta_finish_device (kta_finish, kta_exchange) takes, copied to out[n_u64]: after kta_exchange the
 * whole job's vector on every rank.  The live accumulator is never reduced. */
int kta_exchange_hot_keys(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* Device pointer / length (u64) of that snapshot: what collectives (distributed.py) reduce in place. */
int kta_hot_keys_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
/* Host-side merge of two vectors (acc <- acc + other, word by word): what the exchange's all-reduce SUM implements. */
int kta_merge_hot_keys(uint64_t *acc, const uint64_t *other);
/* Host-side readout of a vector (no device): at most max_out (<= 2048) entries to `entries`, their number to *n_out,
 * the keyed records to *keyed (may be NULL).  KTA_ERR_INVALID for a vector no record set leaves: a bit count above its
 * cell's total, or a total of 2^54 and more. */
int kta_hot_keys_recover(const uint64_t *vec, uint32_t max_out, kta_hot_key *entries, uint32_t *n_out, uint64_t *keyed);
/* The exemplar table, copied to out[KTA_HOT_ROWS * KTA_HOT_CELLS] (staged messages are flushed first; waits for the
 * compute stream).  The exemplar of a reported hash h, x = fmix32(h), is in slot [0][x & 1023] or [1][(x >> 10) & 1023]
 * when one of them is valid and holds h. */
int kta_get_hot_key_exemplars(kta_ctx *ctx, kta_hot_exemplar *out, size_t n_slots);
/* Work counters of the hot-key pass since kta_create / kta_reset (profiling; waits for the compute stream): out[0]
 * keyed records, out[1] groups of lanes that added to LDS as one (a lane alone is a group), out[2] flushes of a
 * workgroup's LDS counters before its end (every workgroup of a launch makes the same number), out[3] launches, out[4]
 * exemplars captured, out[5] workgroups launched. */
int kta_hot_keys_info(kta_ctx *ctx, uint64_t out[6]);
/* Tests: the rounds (4096 records of a workgroup each) after which a workgroup flushes its LDS counters; 0 = the
 * default, the most the 21-bit fields admit (511).  KTA_ERR_INVALID above that. */
int kta_set_hot_flush_rounds(kta_ctx *ctx, uint32_t rounds);

/* Timestamp order (context created with KTA_FLAG_TS_ORDER; definition above KTA_FLAG_TS_ORDER).  The pass needs no key
 * columns.  kta_reset zeroes the vector and clears hi; kta_finish_device snapshots the vector.  Every call below that
 * takes a context fails on one without the flag with KTA_ERR_INVALID and a message naming KTA_FLAG_TS_ORDER.
 * The live accumulator, copied to out[n_u64] (n_u64 = 3 P + 64; staged messages are flushed first). */
int kta_get_ts_order(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* The SNAPSHOT that kta_finish_device (kta_finish, kta_exchange) takes, copied to out[n_u64]: after kta_exchange the
 * whole job's vector on every rank.  The live accumulator is never reduced, so a second exchange counts nothing twice. */
int kta_exchange_ts_order(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* Device pointer / length (u64) of that snapshot: what collectives (distributed.py) reduce in place. */
int kta_ts_order_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
/* Host-side merge of two vectors u64[3 P + 64] (acc <- acc (+) other): SUM over the first 2 P + 64 words, signed MAX over
 * the last P — what the two collectives of the exchange implement.  Precondition, as for the exchange: every partition's
 * records went through ONE of the two contexts, in order (and both were created with the same P and flags). */
int kta_merge_ts_order(uint64_t *acc, const uint64_t *other, uint32_t n_partitions);
/* The largest P a KTA_FLAG_TS_ORDER context may have (a wave of the apply kernel keeps run[P] in LDS). */
int kta_ts_order_max_partitions(void);
/* Work counters of the pass since kta_create / kta_reset (profiling; waits for the compute stream): out[0] launch triples
 * (chunk maxima, prefix, apply), out[1] chunks, out[2] wave instructions (64 records) that held a timestamped record,
 * out[3] of them on the one-partition path, out[4] colliding groups the general path resolved, out[5] the records per
 * chunk of the last launch triple. */
int kta_ts_order_info(kta_ctx *ctx, uint64_t out[6]);
/* Tests: records per chunk, a multiple of 64 (64 is the smallest); 0 = the default, by the length of the slice.
 * KTA_ERR_INVALID otherwise. */
int kta_set_ts_order_chunk(kta_ctx *ctx, uint64_t records);

/* Partitioner (context created with KTA_FLAG_PARTITIONER; definition above KTA_FLAG_PARTITIONER).  The handlers then read
 * key_off / key_bytes and val_len: the staging batches carry key columns as with count_alive_keys, and a device batch
 * handed to the metrics handler without them is refused (KTA_ERR_INVALID, "key columns missing (KTA_FLAG_PARTITIONER)")
 * before anything is launched.  kta_reset zeroes the vector and keeps Q; kta_finish_device snapshots the vector.  Every
 * call below that takes a context fails on one without the flag with KTA_ERR_INVALID and a message naming
 * KTA_FLAG_PARTITIONER.
 * The what-if partition count Q, 1 .. kta_partitioner_max_partitions() (KTA_ERR_INVALID otherwise, before anything is
 * launched or allocated).  Accepted only while the context has been handed no record since kta_create / kta_reset, as
 * kta_set_timeline; the vector, of 2 P + 2 Q words from then on, and its snapshot are zeroed. */
int kta_set_repartition(kta_ctx *ctx, uint32_t q);
/* The live accumulator, copied to out[n_u64] (n_u64 = 2 P + 2 Q; staged messages are flushed first). */
int kta_get_partitioner(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* The SNAPSHOT that kta_finish_device (kta_finish, kta_exchange) takes, copied to out[n_u64]: after kta_exchange the
 * whole job's vector on every rank.  The live accumulator is never reduced, so a second exchange counts nothing twice. */
int kta_exchange_partitioner(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* Device pointer / length (u64) of that snapshot: what collectives (distributed.py) reduce in place. */
int kta_partitioner_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
/* Host-side merge of two vectors u64[2 P + 2 Q] (acc <- acc + other, every word, modulo 2^64): what the collective of
 * the exchange implements.  KTA_ERR_INVALID for a P or Q of 0 or above the limit. */
int kta_merge_partitioner(uint64_t *acc, const uint64_t *other, uint32_t n_partitions, uint32_t q);
/* The largest P a KTA_FLAG_PARTITIONER context may have, and the largest Q (the pass keeps 8 P + 12 Q bytes in LDS). */
int kta_partitioner_max_partitions(void);
/* Work counters of the pass since kta_create / kta_reset (profiling; waits for the compute stream): out[0] keyed records,
 * out[1] launches, out[2] LDS adds to the checked / placed words and out[3] to the target words, both after the lanes of
 * an instruction that share a word were combined, out[4] workgroups launched, out[5] dynamic LDS bytes of a workgroup for
 * this P and Q. */
int kta_partitioner_info(kta_ctx *ctx, uint64_t out[6]);
/* Kafka's murmur2 of key[0, len) (host only; the source the device runs: csrc/kta_murmur2.h).  key may be null when
 * len is 0. */
uint32_t kta_murmur2(const void *key, size_t len);

/* Size percentiles (context created with KTA_FLAG_SIZE_QUANTILES; definition above KTA_FLAG_SIZE_QUANTILES).  The pass reads
 * partition, key_len and val_len in the tiles' own forms — no key columns, no timestamps, and nothing is widened for it.
 * kta_reset zeroes the vector; kta_finish_device snapshots it.  Every call below that takes a context fails on one without
 * the flag with KTA_ERR_INVALID and a message naming KTA_FLAG_SIZE_QUANTILES.
 * The live accumulator, copied to out[n_u64] (n_u64 = P * 3 * 464 + 8; staged messages are flushed first). */
int kta_get_size_quantiles(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* The SNAPSHOT that kta_finish_device (kta_finish, kta_exchange) takes, copied to out[n_u64]: after kta_exchange the
 * whole job's vector on every rank.  The live accumulator is never reduced, so a second exchange counts nothing twice. */
int kta_exchange_size_quantiles(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* Device pointer / length (u64) of that snapshot: what collectives (distributed.py) reduce in place. */
int kta_size_quantiles_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
/* Host-side merge of two vectors u64[P * 3 * 464 + 8] (acc <- acc + other, every word, modulo 2^64): what the collective
 * of the exchange implements.  KTA_ERR_INVALID for a P of 0 or above the limit. */
int kta_merge_size_quantiles(uint64_t *acc, const uint64_t *other, uint32_t n_partitions);
/* The largest P a KTA_FLAG_SIZE_QUANTILES context may have (a workgroup's LDS holds the counters of 28 partitions, and
 * every such slice of the topic streams the batch again). */
int kta_size_quantiles_max_partitions(void);
/* The pass's plan for this context and its work (profiling; staged messages are flushed first, waits for the compute
 * stream): out[0] S, the partitions of a slice, out[1] slices = ceil(P / S), out[2] dynamic LDS bytes of a workgroup,
 * out[3] threads of a workgroup, out[4] workgroups of the last launch (all slices), out[5] LDS adds issued since kta_create
 * / kta_reset, after the lanes of an instruction that share a word were combined. */
int kta_size_quantiles_info(kta_ctx *ctx, uint64_t out[6]);
/* Tests: S, the partitions of a slice, 1 .. 28 (0: the plan's own; more than P: P).  The result does not depend on it. */
int kta_set_size_quantiles_slice(kta_ctx *ctx, uint32_t partitions);
/* The bin of a size (host only; the source the device runs: csrc/kta_size_bins.h). */
uint32_t kta_size_bin(uint32_t size);
/* The least and the largest size of bin `bin` < KTA_SIZE_BINS (host only). */
int kta_size_bin_bounds(uint32_t bin, uint64_t *lo, uint64_t *hi);
/* The num/den quantile (num <= den, den > 0) of one histogram u64[KTA_SIZE_BINS] by nearest rank (host only): returns 1 and
 * the bounds of the answer's bin, 0 when the histogram is empty ("none": *lo and *hi are not written), KTA_ERR_INVALID for
 * bad arguments. */
int kta_size_quantile(const uint64_t *hist464, uint64_t num, uint64_t den, uint64_t *lo, uint64_t *hi);

/* Retention what-if (NOT in the reference; opt-in by call, like the timeline: kta_set_segments): the log segments of every
 * partition under a model of cleanup.policy=delete, from which "with retention.ms=X and / or retention.bytes=Y, how many
 * records and bytes does each partition keep" is answered on the host, exactly, for any number of policies after one pass.
 * The broker deletes whole segments, oldest first, and stops at the first one that must stay — an order-dependent,
 * per-partition, prefix-shaped rule; the pass computes, for every record, its position in its partition's log.
 *
 * Configuration: S = segment_bytes, 1 <= S <= 2^40 (any value, not only powers of two); M = rows_per_partition, 2 <= M and
 * P * M <= 2^20; overhead = record_overhead, a u32 added to every record's model size.
 * Records that take part: every record the metrics handler counts — `which & 1`, partition p in [0, P).  A record with a
 * partition outside [0, P) adds 1 to a global word and touches nothing else.  Records handed only to the alive-key handler
 * (which == 2) and the batches of a compaction replay touch nothing; a filtered context sees only the passing records.
 * Per-partition running state, in consumption order (batches as submitted, records by index) — device state, whose end
 * values are part of the result: C[p] records, B[p] bytes, T[p] tombstones, H[p] the largest timestamp among the records
 * with ts_ms >= 0, stored as H + 1 with 0 for none.  For a record of partition p with the size
 * z = overhead + max(key_len, 0) + max(val_len, 0) (as u64):
 *     s      = min(floor(B[p] / S), M - 1)          the segment its first byte falls into
 *     C[p] += 1;  B[p] += z;  T[p] += (val_len < 0);  if ts_ms >= 0: H[p] = max(H[p], ts_ms)
 *     s_next = min(floor(B[p] / S), M - 1)
 *     if s_next > s:   row[p][s] = { C[p], B[p], T[p], H[p] + 1 }      the record CLOSES segment s
 * Exactly one record closes a given row.  A record larger than S skips rows: they stay all zero, an empty segment.  Row
 * M - 1 never closes: it and the running state hold everything beyond the table.  H at a closing record is the running
 * maximum over the whole partition up to there, not the segment's own: "segment k and all before it are older than the
 * cut" is exactly "the running maximum at the end of k is older than the cut".
 * The vector, u64[(P*M + P) * 4 + 8]: the rows [p*M + s][4], the totals [P][4] (the running state, H + 1 in word 3), eight
 * globals: records counted, records with a partition outside [0, P), rows closed, S, M, overhead, two zero words.
 * Merging: every word except the three configuration globals is a SUM; vectors merge exactly when every partition's records
 * went through ONE context in order (non-owners hold zeros); the configuration globals must agree (kta_merge_segments
 * refuses a mismatch).
 * Identities with the counter vector of the same records: totals[p].C == total[p], totals[p].T == tombstones[p],
 * totals[p].B - overhead * totals[p].C == key_size_sum[p] + value_size_sum[p], global 0 == KTA_G_RECORDS (which counts
 * the records with a partition in [0, P) only), global 1 == KTA_G_BAD_PARTITION.
 * The what-if (kta_retention_whatif), a pure host function of the vector, now_ms, retention_ms and retention_bytes (-1: the
 * rule is off): per partition, walk the closed, non-empty rows oldest first.  A closed row k with end values E_k is deleted
 * when every earlier closed row is deleted and at least one of
 *     time: E_k.H exists and now_ms - E_k.H > retention_ms;     size: totals.B - E_k.B >= retention_bytes
 * holds (the latter is what Kafka's `diff - segment.size >= 0` loop amounts to).  The walk stops at the first row neither
 * rule takes; the open tail is the active segment, which the model never deletes.
 * Model limits: the rolling rule is "the record's first byte falls into the segment", which is prefix-computable — not the
 * broker's greedy "roll when the batch would not fit" — so a boundary can differ by at most one record per segment;
 * segment.ms rolling is not modelled; sizes are key + value + overhead, not bytes on disk (no batch headers, no
 * compression); a prefix without any timestamp is not deleted by time.  B is a u64 and is taken not to wrap.
 *
 * kta_set_segments turns the pass on (or re-configures it): refused (KTA_ERR_INVALID) once the context has been handed a
 * record since kta_create / kta_reset, outside the bounds above, and with more than kta_segments_max_partitions()
 * partitions.  kta_reset keeps the configuration and zeroes the vector with its running state. */
int kta_set_segments(kta_ctx *ctx, uint64_t segment_bytes, uint32_t rows_per_partition, uint32_t record_overhead);
/* u64 words of the vector for P partitions and M rows: (P*M + P) * 4 + 8, below 2^24 (0 outside the bounds). */
uint32_t kta_segments_words(uint32_t n_partitions, uint32_t rows_per_partition);
/* The live vector, copied to out[n_u64] (n_u64 = kta_segments_words(P, M); staged messages are flushed first). */
int kta_get_segments(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* The SNAPSHOT that kta_finish_device (kta_finish, kta_exchange) takes, copied to out[n_u64]: after kta_exchange the
 * whole job's vector on every rank — exact when every partition's records went through ONE rank in order, as kta.gpus=N
 * shards (the timestamp-order pass's precondition).  The grouped launch of kta_exchange reduces every word with SUM but
 * the last five (S, M, overhead, two zero words), which it reduces with MAX: equal on every rank, they stay what they
 * are.  The live vector is never reduced, so a second exchange counts nothing twice. */
int kta_exchange_segments(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* Device pointer / length (u64) of that snapshot: what collectives (distributed.py) reduce in place. */
int kta_segments_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
/* The largest P a context with segments may have (a wave of the apply kernel keeps 41 B per partition in LDS). */
int kta_segments_max_partitions(void);
/* Work counters of the pass since kta_create / kta_reset (profiling; staged messages are flushed first, waits for the
 * compute stream): out[0] chunks, out[1] records of the last launch triple's chunk, out[2] launch triples, out[3] chunks
 * the apply kernel ran its wave step over, out[4] chunks it skipped because no partition crossed a segment boundary in
 * them, out[5] colliding groups the wave step resolved. */
int kta_segments_info(kta_ctx *ctx, uint64_t out[6]);
/* Tests: records per chunk, a multiple of 64 (0: by the slice's length).  The result does not depend on it. */
int kta_set_segments_chunk(kta_ctx *ctx, uint64_t records);
/* Host-side merge of two vectors u64[kta_segments_words(P, M)] (acc <- acc + other, every word but S, M, overhead, modulo
 * 2^64).  KTA_ERR_INVALID for bad bounds, and when the two configurations differ (acc is then as it was). */
int kta_merge_segments(uint64_t *acc, const uint64_t *other, uint32_t n_partitions, uint32_t rows_per_partition);
/* The what-if over a vector (pure host; needs no device): out[(P + 1)][KTA_RETENTION_WORDS], a row per partition and one
 * for the topic (sums; its rule word is the OR of the partitions', its clamped word their count):
 *   [0] segments (closed non-empty rows, + 1 if the open tail holds a record), [1] records, [2] bytes, [3] tombstones now,
 *   [4] records, [5] bytes, [6] tombstones kept, [7] segments deleted, [8] rule: 0 nothing deleted, 1 the time rule reached
 *   at least as far as the size rule, 2 the size rule further, [9] the partition outgrew its M rows
 *   (floor(totals.B / S) >= M - 1: the last row holds the rest and is treated as active).
 * retention_ms / retention_bytes: -1 turns the rule off; values below -1 are KTA_ERR_INVALID. */
#define KTA_RETENTION_WORDS 10
int kta_retention_whatif(const uint64_t *vec, uint32_t n_partitions, uint32_t rows_per_partition, int64_t now_ms, int64_t retention_ms,
                         int64_t retention_bytes, uint64_t *out, size_t n_u64);

/* Record batches (context created with KTA_FLAG_RECORD_BATCHES; definition above KTA_FLAG_RECORD_BATCHES).  kta_reset zeroes
 * the vector; kta_finish_device snapshots it; kta_exchange reduces the snapshot (SUM prefix, MAX suffix).  Every call below
 * that takes a context fails on one without the flag with KTA_ERR_INVALID and a message naming KTA_FLAG_RECORD_BATCHES.
 * The live accumulator, copied to out[n_u64] (n_u64 = KTA_RB_WORDS(P); staged messages are flushed first). */
int kta_get_record_batches(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* The SNAPSHOT that kta_finish_device (kta_finish, kta_exchange) takes, copied to out[n_u64]: after kta_exchange the whole
 * job's vector on every rank.  The live accumulator is never reduced, so a second exchange counts nothing twice. */
int kta_exchange_record_batches(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* Device pointer / length (u64) of that snapshot (what collectives reduce in place), and of the live vector. */
int kta_record_batches_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
int kta_record_batches_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
/* Host-side merge of two vectors u64[KTA_RB_WORDS(P)]: acc <- acc + other over the SUM prefix, max(acc, other) behind it.
 * KTA_ERR_INVALID for a P outside [1, 4096]. */
int kta_merge_record_batches(uint64_t *acc, const uint64_t *other, uint32_t n_partitions);
/* The number of distinct producer ids read off a vector's sketch (host only): HyperLogLog's estimate with linear counting
 * while it is small and registers are empty; 0 for an empty sketch. */
int kta_record_batches_estimate_producers(const uint64_t *vec, uint32_t n_partitions, double *out);
/* 1 when the identities between the words of one vector hold, 0 when not (host only). */
int kta_record_batches_identities(const uint64_t *vec, uint32_t n_partitions);
/* The same rule on the host, for tests (the product accumulates on the device only): the batches that kta_kafka_index_host
 * finds in bytes[0, len) of `partition` are added to vec[KTA_RB_WORDS(P)].  inflated: one exact inflated size per
 * descriptor, or NULL to take the index's own value (exact for no codec, gzip and Snappy; a bound for LZ4 and zstd). */
int kta_record_batches_host(const uint8_t *bytes, uint64_t len, int32_t partition, const uint64_t *inflated, uint64_t *vec,
                            uint32_t n_partitions);

/* Payload (context created with KTA_FLAG_PAYLOAD; definition above KTA_FLAG_PAYLOAD).  kta_reset zeroes the vector;
 * kta_finish_device snapshots it; kta_exchange reduces the snapshot (all SUM).  Every call below that takes a context fails
 * on one without the flag with KTA_ERR_INVALID and a message naming KTA_FLAG_PAYLOAD.
 * The live accumulator, copied to out[n_u64] (n_u64 = KTA_PAYLOAD_WORDS(P); staged messages are flushed first). */
int kta_get_payload(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* The SNAPSHOT that kta_finish_device (kta_finish, kta_exchange) takes, copied to out[n_u64]: after kta_exchange the whole
 * job's vector on every rank.  The live accumulator is never reduced, so a second exchange counts nothing twice. */
int kta_exchange_payload(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* Device pointer / length (u64) of that snapshot (what collectives reduce in place), and of the live vector. */
int kta_payload_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
int kta_payload_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
/* Host-side merge of two vectors u64[KTA_PAYLOAD_WORDS(P)]: acc <- acc + other.  KTA_ERR_INVALID for a P outside [1, 4096]. */
int kta_merge_payload(uint64_t *acc, const uint64_t *other, uint32_t n_partitions);
/* 1 when the identities between the words of one vector hold, 0 when not (host only): the class counts sum to the records
 * and the bytes of null and empty are 0, per partition; the histogram sums to records - bad_headers and its bin 0 equals
 * records - with_headers - bad_headers, over the topic; each table row's T and B sum to the framed records and bytes; no bit
 * counter exceeds its cell's T.  counter_vec: NULL, or the counter vector u64[7 P + 8] of the same UNFILTERED run without
 * failed batches: records == total_messages (which includes the tombstones) and null == tombstones, per partition. */
int kta_payload_identities(const uint64_t *vec, const uint64_t *counter_vec, uint32_t n_partitions);
/* The schema ids read off a vector's table (host only), sorted by records (most first), then bytes, then id: *n of them,
 * the first min(*n, cap) in ids / records / bytes (cap 0: the arrays may be NULL).  A cell is PURE when T > 0, every bit
 * counter is 0 or T and the id so spelled maps to this cell in this row; a pure cell gives its id's exact records and bytes.
 * A recovered id is peeled — subtracted from its cell in the other row — and the rows are looked at again until nothing
 * changes (an invertible Bloom lookup table: what it lists is exact).  *unresolved_records / *unresolved_bytes (may be NULL):
 * what then remains in row 0, the records in cells that hold several ids — reported, never guessed at. */
int kta_payload_schema_ids(const uint64_t *vec, uint32_t n_partitions, uint32_t *ids, uint64_t *records, uint64_t *bytes, size_t cap,
                           size_t *n, uint64_t *unresolved_records, uint64_t *unresolved_bytes);
/* The same rule on the host, for tests and the CPU suite (the product accumulates on the device only): the records of the
 * batches that kta_kafka_index_host finds in bytes[0, len) of `partition` are added to vec[KTA_PAYLOAD_WORDS(P)];
 * compressed batches are inflated with kta_*_inflate_host.  A partition outside [0, P) adds nothing.  No filter. */
int kta_payload_host(const uint8_t *bytes, uint64_t len, int32_t partition, uint64_t *vec, uint32_t n_partitions);

/* Header names (context created with KTA_FLAG_HEADER_NAMES; definition above KTA_FLAG_HEADER_NAMES).  kta_reset zeroes the
 * vector and the name table; kta_finish_device snapshots the vector; kta_exchange reduces the snapshot (all SUM).  Every call
 * below that takes a context fails on one without the flag with KTA_ERR_INVALID and a message naming KTA_FLAG_HEADER_NAMES.
 * The live accumulator, copied to out[n_u64] (n_u64 = KTA_HEADER_NAMES_WORDS; staged messages are flushed first). */
int kta_get_header_names(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* The SNAPSHOT that kta_finish_device (kta_finish, kta_exchange) takes: after kta_exchange the whole job's vector on every rank. */
int kta_exchange_header_names(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* Device pointer / length (u64) of that snapshot (what collectives reduce in place), and of the live vector. */
int kta_header_names_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
int kta_header_names_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
/* Host-side merge of two vectors u64[KTA_HEADER_NAMES_WORDS]: acc <- acc + other. */
int kta_merge_header_names(uint64_t *acc, const uint64_t *other);
/* This context's name table, copied to out[n_slots] (n_slots = KTA_HEADER_NAMES_SLOTS); a slot that is not published comes
 * back zeroed. */
int kta_get_header_name_table(kta_ctx *ctx, kta_header_name *out, size_t n_slots);
/* 1 when the identities between the words of one vector hold, 0 when not (host only): the two zero words are zero; each
 * row's T, L, V and Z sum to the globals; no bit counter exceeds its cell's T.  payload_vec: NULL, or the payload vector
 * u64[KTA_PAYLOAD_WORDS(P)] of the same run: occurrences, name bytes, value bytes, null values and records with headers
 * equal the sums over the partitions of headers, header_key_bytes, header_value_bytes, header_null_values and
 * with_headers, and the records looked at equal records - bad_headers. */
int kta_header_names_identities(const uint64_t *vec, const uint64_t *payload_vec, uint32_t n_partitions);
/* The names read off a vector's table (host only) by the peel of kta_payload_schema_ids, where a pure cell's L must also be
 * a multiple of its T: *n rows, the first min(*n, cap) in rows (cap 0: rows may be NULL), sorted by occurrences (most first),
 * then value bytes, then hash.  table: NULL, or a name table kta_header_name[KTA_HEADER_NAMES_SLOTS]; a row has its name when
 * a published slot of either of its cells holds its hash.  *unresolved_occurrences / *unresolved_value_bytes (may be NULL):
 * what then remains in row 0, the occurrences in cells that hold several names — reported, never guessed at. */
int kta_header_names_list(const uint64_t *vec, const kta_header_name *table, kta_header_name_row *rows, size_t cap, size_t *n,
                          uint64_t *unresolved_occurrences, uint64_t *unresolved_value_bytes);
/* The same rule on the host, for tests and the CPU suite, as kta_payload_host: added to vec[KTA_HEADER_NAMES_WORDS] and, when
 * not NULL, to table[KTA_HEADER_NAMES_SLOTS] (first writer wins).  A partition outside [0, P) adds nothing.  No filter. */
int kta_header_names_host(const uint8_t *bytes, uint64_t len, int32_t partition, uint64_t *vec, kta_header_name *table, uint32_t n_partitions);

/* Value bytes (context created with KTA_FLAG_VALUE_BYTES; definition above KTA_FLAG_VALUE_BYTES).  kta_reset zeroes the
 * vector; kta_finish_device snapshots it; kta_exchange reduces the snapshot (all SUM).  Every call below that takes a context
 * fails on one without the flag with KTA_ERR_INVALID and a message naming KTA_FLAG_VALUE_BYTES.
 * The live accumulator, copied to out[n_u64] (n_u64 = KTA_VALUE_BYTES_WORDS(P); staged messages are flushed first). */
int kta_get_value_bytes(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* The SNAPSHOT that kta_finish_device (kta_finish, kta_exchange) takes: after kta_exchange the whole job's vector on every rank. */
int kta_exchange_value_bytes(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* Device pointer / length (u64) of that snapshot (what collectives reduce in place), and of the live vector. */
int kta_value_bytes_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
int kta_value_bytes_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
/* Host-side merge of two vectors u64[KTA_VALUE_BYTES_WORDS(P)]: acc <- acc + other. */
int kta_merge_value_bytes(uint64_t *acc, const uint64_t *other, uint32_t n_partitions);
/* 1 when the identities between the words of one vector hold, 0 when not (host only), per partition: the bins sum to bytes;
 * repeats <= bytes - values; values <= records; words 260 .. 263 are zero.  payload_vec: NULL, or the payload vector
 * u64[KTA_PAYLOAD_WORDS(P)] of the same run: records equal the payload's records, bytes the sum of its five class-byte words,
 * values its framed + json + other.  counter_vec: NULL, or the counter vector of the same unfiltered run without failed
 * batches, as kta_payload_identities takes it: records equal the total messages. */
int kta_value_bytes_identities(const uint64_t *vec, uint32_t n_partitions, const uint64_t *payload_vec, const uint64_t *counter_vec);
/* The read-off of words[KTA_VALUE_BYTES_PARTITION_WORDS]: one partition's words, or their sum over the topic (host only). */
int kta_value_bytes_summary(const uint64_t *words, kta_value_bytes_summary_t *out);
/* The same rule on the host, for tests and the CPU suite, as kta_payload_host: added to vec[KTA_VALUE_BYTES_WORDS(P)].  A
 * partition outside [0, P) adds nothing.  No filter. */
int kta_value_bytes_host(const uint8_t *bytes, uint64_t len, int32_t partition, uint64_t *vec, uint32_t n_partitions);

/* Compression what-if (context created with KTA_FLAG_COMPRESS_WHATIF; definition above KTA_FLAG_COMPRESS_WHATIF).  kta_reset
 * zeroes the vector; kta_finish_device snapshots it; kta_exchange reduces the snapshot (all SUM).  Every call below that
 * takes a context fails on one without the flag with KTA_ERR_INVALID and a message naming KTA_FLAG_COMPRESS_WHATIF.
 * The live accumulator, copied to out[n_u64] (n_u64 = KTA_COMPRESS_WHATIF_WORDS(P); staged messages are flushed first). */
int kta_get_compress_whatif(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* The SNAPSHOT that kta_finish_device (kta_finish, kta_exchange) takes: after kta_exchange the whole job's vector on every rank. */
int kta_exchange_compress_whatif(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* Device pointer / length (u64) of that snapshot (what collectives reduce in place), and of the live vector. */
int kta_compress_whatif_result_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
int kta_compress_whatif_vector(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
/* Host-side merge of two vectors u64[KTA_COMPRESS_WHATIF_WORDS(P)]: acc <- acc + other. */
int kta_merge_compress_whatif(uint64_t *acc, const uint64_t *other, uint32_t n_partitions);
/* 1 when the identities between the words of one vector hold, 0 when not (host only): the codec table's sums equal the
 * partitions' sums; per partition stored_blocks <= blocks, match_bytes <= raw_bytes, model_bytes <= raw_bytes + 11 batches +
 * 4 blocks, match_bytes >= 4 sequences. */
int kta_compress_whatif_identities(const uint64_t *vec, uint32_t n_partitions);

/* Compaction what-if (context created with KTA_FLAG_COMPACTION; definition above KTA_FLAG_COMPACTION).  In replay mode a
 * device batch without key columns is refused (KTA_ERR_INVALID, "key columns missing (KTA_FLAG_COMPACTION)") before
 * anything is launched.  The vector is the context's own: kta_finish_device takes no snapshot of it and no exchange reduces
 * it.  Every call below that takes a context fails on one without the flag with KTA_ERR_INVALID and a message naming
 * KTA_FLAG_COMPACTION.
 * Replay mode on (non-zero) or off (0); setting the mode it is in does nothing. */
int kta_compaction_replay(kta_ctx *ctx, int on);
/* The live vector, copied to out[n_u64] (n_u64 = 5 P + 6; staged messages are flushed first). */
int kta_get_compaction(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* The largest P a KTA_FLAG_COMPACTION context may have (the pass keeps 32 P bytes in LDS). */
int kta_compaction_max_partitions(void);
/* Work counters of the pass since kta_create / kta_reset (profiling; waits for the compute stream): out[0] keyed records
 * looked at (one table read each), out[1] launches, out[2] workgroups launched, out[3] LDS adds (survivors only),
 * out[4] dynamic LDS bytes of a workgroup for this P, out[5] reserved, 0. */
int kta_compaction_info(kta_ctx *ctx, uint64_t out[6]);

/* Compact,delete what-if (opt-in; joins the compaction replay with the segments of kta_set_segments): what a topic with
 * cleanup.policy=compact,delete would keep.  During a replay (kta_compaction_replay) every record whose partition lies in
 * [0, P) advances its partition's kept state {L, B, T, K}: with z the record's model size (as kta_set_segments defines it),
 * B += z for every record — its position, the sum the first pass's segment state holds —, L += 1 and K += z for a live
 * survivor, T += 1 and K += z for a tombstone that survives; unkeyed, superseded and unknown records add to B only.  A
 * record that closes row s (the rule of kta_set_segments) stores the kept state as it is after that record in kept row
 * [p][s].  The kept vector has the segment vector's shape u64[kta_segments_words(P, M)]: rows, totals — the running state,
 * which carries from batch to batch within a replay —, then the globals: records taking part, records outside [0, P), rows
 * closed, S, M, overhead, 0, 0.  With the first pass's segment vector and the replay's compaction vector it satisfies:
 * globals 0-5 equal the segment vector's; totals.B and every closed row's B equal the segment vector's, and the same rows
 * are closed; totals.L / totals.T are the compaction vector's live / tombstone records; totals.K = overhead * (L + T) + live
 * key bytes + live value bytes + tombstone key bytes; L, T and K do not decrease down a partition's closed rows.
 *
 * kta_set_compact_delete: on (non-zero) or off (0).  KTA_ERR_INVALID for a context without KTA_FLAG_COMPACTION, without
 * kta_set_segments, one that has been handed a record since kta_create / kta_reset, or with more than
 * kta_compact_delete_max_partitions() partitions (the smaller of the two passes' bounds).  kta_set_segments turns it off:
 * call it after.  kta_comm_create with nranks > 1 refuses such a context, as it refuses every KTA_FLAG_COMPACTION one.
 * With the switch off a replay writes what it wrote before and nothing else.  kta_reset and kta_compaction_replay(ctx, 1)
 * zero the kept vector but for its configuration words. */
int kta_set_compact_delete(kta_ctx *ctx, int on);
int kta_compact_delete_max_partitions(void);
/* The live kept vector, copied to out[n_u64] (n_u64 = kta_segments_words(P, M); staged messages are flushed first). */
int kta_get_compact_delete(kta_ctx *ctx, uint64_t *out, size_t n_u64);
/* Work counters of the kept-row kernels since kta_set_compact_delete / kta_reset / the replay's start (profiling; waits for
 * the compute stream): out[0] launches, out[1] chunks, out[2] chunks the apply kernel went through (the others closed no
 * row), out[3] bytes of the class column (a byte per record of the largest replay slice, at most 128 MiB). */
int kta_compact_delete_info(kta_ctx *ctx, uint64_t out[4]);
/* The what-if (pure host; needs no device) from the first pass's segment vector, the replay's kept vector and the replay's
 * compaction vector u64[5 P + 6].  Per partition the closed rows are walked oldest first, as kta_retention_whatif walks
 * them; `last` is the last closed row, `klast` its kept row (zeros without one); the active segment A = totals - last of
 * the segment vector is never cleaned and never deleted; the compacted log is klast plus A.  Row k is deleted by the time
 * rule as in kta_retention_whatif (H is the first pass's running maximum over all records: a cleaned segment's own largest
 * timestamp can only be older, so the model keeps at least what the broker keeps), by the size rule when retention_bytes
 * >= 0 and (klast.K + A.B) - kept[k].K >= retention_bytes (compacted sizes).  Both take a prefix; `cut` is the last row
 * deleted.  out[(P + 1)][KTA_COMPACT_DELETE_WORDS], a row per partition and one for the topic (sums; its rule word is the
 * OR of the partitions', its clamped word their count):
 *   [0] records, [1] bytes now; [2] records, [3] bytes after compaction alone: klast.L + klast.T + A.C, klast.K + A.B;
 *   [4] records, [5] bytes under compact,delete: [2] - (kcut.L + kcut.T), [3] - kcut.K; [6] tombstones among [4]:
 *   klast.T - kcut.T + A.T; [7] segments deleted; [8] rule and [9] clamped as kta_retention_whatif's [8] and [9].
 * KTA_ERR_INVALID for bad arguments, and when an identity above fails or the compaction vector's unknown != 0: the replay
 * did not match the first pass. */
#define KTA_COMPACT_DELETE_WORDS 10
int kta_compact_delete_whatif(const uint64_t *seg_vec, const uint64_t *kept_vec, const uint64_t *comp_vec, uint32_t n_partitions,
                              uint32_t rows_per_partition, int64_t now_ms, int64_t retention_ms, int64_t retention_bytes, uint64_t *out,
                              size_t n_u64);

/* ---- alive-key table access (tests, multi-GPU merge) ------------------------------ */
/* Export the alive set as a 2^32-bit little-endian bitmap (bit h%32 of u32 word h/32;
 * 512 MiB) into host memory — the same layout as BitSet's storage (metric.rs:263). */
int kta_export_alive_bitmap(kta_ctx *ctx, void *dst_host_512MiB);
/* Device pointer of the last-writer table: u64[2^32], entry = ((seq+1)<<1)|alive, 0 = never
 * written.  Element-wise MAX across GPUs merges shards exactly (then call
 * kta_alive_table_modified).  sum_all_alive is normally kept as a running count by the update
 * kernel (returning atomicMax: +flag(new) - flag(old) whenever an entry is replaced), so
 * kta_finish does not scan the table. */
int kta_alive_table(kta_ctx *ctx, void **device_ptr, size_t *n_u64);
/* Compact exchange of the table between partition-sharded GPUs.  Export: the entries ever written
 * (value != 0) as device arrays slot u32[n] / value u64[n] (owned by the context, valid until the
 * next export); at most one per distinct key hash the shard has seen, i.e. 12 bytes per key instead
 * of the 32 GiB table.  Import: table[slot] = max(table[slot], value) for foreign entries (device
 * pointers), keeping the running alive count exact.  Importing every other shard's export into one
 * context reproduces the global last-writer state. */
int kta_alive_export_entries(kta_ctx *ctx, void **d_slots, void **d_vals, uint64_t *n);
int kta_alive_import_entries(kta_ctx *ctx, const void *d_slots, const void *d_vals, uint64_t n);
/* Alive keys whose hash slot lies in [slot_lo, slot_hi) (0 <= lo <= hi <= 2^32): the share of the owner
 * of a hash range after the hash-range exchange of a multi-GPU run (distributed.py,
 * exchange_alive_by_hash_range; SURVEY section 8(e) option ii).  Synchronous. */
int kta_alive_count_range(kta_ctx *ctx, uint64_t slot_lo, uint64_t slot_hi, uint64_t *count);

/* Tell the context that the table was changed behind its back (e.g. merged with other GPUs' tables
 * by an all-reduce MAX): the running alive count is dropped and the next kta_finish recounts by
 * scanning the table. */
int kta_alive_table_modified(kta_ctx *ctx);
/* Hash `n` keys on the device with the reference's FNV variant (fnv32.rs:92-101). */
int kta_fnv32_device(kta_ctx *ctx, const uint8_t *key_bytes_host, const uint32_t *key_off_host,
                     const int32_t *key_len_host, uint64_t n, uint64_t n_key_bytes,
                     uint32_t *hash_out_host);

/* ---- report -------------------------------------------------------------------------- */
/* Render what the reference prints after the scan (src/main.rs:123-178) from a counter vector:
 * the text block, chrono's `DateTime<Utc>` Display, `{:.4}` of the f32 dirty ratio and the
 * prettytable.  `now_*` stands in for Utc::now() at MessageMetrics::new (metric.rs:39);
 * start/end offsets may be NULL (0 / per-partition record count).  *out_len receives the full
 * length; the text is truncated to out_cap-1 bytes + NUL.  Returns KTA_ERR_DIV_BY_ZERO where
 * the reference panics (a partition with key bytes but no alive record, metric.rs:135) and
 * KTA_ERR_TIMESTAMP_RANGE, without a text, for a vector the reference could not have produced (above). */
int kta_render_report(const char *topic, uint64_t duration_secs, const uint64_t *vec,
                      uint32_t n_partitions, int count_alive_keys, int64_t now_sec, uint32_t now_ns,
                      const int64_t *start_offsets, const int64_t *end_offsets, char *out,
                      size_t out_cap, size_t *out_len);

/* The opt-in analytics section that kta-analyzer prints after the reference report (--librdkafka
 * kta.analytics=1), from an analytics vector: a title line saying that it is not part of the reference report,
 * a size table (Bytes | Keys | Keys % | Values | Vals %: rows None and 0 always, then each log2 bucket whose key
 * or value count is non-zero; percentages of all records, %.2f), a per-partition table (P | Earliest | Latest |
 * Smallest | Largest: times in seconds as the report's Earliest Message, `-` for a partition without records /
 * without non-tombstones) and a closing `=` rule.  Output buffer conventions as kta_render_report. */
int kta_render_analytics(const uint64_t *vec, uint32_t n_partitions, char *out, size_t out_cap, size_t *out_len);

/* The opt-in timeline section that kta-analyzer prints after the reference report (and after the analytics section)
 * with --librdkafka kta.timeline=<width>, from a timeline vector u64[(n_buckets + 3) * 3] (host only, no device):
 * a title line saying that it is not part of the reference report with the width and the start, a table
 * (From | Records | Records % | Tmb | Bytes) whose rows "No timestamp", "Before <start>" and "After <end>" are always
 * printed and whose bucket rows, labelled with their start (format of the report's Earliest Message), run from the
 * first to the last non-empty bucket; percentages of all timeline records, %.2f; then a closing `=` rule.
 * Output buffer conventions as kta_render_report. */
int kta_render_timeline(const uint64_t *vec, int64_t origin_ms, int64_t bucket_ms, uint32_t n_buckets, char *out,
                        size_t out_cap, size_t *out_len);

/* The opt-in key sketch section that kta-analyzer prints after the reference report (and after the analytics and
 * timeline sections) with --librdkafka kta.distinct_keys=1, from a sketch vector u64[P * 4096] and the counter vector
 * u64[P * 7 + 8] of the same records (host only): a title line that gives the method and its standard error and says
 * that it is not part of the reference report, a table (P | Keyed records | Distinct keys | Records per key: keyed
 * records = key_non_null, distinct keys = the estimate rounded to an integer, records per key %.2f; `-` for a partition
 * without keyed records), a topic row with the topic-wide estimate, and a closing `=` rule.  Output buffer conventions
 * as kta_render_report. */
int kta_render_distinct_keys(const uint64_t *sketch_vec, const uint64_t *counter_vec, uint32_t n_partitions, char *out,
                             size_t out_cap, size_t *out_len);

/* The opt-in hot-key section that kta-analyzer prints after the reference report (and after the other opt-in sections)
 * with --librdkafka kta.hot_keys=K (1 <= K <= KTA_HOT_MAX_REPORTED), from a hot-key vector and an exemplar table
 * (kta_hot_exemplar[2048], or NULL for none; host only): a title line that names the method and says that it is not
 * part of the reference report, a table (# | Key | Hash | Records (at most) | (at least) | Share of keyed records: the
 * key's first 32 bytes with printable ASCII except the backslash as is and every other byte as \xNN, `...` behind a
 * longer key, `-` without an exemplar; the hash as 8 hex digits; the share is the upper bound's, %.2f) and a closing
 * `=` rule.  When no key is reported: the title and one line saying so.  Output buffer conventions as
 * kta_render_report. */
int kta_render_hot_keys(const uint64_t *vec, const kta_hot_exemplar *exemplars, uint32_t max_keys, char *out,
                        size_t out_cap, size_t *out_len);

/* The opt-in timestamp-order section that kta-analyzer prints after the reference report (and after the analytics,
 * timeline and distinct-key sections, before the hot keys) with --librdkafka kta.ts_order=1, from a timestamp-order vector
 * u64[3 P + 64] and the counter vector u64[P * 7 + 8] of the same records (host only): a title line saying that it is not
 * part of the reference report; a table (P | Records | Late records | Late % | Mean lateness ms | Max lateness ms: Records
 * = total_messages, Late % of them, %.2f; the mean is late_ms_sum / late, truncating; `-` for the mean and the max of a
 * partition without a late record); a Topic row; a line `Records without a timestamp: ` total - timed; unless no record is
 * late (one line saying so), a table (Late by | Records | Cumulative %) from the first to the last non-empty histogram
 * bucket, rows labelled `< 2^(k+1) ms` written as a number, Cumulative % the share of the timestamped records that are in
 * order or late by less than the row's bound (%.2f): the figure a grace period is read from; a closing `=` rule.
 * Output buffer conventions as kta_render_report. */
int kta_render_ts_order(const uint64_t *vec, const uint64_t *counter_vec, uint32_t n_partitions, char *out, size_t out_cap,
                        size_t *out_len);

/* The opt-in partitioner section that kta-analyzer prints last of all (after the hot keys) with --librdkafka
 * kta.partitioner=murmur2, from a partitioner vector u64[2 P + 2 Q] and the counter vector u64[P * 7 + 8] of the same
 * records (host only).  Percentages are %.2f, ratios %.2f, `-` where the denominator is 0.
 *   `Partitioner check: keyed records on the partition Kafka's default partitioner (murmur2) gives their key
 *    (kta.partitioner=murmur2; not part of the reference report)` — one line;
 *   a table (P | Keyed records | On murmur2's partition | %) with a row per partition — `-` in the last two columns of a
 *    partition without keyed records — and a Topic row;
 *   `Records without a key: N (the default partitioner spreads them without a hash)`, N the sum of key_null;
 *   the verdict, one of
 *    `No record has a key: nothing to check.`                                                  (no keyed record)
 *    `All keyed records lie on murmur2's partition: the topic is keyed as Kafka's default partitioner keys it.`
 *    `No more keyed records lie on murmur2's partition than chance puts there (X % against 1/P = Y %): the topic was not
 *     written by Kafka's default partitioner with P partitions.`       (P > 2 and placed * P <= 2 * checked; one line)
 *    `X % of the keyed records lie on murmur2's partition: the topic is only partly keyed as Kafka's default partitioner
 *     keys it.`                                                                                            (one line)
 *   `Repartition what-if: the keyed records over Q = <Q> partitions by murmur2`;
 *   a table (Target | Records | Records % | Bytes | Bytes %) over the Q targets, the shares of the sums over the targets;
 *   `Largest / mean at Q = <Q>: records A, bytes B; the topic as it is (P = <P>): records C, bytes D` — A and B over the
 *    targets, C over key_non_null[p], D over key_size_sum[p] + value_size_sum[p] of the counter vector;
 *   a closing `=` rule.
 * Output buffer conventions as kta_render_report. */
int kta_render_partitioner(const uint64_t *vec, const uint64_t *counter_vec, uint32_t n_partitions, uint32_t q, char *out,
                           size_t out_cap, size_t *out_len);
/* The opt-in size-percentile section that kta-analyzer prints after the report's closing rule (and after the analytics
 * section) with --librdkafka kta.percentiles=1, from a size vector u64[P * 3 * 464 + 8] and the counter vector
 * u64[P * 7 + 8] of the same records (host only):
 *   `Size percentiles per partition, in bytes (kta.percentiles=1; not part of the reference report)` — one line;
 *   three times a line `Key sizes` / `Value sizes` / `Message sizes (key + value of the non-tombstones)` and a table
 *    (P | Count | p50 | p90 | p99 | p99.9 | Max) with a row per partition and a last row `All`, the sum over the
 *    partitions: Count is the histogram's count, a percentile the hi of kta_size_quantile's bin at 50/100, 90/100, 99/100,
 *    999/1000, Max the hi of the last bin that is not empty; `-` where the count is zero;
 *   `Sizes below 32 B are exact; a size of 32 B and more is the upper end of its bin, at most 6.25 % wide.`;
 *   a closing `=` rule.
 * KTA_ERR_INVALID, and nothing written, when the identities above KTA_FLAG_SIZE_QUANTILES do not hold between the two
 * vectors.  Output buffer conventions as kta_render_report. */
int kta_render_size_percentiles(const uint64_t *vec, const uint64_t *counter_vec, uint32_t n_partitions, char *out, size_t out_cap,
                                size_t *out_len);
/* The opt-in compaction section that kta-analyzer prints after the partitioner section and before the filter section with
 * -c --librdkafka kta.compaction=1, from a compaction vector u64[5 P + 6] and the counter vector u64[P * 7 + 8] of the
 * first pass (host only).  Shares are %.2f, `n/a` where the denominator is 0.
 *   `Compaction what-if: the records and bytes log compaction would keep (kta.compaction=1; not part of the reference
 *    report)` — one line;
 *   a table (P | Records | Kept | Live | Tombstones | Records reclaimed % | Bytes | Bytes kept | Bytes reclaimed %) with a
 *    row per partition and a Topic row: Records is total_messages, Bytes key_size_sum + value_size_sum of the counter
 *    vector, Kept = Live + Tombstones, Bytes kept = live key + live value + tombstone key bytes, reclaimed = 1 - kept / now;
 *   `Records without a key: N (not kept: compaction goes by key)`, N the vector's unkeyed;
 *   `Kept outside the partition range: L live, T tombstones` when either is non-zero;
 *   `Keys are counted by 32-bit hash slot, topic-wide, as "Alive keys" is: a key written to several partitions is kept once.`;
 *   a closing `=` rule.
 * When unknown != 0, or replayed differs from the counter vector's records plus bad-partition records, the replay did not
 * match the first pass: the section is the first line, `The replay did not match the first pass: replayed R of N records,
 * U of them unknown to the table. Nothing is reported.` and the rule, and the call returns KTA_ERR_INVALID (the text is
 * still written).  Output buffer conventions as kta_render_report. */
int kta_render_compaction(const uint64_t *vec, const uint64_t *counter_vec, uint32_t n_partitions, char *out, size_t out_cap,
                          size_t *out_len);
/* The section kta-analyzer prints with --librdkafka kta.segments=<size> (1g, 512m, 64k or bytes; kta.segments.rows=M,
 * default 1024, lowered so that P * M <= 2^20; kta.segments.overhead=B, default 0; kta.retention.ms=<duration> in the
 * timeline's syntax, kta.retention.bytes=<size>, kta.retention.now=<unix seconds>, default the run's start time) after the
 * partitioner and compaction sections and before the filter's, from a segment vector (definition above kta_set_segments);
 * not part of the reference report:
 *   `Retention what-if: model log segments of <S> bytes per partition (kta.segments), retention.ms=<ms>,
 *    retention.bytes=<bytes>, now=<ms> ms (not part of the reference report)` — `-` for a rule that is off, and `no
 *    retention policy given` in place of the three when both are;
 *   a table (P | Segments | Records | Bytes | Records kept | Bytes kept | Reclaimed % | Rule), one row per partition and an
 *    `All` row — Segments ends in `+` for a partition that outgrew its M rows, Reclaimed % has two decimals (`-` without
 *    bytes), Rule is `time`, `size` or `-` (`time+size` in the All row when partitions differ) —, only the first four
 *    columns when no policy is given;
 *   a line counting the partitions that outgrew their rows, when there are any; the model-limits note; a closing `=` rule.
 * KTA_ERR_INVALID for what kta_retention_whatif refuses.  Output buffer conventions as kta_render_report. */
int kta_render_retention(const uint64_t *vec, uint32_t n_partitions, uint32_t rows_per_partition, int64_t now_ms, int64_t retention_ms,
                         int64_t retention_bytes, char *out, size_t out_cap, size_t *out_len);
/* The section kta-analyzer prints with -c --librdkafka kta.compaction=1,kta.segments=<size>,kta.compact_delete=1 (and the
 * kta.retention.* keys) after the retention section and before the filter's, from the three vectors of
 * kta_compact_delete_whatif; not part of the reference report:
 *   `Compact,delete what-if: cleanup.policy=compact,delete over model log segments of <S> bytes per partition
 *    (kta.compact_delete), retention.ms=<ms>, retention.bytes=<bytes>, now=<ms> ms; the active segment is not cleaned (not
 *    part of the reference report)` — `-` for a rule that is off, for now as well when the time rule is off;
 *   a table (P | Records | Bytes | Compacted records | Compacted bytes | Kept records | Kept bytes | Tombstones kept |
 *    Reclaimed % | Rule), one row per partition and an `All` row — P ends in `+` for a partition that outgrew its M rows,
 *    Reclaimed % = 1 - kept bytes / bytes with two decimals (`-` without bytes), Rule is `time`, `size` or `-` (`time+size`
 *    in the All row when partitions differ);
 *   the model-limits note; a closing `=` rule.
 * When kta_compact_delete_whatif reports a mismatch the section is the first line, `The replay did not match the first
 * pass. Nothing is reported.` and the rule, and the call returns KTA_ERR_INVALID (the text is still written); for other
 * bad arguments KTA_ERR_INVALID and nothing is written.  Output buffer conventions as kta_render_report. */
int kta_render_compact_delete(const uint64_t *seg_vec, const uint64_t *kept_vec, const uint64_t *comp_vec, uint32_t n_partitions,
                              uint32_t rows_per_partition, int64_t now_ms, int64_t retention_ms, int64_t retention_bytes, char *out,
                              size_t out_cap, size_t *out_len);
/* The section kta-analyzer prints after everything else when a filter was given (--librdkafka kta.from=<epoch seconds>,
 * kta.to=<epoch seconds>, kta.partitions=0,3-5); not part of the reference report:
 *   `Record filter: everything above describes the records that passed, and no others (kta.from, kta.to, kta.partitions;
 *    not part of the reference report)`;
 *   a table (Filter | Value) with the rows `From (timestamp >=)` and `To (timestamp <)` — `<seconds> s (<ms> ms)`, with
 *    three decimals where the bound is not a whole second, `-` without the bound —, `Partitions` — the set as ascending
 *    ranges `0,3-5`, `all` without one, `none` for the empty set —, `Records seen`, `Records passed` (kta_filter_info's
 *    first two words, summed over the ranks of a sharded run) and `Passed %` (two decimals; `-` when nothing was seen);
 *   a closing `=` rule.
 * partition_bitmap: NULL, or ceil(n_partitions / 32) words as kta_set_filter takes them.  Output buffer conventions as
 * kta_render_report. */
/* The opt-in record-batch section that kta-analyzer prints behind every other section with --librdkafka
 * kta.record_batches=1, from a record-batch vector (host only):
 *   a title line saying that it is not part of the reference report;
 *   a table (P | Batches | Rec/batch | Largest | B/batch | Largest | Span ms | Compressed % | Ratio | Holes | Holes % |
 *    Idempotent % | Transactional % | LogAppendTime % | Epoch | Failed) with a row per partition and a `Topic` row: the means
 *    and shares with two decimals, Ratio = payload / recbytes of the compressed batches, Holes = extent - records and its
 *    share of the extent, Epoch the highest leader epoch (`-` when none);
 *   a table per codec (Codec | Batches | Records | Bytes on disk | Inflated bytes | Ratio | Rec/batch p50 | p90 | B/batch p50
 *    | p90): the percentiles are the upper ends of their histogram bins;
 *   `Producers (estimated, +/- 3.25 %): N`;
 *   the notes: what is not counted, with skipped[0..2] = the host index's control batches, magic 0/1 sets and batches of an
 *    unknown codec summed over the run (NULL: zeros), and, when `filtered`, that the batches are those that overlap the
 *    window; a closing `=` rule.
 * A ratio, mean or share whose denominator is 0 prints `n/a`.  Output buffer conventions as kta_render_report. */
int kta_render_record_batches(const uint64_t *vec, uint32_t n_partitions, int filtered, const uint64_t *skipped, char *out,
                              size_t out_cap, size_t *out_len);
/* The opt-in payload section that kta-analyzer prints behind every other section with --librdkafka kta.payload=1, from a
 * payload vector (host only):
 *   a title line saying that it is not part of the reference report;
 *   a table (P | Records | Null % | Empty % | Framed % | JSON % | Other % | With headers | Headers/rec | Header bytes % | Bad
 *    headers) with a row per partition and a `Topic` row: the shares of the records with two decimals, Headers/rec = headers
 *    over the records whose headers are good, Header bytes % = header_wire_bytes over key + value + header_wire_bytes with
 *    key + value = the counter vector's key_size_sum + value_size_sum (counter_vec NULL: `n/a`);
 *   the histogram of headers per record (Headers | Records), bins 0 .. 14 and >= 15;
 *   the schema ids (Schema id | Records | Bytes | B/record) sorted by records, at most 64 rows, then `... and K more`, then
 *    the unresolved remainder when it is not zero;
 *   a note with the section's limits, and a closing `=` rule.
 * A share or mean whose denominator is 0 prints `n/a`.  Output buffer conventions as kta_render_report. */
int kta_render_payload(const uint64_t *vec, const uint64_t *counter_vec, uint32_t n_partitions, char *out, size_t out_cap, size_t *out_len);
/* The opt-in header-name section that kta-analyzer prints behind the payload section's position with --librdkafka
 * kta.headers=1, from a header-name vector and (or NULL) a name table (host only):
 *   a title line that names the knob and says that it is not part of the reference report;
 *   a line with the globals;
 *   a table (# | Name | Hash | Occurrences | per record with headers | Name bytes | Value bytes | Mean value | Null values |
 *    Share of header bytes) of the listed names, at most max_names rows, then `... and K more`: the name escaped as
 *    kta_render_hot_keys escapes keys, `...` behind a name longer than 48 bytes, `#%08x` of the hash without an exemplar; per
 *    record with headers = occurrences over the records with headers (a mean); Mean value = value bytes over the occurrences
 *    whose value is not null; Share = the name's name + value bytes over the topic's;
 *   a line for the unresolved remainder when there is one; a closing `=` rule.
 * A figure whose denominator is 0 prints `n/a`.  Output buffer conventions as kta_render_report. */
int kta_render_header_names(const uint64_t *vec, const kta_header_name *table, uint32_t max_names, char *out, size_t out_cap, size_t *out_len);
/* The opt-in value-byte section that kta-analyzer prints behind the header-name section's position with --librdkafka
 * kta.value_bytes=1, from a value-byte vector (host only):
 *   a title line that names the knob and says that it is not part of the reference report;
 *   a table (P | Records | Values | Value bytes | H0 bits/byte | Order-0 floor % | Printable % | Zero % | High-bit % |
 *    Repeat % | Distinct | Top byte | Class), a row per partition and a `Topic` row of their sum: H0 with two decimals; the
 *    floor and the shares as percentages of the value bytes with two decimals; Top byte as 0xHH and its share;
 *   a note: the class is a heuristic; H0 bounds an order-0 entropy coder alone — LZ matching, most of what gzip, LZ4 or
 *    zstd win on JSON, is not in it; and a closing `=` rule.
 * A share whose denominator is 0 prints `n/a`.  Output buffer conventions as kta_render_report. */
int kta_render_value_bytes(const uint64_t *vec, uint32_t n_partitions, char *out, size_t out_cap, size_t *out_len);
/* The opt-in compression what-if section that kta-analyzer prints behind the value-byte section's position with --librdkafka
 * kta.compress_whatif=lz4, from a what-if vector (host only):
 *   a title line that names the knob and says that it is not part of the reference report;
 *   a table (P | Batches | Record bytes/batch | Record bytes | On disk now | Now ratio | LZ4 model | Model ratio | Saving vs
 *    now % | Stored blocks % | Match %), a row per partition and a `Topic` row of their sum: the ratios are record bytes over
 *    the bytes with two decimals, the saving is 1 - model / now, the match share is of the record bytes;
 *   a table by the batches' current codec (Codec | Batches | Record bytes | On disk now | Now ratio | LZ4 model | Model ratio);
 *   notes: the model in one sentence; it is a floor; the 61 header bytes are on neither side; the ratio is at the topic's
 *    present batching; and a closing `=` rule.
 * A figure whose denominator is 0 prints `n/a`.  Output buffer conventions as kta_render_report. */
int kta_render_compress_whatif(const uint64_t *vec, uint32_t n_partitions, char *out, size_t out_cap, size_t *out_len);
int kta_render_filter(int64_t from_ms, int64_t to_ms, const uint32_t *partition_bitmap, uint32_t n_partitions, uint64_t seen,
                      uint64_t passed, char *out, size_t out_cap, size_t *out_len);

/* ---- profiling hooks --------------------------------------------------------------- */
/* With kta_set_timing(ctx, 1) every kernel launch is bracketed by a pair of HIP events recorded
 * on the compute stream (no host synchronisation while recording).  kta_kernel_time_stats waits
 * for the stream and returns, per kernel kind ([0] metrics scan, [1] partial fold, [2] alive-key
 * update), the average duration in ms and the number of launches since the previous call
 * (avg -1 when none). */
int kta_set_timing(kta_ctx *ctx, int enable);
int kta_kernel_time_stats(kta_ctx *ctx, float avg_ms[3], uint64_t launches[3]);
/* Launch-geometry knobs (0 = default): scan workgroups, scan kernel flavour (16 = non-temporal loads; 32 = do not use
 * tile summaries: every tile's timestamps are loaded; 64 = ignore the plane marks: a summarised tile is read in its
 * u16 form, 6 B per record),
 * alive workgroups, alive kernel: 0 plain atomicMax, 1 returning atomicMax + running alive count, 2 the
 * same walked backwards with a pre-read that skips superseded records, 3 (default) / 4 the partitioned
 * pass (hash + partition by the hash's top 10 / 9 bits, then per-bucket merge in LDS) for batches of 2^21
 * records and more without a seq column — kernel 2 otherwise, and for the batches that follow one whose
 * keys were mostly unique; 13 / 14 the partitioned pass for every batch (tests); 8 / 9 ablation halves. */
int kta_set_tuning(kta_ctx *ctx, int scan_workgroups, int scan_variant, int alive_workgroups,
                   int alive_variant);
/* Both handlers of a batch (kafka.rs:107-109: every handler for every message) as ONE pass over it where that is
 * possible (bit set state, at most 256 partitions, no analytics): on by default; 0 = always two passes (scan, then
 * the alive-key pass).  Results are bit-identical either way.  The environment variable KTA_NO_FUSE=1, read by
 * kta_create, only sets the initial value.  In the fused pass all kernel time is booked on timer kind 2 (the
 * alive-key update) and kinds 0 / 1 see only the fold: kta_kernel_time_stats returns launches[0] == 0 there. */
int kta_set_fuse(kta_ctx *ctx, int enable);
/* What the partitioned alive-key pass did since kta_create / kta_reset:
 * out[0] the most records one launch pair takes (larger batches are applied piece after piece), out[1] launch pairs,
 * out[2] of them with both handlers in the one pass, out[3] of them whose metrics handler ran as a scan although the
 * batch began fused, out[4] buckets handed to the fallback kernel (hot keys that overflow their segments; exact, slow) —
 * counted on the device by every launch pair; this call waits for the context's compute stream to read the word —,
 * out[5] the fuse switch. */
int kta_alive_pass_info(kta_ctx *ctx, uint64_t out[6]);

#ifdef __cplusplus
}
#endif
#endif /* KTA_HIP_H */

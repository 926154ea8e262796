// metric.hpp — C++ host mirror of the reference's handler interface over the C ABI (kta_hip.h).
//
//   reference (under /root/reference)                          here
//   src/kafka.rs:18-20   trait MetricHandler                   kta::MetricHandler
//   src/metric.rs:12-26  struct MessageMetrics (+ accessors)   kta::MessageMetrics   (view of a kta_result)
//   src/metric.rs:262-285 LogCompactionInMemoryMetrics         kta::LogCompactionInMemoryMetrics (view)
//   both `impl MetricHandler` (metric.rs:206, 288)             kta::HipMetricHandler: ONE handler feeds
//                                                              both reference handlers' state on the GPU
//
// The reference registers two handlers and calls each per message (kafka.rs:107-109); here one
// handler stages the message once and the device runs both accumulations.  Same accessor names,
// same integer semantics, same failure behaviour (the averages "panic" on divide by zero).
#pragma once

#include <stdint.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "kta_hip.h"

namespace kta {

// What the handlers read from a rdkafka BorrowedMessage (metric.rs:208-209, 218, 233).
struct Message {
    int32_t partition = 0;
    int64_t offset = 0;
    int64_t timestamp_ms = -1;     // raw rdkafka timestamp; -1 == not available
    const uint8_t *key = nullptr;  // nullptr == key None
    int64_t key_len = -1;
    int64_t payload_len = -1;      // -1 == payload None (tombstone); bytes are never read
};

struct RustPanic : std::runtime_error {
    std::string location;
    RustPanic(const std::string &msg, const std::string &loc) : std::runtime_error(msg), location(loc) {}
};

struct DateTimeUtc {  // chrono DateTime<Utc>, ordered by (sec, ns)
    int64_t sec = 0;
    uint32_t ns = 0;
    bool operator>(const DateTimeUtc &o) const { return sec > o.sec || (sec == o.sec && ns > o.ns); }
    bool operator<(const DateTimeUtc &o) const { return o > *this; }
};

class MetricHandler {  // kafka.rs:18-20
public:
    virtual ~MetricHandler() {}
    virtual void handle_message(const Message &m) = 0;
};

class MessageMetrics {  // accessors: metric.rs:104-195
public:
    MessageMetrics() {}
    MessageMetrics(const kta_result &r, std::vector<uint64_t> counters, DateTimeUtc now);
    uint64_t total(int32_t p) const { return metric(p, KTA_C_TOTAL); }
    uint64_t tombstones(int32_t p) const { return metric(p, KTA_C_TOMBSTONES); }
    uint64_t alive(int32_t p) const { return metric(p, KTA_C_ALIVE); }
    uint64_t key_null(int32_t p) const { return metric(p, KTA_C_KEY_NULL); }
    uint64_t key_non_null(int32_t p) const { return metric(p, KTA_C_KEY_NON_NULL); }
    uint64_t key_size_sum(int32_t p) const { return metric(p, KTA_C_KEY_SIZE_SUM); }
    uint64_t value_size_sum(int32_t p) const { return metric(p, KTA_C_VALUE_SIZE_SUM); }
    uint64_t key_size_avg(int32_t p) const;      // metric.rs:132-139 (throws RustPanic)
    uint64_t value_size_avg(int32_t p) const;    // metric.rs:141-148
    uint64_t message_size_avg(int32_t p) const;  // metric.rs:150-157
    float dirty_ratio(int32_t p) const;          // metric.rs:159-167
    const DateTimeUtc &latest_message() const { return latest_; }
    const DateTimeUtc &earliest_message() const { return earliest_; }
    uint64_t smallest_message() const;           // metric.rs:177-183
    uint64_t largest_message() const { return res_.largest_message; }
    uint64_t overall_count() const { return res_.overall_count; }
    uint64_t overall_size() const { return res_.overall_size; }

private:
    uint64_t metric(int32_t p, int c) const;     // metric.rs:198-203
    kta_result res_{};
    std::vector<uint64_t> c_;
    DateTimeUtc earliest_, latest_;
};

// The additive analytics (KTA_FLAG_ANALYTICS; no reference counterpart), decoded as kta_get_analytics does.
struct Analytics {
    kta_analytics hist{};
    std::vector<int64_t> min_ts_sec, max_ts_sec;      // INT64_MAX / INT64_MIN: no record in the partition
    std::vector<uint64_t> smallest, largest;          // UINT64_MAX / 0: no non-tombstone in the partition
    uint64_t records() const;                         // every record lands in exactly one key-size bucket
};

// The timeline's configuration (kta_set_timeline; no reference counterpart).
struct TimelineConfig {
    int64_t origin_ms = 0, bucket_ms = 0;
    uint32_t n_buckets = 0;     // 0: no timeline
};

class LogCompactionInMemoryMetrics {  // metric.rs:262-285
public:
    LogCompactionInMemoryMetrics() {}
    explicit LogCompactionInMemoryMetrics(const kta_result &r) : alive_(r.alive_keys) {}
    size_t sum_all_alive() const { return (size_t)alive_; }

private:
    uint64_t alive_ = 0;
};

// The GPU-backed handler.  Construction == MessageMetrics::new() (+ LogCompactionInMemoryMetrics::new()
// when count_alive_keys): `now` stands in for Utc::now() (metric.rs:39).
class HipMetricHandler : public MetricHandler {
public:
    HipMetricHandler(int32_t n_partitions, bool count_alive_keys, int device = 0, uint64_t batch_capacity = 0,
                     uint64_t key_bytes_capacity = 0, uint32_t flags = 0, const TimelineConfig &timeline = TimelineConfig{},
                     uint32_t repartition = 0 /* KTA_FLAG_PARTITIONER: the what-if partition count Q; 0: P */);
    ~HipMetricHandler() override;
    HipMetricHandler(const HipMetricHandler &) = delete;
    HipMetricHandler &operator=(const HipMetricHandler &) = delete;

    void handle_message(const Message &m) override;  // kafka.rs:107-109
    // The trait has no end-of-stream hook; call this where main.rs:121 is (before the report).
    // tolerate_undelivered: records of batches that failed check.crcs / framing were written with
    // partition -1 (never counted); with true they are reported through undelivered_records()
    // instead of failing the run (the reference warns on Kafka errors and goes on, kafka.rs:95-97).
    void finish(bool tolerate_undelivered = false);
    // A rank of a partition-sharded run (one handler per GPU): join the job's communicator, and at the end
    // exchange() instead of finish() — afterwards metrics() / log_compaction() are the whole job's on every rank.
    void comm_create(int nranks, int rank, const uint8_t *unique_id);
    void exchange(bool tolerate_undelivered = false);
    uint64_t undelivered_records() const { return undelivered_; }
    // With KTA_FLAG_ANALYTICS: the analytics of the snapshot finish() / exchange() took (after exchange(), the whole
    // job's); nullptr without the flag.
    const Analytics *analytics() const { return analytics_on_ ? &analytics_ : nullptr; }
    // With a timeline: the vector u64[(n_buckets + 3) * 3] of the snapshot finish() / exchange() took (after
    // exchange(), the whole job's); nullptr without one.
    const std::vector<uint64_t> *timeline() const { return timeline_.n_buckets ? &tvec_ : nullptr; }
    const TimelineConfig &timeline_config() const { return timeline_; }
    // With KTA_FLAG_KEY_SKETCH: the key sketch u64[P * 4096] of the snapshot finish() / exchange() took (after exchange(),
    // the whole job's); nullptr without the flag.
    const std::vector<uint64_t> *key_sketch() const { return sketch_on_ ? &svec_ : nullptr; }
    // With KTA_FLAG_HOT_KEYS: the hot-key vector u64[2 * 1024 * 23] of the snapshot finish() / exchange() took (after
    // exchange(), the whole job's) and this context's own exemplar table [2 * 1024]; nullptr without the flag.
    const std::vector<uint64_t> *hot_keys() const { return hot_on_ ? &hvec_ : nullptr; }
    const std::vector<kta_hot_exemplar> *hot_key_exemplars() const { return hot_on_ ? &hex_ : nullptr; }
    // With KTA_FLAG_TS_ORDER: the timestamp-order vector u64[3 P + 64] of the snapshot finish() / exchange() took (after
    // exchange(), the whole job's); nullptr without the flag.
    const std::vector<uint64_t> *ts_order() const { return tso_on_ ? &ovec_ : nullptr; }
    // With KTA_FLAG_PARTITIONER: the partitioner vector u64[2 P + 2 Q] of the snapshot finish() / exchange() took (after
    // exchange(), the whole job's); nullptr without the flag.
    const std::vector<uint64_t> *partitioner() const { return part_on_ ? &pvec_ : nullptr; }
    uint32_t repartition() const { return part_q_; }
    // With KTA_FLAG_SIZE_QUANTILES: the size vector u64[P * 3 * 464 + 8] of the snapshot finish() / exchange() took (after
    // exchange(), the whole job's); nullptr without the flag.
    const std::vector<uint64_t> *size_quantiles() const { return sizeq_on_ ? &qvec_ : nullptr; }
    // With KTA_FLAG_RECORD_BATCHES: the record-batch vector u64[20 P + 1524] of that snapshot; nullptr without the flag.
    const std::vector<uint64_t> *record_batches() const { return rb_on_ ? &bvec_ : nullptr; }
    // With KTA_FLAG_PAYLOAD: the payload vector u64[24 P + 69648] of that snapshot; nullptr without the flag.
    const std::vector<uint64_t> *payload() const { return pl_on_ ? &lvec_ : nullptr; }
    // With KTA_FLAG_HEADER_NAMES: the header-name vector u64[73736] of that snapshot and this context's own name table [2 * 1024];
    // nullptr without the flag.
    const std::vector<uint64_t> *header_names() const { return hn_on_ ? &nvec_ : nullptr; }
    const std::vector<kta_header_name> *header_name_table() const { return hn_on_ ? &ntab_ : nullptr; }
    // With KTA_FLAG_VALUE_BYTES: the value-byte vector u64[264 P] of that snapshot; nullptr without the flag.
    const std::vector<uint64_t> *value_bytes() const { return vb_on_ ? &yvec_ : nullptr; }
    // With KTA_FLAG_COMPRESS_WHATIF: the compression what-if vector u64[8 P + 20] of that snapshot; nullptr without the flag.
    const std::vector<uint64_t> *compress_whatif() const { return cw_on_ ? &wvec_ : nullptr; }
    // The segment pass of the retention what-if (kta_set_segments): right after construction, before any record; then the
    // segment vector u64[(P M + P) 4 + 8] of the snapshot finish() / exchange() took (after exchange(), the whole job's);
    // nullptr without it.
    void set_segments(uint64_t segment_bytes, uint32_t rows_per_partition, uint32_t record_overhead);
    const std::vector<uint64_t> *segments() const { return seg_rows_ ? &gvec_ : nullptr; }
    // With KTA_FLAG_COMPACTION: replay mode on / off (kta_compaction_replay) — after finish(), feed the source a second time
    // between replay_compaction(true) and replay_compaction(false) — and then the live compaction vector u64[5 P + 6].
    void replay_compaction(bool on);
    std::vector<uint64_t> compaction();
    // The compact,delete what-if (kta_set_compact_delete): after set_segments, before any record, with KTA_FLAG_COMPACTION;
    // then, behind the replay, the live kept vector u64[(P M + P) 4 + 8].
    void set_compact_delete(bool on);
    std::vector<uint64_t> compact_delete();
    const MessageMetrics &metrics() const { return metrics_; }
    const LogCompactionInMemoryMetrics *log_compaction() const { return alive_ ? &lc_ : nullptr; }
    kta_ctx *ctx() { return ctx_; }
    DateTimeUtc now() const { return now_; }

private:
    void check(int rc, const char *what);
    void read_analytics();   // the analytics, the timeline, the key sketch and the hot keys of the snapshot
    kta_ctx *ctx_ = nullptr;
    int32_t P_;
    bool alive_;
    DateTimeUtc now_;
    MessageMetrics metrics_;
    LogCompactionInMemoryMetrics lc_;
    uint64_t undelivered_ = 0;
    bool analytics_on_ = false;
    Analytics analytics_;
    TimelineConfig timeline_;
    std::vector<uint64_t> tvec_;
    bool sketch_on_ = false;
    std::vector<uint64_t> svec_;
    bool hot_on_ = false;
    std::vector<uint64_t> hvec_;
    std::vector<kta_hot_exemplar> hex_;
    bool tso_on_ = false;
    std::vector<uint64_t> ovec_;
    bool part_on_ = false;
    uint32_t part_q_ = 0;
    std::vector<uint64_t> pvec_;
    bool sizeq_on_ = false;
    std::vector<uint64_t> qvec_;
    bool rb_on_ = false;
    std::vector<uint64_t> bvec_;
    bool pl_on_ = false;
    std::vector<uint64_t> lvec_;
    bool hn_on_ = false;
    std::vector<uint64_t> nvec_;
    std::vector<kta_header_name> ntab_;
    bool vb_on_ = false;
    std::vector<uint64_t> yvec_;
    bool cw_on_ = false;
    std::vector<uint64_t> wvec_;
    uint32_t seg_rows_ = 0;   // M; 0: no segments
    std::vector<uint64_t> gvec_;
};

// chrono 0.4.19 `Display for DateTime<Utc>` (main.rs:132-133)
std::string format_datetime_utc(int64_t sec, uint32_t ns);
// Rust `format!("{0:.4}", f32)` (main.rs:162)
std::string format_f32_4(float x);
// main.rs:123-178 — everything the reference prints after the scan, byte for byte
std::string render_report(const std::string &topic, uint64_t duration_secs, const MessageMetrics &m,
                          const LogCompactionInMemoryMetrics *lc, const std::vector<int32_t> &partitions,
                          const std::vector<int64_t> &start_offsets, const std::vector<int64_t> &end_offsets);
// the opt-in section kta-analyzer prints after the report with kta.analytics=1 (kta_render_analytics)
std::string render_analytics(const Analytics &a);
// the opt-in section kta-analyzer prints after the report (and the analytics) with kta.timeline=<width>
// (kta_render_timeline)
std::string render_timeline(const uint64_t *vec, int64_t origin_ms, int64_t bucket_ms, uint32_t n_buckets);
// a timeline width as kta.timeline takes it (86400000 -> "1d", 90000 -> "90s", 7 -> "7ms")
std::string format_width_ms(int64_t w);
// the opt-in section kta-analyzer prints after the report (and the analytics and the timeline) with kta.distinct_keys=1
// (kta_render_distinct_keys): sketch u64[P * 4096], keyed[p] = key_non_null of partition p
std::string render_distinct_keys(const uint64_t *sketch, const std::vector<uint64_t> &keyed);
// the opt-in section kta-analyzer prints with kta.ts_order=1 after those and before the hot keys (kta_render_ts_order):
// vec u64[3 P + 64], records[p] = total_messages of partition p
std::string render_ts_order(const uint64_t *vec, const std::vector<uint64_t> &records);
// the opt-in section kta-analyzer prints last with kta.hot_keys=K (kta_render_hot_keys): vec u64[2 * 1024 * 23],
// exemplars [2 * 1024] or null; empty for a vector kta_hot_keys_recover refuses
std::string render_hot_keys(const uint64_t *vec, const kta_hot_exemplar *exemplars, uint32_t max_keys);
// the opt-in section kta-analyzer prints last of all with kta.partitioner=murmur2 (kta_render_partitioner): vec
// u64[2 P + 2 Q], counters u64[P * 7 + 8] (the counter vector of the same records; its globals are not read)
std::string render_partitioner(const uint64_t *vec, const uint64_t *counters, uint32_t P, uint32_t Q);
// the opt-in section kta-analyzer prints with kta.percentiles=1 after the report's closing rule and the analytics
// (kta_render_size_percentiles): vec u64[P * 3 * 464 + 8]
std::string render_size_percentiles(const uint64_t *vec, uint32_t P);
// (kta_render_record_batches): vec u64[20 P + 1524]; skipped: control batches, magic 0/1 sets, unknown codecs of the run
std::string render_record_batches(const uint64_t *vec, uint32_t P, bool filtered, const uint64_t skipped[3]);
// (kta_render_payload): vec u64[24 P + 69648]; counters: the counter vector (key_size_sum, value_size_sum) or nullptr
std::string render_payload(const uint64_t *vec, const uint64_t *counters, uint32_t P);
// (kta_render_header_names): vec u64[73736]; table: a name table [2 * 1024] or nullptr; at most max_names rows
std::string render_header_names(const uint64_t *vec, const kta_header_name *table, uint32_t max_names);
// (kta_render_value_bytes): vec u64[264 P]
std::string render_value_bytes(const uint64_t *vec, uint32_t P);
// (kta_render_compress_whatif): vec u64[8 P + 20]
std::string render_compress_whatif(const uint64_t *vec, uint32_t P);
// the opt-in section kta-analyzer prints with kta.segments=<size> after the partitioner and compaction sections and before
// the filter's (kta_render_retention): vec u64[(P M + P) 4 + 8]; retention -1: the rule is off
std::string render_retention(const uint64_t *vec, uint32_t P, uint32_t M, int64_t now_ms, int64_t retention_ms, int64_t retention_bytes);
// the opt-in section kta-analyzer prints with -c and kta.compaction=1 after the partitioner section and before the filter
// section (kta_render_compaction): vec u64[5 P + 6], counters u64[P * 7 + 8] (the first pass's counter vector).  *matched
// (when given): whether the replay matched the first pass; a section that says it did not otherwise
std::string render_compaction(const uint64_t *vec, const uint64_t *counters, uint32_t P, bool *matched = nullptr);
// The opt-in compact,delete section (kta.compact_delete=1; kta_render_compact_delete), printed after the retention section
// and before the filter's: seg / kept u64[(P M + P) 4 + 8], comp u64[5 P + 6].  *matched: false when the replay did not match
// the first pass (the section then says so).  Empty: arguments kta_compact_delete_whatif refuses for another reason.
std::string render_compact_delete(const uint64_t *seg, const uint64_t *kept, const uint64_t *comp, uint32_t P, uint32_t M, int64_t now_ms,
                                  int64_t retention_ms, int64_t retention_bytes, bool *matched = nullptr);
// the section kta-analyzer prints after everything else when a filter was given (kta.from, kta.to, kta.partitions;
// kta_render_filter): bitmap null or ceil(P / 32) words as kta_set_filter takes them; the counts are kta_filter_info's
std::string render_filter(int64_t from_ms, int64_t to_ms, const uint32_t *bitmap, uint32_t P, uint64_t seen, uint64_t passed);

}  // namespace kta

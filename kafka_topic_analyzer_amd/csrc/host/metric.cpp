// metric.cpp — host-side accessors and the GPU-backed MetricHandler (see metric.hpp).
#include "metric.hpp"

#include <time.h>

namespace kta {

MessageMetrics::MessageMetrics(const kta_result &r, std::vector<uint64_t> counters, DateTimeUtc now)
    : res_(r), c_(std::move(counters))
{
    // metric.rs:39-40: earliest = Utc::now(), latest = epoch 0; then what
    // cmp_and_set_message_timestamp (metric.rs:65-72) would have done with the device extrema.
    earliest_ = now;
    latest_ = DateTimeUtc{0, 0};
    if (r.any_records) {
        DateTimeUtc lo{r.min_ts_sec, 0}, hi{r.max_ts_sec, 0};
        if (earliest_ > lo) earliest_ = lo;
        if (latest_ < hi) latest_ = hi;
    }
}

uint64_t MessageMetrics::metric(int32_t p, int c) const
{
    if (p < 0 || (uint32_t)p >= res_.n_partitions) return 0;  // None => 0 (metric.rs:201)
    return c_[(size_t)p * KTA_NCOUNTERS + c];
}

static uint64_t avg_or_panic(uint64_t sum, uint64_t alive, const char *loc)
{
    if (sum > 0) {
        if (alive == 0) throw RustPanic("attempt to divide by zero", loc);
        return sum / alive;
    }
    return 0;
}

uint64_t MessageMetrics::key_size_avg(int32_t p) const
{
    return avg_or_panic(key_size_sum(p), alive(p), "src/metric.rs:135:13");
}

uint64_t MessageMetrics::value_size_avg(int32_t p) const
{
    return avg_or_panic(value_size_sum(p), alive(p), "src/metric.rs:144:13");
}

uint64_t MessageMetrics::message_size_avg(int32_t p) const
{
    return avg_or_panic(key_size_sum(p) + value_size_sum(p), alive(p), "src/metric.rs:153:13");
}

float MessageMetrics::dirty_ratio(int32_t p) const
{
    const uint64_t total_messages = total(p), tomb = tombstones(p);
    if (total_messages > 0 && tomb > 0) {
        // two f32 roundings, exactly as `tombstones as f32 / (total_messages as f32 / 100.0f32)`;
        // compiled with -ffp-contract=off, volatile keeps each step in f32
        volatile float t = (float)tomb;
        volatile float tm = (float)total_messages;
        volatile float d = tm / 100.0f;
        volatile float r = t / d;
        return r;
    }
    return 0.0f;
}

uint64_t MessageMetrics::smallest_message() const
{
    return res_.smallest_message == UINT64_MAX ? 0 : res_.smallest_message;
}

HipMetricHandler::HipMetricHandler(int32_t n_partitions, bool count_alive_keys, int device, uint64_t batch_capacity,
                                   uint64_t key_bytes_capacity, uint32_t flags, const TimelineConfig &timeline, uint32_t repartition)
    : P_(n_partitions), alive_(count_alive_keys), analytics_on_((flags & KTA_FLAG_ANALYTICS) != 0), timeline_(timeline),
      sketch_on_((flags & KTA_FLAG_KEY_SKETCH) != 0), hot_on_((flags & KTA_FLAG_HOT_KEYS) != 0),
      tso_on_((flags & KTA_FLAG_TS_ORDER) != 0), part_on_((flags & KTA_FLAG_PARTITIONER) != 0),
      part_q_(part_on_ ? (repartition ? repartition : (uint32_t)n_partitions) : 0u), sizeq_on_((flags & KTA_FLAG_SIZE_QUANTILES) != 0),
      rb_on_((flags & KTA_FLAG_RECORD_BATCHES) != 0), pl_on_((flags & KTA_FLAG_PAYLOAD) != 0),
      hn_on_((flags & KTA_FLAG_HEADER_NAMES) != 0), vb_on_((flags & KTA_FLAG_VALUE_BYTES) != 0),
      cw_on_((flags & KTA_FLAG_COMPRESS_WHATIF) != 0)
{
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);  // Utc::now() (metric.rs:39)
    now_ = DateTimeUtc{(int64_t)ts.tv_sec, (uint32_t)ts.tv_nsec};
    kta_config cfg{};
    cfg.device_id = device;
    cfg.n_partitions = n_partitions;
    cfg.count_alive_keys = count_alive_keys ? 1 : 0;
    cfg.batch_capacity = batch_capacity;
    cfg.key_bytes_capacity = key_bytes_capacity;
    cfg.flags = flags;
    int rc = kta_create(&cfg, &ctx_);
    if (rc != KTA_OK) throw std::runtime_error(std::string("kta_create failed: ") + kta_last_error(nullptr));
    if (timeline_.n_buckets) {
        rc = kta_set_timeline(ctx_, timeline_.origin_ms, timeline_.bucket_ms, timeline_.n_buckets);
        if (rc != KTA_OK) {
            const std::string msg = std::string("kta_set_timeline failed: ") + kta_last_error(ctx_);
            kta_destroy(ctx_);
            ctx_ = nullptr;
            throw std::runtime_error(msg);
        }
    }
    if (part_on_ && repartition) {
        rc = kta_set_repartition(ctx_, repartition);
        if (rc != KTA_OK) {
            const std::string msg = std::string("kta_set_repartition failed: ") + kta_last_error(ctx_);
            kta_destroy(ctx_);
            ctx_ = nullptr;
            throw std::runtime_error(msg);
        }
    }
}

HipMetricHandler::~HipMetricHandler() { kta_destroy(ctx_); }

void HipMetricHandler::check(int rc, const char *what)
{
    if (rc != KTA_OK) throw std::runtime_error(std::string(what) + ": " + kta_last_error(ctx_));
}

// NaiveDateTime::from_timestamp(timestamp / 1000, 0) of a record outside chrono 0.4.19's range: the reference
// dies on that record (kafka.rs:104, before any handler; metric.rs:210 holds the same call).  The device counts the
// record like any other; the extrema tell at the end of the stream, which is where this mirror can say it.  (The
// reference's own location string is the expect() inside the chrono crate, under the builder's cargo registry.)
static const char *const kDateTimePanic = "invalid or out-of-range datetime";
static const char *const kDateTimePanicAt = "chrono-0.4.19/src/naive/datetime.rs (NaiveDateTime::from_timestamp, src/kafka.rs:104)";

void HipMetricHandler::handle_message(const Message &m)
{
    // metric.rs:209-210: the handler's own NaiveDateTime::from_timestamp(timestamp / 1000, 0) — the message is in
    // hand here, so a timestamp outside chrono's range ends the run on this very record, as in the reference
    const int64_t secs = (m.timestamp_ms == -1 ? 0 : m.timestamp_ms) / 1000;
    if (secs < KTA_CHRONO_MIN_SEC || secs > KTA_CHRONO_MAX_SEC)
        throw RustPanic(kDateTimePanic, "chrono-0.4.19/src/naive/datetime.rs (NaiveDateTime::from_timestamp, src/metric.rs:210)");
    check(kta_handle_message(ctx_, m.partition, m.timestamp_ms, m.key, m.key ? m.key_len : -1, m.payload_len),
          "kta_handle_message");
}

void HipMetricHandler::finish(bool tolerate_undelivered)
{
    kta_result r{};
    std::vector<uint64_t> counters((size_t)P_ * KTA_NCOUNTERS);
    const int rc = kta_finish(ctx_, &r, counters.data());
    if (rc == KTA_ERR_TIMESTAMP_RANGE) throw RustPanic(kDateTimePanic, kDateTimePanicAt);
    if (!(rc == KTA_ERR_BAD_PARTITION && tolerate_undelivered)) check(rc, "kta_finish");
    undelivered_ = r.bad_partition_records;
    metrics_ = MessageMetrics(r, std::move(counters), now_);
    lc_ = LogCompactionInMemoryMetrics(r);
    read_analytics();
}

void HipMetricHandler::set_segments(uint64_t segment_bytes, uint32_t rows_per_partition, uint32_t record_overhead)
{
    check(kta_set_segments(ctx_, segment_bytes, rows_per_partition, record_overhead), "kta_set_segments");
    seg_rows_ = rows_per_partition;
}

void HipMetricHandler::replay_compaction(bool on) { check(kta_compaction_replay(ctx_, on ? 1 : 0), "kta_compaction_replay"); }

std::vector<uint64_t> HipMetricHandler::compaction()
{
    std::vector<uint64_t> v((size_t)KTA_COMPACTION_WORDS * (size_t)P_ + KTA_COMPACTION_GLOBALS, 0);
    check(kta_get_compaction(ctx_, v.data(), v.size()), "kta_get_compaction");
    return v;
}

void HipMetricHandler::set_compact_delete(bool on) { check(kta_set_compact_delete(ctx_, on ? 1 : 0), "kta_set_compact_delete"); }

std::vector<uint64_t> HipMetricHandler::compact_delete()
{
    std::vector<uint64_t> v(kta_segments_words(P_, seg_rows_), 0);
    check(kta_get_compact_delete(ctx_, v.data(), v.size()), "kta_get_compact_delete");
    return v;
}

void HipMetricHandler::comm_create(int nranks, int rank, const uint8_t *unique_id)
{
    check(kta_comm_create(ctx_, nranks, rank, unique_id), "kta_comm_create");
}

void HipMetricHandler::exchange(bool tolerate_undelivered)
{
    check(kta_exchange(ctx_), "kta_exchange");
    kta_result r{};
    std::vector<uint64_t> counters((size_t)P_ * KTA_NCOUNTERS);
    const int rc = kta_exchange_result(ctx_, &r, counters.data());
    if (rc == KTA_ERR_TIMESTAMP_RANGE) throw RustPanic(kDateTimePanic, kDateTimePanicAt);
    if (!(rc == KTA_ERR_BAD_PARTITION && tolerate_undelivered)) check(rc, "kta_exchange_result");
    undelivered_ = r.bad_partition_records;
    metrics_ = MessageMetrics(r, std::move(counters), now_);
    lc_ = LogCompactionInMemoryMetrics(r);
    read_analytics();
}

void HipMetricHandler::read_analytics()
{
    if (timeline_.n_buckets) {
        tvec_.assign((size_t)(timeline_.n_buckets + 3) * KTA_TIMELINE_COLS, 0);
        check(kta_exchange_timeline(ctx_, tvec_.data(), tvec_.size()), "kta_exchange_timeline");
    }
    if (sketch_on_) {
        svec_.assign((size_t)P_ * KTA_SKETCH_REGISTERS, 0);
        check(kta_exchange_key_sketch(ctx_, svec_.data(), svec_.size()), "kta_exchange_key_sketch");
    }
    if (hot_on_) {
        hvec_.assign(KTA_HOT_VECTOR_WORDS, 0);
        check(kta_exchange_hot_keys(ctx_, hvec_.data(), hvec_.size()), "kta_exchange_hot_keys");
        hex_.assign((size_t)KTA_HOT_ROWS * KTA_HOT_CELLS, kta_hot_exemplar{});
        check(kta_get_hot_key_exemplars(ctx_, hex_.data(), hex_.size()), "kta_get_hot_key_exemplars");
    }
    if (tso_on_) {
        ovec_.assign(3 * (size_t)P_ + 64, 0);
        check(kta_exchange_ts_order(ctx_, ovec_.data(), ovec_.size()), "kta_exchange_ts_order");
    }
    if (part_on_) {
        pvec_.assign(2 * (size_t)P_ + 2 * (size_t)part_q_, 0);
        check(kta_exchange_partitioner(ctx_, pvec_.data(), pvec_.size()), "kta_exchange_partitioner");
    }
    if (sizeq_on_) {
        qvec_.assign((size_t)P_ * KTA_SIZE_QUANTITIES * KTA_SIZE_BINS + KTA_SIZE_GLOBALS, 0);
        check(kta_exchange_size_quantiles(ctx_, qvec_.data(), qvec_.size()), "kta_exchange_size_quantiles");
    }
    if (rb_on_) {
        bvec_.assign(KTA_RB_WORDS(P_), 0);
        check(kta_exchange_record_batches(ctx_, bvec_.data(), bvec_.size()), "kta_exchange_record_batches");
    }
    if (pl_on_) {
        lvec_.assign(KTA_PAYLOAD_WORDS(P_), 0);
        check(kta_exchange_payload(ctx_, lvec_.data(), lvec_.size()), "kta_exchange_payload");
    }
    if (hn_on_) {
        nvec_.assign(KTA_HEADER_NAMES_WORDS, 0);
        check(kta_exchange_header_names(ctx_, nvec_.data(), nvec_.size()), "kta_exchange_header_names");
        ntab_.assign(KTA_HEADER_NAMES_SLOTS, kta_header_name{});
        check(kta_get_header_name_table(ctx_, ntab_.data(), ntab_.size()), "kta_get_header_name_table");
    }
    if (vb_on_) {
        yvec_.assign(KTA_VALUE_BYTES_WORDS(P_), 0);
        check(kta_exchange_value_bytes(ctx_, yvec_.data(), yvec_.size()), "kta_exchange_value_bytes");
    }
    if (cw_on_) {
        wvec_.assign(KTA_COMPRESS_WHATIF_WORDS(P_), 0);
        check(kta_exchange_compress_whatif(ctx_, wvec_.data(), wvec_.size()), "kta_exchange_compress_whatif");
    }
    if (seg_rows_) {
        gvec_.assign(kta_segments_words((uint32_t)P_, seg_rows_), 0);
        check(kta_exchange_segments(ctx_, gvec_.data(), gvec_.size()), "kta_exchange_segments");
    }
    if (!analytics_on_) return;
    Analytics &a = analytics_;
    a.min_ts_sec.assign((size_t)P_, 0);
    a.max_ts_sec.assign((size_t)P_, 0);
    a.smallest.assign((size_t)P_, 0);
    a.largest.assign((size_t)P_, 0);
    check(kta_exchange_analytics(ctx_, &a.hist, a.min_ts_sec.data(), a.max_ts_sec.data(), a.smallest.data(),
                                 a.largest.data()),
          "kta_exchange_analytics");
}

uint64_t Analytics::records() const
{
    uint64_t n = 0;
    for (int b = 0; b < KTA_HIST_BUCKETS; b++) n += hist.key_size_hist[b];
    return n;
}

}  // namespace kta

// kta_record_batches.h — the record-batch section (KTA_FLAG_RECORD_BATCHES, include/kta_hip.h): the one statement of what a
// Kafka v2 record batch adds to the section's vector, the layout of that vector, the identities between its words and the
// read-off of the producer estimate.  Shared by the kernel (kta_record_batches.hip), the host functions that read, merge and
// restate the vector (kta_api.hip) and the stand-alone check (tests/native/record_batches_check.cpp): plain C++, no HIP
// header.  No reference counterpart.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "kta_kafka.h"

#if defined(__HIPCC__)
#define KTA_RB_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define KTA_RB_HD inline
#endif

namespace kta {

// ---- the vector: u64[20 P + 1524] ------------------------------------------------------------------------------------
//   [16 p, 16 p + 16)                 partition p's sums (RbPartitionWord)
//   [16 P + 100 c, 16 P + 100 c + 100) codec c's sums (RbCodecWord) and its three histograms of 32 bins
//   -- SUM above (16 P + 500 words), unsigned MAX below --
//   [16 P + 500 + 4 p, .. + 4)        partition p's maxima (RbMaxWord)
//   [20 P + 500, 20 P + 1524)         the producer sketch: HyperLogLog, 2^10 registers
enum RbPartitionWord : uint32_t {
    kRbBatches = 0, kRbRecords, kRbWire, kRbPayload, kRbCompressed, kRbCompressedRecbytes, kRbCompressedPayload, kRbExtent,
    kRbTransactional, kRbIdempotent, kRbLogAppendTime, kRbSpanMs, kRbFailed, kRbPartitionSums /* 13; words 13..15 are zero */,
    kRbPartitionWords = 16
};
enum RbCodecWord : uint32_t {
    kRbCodecBatches = 0, kRbCodecRecords, kRbCodecRecbytes, kRbCodecPayload, kRbCodecHistRecords = 4, kRbCodecHistWire = 36,
    kRbCodecHistSpan = 68, kRbCodecWords = 100
};
enum RbMaxWord : uint32_t { kRbMaxRecords = 0, kRbMaxWire, kRbMaxEpoch1, kRbMaxSpanMs, kRbMaxWords = 4 };
constexpr uint32_t kRbCodecs = 5;            // 0 none, 1 gzip, 2 Snappy, 3 LZ4, 4 zstd
constexpr uint32_t kRbHistBins = 32;
constexpr uint32_t kRbSketchBits = 10;
constexpr uint32_t kRbSketchRegs = 1u << kRbSketchBits;
constexpr uint32_t kRbCodecTable = kRbCodecs * kRbCodecWords;   // 500
constexpr uint64_t kRbSpanMax = 0x7FFFFFFFull;
constexpr double kRbStdError = 0.0325;       // 1.04 / sqrt(1024)

KTA_RB_HD size_t rb_sum_words(uint32_t P) { return (size_t)kRbPartitionWords * P + kRbCodecTable; }
KTA_RB_HD size_t rb_codec_at(uint32_t P, uint32_t c) { return (size_t)kRbPartitionWords * P + (size_t)kRbCodecWords * c; }
KTA_RB_HD size_t rb_max_at(uint32_t P, uint32_t p) { return rb_sum_words(P) + (size_t)kRbMaxWords * p; }
KTA_RB_HD size_t rb_sketch_at(uint32_t P) { return rb_sum_words(P) + (size_t)kRbMaxWords * P; }
KTA_RB_HD size_t rb_len(uint32_t P) { return rb_sketch_at(P) + kRbSketchRegs; }

// ---- the fields of a batch that its descriptor does not carry ----------------------------------------------------------
// hdr: the batch's 61 header bytes (the blob at byte_off), big endian, at ANY alignment: bytes are read one by one.
struct RbFields {
    int32_t leader_epoch;        // 12
    int32_t attributes;          // 21 (i16)
    int32_t last_offset_delta;   // 23
    int64_t producer_id;         // 43
};
KTA_RB_HD uint32_t rb_be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]; }
KTA_RB_HD RbFields rb_fields(const uint8_t *hdr)
{
    RbFields f;
    f.leader_epoch = (int32_t)rb_be32(hdr + 12);
    f.attributes = (int32_t)(int16_t)(uint16_t)(((uint32_t)hdr[21] << 8) | (uint32_t)hdr[22]);
    f.last_offset_delta = (int32_t)rb_be32(hdr + 23);
    f.producer_id = (int64_t)(((uint64_t)rb_be32(hdr + 43) << 32) | (uint64_t)rb_be32(hdr + 47));
    return f;
}
// A descriptor whose header does not lie inside the `len` bytes it indexes is no batch of that blob (the index never
// writes one): it is counted as failed, and its header is not read.
KTA_RB_HD bool rb_header_inside(uint64_t byte_off, uint64_t len) { return byte_off <= len && len - byte_off >= KTA_KAFKA_BATCH_HEADER; }

// bin 0 for x == 0, otherwise min(31, 1 + floor(log2 x))
KTA_RB_HD uint32_t rb_bin(uint64_t x)
{
    if (x == 0) return 0u;
    const uint32_t b = 64u - (uint32_t)__builtin_clzll(x);
    return b < kRbHistBins - 1u ? b : kRbHistBins - 1u;
}

KTA_RB_HD uint64_t rb_splitmix64(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- THE RULE: what one batch adds -------------------------------------------------------------------------------------
// The descriptor is read after the inflate and decode kernels of its call: status is final and payload_end - payload_off is
// the exact inflated size.  A failed batch (status != 0, or a header outside the blob) adds 1 to its partition's kRbFailed
// and nothing else anywhere.
struct RbBatch {
    bool failed;
    uint32_t codec;              // 0..4
    uint64_t sums[kRbPartitionSums];
    uint64_t maxima[kRbMaxWords];
    uint64_t recbytes;           // batch_bytes - 61
    bool idempotent;
    uint32_t reg, rank;          // the sketch's register and rank (idempotent batches)
};

KTA_RB_HD uint32_t rb_codec(uint32_t flags)
{
    return (flags & KTA_KB_GZIP) ? 1u : (flags & KTA_KB_SNAPPY) ? 2u : (flags & KTA_KB_LZ4) ? 3u : (flags & KTA_KB_ZSTD) ? 4u : 0u;
}

// span_ms = clamp(max_ts_ms - base_ts_ms, 0, 2^31 - 1), without a signed overflow
KTA_RB_HD uint64_t rb_span(int64_t base_ts_ms, int64_t max_ts_ms)
{
    if (max_ts_ms <= base_ts_ms) return 0;
    const uint64_t d = (uint64_t)max_ts_ms - (uint64_t)base_ts_ms;
    return d < kRbSpanMax ? d : kRbSpanMax;
}

KTA_RB_HD RbBatch rb_failed_batch()
{
    RbBatch b;
    b.failed = true, b.codec = 0, b.recbytes = 0, b.idempotent = false, b.reg = 0, b.rank = 0;
    for (uint32_t k = 0; k < kRbPartitionSums; k++) b.sums[k] = 0;
    for (uint32_t k = 0; k < kRbMaxWords; k++) b.maxima[k] = 0;
    b.sums[kRbFailed] = 1;
    return b;
}

KTA_RB_HD RbBatch rb_batch(const kta_kafka_batch_desc &d, const RbFields &f)
{
    if (d.status != 0) return rb_failed_batch();
    RbBatch b;
    b.failed = false;
    b.codec = rb_codec(d.flags);
    const uint64_t records = d.n_records > 0 ? (uint64_t)d.n_records : 0;
    const uint64_t wire = d.batch_bytes;
    b.recbytes = wire >= KTA_KAFKA_BATCH_HEADER ? wire - KTA_KAFKA_BATCH_HEADER : 0;
    const uint64_t payload = d.payload_end >= d.payload_off ? d.payload_end - d.payload_off : 0;
    const uint64_t span = rb_span(d.base_ts_ms, d.max_ts_ms);
    const int64_t last1 = (int64_t)f.last_offset_delta + 1;
    const uint64_t extent = last1 > (int64_t)records ? (uint64_t)last1 : records;
    const bool compressed = b.codec != 0;
    b.idempotent = f.producer_id >= 0;
    b.sums[kRbBatches] = 1;
    b.sums[kRbRecords] = records;
    b.sums[kRbWire] = wire;
    b.sums[kRbPayload] = payload;
    b.sums[kRbCompressed] = compressed ? 1 : 0;
    b.sums[kRbCompressedRecbytes] = compressed ? b.recbytes : 0;
    b.sums[kRbCompressedPayload] = compressed ? payload : 0;
    b.sums[kRbExtent] = extent;
    b.sums[kRbTransactional] = (d.flags & KTA_KB_TRANSACTIONAL) ? 1 : 0;
    b.sums[kRbIdempotent] = b.idempotent ? 1 : 0;
    b.sums[kRbLogAppendTime] = (d.flags & KTA_KB_LOG_APPEND_TIME) ? 1 : 0;
    b.sums[kRbSpanMs] = span;
    b.sums[kRbFailed] = 0;
    b.maxima[kRbMaxRecords] = records;
    b.maxima[kRbMaxWire] = wire;
    b.maxima[kRbMaxEpoch1] = f.leader_epoch >= 0 ? (uint64_t)f.leader_epoch + 1 : 0;   // (0: none seen, or epoch -1)
    b.maxima[kRbMaxSpanMs] = span;
    const uint64_t h = rb_splitmix64((uint64_t)f.producer_id);
    b.reg = (uint32_t)(h >> (64 - kRbSketchBits));
    b.rank = 1u + (uint32_t)__builtin_clzll((h << kRbSketchBits) | (1ull << (kRbSketchBits - 1)));
    return b;
}

// Which batches are counted.  A partition outside [0, P) never is (its records land in KTA_G_BAD_PARTITION).  With a filter
// (kta_set_filter; kta_filter.h has the record rule) a batch is counted iff its partition is selected and its
// [base_ts_ms, max_ts_ms] overlaps [from_ms, to_ms): base_ts_ms < to_ms && max_ts_ms >= from_ms, a bound that is absent
// being open — the tile summary's decision (filter_tile_decide) at batch grain: "batches that overlap the window".
// The filter as this pass takes it, FilterSpec's window and set: from_ms == INT64_MIN / to_ms == INT64_MAX no bound on that
// side; bitmap null: no partition set, else ceil(P / 32) words, bit p of word p / 32 for partition p.
struct RbFilter {
    int64_t from_ms, to_ms;
    const uint32_t *bitmap;
};
KTA_RB_HD RbFilter rb_no_filter() { return RbFilter{INT64_MIN, INT64_MAX, nullptr}; }
KTA_RB_HD bool rb_counted(const RbFilter &f, uint32_t P, int32_t partition, int64_t base_ts_ms, int64_t max_ts_ms)
{
    if ((uint32_t)partition >= P) return false;   // (a negative partition is a large unsigned one)
    if (f.bitmap && !((f.bitmap[(uint32_t)partition >> 5] >> ((uint32_t)partition & 31u)) & 1u)) return false;
    if (f.to_ms != INT64_MAX && !(base_ts_ms < f.to_ms)) return false;
    if (f.from_ms != INT64_MIN && !(max_ts_ms >= f.from_ms)) return false;
    return true;
}

// The rule on the host, one batch into a vector (the device adds the same RbBatch through LDS and atomics).
inline void rb_accumulate(uint64_t *vec, uint32_t P, uint32_t partition, const RbBatch &b)
{
    uint64_t *pw = vec + (size_t)kRbPartitionWords * partition;
    for (uint32_t k = 0; k < kRbPartitionSums; k++) pw[k] += b.sums[k];
    if (b.failed) return;
    uint64_t *cw = vec + rb_codec_at(P, b.codec);
    cw[kRbCodecBatches] += 1;
    cw[kRbCodecRecords] += b.sums[kRbRecords];
    cw[kRbCodecRecbytes] += b.recbytes;
    cw[kRbCodecPayload] += b.sums[kRbPayload];
    cw[kRbCodecHistRecords + rb_bin(b.sums[kRbRecords])] += 1;
    cw[kRbCodecHistWire + rb_bin(b.sums[kRbWire])] += 1;
    cw[kRbCodecHistSpan + rb_bin(b.sums[kRbSpanMs])] += 1;
    uint64_t *mw = vec + rb_max_at(P, partition);
    for (uint32_t k = 0; k < kRbMaxWords; k++)
        if (b.maxima[k] > mw[k]) mw[k] = b.maxima[k];
    if (b.idempotent) {
        uint64_t *reg = vec + rb_sketch_at(P) + b.reg;
        if (b.rank > *reg) *reg = b.rank;
    }
}

// ---- identities ----------------------------------------------------------------------------------------------------------
inline uint64_t rb_partition_total(const uint64_t *vec, uint32_t P, uint32_t word)
{
    uint64_t s = 0;
    for (uint32_t p = 0; p < P; p++) s += vec[(size_t)kRbPartitionWords * p + word];
    return s;
}
inline uint64_t rb_codec_total(const uint64_t *vec, uint32_t P, uint32_t word, uint32_t first_codec)
{
    uint64_t s = 0;
    for (uint32_t c = first_codec; c < kRbCodecs; c++) s += vec[rb_codec_at(P, c) + word];
    return s;
}
// Every identity between the words of one vector:
//   sum over codecs of batches / records / payload == sum over partitions of words 0 / 1 / 3;
//   words 5 and 6 summed over partitions == words 2 and 3 summed over codecs 1..4;
//   each of a codec's three histograms sums to its batches;  words 13..15 of a partition are zero.
inline bool rb_identities_hold(const uint64_t *vec, uint32_t P)
{
    if (rb_codec_total(vec, P, kRbCodecBatches, 0) != rb_partition_total(vec, P, kRbBatches)) return false;
    if (rb_codec_total(vec, P, kRbCodecRecords, 0) != rb_partition_total(vec, P, kRbRecords)) return false;
    if (rb_codec_total(vec, P, kRbCodecPayload, 0) != rb_partition_total(vec, P, kRbPayload)) return false;
    if (rb_codec_total(vec, P, kRbCodecRecbytes, 1) != rb_partition_total(vec, P, kRbCompressedRecbytes)) return false;
    if (rb_codec_total(vec, P, kRbCodecPayload, 1) != rb_partition_total(vec, P, kRbCompressedPayload)) return false;
    if (rb_codec_total(vec, P, kRbCodecBatches, 1) != rb_partition_total(vec, P, kRbCompressed)) return false;
    for (uint32_t c = 0; c < kRbCodecs; c++) {
        const uint64_t *cw = vec + rb_codec_at(P, c);
        for (uint32_t h : {(uint32_t)kRbCodecHistRecords, (uint32_t)kRbCodecHistWire, (uint32_t)kRbCodecHistSpan}) {
            uint64_t s = 0;
            for (uint32_t b = 0; b < kRbHistBins; b++) s += cw[h + b];
            if (s != cw[kRbCodecBatches]) return false;
        }
    }
    for (uint32_t p = 0; p < P; p++)
        for (uint32_t k = kRbPartitionSums; k < kRbPartitionWords; k++)
            if (vec[(size_t)kRbPartitionWords * p + k] != 0) return false;
    return true;
}
// With the counter vector of the same run (no failed batch, no filter): sum over partitions of word 1 == the counters' total
// records plus their tombstones, every record delivered on a valid partition.
inline uint64_t rb_records_delivered(const uint64_t *vec, uint32_t P) { return rb_partition_total(vec, P, kRbRecords); }

// ---- the producer estimate ---------------------------------------------------------------------------------------------
// HyperLogLog over regs[1024] (ranks, 0 = empty): E = alpha m^2 / sum 2^-reg, alpha = 0.7213 / (1 + 1.079 / m); linear
// counting m ln(m / V) while E <= 2.5 m and V > 0 registers are empty.  Standard error 1.04 / sqrt(m) = 3.25 %.
inline double rb_estimate(const uint64_t *regs)
{
    const double m = (double)kRbSketchRegs;
    double sum = 0.0;
    uint32_t empty = 0;
    for (uint32_t i = 0; i < kRbSketchRegs; i++) {
        const uint64_t r = regs[i] < 64 ? regs[i] : 64;
        sum += ldexp(1.0, -(int)r);
        empty += regs[i] == 0;
    }
    if (empty == kRbSketchRegs) return 0.0;
    const double e = 0.7213 / (1.0 + 1.079 / m) * m * m / sum;
    if (e <= 2.5 * m && empty) return m * log(m / (double)empty);
    return e;
}

} // namespace kta

// kta_value_bytes.h — the value-byte section (KTA_FLAG_VALUE_BYTES, include/kta_hip.h): the one statement of what a record of
// a Kafka v2 batch adds to the section's vector — a histogram of the bytes of its value and the bytes that repeat the one in
// front of them —, the layout of that vector, the identities between its words and the read-off (entropy, shares, class).
// Shared by the kernel (kta_value_bytes.hip), the host functions that read, merge and restate the vector (kta_api.hip), the
// renderer (host/report.cpp) and the stand-alone check (tests/native/value_bytes_check.cpp): plain C++, no HIP header.  Which
// records count and the record grammar are kta_payload.h's.  No reference counterpart.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "kta_payload.h"

namespace kta {

// ---- the vector: u64[264 P], every word a SUM ---------------------------------------------------------------------------
//   [264 p, 264 p + 256)      partition p's bins: bin b counts the value bytes equal to b
//   264 p + 256 .. 259        records (counted), values (val_len > 0), bytes, repeats
//   264 p + 260 .. 263        zero
enum ValueBytesWord : uint32_t {
    kVbBins = 256,
    kVbRecords = 256, kVbValues, kVbBytes, kVbRepeats,
    kVbPartitionSums = 260,   // words 260..263 are zero
    kVbPartitionWords = 264
};

KTA_PL_HD size_t value_bytes_len(uint32_t P) { return (size_t)kVbPartitionWords * P; }

// ---- THE RULE: what one counted record adds (host form; the kernel adds the same words from LDS and registers) ----------
// A record COUNTS under the payload section's rule (kta_payload.h, above payload_add).  val_len: -1 null.  Every byte b at
// position i of a value of val_len > 0 adds 1 to bin b, and 1 to repeats when i > 0 and it equals the byte at i - 1 of the
// same value: never the byte in front of the value.
inline void value_bytes_add(uint64_t *vec, uint32_t partition, long long val_len, const uint8_t *value)
{
    uint64_t *w = vec + (size_t)kVbPartitionWords * partition;
    w[kVbRecords]++;
    if (val_len <= 0) return;
    w[kVbValues]++, w[kVbBytes] += (uint64_t)val_len;
    for (long long i = 0; i < val_len; i++) {
        w[value[i]]++;
        if (i > 0 && value[i] == value[i - 1]) w[kVbRepeats]++;
    }
}

// The records of one batch's payload [pos, end), as payload_batch_host walks them.
template <class Passes>
inline void value_bytes_batch_host(uint64_t *vec, uint32_t partition, const uint8_t *bytes, uint64_t pos, uint64_t end, uint64_t n_records, Passes passes)
{
    payload_records_host(bytes, pos, end, n_records, passes,
                         [&](long long val_len, uint64_t value, uint64_t, uint64_t) { value_bytes_add(vec, partition, val_len, bytes + value); });
}

// ---- the identities between the words of one vector ---------------------------------------------------------------------
// payload: NULL, or the payload vector of the same run: records, bytes (the five class-byte words) and values (framed + json
// + other) agree per partition.  counters: NULL, or the counter vector as payload_identities_hold takes it (an unfiltered run
// without failed batches): records == total messages, per partition.
inline bool value_bytes_identities_hold(const uint64_t *vec, uint32_t P, const uint64_t *payload = nullptr, const uint64_t *counters = nullptr,
                                        size_t stride = 0)
{
    for (uint32_t p = 0; p < P; p++) {
        const uint64_t *w = vec + (size_t)kVbPartitionWords * p;
        uint64_t in_bins = 0;
        for (uint32_t b = 0; b < kVbBins; b++) in_bins += w[b];
        if (in_bins != w[kVbBytes] || w[kVbValues] > w[kVbRecords] || w[kVbValues] > w[kVbBytes] || w[kVbRepeats] > w[kVbBytes] - w[kVbValues]) return false;
        for (uint32_t k = kVbPartitionSums; k < kVbPartitionWords; k++)
            if (w[k]) return false;
        if (payload) {
            const uint64_t *l = payload + (size_t)kPlPartitionWords * p;
            uint64_t class_bytes = 0;
            for (uint32_t c = 0; c < kPlClasses; c++) class_bytes += l[kPlClassBytes + c];
            if (w[kVbRecords] != l[kPlRecords] || w[kVbBytes] != class_bytes ||
                w[kVbValues] != l[kPlClass + kPlFramed] + l[kPlClass + kPlJson] + l[kPlClass + kPlOther])
                return false;
        }
        if (counters && w[kVbRecords] != counters[stride * p]) return false;
    }
    return true;
}

// ---- the read-off -------------------------------------------------------------------------------------------------------
// Of one partition's 264 words, or of their sum over the topic.  entropy_bits: H0 = - sum (c / B) log2(c / B) in double, over
// the non-zero bins in ascending byte order; 0 when B = 0.  floor_bytes: ceil(B H0 / 8), what an order-0 entropy coder alone
// could not go below.  printable: bins 0x20 .. 0x7E plus \t \n \r.  top_byte: the most common byte, the lowest on a tie.
// The class is a HEURISTIC, the first that holds: none (B = 0), text (printable >= 95 % of B), dense (B >= 65 536 and H0 >=
// 7.5: compressed, encrypted or random already), binary.
enum ValueBytesClass : uint32_t { kVbNone = 0, kVbText, kVbDense, kVbBinary };
constexpr uint64_t kVbDenseMinBytes = 65536;
constexpr double kVbDenseMinBits = 7.5;

struct ValueBytesSummary {
    uint64_t records, values, bytes, repeats;
    uint64_t distinct, floor_bytes, printable, zero, high, top_count;
    double entropy_bits;
    uint32_t top_byte, cls;
};

inline const char *value_bytes_class_name(uint32_t cls) { return cls == kVbNone ? "none" : cls == kVbText ? "text" : cls == kVbDense ? "dense" : "binary"; }

inline ValueBytesSummary value_bytes_summary(const uint64_t *w)
{
    ValueBytesSummary s;
    s.records = w[kVbRecords], s.values = w[kVbValues], s.bytes = w[kVbBytes], s.repeats = w[kVbRepeats];
    s.distinct = s.printable = s.high = s.top_count = 0, s.zero = w[0], s.top_byte = 0;
    uint64_t B = 0;
    for (uint32_t b = 0; b < kVbBins; b++) B += w[b];                          // (== bytes in a vector the rule wrote)
    double h = 0.0;
    for (uint32_t b = 0; b < kVbBins; b++) {
        const uint64_t c = w[b];
        if (!c) continue;
        s.distinct++;
        if ((b >= 0x20u && b <= 0x7Eu) || b == '\t' || b == '\n' || b == '\r') s.printable += c;
        if (b >= 0x80u) s.high += c;
        if (c > s.top_count) s.top_count = c, s.top_byte = b;
        const double q = (double)c / (double)B;
        h -= q * log2(q);
    }
    if (h < 0.0) h = 0.0;                                                      // (-0.0 of a single bin)
    s.entropy_bits = h;
    s.floor_bytes = (uint64_t)ceil((double)B * h / 8.0);
    // printable >= 95 % of B, in integers: 20 printable >= 19 B (128 bits: B may be anything a u64 holds)
    const bool text = (unsigned __int128)s.printable * 20u >= (unsigned __int128)B * 19u;
    s.cls = B == 0 ? kVbNone : text ? kVbText : (B >= kVbDenseMinBytes && h >= kVbDenseMinBits) ? kVbDense : kVbBinary;
    return s;
}

// The sum over the partitions, as value_bytes_summary takes it.
inline void value_bytes_topic(const uint64_t *vec, uint32_t P, uint64_t out[kVbPartitionWords])
{
    for (uint32_t k = 0; k < kVbPartitionWords; k++) out[k] = 0;
    for (uint32_t p = 0; p < P; p++)
        for (uint32_t k = 0; k < kVbPartitionWords; k++) out[k] += vec[(size_t)kVbPartitionWords * p + k];
}

} // namespace kta

// record_batches_check.cpp — csrc/kta_record_batches.h on the CPU, as a program of its own (built with
// -fsanitize=address,undefined by tests/test_record_batches_host.py and run directly): the header fields read at every
// alignment of byte_off from heap buffers that END with the header (a read past byte 60 is an ASan report), the bounds test
// for truncated headers, the rule on extreme field values against the definition said again, the layout, the identities
// after a few thousand accumulated batches and the estimator.  Prints "OK <checks>" and returns 0, or says what failed and
// returns 1.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "kta_record_batches.h"

namespace {

int g_failed = 0;
long g_checks = 0;

#define CHECK(cond, ...)                                     \
    do {                                                     \
        g_checks++;                                          \
        if (!(cond)) {                                       \
            if (g_failed++ < 20) {                           \
                fprintf(stderr, "line %d: ", __LINE__);      \
                fprintf(stderr, __VA_ARGS__);                \
                fprintf(stderr, "\n");                       \
            }                                                \
        }                                                    \
    } while (0)

void put_be(uint8_t *p, uint64_t v, int bytes)
{
    for (int i = 0; i < bytes; i++) p[i] = (uint8_t)(v >> (8 * (bytes - 1 - i)));
}

// a 61-byte header with the four fields, everything else 0xEE
void make_header(uint8_t *h, int32_t epoch, int16_t attrs, int32_t lod, int64_t pid)
{
    memset(h, 0xEE, KTA_KAFKA_BATCH_HEADER);
    put_be(h + 12, (uint32_t)epoch, 4);
    put_be(h + 21, (uint16_t)attrs, 2);
    put_be(h + 23, (uint32_t)lod, 4);
    put_be(h + 43, (uint64_t)pid, 8);
}

uint32_t bin_by_definition(uint64_t x)
{
    if (x == 0) return 0;
    uint32_t e = 0;
    while (e < 63 && (x >> (e + 1)) != 0) e++;
    return 1 + e < 31 ? 1 + e : 31;
}

kta_kafka_batch_desc desc(int32_t n, uint32_t bytes, int64_t base, int64_t max, uint32_t flags, uint32_t status, uint64_t off, uint64_t end)
{
    kta_kafka_batch_desc d;
    memset(&d, 0, sizeof d);
    d.n_records = n, d.batch_bytes = bytes, d.base_ts_ms = base, d.max_ts_ms = max, d.flags = flags, d.status = status;
    d.payload_off = off, d.payload_end = end;
    return d;
}

} // namespace

int main()
{
    using namespace kta;
    // ---- layout
    for (uint32_t P : {1u, 7u, 4096u}) {
        CHECK(rb_len(P) == 20ull * P + 1524, "len");
        CHECK(rb_sum_words(P) == 16ull * P + 500, "sum words");
        CHECK(rb_codec_at(P, 4) + kRbCodecWords == rb_sum_words(P), "codec table ends the SUM prefix");
        CHECK(rb_max_at(P, P - 1) + kRbMaxWords == rb_sketch_at(P) && rb_sketch_at(P) + kRbSketchRegs == rb_len(P), "MAX suffix");
    }
    CHECK(kRbCodecHistSpan + kRbHistBins == kRbCodecWords && kRbCodecHistWire + kRbHistBins == kRbCodecHistSpan, "histograms");

    // ---- the fields at every alignment, the header the LAST bytes of its heap buffer
    const int32_t epochs[] = {-1, 0, 5, INT32_MAX, INT32_MIN};
    const int16_t attrs[] = {0, 0x18, 0x7FFF, (int16_t)0x8000, -1};
    const int32_t lods[] = {-1, 0, 41, INT32_MAX, INT32_MIN};
    const int64_t pids[] = {-1, 0, 1, INT64_MAX, INT64_MIN, 0x0102030405060708ll};
    for (size_t align = 0; align < 16; align++)
        for (int32_t e : epochs)
            for (int16_t a : attrs)
                for (int32_t l : lods)
                    for (int64_t p : pids) {
                        std::vector<uint8_t> buf(align + KTA_KAFKA_BATCH_HEADER);
                        make_header(buf.data() + align, e, a, l, p);
                        CHECK(rb_header_inside(align, buf.size()), "inside");
                        const RbFields f = rb_fields(buf.data() + align);
                        CHECK(f.leader_epoch == e && f.attributes == (int32_t)a && f.last_offset_delta == l && f.producer_id == p,
                              "fields at alignment %zu", align);
                    }
    // ---- truncated headers at the end of a buffer: refused by the bounds test, never read
    for (uint64_t len = 0; len < 200; len++)
        for (uint64_t off = 0; off < 210; off++)
            CHECK(rb_header_inside(off, len) == (off + KTA_KAFKA_BATCH_HEADER <= len), "bounds %llu %llu", (unsigned long long)off, (unsigned long long)len);
    CHECK(!rb_header_inside(UINT64_MAX, 100) && !rb_header_inside(UINT64_MAX - 30, UINT64_MAX), "bounds do not wrap");

    // ---- bin, span
    for (int e = 0; e < 64; e++)
        for (int64_t d = -1; d <= 1; d++) {
            const uint64_t x = (1ull << e) + (uint64_t)d;
            CHECK(rb_bin(x) == bin_by_definition(x), "bin %llu", (unsigned long long)x);
        }
    CHECK(rb_bin(0) == 0 && rb_bin(1) == 1 && rb_bin(2) == 2 && rb_bin(3) == 2 && rb_bin(UINT64_MAX) == 31, "bin ends");
    CHECK(rb_span(5, 5) == 0 && rb_span(5, 6) == 1 && rb_span(6, 5) == 0, "span small");
    CHECK(rb_span(0, 0x7FFFFFFF) == 0x7FFFFFFF && rb_span(0, 0x80000000ll) == 0x7FFFFFFF, "span clamp");
    CHECK(rb_span(INT64_MIN, INT64_MAX) == 0x7FFFFFFF && rb_span(INT64_MAX, INT64_MIN) == 0 && rb_span(-1, INT64_MAX) == 0x7FFFFFFF, "span extremes");

    // ---- the rule on extreme values
    {
        uint8_t h[KTA_KAFKA_BATCH_HEADER];
        make_header(h, 5, 0, 9, 77);
        RbBatch b = rb_batch(desc(4, 161, 1000, 1003, KTA_KB_LZ4 | KTA_KB_TRANSACTIONAL, 0, 4096, 4096 + 300), rb_fields(h));
        CHECK(!b.failed && b.codec == 3 && b.recbytes == 100 && b.idempotent, "lz4 batch");
        CHECK(b.sums[kRbBatches] == 1 && b.sums[kRbRecords] == 4 && b.sums[kRbWire] == 161 && b.sums[kRbPayload] == 300 && b.sums[kRbCompressed] == 1 &&
                  b.sums[kRbCompressedRecbytes] == 100 && b.sums[kRbCompressedPayload] == 300 && b.sums[kRbExtent] == 10 &&
                  b.sums[kRbTransactional] == 1 && b.sums[kRbIdempotent] == 1 && b.sums[kRbLogAppendTime] == 0 && b.sums[kRbSpanMs] == 3 &&
                  b.sums[kRbFailed] == 0,
              "sums");
        CHECK(b.maxima[kRbMaxRecords] == 4 && b.maxima[kRbMaxWire] == 161 && b.maxima[kRbMaxEpoch1] == 6 && b.maxima[kRbMaxSpanMs] == 3, "maxima");
        CHECK(b.reg < kRbSketchRegs && b.rank >= 1 && b.rank <= 55, "register and rank");
        make_header(h, -1, 0, INT32_MAX, -1);
        b = rb_batch(desc(INT32_MAX, UINT32_MAX, INT64_MIN, INT64_MAX, KTA_KB_LOG_APPEND_TIME, 0, 61, (uint64_t)UINT32_MAX), rb_fields(h));
        CHECK(b.codec == 0 && !b.idempotent && b.sums[kRbExtent] == 0x80000000ull && b.sums[kRbSpanMs] == 0x7FFFFFFF && b.maxima[kRbMaxEpoch1] == 0 &&
                  b.sums[kRbLogAppendTime] == 1 && b.sums[kRbCompressedRecbytes] == 0,
              "extremes");
        make_header(h, INT32_MIN, -1, INT32_MIN, INT64_MIN);
        b = rb_batch(desc(3, 61, 0, 0, 0, 0, 10, 5 /* end before off */), rb_fields(h));
        CHECK(b.sums[kRbExtent] == 3 && b.sums[kRbPayload] == 0 && b.recbytes == 0 && b.maxima[kRbMaxEpoch1] == 0 && !b.idempotent, "degenerate");
        b = rb_batch(desc(3, 100, 0, 9, KTA_KB_GZIP, KTA_KB_BAD_FRAMING, 0, 50), rb_fields(h));
        CHECK(b.failed && b.sums[kRbFailed] == 1, "failed");
        for (uint32_t k = 0; k < kRbPartitionSums; k++) CHECK(k == kRbFailed || b.sums[k] == 0, "a failed batch adds nothing else");
        for (int r = 0; r < 10; r++) CHECK(rb_codec(r == 0 ? 0u : r == 1 ? KTA_KB_GZIP : r == 2 ? KTA_KB_SNAPPY : r == 3 ? KTA_KB_LZ4 : KTA_KB_ZSTD) == (uint32_t)(r < 5 ? r : 4), "codec");
    }
    // every rank the sketch can take: h with `z` leading zeros behind the register bits
    for (uint32_t z = 0; z <= 54; z++) {
        const uint64_t tail = z == 54 ? 0 : 1ull << (53 - z);
        const uint64_t w = (tail << kRbSketchBits) | (1ull << (kRbSketchBits - 1));
        CHECK(1u + (uint32_t)__builtin_clzll(w) == z + 1, "rank %u", z);
    }

    // ---- the counted-batch predicate
    {
        const uint32_t bitmap[1] = {0x5u};   // partitions 0 and 2
        const RbFilter none = rb_no_filter(), set{INT64_MIN, INT64_MAX, bitmap}, win{100, 200, nullptr}, both{100, 200, bitmap};
        CHECK(rb_counted(none, 4, 3, 0, 0) && !rb_counted(none, 4, 4, 0, 0) && !rb_counted(none, 4, -1, 0, 0), "partition range");
        CHECK(rb_counted(set, 4, 0, 0, 0) && !rb_counted(set, 4, 1, 0, 0) && rb_counted(set, 4, 2, 0, 0), "set");
        CHECK(rb_counted(win, 4, 1, 50, 100) && !rb_counted(win, 4, 1, 50, 99) && rb_counted(win, 4, 1, 199, 500) && !rb_counted(win, 4, 1, 200, 500) &&
                  rb_counted(win, 4, 1, 0, 1000),
              "window overlap");
        CHECK(rb_counted(both, 4, 2, 150, 150) && !rb_counted(both, 4, 1, 150, 150), "both");
        const RbFilter from_only{100, INT64_MAX, nullptr}, to_only{INT64_MIN, 200, nullptr};
        CHECK(rb_counted(from_only, 4, 0, INT64_MAX, INT64_MAX) && !rb_counted(from_only, 4, 0, 0, 99) && rb_counted(to_only, 4, 0, INT64_MIN, INT64_MIN) &&
                  !rb_counted(to_only, 4, 0, 200, 300),
              "open bounds");
    }

    // ---- a few thousand batches: the identities, and the host accumulation against sums kept here
    {
        const uint32_t P = 5;
        std::vector<uint64_t> vec(rb_len(P), 0);
        uint64_t x = 88172645463325252ull, batches = 0, failed = 0;
        uint8_t h[KTA_KAFKA_BATCH_HEADER];
        for (int i = 0; i < 5000; i++) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            const uint32_t codec = (uint32_t)(x % 5), p = (uint32_t)((x >> 8) % P);
            const uint32_t flags = (codec == 1 ? KTA_KB_GZIP : codec == 2 ? KTA_KB_SNAPPY : codec == 3 ? KTA_KB_LZ4 : codec == 4 ? KTA_KB_ZSTD : 0u) |
                                   ((x >> 16) & 1 ? KTA_KB_TRANSACTIONAL : 0u) | ((x >> 17) & 1 ? KTA_KB_LOG_APPEND_TIME : 0u);
            const int32_t n = 1 + (int32_t)((x >> 20) % 3000);
            const uint32_t bytes = 61 + (uint32_t)((x >> 32) % 100000);
            const uint64_t payload = codec ? (x >> 40) % 500000 : bytes - 61;
            const bool bad = (x >> 60) == 0;
            make_header(h, (int32_t)((x >> 24) % 9) - 1, 0, n - 1 + (int32_t)((x >> 28) % 3), (x >> 18) & 1 ? -1 : (int64_t)((x >> 44) % 300));
            rb_accumulate(vec.data(), P, p, rb_batch(desc(n, bytes, 1000, 1000 + (int64_t)((x >> 50) % 70000), flags, bad ? 2u : 0u, 1 << 20, (1 << 20) + payload), rb_fields(h)));
            batches += !bad, failed += bad;
        }
        CHECK(rb_identities_hold(vec.data(), P), "identities");
        CHECK(rb_partition_total(vec.data(), P, kRbBatches) == batches && rb_partition_total(vec.data(), P, kRbFailed) == failed, "totals");
        vec[rb_codec_at(P, 2) + kRbCodecHistWire + 3] += 1;
        CHECK(!rb_identities_hold(vec.data(), P), "a broken histogram is seen");
    }

    // ---- the estimator: empty, exact while few, within 4 standard errors at 100 000
    {
        std::vector<uint64_t> regs(kRbSketchRegs, 0);
        CHECK(rb_estimate(regs.data()) == 0.0, "empty");
        auto add = [&](uint64_t id) {
            const uint64_t hh = rb_splitmix64(id);
            const uint32_t reg = (uint32_t)(hh >> 54), rank = 1u + (uint32_t)__builtin_clzll((hh << 10) | (1ull << 9));
            if (rank > regs[reg]) regs[reg] = rank;
        };
        add(12345);
        CHECK((long)(rb_estimate(regs.data()) + 0.5) == 1, "one id");
        for (uint64_t id = 0; id < 100000; id++) add(id * 7919 + 13);
        const double e = rb_estimate(regs.data());
        CHECK(e > 100000 * (1 - 4 * kRbStdError) && e < 100000 * (1 + 4 * kRbStdError), "estimate %f", e);
        CHECK(rb_splitmix64(0) == 0xE220A8397B1DCDAFull, "splitmix64's first output for seed 0");
    }

    if (g_failed) {
        fprintf(stderr, "%d of %ld checks failed\n", g_failed, g_checks);
        return 1;
    }
    printf("OK %ld\n", g_checks);
    return 0;
}

// value_bytes_check.cpp — test infrastructure: csrc/kta_value_bytes.h (and through it kta_payload.h's record walk) driven
// natively with boundary vectors, a program of its own so that it can be built with -fsanitize=address,undefined and run
// directly (tests/test_value_bytes_host.py).  It checks the rule, the identities — each of them broken once — and the read-off
// on: an empty vector, one byte, a constant value, all 256 byte values alike, a text, counts near 2^63, and a record section
// walked on the host.  (The rendered section lives in host/report.cpp, which needs the library: tests/test_value_bytes_host.py
// holds it against the restatement and a golden text.)  Exit status 0 and "OK" when every check holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "kta_value_bytes.h"

using namespace kta;

static int failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);        \
            failures++;                                             \
        }                                                           \
    } while (0)

static void add(std::vector<uint64_t> &vec, uint32_t partition, const std::string &value)
{
    value_bytes_add(vec.data(), partition, (long long)value.size(), reinterpret_cast<const uint8_t *>(value.data()));
}

int main()
{
    const uint32_t P = 3;
    // empty: class none, no entropy, nothing divides by zero
    {
        std::vector<uint64_t> vec(value_bytes_len(P), 0);
        CHECK(value_bytes_identities_hold(vec.data(), P));
        const ValueBytesSummary s = value_bytes_summary(vec.data());
        CHECK(s.cls == kVbNone && s.bytes == 0 && s.entropy_bits == 0.0 && s.floor_bytes == 0 && s.distinct == 0 && s.top_count == 0);
    }
    // null and empty values count as records only; one byte; a constant value
    {
        std::vector<uint64_t> vec(value_bytes_len(P), 0);
        value_bytes_add(vec.data(), 1, -1, nullptr);
        value_bytes_add(vec.data(), 1, 0, nullptr);
        add(vec, 1, "A");
        const uint64_t *w = vec.data() + kVbPartitionWords;
        CHECK(w[kVbRecords] == 3 && w[kVbValues] == 1 && w[kVbBytes] == 1 && w[kVbRepeats] == 0 && w['A'] == 1);
        ValueBytesSummary s = value_bytes_summary(w);
        CHECK(s.cls == kVbText && s.entropy_bits == 0.0 && s.floor_bytes == 0 && s.distinct == 1 && s.top_byte == 'A' && s.top_count == 1 && s.printable == 1);
        add(vec, 1, std::string(1000, '\0'));
        CHECK(w[kVbRepeats] == 999 && w[0] == 1000 && value_bytes_identities_hold(vec.data(), P));
        s = value_bytes_summary(w);
        CHECK(s.cls == kVbBinary && s.zero == 1000 && s.top_byte == 0 && s.entropy_bits > 0.0 && s.entropy_bits < 0.02);
        CHECK(vec[0] == 0 && vec[2 * kVbPartitionWords + kVbRecords] == 0);     // the other partitions are untouched
    }
    // all 256 byte values alike: H0 = 8 exactly, the floor is the bytes; dense only from 65 536 bytes on; a tie goes to the lowest byte
    {
        std::vector<uint64_t> vec(value_bytes_len(P), 0);
        std::string all;
        for (int b = 0; b < 256; b++) all += (char)b;
        for (int k = 0; k < 255; k++) add(vec, 0, all);
        ValueBytesSummary s = value_bytes_summary(vec.data());
        CHECK(s.entropy_bits == 8.0 && s.floor_bytes == s.bytes && s.bytes == 255 * 256 && s.cls == kVbBinary && s.top_byte == 0 && s.top_count == 255);
        CHECK(s.high == s.bytes / 2 && s.printable == 255 * 98 && s.distinct == 256 && s.repeats == 0);
        add(vec, 0, all);
        s = value_bytes_summary(vec.data());
        CHECK(s.bytes == 65536 && s.cls == kVbDense && value_bytes_identities_hold(vec.data(), P));
    }
    // text: 95 % printable is text, one byte less is not
    {
        std::vector<uint64_t> vec(value_bytes_len(P), 0);
        add(vec, 2, std::string(95, 'a') + std::string(5, '\x01'));
        CHECK(value_bytes_summary(vec.data() + 2 * kVbPartitionWords).cls == kVbText);
        add(vec, 2, std::string(94, '\n') + std::string(6, '\x7f'));
        CHECK(value_bytes_summary(vec.data() + 2 * kVbPartitionWords).cls == kVbBinary);
        uint64_t topic[kVbPartitionWords];
        value_bytes_topic(vec.data(), P, topic);
        CHECK(topic[kVbBytes] == 200 && topic['a'] == 95 && topic[kVbRecords] == 2);
    }
    // counts near 2^63: the sums and the products of the class rule do not wrap
    {
        std::vector<uint64_t> vec(value_bytes_len(1), 0);
        vec['x'] = 1ull << 62, vec[0xFF] = 1ull << 62, vec[kVbBytes] = 1ull << 63, vec[kVbValues] = 5, vec[kVbRecords] = 5;
        CHECK(value_bytes_identities_hold(vec.data(), 1));
        const ValueBytesSummary s = value_bytes_summary(vec.data());
        CHECK(s.entropy_bits == 1.0 && s.cls == kVbBinary && s.floor_bytes == 1ull << 60 && s.top_byte == 'x');
    }
    // the identities, each broken once
    {
        std::vector<uint64_t> vec(value_bytes_len(P), 0), payload(payload_len(P), 0), counters(7 * P + 8, 0);
        add(vec, 1, "aab"), add(vec, 1, "{}"), value_bytes_add(vec.data(), 1, -1, nullptr);
        uint64_t *l = payload.data() + kPlPartitionWords;
        l[kPlRecords] = 3, l[kPlClass + kPlNull] = 1, l[kPlClass + kPlJson] = 1, l[kPlClass + kPlOther] = 1, l[kPlClassBytes + kPlJson] = 2;
        l[kPlClassBytes + kPlOther] = 3;
        counters[7] = 3;
        CHECK(value_bytes_identities_hold(vec.data(), P, payload.data(), counters.data(), 7));
        uint64_t *w = vec.data() + kVbPartitionWords;
        CHECK(w[kVbRepeats] == 1);
        struct { uint64_t *word; uint64_t by; } breaks[] = {{&w['a'], 1}, {&w[kVbBytes], 1}, {&w[kVbRepeats], 3}, {&w[kVbValues], 2}, {&w[260], 1}, {&w[263], 1}};
        for (auto &b : breaks) {
            *b.word += b.by;
            CHECK(!value_bytes_identities_hold(vec.data(), P));
            *b.word -= b.by;
        }
        CHECK(value_bytes_identities_hold(vec.data(), P));
        uint64_t *with_payload[] = {&l[kPlRecords], &l[kPlClassBytes + kPlFramed], &l[kPlClass + kPlFramed]};
        for (uint64_t *word : with_payload) {
            *word += 1;
            CHECK(value_bytes_identities_hold(vec.data(), P) && !value_bytes_identities_hold(vec.data(), P, payload.data()));
            *word -= 1;
        }
        counters[7] = 4;
        CHECK(!value_bytes_identities_hold(vec.data(), P, payload.data(), counters.data(), 7) && value_bytes_identities_hold(vec.data(), P, payload.data()));
    }
    // the host walk: a value whose first byte equals the byte in front of it is no repeat; a record with bad framing ends the batch
    {
        const uint8_t recs[] = {// record 0: length 9; attributes, tsDelta, offsetDelta, key -1, value length 3: 06 06 07, no headers
                                18, 0, 0, 0, 1, 6, 6, 6, 7, 0,
                                // record 1: length 8; key "\0" (length 1), a value of length 1: 00, no headers
                                16, 0, 0, 2, 2, 0, 2, 0, 0,
                                // record 2: length 7; a value length that overruns the record
                                14, 0, 0, 4, 1, 40, 1, 0};
        std::vector<uint64_t> vec(value_bytes_len(2), 0);
        value_bytes_batch_host(vec.data(), 1, recs, 0, sizeof recs, 3, [](long long) { return true; });
        const uint64_t *w = vec.data() + kVbPartitionWords;
        CHECK(w[kVbRecords] == 2 && w[kVbValues] == 2 && w[kVbBytes] == 4 && w[kVbRepeats] == 1 && w[6] == 2 && w[7] == 1 && w[0] == 1);
        CHECK(value_bytes_identities_hold(vec.data(), 2));
    }
    if (failures) return 1;
    printf("OK\n");
    return 0;
}

// compaction_check.cpp — csrc/kta_compaction.h on the CPU, as a program of its own (built with
// -fsanitize=address,undefined by tests/test_compaction_host.py and run directly): every class of the rule at its boundary
// values — the slot's entry 0, v - 1, v, v + 1 and the alive bit alone differing; key_len -1 / 0; val_len -1 / 0; partition
// -1 / 0 / P - 1 / P — against the definition said again, the vector's layout and the packing of the LDS word W0.  Prints
// "OK <checks>" and returns 0, or says what failed and returns 1.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "kta_compaction.h"

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

// the definition of include/kta_hip.h, said again with nothing shared but the enumerators
kta::CompactionClass by_definition(uint64_t entry, uint64_t s, int32_t key_len, int32_t val_len, int32_t partition, uint32_t P)
{
    if (key_len < 0) return kta::kCompactionUnkeyed;
    const uint64_t v = (s + 1) * 2 + (val_len >= 0 ? 1 : 0);
    if (entry != v) return entry > v ? kta::kCompactionSuperseded : kta::kCompactionUnknown;
    const bool inside = partition >= 0 && (int64_t)partition < (int64_t)P;
    if (val_len >= 0) return inside ? kta::kCompactionLive : kta::kCompactionLiveOutside;
    return inside ? kta::kCompactionTombstone : kta::kCompactionTombstoneOutside;
}

} // namespace

int main()
{
    long seen[kta::kCompactionClasses] = {};
    for (uint32_t P : {1u, 6u, 4096u}) {
        for (uint64_t s : {0ull, 1ull, 7ull, (1ull << 40) + 3, (1ull << 62) - 2}) {
            for (int32_t val_len : {-1, 0, 1, INT32_MAX}) {
                const uint64_t v = kta::compaction_value(s, val_len);
                CHECK(v == (((s + 1) << 1) | (val_len >= 0 ? 1u : 0u)), "value of s=%llu", (unsigned long long)s);
                // 0, v - 1, v, v + 1, the alive bit alone differing (v ^ 1), far below and far above
                const std::vector<uint64_t> entries = {0, v - 1, v, v + 1, v ^ 1, 1, v / 2, v + 1000, UINT64_MAX};
                for (uint64_t entry : entries)
                    for (int32_t key_len : {-1, 0, 1, 300})
                        for (int32_t partition : {-1, 0, (int32_t)P - 1, (int32_t)P, (int32_t)P + 3, INT32_MIN, INT32_MAX}) {
                            const kta::CompactionClass got = kta::compaction_classify(entry, s, key_len, val_len, partition, P);
                            const kta::CompactionClass want = by_definition(entry, s, key_len, val_len, partition, P);
                            CHECK(got == want, "entry=%llu s=%llu kl=%d vl=%d p=%d P=%u: %u, not %u", (unsigned long long)entry,
                                  (unsigned long long)s, key_len, val_len, partition, P, (unsigned)got, (unsigned)want);
                            seen[got]++;
                        }
            }
        }
    }
    for (uint32_t k = 0; k < kta::kCompactionClasses; k++) CHECK(seen[k] > 0, "class %u never met", k);

    // the cases of the table in the header, one by one (P = 6, s = 9: v = 21 live, 20 tombstone)
    CHECK(kta::compaction_classify(21, 9, -1, 5, 0, 6) == kta::kCompactionUnkeyed, "key None");
    CHECK(kta::compaction_classify(21, 9, 0, 5, 0, 6) == kta::kCompactionLive, "the empty key is a key");
    CHECK(kta::compaction_classify(21, 9, 3, 0, 5, 6) == kta::kCompactionLive, "the empty value is a value");
    CHECK(kta::compaction_classify(20, 9, 3, -1, 5, 6) == kta::kCompactionTombstone, "a tombstone kept");
    CHECK(kta::compaction_classify(21, 9, 3, -1, 5, 6) == kta::kCompactionSuperseded, "the alive bit alone: the entry is newer");
    CHECK(kta::compaction_classify(20, 9, 3, 5, 5, 6) == kta::kCompactionUnknown, "the alive bit alone: the entry is older");
    CHECK(kta::compaction_classify(0, 9, 3, 5, 5, 6) == kta::kCompactionUnknown, "never written");
    CHECK(kta::compaction_classify(0, 0, 3, -1, 5, 6) == kta::kCompactionUnknown, "never written, the first tombstone (v = 2)");
    CHECK(kta::compaction_classify(22, 9, 3, 5, 5, 6) == kta::kCompactionSuperseded, "v + 1");
    CHECK(kta::compaction_classify(21, 9, 3, 5, 6, 6) == kta::kCompactionLiveOutside, "partition P");
    CHECK(kta::compaction_classify(21, 9, 3, 5, -1, 6) == kta::kCompactionLiveOutside, "partition -1");
    CHECK(kta::compaction_classify(20, 9, 3, -1, 6, 6) == kta::kCompactionTombstoneOutside, "a tombstone at partition P");

    // the layout and the LDS word
    CHECK(kta::compaction_len(6) == 36 && kta::compaction_len(4096) == 5 * 4096 + 6, "vector length");
    CHECK(kta::kCompactionWords == 5 && kta::kCompactionGlobals == 6 && kta::kCompactionLdsWords * 8 == 32, "32 B per partition in LDS");
    uint64_t w0 = 0;
    for (uint64_t i = 0; i < 1000; i++) w0 += kta::compaction_w0(true);
    for (uint64_t i = 0; i < 77; i++) w0 += kta::compaction_w0(false);
    CHECK(kta::compaction_w0_live(w0) == 1000 && kta::compaction_w0_tombstones(w0) == 77, "W0 halves");
    w0 = kta::kCompactionLaunchMax * kta::compaction_w0(true) + kta::kCompactionLaunchMax * kta::compaction_w0(false);
    CHECK(kta::compaction_w0_live(w0) == kta::kCompactionLaunchMax && kta::compaction_w0_tombstones(w0) == kta::kCompactionLaunchMax,
          "a launch's most records fit either half");

    if (g_failed) {
        fprintf(stderr, "%d of %ld checks failed\n", g_failed, g_checks);
        return 1;
    }
    printf("OK %ld\n", g_checks);
    return 0;
}

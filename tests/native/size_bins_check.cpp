// size_bins_check.cpp — csrc/kta_size_bins.h on the CPU, as a program of its own (built with -fsanitize=address,undefined by
// tests/test_size_quantiles_host.py and run directly): the bin of every bin's bounds and of both sides of every place where
// the rule changes against the definition said again, the bounds' own properties, the vector's layout, the read-off
// against a sorted array's nearest rank and the identities.  Prints "OK <checks>" and returns 0, or says what failed and
// returns 1.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "kta_size_bins.h"

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

// the definition of include/kta_hip.h, said again with a loop instead of a count of leading zeros
uint32_t by_definition(uint64_t v)
{
    if (v < 32) return (uint32_t)v;
    uint32_t e = 0;
    while ((v >> (e + 1)) != 0) e++;
    return 32 + 16 * (e - 5) + (uint32_t)((v >> (e - 4)) & 15);
}

uint64_t sorted_rank(std::vector<uint32_t> s, uint64_t num, uint64_t den)
{
    std::sort(s.begin(), s.end());
    uint64_t r = (num * s.size() + den - 1) / den;
    if (r < 1) r = 1;
    return s[r - 1];
}

} // namespace

int main()
{
    CHECK(kta::kSizeBins == 464 && kta::kSizeQuantities == 3 && kta::kSizeGlobals == 8, "the constants");
    // every bin: its bounds fall into it, its neighbours' do not, the bins tile [0, 2^32)
    for (uint32_t b = 0; b < kta::kSizeBins; b++) {
        const uint64_t lo = kta::size_bin_lo(b), hi = kta::size_bin_hi(b);
        CHECK(lo <= hi && hi <= 0xFFFFFFFFull, "bin %u: [%llu, %llu]", b, (unsigned long long)lo, (unsigned long long)hi);
        CHECK(kta::size_bin((uint32_t)lo) == b && kta::size_bin((uint32_t)hi) == b, "bin %u holds its bounds", b);
        CHECK(by_definition(lo) == b && by_definition(hi) == b, "bin %u by definition", b);
        CHECK(hi + 1 == kta::size_bin_lo(b + 1), "bin %u: hi + 1 is the next lo", b);
        if (b >= 32) CHECK(hi * 16 <= lo * 17, "bin %u is at most 1/16 of its lower bound wide", b);
        else CHECK(lo == b && hi == b, "bin %u is exact", b);
        if (b > 0) CHECK(kta::size_bin((uint32_t)(lo - 1)) == b - 1, "below bin %u", b);
    }
    CHECK(kta::size_bin_lo(0) == 0 && kta::size_bin_hi(463) == 0xFFFFFFFFull && kta::size_bin_lo(464) == (1ull << 32), "the ends");
    // both sides of every place where the rule changes
    for (uint64_t v : {0ull, 1ull, 31ull, 32ull, 33ull, 63ull, 64ull, 65534ull, 65535ull, 65536ull, (1ull << 31) - 1, 1ull << 31, (1ull << 32) - 1})
        CHECK(kta::size_bin((uint32_t)v) == by_definition(v), "size %llu: bin %u, not %u", (unsigned long long)v, kta::size_bin((uint32_t)v), by_definition(v));
    CHECK(kta::size_bin(31) == 31 && kta::size_bin(32) == 32 && kta::size_bin(63) == 47 && kta::size_bin(64) == 48 && kta::size_bin(0xFFFFFFFFu) == 463,
          "the bins the header names");
    // a sweep with a stride that meets every octave
    for (uint64_t v = 0; v < (1ull << 32); v += 65521) CHECK(kta::size_bin((uint32_t)v) == by_definition(v), "size %llu", (unsigned long long)v);
    // the message size
    CHECK(kta::size_message(-1, 5) == 5 && kta::size_message(0, 5) == 5 && kta::size_message(7, 5) == 12, "max(key_len, 0) + val_len");
    CHECK(kta::size_message(INT32_MAX, INT32_MAX) == 0xFFFFFFFEu, "the largest message fits u32");
    // the layout
    CHECK(kta::size_quantiles_len(1) == 1400 && kta::size_quantiles_len(256) == 256u * 1392u + 8u, "vector length");
    CHECK(kta::size_quantiles_word(0, 0, 0) == 0 && kta::size_quantiles_word(2, 1, 7) == (2 * 3 + 1) * 464 + 7, "word index");

    // the read-off against a sorted array, for N = 1, 2, 1000, 1001 and the empty histogram
    uint32_t bin = 77;
    std::vector<uint64_t> hist(kta::kSizeBins, 0);
    CHECK(!kta::size_quantile(hist.data(), 50, 100, &bin) && bin == 77, "the empty histogram has no answer");
    uint64_t x = 88172645463325252ull;
    for (size_t n : {1u, 2u, 1000u, 1001u}) {
        std::vector<uint32_t> sizes(n);
        std::fill(hist.begin(), hist.end(), 0);
        for (size_t i = 0; i < n; i++) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            sizes[i] = (uint32_t)(x >> 32) >> (x % 32);      // every magnitude
            hist[kta::size_bin(sizes[i])]++;
        }
        const uint64_t q[6][2] = {{50, 100}, {90, 100}, {99, 100}, {999, 1000}, {0, 100}, {100, 100}};
        for (const auto &nd : q) {
            CHECK(kta::size_quantile(hist.data(), nd[0], nd[1], &bin), "N = %zu has an answer", n);
            const uint64_t want = sorted_rank(sizes, nd[0], nd[1]);
            CHECK(kta::size_bin_lo(bin) <= want && want <= kta::size_bin_hi(bin), "N = %zu, %llu/%llu: bin %u does not hold %llu", n,
                  (unsigned long long)nd[0], (unsigned long long)nd[1], bin, (unsigned long long)want);
        }
    }
    // counts near 2^64: the product takes 128 bits
    std::fill(hist.begin(), hist.end(), 0);
    hist[3] = 1ull << 63, hist[400] = (1ull << 63) - 1;
    CHECK(kta::size_quantile(hist.data(), 50, 100, &bin) && bin == 3, "half of 2^64 - 1 records");
    CHECK(kta::size_quantile(hist.data(), 999, 1000, &bin) && bin == 400, "p99.9 of 2^64 - 1 records");

    // the identities: a vector made from records matches their counters, and no longer after one more record
    const uint32_t P = 3, NC = 7;
    std::vector<uint64_t> vec(kta::size_quantiles_len(P), 0), cnt((size_t)P * NC + 8, 0);
    auto add = [&](uint32_t p, int32_t kl, int32_t vl) {
        uint64_t *g = vec.data() + (size_t)P * kta::kSizePartitionWords;
        g[kta::kSizeGlobalRecords]++, cnt[(size_t)P * NC + 2]++;
        if (kl >= 0) vec[kta::size_quantiles_word(p, kta::kSizeKey, kta::size_bin((uint32_t)kl))]++, cnt[(size_t)p * NC + 4]++, g[kta::kSizeGlobalKeyed]++;
        if (vl >= 0) {
            vec[kta::size_quantiles_word(p, kta::kSizeValue, kta::size_bin((uint32_t)vl))]++;
            vec[kta::size_quantiles_word(p, kta::kSizeMessage, kta::size_bin(kta::size_message(kl, vl)))]++;
            cnt[(size_t)p * NC + 2]++, g[kta::kSizeGlobalAlive]++;
        }
    };
    add(0, -1, 5), add(0, 3, -1), add(2, 70000, 65535), add(2, 0, 0), add(2, -1, -1);
    CHECK(kta::size_quantiles_match(vec.data(), cnt.data(), P, NC, 4, 2, 2, 0), "a vector and its counters");
    vec[kta::size_quantiles_word(1, kta::kSizeKey, 9)]++;
    CHECK(!kta::size_quantiles_match(vec.data(), cnt.data(), P, NC, 4, 2, 2, 0), "a key too many");
    vec[kta::size_quantiles_word(1, kta::kSizeKey, 9)]--;
    cnt[(size_t)P * NC + 0]++;
    CHECK(!kta::size_quantiles_match(vec.data(), cnt.data(), P, NC, 4, 2, 2, 0), "a bad-partition record the vector did not see");

    if (g_failed) {
        fprintf(stderr, "%d of %ld checks failed\n", g_failed, g_checks);
        return 1;
    }
    printf("OK %ld\n", g_checks);
    return 0;
}

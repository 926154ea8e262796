// kta_size_bins.h — the size percentiles (KTA_FLAG_SIZE_QUANTILES, include/kta_hip.h): the one statement of the bin a size
// falls into, a bin's bounds, the layout of the result vector, the nearest-rank read-off and the identities that tie the
// vector to the counter vector.  Shared by the kernel (kta_size_quantiles.hip), the host code that reads the vector and the
// stand-alone check (tests/native/size_bins_check.cpp): plain C++, no HIP header.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KTA_SIZE_BINS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define KTA_SIZE_BINS_HD inline
#endif

namespace kta {

constexpr uint32_t kSizeBins = 464;             // KTA_SIZE_BINS: 32 exact bins, then 16 per octave for the octaves 5 .. 31
constexpr uint32_t kSizeExact = 32;             // sizes below this have a bin of their own
constexpr uint32_t kSizeQuantities = 3;         // K key_len, V val_len, M max(key_len, 0) + val_len
constexpr uint32_t kSizeGlobals = 8;
enum : uint32_t { kSizeKey = 0, kSizeValue = 1, kSizeMessage = 2 };
enum : uint32_t { kSizeGlobalRecords = 0, kSizeGlobalBadPartition = 1, kSizeGlobalKeyed = 2, kSizeGlobalAlive = 3 };
constexpr uint32_t kSizePartitionWords = kSizeQuantities * kSizeBins;   // 1392 words of a partition

// THE RULE.  v < 32: the bin is v.  Otherwise e = floor(log2 v) and the bin is 32 + 16 (e - 5) + the four bits below v's
// leading one: a bin is at most 1/16 of its lower bound wide.
KTA_SIZE_BINS_HD uint32_t size_bin(uint32_t v)
{
    if (v < kSizeExact) return v;
    const uint32_t e = 31u - (uint32_t)__builtin_clz(v);
    return kSizeExact + 16u * (e - 5u) + ((v >> (e - 4u)) & 15u);
}
// The least size of bin b, b <= 464 (lo(464) = 2^32: one past the largest size).
KTA_SIZE_BINS_HD uint64_t size_bin_lo(uint32_t b)
{
    if (b < kSizeExact) return b;
    return (uint64_t)(16u + (b - kSizeExact) % 16u) << ((b - kSizeExact) / 16u + 1u);
}
// The largest size of bin b, b < 464: hi(463) = 2^32 - 1.
KTA_SIZE_BINS_HD uint64_t size_bin_hi(uint32_t b) { return size_bin_lo(b + 1u) - 1u; }

// The result vector u64[P * 3 * 464 + 8]: word (p * 3 + q) * 464 + b of partition p, quantity q, bin b, then the globals.
KTA_SIZE_BINS_HD size_t size_quantiles_len(uint32_t P) { return (size_t)P * kSizePartitionWords + kSizeGlobals; }
KTA_SIZE_BINS_HD size_t size_quantiles_word(uint32_t p, uint32_t q, uint32_t b) { return ((size_t)p * kSizeQuantities + q) * kSizeBins + b; }

// A record's message size, for val_len >= 0: the reference's message_size of a non-tombstone (metric.rs:212-251).
KTA_SIZE_BINS_HD uint32_t size_message(int32_t key_len, int32_t val_len) { return (uint32_t)(key_len > 0 ? key_len : 0) + (uint32_t)val_len; }

// THE READ-OFF.  Nearest rank: r = max(1, ceil(num N / den)), N the histogram's count, the product in 128 bits; the answer
// is the first bin whose running count reaches r.  false: N == 0, there is no answer.  num <= den, den > 0.
inline bool size_quantile(const uint64_t *hist, uint64_t num, uint64_t den, uint32_t *bin)
{
    unsigned __int128 N = 0;
    for (uint32_t b = 0; b < kSizeBins; b++) N += hist[b];
    if (N == 0) return false;
    unsigned __int128 r = ((unsigned __int128)num * N + den - 1) / den;
    if (r < 1) r = 1;
    unsigned __int128 run = 0;
    for (uint32_t b = 0; b < kSizeBins; b++) {
        run += hist[b];
        if (run >= r) {
            *bin = b;
            return true;
        }
    }
    *bin = kSizeBins - 1;   // (never: r <= N)
    return true;
}

// THE IDENTITIES between a size vector and the counter vector u64[P * 7 + 8] of the same records (kta_hip.h): per
// partition the K bins sum to key_non_null and the V bins and the M bins to alive; global 1 is the records counted and
// global 2 the records outside [0, P).  c_key_non_null, c_alive: the counter's index among a partition's `ncounters` words;
// g_records, g_bad: the global's index behind them.
inline bool size_quantiles_match(const uint64_t *vec, const uint64_t *counters, uint32_t P, uint32_t ncounters, uint32_t c_key_non_null,
                                 uint32_t c_alive, uint32_t g_records, uint32_t g_bad)
{
    for (uint32_t p = 0; p < P; p++) {
        uint64_t s[kSizeQuantities] = {0, 0, 0};
        for (uint32_t q = 0; q < kSizeQuantities; q++)
            for (uint32_t b = 0; b < kSizeBins; b++) s[q] += vec[size_quantiles_word(p, q, b)];
        const uint64_t *c = counters + (size_t)p * ncounters;
        if (s[kSizeKey] != c[c_key_non_null] || s[kSizeValue] != c[c_alive] || s[kSizeMessage] != c[c_alive]) return false;
    }
    const uint64_t *g = vec + (size_t)P * kSizePartitionWords, *cg = counters + (size_t)P * ncounters;
    return g[kSizeGlobalRecords] == cg[g_records] && g[kSizeGlobalBadPartition] == cg[g_bad];
}

} // namespace kta

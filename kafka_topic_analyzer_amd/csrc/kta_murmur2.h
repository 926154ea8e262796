// kta_murmur2.h — Kafka's murmur2 (org.apache.kafka.common.utils.Utils.murmur2: seed 0x9747b28c, m = 0x5bd1e995, r = 24,
// little-endian 4-byte words, the 1..3 tail bytes xored in and multiplied once) and the exact remainder by a run-time
// divisor that the partitioner pass (kta_partitioner.hip, KTA_FLAG_PARTITIONER) puts behind it.  One source for the
// device, for the library's host helper kta_murmur2 and for the native test (tests/native/murmur2_check.cpp): plain
// C++, no intrinsic.  The words of a key are little-endian loads at any address; gfx950 runs in unaligned access mode.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define KTA_MM2_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define KTA_MM2_HD inline
#endif

namespace kta {

constexpr uint32_t kMurmur2Seed = 0x9747b28cu;
constexpr uint32_t kMurmur2M = 0x5bd1e995u;

// one 4-byte word into h
KTA_MM2_HD uint32_t murmur2_word(uint32_t h, uint32_t k)
{
    k *= kMurmur2M;
    k ^= k >> 24;
    k *= kMurmur2M;
    return (h * kMurmur2M) ^ k;
}

// the last len & 3 bytes (the low bytes of w; its other bytes are anything), then the final mix
KTA_MM2_HD uint32_t murmur2_finish(uint32_t h, uint32_t w, uint32_t len)
{
    const uint32_t t = len & 3u;
    if (t) h = (h ^ (w & (0xFFFFFFFFu >> (32u - 8u * t)))) * kMurmur2M;
    h ^= h >> 13;
    h *= kMurmur2M;
    return h ^ (h >> 15);
}

KTA_MM2_HD uint32_t murmur2_load32(const uint8_t *p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

// murmur2 of a 16-byte key
KTA_MM2_HD uint32_t murmur2_16(const uint32_t (&w)[4])
{
    uint32_t h = kMurmur2Seed ^ 16u;
#pragma unroll
    for (int d = 0; d < 4; d++) h = murmur2_word(h, w[d]);
    return murmur2_finish(h, 0u, 16u);
}

// Four 16-byte keys at once, their chains interleaved word by word.
KTA_MM2_HD void murmur2_16x4(uint32_t (&h)[4], const uint32_t (&w)[4][4])
{
#pragma unroll
    for (int j = 0; j < 4; j++) h[j] = kMurmur2Seed ^ 16u;
#pragma unroll
    for (int d = 0; d < 4; d++) {
#pragma unroll
        for (int j = 0; j < 4; j++) h[j] = murmur2_word(h[j], w[j][d]);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) h[j] = murmur2_finish(h[j], 0u, 16u);
}

// murmur2 of the len bytes at key, whose first 16 bytes (w0..w3: whatever lies there when the key is shorter) were loaded
// before.  Reads key[16 .. len) in 4-byte words, and for a key longer than 16 bytes with a tail ONE word that begins
// inside the key and ends at most 3 bytes past it: inside the 16 bytes that key_bytes is readable past its last key.
KTA_MM2_HD uint32_t murmur2_prefetched(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, const uint8_t *key, uint32_t len)
{
    uint32_t h = kMurmur2Seed ^ len;
    const uint32_t words = len >> 2;
    if (words > 0u) h = murmur2_word(h, w0);
    if (words > 1u) h = murmur2_word(h, w1);
    if (words > 2u) h = murmur2_word(h, w2);
    if (words > 3u) h = murmur2_word(h, w3);
    if (words < 4u) return murmur2_finish(h, words == 0u ? w0 : (words == 1u ? w1 : (words == 2u ? w2 : w3)), len);
    const uint8_t *k = key + 16;
    uint32_t left = words - 4u;
    while (left >= 4u) {
        struct {
            uint32_t a, b, c, d;
        } v;
        memcpy(&v, k, 16);
        h = murmur2_word(murmur2_word(murmur2_word(murmur2_word(h, v.a), v.b), v.c), v.d);
        k += 16;
        left -= 4u;
    }
    while (left) {
        h = murmur2_word(h, murmur2_load32(k));
        k += 4;
        left--;
    }
    return murmur2_finish(h, (len & 3u) ? murmur2_load32(k) : 0u, len);
}

// t mod d for 0 <= t < 2^31 and 1 <= d <= 2^16, exact, without a division per record: with L = ceil(log2 d) and
// mul = ceil(2^(31 + L) / d) (below 2^32 for these d) floor(t / d) = (t * mul) >> (31 + L) for every t < 2^31, because
// 2^(31+L) <= mul d <= 2^(31+L) + 2^L (Granlund & Montgomery 1994, theorem 4.2).  d = 1 has L = 0 and is told apart.
struct ModU31 {
    uint32_t d, mul, shift;   // shift = L - 1 behind the high half of the product
};

inline ModU31 mod_u31_make(uint32_t d)
{
    uint32_t L = 0;
    while ((1u << L) < d) L++;
    const uint64_t two = 1ull << (31 + L);
    return ModU31{d, (uint32_t)((two + d - 1) / d), L ? L - 1u : 0u};
}

KTA_MM2_HD uint32_t mod_u31(uint32_t t, const ModU31 &m)
{
    const uint32_t q = (uint32_t)(((uint64_t)t * m.mul) >> 32) >> m.shift;
    return m.d == 1u ? 0u : t - q * m.d;
}

} // namespace kta

// murmur2_check.cpp — the partitioner pass's hash and remainder (csrc/kta_murmur2.h, the source the kernel compiles) run
// natively under AddressSanitizer + UBSan.
//   1. murmur2_prefetched, the entry the kernel calls, for every key length 0..80 at each of the four byte alignments:
//      the key sits at the END of a heap block of exactly offset + len + 16 bytes — the 16 bytes that key_bytes is
//      readable past its last key and not one more —, so a read beyond the contract aborts here.  The first 16 bytes are
//      loaded as the kernel's unconditional prefetch loads them.  Compared with a byte-wise murmur2 written here.
//   2. murmur2_16 and murmur2_16x4 against the same.
//   3. Kafka's known answers.
//   4. mod_u31 against % for every divisor 1..4096 (and some up to 65536) over the 31-bit values where a reciprocal can
//      go wrong: around every multiple boundary near 0 and near 2^31, and a pseudo-random sample.
// Prints "OK <checks>" and exits 0; the first mismatch prints what differed and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kta_murmur2.h"

static uint32_t murmur2_bytes(const uint8_t *d, uint32_t n)
{
    const uint32_t m = 0x5bd1e995u;
    uint32_t h = 0x9747b28cu ^ n;
    for (uint32_t i = 0; i + 4 <= n; i += 4) {
        uint32_t k = (uint32_t)d[i] | (uint32_t)d[i + 1] << 8 | (uint32_t)d[i + 2] << 16 | (uint32_t)d[i + 3] << 24;
        k *= m;
        k ^= k >> 24;
        k *= m;
        h *= m;
        h ^= k;
    }
    const uint32_t i = n & ~3u;
    switch (n & 3u) {
    case 3: h ^= (uint32_t)d[i + 2] << 16;   // fall through
    case 2: h ^= (uint32_t)d[i + 1] << 8;    // fall through
    case 1: h ^= d[i]; h *= m;
    }
    h ^= h >> 13;
    h *= m;
    h ^= h >> 15;
    return h;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

static uint32_t prefetched_at_block_end(const uint8_t *key_src, uint32_t len, uint32_t offset)
{
    const size_t size = (size_t)offset + len + 16;
    uint8_t *block = (uint8_t *)malloc(size);
    memset(block, 0xA5, size);
    uint8_t *key = block + offset;
    memcpy(key, key_src, len);
    uint32_t w[4];
    memcpy(w, key, 16);                      // the kernel's unconditional 16-byte prefetch
    const uint32_t h = kta::murmur2_prefetched(w[0], w[1], w[2], w[3], key, len);
    free(block);
    return h;
}

int main()
{
    unsigned long checks = 0;
    uint8_t src[96];
    for (uint32_t len = 0; len <= 80; len++)
        for (uint32_t offset = 0; offset < 4; offset++)
            for (int round = 0; round < 4; round++) {
                for (uint32_t i = 0; i < sizeof src; i++) src[i] = (uint8_t)(round == 0 ? 0xFF : rnd());
                const uint32_t got = prefetched_at_block_end(src, len, offset), want = murmur2_bytes(src, len);
                if (got != want) {
                    printf("murmur2_prefetched: len %u offset %u: %08x, byte-wise %08x\n", len, offset, got, want);
                    return 1;
                }
                checks++;
            }
    for (int round = 0; round < 100; round++) {
        uint32_t w[4][4], h4[4];
        for (auto &k : w)
            for (uint32_t &x : k) x = rnd();
        kta::murmur2_16x4(h4, w);
        for (int j = 0; j < 4; j++) {
            uint8_t b[16];
            memcpy(b, w[j], 16);
            const uint32_t want = murmur2_bytes(b, 16);
            if (h4[j] != want || kta::murmur2_16(w[j]) != want) {
                printf("murmur2_16x4 / murmur2_16: key %d: %08x / %08x, byte-wise %08x\n", j, h4[j], kta::murmur2_16(w[j]), want);
                return 1;
            }
            checks++;
        }
    }
    static const struct {
        const char *key;
        int32_t hash;
    } known[] = {{"21", -973932308}, {"foobar", -790332482}, {"a-little-bit-long-string", -985981536},
                 {"a-little-bit-longer-string", -1486304829}, {"lkjh234lh9fiuh90y23oiuhsafujhadof229phr9h19h89h8", -58897971},
                 {"abc", 479470107}, {"", 275646681}};
    for (const auto &k : known) {
        const uint32_t len = (uint32_t)strlen(k.key);
        for (uint32_t offset = 0; offset < 4; offset++) {
            const uint32_t got = prefetched_at_block_end((const uint8_t *)k.key, len, offset);
            if (got != (uint32_t)k.hash || murmur2_bytes((const uint8_t *)k.key, len) != (uint32_t)k.hash) {
                printf("known answer \"%s\": %08x, expected %08x\n", k.key, got, (uint32_t)k.hash);
                return 1;
            }
            checks++;
        }
    }
    const uint32_t top = 0x7fffffffu;
    for (uint32_t d = 1; d <= 65536; d = d < 4096 ? d + 1 : d + 977) {
        const kta::ModU31 m = kta::mod_u31_make(d);
        auto check = [&](uint32_t t) {
            if (kta::mod_u31(t, m) == t % d) return true;
            printf("mod_u31: %u mod %u = %u, got %u\n", t, d, t % d, kta::mod_u31(t, m));
            return false;
        };
        for (uint32_t k = 0; k < 3; k++)
            for (int e = -2; e <= 2; e++) {
                const int64_t lo = (int64_t)k * d + e, hi = (int64_t)(top / d - k) * d + e;
                if (lo >= 0 && lo <= top && !check((uint32_t)lo)) return 1;
                if (hi >= 0 && hi <= top && !check((uint32_t)hi)) return 1;
                checks += 2;
            }
        if (!check(top) || !check(top - 1) || !check(1u << 30) || !check((1u << 30) - 1)) return 1;
        for (int s = 0; s < 64; s++)
            if (!check(rnd() & top)) return 1;
        checks += 68;
    }
    printf("OK %lu\n", checks);
    return 0;
}

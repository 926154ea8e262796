// tile_size_check.cpp — csrc/kta_tile.h's size extrema on the CPU, a program of its own (tests/test_tile_size_host.py
// builds it with AddressSanitizer + UBSan and runs it): tile_plane_host writes the least and the largest key + value size
// of the tile's valued records exactly when it marks the tile, a None key counts as 0, a tile without a valued record
// gets 0xFFFFFFFF / 0, a tile that is not marked leaves the two words alone, and the plane it writes does not depend on
// whether the words are asked for.  The two words are a heap block of exactly their size.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "kta_tile.h"

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            failures++;                                    \
            fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                  \
            fprintf(stderr, "\n");                         \
        }                                                  \
    } while (0)

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint64_t rng()
{
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

constexpr uint64_t T = KTA_TILE_RECORDS;
constexpr uint32_t POISON = 0x5A5A5A5Au;

struct Tile {
    std::vector<int32_t> p, k, v;
    std::vector<int64_t> t;
    explicit Tile(uint64_t m) : p(m), k(m), v(m), t(m)
    {
        for (uint64_t j = 0; j < m; j++) {
            p[j] = (int32_t)(rng() % 256), k[j] = (int32_t)(rng() % 40) + 10, v[j] = (int32_t)(rng() % 900) + 100;
            t[j] = 1700000000000ll + (int64_t)j;
        }
    }
};

// -> the mark; lo / hi: the two words (POISON where tile_plane_host left them alone)
static uint32_t run(const char *what, const Tile &c, uint32_t &lo, uint32_t &hi)
{
    const uint64_t m = c.p.size();
    std::vector<int32_t> part(T), klen(T), vlen(T);
    std::vector<int64_t> ts(T, 0), ts_plain(T, 0);
    kta_tile_sum sum;
    const kta_tile_hdr h = kta::tile_pack_host(c.p.data(), c.t.data(), c.k.data(), c.v.data(), m, true, part.data(), ts.data(),
                                               klen.data(), vlen.data(), &sum);
    memcpy(ts_plain.data(), ts.data(), T * 8);
    std::vector<uint32_t> words(2, POISON);
    const uint32_t mark = kta::tile_plane_host(h, c.p.data(), c.k.data(), c.v.data(), m, ts.data(), words.data());
    const uint32_t mark_plain = kta::tile_plane_host(h, c.p.data(), c.k.data(), c.v.data(), m, ts_plain.data());
    CHECK(mark == mark_plain, "%s: the mark depends on whether the words are asked for", what);
    CHECK(memcmp(ts.data(), ts_plain.data(), T * 8) == 0, "%s: the plane depends on whether the words are asked for", what);
    lo = words[0], hi = words[1];
    if (!mark) CHECK(lo == POISON && hi == POISON, "%s: no mark, but the words were written", what);
    return mark;
}

// the two words as the metrics scan's rule gives them, record by record
static void by_hand(const Tile &c, uint32_t &lo, uint32_t &hi)
{
    lo = 0xFFFFFFFFu, hi = 0u;
    for (uint64_t j = 0; j < c.p.size(); j++) {
        if (c.v[j] == -1) continue;
        const uint32_t sz = (uint32_t)(c.k[j] == -1 ? 0 : c.k[j]) + (uint32_t)c.v[j];
        lo = sz < lo ? sz : lo, hi = sz > hi ? sz : hi;
    }
}

static void expect(const char *what, const Tile &c, uint32_t want_mark, uint32_t want_lo, uint32_t want_hi)
{
    uint32_t lo, hi;
    const uint32_t mark = run(what, c, lo, hi);
    CHECK(mark == want_mark, "%s: mark %u", what, mark);
    if (mark) CHECK(lo == want_lo && hi == want_hi, "%s: words %u / %u, expected %u / %u", what, lo, hi, want_lo, want_hi);
}

int main()
{
    CHECK(kta::kTileSideBytes == 36, "header 16, summary 8, mark 4, size extrema 8");
    kta_tile_hdr *base = nullptr;
    CHECK(reinterpret_cast<char *>(kta::tile_sizes_behind(base, 5)) - reinterpret_cast<char *>(base) == 5 * 28,
          "the size extrema lie behind the marks");
    CHECK(kta::kTileSizeMinNone == 0xFFFFFFFFu && kta::kTileSizeMaxNone == 0u, "the words of a tile without a valued record");
    // a record's share
    uint32_t lo = kta::kTileSizeMinNone, hi = kta::kTileSizeMaxNone;
    kta::tile_size_fold(7, -1, lo, hi);
    CHECK(lo == kta::kTileSizeMinNone && hi == kta::kTileSizeMaxNone, "a tombstone has no size, whatever its key");
    kta::tile_size_fold(-1, 30, lo, hi);
    CHECK(lo == 30 && hi == 30, "a None key counts as 0");
    kta::tile_size_fold(0, 0, lo, hi);
    kta::tile_size_fold(254, 65534, lo, hi);
    CHECK(lo == 0 && hi == 254 + 65534, "an empty record and the largest that fits");

    // whole tiles: sizes lie in [110, 1048] unless a case says otherwise
    for (int round = 0; round < 20; round++) {
        Tile c(T);
        for (uint64_t j = 0; j < T; j++) {
            if (rng() % 10 == 0) c.k[j] = -1;
            if (rng() % 10 == 0) c.v[j] = -1;
        }
        uint32_t want_lo, want_hi;
        by_hand(c, want_lo, want_hi);
        expect("random tile", c, 1u, want_lo, want_hi);
    }
    for (uint64_t at : {(uint64_t)0, (uint64_t)517, T - 1}) {
        uint32_t want_lo, want_hi;
        Tile c(T);
        c.k[at] = 0, c.v[at] = 0;
        c.k[(at + 5) % T] = 254, c.v[(at + 5) % T] = 65534;
        expect("extremes at the tile's ends", c, 1u, 0u, 254u + 65534u);
        Tile d(T);
        d.k[at] = -1, d.v[at] = 1;                         // smaller than every key alone
        by_hand(d, want_lo, want_hi);
        CHECK(want_lo == 1u, "the case's smallest size is the None key's value");
        expect("a None key with the smallest value", d, 1u, 1u, want_hi);
        Tile e(T);
        e.k[at] = 254, e.v[at] = -1;                       // the longest key, but no value: not a size
        by_hand(e, want_lo, want_hi);
        CHECK(want_hi <= 1048u, "the case's tombstone is not a size");
        expect("a tombstone with the longest key", e, 1u, want_lo, want_hi);
    }
    {
        Tile c(T);
        for (uint64_t j = 0; j < T; j++) c.v[j] = -1;
        expect("no valued record", c, 1u, 0xFFFFFFFFu, 0u);
        for (uint64_t j = 0; j < T; j++) c.k[j] = -1;
        expect("null-key tombstones only", c, 1u, 0xFFFFFFFFu, 0u);
        c.k[77] = 254, c.v[77] = 65534;
        expect("one valued record", c, 1u, 254u + 65534u, 254u + 65534u);
    }
    // tiles that are not marked leave the words alone (run checks it)
    {
        Tile c(T);
        c.k[9] = 255;
        expect("key 255", c, 0u, 0, 0);
        Tile d(T - 1);
        expect("partial tile", d, 0u, 0, 0);
        Tile e(T);
        e.t[1] = 0, e.t[5] = 1ll << 31;
        expect("raw tile", e, 0u, 0, 0);
    }
    if (failures) {
        fprintf(stderr, "tile_size_check: %d failure(s)\n", failures);
        return 1;
    }
    printf("tile_size_check OK\n");
    return 0;
}

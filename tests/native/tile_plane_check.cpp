// tile_plane_check.cpp — csrc/kta_tile.h's scan plane on the CPU, a program of its own (tests/test_tile_plane_host.py
// builds it with AddressSanitizer + UBSan and runs it): the fit rule at its edges, pack / unpack of every fitting triple
// it draws, the mark of a tile (one record that does not fit, a tile of fewer than KTA_TILE_RECORDS records, a tile
// that is not compact), and that tile_pack_host's images next to tile_plane_host's are byte for byte what tile_pack_host
// alone writes outside bytes [4096, 8192) of the ts image.  Inputs and images are heap blocks of exactly their size.
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

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng()
{
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

constexpr uint64_t T = KTA_TILE_RECORDS;
constexpr unsigned char POISON = 0x5A;

struct Images {
    std::vector<int32_t> part, klen, vlen;
    std::vector<int64_t> ts;
    Images() : part(T), klen(T), vlen(T), ts(T)
    {
        memset(part.data(), POISON, T * 4), memset(klen.data(), POISON, T * 4), memset(vlen.data(), POISON, T * 4);
        memset(ts.data(), POISON, T * 8);
    }
};

// A tile of m records that all fit, then `spoil` applied; -> the mark.  Checks the images against tile_pack_host alone.
template <class Spoil>
static uint32_t tile_case(const char *what, uint64_t m, bool lens16, Spoil spoil, bool expect_compact = true)
{
    std::vector<int32_t> p(m), k(m), v(m);
    std::vector<int64_t> t(m);
    for (uint64_t j = 0; j < m; j++) {
        p[j] = (int32_t)(rng() % 256), k[j] = (int32_t)(rng() % 256) - 1, v[j] = (int32_t)(rng() % 65536) - 1;
        t[j] = rng() % 50 == 0 ? -1 : 1700000000000ll + (int64_t)(rng() % 100000);
    }
    if (m) p[0] = 255, k[0] = 254, v[0] = 65534;               // the largest values that fit
    if (m > 1) p[1] = 0, k[1] = -1, v[1] = -1;                  // the markers
    if (m > 2) k[2] = 0, v[2] = 0;                              // empty key, empty value
    spoil(p, k, v, t);
    Images plain, with;
    const kta_tile_hdr hp = kta::tile_pack_host(p.data(), t.data(), k.data(), v.data(), m, lens16, plain.part.data(), plain.ts.data(),
                                                plain.klen.data(), plain.vlen.data());
    kta_tile_sum sum;
    const kta_tile_hdr hw = kta::tile_pack_host(p.data(), t.data(), k.data(), v.data(), m, lens16, with.part.data(), with.ts.data(),
                                                with.klen.data(), with.vlen.data(), &sum);
    const uint32_t mark = kta::tile_plane_host(hw, p.data(), k.data(), v.data(), m, with.ts.data());
    CHECK(memcmp(&hp, &hw, sizeof hp) == 0, "%s: the header changed", what);
    CHECK((hw.mode == KTA_TILE_COMPACT) == expect_compact, "%s: mode %u", what, hw.mode);
    CHECK(memcmp(plain.part.data(), with.part.data(), T * 4) == 0, "%s: partition image differs", what);
    CHECK(memcmp(plain.klen.data(), with.klen.data(), T * 4) == 0, "%s: key_len image differs", what);
    CHECK(memcmp(plain.vlen.data(), with.vlen.data(), T * 4) == 0, "%s: val_len image differs", what);
    const unsigned char *a = reinterpret_cast<const unsigned char *>(plain.ts.data()), *b = reinterpret_cast<const unsigned char *>(with.ts.data());
    CHECK(memcmp(a, b, kta::kTilePlaneOffset) == 0, "%s: ts image differs below the plane", what);
    if (hw.mode != KTA_TILE_COMPACT || !mark)
        CHECK(memcmp(a, b, T * 8) == 0, "%s: no plane, but the ts image was written", what);
    CHECK(mark <= 1u, "%s: mark %u", what, mark);
    if (mark) {
        CHECK(sum.flags & KTA_TILE_SUM_VALID, "%s: a mark without a VALID summary", what);
        for (uint64_t j = 0; j < m; j++) {
            uint32_t w;
            memcpy(&w, b + kta::tile_plane_at((uint32_t)j), 4);
            CHECK(w == kta::tile_plane_pack(p[j], k[j], v[j]), "%s: word %llu", what, (unsigned long long)j);
            CHECK(kta::tile_plane_part(w) == p[j] && kta::tile_plane_key(w) == k[j] && kta::tile_plane_val(w) == v[j],
                  "%s: record %llu does not unpack", what, (unsigned long long)j);
        }
    }
    return mark;
}

int main()
{
    // the fit rule at its edges
    const int32_t ps[] = {-1, 0, 255, 256}, ks[] = {-1, 0, 254, 255}, vs[] = {-1, 0, 65534, 65535};
    const bool pf[] = {false, true, true, false}, kf[] = {true, true, true, false}, vf[] = {true, true, true, false};
    for (int a = 0; a < 4; a++)
        for (int b = 0; b < 4; b++)
            for (int c = 0; c < 4; c++) {
                const bool want = pf[a] && kf[b] && vf[c];
                CHECK(kta::tile_plane_fits(ps[a], ks[b], vs[c]) == want, "fits(%d, %d, %d)", ps[a], ks[b], vs[c]);
                if (!want) continue;
                const uint32_t w = kta::tile_plane_pack(ps[a], ks[b], vs[c]);
                CHECK(kta::tile_plane_part(w) == ps[a] && kta::tile_plane_key(w) == ks[b] && kta::tile_plane_val(w) == vs[c],
                      "pack(%d, %d, %d) = %08x does not unpack", ps[a], ks[b], vs[c], w);
            }
    CHECK(!kta::tile_plane_fits(-2, 0, 0) && !kta::tile_plane_fits(0, -2, 0) && !kta::tile_plane_fits(0, 0, -2) &&
              !kta::tile_plane_fits(65535, 0, 0) && !kta::tile_plane_fits(0, 65535, 0) && !kta::tile_plane_fits(0, 0, INT32_MAX) &&
              !kta::tile_plane_fits(INT32_MIN, 0, 0),
          "values far outside fit");
    CHECK(kta::tile_plane_pack(255, -1, -1) == 0xFFFFFFFFu && kta::tile_plane_pack(0, 0, 0) == 0u, "the words of the corners");
    CHECK(kta::tile_plane_pack(0x12, 0x34, 0x5678) == 0x56783412u, "partition | key << 8 | val << 16");
    CHECK(kta::tile_plane_at(0) == 4096u && kta::tile_plane_at(1023) == 8188u, "word j is at byte 4096 + 4 j");
    // pack and unpack, exact for every fitting triple drawn
    for (int i = 0; i < 200000; i++) {
        const int32_t p = (int32_t)(rng() % 256), k = (int32_t)(rng() % 256) - 1, v = (int32_t)(rng() % 65536) - 1;
        CHECK(kta::tile_plane_fits(p, k, v), "drawn (%d, %d, %d) fits", p, k, v);
        const uint32_t w = kta::tile_plane_pack(p, k, v);
        CHECK(kta::tile_plane_part(w) == p && kta::tile_plane_key(w) == k && kta::tile_plane_val(w) == v, "(%d, %d, %d) -> %08x", p, k, v, w);
    }
    // whole tiles
    using V32 = std::vector<int32_t>;
    using V64 = std::vector<int64_t>;
    auto nothing = [](V32 &, V32 &, V32 &, V64 &) {};
    for (int lens16 = 0; lens16 < 2; lens16++) {
        CHECK(tile_case("all fit", T, lens16, nothing) == 1u, "a whole tile of fitting records is marked (lens16 %d)", lens16);
        for (uint64_t at : {(uint64_t)0, (uint64_t)517, T - 1}) {
            CHECK(tile_case("key 255", T, lens16, [&](V32 &, V32 &k, V32 &, V64 &) { k[at] = 255; }) == 0u, "key 255 at %llu", (unsigned long long)at);
            CHECK(tile_case("partition -1", T, lens16, [&](V32 &p, V32 &, V32 &, V64 &) { p[at] = -1; }) == 0u, "partition -1");
            CHECK(tile_case("partition 256", T, lens16, [&](V32 &p, V32 &, V32 &, V64 &) { p[at] = 256; }) == 0u, "partition 256");
            CHECK(tile_case("value 65535", T, lens16, [&](V32 &, V32 &, V32 &v, V64 &) { v[at] = 65535; }) == 0u, "value 65535");
            CHECK(tile_case("value 70000", T, lens16, [&](V32 &, V32 &, V32 &v, V64 &) { v[at] = 70000; }) == 0u, "value 70000");
        }
        CHECK(tile_case("raw tile", T, lens16, [](V32 &, V32 &, V32 &, V64 &t) { t[1] = 0, t[5] = 1ll << 31; }, false) == 0u, "a raw tile has no plane");
        for (uint64_t m : {(uint64_t)1, (uint64_t)4, T - 1})
            CHECK(tile_case("partial tile", m, lens16, nothing) == 0u, "a tile of %llu records is not marked", (unsigned long long)m);
    }
    if (failures) {
        fprintf(stderr, "tile_plane_check: %d failure(s)\n", failures);
        return 1;
    }
    printf("tile_plane_check OK\n");
    return 0;
}

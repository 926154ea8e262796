// filter_check.cpp — csrc/kta_filter.h on the CPU, as a program of its own (built with -fsanitize=address,undefined by
// tests/test_filter_host.py and run directly): the record predicate at its edges, the tile decision against brute force
// over the records of tiles packed by tile_pack_host, and the four-wave rank (filter_tile_rank, the scatter kernel's own
// text) as a compaction of single tiles of every count class against a sequential loop.  Prints "OK <checks>" and
// returns 0, or says what failed and returns 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "kta_filter.h"

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

uint64_t g_rng = 0x243F6A8885A308D3ull;
uint64_t rnd()
{
    g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
    return g_rng;
}

// the definition, said again with nothing shared but the types
bool passes_by_definition(const kta::FilterSpec &f, const std::vector<uint32_t> &bm, int32_t p, int64_t t)
{
    if (f.parts) {
        if (p < 0 || (uint32_t)p >= f.P) return false;
        if (!(bm[(size_t)p / 32] & (1u << (p % 32)))) return false;
    }
    const bool from = f.from_ms != INT64_MIN, to = f.to_ms != INT64_MAX;
    if (!from && !to) return true;
    if (t == -1) return false;
    if (from && t < f.from_ms) return false;
    if (to && t >= f.to_ms) return false;
    return true;
}

void check_predicate()
{
    const uint32_t P = 37;
    std::vector<uint32_t> bm(kta::filter_bitmap_words(P), 0u);
    for (uint32_t p : {0u, 3u, 31u, 32u, 36u}) bm[p / 32] |= 1u << (p % 32);
    const int64_t edges[] = {INT64_MIN, INT64_MIN + 1, -1000, -2, -1, 0, 1, 999, 1000, 1001, 4999, 5000, 5001, INT64_MAX - 1, INT64_MAX};
    const int64_t bounds[][2] = {{INT64_MIN, INT64_MAX}, {1000, 5000}, {INT64_MIN, 5000}, {1000, INT64_MAX}, {-1000, 0}, {-2, 1},
                                 {INT64_MIN + 1, INT64_MAX - 1}, {INT64_MAX - 1, INT64_MAX}, {INT64_MIN, INT64_MIN + 1}};
    const int32_t parts[] = {INT32_MIN, -2, -1, 0, 1, 3, 31, 32, 35, 36, 37, 38, 63, 64, 65535, INT32_MAX};
    for (auto &b : bounds)
        for (uint32_t with_set = 0; with_set < 2; with_set++) {
            const kta::FilterSpec f{b[0], b[1], P, with_set};
            for (int64_t t : edges)
                for (int32_t p : parts)
                    CHECK(kta::filter_record_passes(f, bm.data(), p, t) == passes_by_definition(f, bm, p, t),
                          "predicate: window [%lld, %lld) set %u partition %d ts %lld", (long long)b[0], (long long)b[1], with_set, p, (long long)t);
        }
    // said once more as literals: the bounds are inclusive below and exclusive above, on raw milliseconds
    const kta::FilterSpec w{1000, 5000, P, 0};
    CHECK(kta::filter_record_passes(w, nullptr, 2, 1000) && !kta::filter_record_passes(w, nullptr, 2, 999), "from is inclusive");
    CHECK(kta::filter_record_passes(w, nullptr, 2, 4999) && !kta::filter_record_passes(w, nullptr, 2, 5000), "to is exclusive");
    CHECK(!kta::filter_record_passes(w, nullptr, 2, -1), "-1 fails under a bound");
    CHECK(kta::filter_record_passes(w, nullptr, 99, 2000), "a bad partition passes without a set");
    const kta::FilterSpec s{INT64_MIN, INT64_MAX, P, 1};
    CHECK(kta::filter_record_passes(s, bm.data(), 3, -1) && !kta::filter_record_passes(s, bm.data(), 99, 5), "set only");
}

struct Tile {
    std::vector<int32_t> p, k, v;
    std::vector<int64_t> t;
};

// pack with the host packer, decide from header and summary, and hold the answer against every record
void check_tile(const Tile &tl, const kta::FilterSpec &f, const std::vector<uint32_t> &bm, const char *what, int want /* -1: any */)
{
    const uint64_t m = tl.p.size();
    std::vector<int32_t> part(KTA_TILE_RECORDS), klen(KTA_TILE_RECORDS), vlen(KTA_TILE_RECORDS);
    std::vector<int64_t> ts(KTA_TILE_RECORDS);
    kta_tile_sum sum{0xFFFFFFFFu, 0xFFFF, 0xFFFF};
    const kta_tile_hdr h = kta::tile_pack_host(tl.p.data(), tl.t.data(), tl.k.data(), tl.v.data(), m, true, part.data(), ts.data(), klen.data(),
                                               vlen.data(), &sum);
    const kta::FilterTile d = kta::filter_tile_decide(f, h, sum, m == KTA_TILE_RECORDS);
    uint64_t pass = 0;
    for (uint64_t j = 0; j < m; j++) pass += passes_by_definition(f, bm, tl.p[j], tl.t[j]);
    if (d == kta::FILTER_TILE_NONE) CHECK(pass == 0, "%s: decided NONE, %llu records pass", what, (unsigned long long)pass);
    if (d == kta::FILTER_TILE_ALL) CHECK(pass == m && m == KTA_TILE_RECORDS, "%s: decided ALL, %llu of %llu pass", what, (unsigned long long)pass, (unsigned long long)m);
    if (want >= 0) CHECK((int)d == want, "%s: decided %d, expected %d", what, (int)d, want);
    // a tile that is not whole, not compact or not summarised is always read
    CHECK(kta::filter_tile_decide(f, h, sum, false) == kta::FILTER_TILE_READ, "%s: a cut tile must be read", what);
    CHECK(kta::filter_tile_decide(f, h, kta_tile_sum{0, 0, 0}, true) == kta::FILTER_TILE_READ, "%s: no summary, must be read", what);
    kta_tile_hdr raw = h;
    raw.mode = KTA_TILE_RAW;
    CHECK(kta::filter_tile_decide(f, raw, sum, true) == kta::FILTER_TILE_READ, "%s: a raw tile must be read", what);
}

Tile span_tile(int64_t lo, int64_t hi, uint32_t P, uint64_t m = KTA_TILE_RECORDS)
{
    Tile tl;
    for (uint64_t j = 0; j < m; j++) {
        tl.p.push_back((int32_t)(rnd() % P));
        tl.t.push_back(j == 0 ? lo : j == 1 ? hi : lo + (int64_t)(rnd() % (uint64_t)(hi - lo + 1)));
        tl.k.push_back(3), tl.v.push_back(7);
    }
    return tl;
}

void check_tiles()
{
    const uint32_t P = 9;
    std::vector<uint32_t> bm(1, 0b101001u);
    const int64_t F = 1000000, T = 2000000;
    const kta::FilterSpec win{F, T, P, 0}, win_set{F, T, P, 1}, set_only{INT64_MIN, INT64_MAX, P, 1}, from_only{F, INT64_MAX, P, 0},
        to_only{INT64_MIN, T, P, 0};
    using kta::FILTER_TILE_ALL;
    using kta::FILTER_TILE_NONE;
    using kta::FILTER_TILE_READ;
    check_tile(span_tile(F, T - 1, P), win, bm, "just inside", FILTER_TILE_ALL);
    check_tile(span_tile(F, T - 1, P), win_set, bm, "just inside, with a set", FILTER_TILE_READ);
    check_tile(span_tile(F - 1, T - 1, P), win, bm, "one ms early", FILTER_TILE_READ);
    check_tile(span_tile(F, T, P), win, bm, "one ms late", FILTER_TILE_READ);
    check_tile(span_tile(F - 5000, F - 1, P), win, bm, "just before", FILTER_TILE_NONE);
    check_tile(span_tile(F - 5000, F - 1, P), win_set, bm, "just before, with a set", FILTER_TILE_NONE);
    check_tile(span_tile(F - 5000, F, P), win, bm, "touches from", FILTER_TILE_READ);
    check_tile(span_tile(T, T + 5000, P), win, bm, "just after", FILTER_TILE_NONE);
    check_tile(span_tile(T - 1, T + 5000, P), win, bm, "touches to", FILTER_TILE_READ);
    check_tile(span_tile(F - 10, T + 10, P), win, bm, "straddles both", FILTER_TILE_READ);
    check_tile(span_tile(F + 5, F + 900, P), from_only, bm, "from only, inside", FILTER_TILE_ALL);
    check_tile(span_tile(F - 900, F - 5, P), from_only, bm, "from only, before", FILTER_TILE_NONE);
    check_tile(span_tile(T - 900, T - 5, P), to_only, bm, "to only, inside", FILTER_TILE_ALL);
    check_tile(span_tile(T, T + 5, P), to_only, bm, "to only, after", FILTER_TILE_NONE);
    check_tile(span_tile(F, T - 1, P), set_only, bm, "a set alone decides nothing", FILTER_TILE_READ);
    check_tile(span_tile(F, T - 1, P, 517), win, bm, "the partial last tile has no summary", FILTER_TILE_READ);
    {   // UNTIMED: a record of -1 inside the window's span
        Tile tl = span_tile(F, T - 1, P);
        tl.t[500] = -1;
        check_tile(tl, win, bm, "untimed record inside", FILTER_TILE_READ);
        Tile out = span_tile(T, T + 50, P);
        out.t[7] = -1;
        check_tile(out, win, bm, "untimed record outside", FILTER_TILE_NONE);
        Tile none = span_tile(F, T - 1, P);
        for (auto &x : none.t) x = -1;
        check_tile(none, win, bm, "no timestamp at all", FILTER_TILE_NONE);
        check_tile(none, set_only, bm, "no timestamp at all, a set alone", FILTER_TILE_READ);
    }
    {   // part_max: a record of partition -1 is stored as 0xFFFF; one at or beyond P is a bad partition that still passes
        Tile tl = span_tile(F, T - 1, P);
        tl.p[9] = -1;
        check_tile(tl, win, bm, "part_max == 0xFFFF", FILTER_TILE_READ);
        Tile bad = span_tile(F, T - 1, P);
        bad.p[1000] = (int32_t)P;
        check_tile(bad, win, bm, "part_max == P", FILTER_TILE_READ);
        Tile top = span_tile(F, T - 1, P);
        top.p[3] = (int32_t)P - 1;
        check_tile(top, win, bm, "part_max == P - 1", FILTER_TILE_ALL);
        Tile wide = span_tile(F, T - 1, P);
        wide.p[3] = 70000;                      // does not fit u16: the tile stays raw
        check_tile(wide, win, bm, "a raw tile", FILTER_TILE_READ);
    }
    {   // the far ends of i64
        check_tile(span_tile(INT64_MAX - 100, INT64_MAX, P), from_only, bm, "up to INT64_MAX, from only", FILTER_TILE_ALL);
        check_tile(span_tile(INT64_MAX - 100, INT64_MAX, P), kta::FilterSpec{0, INT64_MAX - 1, P, 0}, bm, "up to INT64_MAX, to below", FILTER_TILE_READ);
        check_tile(span_tile(INT64_MIN + 1, INT64_MIN + 100, P), to_only, bm, "from INT64_MIN + 1, to only", FILTER_TILE_ALL);
        check_tile(span_tile(INT64_MIN + 1, INT64_MIN + 100, P), win, bm, "from INT64_MIN + 1, window", FILTER_TILE_NONE);
    }
    for (int round = 0; round < 400; round++) {   // random tiles and windows around them
        const int64_t lo = F + (int64_t)(rnd() % 3000) - 1500, hi = lo + (int64_t)(rnd() % 3000);
        Tile tl = span_tile(lo, hi, round % 3 ? P : P + 2);
        if (round % 5 == 0) tl.t[rnd() % KTA_TILE_RECORDS] = -1;
        if (round % 7 == 0) tl.p[rnd() % KTA_TILE_RECORDS] = -1;
        const int64_t a = F + (int64_t)(rnd() % 3000) - 1500, b = a + 1 + (int64_t)(rnd() % 3000);
        const kta::FilterSpec f{round % 11 == 0 ? INT64_MIN : a, round % 13 == 0 ? INT64_MAX : b, P, (uint32_t)(round & 1)};
        check_tile(tl, f, bm, "random", -1);
    }
}

// One tile through the scatter's rank: four waves, four instructions of 64 each, the ballots built from the predicate,
// every passing record stored at its rank — against the sequential compaction.
void check_rank(const std::vector<uint8_t> &pass, const char *what)
{
    uint64_t ballot[4][4] = {};
    for (uint32_t j = 0; j < KTA_TILE_RECORDS; j++)
        if (pass[j]) ballot[j / 256][(j % 256) / 64] |= 1ull << (j % 64);
    uint32_t wave_total[4], count = 0;
    for (uint32_t w = 0; w < 4; w++) {
        wave_total[w] = 0;
        for (uint32_t k = 0; k < 4; k++) wave_total[w] += (uint32_t)__builtin_popcountll(ballot[w][k]);
        count += wave_total[w];
    }
    std::vector<uint32_t> want, got(count, 0xFFFFFFFFu);
    for (uint32_t j = 0; j < KTA_TILE_RECORDS; j++)
        if (pass[j]) want.push_back(j);
    CHECK(want.size() == count, "%s: count %u, expected %zu", what, count, want.size());
    for (uint32_t w = 0, base = 0; w < 4; base += wave_total[w], w++)
        for (uint32_t k = 0; k < 4; k++)
            for (uint32_t lane = 0; lane < 64; lane++) {
                if (!((ballot[w][k] >> lane) & 1ull)) continue;
                const uint32_t r = kta::filter_tile_rank(base, ballot[w], k, lane);
                CHECK(r < count, "%s: rank %u of %u", what, r, count);
                if (r < count) {
                    CHECK(got[r] == 0xFFFFFFFFu, "%s: rank %u given twice", what, r);
                    got[r] = w * 256 + k * 64 + lane;
                }
            }
    CHECK(got == want, "%s: the compaction is not the sequential one", what);
}

void check_ranks()
{
    for (uint32_t cls : {0u, 1u, 63u, 64u, 65u, 1023u, 1024u})
        for (int shape = 0; shape < 4; shape++) {
            std::vector<uint8_t> pass(KTA_TILE_RECORDS, 0);
            if (shape == 0) {                                   // the first cls records
                for (uint32_t j = 0; j < cls; j++) pass[j] = 1;
            } else if (shape == 1) {                            // the last
                for (uint32_t j = 0; j < cls; j++) pass[KTA_TILE_RECORDS - 1 - j] = 1;
            } else {                                            // anywhere
                for (uint32_t left = cls; left;) {
                    const uint32_t j = (uint32_t)(rnd() % KTA_TILE_RECORDS);
                    if (!pass[j]) pass[j] = 1, left--;
                }
            }
            char what[64];
            snprintf(what, sizeof what, "count class %u, shape %d", cls, shape);
            check_rank(pass, what);
        }
    CHECK(kta::filter_slice_tiles(0, 0) == 0 && kta::filter_slice_tiles(0, 1) == 1 && kta::filter_slice_tiles(0, 1024) == 1 &&
              kta::filter_slice_tiles(0, 1025) == 2 && kta::filter_slice_tiles(300, 1024) == 2 && kta::filter_slice_tiles(1023, 2) == 2 &&
              kta::filter_slice_tiles(1024, 1024) == 1 && kta::filter_slice_tiles(300, (1ull << 26)) == (1ull << 16) + 1,
          "filter_slice_tiles");
}

} // namespace

int main()
{
    check_predicate();
    check_tiles();
    check_ranks();
    if (g_failed) {
        fprintf(stderr, "%d of %ld checks failed\n", g_failed, g_checks);
        return 1;
    }
    printf("OK %ld\n", g_checks);
    return 0;
}

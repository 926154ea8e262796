// csrc/kta_plane_pack.h on the CPU: the words the plane loop adds to one front slot — count | raw key sum | raw value
// sum in one 64-bit word, null keys | tombstones in a 32-bit word added only where it is not zero — filled to exactly
// the bound of one plane interval for 1, 2, 4, 8 and 64 replicas, record by record and as uniform quads, through the
// header's own pack / unpack / interval functions, against plain 64-bit sums.  And one record beyond the bound: the
// count field carries, which is what the header's asserts exclude.  Built with AddressSanitizer + UBSan by
// tests/test_plane_pack_host.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "kta_plane_pack.h"

using namespace kta;

namespace {

constexpr uint32_t kFrontFlushTiles = 32;   // kta_kernels.hip

int failures = 0;
#define CHECK(cond, ...)                                                                                                  \
    do {                                                                                                                  \
        if (!(cond)) {                                                                                                    \
            printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond);                                                        \
            printf(__VA_ARGS__);                                                                                          \
            printf("\n");                                                                                                 \
            if (++failures > 20) exit(1);                                                                                 \
        }                                                                                                                 \
    } while (0)

struct Rec {
    int32_t k, v;   // lengths as the oracle sees them: -1 for none
};
uint32_t stored_k(const Rec &r) { return r.k < 0 ? kPlaneKeyNone : (uint32_t)r.k; }
uint32_t stored_v(const Rec &r) { return r.v < 0 ? kPlaneValNone : (uint32_t)r.v; }

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd()
{
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

// A front slot as the kernel keeps it: the 64-bit add wraps like the LDS add, the flag add is a 32-bit add into the low
// dword of the second word and is left out where the flags are zero.
struct Slot {
    uint64_t w = 0, f = 0;
    uint64_t flag_adds = 0;
    void add(const PlaneAdd &a)
    {
        w += plane_word(a);
        if (a.flags) {
            f = (f & ~0xFFFFFFFFull) | (uint32_t)((uint32_t)f + a.flags);
            flag_adds++;
        }
    }
};

struct Plain {
    uint64_t cnt = 0, tb = 0, kn = 0, ks = 0, vs = 0;
    void add(const Rec &r)
    {
        cnt++;
        tb += r.v < 0;
        kn += r.k < 0;
        ks += r.k < 0 ? 0u : (uint32_t)r.k;
        vs += r.v < 0 ? 0u : (uint32_t)r.v;
    }
};

void compare(const Slot &s, const Plain &want, const char *what, uint32_t R, bool quads)
{
    PlaneSums got;
    plane_unpack(got, s.w, s.f);
    plane_corrected(got);
    CHECK(got.cnt == want.cnt && got.tb == want.tb && got.kn == want.kn && got.ks == want.ks && got.vs == want.vs,
          "%s, R = %u, %s: got %llu %llu %llu %llu %llu, want %llu %llu %llu %llu %llu", what, R, quads ? "quads" : "records",
          (unsigned long long)got.cnt, (unsigned long long)got.tb, (unsigned long long)got.kn, (unsigned long long)got.ks,
          (unsigned long long)got.vs, (unsigned long long)want.cnt, (unsigned long long)want.tb, (unsigned long long)want.kn,
          (unsigned long long)want.ks, (unsigned long long)want.vs);
}

// The records of one slot over one interval, one at a time and as uniform quads.
void fill(const std::vector<Rec> &recs, const char *what, uint32_t R)
{
    Plain want;
    Slot one, quad;
    for (const Rec &r : recs) {
        want.add(r);
        const PlaneAdd a = plane_pack_record(stored_k(r), stored_v(r));
        CHECK(a.lo == (1u | (stored_k(r) << 14)) && a.hi == (stored_v(r) << 3), "the record's dwords");
        CHECK(a.flags == ((uint32_t)(r.k < 0) | ((uint32_t)(r.v < 0) << 16)), "the record's flag word");
        one.add(a);
    }
    for (size_t i = 0; i + 4 <= recs.size(); i += 4) {
        uint32_t ku = 0, vu = 0, kn = 0, tb = 0;
        for (size_t j = i; j < i + 4; j++) {
            ku += stored_k(recs[j]), vu += stored_v(recs[j]);
            kn += recs[j].k < 0, tb += recs[j].v < 0;
        }
        quad.add(plane_pack(4u, ku, vu, kn, tb));
    }
    compare(one, want, what, R, false);
    compare(quad, want, what, R, true);
    CHECK(one.w == quad.w && one.f == quad.f, "%s, R = %u: records and quads leave other words", what, R);
    uint64_t flagged = 0;
    for (const Rec &r : recs) flagged += r.k < 0 || r.v < 0;
    CHECK(one.flag_adds == flagged, "%s, R = %u: %llu flag adds for %llu flagged records", what, R,
          (unsigned long long)one.flag_adds, (unsigned long long)flagged);
    CHECK((one.f >> 32) == 0, "the flag add stays in the low dword");
}

// Two replicas at the bound: each unpacked on its own gives the partition's sums; their words summed first do not.
void replicas_are_unpacked_one_by_one()
{
    Slot a, b;
    Plain want;
    for (uint64_t i = 0; i < kPlaneSlotRecords; i++) {
        const Rec r{-1, -1};
        a.add(plane_pack_record(stored_k(r), stored_v(r)));
        b.add(plane_pack_record(stored_k(r), stored_v(r)));
        want.add(r), want.add(r);
    }
    PlaneSums each;
    plane_unpack(each, a.w, a.f);
    plane_unpack(each, b.w, b.f);
    plane_corrected(each);
    CHECK(each.cnt == want.cnt && each.tb == want.tb && each.kn == want.kn && each.ks == 0 && each.vs == 0, "two replicas, each unpacked");
    PlaneSums summed;
    plane_unpack(summed, a.w + b.w, a.f + b.f);
    CHECK(summed.cnt != want.cnt, "the replicas' summed words carry: 2 x 8192 records do not fit the count field");
}

}   // namespace

int main()
{
    const uint32_t reps[] = {0, 1, 2, 3, 6};   // R = 1, 2, 4, 8, 64
    for (uint32_t rl : reps) {
        const uint32_t R = 1u << rl;
        const uint32_t tiles = plane_interval_tiles(rl, kFrontFlushTiles);
        const uint64_t n = plane_slot_records(rl, kFrontFlushTiles);
        CHECK(tiles == (8u * R < kFrontFlushTiles ? 8u * R : kFrontFlushTiles), "R = %u: an interval of %u tiles", R, tiles);
        CHECK(n == (uint64_t)tiles * (kPlaneTileRecords / R) && n <= kPlaneSlotRecords, "R = %u: %llu records per slot", R, (unsigned long long)n);
        CHECK((rl > 2) == (n < kPlaneSlotRecords), "R = 1, 2, 4 reach the bound itself");
        fill(std::vector<Rec>(n, Rec{254, 65534}), "the longest lengths", R);
        fill(std::vector<Rec>(n, Rec{-1, -1}), "both markers", R);
        fill(std::vector<Rec>(n, Rec{0, 0}), "empty key and value", R);
        for (int round = 0; round < 8; round++) {
            std::vector<Rec> recs(n);
            const uint32_t flag_permille = round < 4 ? 100u : 1000u * (uint32_t)(round - 4) / 3u;   // config 4's tenth, then 0 .. all
            for (Rec &r : recs) {
                r.k = rnd() % 1000u < flag_permille ? -1 : (int32_t)(rnd() % 255u);
                r.v = rnd() % 1000u < flag_permille ? -1 : (int32_t)(rnd() % 65535u);
                if (rnd() % 16u == 0) r = Rec{254, 65534};
            }
            fill(recs, "a random mix", R);
        }
    }
    replicas_are_unpacked_one_by_one();

    // One record beyond the bound: 8193 tombstones' markers are 536 928 255 >= 2^29, so the raw value sum leaves the word
    // — the field holds the bound and not one record more, which is what the header's assert states.  And twice the
    // bound — what kFrontFlushTiles tiles would give a slot of two replicas — carries out of the count into the key sum.
    {
        Slot v;
        for (uint64_t i = 0; i < kPlaneSlotRecords; i++) v.add(plane_pack_record(kPlaneKeyNone, kPlaneValNone));
        PlaneSums at;
        plane_unpack(at, v.w, v.f);
        CHECK(at.vs == kPlaneSlotRecords * (uint64_t)kPlaneValNone && at.cnt == kPlaneSlotRecords, "the bound itself is held");
        v.add(plane_pack_record(kPlaneKeyNone, kPlaneValNone));
        PlaneSums past;
        plane_unpack(past, v.w, v.f);
        CHECK((kPlaneSlotRecords + 1) * kPlaneValNone >= (1ull << kPlaneValBits), "8193 x 0xFFFF does not fit 29 bits");
        CHECK(past.cnt == kPlaneSlotRecords + 1 && past.vs != (kPlaneSlotRecords + 1) * (uint64_t)kPlaneValNone,
              "one record beyond the bound: the raw value sum left the word (vs %llu)", (unsigned long long)past.vs);
        Slot s;
        for (uint64_t i = 0; i < 2 * kPlaneSlotRecords; i++) s.add(plane_pack_record(0, 0));
        PlaneSums got;
        plane_unpack(got, s.w, s.f);
        CHECK(got.cnt == 0 && got.ks == 1, "2 x 8192 records of (0, 0): the count carried into the key sum (cnt %llu, ks %llu)",
              (unsigned long long)got.cnt, (unsigned long long)got.ks);
        CHECK(kFrontFlushTiles * (kPlaneTileRecords / 2u) == 2 * kPlaneSlotRecords && plane_slot_records(1, kFrontFlushTiles) == kPlaneSlotRecords,
              "which 32 tiles would be for two replicas, and the rule's 16 tiles are not");
    }

    if (failures) {
        printf("plane_pack_check: %d failures\n", failures);
        return 1;
    }
    printf("plane_pack_check OK\n");
    return 0;
}

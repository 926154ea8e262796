// segments_check.cpp — test infrastructure: a program of its own that runs the rule header of the retention what-if
// (csrc/kta_segments.h) natively, built with -fsanitize=address,undefined by tests/test_segments_host.py.  Randomised
// records next to INT32_MAX lengths and segments of 2^40 bytes go through the closing rule; the vector is held against a
// second, per-partition computation (positions from plain prefix sums, rows from a search for the closing record), its
// identities and merge are checked, and the what-if walk is held against the broker's two loops run literally over the
// list of segments.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "kta_segments.h"

using namespace kta;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

struct Rec {
    int32_t p, k, v;
    int64_t t;
};

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            printf("FAILED line %d: %s\n", __LINE__, #c);             \
            exit(1);                                                  \
        }                                                             \
    } while (0)

static void whatif_literal(const std::vector<uint64_t> &vec, uint32_t P, uint32_t M, int64_t now, int64_t rms, int64_t rb, std::vector<uint64_t> &out)
{
    out.assign((size_t)(P + 1) * kRetWords, 0);
    const uint64_t S = vec[segments_globals_at(P, M) + kSegGlobalS];
    for (uint32_t p = 0; p < P; p++) {
        struct Seg { uint64_t c, b, t, h1; };
        std::vector<Seg> log;
        uint64_t pc = 0, pb = 0, pt = 0;
        for (uint32_t s = 0; s + 1 < M; s++) {
            const uint64_t *r = &vec[segments_row_at(p, M, s)];
            if (!r[kSegC]) continue;
            log.push_back(Seg{r[kSegC] - pc, r[kSegB] - pb, r[kSegT] - pt, r[kSegH1]});
            pc = r[kSegC], pb = r[kSegB], pt = r[kSegT];
        }
        const uint64_t *t = &vec[segments_total_at(P, M, p)];
        const Seg active{t[kSegC] - pc, t[kSegB] - pb, t[kSegT] - pt, 0};
        const size_t nseg = log.size();
        size_t n_time = 0, n_size_alone = 0, first = 0;
        if (rms >= 0)
            while (first < nseg && log[first].h1 != 0 && (__int128)now - (__int128)(log[first].h1 - 1) > (__int128)rms) first++, n_time++;
        if (rb >= 0) {
            __int128 diff = (__int128)t[kSegB] - rb;
            for (size_t i = 0; i < nseg && diff - (__int128)log[i].b >= 0; i++) diff -= log[i].b, n_size_alone++;
            __int128 size = 0;
            for (size_t i = first; i < nseg; i++) size += log[i].b;
            diff = size + active.b - rb;
            while (first < nseg && diff - (__int128)log[first].b >= 0) diff -= log[first].b, first++;
        }
        uint64_t *o = &out[(size_t)p * kRetWords];
        o[kRetSegments] = nseg + (active.c ? 1 : 0);
        o[kRetRecords] = t[kSegC], o[kRetBytes] = t[kSegB], o[kRetTombstones] = t[kSegT];
        o[kRetRecordsKept] = active.c, o[kRetBytesKept] = active.b, o[kRetTombstonesKept] = active.t;
        for (size_t i = first; i < nseg; i++) o[kRetRecordsKept] += log[i].c, o[kRetBytesKept] += log[i].b, o[kRetTombstonesKept] += log[i].t;
        o[kRetSegmentsDeleted] = first;
        o[kRetRule] = first == 0 ? 0 : n_time >= n_size_alone ? 1 : 2;
        o[kRetClamped] = t[kSegB] / S >= (uint64_t)(M - 1) ? 1 : 0;
        uint64_t *all = &out[(size_t)P * kRetWords];
        for (uint32_t k = 0; k < kRetWords; k++) {
            if (k == kRetRule) all[k] |= o[k];
            else all[k] += o[k];
        }
    }
}

int main()
{
    const uint64_t Ss[] = {1, 7, 1000, 65536, (1ull << 31) - 1, 1ull << 33, 1ull << 40};
    const uint32_t Ms[] = {2, 3, 17, 500};
    uint64_t cases = 0, closed_total = 0, deleted_total = 0;
    for (uint64_t S : Ss)
        for (uint32_t M : Ms)
            for (uint32_t P : {1u, 3u, 8u}) {
                const uint32_t overhead = (uint32_t)(rnd() % 3 == 0 ? 0 : rnd() % 100);
                const int big = (int)(rnd() % 3);   // 0: small sizes, 1: some INT32_MAX, 2: mostly INT32_MAX
                const uint32_t n = 2000;
                std::vector<Rec> recs(n);
                int64_t ts = 1600000000000ll;
                for (Rec &r : recs) {
                    r.p = rnd() % 20 == 0 ? (rnd() % 2 ? -1 : (int32_t)P) : (int32_t)(rnd() % P);
                    const bool huge = big == 2 ? rnd() % 4 != 0 : big == 1 ? rnd() % 10 == 0 : false;
                    r.k = huge ? INT32_MAX : (int32_t)(rnd() % 60) - 1;
                    r.v = rnd() % 5 == 0 ? -1 : huge && rnd() % 2 ? INT32_MAX : (int32_t)(rnd() % (S < 5000 ? 3 * S + 2 : 5000));
                    ts += (int64_t)(rnd() % 2000) - 600;
                    r.t = rnd() % 30 == 0 ? -1 : rnd() % 200 == 0 ? INT64_MAX : ts;
                }
                CHECK(segments_config_ok(S, M, P));
                std::vector<uint64_t> vec(segments_len(P, M)), other(segments_len(P, M));
                segments_init(vec.data(), P, S, M, overhead);
                for (const Rec &r : recs) segments_apply_record(vec.data(), P, M, r.p, r.k, r.v, r.t);
                // the second computation: per partition, positions, then for every row the one record that closes it
                std::vector<uint64_t> counters((size_t)P * 7, 0);
                uint64_t g_records = 0, g_bad = 0, closed = 0;
                for (uint32_t p = 0; p < P; p++) {
                    uint64_t c = 0, b = 0, t = 0, h1 = 0;
                    std::vector<uint64_t> want((size_t)M * kSegWords, 0);
                    for (const Rec &r : recs) {
                        if (r.p != (int32_t)p) continue;
                        const uint64_t before = b;
                        c++, b += (uint64_t)overhead + (r.k > 0 ? r.k : 0) + (r.v > 0 ? r.v : 0), t += r.v < 0;
                        if (r.t >= 0 && (uint64_t)r.t + 1 > h1) h1 = (uint64_t)r.t + 1;
                        const uint64_t s0 = before / S < M - 1 ? before / S : M - 1, s1 = b / S < M - 1 ? b / S : M - 1;
                        if (s1 > s0) {
                            CHECK(want[s0 * kSegWords] == 0);   // exactly one record closes a row
                            want[s0 * kSegWords + 0] = c, want[s0 * kSegWords + 1] = b, want[s0 * kSegWords + 2] = t, want[s0 * kSegWords + 3] = h1;
                            closed++;
                        }
                        counters[(size_t)p * 7 + 0]++, counters[(size_t)p * 7 + 1] += r.v < 0;
                        counters[(size_t)p * 7 + 5] += r.k > 0 ? r.k : 0, counters[(size_t)p * 7 + 6] += r.v > 0 ? r.v : 0;
                    }
                    for (uint32_t e = 0; e < M * kSegWords; e++) CHECK(vec[segments_row_at(p, M, 0) + e] == want[e]);
                    const uint64_t *tot = &vec[segments_total_at(P, M, p)];
                    CHECK(tot[kSegC] == c && tot[kSegB] == b && tot[kSegT] == t && tot[kSegH1] == h1);
                    for (uint32_t e = 0; e < kSegWords; e++) CHECK(vec[segments_row_at(p, M, M - 1) + e] == 0);   // the last row never closes
                }
                for (const Rec &r : recs) ((uint32_t)r.p < P ? g_records : g_bad)++;
                const uint64_t *g = &vec[segments_globals_at(P, M)];
                CHECK(g[kSegGlobalClosed] == closed && g[kSegGlobalS] == S && g[kSegGlobalM] == M && g[kSegGlobalOverhead] == overhead);
                CHECK(g[6] == 0 && g[7] == 0);
                CHECK(segments_identities_hold(vec.data(), P, M, counters.data(), g_records, g_bad));
                closed_total += closed;
                // merge: by partition (owners hold their partitions, the others zeros) the sum is the whole
                std::vector<uint64_t> a(segments_len(P, M)), b2(segments_len(P, M));
                segments_init(a.data(), P, S, M, overhead), segments_init(b2.data(), P, S, M, overhead);
                for (const Rec &r : recs) segments_apply_record(((uint32_t)r.p < P ? r.p % 2 : r.p == -1) ? a.data() : b2.data(), P, M, r.p, r.k, r.v, r.t);
                CHECK(segments_merge(a.data(), b2.data(), P, M));
                CHECK(a == vec);
                segments_init(other.data(), P, S + 1 <= kSegmentsMaxBytes ? S + 1 : S - 1, M, overhead);
                const std::vector<uint64_t> keep = a;
                CHECK(!segments_merge(a.data(), other.data(), P, M) && a == keep);
                // the what-if against the two loops, over a grid of policies around the data's own timestamps and sizes
                const int64_t nows[] = {ts + 1000, ts - 500000, 0, INT64_MAX, -5};
                const int64_t rmss[] = {-1, 0, 1000, 400000, INT64_MAX};
                uint64_t maxb = 0;
                for (uint32_t p = 0; p < P; p++) maxb = vec[segments_total_at(P, M, p) + kSegB] > maxb ? vec[segments_total_at(P, M, p) + kSegB] : maxb;
                const int64_t rbs[] = {-1, 0, 1, (int64_t)(maxb / 2), (int64_t)(maxb < (uint64_t)INT64_MAX ? maxb : INT64_MAX), INT64_MAX};
                std::vector<uint64_t> got((size_t)(P + 1) * kRetWords), want;
                for (int64_t now : nows)
                    for (int64_t rms : rmss)
                        for (int64_t rb : rbs) {
                            retention_whatif(vec.data(), P, M, now, rms, rb, got.data());
                            whatif_literal(vec, P, M, now, rms, rb, want);
                            CHECK(got == want);
                            deleted_total += got[(size_t)P * kRetWords + kRetSegmentsDeleted];
                            cases++;
                        }
            }
    CHECK(closed_total > 1000 && deleted_total > 1000);
    printf("OK %llu what-if cases, %llu rows closed, %llu segments deleted\n", (unsigned long long)cases, (unsigned long long)closed_total,
           (unsigned long long)deleted_total);
    return 0;
}

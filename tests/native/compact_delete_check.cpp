// compact_delete_check.cpp — test infrastructure: a program of its own that runs the rule header of the compact,delete
// what-if (csrc/kta_compact_delete.h) natively, built with -fsanitize=address,undefined by tests/test_compact_delete_host.py.
// Randomised records with random classes next to INT32_MAX lengths and segments of 1 byte to 2^40 go through
// kept_apply_record beside segments_apply_record; the kept vector is held against a second, per-partition computation, the
// identities against compaction words summed the same way (and against perturbed vectors), and the what-if walk against
// the broker's two loops run literally over the list of cleaned segments.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "kta_compact_delete.h"

using namespace kta;

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}

struct Rec {
    int32_t p, k, v;
    int64_t t;
    uint8_t cls;
};

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            printf("FAILED line %d: %s\n", __LINE__, #c);             \
            exit(1);                                                  \
        }                                                             \
    } while (0)

static void whatif_literal(const std::vector<uint64_t> &seg, const std::vector<uint64_t> &kept, uint32_t P, uint32_t M, int64_t now, int64_t rms,
                           int64_t rb, std::vector<uint64_t> &out)
{
    out.assign((size_t)(P + 1) * kCdWords, 0);
    const uint64_t S = seg[segments_globals_at(P, M) + kSegGlobalS];
    for (uint32_t p = 0; p < P; p++) {
        struct Seg { uint64_t records, bytes, tombstones, h1; };   // a cleaned segment: its survivors
        std::vector<Seg> log;
        uint64_t pl = 0, pt = 0, pk = 0, lc = 0, lb = 0, lt = 0;
        for (uint32_t s = 0; s + 1 < M; s++) {
            const uint64_t *r = &seg[segments_row_at(p, M, s)], *rk = &kept[segments_row_at(p, M, s)];
            if (!r[kSegC]) continue;
            log.push_back(Seg{rk[kKeptL] - pl + rk[kKeptT] - pt, rk[kKeptK] - pk, rk[kKeptT] - pt, r[kSegH1]});
            pl = rk[kKeptL], pt = rk[kKeptT], pk = rk[kKeptK];
            lc = r[kSegC], lb = r[kSegB], lt = r[kSegT];
        }
        const uint64_t *t = &seg[segments_total_at(P, M, p)];
        const Seg active{t[kSegC] - lc, t[kSegB] - lb, t[kSegT] - lt, 0};   // whole: never cleaned
        const size_t nseg = log.size();
        size_t n_time = 0, n_size_alone = 0, first = 0;
        if (rms >= 0)
            while (first < nseg && log[first].h1 != 0 && (__int128)now - (__int128)(log[first].h1 - 1) > (__int128)rms) first++, n_time++;
        if (rb >= 0) {
            __int128 size = active.bytes;
            for (size_t i = 0; i < nseg; i++) size += log[i].bytes;
            __int128 diff = size - rb;
            for (size_t i = 0; i < nseg && diff - (__int128)log[i].bytes >= 0; i++) diff -= log[i].bytes, n_size_alone++;
            size = active.bytes;
            for (size_t i = first; i < nseg; i++) size += log[i].bytes;
            diff = size - rb;
            while (first < nseg && diff - (__int128)log[first].bytes >= 0) diff -= log[first].bytes, first++;
        }
        uint64_t *o = &out[(size_t)p * kCdWords];
        o[kCdRecords] = t[kSegC], o[kCdBytes] = t[kSegB];
        o[kCdCompactedRecords] = active.records, o[kCdCompactedBytes] = active.bytes;
        for (size_t i = 0; i < nseg; i++) o[kCdCompactedRecords] += log[i].records, o[kCdCompactedBytes] += log[i].bytes;
        o[kCdKeptRecords] = active.records, o[kCdKeptBytes] = active.bytes, o[kCdKeptTombstones] = active.tombstones;
        for (size_t i = first; i < nseg; i++)
            o[kCdKeptRecords] += log[i].records, o[kCdKeptBytes] += log[i].bytes, o[kCdKeptTombstones] += log[i].tombstones;
        o[kCdSegmentsDeleted] = first;
        o[kCdRule] = first == 0 ? 0 : n_time >= n_size_alone ? 1 : 2;
        o[kCdClamped] = t[kSegB] / S >= (uint64_t)(M - 1) ? 1 : 0;
        uint64_t *all = &out[(size_t)P * kCdWords];
        for (uint32_t k = 0; k < kCdWords; k++) {
            if (k == kCdRule) all[k] |= o[k];
            else all[k] += o[k];
        }
    }
}

int main()
{
    // the class byte of every class
    CHECK(kept_class_byte(kCompactionLive) == 1 && kept_class_byte(kCompactionTombstone) == 2);
    for (CompactionClass k : {kCompactionUnkeyed, kCompactionSuperseded, kCompactionUnknown, kCompactionLiveOutside, kCompactionTombstoneOutside})
        CHECK(kept_class_byte(k) == 0);
    const uint64_t Ss[] = {1, 7, 1000, 65536, (1ull << 31) - 1, 1ull << 33, 1ull << 40};
    const uint32_t Ms[] = {2, 3, 17, 500};
    uint64_t cases = 0, closed_total = 0, deleted_total = 0, kept_in_closed = 0;
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
                    r.t = rnd() % 30 == 0 ? -1 : ts;
                    // a class the record can have: unkeyed records are not kept, a kept tombstone has no value
                    const bool kept = r.k >= 0 && rnd() % 3 == 0;
                    r.cls = !kept ? kKeptClassNone : r.v < 0 ? kKeptClassTombstone : kKeptClassLive;
                }
                CHECK(segments_config_ok(S, M, P));
                std::vector<uint64_t> seg(segments_len(P, M)), kept(segments_len(P, M)), comp(compaction_len(P), 0);
                segments_init(seg.data(), P, S, M, overhead), segments_init(kept.data(), P, S, M, overhead);
                for (const Rec &r : recs) {
                    segments_apply_record(seg.data(), P, M, r.p, r.k, r.v, r.t);
                    kept_apply_record(kept.data(), P, M, r.p, r.k, r.v, r.cls);
                    comp[(size_t)kCompactionWords * P + kCompactionReplayed]++;
                    if ((uint32_t)r.p >= P) continue;
                    uint64_t *c = &comp[(size_t)kCompactionWords * r.p];
                    if (r.cls == kKeptClassLive) c[kCompactionLiveRecords]++, c[kCompactionLiveKeyBytes] += r.k, c[kCompactionLiveValueBytes] += r.v;
                    if (r.cls == kKeptClassTombstone) c[kCompactionTombstoneRecords]++, c[kCompactionTombstoneKeyBytes] += r.k;
                }
                // the second computation: per partition, positions, then for every row the one record that closes it
                uint64_t closed = 0;
                for (uint32_t p = 0; p < P; p++) {
                    uint64_t l = 0, b = 0, t = 0, kk = 0;
                    std::vector<uint64_t> want((size_t)M * kSegWords, 0);
                    for (const Rec &r : recs) {
                        if (r.p != (int32_t)p) continue;
                        const uint64_t before = b, z = (uint64_t)overhead + (r.k > 0 ? r.k : 0) + (r.v > 0 ? r.v : 0);
                        b += z;
                        if (r.cls == 1) l++, kk += z;
                        if (r.cls == 2) t++, kk += z;
                        const uint64_t s0 = before / S < M - 1 ? before / S : M - 1, s1 = b / S < M - 1 ? b / S : M - 1;
                        if (s1 > s0) {
                            CHECK(want[s0 * kSegWords + kKeptB] == 0);   // exactly one record closes a row
                            want[s0 * kSegWords + kKeptL] = l, want[s0 * kSegWords + kKeptB] = b, want[s0 * kSegWords + kKeptT] = t;
                            want[s0 * kSegWords + kKeptK] = kk;
                            closed++;
                            kept_in_closed += l + t;
                        }
                    }
                    for (uint32_t e = 0; e < M * kSegWords; e++) CHECK(kept[segments_row_at(p, M, 0) + e] == want[e]);
                    const uint64_t *tot = &kept[segments_total_at(P, M, p)];
                    CHECK(tot[kKeptL] == l && tot[kKeptB] == b && tot[kKeptT] == t && tot[kKeptK] == kk);
                }
                const uint64_t *g = &kept[segments_globals_at(P, M)];
                CHECK(g[kSegGlobalClosed] == closed && g[kSegGlobalS] == S && g[kSegGlobalM] == M && g[kSegGlobalOverhead] == overhead);
                CHECK(g[6] == 0 && g[7] == 0);
                closed_total += closed;
                // the identities, and what breaks each of them
                CHECK(compact_delete_identities_hold(seg.data(), kept.data(), comp.data(), P, M));
                {
                    std::vector<uint64_t> bad = kept;
                    bad[segments_total_at(P, M, 0) + kKeptB] += 1;
                    CHECK(!compact_delete_identities_hold(seg.data(), bad.data(), comp.data(), P, M));
                    bad = kept, bad[segments_total_at(P, M, P - 1) + kKeptK] += 1;
                    CHECK(!compact_delete_identities_hold(seg.data(), bad.data(), comp.data(), P, M));
                    bad = kept, bad[segments_globals_at(P, M) + kSegGlobalS] ^= 1;
                    CHECK(!compact_delete_identities_hold(seg.data(), bad.data(), comp.data(), P, M));
                    bad = kept, bad[segments_globals_at(P, M) + kSegGlobalRecords] += 1;
                    CHECK(!compact_delete_identities_hold(seg.data(), bad.data(), comp.data(), P, M));
                    std::vector<uint64_t> badc = comp;
                    badc[(size_t)kCompactionWords * P + kCompactionUnknownRecords] = 1;
                    CHECK(!compact_delete_identities_hold(seg.data(), kept.data(), badc.data(), P, M));
                    badc = comp, badc[kCompactionLiveRecords] += 1;
                    CHECK(!compact_delete_identities_hold(seg.data(), kept.data(), badc.data(), P, M));
                    if (closed) {   // a closed row the kept vector lacks; a row's B that is another
                        for (uint32_t p = 0; p < P; p++)
                            for (uint32_t s = 0; s < M; s++)
                                if (seg[segments_row_at(p, M, s) + kSegC]) {
                                    bad = kept, bad[segments_row_at(p, M, s) + kKeptB] = 0;
                                    CHECK(!compact_delete_identities_hold(seg.data(), bad.data(), comp.data(), P, M));
                                    bad = kept, bad[segments_row_at(p, M, s) + kKeptB] += 1;
                                    CHECK(!compact_delete_identities_hold(seg.data(), bad.data(), comp.data(), P, M));
                                    bad = kept, bad[segments_row_at(p, M, s) + kKeptL] = UINT64_MAX;   // not monotone (or above the total)
                                    CHECK(!compact_delete_identities_hold(seg.data(), bad.data(), comp.data(), P, M));
                                    p = P, s = M;
                                }
                    }
                }
                // the what-if against the two loops, over a grid of policies around the data's own timestamps and sizes
                const int64_t nows[] = {ts + 1000, ts - 500000, 0, INT64_MAX, -5};
                const int64_t rmss[] = {-1, 0, 1000, 400000, INT64_MAX};
                uint64_t maxk = 0;
                for (uint32_t p = 0; p < P; p++) maxk = kept[segments_total_at(P, M, p) + kKeptK] > maxk ? kept[segments_total_at(P, M, p) + kKeptK] : maxk;
                const int64_t rbs[] = {-1, 0, 1, (int64_t)(maxk / 2), (int64_t)(maxk < (uint64_t)INT64_MAX ? maxk : INT64_MAX), INT64_MAX};
                std::vector<uint64_t> got((size_t)(P + 1) * kCdWords), want;
                for (int64_t now : nows)
                    for (int64_t rms : rmss)
                        for (int64_t rb : rbs) {
                            compact_delete_whatif(seg.data(), kept.data(), P, M, now, rms, rb, got.data());
                            whatif_literal(seg, kept, P, M, now, rms, rb, want);
                            CHECK(got == want);
                            for (uint32_t p = 0; p <= P; p++) {   // what the words mean to one another
                                const uint64_t *o = &got[(size_t)p * kCdWords];
                                CHECK(o[kCdKeptRecords] <= o[kCdCompactedRecords] && o[kCdCompactedRecords] <= o[kCdRecords]);
                                CHECK(o[kCdKeptBytes] <= o[kCdCompactedBytes] && o[kCdCompactedBytes] <= o[kCdBytes]);
                                CHECK(o[kCdKeptTombstones] <= o[kCdKeptRecords]);
                            }
                            deleted_total += got[(size_t)P * kCdWords + kCdSegmentsDeleted];
                            cases++;
                        }
            }
    CHECK(closed_total > 1000 && deleted_total > 1000 && kept_in_closed > 1000);
    printf("OK %llu what-if cases, %llu rows closed, %llu segments deleted\n", (unsigned long long)cases, (unsigned long long)closed_total,
           (unsigned long long)deleted_total);
    return 0;
}

// kta_segments_wave.h — the wave step of the retention what-if's segment pass (kta_set_segments, include/kta_hip.h; the
// rule is kta_segments.h's): one instruction of a wave holds 64 consecutive records, lane order is record order, and
// every lane that takes part needs its partition's running state {C, B, T, H + 1} INCLUDING its own record —
//   run[p] + the records of the lower lanes of its partition + its own
// — after which run[p] holds the whole instruction.  A lane whose record closes a row (segments_closes) says so.
// (Included by kta_segments.hip and, compiled for the host over tests/native/wave_emu.h, by tests/native/segments_emu.cpp:
// the CPU suite runs this text.)
//
// The two paths are kta_ts_order_wave.h's, with sums beside the maximum:
//   one partition   every lane that takes part has the first one's partition: one wave-wide inclusive prefix — B a u64
//                   sum, records | tombstones << 16 one u32 sum, H + 1 a u64 maximum —, seeded with run[p]; lane 63 writes.
//   general         byte-tag collision groups, one prefix per colliding partition; the lanes left over are alone in their
//                   partitions and read and write run[p] themselves.
// No lane pays a 64-bit division unless its partition reaches a boundary in this instruction: nxt[p], beside run[p], is
// the next offset at which the partition's segment changes (segments_next_boundary of run[p].B); a lane whose B stays
// below it closes nothing, and only the lane that writes run[p] past it works out the next one.
//
// KEPT (the compact,delete what-if's kept rows, kta_compact_delete.h): the same step over the words {L, B, T, K} — the
// count contribution is the flag `counted` instead of the constant 1, `tomb` says "a tombstone that survives", and the
// fourth word is the SUM of the values handed in as h1 (the record's size where it survives, else 0) instead of their
// maximum.  Positions (B, nxt, closes) are the same in both instantiations.
// (Whoever includes this — inside a namespace of its own — has included kta_segments.h before.)
#pragma once

#ifndef KTA_READLANE
#define KTA_READLANE(v, l) ((uint32_t)__builtin_amdgcn_readlane((int)(v), (int)(l)))
#endif
#ifndef KTA_BALLOT64
#define KTA_BALLOT64(p) ((uint64_t)__builtin_amdgcn_ballot_w64(p))
#endif
#ifndef KTA_SHFL_UP
#define KTA_SHFL_UP(v, off) __shfl_up((v), (off))
#endif
// between the LDS operations of two instructions of a wave whose order matters (the hardware keeps a wave's LDS
// operations in program order; this keeps the compiler from moving them)
#ifndef KTA_SEG_LDS_ORDER
#define KTA_SEG_LDS_ORDER() asm volatile("" ::: "memory")
#endif

// a record that takes part: counted by the metrics handler (a negative partition is a large unsigned one)
__device__ __forceinline__ bool seg_takes_part(int32_t p, uint32_t P) { return (uint32_t)p < P; }

__device__ __forceinline__ uint64_t seg_max(uint64_t a, uint64_t b) { return a > b ? a : b; }
// how the fourth word combines: the maximum, or (KEPT) the sum
template <bool KEPT> __device__ __forceinline__ uint64_t seg_join(uint64_t a, uint64_t b) { return KEPT ? a + b : seg_max(a, b); }

__device__ __forceinline__ uint64_t seg_shfl_up(uint64_t v, uint32_t off)
{
    const uint32_t lo = KTA_SHFL_UP((uint32_t)v, off);
    const uint32_t hi = KTA_SHFL_UP((uint32_t)(v >> 32), off);
    return ((uint64_t)hi << 32) | lo;
}

// a lane's own record, then the inclusive prefix over lanes [0, lane]
struct SegPrefix {
    uint64_t b;     // bytes
    uint32_t ct;    // records | tombstones << 16
    uint64_t h;     // H + 1 (0: none); KEPT: kept bytes
};
__device__ __forceinline__ SegPrefix seg_own(bool in, uint64_t z, bool tomb, uint64_t h1, bool counted = true)
{
    return in ? SegPrefix{z, (counted ? 1u : 0u) | (tomb ? 1u << 16 : 0u), h1} : SegPrefix{0, 0, 0};
}
template <bool KEPT = false> __device__ __forceinline__ void seg_prefix(uint32_t lane, SegPrefix &a)
{
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint64_t tb = seg_shfl_up(a.b, off), th = seg_shfl_up(a.h, off);
        const uint32_t tc = KTA_SHFL_UP(a.ct, off);
        if (lane >= off) a.b += tb, a.ct += tc, a.h = seg_join<KEPT>(a.h, th);
    }
}

// What a lane that takes part gets: its partition's state with its record in it, and whether that record closes `row`.
struct SegAt {
    uint64_t v[kta::kSegWords];
    uint32_t row;
    bool closes;
};

// seed: run[p] and nxt[p] as they were before the instruction; a: the lane's inclusive prefix; z: its record's size
template <bool KEPT = false>
__device__ __forceinline__ void seg_place(const uint64_t (&seed)[kta::kSegWords], uint64_t nx, const SegPrefix &a, uint64_t z, uint64_t S, uint32_t M,
                                          SegAt &at)
{
    at.v[kta::kSegC] = seed[kta::kSegC] + (a.ct & 0xFFFFu);
    at.v[kta::kSegB] = seed[kta::kSegB] + a.b;
    at.v[kta::kSegT] = seed[kta::kSegT] + (a.ct >> 16);
    at.v[kta::kSegH1] = seg_join<KEPT>(seed[kta::kSegH1], a.h);
    at.closes = false;
    at.row = 0;
    if (at.v[kta::kSegB] >= nx) at.closes = kta::segments_closes(at.v[kta::kSegB] - z, at.v[kta::kSegB], S, M, &at.row);
}
// run[p] = seed + a, a the prefix of the partition's last lane; nxt[p] follows when B got past it
template <bool KEPT = false>
__device__ __forceinline__ void seg_advance(uint64_t *run_p, uint64_t *nxt_p, const uint64_t (&seed)[kta::kSegWords], uint64_t nx,
                                            const SegPrefix &a, uint64_t S, uint32_t M)
{
    const uint64_t b = seed[kta::kSegB] + a.b;
    run_p[kta::kSegC] = seed[kta::kSegC] + (a.ct & 0xFFFFu);
    run_p[kta::kSegB] = b;
    run_p[kta::kSegT] = seed[kta::kSegT] + (a.ct >> 16);
    run_p[kta::kSegH1] = seg_join<KEPT>(seed[kta::kSegH1], a.h);
    if (b >= nx) *nxt_p = kta::segments_next_boundary(b, S, M);
}

// the lanes `in` — all of partition pg — as one group (every lane of the wave takes the steps)
template <bool KEPT = false>
__device__ __forceinline__ void seg_group(uint64_t *run, uint64_t *nxt, uint32_t lane, bool in, uint32_t pg, uint64_t z, bool tomb, uint64_t h1,
                                          uint64_t S, uint32_t M, SegAt &at, bool counted = true)
{
    SegPrefix a = seg_own(in, z, tomb, h1, counted);
    seg_prefix<KEPT>(lane, a);
    uint64_t seed[kta::kSegWords];
#pragma unroll
    for (uint32_t k = 0; k < kta::kSegWords; k++) seed[k] = run[(size_t)pg * kta::kSegWords + k];
    const uint64_t nx = nxt[pg];
    if (in) seg_place<KEPT>(seed, nx, a, z, S, M, at);
    KTA_SEG_LDS_ORDER();
    if (lane == 63) seg_advance<KEPT>(run + (size_t)pg * kta::kSegWords, nxt + pg, seed, nx, a, S, M);   // (lane 63's prefix is the group's sum)
    KTA_SEG_LDS_ORDER();
}

// One instruction.  run: the wave's table u64[P][4] (LDS), nxt: u64[P] (LDS), tag: the wave's byte table u8[P] (LDS; any
// contents).  on: the lane holds a record of partition p that takes part, of size z, a tombstone or not, with the
// timestamp word h1 (the values of the other lanes are not looked at).  at: what a lane that is on gets (untouched
// otherwise).  n_one / n_groups (the same on every lane) count the instructions that took the one-partition path and the
// colliding groups resolved.  Every lane of the wave must call it.  KEPT: see the head of this file.
template <bool KEPT = false>
__device__ __forceinline__ void seg_wave_step(uint64_t *run, uint64_t *nxt, uint8_t *tag, uint32_t lane, bool on, uint32_t p, uint64_t z, bool tomb,
                                              uint64_t h1, uint64_t S, uint32_t M, SegAt &at, uint32_t &n_one, uint32_t &n_groups,
                                              bool counted = true)
{
    const uint64_t live = KTA_BALLOT64(on);
    if (live == 0) return;
    const uint32_t p0 = KTA_READLANE(p, (uint32_t)__builtin_ctzll(live));
    if (KTA_BALLOT64(on && p != p0) == 0) {
        seg_group<KEPT>(run, nxt, lane, on, p0, z, tomb, h1, S, M, at, counted);
        n_one++;
        return;
    }
    if (on) tag[p] = (uint8_t)lane;
    KTA_SEG_LDS_ORDER();
    const uint32_t seen = on ? (uint32_t) * static_cast<const volatile uint8_t *>(tag + p) : lane;
    KTA_SEG_LDS_ORDER();
    uint64_t todo = KTA_BALLOT64(on && seen != lane);   // lost their byte to another lane of their partition
    uint64_t grouped = 0;
    while (todo) {                                      // (wave-uniform) one trip per colliding partition
        const uint32_t pg = KTA_READLANE(p, (uint32_t)__builtin_ctzll(todo));
        const bool in = on && p == pg;
        const uint64_t grp = KTA_BALLOT64(in);
        seg_group<KEPT>(run, nxt, lane, in, pg, z, tomb, h1, S, M, at, counted);
        grouped |= grp;
        todo &= ~grp;
        n_groups++;
    }
    if (on && !((grouped >> lane) & 1ull)) {            // alone in its partition
        const SegPrefix a = seg_own(true, z, tomb, h1, counted);
        uint64_t seed[kta::kSegWords];
#pragma unroll
        for (uint32_t k = 0; k < kta::kSegWords; k++) seed[k] = run[(size_t)p * kta::kSegWords + k];
        const uint64_t nx = nxt[p];
        seg_place<KEPT>(seed, nx, a, z, S, M, at);
        seg_advance<KEPT>(run + (size_t)p * kta::kSegWords, nxt + p, seed, nx, a, S, M);
    }
    KTA_SEG_LDS_ORDER();
}

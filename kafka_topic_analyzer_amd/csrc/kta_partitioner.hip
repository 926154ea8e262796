// kta_partitioner.hip — the opt-in partitioner pass (KTA_FLAG_PARTITIONER, include/kta_hip.h): Kafka's murmur2 of every
// keyed record, whether the record lies on the partition the Java default partitioner gives its key (checked / placed per
// partition) and where its records and bytes would go with Q partitions (target_records / target_bytes) — sums only, so
// the vector is exact whatever the order, the batching or the sharding.  No reference counterpart.
//
//   kta_partitioner   streams partition (u16 in compact tiles), key_len, key_off, val_len and the key bytes once, as
//                     kta_key_sketch does (256-record wave steps, non-temporal column loads one step ahead, the
//                     unconditional 16-byte key prefetch, four interleaved chains when the wave holds 16-byte keys:
//                     kta_murmur2.h), and accumulates in LDS, sized by P and Q at the launch:
//                       part[P << rp]   u64: checked in the low half, placed in the high half — one ds_add_u64
//                       bytes[Q << rq]  u64: target_bytes                                      — one ds_add_u64
//                       recs[Q << rq]   u32: target_records                                    — one ds_add_u32
//                     A launch takes at most 2^30 records, so no half and no u32 overflows and nothing is flushed before
//                     the end: there the workgroup sums the replicas and adds the non-zero words to the live u64
//                     accumulator.  A word has 2^rp (2^rq) replicas, chosen by the lane, while the arrays stay within
//                     4 KiB + 12 KiB: a topic of few partitions spreads over the banks instead of queueing on one word.
//                     Lanes of one instruction that share a word are combined first: the first keyed lane's group adds
//                     once, kPartCombine times over, and what is left adds alone.  For part the weights are two
//                     popcounts of ballots; for a target the bytes of the group are summed across the wave, only when
//                     the group has kPartGroupMin lanes and more.  One key repeated is then one add per 64 records and
//                     word, two keys alternating lane by lane two, a run of one partition one.
//                     t % P and t % Q are a multiplication by the host's reciprocal (mod_u31: exact for every 31-bit t).
#include "kta_key_stream.h"
#include "kta_murmur2.h"

#include <algorithm>

namespace kta {

namespace {

constexpr uint32_t kPartStep = 256;              // records of one wave step: instruction j of it takes the records 64 j + lane
constexpr int kPartCombine = 2;                  // groups of one word combined per instruction
constexpr uint32_t kPartGroupMin = 4;            // a target group below this adds lane by lane (no sum across the wave)
constexpr uint32_t kPartRepMax = 5;              // log2 of the most replicas of a word: the 32 lanes of a bank group
constexpr uint32_t kPartRepPartBytes = 4096;     // part[] is replicated while it stays within this,
constexpr uint32_t kPartRepTargetBytes = 12288;  // bytes[] and recs[] together within this
constexpr uint32_t kPartSmallLds = kPartRepPartBytes + kPartRepTargetBytes;   // up to here: 256 threads, 7 workgroups per CU
constexpr uint32_t kPartCuLds = 160u * 1024u;
constexpr uint32_t kPartStaticLds = 64;          // s_stat, rounded up

struct PartitionerPlan {
    uint32_t rep_p_log2, rep_q_log2;
    uint32_t lds_bytes;
    uint32_t threads;      // 256, or 1024 when the arrays are larger than kPartSmallLds
    uint32_t wg_per_cu;
};

PartitionerPlan plan_partitioner(uint32_t P, uint32_t Q)
{
    PartitionerPlan pl{};
    while (pl.rep_p_log2 < kPartRepMax && ((uint64_t)P * 8u << (pl.rep_p_log2 + 1)) <= kPartRepPartBytes) pl.rep_p_log2++;
    while (pl.rep_q_log2 < kPartRepMax && ((uint64_t)Q * 12u << (pl.rep_q_log2 + 1)) <= kPartRepTargetBytes) pl.rep_q_log2++;
    pl.lds_bytes = (P * 8u << pl.rep_p_log2) + (Q * 12u << pl.rep_q_log2);
    if (pl.lds_bytes <= kPartSmallLds) {
        pl.threads = 256, pl.wg_per_cu = 7;       // 28 waves per CU: the kernel takes 68 vector registers, seven waves per SIMD
    } else {
        pl.threads = 1024;                        // 16 waves share the arrays; two workgroups where two fit
        pl.wg_per_cu = 2u * (pl.lds_bytes + kPartStaticLds) <= kPartCuLds ? 2 : 1;
    }
    return pl;
}

// murmur2 of the four keys of a lane's step from the prefetched bytes (key None: 0, not used)
__device__ __forceinline__ void murmur2_keys4(uint32_t (&h)[4], const uint4 (&keys)[4], const uint8_t *key_bytes, const int32_t (&kl)[4],
                                              const uint32_t (&ko)[4])
{
    if (__all(kl[0] == 16 && kl[1] == 16 && kl[2] == 16 && kl[3] == 16)) {
        const uint32_t w[4][4] = {{keys[0].x, keys[0].y, keys[0].z, keys[0].w}, {keys[1].x, keys[1].y, keys[1].z, keys[1].w},
                                  {keys[2].x, keys[2].y, keys[2].z, keys[2].w}, {keys[3].x, keys[3].y, keys[3].z, keys[3].w}};
        murmur2_16x4(h, w);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            h[j] = kl[j] >= 0 ? murmur2_prefetched(keys[j].x, keys[j].y, keys[j].z, keys[j].w, key_bytes + (kl[j] > 0 ? ko[j] : 0u), (uint32_t)kl[j]) : 0u;
    }
}

// val_len of the records load_keyed_cols takes for this step: the same clamped indices, unconditional
__device__ __forceinline__ void load_val_len4(const int32_t *val_len, const uint64_t &step, const uint64_t &nsteps, const uint64_t &n,
                                              const uint32_t &lane, int32_t (&vl)[4])
{
    const bool ok = step < nsteps;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint64_t i = step * kPartStep + 64u * j + lane;
        vl[j] = __builtin_nontemporal_load(val_len + (ok && i < n ? i : n - 1));
    }
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void kta_partitioner(PartitionerColumns c, uint64_t n, ModU31 mp, ModU31 mq, uint32_t rep_p_log2,
                                                           uint32_t rep_q_log2, unsigned long long *acc, unsigned long long *stats)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_bytes[];   // [Q << rq]
    const uint32_t P = mp.d, Q = mq.d;
    const uint32_t n_target = Q << rep_q_log2, n_part = P << rep_p_log2;
    unsigned long long *s_part = s_bytes + n_target;                                // [P << rp]
    uint32_t *s_recs = reinterpret_cast<uint32_t *>(s_part + n_part);              // [Q << rq]
    __shared__ unsigned long long s_stat[3];
    for (uint32_t e = threadIdx.x; e < n_target; e += THREADS) s_bytes[e] = 0ull, s_recs[e] = 0u;
    for (uint32_t e = threadIdx.x; e < n_part; e += THREADS) s_part[e] = 0ull;
    if (threadIdx.x < 3) s_stat[threadIdx.x] = 0ull;
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t rep_p = lane & ((1u << rep_p_log2) - 1u), rep_q = lane & ((1u << rep_q_log2) - 1u);
    const uint64_t nsteps = (n + kPartStep - 1) / kPartStep;
    const uint64_t waves = (uint64_t)gridDim.x * (THREADS / 64);
    uint64_t step = (uint64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    uint32_t n_keyed = 0, n_padd = 0, n_qadd = 0;   // (wave-uniform: popcounts of ballots)

    KeyedCols cur;
    int32_t cur_vl[4];
    load_keyed_cols<kPartStep>(c.k, step, nsteps, n, lane, cur);
    load_val_len4(c.val_len, step, nsteps, n, lane, cur_vl);
    while (step < nsteps) {
        uint4 keys[4];
        prefetch_keys4<false>(c.k.key_bytes, cur.kl, cur.ko, keys);
        const uint64_t next = step + waves;
        KeyedCols nxt;
        int32_t nxt_vl[4];
        load_keyed_cols<kPartStep>(c.k, next, nsteps, n, lane, nxt);
        load_val_len4(c.val_len, next, nsteps, n, lane, nxt_vl);
        uint32_t h[4];
        murmur2_keys4(h, keys, c.k.key_bytes, cur.kl, cur.ko);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            // key Some (the empty key included) in a partition the metrics handler counts
            const bool keyed = cur.kl[j] >= 0 && (uint32_t)cur.pt[j] < P;
            const uint32_t t = h[j] & 0x7fffffffu;
            const uint32_t q = mod_u31(t, mq);
            const uint32_t p = keyed ? (uint32_t)cur.pt[j] : 0u;
            const bool placed = keyed && mod_u31(t, mp) == p;
            const uint32_t bytes = (uint32_t)cur.kl[j] + (uint32_t)max(cur_vl[j], 0);   // below 2^32
            n_keyed += (uint32_t)__popcll(__ballot(keyed));

            // checked / placed: the lanes of the first keyed lane's partition add as one, kPartCombine times; the others alone
            bool todo = keyed;
            uint32_t wc = 0, wp = 0;
#pragma unroll
            for (int g = 0; g < kPartCombine; g++) {
                const unsigned long long m = __ballot(todo);
                if (m == 0ull) break;
                const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
                const uint32_t lp = (uint32_t)__builtin_amdgcn_readlane((int)p, leader);
                const bool same = todo && p == lp;
                const uint32_t sc = (uint32_t)__popcll(__ballot(same)), sp = (uint32_t)__popcll(__ballot(same && placed));
                if ((int)lane == leader) wc = sc, wp = sp;
                todo = todo && !same;
            }
            if (todo) wc = 1u, wp = placed ? 1u : 0u;
            n_padd += (uint32_t)__popcll(__ballot(wc != 0u));
            if (wc) atomicAdd(s_part + ((p << rep_p_log2) | rep_p), ((unsigned long long)wp << 32) | wc);

            // the target: likewise on t % Q; a group's bytes are summed across the wave when it is worth an add
            todo = keyed;
            uint32_t wr = 0;
            unsigned long long wb = 0ull;
#pragma unroll
            for (int g = 0; g < kPartCombine; g++) {
                const unsigned long long m = __ballot(todo);
                if (m == 0ull) break;
                const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
                const uint32_t lq = (uint32_t)__builtin_amdgcn_readlane((int)q, leader);
                const bool same = todo && q == lq;
                const uint32_t size = (uint32_t)__popcll(__ballot(same));
                if (size >= kPartGroupMin) {
                    unsigned long long s = same ? (unsigned long long)bytes : 0ull;
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
                    if ((int)lane == leader) wr = size, wb = s;
                } else if (same) {
                    wr = 1u, wb = bytes;
                }
                todo = todo && !same;
            }
            if (todo) wr = 1u, wb = bytes;
            n_qadd += (uint32_t)__popcll(__ballot(wr != 0u));
            if (wr) {
                const uint32_t e = (q << rep_q_log2) | rep_q;
                atomicAdd(s_bytes + e, wb);
                atomicAdd(s_recs + e, wr);
            }
        }
        cur = nxt;
#pragma unroll
        for (int j = 0; j < 4; j++) cur_vl[j] = nxt_vl[j];
        step = next;
    }
    if (lane == 0) {
        atomicAdd(&s_stat[0], (unsigned long long)n_keyed);
        atomicAdd(&s_stat[1], (unsigned long long)n_padd);
        atomicAdd(&s_stat[2], (unsigned long long)n_qadd);
    }
    __syncthreads();
    // the workgroup's sums over the replicas, the non-zero ones to the accumulator u64[2 P + 2 Q]
    for (uint32_t p = threadIdx.x; p < P; p += THREADS) {
        unsigned long long checked = 0ull, placed = 0ull;
        for (uint32_t r = 0; r < (1u << rep_p_log2); r++) {
            const unsigned long long v = s_part[(p << rep_p_log2) + r];
            checked += v & 0xFFFFFFFFull, placed += v >> 32;
        }
        if (checked) atomicAdd(acc + 2u * (size_t)p, checked);
        if (placed) atomicAdd(acc + 2u * (size_t)p + 1u, placed);
    }
    for (uint32_t q = threadIdx.x; q < Q; q += THREADS) {
        unsigned long long recs = 0ull, bytes = 0ull;
        for (uint32_t r = 0; r < (1u << rep_q_log2); r++) {
            recs += s_recs[(q << rep_q_log2) + r];
            bytes += s_bytes[(q << rep_q_log2) + r];
        }
        if (recs) atomicAdd(acc + 2u * (size_t)P + 2u * (size_t)q, recs);
        if (bytes) atomicAdd(acc + 2u * (size_t)P + 2u * (size_t)q + 1u, bytes);
    }
    if (threadIdx.x < 3 && s_stat[threadIdx.x]) atomicAdd(stats + threadIdx.x, s_stat[threadIdx.x]);
}

} // namespace

void partitioner_lds_plan(uint32_t P, uint32_t Q, uint32_t out[3])
{
    const PartitionerPlan pl = plan_partitioner(P, Q);
    out[0] = pl.lds_bytes, out[1] = pl.threads, out[2] = pl.wg_per_cu;
}

hipError_t launch_partitioner(const PartitionerColumns &c, uint64_t n, uint32_t P, uint32_t Q, uint64_t *acc, uint64_t *stats,
                              int cu_count, uint32_t *workgroups, hipStream_t s)
{
    *workgroups = 0;
    if (n == 0) return hipSuccess;
    if (n > kPartitionerLaunchMax || P == 0 || Q == 0 || P > kPartitionerMaxPartitions || Q > kPartitionerMaxPartitions)
        return hipErrorInvalidValue;
    const PartitionerPlan pl = plan_partitioner(P, Q);
    const uint32_t wg_waves = pl.threads / 64;
    const uint64_t steps = (n + kPartStep - 1) / kPartStep;
    const uint64_t want = (steps + wg_waves - 1) / wg_waves;
    const uint64_t cap = (uint64_t)(cu_count > 0 ? cu_count : 256) * pl.wg_per_cu;
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    const ModU31 mp = mod_u31_make(P), mq = mod_u31_make(Q);
    unsigned long long *a = reinterpret_cast<unsigned long long *>(acc), *st = reinterpret_cast<unsigned long long *>(stats);
    if (pl.threads == 256) {
        hipLaunchKernelGGL(kta_partitioner<256>, dim3(grid), dim3(256), pl.lds_bytes, s, c, n, mp, mq, pl.rep_p_log2, pl.rep_q_log2, a, st);
    } else {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&kta_partitioner<1024>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kta_partitioner<1024>, dim3(grid), dim3(1024), pl.lds_bytes, s, c, n, mp, mq, pl.rep_p_log2, pl.rep_q_log2, a, st);
    }
    *workgroups = grid;
    return hipGetLastError();
}

} // namespace kta

// kta_compaction.hip — the compaction what-if (KTA_FLAG_COMPACTION, include/kta_hip.h): a replay of the records the first
// pass was handed against the last-writer table it left, which adds up per partition the records and bytes that log
// compaction would keep — sums only, exact.  The rule is kta_compaction.h's.  No reference counterpart.
//
//   kta_compaction_survivors   streams partition (u16 in compact tiles), key_len, key_off, val_len, the seq column where
//                     the batch has one and the key bytes once, as kta_partitioner does (256-record wave steps,
//                     non-temporal column loads one step ahead, the unconditional 16-byte key prefetch, four interleaved
//                     FNV chains when the wave holds 16-byte keys: kta_key_stream.h).  What is new is one random 8-byte
//                     read per keyed record from the 32 GiB table, a 64-byte line nothing else in the wave shares.  It is
//                     pipelined one step deep: the four slot loads of a step are issued as soon as its hashes exist and
//                     classified in the next iteration, behind the next step's key prefetch, column loads and hashing — a
//                     wave always has four random loads per lane in flight.  No load sits behind a branch: key None
//                     reads slot 0 and discards it.
//                     Only survivors accumulate, in LDS, 32 B per partition (kta_compaction.h): W0 one ds_add_u64 for
//                     live | tombstones << 32, W1 / W2 the live key and value bytes, W3 the tombstones' key bytes.  A word
//                     has 2^r replicas, chosen by the lane, while the array stays within 16 KiB.  A launch takes at most
//                     2^30 records, so no half of W0 overflows and nothing is flushed before the end: there the workgroup
//                     sums the replicas and adds the non-zero words to the live u64 vector.  The globals are popcounts
//                     of ballots, kept per wave in scalar registers.
#include "kta_compact_delete.h"
#include "kta_compaction.h"
#include "kta_key_stream.h"

namespace kta {

namespace {

constexpr uint32_t kCompStep = 256;              // records of one wave step: instruction j of it takes the records 64 j + lane
constexpr uint32_t kCompRepMax = 5;              // log2 of the most replicas of a word: the 32 lanes of a bank group
constexpr uint32_t kCompSmallLds = 16384;        // the words are replicated while they stay within this: 256 threads
constexpr uint32_t kCompCuLds = 160u * 1024u;
constexpr uint32_t kCompStaticLds = 64;          // s_glob, rounded up
constexpr uint32_t kCompPartBytes = kCompactionLdsWords * 8u;
constexpr uint32_t kCompStats = 2;               // keyed records looked at, LDS adds

struct CompactionPlan {
    uint32_t rep_log2;
    uint32_t lds_bytes;
    uint32_t threads;      // 256, or 1024 when the words are more than kCompSmallLds
    uint32_t wg_per_cu;
};

CompactionPlan plan_compaction(uint32_t P)
{
    CompactionPlan pl{};
    while (pl.rep_log2 < kCompRepMax && ((uint64_t)P * kCompPartBytes << (pl.rep_log2 + 1)) <= kCompSmallLds) pl.rep_log2++;
    pl.lds_bytes = P * kCompPartBytes << pl.rep_log2;
    if (pl.lds_bytes <= kCompSmallLds) {
        pl.threads = 256, pl.wg_per_cu = 4;      // 16 waves per CU: the kernel takes under 128 vector registers, four waves per SIMD
    } else {
        pl.threads = 1024;                        // 16 waves share the words; two workgroups where two fit
        pl.wg_per_cu = 2u * (pl.lds_bytes + kCompStaticLds) <= kCompCuLds ? 2 : 1;
    }
    return pl;
}

// val_len and the sequence numbers of the records load_keyed_cols takes for this step: the same clamped indices, unconditional
__device__ __forceinline__ void load_val_seq4(const CompactionColumns &c, const uint64_t &base_seq, const uint64_t &step, const uint64_t &nsteps,
                                              const uint64_t &n, const uint32_t &lane, int32_t (&vl)[4], uint64_t (&sq)[4])
{
    const bool ok = step < nsteps;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint64_t i = step * kCompStep + 64u * j + lane;
        const uint64_t ic = ok && i < n ? i : n - 1;
        vl[j] = __builtin_nontemporal_load(c.val_len + ic);
        sq[j] = c.seq ? __builtin_nontemporal_load(c.seq + ic) : base_seq + ic;   // (uniform)
    }
}

// A step whose slot loads are in flight: what its classification needs.
struct PendingStep {
    uint64_t entry[4];     // table[h]
    uint64_t sq[4];
    int32_t kl[4];         // -1: key None, or no record
    int32_t vl[4];
    int32_t pt[4];
    uint32_t in;           // bit j: record 64 j + lane of the step lies in the batch
};
// (CLASS: with the step's first record)
template <bool CLASS> struct PendingStepOf : PendingStep {};
template <> struct PendingStepOf<true> : PendingStep {
    uint64_t at;
};

// The kernel's text.  CLASS: every record's class byte (kta_compact_delete.h: 0 not kept, 1 live, 2 tombstone kept) goes to
// cls[record], one plain byte store where the record is classified — what the kept-row kernels of the compact,delete
// what-if read (kta_segments.hip).  Without it nothing of cls is looked at and the text is the one the kernel always had.
template <int THREADS, bool CLASS>
__device__ __forceinline__ void compaction_survivors(CompactionColumns c, uint64_t n, uint64_t base_seq, uint32_t P, uint32_t rep_log2,
                                                     const unsigned long long *__restrict__ table, unsigned long long *acc,
                                                     unsigned long long *stats, uint8_t *__restrict__ cls)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_part[];    // [P << rep][4]
    __shared__ unsigned long long s_glob[kCompactionGlobals + kCompStats];
    const uint32_t n_words = (P << rep_log2) * kCompactionLdsWords;
    for (uint32_t e = threadIdx.x; e < n_words; e += THREADS) s_part[e] = 0ull;
    if (threadIdx.x < kCompactionGlobals + kCompStats) s_glob[threadIdx.x] = 0ull;
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t rep = lane & ((1u << rep_log2) - 1u);
    const uint64_t nsteps = (n + kCompStep - 1) / kCompStep;
    const uint64_t waves = (uint64_t)gridDim.x * (THREADS / 64);
    uint64_t step = (uint64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    // (wave-uniform: popcounts of ballots)
    uint32_t n_replayed = 0, n_unkeyed = 0, n_unknown = 0, n_live_out = 0, n_tomb_out = 0, n_keyed = 0, n_adds = 0;

    // the step whose slot loads were issued an iteration ago: its classes, its survivors into LDS
    auto settle = [&](const PendingStepOf<CLASS> &pd) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool in = (pd.in >> j) & 1u;
            const CompactionClass k = compaction_classify(pd.entry[j], pd.sq[j], pd.kl[j], pd.vl[j], pd.pt[j], P);
            if constexpr (CLASS)
                if (in) cls[pd.at + 64u * j + lane] = kept_class_byte(k);
            n_replayed += (uint32_t)__popcll(__ballot(in));
            n_unkeyed += (uint32_t)__popcll(__ballot(in && k == kCompactionUnkeyed));
            n_unknown += (uint32_t)__popcll(__ballot(in && k == kCompactionUnknown));
            n_live_out += (uint32_t)__popcll(__ballot(in && k == kCompactionLiveOutside));
            n_tomb_out += (uint32_t)__popcll(__ballot(in && k == kCompactionTombstoneOutside));
            n_keyed += (uint32_t)__popcll(__ballot(in && k != kCompactionUnkeyed));
            const bool live = in && k == kCompactionLive, tomb = in && k == kCompactionTombstone;
            const unsigned long long kept = __ballot(live || tomb);
            if (kept == 0ull) continue;              // (uniform) typically most instructions of a compacted topic's replay
            n_adds += 3u * (uint32_t)__popcll(__ballot(live)) + 2u * (uint32_t)__popcll(__ballot(tomb));
            if (live || tomb) {
                unsigned long long *w = s_part + ((((uint32_t)pd.pt[j] << rep_log2) | rep) * kCompactionLdsWords);
                atomicAdd(w, (unsigned long long)compaction_w0(live));
                if (live) {
                    atomicAdd(w + 1, (unsigned long long)(uint32_t)pd.kl[j]);
                    atomicAdd(w + 2, (unsigned long long)(uint32_t)pd.vl[j]);
                } else {
                    atomicAdd(w + 3, (unsigned long long)(uint32_t)pd.kl[j]);
                }
            }
        }
    };

    KeyedCols cur;
    int32_t cur_vl[4];
    uint64_t cur_sq[4];
    load_keyed_cols<kCompStep>(c.k, step, nsteps, n, lane, cur);
    load_val_seq4(c, base_seq, step, nsteps, n, lane, cur_vl, cur_sq);
    PendingStepOf<CLASS> pd;
    bool pending = false;                            // (uniform)
    while (step < nsteps) {
        uint4 keys[4];
        prefetch_keys4<false>(c.k.key_bytes, cur.kl, cur.ko, keys);
        const uint64_t next = step + waves;
        KeyedCols nxt;
        int32_t nxt_vl[4];
        uint64_t nxt_sq[4];
        load_keyed_cols<kCompStep>(c.k, next, nsteps, n, lane, nxt);
        load_val_seq4(c, base_seq, next, nsteps, n, lane, nxt_vl, nxt_sq);
        uint32_t h[4];
        hash_keys4(h, keys, c.k.key_bytes, cur.kl, cur.ko);
        // this step's slots, requested now and looked at in the next iteration (key None: slot 0, discarded)
        PendingStepOf<CLASS> now;
        now.in = 0u;
        if constexpr (CLASS) now.at = step * kCompStep;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            now.entry[j] = table[cur.kl[j] >= 0 ? h[j] : 0u];
            now.sq[j] = cur_sq[j], now.kl[j] = cur.kl[j], now.vl[j] = cur_vl[j], now.pt[j] = cur.pt[j];
            now.in |= (step * kCompStep + 64u * j + lane < n ? 1u : 0u) << j;
        }
        if (pending) settle(pd);
        pd = now;
        pending = true;
        cur = nxt;
#pragma unroll
        for (int j = 0; j < 4; j++) cur_vl[j] = nxt_vl[j], cur_sq[j] = nxt_sq[j];
        step = next;
    }
    if (pending) settle(pd);
    if (lane == 0) {
        atomicAdd(&s_glob[kCompactionReplayed], (unsigned long long)n_replayed);
        atomicAdd(&s_glob[kCompactionUnkeyedRecords], (unsigned long long)n_unkeyed);
        atomicAdd(&s_glob[kCompactionUnknownRecords], (unsigned long long)n_unknown);
        atomicAdd(&s_glob[kCompactionLiveOutsideRecords], (unsigned long long)n_live_out);
        atomicAdd(&s_glob[kCompactionTombstonesOutsideRecords], (unsigned long long)n_tomb_out);
        atomicAdd(&s_glob[kCompactionGlobals], (unsigned long long)n_keyed);
        atomicAdd(&s_glob[kCompactionGlobals + 1], (unsigned long long)n_adds);
    }
    __syncthreads();
    // the workgroup's sums over the replicas, the non-zero ones to the vector u64[5 P + 6]
    for (uint32_t p = threadIdx.x; p < P; p += THREADS) {
        unsigned long long w0_live = 0ull, w0_tomb = 0ull, w1 = 0ull, w2 = 0ull, w3 = 0ull;
        for (uint32_t r = 0; r < (1u << rep_log2); r++) {
            const unsigned long long *w = s_part + (((p << rep_log2) + r) * kCompactionLdsWords);
            w0_live += compaction_w0_live(w[0]), w0_tomb += compaction_w0_tombstones(w[0]);
            w1 += w[1], w2 += w[2], w3 += w[3];
        }
        unsigned long long *o = acc + (size_t)kCompactionWords * p;
        if (w0_live) atomicAdd(o + kCompactionLiveRecords, w0_live);
        if (w1) atomicAdd(o + kCompactionLiveKeyBytes, w1);
        if (w2) atomicAdd(o + kCompactionLiveValueBytes, w2);
        if (w0_tomb) atomicAdd(o + kCompactionTombstoneRecords, w0_tomb);
        if (w3) atomicAdd(o + kCompactionTombstoneKeyBytes, w3);
    }
    if (threadIdx.x < kCompactionGlobals && s_glob[threadIdx.x]) atomicAdd(acc + (size_t)kCompactionWords * P + threadIdx.x, s_glob[threadIdx.x]);
    if (threadIdx.x < kCompStats && s_glob[kCompactionGlobals + threadIdx.x]) atomicAdd(stats + threadIdx.x, s_glob[kCompactionGlobals + threadIdx.x]);
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void kta_compaction_survivors(CompactionColumns c, uint64_t n, uint64_t base_seq, uint32_t P, uint32_t rep_log2,
                                                                    const unsigned long long *__restrict__ table, unsigned long long *acc,
                                                                    unsigned long long *stats)
{
    compaction_survivors<THREADS, false>(c, n, base_seq, P, rep_log2, table, acc, stats, nullptr);
}

// the same with the class column (cls: u8[n], every byte written)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void kta_compaction_survivors_class(CompactionColumns c, uint64_t n, uint64_t base_seq, uint32_t P,
                                                                          uint32_t rep_log2, const unsigned long long *__restrict__ table,
                                                                          unsigned long long *acc, unsigned long long *stats, uint8_t *__restrict__ cls)
{
    compaction_survivors<THREADS, true>(c, n, base_seq, P, rep_log2, table, acc, stats, cls);
}

} // namespace

void compaction_lds_plan(uint32_t P, uint32_t out[3])
{
    const CompactionPlan pl = plan_compaction(P);
    out[0] = pl.lds_bytes, out[1] = pl.threads, out[2] = pl.wg_per_cu;
}

hipError_t launch_compaction(const CompactionColumns &c, uint64_t n, uint64_t base_seq, uint32_t P, const uint64_t *table, uint64_t *acc,
                             uint64_t *stats, int cu_count, uint32_t *workgroups, hipStream_t s, uint8_t *cls)
{
    *workgroups = 0;
    if (n == 0) return hipSuccess;
    if (n > kCompactionLaunchMax || P == 0 || P > kCompactionMaxPartitions || !table) return hipErrorInvalidValue;
    const CompactionPlan pl = plan_compaction(P);
    const uint32_t wg_waves = pl.threads / 64;
    const uint64_t steps = (n + kCompStep - 1) / kCompStep;
    const uint64_t want = (steps + wg_waves - 1) / wg_waves;
    const uint64_t cap = (uint64_t)(cu_count > 0 ? cu_count : 256) * pl.wg_per_cu;
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    const unsigned long long *t = reinterpret_cast<const unsigned long long *>(table);
    unsigned long long *a = reinterpret_cast<unsigned long long *>(acc), *st = reinterpret_cast<unsigned long long *>(stats);
    if (cls) {
        if (pl.threads == 256) {
            hipLaunchKernelGGL(kta_compaction_survivors_class<256>, dim3(grid), dim3(256), pl.lds_bytes, s, c, n, base_seq, P, pl.rep_log2, t, a, st, cls);
        } else {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&kta_compaction_survivors_class<1024>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(kta_compaction_survivors_class<1024>, dim3(grid), dim3(1024), pl.lds_bytes, s, c, n, base_seq, P, pl.rep_log2, t, a, st,
                               cls);
        }
    } else if (pl.threads == 256) {
        hipLaunchKernelGGL(kta_compaction_survivors<256>, dim3(grid), dim3(256), pl.lds_bytes, s, c, n, base_seq, P, pl.rep_log2, t, a, st);
    } else {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&kta_compaction_survivors<1024>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kta_compaction_survivors<1024>, dim3(grid), dim3(1024), pl.lds_bytes, s, c, n, base_seq, P, pl.rep_log2, t, a, st);
    }
    *workgroups = grid;
    return hipGetLastError();
}

} // namespace kta

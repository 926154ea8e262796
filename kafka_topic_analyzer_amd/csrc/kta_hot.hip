// kta_hot.hip — the opt-in hot-key sketch (KTA_FLAG_HOT_KEYS, include/kta_hip.h): two rows of 1024 cells, each a total and
// 22 bit counters, over x = fmix32(fnv(key)) of every keyed record — sums only, so the vector is exact whatever the order,
// the batching or the sharding; the heavy keys are read out of it on the host (kta_hot_keys_recover).  No reference
// counterpart.
//
//   kta_hot_keys        streams partition (u16 in compact tiles), key_len, key_off and the key bytes once, as kta_key_sketch
//                       does (256-record wave steps, non-temporal column loads one step ahead, the unconditional 16-byte
//                       key prefetch, fnv_16x4 when the wave holds 16-byte keys), and accumulates in LDS: a cell is 23
//                       counts in 21-bit fields, three to a u64 word, so a record is 16 ds_add_u64 (a word whose three
//                       bits are clear is skipped) and both rows are 128 KiB.  The words lie [row][word][cell], so that the
//                       lanes of an instruction, which differ in their cells, spread over the banks.  One workgroup of 16
//                       waves per CU (the LDS admits one); its waves take one step per round, 4096 records of the
//                       workgroup, and after flush_rounds rounds (at most 511: 511 * 4096 < 2^21, counted in records, so a
//                       combined add of 64 counts 64) the workgroup adds its non-zero fields to the live u64 accumulator
//                       and clears them; once more at the end.
//                       Lanes of equal x are combined before the adds: the first keyed lane's group adds once with its
//                       size, kHotCombine times over, and what is left adds alone.  One hot key is then one add per 64
//                       records and word, two keys alternating lane by lane two.
//                       Exemplars: a record whose x is its cell's marked candidate (LDS copies of want / mark) clears the
//                       mark for its workgroup, claims the slot with one compare-and-swap and writes its key — one writer
//                       per slot and launch.
//   kta_hot_candidates  before every launch: every cell's candidate x from the live accumulator (the bits set in more than
//                       half of the cell's records), marked when the cell's slot does not hold it; clears the claims.
#include "kta_key_stream.h"

#include <algorithm>

namespace kta {

namespace {

constexpr int kHotThreads = 1024;
constexpr int kHotWaves = kHotThreads / 64;
constexpr uint32_t kHotStep = 256;               // records of one wave step: instruction j of it takes the records 64 j + lane
constexpr uint32_t kHotRound = kHotWaves * kHotStep;   // records of a workgroup's round
constexpr uint32_t kHotFieldBits = 21;
constexpr uint32_t kHotFieldMask = (1u << kHotFieldBits) - 1u;
constexpr uint32_t kHotCellWords = 8;            // 23 fields, three to a word
constexpr uint32_t kHotSlots = KTA_HOT_ROWS * KTA_HOT_CELLS;
constexpr uint32_t kHotLdsWords = kHotSlots * kHotCellWords;
constexpr int kHotCombine = 2;                   // groups of equal x combined per instruction
static_assert(kHotFlushRoundsMax * kHotRound <= kHotFieldMask, "a field holds the records of a flush period");
static_assert(kHotLdsBytes == kHotLdsWords * 8 + kHotSlots * 4 + kHotSlots / 8, "counters, want, mark");

__global__ __launch_bounds__(kHotThreads) void kta_hot_keys(SketchColumns c, uint64_t n, uint32_t P, unsigned long long *acc,
                                                            const uint32_t *__restrict__ want, const uint32_t *__restrict__ mark,
                                                            uint32_t *claim, kta_hot_exemplar *slots, uint32_t flush_rounds,
                                                            unsigned long long *stats)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_cnt[];   // [row][word][cell]
    uint32_t *s_want = reinterpret_cast<uint32_t *>(s_cnt + kHotLdsWords);       // [row][cell]
    uint32_t *s_mark = s_want + kHotSlots;                                         // a bit per [row][cell]
    __shared__ unsigned long long s_stat[4];
    for (uint32_t e = threadIdx.x; e < kHotLdsWords; e += kHotThreads) s_cnt[e] = 0ull;
    for (uint32_t e = threadIdx.x; e < kHotSlots; e += kHotThreads) s_want[e] = want[e];
    if (threadIdx.x < kHotSlots / 32) s_mark[threadIdx.x] = mark[threadIdx.x];
    if (threadIdx.x < 4) s_stat[threadIdx.x] = 0ull;
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nsteps = (n + kHotStep - 1) / kHotStep;
    const uint64_t per_round = (uint64_t)gridDim.x * kHotWaves;
    const uint64_t rounds = (nsteps + per_round - 1) / per_round;   // the same for every wave of the grid
    uint64_t step = (uint64_t)blockIdx.x * kHotWaves + (threadIdx.x >> 6);
    uint32_t n_keyed = 0, n_groups = 0, n_flush = 0, n_claim = 0;   // (wave-uniform but n_claim)

    // the workgroup's non-zero fields to the accumulator (between two barriers)
    auto flush = [&]() __attribute__((always_inline)) {
        for (uint32_t e = threadIdx.x; e < kHotLdsWords; e += kHotThreads) {
            const unsigned long long v = s_cnt[e];
            if (v == 0ull) continue;
            s_cnt[e] = 0ull;
            const uint32_t row = e / (kHotCellWords * KTA_HOT_CELLS), word = (e / KTA_HOT_CELLS) % kHotCellWords, cell = e % KTA_HOT_CELLS;
            unsigned long long *a = acc + ((size_t)row * KTA_HOT_CELLS + cell) * KTA_HOT_WORDS;
#pragma unroll
            for (uint32_t f = 0; f < 3; f++) {
                const unsigned long long cnt = (v >> (kHotFieldBits * f)) & kHotFieldMask;
                if (cnt && 3u * word + f < KTA_HOT_WORDS) atomicAdd(a + 3u * word + f, cnt);
            }
        }
    };

    // weight w of this lane's x into its cell of `row`: the total and the set bits of y, three fields to a word
    auto add_row = [&](uint32_t row, uint32_t cell, uint32_t y, uint32_t w) __attribute__((always_inline)) {
        const uint32_t fields = 1u | (y << 1);   // bit 0: the total; bit 1 + b: bit b of y
        unsigned long long *base = s_cnt + (size_t)row * kHotCellWords * KTA_HOT_CELLS + cell;
#pragma unroll
        for (uint32_t k = 0; k < kHotCellWords; k++) {
            const uint32_t v = (fields >> (3u * k)) & 7u;
            const uint32_t lo = w * ((v & 1u) | ((v & 2u) << 20));   // the fields at bits 0 and 21
            const uint32_t hi = w * ((v & 4u) << 8);                 // the field at bit 42
            if (v) atomicAdd(base + (size_t)k * KTA_HOT_CELLS, ((unsigned long long)hi << 32) | lo);
        }
    };

    KeyedCols cur;
    load_keyed_cols<kHotStep>(c, step, nsteps, n, lane, cur);
    for (uint64_t round = 0; round < rounds; round++) {
        if (round != 0 && round % flush_rounds == 0) {
            __syncthreads();
            flush();
            __syncthreads();
            n_flush++;
        }
        uint4 keys[4];
        prefetch_keys4<false>(c.key_bytes, cur.kl, cur.ko, keys);
        const uint64_t next = step + per_round;
        KeyedCols nxt;
        load_keyed_cols<kHotStep>(c, next, nsteps, n, lane, nxt);
        uint32_t h[4];
        hash_keys4(h, keys, c.key_bytes, cur.kl, cur.ko);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            // key Some (the empty key included) in a partition the metrics handler counts
            const bool keyed = cur.kl[j] >= 0 && (uint32_t)cur.pt[j] < P;
            const uint32_t x = fmix32(h[j]);
            const uint32_t c0 = x & (KTA_HOT_CELLS - 1u), c1 = (x >> 10) & (KTA_HOT_CELLS - 1u);
            n_keyed += (uint32_t)__popcll(__ballot(keyed));
            // the lanes of the first keyed lane's x add as one, kHotCombine times; the others each alone
            bool todo = keyed;
            uint32_t w = 0;
#pragma unroll
            for (int g = 0; g < kHotCombine; g++) {
                const unsigned long long m = __ballot(todo);
                if (m == 0ull) break;
                const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
                const uint32_t lx = (uint32_t)__builtin_amdgcn_readlane((int)x, leader);
                const bool same = todo && x == lx;
                const uint32_t size = (uint32_t)__popcll(__ballot(same));
                if ((int)lane == leader) w = size;
                todo = todo && !same;
            }
            if (todo) w = 1u;
            n_groups += (uint32_t)__popcll(__ballot(w != 0u));
            if (w) {
                add_row(0u, c0, x >> 10, w);
                add_row(1u, c1, c0 | ((x >> 20) << 10), w);
            }
            // exemplars: the record's x is the marked candidate of one of its cells
            const uint32_t i0 = c0, i1 = KTA_HOT_CELLS + c1;
            const bool m0 = keyed && s_want[i0] == x && ((s_mark[i0 >> 5] >> (i0 & 31u)) & 1u);
            const bool m1 = keyed && s_want[i1] == x && ((s_mark[i1 >> 5] >> (i1 & 31u)) & 1u);
            if (m0 || m1) {
#pragma unroll
                for (int r = 0; r < 2; r++) {
                    if (!(r ? m1 : m0)) continue;
                    const uint32_t i = r ? i1 : i0, bit = 1u << (i & 31u);
                    // the lane that clears the workgroup's mark tries for the slot; the first of the grid writes it
                    if (!(atomicAnd(&s_mark[i >> 5], ~bit) & bit)) continue;
                    if (atomicCAS(claim + i, 0u, 1u) != 0u) continue;
                    kta_hot_exemplar *s = slots + i;
                    const uint32_t kl = (uint32_t)cur.kl[j];
                    const uint8_t *kb = c.key_bytes + (kl ? cur.ko[j] : 0u);
                    for (uint32_t b = 0; b < KTA_HOT_EXEMPLAR_BYTES; b++) s->bytes[b] = b < kl ? kb[b] : (uint8_t)0;
                    s->hash = h[j];
                    s->key_len = kl;
                    s->pad = 0u;
                    s->valid = 1u;
                    n_claim++;
                }
            }
        }
        cur = nxt;
        step = next;
    }
    __syncthreads();
    flush();
    if (lane == 0) {
        atomicAdd(&s_stat[0], (unsigned long long)n_keyed);
        atomicAdd(&s_stat[1], (unsigned long long)n_groups);
    }
    if (threadIdx.x == 0) s_stat[2] = n_flush;
    if (n_claim) atomicAdd(&s_stat[3], (unsigned long long)n_claim);
    __syncthreads();
    if (threadIdx.x < 4 && s_stat[threadIdx.x]) atomicAdd(stats + threadIdx.x, s_stat[threadIdx.x]);
}

__global__ __launch_bounds__(256) void kta_hot_candidates(const unsigned long long *__restrict__ acc,
                                                          const kta_hot_exemplar *__restrict__ slots, uint32_t *__restrict__ want,
                                                          uint32_t *__restrict__ mark, uint32_t *__restrict__ claim)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;   // the grid is exactly the slots
    const uint32_t row = i / KTA_HOT_CELLS, cell = i % KTA_HOT_CELLS;
    const unsigned long long *a = acc + (size_t)i * KTA_HOT_WORDS;
    const unsigned long long T = a[0];
    uint32_t y = 0;
    for (uint32_t b = 0; b < KTA_HOT_WORDS - 1u; b++)
        if (2ull * a[1 + b] > T) y |= 1u << b;
    const uint32_t x = row == 0u ? (cell | (y << 10)) : ((y & (KTA_HOT_CELLS - 1u)) | (cell << 10) | ((y >> 10) << 20));
    const bool marked = T != 0ull && !(slots[i].valid && fmix32(slots[i].hash) == x);
    want[i] = x;
    claim[i] = 0u;
    const unsigned long long m = __ballot(marked);
    if ((threadIdx.x & 63u) == 0u) {
        mark[(i >> 6) * 2u] = (uint32_t)m;
        mark[(i >> 6) * 2u + 1u] = (uint32_t)(m >> 32);
    }
}

} // namespace

hipError_t launch_hot_keys(const SketchColumns &c, uint64_t n, uint32_t P, const HotState &st, uint32_t flush_rounds, int cu_count,
                           uint32_t *workgroups, hipStream_t s)
{
    *workgroups = 0;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(kta_hot_candidates, dim3(kHotSlots / 256), dim3(256), 0, s, reinterpret_cast<const unsigned long long *>(st.acc),
                       st.slots, st.want, st.mark, st.claim);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(&kta_hot_keys), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHotLdsBytes);
    if (e != hipSuccess) return e;
    const uint64_t steps = (n + kHotStep - 1) / kHotStep;
    const uint64_t want = (steps + kHotWaves - 1) / kHotWaves;
    const uint64_t cap = (uint64_t)(cu_count > 0 ? cu_count : 256);   // one workgroup's LDS fills a CU
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    const uint32_t fr = flush_rounds == 0u || flush_rounds > kHotFlushRoundsMax ? kHotFlushRoundsMax : flush_rounds;
    hipLaunchKernelGGL(kta_hot_keys, dim3(grid), dim3(kHotThreads), kHotLdsBytes, s, c, n, P, reinterpret_cast<unsigned long long *>(st.acc),
                       st.want, st.mark, st.claim, st.slots, fr, reinterpret_cast<unsigned long long *>(st.stats));
    *workgroups = grid;
    return hipGetLastError();
}

} // namespace kta

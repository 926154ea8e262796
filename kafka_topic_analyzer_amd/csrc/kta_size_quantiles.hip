// kta_size_quantiles.hip — the opt-in size percentiles (KTA_FLAG_SIZE_QUANTILES, include/kta_hip.h): per partition a
// histogram of 464 bins each of the key sizes, the value sizes and the message sizes — sums only, so the vector is exact
// whatever the order, the batching or the sharding.  The bin rule is kta_size_bins.h's.  No reference counterpart.
//
//   kta_size_quantiles   P * 3 * 464 counters are 1.4 MiB of u32 at 256 partitions: no workgroup's LDS holds them, and
//                     device-scope atomics on random slots run at 18-27 G/s.  So a workgroup keeps
//                     u32[S][3][464] in LDS (5568 B per partition) for a SLICE of S consecutive partitions, streams the
//                     whole batch and bins only the records whose partition lies in its slice; ceil(P / S) slices cover
//                     the topic.  The slice is the grid's second dimension: the workgroups of all slices walk the same
//                     tiles at about the same time, so what one slice's workgroups pulled into the L2 and the MALL the
//                     others find there (variant 1, a diagnostic: one launch per slice instead).
//                     A wave step is a quarter tile, 256 records: lane l takes the four consecutive records 4 l .. 4 l + 3
//                     of it with the tile's own forms, as kta_filter.hip's tile copy does — 8 B of u16 partitions and one
//                     16-byte group of u16 lengths in a keyless batch's tiles (6 B per record, nothing is widened), or
//                     16 B each of the plain i32 columns.  No key columns, no timestamps.
//                     Lanes of one instruction that share a word (partition, quantity, bin) are combined first: the first
//                     lane's group adds once, what is left adds alone.  A run of equal records is one add per instruction
//                     and word, not 64 on one LDS word.
//                     A launch takes at most 2^30 records, so no u32 counter overflows and nothing is flushed before the
//                     end: there the workgroup adds its non-zero counters to the live u64 vector.  The four globals are
//                     popcounts of ballots, counted by slice 0 alone (every slice sees every record).
#include "kta_kernels.h"
#include "kta_size_bins.h"

namespace kta {

namespace {

typedef int qv4i __attribute__((ext_vector_type(4)));
typedef int qv2i __attribute__((ext_vector_type(2)));

constexpr uint32_t kSizeqStep = 256;                       // records of one wave step: a quarter tile
static_assert(KTA_TILE_RECORDS % kSizeqStep == 0, "a wave step lies in one tile");
constexpr uint32_t kSizeqPartBytes = kSizePartitionWords * 4u;   // 5568 B of LDS per partition of the slice
constexpr uint32_t kSizeqCuLds = 160u * 1024u;
constexpr uint32_t kSizeqStaticLds = 64;                   // s_stat
constexpr uint32_t kSizeqSmallSlice = 7;                   // up to here (38 976 B): 256 threads, four workgroups per CU
constexpr uint32_t kSizeqStats = 5;                        // records, bad, keyed, alive, LDS adds

struct SizeqPlan {
    uint32_t slice;        // S: partitions of a slice
    uint32_t slices;       // ceil(P / S)
    uint32_t lds_bytes;
    uint32_t threads;      // 256, or 1024 when the slice is larger than kSizeqSmallSlice
    uint32_t wg_per_cu;
};

// S, the threads and the workgroups per CU, in one place.  A topic of up to kSizeQuantilesMaxSlice partitions is ONE slice
// (the common case: a dozen partitions); a larger one takes slices of kSizeQuantilesMaxSlice, the last one partial.  A
// small slice runs 256 threads, four workgroups per CU; a larger one 1024 threads — 16 waves share the counters —, two
// workgroups per CU where two fit (S <= 14), else one.  forced: the tests' S (0: the plan's).
SizeqPlan plan_size_quantiles(uint32_t P, uint32_t forced)
{
    SizeqPlan pl{};
    pl.slice = forced ? forced : kSizeQuantilesMaxSlice;
    if (pl.slice > kSizeQuantilesMaxSlice) pl.slice = kSizeQuantilesMaxSlice;
    if (pl.slice > P) pl.slice = P;
    pl.slices = (P + pl.slice - 1) / pl.slice;
    pl.lds_bytes = pl.slice * kSizeqPartBytes;
    if (pl.slice <= kSizeqSmallSlice) {
        pl.threads = 256, pl.wg_per_cu = 4;
    } else {
        pl.threads = 1024;
        pl.wg_per_cu = 2u * (pl.lds_bytes + kSizeqStaticLds) <= kSizeqCuLds ? 2 : 1;
    }
    return pl;
}

// One quantity of one instruction: lanes with `on` add 1 to word w of the slice's counters.  The lanes that share the first
// such lane's word add as one; the others add alone.  (Called in uniform control flow.)
__device__ __forceinline__ void add_combined(uint32_t *s_hist, bool on, uint32_t w, uint32_t lane, uint32_t &n_adds)
{
    const unsigned long long m = __ballot(on);
    if (m == 0ull) return;                                   // (uniform)
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
    const uint32_t lw = (uint32_t)__builtin_amdgcn_readlane((int)w, leader);
    const bool same = on && w == lw;
    const unsigned long long sm = __ballot(same);
    uint32_t cnt = on && !same ? 1u : 0u;
    if ((int)lane == leader) cnt = (uint32_t)__popcll(sm);
    n_adds += (uint32_t)(__popcll(m) - __popcll(sm)) + 1u;
    if (cnt) atomicAdd(s_hist + w, cnt);
}

// The lane's four records a .. a + 3 (a a multiple of four, inside tile T) in the tile's own forms.  whole: every one of
// the four lies inside the columns (always so in an allocation of the context's, whose columns cover whole tiles); else
// the last group of a caller's own columns, read record by record below `end`.
__device__ __forceinline__ void load_four(const ScanColumns &c, const kta_tile_hdr &h, uint64_t T, uint64_t a, bool whole, uint64_t end,
                                          int32_t (&p)[4], int32_t (&kl)[4], int32_t (&vl)[4])
{
    if (!whole) {
        const uint16_t *g16 = reinterpret_cast<const uint16_t *>(c.key_len + T * KTA_TILE_RECORDS);   // (a u16 tile's groups)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            p[j] = kl[j] = vl[j] = -1;
            if (a + j >= end) continue;
            const uint32_t r = (uint32_t)((a + j) % KTA_TILE_RECORDS);
            long long no_ts;
            tile_record_h<false, false>(c.partition, nullptr, h, T, a + j, p[j], no_ts);
            const bool lens16 = h.lens == KTA_TILE_LENS_U16;
            kl[j] = lens16 ? tile_unpack_len(g16[tile_klen_slot(r)]) : c.key_len[a + j];
            vl[j] = lens16 ? tile_unpack_len(g16[tile_vlen_slot(r)]) : c.val_len[a + j];
        }
        return;
    }
    if (h.mode == KTA_TILE_COMPACT) {
        const uint64_t ci = tile_compact_at(a, T);
        const qv2i pw = __builtin_nontemporal_load(reinterpret_cast<const qv2i *>(reinterpret_cast<const uint16_t *>(c.partition) + ci));
        uint32_t u[4];
        tile_u16x4((uint32_t)pw.x, (uint32_t)pw.y, u);
#pragma unroll
        for (int j = 0; j < 4; j++) p[j] = tile_unpack_part(u[j]);
    } else {
        const qv4i pw = __builtin_nontemporal_load(reinterpret_cast<const qv4i *>(c.partition + a));
        p[0] = pw.x, p[1] = pw.y, p[2] = pw.z, p[3] = pw.w;
    }
    if (h.lens == KTA_TILE_LENS_U16) {                        // the group of the tile these four records are
        const uint32_t g = (uint32_t)(a % KTA_TILE_RECORDS) / 4u;
        const qv4i gw = __builtin_nontemporal_load(reinterpret_cast<const qv4i *>(c.key_len + T * KTA_TILE_RECORDS) + g);
        uint32_t ku[4], vu[4];
        tile_u16x4((uint32_t)gw.x, (uint32_t)gw.y, ku);
        tile_u16x4((uint32_t)gw.z, (uint32_t)gw.w, vu);
#pragma unroll
        for (int j = 0; j < 4; j++) kl[j] = tile_unpack_len(ku[j]), vl[j] = tile_unpack_len(vu[j]);
    } else {
        const qv4i kw = __builtin_nontemporal_load(reinterpret_cast<const qv4i *>(c.key_len + a));
        const qv4i vw = __builtin_nontemporal_load(reinterpret_cast<const qv4i *>(c.val_len + a));
        kl[0] = kw.x, kl[1] = kw.y, kl[2] = kw.z, kl[3] = kw.w;
        vl[0] = vw.x, vl[1] = vw.y, vl[2] = vw.z, vl[3] = vw.w;
    }
}

// LOADS_ONLY (a diagnostic, variant 9): the loads and nothing else — the pass's own bound.
template <int THREADS, bool LOADS_ONLY>
__global__ __launch_bounds__(THREADS) void kta_size_quantiles(ScanColumns c, uint64_t n, uint32_t P, uint32_t S, uint32_t slice0,
                                                              unsigned long long *acc, unsigned long long *stats)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_hist[];   // [s_here][3][464]
    __shared__ unsigned long long s_stat[kSizeqStats];
    const uint32_t slice = slice0 + blockIdx.y;
    const uint32_t p_lo = slice * S;
    const uint32_t s_here = P - p_lo < S ? P - p_lo : S;     // the last slice may be partial
    const uint32_t n_words = s_here * kSizePartitionWords;
    for (uint32_t e = threadIdx.x; e < n_words; e += THREADS) s_hist[e] = 0u;
    if (threadIdx.x < kSizeqStats) s_stat[threadIdx.x] = 0ull;
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u;
    // the batch is records [a0, a1) of the columns: of the allocation in a tile-compact batch, of the batch itself in a raw one
    const uint64_t a0 = c.hdr ? c.rec0 : 0, a1 = a0 + n;
    const uint64_t q1 = (a1 + kSizeqStep - 1) / kSizeqStep;
    const uint64_t waves = (uint64_t)gridDim.x * (THREADS / 64);
    const bool globals = slice == 0;                         // (uniform)
    uint32_t n_rec = 0, n_bad = 0, n_keyed = 0, n_alive = 0, n_adds = 0;   // (wave-uniform: popcounts of ballots)
    uint32_t sink = 0;

    for (uint64_t q = a0 / kSizeqStep + (uint64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6); q < q1; q += waves) {
        const uint64_t a = q * kSizeqStep + 4u * lane, T = a / KTA_TILE_RECORDS;
        const kta_tile_hdr h = c.hdr ? c.hdr[T] : kta_tile_hdr{0, KTA_TILE_RAW, KTA_TILE_LENS_I32};
        int32_t p[4], kl[4], vl[4];
        load_four(c, h, T, a, c.sum != nullptr || a + 4 <= a1, a1, p, kl, vl);   // (summaries: an allocation of the context's)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (LOADS_ONLY) {
                sink ^= (uint32_t)p[j] ^ (uint32_t)kl[j] ^ (uint32_t)vl[j];
                continue;
            }
            const bool in = a + j >= a0 && a + j < a1;
            const bool counted = in && (uint32_t)p[j] < P;   // (a negative partition is a large unsigned one)
            const bool keyed = counted && kl[j] >= 0, alive = counted && vl[j] >= 0;
            if (globals) {
                n_rec += (uint32_t)__popcll(__ballot(counted));
                n_bad += (uint32_t)__popcll(__ballot(in && !counted));
                n_keyed += (uint32_t)__popcll(__ballot(keyed));
                n_alive += (uint32_t)__popcll(__ballot(alive));
            }
            const uint32_t ps = (uint32_t)p[j] - p_lo;       // the partition's place in the slice
            const bool mine = counted && ps < s_here;
            if (__ballot(mine) == 0ull) continue;            // (uniform) no record of this slice in the instruction
            const uint32_t base = (mine ? ps : 0u) * kSizePartitionWords;
            add_combined(s_hist, mine && kl[j] >= 0, base + kSizeKey * kSizeBins + size_bin((uint32_t)kl[j]), lane, n_adds);
            add_combined(s_hist, mine && vl[j] >= 0, base + kSizeValue * kSizeBins + size_bin((uint32_t)vl[j]), lane, n_adds);
            add_combined(s_hist, mine && vl[j] >= 0, base + kSizeMessage * kSizeBins + size_bin(size_message(kl[j], vl[j])), lane, n_adds);
        }
    }
    if (LOADS_ONLY) {
        if (sink == 0x9e3779b9u && n == 0) stats[kSizeqStats] = sink;   // (never: n > 0) keeps the loads
        return;
    }
    if (lane == 0) {
        if (globals) {
            atomicAdd(&s_stat[kSizeGlobalRecords], (unsigned long long)n_rec);
            atomicAdd(&s_stat[kSizeGlobalBadPartition], (unsigned long long)n_bad);
            atomicAdd(&s_stat[kSizeGlobalKeyed], (unsigned long long)n_keyed);
            atomicAdd(&s_stat[kSizeGlobalAlive], (unsigned long long)n_alive);
        }
        atomicAdd(&s_stat[4], (unsigned long long)n_adds);
    }
    __syncthreads();
    // the workgroup's non-zero counters to the vector: the slice's partitions are consecutive there as they are here
    unsigned long long *out = acc + (size_t)p_lo * kSizePartitionWords;
    for (uint32_t e = threadIdx.x; e < n_words; e += THREADS) {
        const uint32_t v = s_hist[e];
        if (v) atomicAdd(out + e, (unsigned long long)v);
    }
    if (threadIdx.x < 4 && s_stat[threadIdx.x]) atomicAdd(acc + (size_t)P * kSizePartitionWords + threadIdx.x, s_stat[threadIdx.x]);
    if (threadIdx.x == 4 && s_stat[4]) atomicAdd(stats, s_stat[4]);
}

template <int THREADS, bool LOADS_ONLY>
hipError_t launch_one(const SizeqPlan &pl, dim3 grid, const ScanColumns &c, uint64_t n, uint32_t P, uint32_t slice0, unsigned long long *acc,
                      unsigned long long *stats, hipStream_t s)
{
    if (pl.lds_bytes > 48u * 1024u) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&kta_size_quantiles<THREADS, LOADS_ONLY>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((kta_size_quantiles<THREADS, LOADS_ONLY>), grid, dim3(THREADS), pl.lds_bytes, s, c, n, P, pl.slice, slice0, acc, stats);
    return hipGetLastError();
}

} // namespace

void size_quantiles_plan(uint32_t P, uint32_t forced_slice, uint32_t out[5])
{
    const SizeqPlan pl = plan_size_quantiles(P, forced_slice);
    out[0] = pl.slice, out[1] = pl.slices, out[2] = pl.lds_bytes, out[3] = pl.threads, out[4] = pl.wg_per_cu;
}

hipError_t launch_size_quantiles(const ScanColumns &c, uint64_t n, uint32_t P, uint32_t forced_slice, int variant, uint64_t *acc, uint64_t *stats,
                                 int cu_count, uint32_t *workgroups, hipStream_t s)
{
    *workgroups = 0;
    if (n == 0) return hipSuccess;
    if (n > kSizeQuantilesLaunchMax || P == 0 || P > kSizeQuantilesMaxPartitions) return hipErrorInvalidValue;
    const SizeqPlan pl = plan_size_quantiles(P, forced_slice);
    const uint32_t wg_waves = pl.threads / 64;
    const uint64_t a0 = c.hdr ? c.rec0 : 0;
    const uint64_t steps = (a0 + n + kSizeqStep - 1) / kSizeqStep - a0 / kSizeqStep;
    const uint64_t want = (steps + wg_waves - 1) / wg_waves;
    const bool serial = variant == 1;
    // all slices resident at once: the CUs' workgroups are shared out among them (one launch per slice: each has them all)
    uint64_t cap = (uint64_t)(cu_count > 0 ? cu_count : 256) * pl.wg_per_cu;
    if (!serial) cap = cap / pl.slices ? cap / pl.slices : 1;
    const uint32_t gx = (uint32_t)(want < cap ? want : cap);
    unsigned long long *a = reinterpret_cast<unsigned long long *>(acc), *st = reinterpret_cast<unsigned long long *>(stats);
    for (uint32_t slice0 = 0; slice0 < pl.slices; slice0 += serial ? 1u : pl.slices) {
        const dim3 grid(gx, serial ? 1u : pl.slices);
        hipError_t e;
        if (variant == 9) e = pl.threads == 256 ? launch_one<256, true>(pl, grid, c, n, P, slice0, a, st, s) : launch_one<1024, true>(pl, grid, c, n, P, slice0, a, st, s);
        else e = pl.threads == 256 ? launch_one<256, false>(pl, grid, c, n, P, slice0, a, st, s) : launch_one<1024, false>(pl, grid, c, n, P, slice0, a, st, s);
        if (e != hipSuccess) return e;
    }
    *workgroups = gx * pl.slices;
    return hipSuccess;
}

} // namespace kta

// kta_ts_order.hip — the opt-in timestamp-order pass (KTA_FLAG_TS_ORDER, include/kta_hip.h): per partition the records
// that arrive with a timestamp older than one their partition delivered before them, how late they are, and a log2
// histogram of the lateness.  A running maximum per partition over the record stream in consumption order — not a
// commutative accumulation —, so a slice of a batch takes three launches, none of which waits for another workgroup:
//
//   kta_tso_chunk_max  the slice is cut into contiguous chunks, a wave per chunk: the per-partition maximum of the chunk's
//                      timestamped records, in a wave-private LDS table, to row [chunk] of the workspace i64[chunks][P]
//                      (-1: none).  Order does not matter here: LDS max atomics, and one wave reduction for a step of 256
//                      records that all have one partition.
//   kta_tso_prefix     per partition an exclusive prefix maximum down the rows, seeded with hi[p], written back in place;
//                      hi[p] becomes the total.  16 partitions x 64 row segments per workgroup.
//   kta_tso_apply      a wave per chunk again, in order: its LDS table run[P] starts from the chunk's row, every
//                      instruction takes the records 64 j + lane through tso_wave_step (kta_ts_order_wave.h), and the late
//                      records add to the workgroup's LDS accumulators ([P][2] sums, [P] maxima, the histogram replicated
//                      by lane), flushed with device-scope integer atomics at the end: bit-exact.
//
// Both record kernels read partition and timestamp through kta_tile.h's wave-step readers — 2 + 4 B per record of a
// compact tile, 4 + 8 B of a raw one —, non-temporal, a step of 256 records ahead.  No reference counterpart.
#include "kta_kernels.h"

namespace kta {

namespace {

#include "kta_ts_order_wave.h"

constexpr uint32_t kTsoStep = 256;               // records of one wave step: instruction j of it takes the records 64 j + lane
constexpr uint32_t kTsoHistRep = 16;             // copies of the histogram, by lane
constexpr uint32_t kTsoHistWords = 64 * kTsoHistRep;

struct TsoRecs {
    int32_t p[4];       // -1: no record
    long long t[4];
};

// The step of 256 records from batch index a of a chunk that ends at e (ok: the step exists).  Every load is
// unconditional — the index clamped into the chunk, the result masked —, so that a wave requests its next step before it
// works on this one.
__device__ __forceinline__ void tso_load(const ScanColumns &c, const uint64_t &a, const uint64_t &e, bool ok, uint32_t lane, TsoRecs &r)
{
    const StepTile st = step_tile(c.hdr, c.rec0 + a, kTsoStep, ok);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint64_t i = a + 64u * j + lane;
        const bool in = ok && i < e;
        const uint64_t ic = in ? i : e - 1;
        if (c.hdr) {
            step_tile_record<true>(st, c.partition, reinterpret_cast<const int64_t *>(c.ts_ms), c.hdr, c.rec0 + ic, r.p[j], r.t[j]);
        } else {
            r.p[j] = __builtin_nontemporal_load(c.partition + ic);
            r.t[j] = (long long)__builtin_nontemporal_load(c.ts_ms + ic);
        }
        if (!in) r.p[j] = -1;
    }
}

__global__ __launch_bounds__(256) void kta_tso_chunk_max(ScanColumns c, uint64_t n, uint64_t chunk, uint32_t rows, uint32_t P,
                                                         long long *__restrict__ ws)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_mem[];
    const uint32_t W = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    long long *run = reinterpret_cast<long long *>(s_mem) + (size_t)wave * P;
    const uint32_t row = blockIdx.x * W + wave;
    if (row >= rows) return;                     // (no workgroup barrier below: the tables are wave-private)
    for (uint32_t p = lane; p < P; p += 64u) run[p] = -1;
    KTA_TSO_LDS_ORDER();
    const uint64_t s = (uint64_t)row * chunk, e = s + chunk < n ? s + chunk : n;
    const uint64_t nsteps = (e - s + kTsoStep - 1) / kTsoStep;
    TsoRecs cur;
    tso_load(c, s, e, true, lane, cur);
    for (uint64_t step = 0; step < nsteps; step++) {
        const uint64_t next = s + (step + 1) * kTsoStep;
        TsoRecs nxt;
        tso_load(c, next, e, step + 1 < nsteps, lane, nxt);
        bool on[4];
        long long m = -1;
        bool mine = false;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            on[j] = tso_timestamped(cur.p[j], cur.t[j], P);
            if (on[j]) m = tso_max(m, cur.t[j]);
            mine = mine || on[j];
        }
        const uint64_t live = KTA_BALLOT64(mine);
        if (live != 0) {
            // a lane's first timestamped record names its partition; the step has one partition when all agree
            const uint32_t pl = (uint32_t)(on[0] ? cur.p[0] : on[1] ? cur.p[1] : on[2] ? cur.p[2] : cur.p[3]);
            const uint32_t p0 = KTA_READLANE(pl, (uint32_t)__builtin_ctzll(live));
            bool other = false;
#pragma unroll
            for (int j = 0; j < 4; j++) other = other || (on[j] && (uint32_t)cur.p[j] != p0);
            if (KTA_BALLOT64(other) == 0) {
#pragma unroll
                for (uint32_t off = 32; off >= 1; off >>= 1) {
                    const uint32_t lo = __shfl_xor((uint32_t)(unsigned long long)m, off), hi = __shfl_xor((uint32_t)((unsigned long long)m >> 32), off);
                    m = tso_max(m, (long long)(((unsigned long long)hi << 32) | lo));
                }
                if (lane == 0) run[p0] = tso_max(run[p0], m);
                KTA_TSO_LDS_ORDER();
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (on[j]) __hip_atomic_fetch_max(run + cur.p[j], cur.t[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        cur = nxt;
    }
    KTA_TSO_LDS_ORDER();
    long long *out = ws + (size_t)row * P;
    for (uint32_t p = lane; p < P; p += 64u) out[p] = run[p];
}

constexpr uint32_t kTsoPrefixParts = 16, kTsoPrefixSegs = 64;

__global__ __launch_bounds__(kTsoPrefixParts *kTsoPrefixSegs) void kta_tso_prefix(long long *__restrict__ ws, uint32_t rows, uint32_t P,
                                                                                   long long *__restrict__ hi)
{
    __shared__ long long s_m[kTsoPrefixSegs][kTsoPrefixParts];
    const uint32_t px = threadIdx.x % kTsoPrefixParts, seg = threadIdx.x / kTsoPrefixParts;
    const uint32_t p = blockIdx.x * kTsoPrefixParts + px;
    const uint32_t per = (rows + kTsoPrefixSegs - 1) / kTsoPrefixSegs;
    const uint32_t r0 = seg * per < rows ? seg * per : rows, r1 = r0 + per < rows ? r0 + per : rows;
    long long m = -1, run = -1;
    if (p < P) {
        run = hi[p];                             // (every reader before the barrier, the one writer behind it)
        for (uint32_t r = r0; r < r1; r++) m = tso_max(m, ws[(size_t)r * P + p]);
    }
    s_m[seg][px] = m;
    __syncthreads();
    if (p >= P) return;
    for (uint32_t sg = 0; sg < seg; sg++) run = tso_max(run, s_m[sg][px]);
    for (uint32_t r = r0; r < r1; r++) {
        long long *w = ws + (size_t)r * P + p;
        const long long v = *w;
        *w = run;
        run = tso_max(run, v);
    }
    if (seg == kTsoPrefixSegs - 1) hi[p] = run;   // (the last segment's end is the column's: the segments behind r1 are empty)
}

__global__ __launch_bounds__(256) void kta_tso_apply(ScanColumns c, uint64_t n, uint64_t chunk, uint32_t rows, uint32_t P,
                                                     const long long *__restrict__ ws, unsigned long long *vec, unsigned long long *stats)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_mem[];
    __shared__ unsigned long long s_stat[4];     // timestamped records, instructions with one, of them one partition, groups
    const uint32_t W = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    unsigned long long *s_late = s_mem;                          // [P][2]: late records, their lateness
    unsigned long long *s_most = s_late + 2 * (size_t)P;         // [P]: the largest lateness
    unsigned long long *s_hist = s_most + P;                     // [64][kTsoHistRep]
    long long *run = reinterpret_cast<long long *>(s_hist + kTsoHistWords) + (size_t)wave * P;
    uint8_t *tag = reinterpret_cast<uint8_t *>(reinterpret_cast<long long *>(s_hist + kTsoHistWords) + (size_t)W * P) + (size_t)wave * P;
    for (uint32_t e = threadIdx.x; e < 3u * P + kTsoHistWords; e += blockDim.x) s_mem[e] = 0ull;
    if (threadIdx.x < 4) s_stat[threadIdx.x] = 0ull;
    const uint32_t row = blockIdx.x * W + wave;
    const bool has = row < rows;
    if (has)
        for (uint32_t p = lane; p < P; p += 64u) run[p] = ws[(size_t)row * P + p];
    __syncthreads();

    uint32_t n_timed = 0, n_instr = 0, n_one = 0, n_groups = 0;   // (wave-uniform)
    if (has) {
        const uint64_t s = (uint64_t)row * chunk, e = s + chunk < n ? s + chunk : n;
        const uint64_t nsteps = (e - s + kTsoStep - 1) / kTsoStep;
        TsoRecs cur;
        tso_load(c, s, e, true, lane, cur);
        for (uint64_t step = 0; step < nsteps; step++) {
            const uint64_t next = s + (step + 1) * kTsoStep;
            TsoRecs nxt;
            tso_load(c, next, e, step + 1 < nsteps, lane, nxt);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool on = tso_timestamped(cur.p[j], cur.t[j], P);
                const uint32_t timed = (uint32_t)__popcll(KTA_BALLOT64(on));
                n_timed += timed;
                n_instr += timed != 0u;
                const long long prev = tso_wave_step(run, tag, lane, on, (uint32_t)cur.p[j], cur.t[j], n_one, n_groups);
                if (on && prev > cur.t[j]) {
                    const unsigned long long d = (unsigned long long)prev - (unsigned long long)cur.t[j];   // 1 <= d < 2^63
                    const uint32_t p = (uint32_t)cur.p[j];
                    atomicAdd(s_late + 2 * (size_t)p, 1ull);
                    atomicAdd(s_late + 2 * (size_t)p + 1, d);
                    __hip_atomic_fetch_max(s_most + p, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    atomicAdd(s_hist + (63u - (uint32_t)__builtin_clzll(d)) * kTsoHistRep + (lane & (kTsoHistRep - 1u)), 1ull);
                }
            }
            cur = nxt;
        }
    }
    if (lane == 0 && n_timed) {
        atomicAdd(&s_stat[0], (unsigned long long)n_timed);
        atomicAdd(&s_stat[1], (unsigned long long)n_instr);
        atomicAdd(&s_stat[2], (unsigned long long)n_one);
        atomicAdd(&s_stat[3], (unsigned long long)n_groups);
    }
    __syncthreads();
    // vec: [P][2] | hist[63] | timed | most[P]
    for (uint32_t e = threadIdx.x; e < 2u * P; e += blockDim.x)
        if (s_late[e]) atomicAdd(vec + e, s_late[e]);
    for (uint32_t p = threadIdx.x; p < P; p += blockDim.x)
        if (s_most[p]) __hip_atomic_fetch_max(vec + 2 * (size_t)P + 64 + p, s_most[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (uint32_t e = threadIdx.x; e < 67u; e += blockDim.x) {   // the histogram's 63 words, timed, then the three work counters
        unsigned long long h = 0;
        if (e < 63u)
            for (uint32_t r = 0; r < kTsoHistRep; r++) h += s_hist[e * kTsoHistRep + r];
        else
            h = s_stat[e - 63u];
        if (h) atomicAdd(e < 64u ? vec + 2 * (size_t)P + e : stats + (e - 64u), h);
    }
}

} // namespace

uint32_t ts_order_waves(uint32_t P) { return P <= 1024u ? 4u : P <= 2048u ? 2u : 1u; }

hipError_t launch_ts_order(const ScanColumns &c, uint64_t n, uint64_t chunk, uint32_t P, const TsOrderState &st, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    const uint32_t rows = (uint32_t)((n + chunk - 1) / chunk);
    const uint32_t W = ts_order_waves(P), blocks = (rows + W - 1) / W;
    const uint32_t lds_max = W * P * 8u;
    const uint32_t lds_apply = (3u * P + kTsoHistWords) * 8u + W * P * 8u + W * ((P + 7u) & ~7u);
    if (lds_apply > 65536u) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&kta_tso_apply), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_apply);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kta_tso_chunk_max, dim3(blocks), dim3(64u * W), lds_max, s, c, n, chunk, rows, P, reinterpret_cast<long long *>(st.ws));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kta_tso_prefix, dim3((P + kTsoPrefixParts - 1) / kTsoPrefixParts), dim3(kTsoPrefixParts * kTsoPrefixSegs), 0, s,
                       reinterpret_cast<long long *>(st.ws), rows, P, reinterpret_cast<long long *>(st.hi));
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kta_tso_apply, dim3(blocks), dim3(64u * W), lds_apply, s, c, n, chunk, rows, P, reinterpret_cast<const long long *>(st.ws),
                       reinterpret_cast<unsigned long long *>(st.vec), reinterpret_cast<unsigned long long *>(st.stats));
    return hipGetLastError();
}

} // namespace kta

// kta_segments.hip — the segment pass of the retention what-if (kta_set_segments, include/kta_hip.h; the rule and the
// vector's layout are kta_segments.h's): for every record its position in its partition's log — the per-partition prefix
// sums {records, bytes, tombstones} and the running maximum timestamp over the interleaved partitions, in consumption
// order and across batches — and, from the positions, the rows of the model segments that records close.  The scheme is
// the timestamp-order pass's (kta_ts_order.hip) with sums beside the maximum: a slice of a batch takes three launches,
// none of which waits for another workgroup.
//
//   kta_seg_chunk_sum  the slice is cut into contiguous chunks, a wave per chunk: the chunk's per-partition {bytes,
//                      records | tombstones << 32, H + 1} in a wave-private LDS table (order does not matter: LDS atomics,
//                      and one wave reduction for a step of 256 records that all have one partition), then as {C, B, T,
//                      H + 1} to row [chunk] of the workspace u64[chunks][P][4].  It also counts the records that take
//                      part and those with a partition outside [0, P), and clears the chunk's flag.
//   kta_seg_prefix     per partition an exclusive prefix down the rows, seeded with the partition's totals in the vector —
//                      the running state, which becomes the new total —, written back in place; a chunk's flag is set
//                      when ANY partition's bytes get past a segment boundary inside it.  One division per thread and
//                      one per crossing: the next boundary is carried down the rows.
//   kta_seg_apply      a wave per chunk again.  A wave whose chunk's flag is clear leaves at once: nothing in it closes a
//                      row.  Otherwise its LDS tables run[P][4] / nxt[P] start from the chunk's row, every instruction
//                      takes the records 64 j + lane through seg_wave_step (kta_segments_wave.h), and the lanes whose
//                      record closes a row store it: exactly one record closes a given row, so plain stores.
//
// Both record kernels read partition, timestamp and both lengths through kta_tile.h's step readers in each tile's own
// form — compact or raw, u16 or i32 lengths —, non-temporal, a step of 256 records ahead.  The scan plane is not read.
//
// The kept rows of the compact,delete what-if (kta_set_compact_delete; kta_compact_delete.h) are the same triple over the
// words {L, B, T, K}, run in the compaction replay behind the launch that wrote the records' class bytes:
//   kta_kept_chunk_sum  the chunk's per-partition {B, L | T << 32, K} — the same 24 B per partition, the same two paths —,
//                       reading partition and lengths as above and the class byte; not the timestamp.
//   kta_kept_prefix     kta_seg_prefix's text with the fourth word combined by sum.
//   kta_kept_apply      kta_seg_apply's text over seg_wave_step<true>: flagged chunks only, plain stores.
// No reference counterpart.
#include "kta_compact_delete.h"
#include "kta_kernels.h"
#include "kta_segments.h"

namespace kta {

namespace {

#include "kta_segments_wave.h"

constexpr uint32_t kSegStep = 256;               // records of one wave step: instruction j of it takes the records 64 j + lane

struct SegRecs {
    int32_t p[4];       // -1: no record (see in)
    long long t[4];
    int32_t k[4], v[4];
    bool in[4];         // the lane has a record
};

// The step of 256 records from batch index a of a chunk that ends at e (ok: the step exists).  Every load is
// unconditional — the index clamped into the chunk, the result masked —, so that a wave requests its next step before it
// works on this one.
__device__ __forceinline__ void seg_load(const ScanColumns &c, const uint64_t &a, const uint64_t &e, bool ok, uint32_t lane, SegRecs &r)
{
    const StepTile st = step_tile(c.hdr, c.rec0 + a, kSegStep, ok);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint64_t i = a + 64u * j + lane;
        const bool in = ok && i < e;
        const uint64_t ic = in ? i : e - 1;
        if (c.hdr) {
            const uint64_t ai = c.rec0 + ic, T = ai / KTA_TILE_RECORDS;
            step_tile_record<true>(st, c.partition, reinterpret_cast<const int64_t *>(c.ts_ms), c.hdr, ai, r.p[j], r.t[j]);
            const uint32_t lens = st.one ? st.h.lens : c.hdr[T].lens;
            if (lens == KTA_TILE_LENS_U16) {
                const uint16_t *g16 = reinterpret_cast<const uint16_t *>(c.key_len + T * KTA_TILE_RECORDS);
                const uint32_t q = (uint32_t)(ai % KTA_TILE_RECORDS);
                r.k[j] = tile_unpack_len(__builtin_nontemporal_load(g16 + tile_klen_slot(q)));
                r.v[j] = tile_unpack_len(__builtin_nontemporal_load(g16 + tile_vlen_slot(q)));
            } else {
                r.k[j] = __builtin_nontemporal_load(c.key_len + ai);
                r.v[j] = __builtin_nontemporal_load(c.val_len + ai);
            }
        } else {
            r.p[j] = __builtin_nontemporal_load(c.partition + ic);
            r.t[j] = (long long)__builtin_nontemporal_load(c.ts_ms + ic);
            r.k[j] = __builtin_nontemporal_load(c.key_len + ic);
            r.v[j] = __builtin_nontemporal_load(c.val_len + ic);
        }
        r.in[j] = in;
        if (!in) r.p[j] = -1;
    }
}

__device__ __forceinline__ uint64_t seg_shfl_xor(uint64_t v, uint32_t off)
{
    const uint32_t lo = __shfl_xor((uint32_t)v, off), hi = __shfl_xor((uint32_t)(v >> 32), off);
    return ((uint64_t)hi << 32) | lo;
}

constexpr uint32_t kSegSumWords = 3;             // the chunk table's words of a partition: B, C | T << 32, H + 1

__global__ __launch_bounds__(256) void kta_seg_chunk_sum(ScanColumns c, uint64_t n, uint64_t chunk, uint32_t rows, uint32_t P, uint32_t overhead,
                                                         unsigned long long *__restrict__ ws, uint32_t *__restrict__ flags,
                                                         unsigned long long *globals)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_mem[];
    const uint32_t W = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    unsigned long long *tab = s_mem + (size_t)wave * P * kSegSumWords;
    const uint32_t row = blockIdx.x * W + wave;
    if (row >= rows) return;                     // (no workgroup barrier below: the tables are wave-private)
    for (uint32_t e = lane; e < P * kSegSumWords; e += 64u) tab[e] = 0ull;
    if (lane == 0) flags[row] = 0u;
    KTA_SEG_LDS_ORDER();
    const uint64_t s = (uint64_t)row * chunk, e = s + chunk < n ? s + chunk : n;
    const uint64_t nsteps = (e - s + kSegStep - 1) / kSegStep;
    uint32_t n_part = 0, n_bad = 0;              // (wave-uniform)
    SegRecs cur;
    seg_load(c, s, e, true, lane, cur);
    for (uint64_t step = 0; step < nsteps; step++) {
        const uint64_t next = s + (step + 1) * kSegStep;
        SegRecs nxt;
        seg_load(c, next, e, step + 1 < nsteps, lane, nxt);
        bool on[4], mine = false;
        uint64_t z[4], h1[4], b = 0, ct = 0, h = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            on[j] = seg_takes_part(cur.p[j], P);
            n_part += (uint32_t)__popcll(KTA_BALLOT64(on[j]));
            n_bad += (uint32_t)__popcll(KTA_BALLOT64(cur.in[j] && !on[j]));
            z[j] = segments_record_size(overhead, cur.k[j], cur.v[j]);
            h1[j] = segments_ts_word(cur.t[j]);
            if (on[j]) b += z[j], ct += 1ull | (cur.v[j] < 0 ? 1ull << 32 : 0ull), h = seg_max(h, h1[j]);
            mine = mine || on[j];
        }
        const uint64_t live = KTA_BALLOT64(mine);
        if (live != 0) {
            // a lane's first record that takes part names its partition; the step has one partition when all agree
            const uint32_t pl = (uint32_t)(on[0] ? cur.p[0] : on[1] ? cur.p[1] : on[2] ? cur.p[2] : cur.p[3]);
            const uint32_t p0 = KTA_READLANE(pl, (uint32_t)__builtin_ctzll(live));
            bool other = false;
#pragma unroll
            for (int j = 0; j < 4; j++) other = other || (on[j] && (uint32_t)cur.p[j] != p0);
            if (KTA_BALLOT64(other) == 0) {
#pragma unroll
                for (uint32_t off = 32; off >= 1; off >>= 1) {
                    b += seg_shfl_xor(b, off);
                    ct += seg_shfl_xor(ct, off);
                    h = seg_max(h, seg_shfl_xor(h, off));
                }
                if (lane == 0) {
                    unsigned long long *t = tab + (size_t)p0 * kSegSumWords;
                    t[0] += b, t[1] += ct, t[2] = seg_max(t[2], h);
                }
                KTA_SEG_LDS_ORDER();
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (on[j]) {
                        unsigned long long *t = tab + (size_t)(uint32_t)cur.p[j] * kSegSumWords;
                        atomicAdd(t, (unsigned long long)z[j]);
                        atomicAdd(t + 1, 1ull | (cur.v[j] < 0 ? 1ull << 32 : 0ull));
                        if (h1[j]) __hip_atomic_fetch_max(t + 2, (unsigned long long)h1[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                KTA_SEG_LDS_ORDER();
            }
        }
        cur = nxt;
    }
    KTA_SEG_LDS_ORDER();
    unsigned long long *out = ws + (size_t)row * P * kSegWords;
    for (uint32_t p = lane; p < P; p += 64u) {
        const unsigned long long *t = tab + (size_t)p * kSegSumWords;
        out[(size_t)p * kSegWords + kSegC] = t[1] & 0xFFFFFFFFull;
        out[(size_t)p * kSegWords + kSegB] = t[0];
        out[(size_t)p * kSegWords + kSegT] = t[1] >> 32;
        out[(size_t)p * kSegWords + kSegH1] = t[2];
    }
    if (lane == 0) {
        if (n_part) atomicAdd(globals + kSegGlobalRecords, (unsigned long long)n_part);
        if (n_bad) atomicAdd(globals + kSegGlobalBadPartition, (unsigned long long)n_bad);
    }
}

constexpr uint32_t kSegPrefixParts = 16, kSegPrefixSegs = 64;

// (SUM: the fourth word is a sum — the kept rows' K — instead of the maximum)
template <bool SUM>
__device__ __forceinline__ void seg_prefix_rows(unsigned long long *__restrict__ ws, const uint32_t rows, const uint32_t P,
                                                unsigned long long *__restrict__ totals, uint32_t *__restrict__ flags, const uint64_t S,
                                                const uint32_t M, unsigned long long (*s_m)[kSegPrefixParts][kSegWords])
{
    const uint32_t px = threadIdx.x % kSegPrefixParts, seg = threadIdx.x / kSegPrefixParts;
    const uint32_t p = blockIdx.x * kSegPrefixParts + px;
    const uint32_t per = (rows + kSegPrefixSegs - 1) / kSegPrefixSegs;
    const uint32_t r0 = seg * per < rows ? seg * per : rows, r1 = r0 + per < rows ? r0 + per : rows;
    unsigned long long m[kSegWords] = {0, 0, 0, 0}, run[kSegWords] = {0, 0, 0, 0};
    if (p < P) {
        for (uint32_t k = 0; k < kSegWords; k++) run[k] = totals[(size_t)p * kSegWords + k];   // (every reader before the barrier, the one writer behind it)
        for (uint32_t r = r0; r < r1; r++) {
            const unsigned long long *w = ws + ((size_t)r * P + p) * kSegWords;
            m[kSegC] += w[kSegC], m[kSegB] += w[kSegB], m[kSegT] += w[kSegT], m[kSegH1] = seg_join<SUM>(m[kSegH1], w[kSegH1]);
        }
    }
    for (uint32_t k = 0; k < kSegWords; k++) s_m[seg][px][k] = m[k];
    __syncthreads();
    if (p >= P) return;
    for (uint32_t sg = 0; sg < seg; sg++) {
        run[kSegC] += s_m[sg][px][kSegC], run[kSegB] += s_m[sg][px][kSegB], run[kSegT] += s_m[sg][px][kSegT];
        run[kSegH1] = seg_join<SUM>(run[kSegH1], s_m[sg][px][kSegH1]);
    }
    uint64_t nx = r0 < r1 ? segments_next_boundary(run[kSegB], S, M) : UINT64_MAX;
    for (uint32_t r = r0; r < r1; r++) {
        unsigned long long *w = ws + ((size_t)r * P + p) * kSegWords;
        unsigned long long v[kSegWords];
        for (uint32_t k = 0; k < kSegWords; k++) v[k] = w[k], w[k] = run[k];
        run[kSegC] += v[kSegC], run[kSegB] += v[kSegB], run[kSegT] += v[kSegT], run[kSegH1] = seg_join<SUM>(run[kSegH1], v[kSegH1]);
        if (run[kSegB] >= nx) {                  // the partition's segment at the chunk's end is not the one at its beginning
            atomicOr(flags + r, 1u);
            nx = segments_next_boundary(run[kSegB], S, M);
        }
    }
    if (seg == kSegPrefixSegs - 1)               // (the last segment's end is the column's: the segments behind r1 are empty)
        for (uint32_t k = 0; k < kSegWords; k++) totals[(size_t)p * kSegWords + k] = run[k];
}

__global__ __launch_bounds__(kSegPrefixParts *kSegPrefixSegs) void kta_seg_prefix(unsigned long long *__restrict__ ws, uint32_t rows, uint32_t P,
                                                                                   unsigned long long *__restrict__ totals,
                                                                                   uint32_t *__restrict__ flags, uint64_t S, uint32_t M)
{
    __shared__ unsigned long long s_m[kSegPrefixSegs][kSegPrefixParts][kSegWords];
    seg_prefix_rows<false>(ws, rows, P, totals, flags, S, M, s_m);
}

__global__ __launch_bounds__(kSegPrefixParts *kSegPrefixSegs) void kta_kept_prefix(unsigned long long *__restrict__ ws, uint32_t rows, uint32_t P,
                                                                                    unsigned long long *__restrict__ totals,
                                                                                    uint32_t *__restrict__ flags, uint64_t S, uint32_t M)
{
    __shared__ unsigned long long s_m[kSegPrefixSegs][kSegPrefixParts][kSegWords];
    seg_prefix_rows<true>(ws, rows, P, totals, flags, S, M, s_m);
}

__global__ __launch_bounds__(256) void kta_seg_apply(ScanColumns c, uint64_t n, uint64_t chunk, uint32_t rows, uint32_t P, uint32_t overhead, uint64_t S,
                                                     uint32_t M, const unsigned long long *__restrict__ ws, const uint32_t *__restrict__ flags,
                                                     unsigned long long *vec, unsigned long long *globals, unsigned long long *stats)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_mem[];
    const uint32_t W = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t row = blockIdx.x * W + wave;
    if (row >= rows) return;                     // (no workgroup barrier below: the tables are wave-private)
    if (flags[row] == 0u) {                      // (wave-uniform) nothing in this chunk closes a row
        if (lane == 0) atomicAdd(stats + 1, 1ull);
        return;
    }
    uint64_t *run = reinterpret_cast<uint64_t *>(s_mem) + (size_t)wave * P * kSegWords;
    uint64_t *nxt = reinterpret_cast<uint64_t *>(s_mem) + (size_t)W * P * kSegWords + (size_t)wave * P;
    uint8_t *tag = reinterpret_cast<uint8_t *>(reinterpret_cast<uint64_t *>(s_mem) + (size_t)W * P * (kSegWords + 1u)) + (size_t)wave * P;
    for (uint32_t p = lane; p < P; p += 64u) {
        const unsigned long long *w = ws + ((size_t)row * P + p) * kSegWords;
        for (uint32_t k = 0; k < kSegWords; k++) run[(size_t)p * kSegWords + k] = w[k];
        nxt[p] = segments_next_boundary(w[kSegB], S, M);
    }
    KTA_SEG_LDS_ORDER();

    uint32_t n_closed = 0, n_one = 0, n_groups = 0;   // (wave-uniform)
    const uint64_t s = (uint64_t)row * chunk, e = s + chunk < n ? s + chunk : n;
    const uint64_t nsteps = (e - s + kSegStep - 1) / kSegStep;
    SegRecs cur;
    seg_load(c, s, e, true, lane, cur);
    for (uint64_t step = 0; step < nsteps; step++) {
        const uint64_t next = s + (step + 1) * kSegStep;
        SegRecs nx;
        seg_load(c, next, e, step + 1 < nsteps, lane, nx);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool on = seg_takes_part(cur.p[j], P);
            SegAt at;
            at.closes = false;
            seg_wave_step(run, nxt, tag, lane, on, (uint32_t)cur.p[j], segments_record_size(overhead, cur.k[j], cur.v[j]), cur.v[j] < 0,
                          segments_ts_word(cur.t[j]), S, M, at, n_one, n_groups);
            const bool closes = on && at.closes;      // at.row < M - 1: a later row exists
            if (closes) {
                unsigned long long *r = vec + segments_row_at((uint32_t)cur.p[j], M, at.row);
                for (uint32_t k = 0; k < kSegWords; k++) r[k] = at.v[k];
            }
            n_closed += (uint32_t)__popcll(KTA_BALLOT64(closes));
        }
        cur = nx;
    }
    if (lane == 0) {
        atomicAdd(stats + 0, 1ull);
        if (n_closed) atomicAdd(globals + kSegGlobalClosed, (unsigned long long)n_closed);
        if (n_one) atomicAdd(stats + 2, (unsigned long long)n_one);
        if (n_groups) atomicAdd(stats + 3, (unsigned long long)n_groups);
    }
}

// ---- the kept rows (kta_compact_delete.h) ----------------------------------------------------------------------------
struct KeptRecs {
    int32_t p[4];       // -1: no record (see in)
    int32_t k[4], v[4];
    uint8_t cls[4];     // the class byte launch_compaction stored
    bool in[4];         // the lane has a record
};

// seg_load without the timestamp, with the class byte of record i of the slice (cls[i]: the launch's record 0 is cls[0]).
__device__ __forceinline__ void kept_load(const ScanColumns &c, const uint8_t *__restrict__ cls, const uint64_t &a, const uint64_t &e, bool ok,
                                          uint32_t lane, KeptRecs &r)
{
    const StepTile st = step_tile(c.hdr, c.rec0 + a, kSegStep, ok);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint64_t i = a + 64u * j + lane;
        const bool in = ok && i < e;
        const uint64_t ic = in ? i : e - 1;
        if (c.hdr) {
            const uint64_t ai = c.rec0 + ic, T = ai / KTA_TILE_RECORDS;
            r.p[j] = step_tile_part<true>(st, c.partition, c.hdr, ai);
            const uint32_t lens = st.one ? st.h.lens : c.hdr[T].lens;
            if (lens == KTA_TILE_LENS_U16) {
                const uint16_t *g16 = reinterpret_cast<const uint16_t *>(c.key_len + T * KTA_TILE_RECORDS);
                const uint32_t q = (uint32_t)(ai % KTA_TILE_RECORDS);
                r.k[j] = tile_unpack_len(__builtin_nontemporal_load(g16 + tile_klen_slot(q)));
                r.v[j] = tile_unpack_len(__builtin_nontemporal_load(g16 + tile_vlen_slot(q)));
            } else {
                r.k[j] = __builtin_nontemporal_load(c.key_len + ai);
                r.v[j] = __builtin_nontemporal_load(c.val_len + ai);
            }
        } else {
            r.p[j] = __builtin_nontemporal_load(c.partition + ic);
            r.k[j] = __builtin_nontemporal_load(c.key_len + ic);
            r.v[j] = __builtin_nontemporal_load(c.val_len + ic);
        }
        r.cls[j] = __builtin_nontemporal_load(cls + ic);
        r.in[j] = in;
        if (!in) r.p[j] = -1;
    }
}

// a record's contribution to L | T << 32
__device__ __forceinline__ uint64_t kept_lt(uint8_t cls) { return cls == kKeptClassLive ? 1ull : cls == kKeptClassTombstone ? 1ull << 32 : 0ull; }

__global__ __launch_bounds__(256) void kta_kept_chunk_sum(ScanColumns c, const uint8_t *__restrict__ cls, uint64_t n, uint64_t chunk, uint32_t rows,
                                                          uint32_t P, uint32_t overhead, unsigned long long *__restrict__ ws,
                                                          uint32_t *__restrict__ flags, unsigned long long *globals)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_mem[];
    const uint32_t W = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    unsigned long long *tab = s_mem + (size_t)wave * P * kSegSumWords;   // B, L | T << 32, K
    const uint32_t row = blockIdx.x * W + wave;
    if (row >= rows) return;                     // (no workgroup barrier below: the tables are wave-private)
    for (uint32_t e = lane; e < P * kSegSumWords; e += 64u) tab[e] = 0ull;
    if (lane == 0) flags[row] = 0u;
    KTA_SEG_LDS_ORDER();
    const uint64_t s = (uint64_t)row * chunk, e = s + chunk < n ? s + chunk : n;
    const uint64_t nsteps = (e - s + kSegStep - 1) / kSegStep;
    uint32_t n_part = 0, n_bad = 0;              // (wave-uniform)
    KeptRecs cur;
    kept_load(c, cls, s, e, true, lane, cur);
    for (uint64_t step = 0; step < nsteps; step++) {
        const uint64_t next = s + (step + 1) * kSegStep;
        KeptRecs nxt;
        kept_load(c, cls, next, e, step + 1 < nsteps, lane, nxt);
        bool on[4], mine = false;
        uint64_t z[4], lt[4], b = 0, ct = 0, kb = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            on[j] = seg_takes_part(cur.p[j], P);
            n_part += (uint32_t)__popcll(KTA_BALLOT64(on[j]));
            n_bad += (uint32_t)__popcll(KTA_BALLOT64(cur.in[j] && !on[j]));
            z[j] = segments_record_size(overhead, cur.k[j], cur.v[j]);
            lt[j] = kept_lt(cur.cls[j]);
            if (on[j]) b += z[j], ct += lt[j], kb += lt[j] ? z[j] : 0ull;
            mine = mine || on[j];
        }
        const uint64_t live = KTA_BALLOT64(mine);
        if (live != 0) {
            const uint32_t pl = (uint32_t)(on[0] ? cur.p[0] : on[1] ? cur.p[1] : on[2] ? cur.p[2] : cur.p[3]);
            const uint32_t p0 = KTA_READLANE(pl, (uint32_t)__builtin_ctzll(live));
            bool other = false;
#pragma unroll
            for (int j = 0; j < 4; j++) other = other || (on[j] && (uint32_t)cur.p[j] != p0);
            if (KTA_BALLOT64(other) == 0) {
#pragma unroll
                for (uint32_t off = 32; off >= 1; off >>= 1) {
                    b += seg_shfl_xor(b, off);
                    ct += seg_shfl_xor(ct, off);
                    kb += seg_shfl_xor(kb, off);
                }
                if (lane == 0) {
                    unsigned long long *t = tab + (size_t)p0 * kSegSumWords;
                    t[0] += b, t[1] += ct, t[2] += kb;
                }
                KTA_SEG_LDS_ORDER();
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (on[j]) {
                        unsigned long long *t = tab + (size_t)(uint32_t)cur.p[j] * kSegSumWords;
                        atomicAdd(t, (unsigned long long)z[j]);
                        if (lt[j]) {
                            atomicAdd(t + 1, (unsigned long long)lt[j]);
                            atomicAdd(t + 2, (unsigned long long)z[j]);
                        }
                    }
                KTA_SEG_LDS_ORDER();
            }
        }
        cur = nxt;
    }
    KTA_SEG_LDS_ORDER();
    unsigned long long *out = ws + (size_t)row * P * kSegWords;
    for (uint32_t p = lane; p < P; p += 64u) {
        const unsigned long long *t = tab + (size_t)p * kSegSumWords;
        out[(size_t)p * kSegWords + kKeptL] = t[1] & 0xFFFFFFFFull;
        out[(size_t)p * kSegWords + kKeptB] = t[0];
        out[(size_t)p * kSegWords + kKeptT] = t[1] >> 32;
        out[(size_t)p * kSegWords + kKeptK] = t[2];
    }
    if (lane == 0) {
        if (n_part) atomicAdd(globals + kSegGlobalRecords, (unsigned long long)n_part);
        if (n_bad) atomicAdd(globals + kSegGlobalBadPartition, (unsigned long long)n_bad);
    }
}

__global__ __launch_bounds__(256) void kta_kept_apply(ScanColumns c, const uint8_t *__restrict__ cls, uint64_t n, uint64_t chunk, uint32_t rows,
                                                      uint32_t P, uint32_t overhead, uint64_t S, uint32_t M, const unsigned long long *__restrict__ ws,
                                                      const uint32_t *__restrict__ flags, unsigned long long *vec, unsigned long long *globals,
                                                      unsigned long long *stats)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_mem[];
    const uint32_t W = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t row = blockIdx.x * W + wave;
    if (row >= rows) return;                     // (no workgroup barrier below: the tables are wave-private)
    if (flags[row] == 0u) {                      // (wave-uniform) nothing in this chunk closes a row
        if (lane == 0) atomicAdd(stats + 1, 1ull);
        return;
    }
    uint64_t *run = reinterpret_cast<uint64_t *>(s_mem) + (size_t)wave * P * kSegWords;
    uint64_t *nxt = reinterpret_cast<uint64_t *>(s_mem) + (size_t)W * P * kSegWords + (size_t)wave * P;
    uint8_t *tag = reinterpret_cast<uint8_t *>(reinterpret_cast<uint64_t *>(s_mem) + (size_t)W * P * (kSegWords + 1u)) + (size_t)wave * P;
    for (uint32_t p = lane; p < P; p += 64u) {
        const unsigned long long *w = ws + ((size_t)row * P + p) * kSegWords;
        for (uint32_t k = 0; k < kSegWords; k++) run[(size_t)p * kSegWords + k] = w[k];
        nxt[p] = segments_next_boundary(w[kKeptB], S, M);
    }
    KTA_SEG_LDS_ORDER();

    uint32_t n_closed = 0, n_one = 0, n_groups = 0;   // (wave-uniform)
    const uint64_t s = (uint64_t)row * chunk, e = s + chunk < n ? s + chunk : n;
    const uint64_t nsteps = (e - s + kSegStep - 1) / kSegStep;
    KeptRecs cur;
    kept_load(c, cls, s, e, true, lane, cur);
    for (uint64_t step = 0; step < nsteps; step++) {
        const uint64_t next = s + (step + 1) * kSegStep;
        KeptRecs nx;
        kept_load(c, cls, next, e, step + 1 < nsteps, lane, nx);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool on = seg_takes_part(cur.p[j], P);
            const uint64_t z = segments_record_size(overhead, cur.k[j], cur.v[j]);
            const bool live = cur.cls[j] == kKeptClassLive, tomb = cur.cls[j] == kKeptClassTombstone;
            SegAt at;
            at.closes = false;
            seg_wave_step<true>(run, nxt, tag, lane, on, (uint32_t)cur.p[j], z, tomb, live || tomb ? z : 0ull, S, M, at, n_one, n_groups, live);
            const bool closes = on && at.closes;      // at.row < M - 1: a later row exists
            if (closes) {
                unsigned long long *r = vec + segments_row_at((uint32_t)cur.p[j], M, at.row);
                for (uint32_t k = 0; k < kSegWords; k++) r[k] = at.v[k];
            }
            n_closed += (uint32_t)__popcll(KTA_BALLOT64(closes));
        }
        cur = nx;
    }
    if (lane == 0) {
        atomicAdd(stats + 0, 1ull);
        if (n_closed) atomicAdd(globals + kSegGlobalClosed, (unsigned long long)n_closed);
        if (n_one) atomicAdd(stats + 2, (unsigned long long)n_one);
        if (n_groups) atomicAdd(stats + 3, (unsigned long long)n_groups);
    }
}

} // namespace

uint32_t segments_waves(uint32_t P);

hipError_t launch_kept_rows(const ScanColumns &c, const uint8_t *cls, uint64_t n, uint64_t chunk, uint32_t P, const SegmentsState &st, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (!cls || P == 0 || P > kCompactDeleteMaxPartitions || chunk == 0 || chunk % 64u || chunk > (1ull << 31)) return hipErrorInvalidValue;
    const uint64_t rows64 = (n + chunk - 1) / chunk;
    if (rows64 * P * kSegWords > kSegmentsWorkspaceWords) return hipErrorInvalidValue;
    const uint32_t rows = (uint32_t)rows64;
    const uint32_t W = segments_waves(P), blocks = (rows + W - 1) / W;
    const uint32_t lds_sum = W * P * kSegSumWords * 8u;
    const uint32_t lds_apply = W * P * (kSegWords + 1u) * 8u + W * ((P + 7u) & ~7u);
    if (lds_apply > 65536u) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&kta_kept_apply), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_apply);
        if (e != hipSuccess) return e;
    }
    unsigned long long *vec = reinterpret_cast<unsigned long long *>(st.vec), *ws = reinterpret_cast<unsigned long long *>(st.ws);
    unsigned long long *totals = vec + segments_total_at(P, st.M, 0), *globals = vec + segments_globals_at(P, st.M);
    hipLaunchKernelGGL(kta_kept_chunk_sum, dim3(blocks), dim3(64u * W), lds_sum, s, c, cls, n, chunk, rows, P, st.overhead, ws, st.flags, globals);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kta_kept_prefix, dim3((P + kSegPrefixParts - 1) / kSegPrefixParts), dim3(kSegPrefixParts * kSegPrefixSegs), 0, s, ws, rows, P,
                       totals, st.flags, st.S, st.M);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kta_kept_apply, dim3(blocks), dim3(64u * W), lds_apply, s, c, cls, n, chunk, rows, P, st.overhead, st.S, st.M, ws, st.flags, vec,
                       globals, reinterpret_cast<unsigned long long *>(st.stats));
    return hipGetLastError();
}

uint32_t segments_waves(uint32_t P) { return P <= 512u ? 4u : P <= 1024u ? 2u : 1u; }

hipError_t launch_segments(const ScanColumns &c, uint64_t n, uint64_t chunk, uint32_t P, const SegmentsState &st, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (P == 0 || P > kSegmentsMaxPartitions || chunk == 0 || chunk % 64u || chunk > (1ull << 31)) return hipErrorInvalidValue;
    const uint64_t rows64 = (n + chunk - 1) / chunk;
    if (rows64 * P * kSegWords > kSegmentsWorkspaceWords) return hipErrorInvalidValue;
    const uint32_t rows = (uint32_t)rows64;
    const uint32_t W = segments_waves(P), blocks = (rows + W - 1) / W;
    const uint32_t lds_sum = W * P * kSegSumWords * 8u;
    const uint32_t lds_apply = W * P * (kSegWords + 1u) * 8u + W * ((P + 7u) & ~7u);
    if (lds_apply > 65536u) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&kta_seg_apply), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_apply);
        if (e != hipSuccess) return e;
    }
    unsigned long long *vec = reinterpret_cast<unsigned long long *>(st.vec), *ws = reinterpret_cast<unsigned long long *>(st.ws);
    unsigned long long *totals = vec + segments_total_at(P, st.M, 0), *globals = vec + segments_globals_at(P, st.M);
    hipLaunchKernelGGL(kta_seg_chunk_sum, dim3(blocks), dim3(64u * W), lds_sum, s, c, n, chunk, rows, P, st.overhead, ws, st.flags, globals);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kta_seg_prefix, dim3((P + kSegPrefixParts - 1) / kSegPrefixParts), dim3(kSegPrefixParts * kSegPrefixSegs), 0, s, ws, rows, P,
                       totals, st.flags, st.S, st.M);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kta_seg_apply, dim3(blocks), dim3(64u * W), lds_apply, s, c, n, chunk, rows, P, st.overhead, st.S, st.M, ws, st.flags, vec,
                       globals, reinterpret_cast<unsigned long long *>(st.stats));
    return hipGetLastError();
}

} // namespace kta

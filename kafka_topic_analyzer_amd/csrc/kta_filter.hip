// kta_filter.hip — the record filter (kta_set_filter, include/kta_hip.h): an order-preserving stream compaction of one
// slice of a device batch into the context's scratch batch, in front of the existing passes.  Three launches per slice on
// the compute stream — count per tile, exclusive prefix of the counts, scatter — and no workgroup ever waits on another:
// what one launch needs from all workgroups of the one before it gets from the stream's order.  The host reads the slice's
// total between the second and the third (it has to wait for it anyway, once per slice): a slice of which nothing or
// everything passes needs no scatter.  The rules (the record
// predicate, the tile decision, the rank) are kta_filter.h's; this file only moves records.
#include "kta_kernels.h"
#include "kta_filter.h"

namespace kta {

namespace {

typedef int fv4i __attribute__((ext_vector_type(4)));
typedef int fv2i __attribute__((ext_vector_type(2)));
typedef long long fv2l __attribute__((ext_vector_type(2)));

constexpr uint32_t kFilterWaves = 4;   // a tile of 1024 records: four waves of four 64-record instructions (kta_filter.h)
static_assert(kFilterWaves * 4u * 64u == KTA_TILE_RECORDS, "filter_tile_rank's geometry");

// Tile t of the slice: layout tile T, its records [lo, hi) of the allocation (kta_filter.h: filter_slice_tiles).
struct FilterTileSpan {
    uint64_t T, lo, hi;
};
__device__ __forceinline__ FilterTileSpan filter_span(const FilterSource &c, uint64_t n, uint32_t t)
{
    FilterTileSpan s;
    s.T = c.a0 / KTA_TILE_RECORDS + t;
    const uint64_t first = s.T * KTA_TILE_RECORDS, end = c.a0 + n;
    s.lo = first > c.a0 ? first : c.a0;
    s.hi = first + KTA_TILE_RECORDS < end ? first + KTA_TILE_RECORDS : end;
    return s;
}

// The tile's header (zero: the raw layout) and what it and the summary decide (uniform).
__device__ __forceinline__ FilterTile filter_decide(const FilterSource &c, const FilterSpec &f, const FilterTileSpan &s, kta_tile_hdr &h)
{
    h = kta_tile_hdr{0, KTA_TILE_RAW, KTA_TILE_LENS_I32};
    if (!c.hdr) return FILTER_TILE_READ;
    h = c.hdr[s.T];
    if (!c.sum) return FILTER_TILE_READ;
    return filter_tile_decide(f, h, c.sum[s.T], s.hi - s.lo == KTA_TILE_RECORDS);
}

// The partition set into LDS (nothing without one).  The caller's barrier follows.
__device__ __forceinline__ void filter_load_bitmap(const FilterSpec &f, const uint32_t *__restrict__ bitmap, uint32_t *s_bitmap)
{
    if (!f.parts) return;
    for (uint32_t w = threadIdx.x; w < filter_bitmap_words(f.P); w += blockDim.x) s_bitmap[w] = bitmap[w];
}

// The four ballots of a wave over its 256 records of the tile: which of them lie in [lo, hi) and pass.  all: the tile's
// count says every record of [lo, hi) passes, so nothing is read.
__device__ __forceinline__ void filter_wave_ballots(const FilterSource &c, const FilterSpec &f, const uint32_t *s_bitmap, const kta_tile_hdr &h,
                                                    const FilterTileSpan &s, bool all, uint32_t wave, uint32_t lane, uint64_t (&ballot)[4])
{
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint64_t a = s.T * KTA_TILE_RECORDS + wave * 256u + k * 64u + lane;
        const bool in = a >= s.lo && a < s.hi;
        bool pass = in;
        if (in && !all) {
            int32_t p;
            long long ts;
            tile_record_h<true>(c.partition, c.ts_ms, h, s.T, a, p, ts);
            pass = filter_record_passes(f, s_bitmap, p, ts);
        }
        ballot[k] = (uint64_t)__builtin_amdgcn_ballot_w64(pass);
    }
}

// 1: count[t] = the passing records of tile t of the slice, and in the word's high half how the tile was decided
// (kFilterClassShift: FilterTile), for kta_filter_offsets to tally — one atomic per class and slice there instead of one
// per tile here, all on the same three words.
constexpr uint32_t kFilterClassShift = 16, kFilterCountMask = 0xFFFFu;
static_assert(KTA_TILE_RECORDS <= kFilterCountMask, "a tile's count fits the low half");

// A workgroup takes kFilterGroup consecutive tiles: its first lanes decide one tile each from header and summary (a slice
// of summarised tiles is kFilterGroup times fewer, and fuller, workgroups), then the four waves read the tiles left over,
// one after the other.
constexpr uint32_t kFilterGroup = 8;

__global__ __launch_bounds__(256) void kta_filter_count(FilterSource c, uint64_t n, FilterSpec f, const uint32_t *__restrict__ bitmap,
                                                        uint32_t *__restrict__ count, uint32_t tiles)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_bitmap[];
    __shared__ uint32_t s_wave[kFilterWaves];
    __shared__ uint32_t s_decided[kFilterGroup];
    const uint32_t g0 = blockIdx.x * kFilterGroup, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (threadIdx.x < kFilterGroup) {
        const uint32_t t = g0 + threadIdx.x;
        uint32_t d = FILTER_TILE_NONE;               // (a tile behind the slice's last: nothing to read)
        if (t < tiles) {
            kta_tile_hdr h;
            d = filter_decide(c, f, filter_span(c, n, t), h);
            if (d != FILTER_TILE_READ) count[t] = (d == FILTER_TILE_ALL ? KTA_TILE_RECORDS : 0u) | (d << kFilterClassShift);
        }
        s_decided[threadIdx.x] = d;
    }
    filter_load_bitmap(f, bitmap, s_bitmap);
    __syncthreads();
    for (uint32_t q = 0; q < kFilterGroup; q++) {
        if (s_decided[q] != FILTER_TILE_READ) continue;   // (uniform)
        const uint32_t t = g0 + q;
        const FilterTileSpan s = filter_span(c, n, t);
        const kta_tile_hdr h = c.hdr ? c.hdr[s.T] : kta_tile_hdr{0, KTA_TILE_RAW, KTA_TILE_LENS_I32};
        uint64_t ballot[4];
        filter_wave_ballots(c, f, s_bitmap, h, s, false, wave, lane, ballot);
        if (lane == 0) s_wave[wave] = (uint32_t)(__popcll(ballot[0]) + __popcll(ballot[1]) + __popcll(ballot[2]) + __popcll(ballot[3]));
        __syncthreads();
        if (threadIdx.x == 0) count[t] = (s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]) | ((uint32_t)FILTER_TILE_READ << kFilterClassShift);
        __syncthreads();                             // (s_wave is the next tile's as well)
    }
}

// 2: offset[t] = the passing records of the tiles below t; offset[tiles] = the slice's total (also to the host's word);
// stats += the tiles decided NONE, decided ALL, read.  One workgroup: every thread takes a stretch of the counts, a
// multiple of four, sums it, the 256 sums are scanned in LDS, and every thread writes its stretch's offsets.  Both loops
// have a trip count the compiler can unroll and loads without a condition (the count buffer holds 256 whole stretches for
// kFilterMaxTiles tiles, kFilterCountWords; what lies behind `tiles` is loaded and masked): several 16-byte loads are in
// flight at once — one load per turn, waited for, made this kernel cost more than all the rest of a slice of summarised
// tiles.  A slice's total is at most 2^26: u32 sums.
constexpr uint32_t kFilterScanThreads = 256;
static_assert((uint64_t)kFilterScanThreads * (((kFilterMaxTiles + kFilterScanThreads - 1) / kFilterScanThreads + 3) & ~3ull) <= kFilterCountWords,
              "the stretches of the largest slice lie inside the count buffer");

__global__ __launch_bounds__(kFilterScanThreads) void kta_filter_offsets(const uint32_t *__restrict__ count, uint32_t tiles,
                                                                         unsigned long long *__restrict__ offset, unsigned long long *stats,
                                                                         unsigned long long *total_host)
{
    __shared__ uint32_t s_sum[kFilterScanThreads];
    __shared__ uint32_t s_class[3];
    if (threadIdx.x < 3) s_class[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t per = ((tiles + kFilterScanThreads - 1) / kFilterScanThreads + 3u) & ~3u;
    const uint32_t t0 = threadIdx.x * per, turns = per / 4u;
    const fv4i *mine4 = reinterpret_cast<const fv4i *>(count + t0);
    uint32_t mine = 0, cls[3] = {0u, 0u, 0u};
#pragma unroll 8
    for (uint32_t i = 0; i < turns; i++) {
        const fv4i w = mine4[i];
        const uint32_t u[4] = {(uint32_t)w.x, (uint32_t)w.y, (uint32_t)w.z, (uint32_t)w.w};
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            const bool on = t0 + 4u * i + q < tiles;
            const uint32_t cl = u[q] >> kFilterClassShift;
            mine += on ? u[q] & kFilterCountMask : 0u;
            cls[0] += on && cl == FILTER_TILE_NONE, cls[1] += on && cl == FILTER_TILE_ALL, cls[2] += on && cl == FILTER_TILE_READ;
        }
    }
    s_sum[threadIdx.x] = mine;
#pragma unroll
    for (uint32_t k = 0; k < 3; k++)
        if (cls[k]) atomicAdd(&s_class[k], cls[k]);
    __syncthreads();
    uint32_t run = 0;
    for (uint32_t q = 0; q < threadIdx.x; q++) run += s_sum[q];
#pragma unroll 4
    for (uint32_t i = 0; i < turns; i++) {
        const fv4i w = mine4[i];
        const uint32_t t = t0 + 4u * i;
        const uint32_t c0 = t < tiles ? (uint32_t)w.x & kFilterCountMask : 0u, c1 = t + 1 < tiles ? (uint32_t)w.y & kFilterCountMask : 0u,
                       c2 = t + 2 < tiles ? (uint32_t)w.z & kFilterCountMask : 0u, c3 = t + 3 < tiles ? (uint32_t)w.w & kFilterCountMask : 0u;
        const unsigned long long o0 = run, o1 = o0 + c0, o2 = o1 + c1, o3 = o2 + c2;
        run += c0 + c1 + c2 + c3;
        if (t + 3 < tiles) {
            *reinterpret_cast<fv2l *>(offset + t) = fv2l{(long long)o0, (long long)o1};
            *reinterpret_cast<fv2l *>(offset + t + 2) = fv2l{(long long)o2, (long long)o3};
        } else {
            if (t < tiles) offset[t] = o0;
            if (t + 1 < tiles) offset[t + 1] = o1;
            if (t + 2 < tiles) offset[t + 2] = o2;
        }
    }
    if (threadIdx.x == kFilterScanThreads - 1) {   // (the stretches behind the last tile are empty: the last thread's end is the total)
        offset[tiles] = run;
        *total_host = run;                       // pinned host memory: there when the host's wait for the stream returns
    }
    if (threadIdx.x < 3 && s_class[threadIdx.x]) atomicAdd(stats + threadIdx.x, (unsigned long long)s_class[threadIdx.x]);
}

// A whole tile all of whose records pass, to records [off, off + 1024) of the scratch batch, off a multiple of four: every
// thread takes the tile's records 4 tid .. 4 tid + 3 and stores 16 bytes at a time (the scratch columns are 16-byte
// aligned, so record off + 4 tid of an i32 column is).  The loads are the tile's own forms: 8 B of u16 partitions and
// 16 B of timestamp offsets of a compact tile, one 16-byte group of u16 lengths, or the plain columns.
__device__ __forceinline__ void filter_copy_tile(const FilterSource &c, const kta_tile_hdr &h, uint64_t T, unsigned long long off, const FilterDest &out)
{
    const uint32_t tid = threadIdx.x;
    const uint64_t a = T * KTA_TILE_RECORDS + 4u * tid;          // the first of the thread's four records
    const unsigned long long d = off + 4u * tid;
    if (d + 4 > out.capacity) return;                            // (never)
    int32_t p[4];
    long long ts[4];
    if (h.mode == KTA_TILE_COMPACT) {
        const uint64_t ci = tile_compact_at(a, T);
        const fv2i pw = __builtin_nontemporal_load(reinterpret_cast<const fv2i *>(reinterpret_cast<const uint16_t *>(c.partition) + ci));
        const fv4i ow = __builtin_nontemporal_load(reinterpret_cast<const fv4i *>(reinterpret_cast<const int32_t *>(c.ts_ms) + ci));
        uint32_t u[4];
        tile_u16x4((uint32_t)pw.x, (uint32_t)pw.y, u);
        const int32_t o[4] = {ow.x, ow.y, ow.z, ow.w};
#pragma unroll
        for (int q = 0; q < 4; q++) p[q] = tile_unpack_part(u[q]), ts[q] = tile_unpack_ts(o[q], h.ts_base);
    } else {
        const fv4i pw = __builtin_nontemporal_load(reinterpret_cast<const fv4i *>(c.partition + a));
        const fv2l t0 = __builtin_nontemporal_load(reinterpret_cast<const fv2l *>(c.ts_ms + a));
        const fv2l t1 = __builtin_nontemporal_load(reinterpret_cast<const fv2l *>(c.ts_ms + a + 2));
        p[0] = pw.x, p[1] = pw.y, p[2] = pw.z, p[3] = pw.w;
        ts[0] = t0.x, ts[1] = t0.y, ts[2] = t1.x, ts[3] = t1.y;
    }
    int32_t kl[4], vl[4];
    if (h.lens == KTA_TILE_LENS_U16) {                          // group tid of the tile: four key lengths, four value lengths
        const fv4i g = __builtin_nontemporal_load(reinterpret_cast<const fv4i *>(c.key_len + T * KTA_TILE_RECORDS) + tid);
        uint32_t ku[4], vu[4];
        tile_u16x4((uint32_t)g.x, (uint32_t)g.y, ku);
        tile_u16x4((uint32_t)g.z, (uint32_t)g.w, vu);
#pragma unroll
        for (int q = 0; q < 4; q++) kl[q] = tile_unpack_len(ku[q]), vl[q] = tile_unpack_len(vu[q]);
    } else {
        const fv4i kw = __builtin_nontemporal_load(reinterpret_cast<const fv4i *>(c.key_len + a));
        const fv4i vw = __builtin_nontemporal_load(reinterpret_cast<const fv4i *>(c.val_len + a));
        kl[0] = kw.x, kl[1] = kw.y, kl[2] = kw.z, kl[3] = kw.w;
        vl[0] = vw.x, vl[1] = vw.y, vl[2] = vw.z, vl[3] = vw.w;
    }
    *reinterpret_cast<fv4i *>(out.partition + d) = fv4i{p[0], p[1], p[2], p[3]};
    *reinterpret_cast<fv4i *>(out.key_len + d) = fv4i{kl[0], kl[1], kl[2], kl[3]};
    *reinterpret_cast<fv4i *>(out.val_len + d) = fv4i{vl[0], vl[1], vl[2], vl[3]};
    *reinterpret_cast<fv2l *>(out.ts_ms + d) = fv2l{ts[0], ts[1]};
    *reinterpret_cast<fv2l *>(out.ts_ms + d + 2) = fv2l{ts[2], ts[3]};
    const uint64_t i = a - c.a0;                                 // the records' index in the slice
    if (out.key_off)
        *reinterpret_cast<fv4i *>(out.key_off + d) = fv4i{(int)c.key_off[i], (int)c.key_off[i + 1], (int)c.key_off[i + 2], (int)c.key_off[i + 3]};
    if (out.seq) {
        unsigned long long q[4];
#pragma unroll
        for (int e = 0; e < 4; e++) q[e] = c.seq ? c.seq[i + e] : c.base_seq + i + e;
        *reinterpret_cast<fv2l *>(out.seq + d) = fv2l{(long long)q[0], (long long)q[1]};
        *reinterpret_cast<fv2l *>(out.seq + d + 2) = fv2l{(long long)q[2], (long long)q[3]};
    }
}

// 3: the passing records of tile t to records [offset[t], offset[t] + count[t]) of the scratch batch, in record order.
__global__ __launch_bounds__(256) void kta_filter_scatter(FilterSource c, uint64_t n, FilterSpec f, const uint32_t *__restrict__ bitmap,
                                                          const uint32_t *__restrict__ count, const unsigned long long *__restrict__ offset,
                                                          FilterDest out)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_bitmap[];
    __shared__ uint32_t s_wave[kFilterWaves];
    const uint32_t t = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t cnt = count[t] & kFilterCountMask;
    if (cnt == 0) return;                        // (uniform)
    const unsigned long long off = offset[t];
    const FilterTileSpan s = filter_span(c, n, t);
    const bool all = cnt == (uint32_t)(s.hi - s.lo);   // every record of the tile inside the slice passes: copied straight through
    const kta_tile_hdr h = c.hdr ? c.hdr[s.T] : kta_tile_hdr{0, KTA_TILE_RAW, KTA_TILE_LENS_I32};
    if (cnt == KTA_TILE_RECORDS && (off & 3ull) == 0) {   // (uniform) a whole tile, 16-byte stores
        filter_copy_tile(c, h, s.T, off, out);
        return;
    }
    if (!all) filter_load_bitmap(f, bitmap, s_bitmap);
    __syncthreads();
    uint64_t ballot[4];
    filter_wave_ballots(c, f, s_bitmap, h, s, all, wave, lane, ballot);
    if (lane == 0) s_wave[wave] = (uint32_t)(__popcll(ballot[0]) + __popcll(ballot[1]) + __popcll(ballot[2]) + __popcll(ballot[3]));
    __syncthreads();
    uint32_t wave_base = 0;
    for (uint32_t w = 0; w < wave; w++) wave_base += s_wave[w];
    const uint16_t *g16 = reinterpret_cast<const uint16_t *>(c.key_len + s.T * KTA_TILE_RECORDS);   // (a u16 tile's groups)
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        if (!((ballot[k] >> lane) & 1ull)) continue;
        const uint32_t j = wave * 256u + k * 64u + lane;
        const uint64_t a = s.T * KTA_TILE_RECORDS + j;
        const uint32_t rank = filter_tile_rank(wave_base, ballot, k, lane);
        const unsigned long long d = off + rank;
        if (rank >= cnt || d >= out.capacity) continue;   // (never: the ballots are the count kernel's; a store stays below offset[t] + count[t])
        int32_t p;
        long long ts;
        tile_record_h<true>(c.partition, c.ts_ms, h, s.T, a, p, ts);
        const bool lens16 = h.lens == KTA_TILE_LENS_U16;
        const int32_t kl = lens16 ? tile_unpack_len(g16[tile_klen_slot(j)]) : c.key_len[a];
        const int32_t vl = lens16 ? tile_unpack_len(g16[tile_vlen_slot(j)]) : c.val_len[a];
        const uint64_t i = a - c.a0;             // the record's index in the slice
        out.partition[d] = p;
        out.ts_ms[d] = ts;
        out.key_len[d] = kl;
        out.val_len[d] = vl;
        if (out.key_off) out.key_off[d] = c.key_off[i];
        if (out.seq) out.seq[d] = c.seq ? c.seq[i] : c.base_seq + i;
    }
}

} // namespace

hipError_t launch_filter_count(const FilterSource &c, uint64_t n, const FilterSpec &f, const uint32_t *bitmap, const FilterWorkspace &ws, hipStream_t s)
{
    const uint64_t tiles = filter_slice_tiles(c.a0, n);
    if (tiles == 0 || tiles > kFilterMaxTiles) return hipErrorInvalidValue;
    const uint32_t lds = f.parts ? filter_bitmap_words(f.P) * 4u : 0u;
    if (lds > kFilterBitmapBytes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kta_filter_count, dim3((uint32_t)((tiles + kFilterGroup - 1) / kFilterGroup)), dim3(256), lds, s, c, n, f, bitmap, ws.count,
                       (uint32_t)tiles);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kta_filter_offsets, dim3(1), dim3(kFilterScanThreads), 0, s, ws.count, (uint32_t)tiles, reinterpret_cast<unsigned long long *>(ws.offset),
                       reinterpret_cast<unsigned long long *>(ws.stats), reinterpret_cast<unsigned long long *>(ws.total_host));
    return hipGetLastError();
}

hipError_t launch_filter_scatter(const FilterSource &c, uint64_t n, const FilterSpec &f, const uint32_t *bitmap, const FilterWorkspace &ws,
                                 const FilterDest &out, hipStream_t s)
{
    const uint64_t tiles = filter_slice_tiles(c.a0, n);
    if (tiles == 0 || tiles > kFilterMaxTiles) return hipErrorInvalidValue;
    const uint32_t lds = f.parts ? filter_bitmap_words(f.P) * 4u : 0u;
    hipLaunchKernelGGL(kta_filter_scatter, dim3((uint32_t)tiles), dim3(256), lds, s, c, n, f, bitmap, ws.count,
                       reinterpret_cast<const unsigned long long *>(ws.offset), out);
    return hipGetLastError();
}

} // namespace kta

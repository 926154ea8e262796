// kta_synth.hip — the synthetic topic source (include/kta_synth.h): host generator, device
// generator (HBM-resident batches for benchmarks) and the BASELINE.json config presets.
// Input generation only: nothing here is on the measured hot path.
#include "../../include/kta_synth.h"

#include "kta_internal.h"
#include "kta_tile.h"

#include <hip/hip_runtime.h>
#include <limits.h>
#include <string.h>

#include <string>

namespace {

constexpr int kWG = 256;
constexpr int kScanItems = 16;                 // records per thread in the offset scan
constexpr int kScanChunk = kWG * kScanItems;   // records per workgroup

__global__ __launch_bounds__(kWG) void synth_fill_cols(kta_synth_spec sp, uint64_t first, uint64_t n,
                                                       int32_t *part, int32_t *klen, int32_t *vlen,
                                                       int64_t *ts, uint64_t *seq)
{
    const uint64_t stride = (uint64_t)gridDim.x * kWG;
    for (uint64_t i = (uint64_t)blockIdx.x * kWG + threadIdx.x; i < n; i += stride) {
        int32_t p, kl, vl;
        int64_t t;
        kta_synth_record(&sp, first + i, &p, &kl, &vl, &t);
        part[i] = p;
        klen[i] = kl;
        vlen[i] = vl;
        ts[i] = t;
        if (seq) seq[i] = first + i;
    }
}

// The tile-compact layout (kta_hip.h): one workgroup per tile, 4 records per lane.  seq goes to the batch's own column;
// the four metric columns are reduced over the tile first — does every id fit a u16, do the timestamps span less than
// 2^31 ms, and (lens16: the allocation has no key columns) does every length fit a u16 — and then stored compact or raw
// into the allocation's tile t0 + T (part, klen, vlen, ts: the allocation's record 0), with its header.  One pass, as
// the raw fill.  A whole compact tile of which every record fits the scan plane (kta_tile.h) gets its plane, 4 B per
// record more, its two size extrema (reduced over the tile with the rest) and then its mark with the summary.
__global__ __launch_bounds__(kWG) void synth_fill_tiles(kta_synth_spec sp, uint64_t first, uint64_t n, int32_t *part,
                                                        int32_t *klen, int32_t *vlen, int64_t *ts, uint64_t *seq,
                                                        kta_tile_hdr *hdr, kta_tile_sum *sum, uint32_t *mark, uint32_t *size, uint64_t t0, uint32_t lens16)
{
    __shared__ long long s_red[kWG / 64][5];
    const uint32_t tid = threadIdx.x;
    const uint64_t ntiles = (n + KTA_TILE_RECORDS - 1) / KTA_TILE_RECORDS;
    for (uint64_t T = blockIdx.x; T < ntiles; T += gridDim.x) {
        int32_t p[4], kl[4], vl[4];
        int64_t t[4];
        long long lo = LLONG_MAX, hi = LLONG_MIN, wide = 0;   // wide: bit 0 a partition id, bit 1 a length outside the u16 form, bit 2 a record outside the plane's
        long long seen = 0;   // the summary's (real records only): bits 0-15 the largest stored u16 partition, bit 16 a timestamp of -1
        uint32_t slo = kta::kTileSizeMinNone, shi = kta::kTileSizeMaxNone;   // the size extrema (kta_tile.h; used only where the tile gets its mark)
        for (uint32_t j = 0; j < 4; j++) {
            const uint64_t i = T * KTA_TILE_RECORDS + 4u * tid + j;
            p[j] = -1;
            t[j] = -1;
            kl[j] = vl[j] = 0;
            if (i >= n) continue;
            kta_synth_record(&sp, first + i, &p[j], &kl[j], &vl[j], &t[j]);
            if (seq) seq[i] = first + i;
            wide |= kta::tile_part_fits(p[j]) ? 0 : 1;
            wide |= kta::tile_len_fits(kl[j]) && kta::tile_len_fits(vl[j]) ? 0 : 2;
            wide |= kta::tile_plane_fits(p[j], kl[j], vl[j]) ? 0 : 4;
            kta::tile_size_fold(kl[j], vl[j], slo, shi);
            const long long pm = kta::tile_pack_part(p[j]);
            seen = (seen & 0x10000) | ((seen & 0xFFFF) > pm ? (seen & 0xFFFF) : pm) | (t[j] == -1 ? 0x10000 : 0);
            if (t[j] != -1) {
                lo = t[j] < lo ? t[j] : lo;
                hi = t[j] > hi ? t[j] : hi;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const long long a = __shfl_xor(lo, off), b = __shfl_xor(hi, off), c = __shfl_xor(wide, off), d = __shfl_xor(seen, off);
            lo = a < lo ? a : lo;
            hi = b > hi ? b : hi;
            wide |= c;
            seen = ((seen | d) & 0x10000) | ((seen & 0xFFFF) > (d & 0xFFFF) ? (seen & 0xFFFF) : (d & 0xFFFF));
            slo = min(slo, (uint32_t)__shfl_xor((int)slo, off));
            shi = max(shi, (uint32_t)__shfl_xor((int)shi, off));
        }
        if ((tid & 63u) == 0u) {
            s_red[tid >> 6][0] = lo;
            s_red[tid >> 6][1] = hi;
            s_red[tid >> 6][2] = wide;
            s_red[tid >> 6][3] = seen;
            s_red[tid >> 6][4] = (long long)(((unsigned long long)slo << 32) | shi);
        }
        __syncthreads();
        for (uint32_t w = 0; w < kWG / 64; w++) {
            lo = s_red[w][0] < lo ? s_red[w][0] : lo;
            hi = s_red[w][1] > hi ? s_red[w][1] : hi;
            wide |= s_red[w][2];
            const long long d = s_red[w][3];
            seen = ((seen | d) & 0x10000) | ((seen & 0xFFFF) > (d & 0xFFFF) ? (seen & 0xFFFF) : (d & 0xFFFF));
            const unsigned long long e = (unsigned long long)s_red[w][4];
            slo = min(slo, (uint32_t)(e >> 32));
            shi = max(shi, (uint32_t)e);
        }
        __syncthreads();   // (s_red is reused by the next tile)
        int64_t base;
        const bool compact = kta::tile_ts_fits(lo, hi, &base) && !(wide & 1);
        const uint64_t A = (t0 + T) * KTA_TILE_RECORDS;   // the tile's first record in the allocation
        if (compact) {
            uint16_t u[4];
            int32_t o[4];
            for (uint32_t j = 0; j < 4; j++) {
                u[j] = kta::tile_pack_part(p[j]);
                o[j] = kta::tile_pack_ts(t[j], base);
            }
            reinterpret_cast<uint2 *>(part)[(2 * A) / 4 + tid] =
                make_uint2(kta::tile_u16x2_word(u[0], u[1]), kta::tile_u16x2_word(u[2], u[3]));
            reinterpret_cast<int4 *>(ts)[(2 * A) / 4 + tid] = make_int4(o[0], o[1], o[2], o[3]);
        } else {
            reinterpret_cast<int4 *>(part)[A / 4 + tid] = make_int4(p[0], p[1], p[2], p[3]);
            reinterpret_cast<longlong2 *>(ts)[A / 2 + 2 * tid] = make_longlong2(t[0], t[1]);
            reinterpret_cast<longlong2 *>(ts)[A / 2 + 2 * tid + 1] = make_longlong2(t[2], t[3]);
        }
        const bool u16 = lens16 && !(wide & 2);
        if (u16) {   // group tid: the lane's four key lengths, then its four value lengths
            using kta::tile_pack_len;
            reinterpret_cast<uint4 *>(klen)[A / 4 + tid] =
                make_uint4(kta::tile_u16x2_word(tile_pack_len(kl[0]), tile_pack_len(kl[1])), kta::tile_u16x2_word(tile_pack_len(kl[2]), tile_pack_len(kl[3])),
                           kta::tile_u16x2_word(tile_pack_len(vl[0]), tile_pack_len(vl[1])), kta::tile_u16x2_word(tile_pack_len(vl[2]), tile_pack_len(vl[3])));
        } else {     // (whole tiles: the allocation covers them, and the records past n are nobody's)
            reinterpret_cast<int4 *>(klen)[A / 4 + tid] = make_int4(kl[0], kl[1], kl[2], kl[3]);
            reinterpret_cast<int4 *>(vlen)[A / 4 + tid] = make_int4(vl[0], vl[1], vl[2], vl[3]);
        }
        // the plane: behind the offsets, in the second half of the tile's bytes of ts; only of a tile this call wrote whole
        const bool plane = mark && compact && !(wide & 4) && n - T * KTA_TILE_RECORDS >= KTA_TILE_RECORDS;
        if (plane)
            reinterpret_cast<uint4 *>(ts)[A / 2 + kta::kTilePlaneOffset / 16u + tid] =
                make_uint4(kta::tile_plane_pack(p[0], kl[0], vl[0]), kta::tile_plane_pack(p[1], kl[1], vl[1]),
                           kta::tile_plane_pack(p[2], kl[2], vl[2]), kta::tile_plane_pack(p[3], kl[3], vl[3]));
        if (tid == 0) {
            if (plane) size[2 * (t0 + T)] = slo, size[2 * (t0 + T) + 1] = shi;   // (before the mark that vouches for them; mark != null: so is size)
            if (mark) mark[t0 + T] = plane ? 1u : 0u;
            hdr[t0 + T] = kta_tile_hdr{compact ? base : 0, compact ? KTA_TILE_COMPACT : KTA_TILE_RAW, u16 ? KTA_TILE_LENS_U16 : KTA_TILE_LENS_I32};
            // the summary with the header (kta_tile.h): of a compact tile this call wrote whole, else none
            const uint64_t m = n - T * KTA_TILE_RECORDS < KTA_TILE_RECORDS ? n - T * KTA_TILE_RECORDS : KTA_TILE_RECORDS;
            if (sum) sum[t0 + T] = compact ? kta::tile_summary(lo, hi, (uint32_t)(seen & 0xFFFF), (seen & 0x10000) != 0, m) : kta_tile_sum{0, 0, 0};
        }
    }
}

__device__ __forceinline__ uint32_t klen_bytes(const int32_t *klen, uint64_t i, uint64_t n)
{
    if (i >= n) return 0u;
    const int32_t k = klen[i];
    return k > 0 ? (uint32_t)k : 0u;
}

// phase A: per-chunk byte totals
__global__ __launch_bounds__(kWG) void synth_chunk_sums(const int32_t *klen, uint64_t n, uint64_t *chunk_sum)
{
    __shared__ uint64_t s[kWG];
    const uint64_t base = (uint64_t)blockIdx.x * kScanChunk + (uint64_t)threadIdx.x * kScanItems;
    uint64_t t = 0;
    for (int j = 0; j < kScanItems; j++) t += klen_bytes(klen, base + j, n);
    s[threadIdx.x] = t;
    __syncthreads();
    for (int off = kWG / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) chunk_sum[blockIdx.x] = s[0];
}

// phase B: exclusive scan of the chunk totals (one workgroup; each thread owns a contiguous span)
__global__ __launch_bounds__(1024) void synth_scan_chunks(uint64_t *chunk_sum, uint64_t n_chunks, uint64_t *total)
{
    __shared__ uint64_t s[1024];
    const uint64_t per = (n_chunks + 1023) / 1024;
    const uint64_t b = (uint64_t)threadIdx.x * per;
    const uint64_t e = b + per < n_chunks ? b + per : n_chunks;
    uint64_t t = 0;
    for (uint64_t i = b; i < e; i++) t += chunk_sum[i];
    s[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = 0;
        for (int i = 0; i < 1024; i++) {
            const uint64_t v = s[i];
            s[i] = run;
            run += v;
        }
        *total = run;
    }
    __syncthreads();
    uint64_t run = s[threadIdx.x];
    for (uint64_t i = b; i < e; i++) {
        const uint64_t v = chunk_sum[i];
        chunk_sum[i] = run;
        run += v;
    }
}

// phase C: batch-local key offsets (packed in record order)
__global__ __launch_bounds__(kWG) void synth_key_offsets(const int32_t *klen, uint64_t n, const uint64_t *chunk_off,
                                                         uint32_t *key_off)
{
    __shared__ uint64_t s[kWG];
    const uint64_t base = (uint64_t)blockIdx.x * kScanChunk + (uint64_t)threadIdx.x * kScanItems;
    uint32_t len[kScanItems];
    uint64_t t = 0;
    for (int j = 0; j < kScanItems; j++) {
        len[j] = klen_bytes(klen, base + j, n);
        t += len[j];
    }
    s[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = chunk_off[blockIdx.x];
        for (int i = 0; i < kWG; i++) {
            const uint64_t v = s[i];
            s[i] = run;
            run += v;
        }
    }
    __syncthreads();
    uint64_t run = s[threadIdx.x];
    for (int j = 0; j < kScanItems; j++) {
        if (base + j < n) key_off[base + j] = (uint32_t)run;
        run += len[j];
    }
}

__global__ __launch_bounds__(kWG) void synth_fill_keys(kta_synth_spec sp, uint64_t first, uint64_t n,
                                                       const int32_t *klen, const uint32_t *key_off,
                                                       uint8_t *key_bytes)
{
    const uint64_t stride = (uint64_t)gridDim.x * kWG;
    for (uint64_t i = (uint64_t)blockIdx.x * kWG + threadIdx.x; i < n; i += stride) {
        const int32_t kl = klen[i];
        if (kl <= 0) continue;
        const uint64_t kid = (uint64_t)kta_synth_key_id(&sp, first + i);
        uint8_t *dst = key_bytes + key_off[i];
        for (uint32_t w = 0; w * 8u < (uint32_t)kl; w++) {
            uint64_t word = kta_synth_key_word(&sp, kid, w);
            const uint32_t m = (uint32_t)kl - w * 8u < 8u ? (uint32_t)kl - w * 8u : 8u;
            for (uint32_t j = 0; j < m; j++) {
                dst[w * 8u + j] = (uint8_t)word;
                word >>= 8;
            }
        }
    }
}

int check_spec(const kta_synth_spec *sp)
{
    if (!sp) return KTA_ERR_INVALID;
    if (sp->n_partitions == 0 || sp->shard_count == 0 || sp->shard_index >= sp->shard_count) return KTA_ERR_INVALID;
    if (kta_synth_local_partitions(sp) == 0) return KTA_ERR_INVALID;
    if (sp->n_key_lens == 0 || sp->n_key_lens > KTA_SYNTH_MAX_KEY_LENS) return KTA_ERR_INVALID;
    if (sp->key_null_permille > 1000 || sp->tombstone_permille + sp->val_empty_permille > 1000) return KTA_ERR_INVALID;
    return KTA_OK;
}

} // namespace

extern "C" {

int kta_synth_fill_host(const kta_synth_spec *spec, uint64_t first, uint64_t n, const kta_batch *b,
                        uint64_t *n_key_bytes)
{
    int rc = check_spec(spec);
    if (rc != KTA_OK || !b) return KTA_ERR_INVALID;
    if (n > b->capacity) return KTA_ERR_CAPACITY;
    uint64_t kb = 0;
    for (uint64_t i = 0; i < n; i++) {
        int32_t p, kl, vl;
        int64_t t;
        kta_synth_record(spec, first + i, &p, &kl, &vl, &t);
        b->partition[i] = p;
        b->key_len[i] = kl;
        b->val_len[i] = vl;
        b->ts_ms[i] = t;
        if (b->seq) b->seq[i] = first + i;
        if (b->key_off) {
            if (kb >= (1ull << 32)) return KTA_ERR_CAPACITY;
            b->key_off[i] = (uint32_t)kb;
        }
        if (kl > 0) {
            if (b->key_bytes) {
                if (kb + (uint64_t)kl > b->key_bytes_capacity) return KTA_ERR_CAPACITY;
                const uint64_t kid = (uint64_t)kta_synth_key_id(spec, first + i);
                for (uint32_t j = 0; j < (uint32_t)kl; j++) b->key_bytes[kb + j] = kta_synth_key_byte(spec, kid, j);
            }
            kb += (uint64_t)kl;
        }
    }
    if (n_key_bytes) *n_key_bytes = kb;
    return KTA_OK;
}

int kta_synth_fill_device(kta_ctx *ctx, const kta_synth_spec *spec, uint64_t first, uint64_t n,
                          const kta_batch *b, uint64_t *n_key_bytes)
{
    if (!ctx || !b) return KTA_ERR_INVALID;
    if (check_spec(spec) != KTA_OK) return fail(ctx, KTA_ERR_INVALID, "invalid synthetic spec");
    if (n > b->capacity) return fail(ctx, KTA_ERR_CAPACITY, "synthetic batch larger than the device batch capacity");
    if (n_key_bytes) *n_key_bytes = 0;
    if (n == 0) return KTA_OK;
    hipStream_t s = kta_internal_stream(ctx);
    KTA_HIP(ctx, hipSetDevice(kta_internal_device(ctx)));
    const uint32_t grid = (uint32_t)((n + kWG - 1) / kWG < 8192 ? (n + kWG - 1) / kWG : 8192);
    // a tile-compact batch from a tile boundary takes the compact fill; anything else the raw one (its tiles made raw first)
    kta_internal_columns ac{};
    if (int rc = kta_internal_resolve(ctx, b, &ac)) return rc;
    kta_tile_hdr *ahdr = ac.hdr;
    const uint64_t rec0 = ac.rec0;
    if (ahdr && rec0 % KTA_TILE_RECORDS != 0) {
        if (int rc = kta_internal_prepare_raw(ctx, b, n)) return rc;
        ahdr = nullptr;
    }
    if (ahdr) {
        const uint64_t nt = (n + KTA_TILE_RECORDS - 1) / KTA_TILE_RECORDS;
        // u16 lengths only where no kernel reads lengths next to keys: an allocation without key columns, and no key columns
        // of the caller's own beside it
        const uint32_t lens16 = ac.keyless && !b->key_off && !b->key_bytes ? 1u : 0u;
        hipLaunchKernelGGL(synth_fill_tiles, dim3((uint32_t)(nt < 8192 ? nt : 8192)), dim3(kWG), 0, s, *spec, first, n, ac.partition,
                           ac.key_len, ac.val_len, ac.ts_ms, b->seq, ahdr, ac.sum, ac.mark, ac.size, rec0 / KTA_TILE_RECORDS, lens16);
    } else {
        hipLaunchKernelGGL(synth_fill_cols, dim3(grid), dim3(kWG), 0, s, *spec, first, n, b->partition, b->key_len,
                           b->val_len, b->ts_ms, b->seq);
    }
    KTA_HIP(ctx, hipGetLastError());
    uint64_t total = 0;
    if (b->key_off && b->key_bytes) {
        const uint64_t n_chunks = (n + kScanChunk - 1) / kScanChunk;
        DeviceBuf<uint64_t> chunks;   // (released on every return; hipFree waits for the device first)
        // This allocation answers KTA_ERR_HIP also when it runs out of memory (everywhere else in the library that is
        // KTA_ERR_NOMEM): callers have seen that code from here since the function exists, and it stays.
        if (hipError_t e = chunks.alloc(n_chunks + 1))
            return fail(ctx, KTA_ERR_HIP, std::string("chunks.alloc(n_chunks + 1): ") + hipGetErrorString(e));
        uint64_t *const d_chunks = chunks.get();
        hipLaunchKernelGGL(synth_chunk_sums, dim3((uint32_t)n_chunks), dim3(kWG), 0, s, b->key_len, n, d_chunks);
        hipLaunchKernelGGL(synth_scan_chunks, dim3(1), dim3(1024), 0, s, d_chunks, n_chunks, d_chunks + n_chunks);
        KTA_HIP(ctx, hipGetLastError());
        KTA_HIP(ctx, hipMemcpyAsync(&total, d_chunks + n_chunks, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        KTA_HIP(ctx, hipStreamSynchronize(s));
        if (total > b->key_bytes_capacity || total >= (1ull << 32)) {
            if (n_key_bytes) *n_key_bytes = total;
            return fail(ctx, KTA_ERR_CAPACITY, "synthetic key bytes exceed the device batch key capacity");
        }
        hipLaunchKernelGGL(synth_key_offsets, dim3((uint32_t)n_chunks), dim3(kWG), 0, s, b->key_len, n, d_chunks,
                           b->key_off);
        hipLaunchKernelGGL(synth_fill_keys, dim3(grid), dim3(kWG), 0, s, *spec, first, n, b->key_len, b->key_off,
                           b->key_bytes);
        KTA_HIP(ctx, hipGetLastError());
        KTA_HIP(ctx, hipStreamSynchronize(s));
    }
    if (n_key_bytes) *n_key_bytes = total;
    return KTA_OK;
}

// The five BASELINE.json configs made concrete.  Mean record =
// key (~61 B incl. nulls) + value (~195 B incl. tombstones) ~ 256 B for the mixed law.
int kta_synth_preset(const char *name, kta_synth_spec *sp, uint64_t *n_records)
{
    if (!name || !sp) return KTA_ERR_INVALID;
    memset(sp, 0, sizeof(*sp));
    sp->shard_index = 0;
    sp->shard_count = 1;
    sp->ts_base_ms = 1600000000000ll;
    uint64_t n = 0;
    auto mixed = [&]() {
        sp->key_null_permille = 50;
        sp->key_empty_permille = 10;
        sp->n_key_lens = 5;
        const uint32_t lens[5] = {8, 16, 36, 64, 200};
        for (int i = 0; i < 5; i++) sp->key_lens[i] = lens[i];
        sp->tombstone_permille = 50;
        sp->val_empty_permille = 10;
        sp->val_mode = KTA_VAL_EXP;
        sp->val_mean = 208;
        sp->val_cap = 65536;
        sp->ts_missing_permille = 1;
        sp->ts_step_us = 10;
        sp->ts_jitter_ms = 3600000;
        sp->part_mode = KTA_PART_RANDOM;
    };
    auto keyed16 = [&](uint64_t distinct, uint32_t tomb_permille) {
        sp->key_null_permille = 0;
        sp->key_empty_permille = 0;
        sp->n_key_lens = 1;
        sp->key_lens[0] = 16;
        sp->n_distinct_keys = distinct;
        sp->tombstone_permille = tomb_permille;
        sp->val_mode = KTA_VAL_FIXED;
        sp->val_mean = 240;
        sp->ts_step_us = 10;
        sp->ts_jitter_ms = 1000;
        sp->part_mode = KTA_PART_KEY_AFFINE;
    };
    if (!strcmp(name, "c1")) { // 1 partition, 1M records, 64 B keys, 256 B values, no nulls
        sp->seed = 1; sp->n_partitions = 1; n = 1000000ull;
        sp->n_key_lens = 1; sp->key_lens[0] = 64; sp->n_distinct_keys = 1000000ull;
        sp->val_mode = KTA_VAL_FIXED; sp->val_mean = 256; sp->ts_step_us = 1000;
        sp->part_mode = KTA_PART_RANDOM;
    } else if (!strcmp(name, "c2")) { // 8 partitions, 100M records, mixed sizes
        sp->seed = 2; sp->n_partitions = 8; n = 100000000ull; mixed();
        sp->n_distinct_keys = 50000000ull;
    } else if (!strcmp(name, "c3")) { // 64 partitions, 1B records, -c, 10M distinct 16 B keys
        sp->seed = 3; sp->n_partitions = 64; n = 1000000000ull; keyed16(10000000ull, 100);
    } else if (!strcmp(name, "c4")) { // 256 partitions, 1B records, mixed sizes, 8-way sharded
        sp->seed = 4; sp->n_partitions = 256; n = 1000000000ull; mixed();
        sp->n_distinct_keys = 100000000ull;
    } else if (!strcmp(name, "c5")) { // 256 partitions, 10B records, -c, 100M keys, 50% tombstones
        sp->seed = 5; sp->n_partitions = 256; n = 10000000000ull; keyed16(100000000ull, 500);
    } else {
        return KTA_ERR_INVALID;
    }
    if (n_records) *n_records = n;
    return KTA_OK;
}

} // extern "C"

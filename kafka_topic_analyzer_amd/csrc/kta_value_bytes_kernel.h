// kta_value_bytes_kernel.h — the value-byte section's kernel (kta_value_bytes, KTA_FLAG_VALUE_BYTES).  kta_value_bytes.hip
// includes this file INSIDE its unnamed namespace, behind kta_decode_coop.h (pin, load_block, KTA_READLANE); beside
// kta_wave_src.h it has no includes of its own: the including file has included kta_filter.h, kta_kafka.h, kta_value_bytes.h
// and kta_records.h (at file scope) and provides the HIP runtime — or, for the CPU suite, tests/native/wave_emu.h
// (tests/native/value_bytes_emu.cpp, tests/test_value_bytes_emu.py): the kernel below is then the very source the GPU runs.
// What the kernel does is said at the top of kta_value_bytes.hip.  The walk of a batch — the descriptor, the window, the
// chain, the parse, the commit rule, the advance — is kta_record_walk.h's, statement for statement, kept here as text: over
// that header this kernel measured up to 2.2 % slower (profiles/record_walk_bench_ab.jsonl).
#pragma once

#ifndef KTA_BALLOT64    // the lanes (of those that call it together) whose predicate holds.  (wave_emu.h: a meeting point.)
#define KTA_BALLOT64(p) ((uint64_t)__builtin_amdgcn_ballot_w64(p))
#endif
#ifndef KTA_UNI         // a value every lane holds alike, moved to a scalar register (the emulator: the value)
#define KTA_UNI(v) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(v)))
#endif

#include "kta_wave_src.h"

constexpr int kVbG = 4;                         // batches per wave
constexpr uint32_t kVbW = 3072;                 // window bytes
constexpr uint32_t kVbR = 16;                   // records per round of a group
constexpr uint32_t kVbL = 64 / kVbG;            // lanes per batch
constexpr uint32_t kVbNLoad = kVbW / (kVbL * 16);
constexpr uint32_t kVbPer = kVbW / 1024;
constexpr uint32_t kVbWavesPerCu = 8;           // resident workgroups per CU (16.6 KiB of LDS each; the grid is that many per CU at most)
// A group's 32-bit bins take at most this many bytes between two flushes: a bin can receive every one of them, so any bound
// below 2^32 keeps it from wrapping; 2^31 leaves the sum of the four groups' bins of one flush below 2^33, held in 64 bits.
constexpr uint32_t kVbFlushBytes = 0x80000000u;
enum VbInfoWord : uint32_t { kVbInfoMidFlushes = 0, kVbInfoPartitionFlushes = 1, kVbInfoWords = 4 };
static_assert(kVbR == kVbL && kVbL == kWsL && kta::rec::line_windows(kVbW), "one parse round; KiB loads");
static_assert(kVbBins % 64 == 0 && kVbBins % kVbL == 0, "the flush strides the bins by the wave and by the group");

// What a lane keeps in registers for the batches of ONE partition (part; -1: nothing yet) since the last flush; the bins of
// its group lie in LDS.
struct VbAcc {
    int32_t part;
    uint64_t records, values, bytes, repeats;
};

// The four bytes of `word`, whose byte 0 lies at position pos0 of the blob: those at positions in [lo, hi) go to the bins;
// one behind `first` (the value's first byte) that equals the byte in front of it is a repeat.  prev: the byte at pos0 - 1
// (any value when pos0 <= first).  COMBINE: kVbCombineNone every byte its own add; kVbCombineDword a dword of four equal bytes
// one add of 4, every other dword four adds; kVbCombinePairs equal bytes of the dword are added once, with their count.
enum VbCombine : uint32_t { kVbCombineNone = 0, kVbCombinePairs = 1, kVbCombineDword = 2 };
template <uint32_t COMBINE>
__device__ __forceinline__ void vb_dword(uint32_t word, uint32_t prev, uint64_t pos0, uint64_t lo, uint64_t hi, uint64_t first, uint32_t *bins, uint64_t &repeats)
{
    uint32_t b[4];
    bool valid[4];
    uint32_t rep = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        b[j] = (word >> (8u * j)) & 0xFFu;
        valid[j] = pos0 + j >= lo && pos0 + j < hi;
        rep += valid[j] && pos0 + j > first && b[j] == (j ? b[j - 1] : prev) ? 1u : 0u;
    }
    repeats += rep;
    if (COMBINE == kVbCombineDword && valid[0] && valid[3] && word == b[0] * 0x01010101u) {   // ([lo, hi) is one range: all four are valid)
        atomicAdd(&bins[b[0]], 4u);
        return;
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        if (COMBINE != kVbCombinePairs) {
            if (valid[j]) atomicAdd(&bins[b[j]], 1u);
            continue;
        }
        bool leader = valid[j];
        uint32_t count = 1;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            if (i < j) leader = leader && !(valid[i] && b[i] == b[j]);
            if (i > j) count += valid[i] && b[i] == b[j] ? 1u : 0u;
        }
        if (leader) atomicAdd(&bins[b[j]], count);
    }
}

// The bytes [a, b) of a value that begins at `first`, added by the sixteen lanes of its group: what lies inside the window
// [wbase, win_end) in dwords from LDS, a lane per dword; what lies behind it in 16-byte blocks from the blob, a lane per block.
// The byte in front of a dword or a block is read where the dword or block is read from: a seam between two lanes, between
// the window and the blob, or between two calls decides nothing.
template <uint32_t COMBINE>
__device__ __forceinline__ void vb_slice(const uint4 *blocks, const uint8_t *win, uint64_t wbase, uint64_t win_end, uint64_t first, uint64_t a, uint64_t b,
                                         uint32_t sub, uint32_t *bins, uint64_t &repeats)
{
    if (a < win_end) {                                                         // (then wbase <= first <= a)
        const uint32_t *w32 = reinterpret_cast<const uint32_t *>(win);
        const uint64_t hi = b < win_end ? b : win_end;
        const uint32_t d_last = (uint32_t)(hi - 1 - wbase) >> 2;
        for (uint32_t d = ((uint32_t)(a - wbase) >> 2) + sub; d <= d_last; d += kVbL) {
            const uint64_t pos0 = wbase + 4ull * d;
            const uint32_t prev = pos0 > first ? win[4u * d - 1u] : 0u;
            vb_dword<COMBINE>(w32[d], prev, pos0, a, hi, first, bins, repeats);
        }
    }
    const uint64_t lo = a > win_end ? a : win_end;
    if (lo < b) {
        const uint8_t *bytes = reinterpret_cast<const uint8_t *>(blocks);
        const uint64_t q_last = (b - 1) >> 4;
        for (uint64_t q = (lo >> 4) + sub; q <= q_last; q += kVbL) {
            const uint64_t pos0 = q << 4;
            const uint4 blk = load_block(bytes + pos0);
            const uint32_t prev = pos0 > first ? bytes[pos0 - 1] : 0u;
            vb_dword<COMBINE>(blk.x, prev, pos0, lo, b, first, bins, repeats);
            vb_dword<COMBINE>(blk.y, blk.x >> 24, pos0 + 4, lo, b, first, bins, repeats);
            vb_dword<COMBINE>(blk.z, blk.y >> 24, pos0 + 8, lo, b, first, bins, repeats);
            vb_dword<COMBINE>(blk.w, blk.z >> 24, pos0 + 12, lo, b, first, bins, repeats);
        }
    }
}

// The bins of every group and the lanes' words added to the vector and cleared; every lane calls it (barriers, cross-lane
// sums).  When every group that holds something holds it for one partition — a blob is one partition in the pipeline — the
// four groups' bins are summed first and the wave adds 256 + 4 words; otherwise each group adds the words of its partition.
__device__ __forceinline__ void vb_flush(VbAcc &a, uint32_t (*s_bins)[kVbBins], unsigned long long *vec, uint32_t lane)
{
    const uint32_t g = lane / kVbL, sub = lane % kVbL;
    __syncthreads();
    const uint64_t holders = KTA_BALLOT64(a.part >= 0);
    if (holders == 0ull) return;                                              // (uniform; the bins are clear)
    const uint32_t first = KTA_UNI((uint32_t)__builtin_ctzll(holders));
    const int32_t p0 = (int32_t)KTA_READLANE((uint32_t)a.part, first);
    const bool one = KTA_BALLOT64(a.part >= 0 && a.part != p0) == 0ull;       // (uniform)
    const uint64_t words[4] = {one ? wave_sum(a.records) : group_sum(a.records), one ? wave_sum(a.values) : group_sum(a.values),
                               one ? wave_sum(a.bytes) : group_sum(a.bytes), one ? wave_sum(a.repeats) : group_sum(a.repeats)};
    const uint32_t slot = one ? lane : sub;
    uint64_t mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) mine = slot == k ? words[k] : mine;
    if (one) {
        unsigned long long *pw = vec + (size_t)kVbPartitionWords * (uint32_t)p0;
        for (uint32_t b = lane; b < kVbBins; b += 64) {
            uint64_t c = 0;
#pragma unroll
            for (int gg = 0; gg < kVbG; gg++) c += s_bins[gg][b];
            if (c) atomicAdd(pw + b, (unsigned long long)c);
        }
        if (lane < 4 && mine) atomicAdd(pw + kVbRecords + lane, (unsigned long long)mine);
    } else if (a.part >= 0) {
        unsigned long long *pw = vec + (size_t)kVbPartitionWords * (uint32_t)a.part;
        for (uint32_t b = sub; b < kVbBins; b += kVbL) {
            const uint32_t c = s_bins[g][b];
            if (c) atomicAdd(pw + b, (unsigned long long)c);
        }
        if (sub < 4 && mine) atomicAdd(pw + kVbRecords + sub, (unsigned long long)mine);
    }
    __syncthreads();
    uint32_t *flat = &s_bins[0][0];                                            // (the four groups' bins lie one behind the other)
    for (uint32_t b = lane; b < kVbG * kVbBins; b += 64) flat[b] = 0u;
    __syncthreads();
    a.part = -1, a.records = a.values = a.bytes = a.repeats = 0;
}

// grid: the number of workgroups; workgroup w takes the batches 4 q .. 4 q + 3 for q = w, w + grid, ...
// FLUSH: the bytes a group's bins take between two flushes (kVbFlushBytes; the CPU suite instantiates it small).
template <uint32_t FLUSH, uint32_t COMBINE>
__global__ __launch_bounds__(64) KTA_WAVES_PER_EU(2, 8) void kta_value_bytes(const uint4 *blocks, const kta_kafka_batch_desc *descs, uint64_t n_batches,
                                                                           uint32_t P, FilterSpec f, const uint32_t *bitmap, unsigned long long *vec,
                                                                           unsigned long long *info, uint32_t grid)
{
    namespace rec = kta::rec;
    constexpr int G = kVbG;
    constexpr uint32_t W = kVbW, R = kVbR, L = kVbL, NLOAD = kVbNLoad, PER = kVbPer;
    static_assert(FLUSH > 0, "a slice of a value has at least one byte");
    __shared__ uint4 s_win[G][W / 16 + 1];        // + 1: the register paths read whole dwords up to 16 bytes ahead
    __shared__ uint32_t s_start[G][R + 1];
    __shared__ uint64_t s_next[G];
    __shared__ uint32_t s_found[G], s_first_incomplete[G], s_first_bad[G];
    __shared__ uint64_t s_vpos[G][R], s_vlen[G][R];   // the round's committed values: where they begin, their bytes (0: nothing to add)
    __shared__ uint32_t s_bins[G][kVbBins];
    const uint32_t lane = threadIdx.x, g = lane / L, sub = lane % L;
    const uint8_t *win = reinterpret_cast<const uint8_t *>(s_win[g]);
    for (uint32_t b = lane; b < G * kVbBins; b += 64) (&s_bins[0][0])[b] = 0u;
    VbAcc acc;
    acc.part = -1, acc.records = acc.values = acc.bytes = acc.repeats = 0;
    uint64_t since = 0;                                 // the bytes this group has put into its bins since the last flush (uniform inside a group)
    uint32_t mid_flushes = 0, partition_flushes = 0;
    __syncthreads();
  for (uint64_t quad = blockIdx.x; quad * G < n_batches; quad += grid) {      // (uniform)
    const uint64_t b = quad * G + g;
    uint64_t end = 0, pos = 0;
    int64_t ts_base = 0, ts_mask = 0;
    uint32_t total = 0, j = 0;
    int32_t partition = 0;
    bool counted = false;                                 // the batch: status 0, partition in [0, P) and in the filter's set
    if (b < n_batches) {
        const kta_kafka_batch_desc &d = descs[b];
        end = d.payload_end; pos = d.payload_off;
        const bool append_time = (d.flags & KTA_KB_LOG_APPEND_TIME) != 0;   // every record carries maxTimestamp
        ts_base = append_time ? d.max_ts_ms : d.base_ts_ms;
        ts_mask = append_time ? 0 : -1;
        total = d.n_records > 0 ? (uint32_t)d.n_records : 0u; partition = d.partition;
        counted = d.status == 0 && (uint32_t)partition < P &&
                  (!f.parts || ((bitmap[(uint32_t)partition >> 5] >> ((uint32_t)partition & 31u)) & 1u));
    }
    // a group's bins hold one partition: another one first sends them to the vector (every lane takes part)
    if (__any(counted && acc.part >= 0 && acc.part != partition)) {
        vb_flush(acc, s_bins, vec, lane);
        since = 0;
        partition_flushes += lane == 0 ? 1u : 0u;
    }
    if (counted) acc.part = partition;
    bool run = counted && j < total;                      // uniform inside a group
    while (__any(run)) {
        uint64_t wbase = 0;
        uint32_t limit = 0, end_rel = 0;
        bool to_the_end = false;
        uint64_t load_base = 0;                           // a group that does not run reads the blob's first block into its own window
        uint32_t load_bytes = 16;
        if (run && pos >= end) run = false;               // (the count promises more records than the batch holds: nothing more)
        if (run) {
            wbase = rec::window_base(pos, W);
            const uint64_t span = ((end + 15) & ~15ull) - wbase, rest = end - wbase;
            const uint32_t wbytes = span < W ? (uint32_t)span : W;         // a multiple of 16, at least 16
            to_the_end = rest <= wbytes;
            limit = to_the_end ? (uint32_t)rest : wbytes;
            end_rel = rest < 0xF0000000ull ? (uint32_t)rest : 0xF0000000u;
            load_base = wbase; load_bytes = wbytes;
            if (sub == 0) { s_first_bad[g] = R + 1; s_first_incomplete[g] = R; }
        }
        {
            uint4 stage[NLOAD];
#pragma unroll
            for (uint32_t u = 0; u < NLOAD; u++) {
                const uint32_t gg = u / PER, c = u % PER;
                const uint64_t gb = (uint64_t)KTA_READLANE((uint32_t)load_base, gg * L) |
                                    ((uint64_t)KTA_READLANE((uint32_t)(load_base >> 32), gg * L) << 32);
                const uint32_t gbytes = KTA_READLANE(load_bytes, gg * L);
                const uint32_t o = (c * 64 + lane) * 16;
                stage[u] = load_block(reinterpret_cast<const uint8_t *>(blocks) + gb + (o < gbytes - 16 ? o : gbytes - 16));
            }
#pragma unroll
            for (uint32_t u = 0; u < NLOAD; u++) pin(stage[u]);
#pragma unroll
            for (uint32_t u = 0; u < NLOAD; u++) s_win[u / PER][(u % PER) * 64 + lane] = stage[u];
        }
        __syncthreads();
        if (run && sub == 0) {                                                 // chain the length prefixes
            const uint32_t *w32 = reinterpret_cast<const uint32_t *>(win);
            const uint32_t want = total - j < R ? total - j : R;
            uint32_t k = 0, cur = (uint32_t)(pos - wbase);
            uint64_t next = 0;
            if (rec::chain(w32, limit, want, s_start[g], k, cur)) {            // a length of three bytes or more: byte by byte
                uint32_t off = cur;
                long long len;
                if (rec::window_varlong(win, off, limit, len)) {
                    const uint64_t rec_end = wbase + off + (uint64_t)len;
                    if (len < 0 || rec_end > end) s_first_bad[g] = k;
                    else { s_start[g][k++] = cur; next = rec_end; }
                } else if (to_the_end) {
                    s_first_bad[g] = k;                                        // ran into the end of the batch
                }                                                              // (else it straddles the window: next round)
            }
            if (!next) next = wbase + cur;
            const uint64_t next_rel = next - wbase;
            s_start[g][k] = next_rel < 0xFFFFFFFFull ? (uint32_t)next_rel : 0xFFFFFFFFu;
            s_found[g] = k;
            s_next[g] = next;
        }
        __syncthreads();
        // this lane's record of the round, held until the round knows how far it commits
        bool have = false;
        uint64_t value = 0, vb = 0;
        if (run && sub < s_found[g]) {
            const uint32_t k = sub;
            const uint32_t start = s_start[g][k], rec_end = s_start[g][k + 1];
            if (rec_end > end_rel) {                                           // the record overruns the batch
                atomicMin(&s_first_bad[g], k);
            } else {
                BlockSrc src{blocks, ~0ull, make_uint4(0, 0, 0, 0)};
                const uint64_t rec_end_abs = wbase + rec_end;
                rec::Record r;
                uint32_t verdict = rec::parse_record(win, start, rec_end, limit, r);
                value = wbase + r.after;                                       // where the value's bytes begin
                if (verdict == rec::REC_VALUE_LENGTH_OUTSIDE) {                // behind a key of the window's size
                    verdict = payload_varlong(src, value, rec_end_abs, r.val_len) ? rec::value_fits(r.val_len, value - wbase, rec_end) : rec::REC_BAD;
                }
                if (verdict == rec::REC_INCOMPLETE) atomicMin(&s_first_incomplete[g], k);
                else if (verdict != rec::REC_OK) atomicMin(&s_first_bad[g], k);
                else if (filter_time_passes(f, ts_base + (r.ts_delta & ts_mask))) {
                    have = true;
                    vb = r.val_len > 0 ? (uint64_t)r.val_len : 0ull;
                }
            }
        }
        __syncthreads();
        // COMMIT: only the records in front of the round's first incomplete and first bad one; their values go to the group
        uint32_t n_commit = 0;
        if (run) {
            const uint32_t found = s_found[g], first_inc = s_first_incomplete[g], first_bad = s_first_bad[g];
            const uint32_t done = first_inc < found ? first_inc : found;
            n_commit = first_bad < done ? first_bad : done;
            const bool mine = have && sub < n_commit;
            if (mine) acc.records++, acc.values += vb != 0, acc.bytes += vb;
            s_vpos[g][sub] = value, s_vlen[g][sub] = mine ? vb : 0ull;
        }
        __syncthreads();
        // the round's values, one after the other, each by the sixteen lanes of its group, in slices of FLUSH bytes at most
        const uint64_t win_end = wbase + limit;
        for (uint32_t k = 0; __any(k < n_commit); k++) {                       // (uniform)
            const uint64_t first = k < n_commit ? s_vpos[g][k] : 0ull, len = k < n_commit ? s_vlen[g][k] : 0ull;
            uint64_t off = 0;
            while (__any(off < len)) {
                const uint64_t rest = len - off, n = rest < FLUSH ? rest : FLUSH;
                if (__any(n != 0 && since + n > FLUSH)) {                      // a 32-bit bin could overflow: the bins go to the vector
                    vb_flush(acc, s_bins, vec, lane);
                    since = 0;
                    mid_flushes += lane == 0 ? 1u : 0u;
                    if (counted) acc.part = partition;
                }
                if (n) {
                    vb_slice<COMBINE>(blocks, win, wbase, win_end, first, first + off, first + off + n, sub, s_bins[g], acc.repeats);
                    since += n, off += n;
                }
            }
        }
        if (run) {
            const uint32_t found = s_found[g], first_inc = s_first_incomplete[g], first_bad = s_first_bad[g];
            const uint32_t done = first_inc < found ? first_inc : found;
            if (first_bad <= done || done == 0) {                              // bad framing, or no progress (a truncated batch): the batch ends here
                run = false;
            } else {
                j += done;
                pos = done < found ? wbase + s_start[g][done] : s_next[g];     // records >= done are redone
                run = j < total;
            }
        }
        __syncthreads();
    }
  }
    vb_flush(acc, s_bins, vec, lane);
    const uint64_t mids = wave_sum(mid_flushes), parts = wave_sum(partition_flushes);
    const uint64_t work = lane == kVbInfoMidFlushes ? mids : lane == kVbInfoPartitionFlushes ? parts : 0ull;
    if (lane < kVbInfoWords && work) atomicAdd(info + lane, (unsigned long long)work);
}

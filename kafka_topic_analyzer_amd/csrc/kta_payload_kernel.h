// kta_payload_kernel.h — the payload section's kernel (kta_payload, KTA_FLAG_PAYLOAD).  kta_payload.hip includes this file
// INSIDE its unnamed namespace, behind kta_decode_coop.h (pin, load_block, KTA_READLANE); beside kta_wave_src.h and kta_record_walk.h — the
// walk over a batch's records: the window, the chain, the parse, the commit rule — it has no includes of its own: the
// including file has included kta_filter.h, kta_kafka.h, kta_payload.h and kta_records.h (at file scope) and provides the
// HIP runtime — or, for the CPU suite, tests/native/wave_emu.h, which runs the 64 lanes of a workgroup as fibers that meet at
// __syncthreads / __any / __shfl_xor / ballots (tests/native/payload_emu.cpp, tests/test_payload_emu.py): the kernel below is
// then the very source the GPU runs.  What the kernel does is said at the top of kta_payload.hip.
#pragma once

#ifndef KTA_BALLOT64    // the lanes (of those that call it together) whose predicate holds.  (wave_emu.h: a meeting point.)
#define KTA_BALLOT64(p) ((uint64_t)__builtin_amdgcn_ballot_w64(p))
#endif
#ifndef KTA_UNI         // a value every lane holds alike, moved to a scalar register (the emulator: the value)
#define KTA_UNI(v) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(v)))
#endif

#include "kta_wave_src.h"       // BlockSrc, WindowSrc, group_sum, wave_sum
#include "kta_record_walk.h"    // the batch, the round's window, chain and parse, the commit rule, the advance

constexpr int kPlG = 4;                         // batches per wave
constexpr uint32_t kPlW = 3072;                 // window bytes
constexpr uint32_t kPlR = 16;                   // records per round of a group
constexpr uint32_t kPlL = 64 / kPlG;            // lanes per batch
constexpr uint32_t kPlWavesPerCu = 12;           // resident workgroups per CU (the launch's grid is that many per CU at most)
constexpr uint32_t kPlIdSlots = 16;             // the workgroup's cache of schema ids: (id, T, B) per slot, in LDS
static_assert(kPlR == kPlL && kPlL == kWsL && kPlL == kPlHistBins && kta::rec::line_windows(kPlW), "one parse round; a lane per histogram bin; KiB loads");
static_assert(kPlPartitionSums <= 64 && kPlCellWords <= 64, "a lane per word in the flushes");

// What a lane has accumulated for the batches of ONE partition (acc_part; -1: nothing yet) since its last flush.
struct PayloadAcc {
    int32_t part;
    uint32_t since;                                     // records since the last flush: the u32 words below count at most one a record
    uint32_t cls[kPlClasses], with, bad;
    uint64_t bytes[kPlClasses - kPlFramed], headers, keyb, valb, nulls, wire;   // (null and empty values have no bytes)
};

// The accumulators of the wave added to the vector and cleared; every lane calls it (cross-lane sums).  When every lane that
// holds something holds it for one partition — a blob is one partition in the pipeline — the words are summed over the wave
// and lanes 0 .. 17 add one word each; otherwise over each group, whose lanes add the words of the group's partition.
__device__ __forceinline__ void payload_flush_acc(PayloadAcc &a, unsigned long long *vec, uint32_t lane)
{
    const uint32_t sub = lane % kPlL;
    const uint64_t holders = KTA_BALLOT64(a.part >= 0);
    if (holders == 0ull) return;                                              // (uniform)
    const uint32_t first = KTA_UNI((uint32_t)__builtin_ctzll(holders));
    const int32_t p0 = (int32_t)KTA_READLANE((uint32_t)a.part, first);
    const bool one = KTA_BALLOT64(a.part >= 0 && a.part != p0) == 0ull;       // (uniform)
    uint64_t words[kPlPartitionSums];
    words[kPlRecords] = 0;
#define KTA_PL_SUM(v) (one ? wave_sum(v) : group_sum(v))
#pragma unroll
    for (uint32_t c = 0; c < kPlClasses; c++) {
        words[kPlClass + c] = KTA_PL_SUM(a.cls[c]);
        words[kPlClassBytes + c] = c >= kPlFramed ? KTA_PL_SUM(a.bytes[c - kPlFramed]) : 0ull;
        words[kPlRecords] += words[kPlClass + c];
    }
    words[kPlWithHeaders] = KTA_PL_SUM(a.with), words[kPlHeaders] = KTA_PL_SUM(a.headers), words[kPlHeaderKeyBytes] = KTA_PL_SUM(a.keyb);
    words[kPlHeaderValueBytes] = KTA_PL_SUM(a.valb), words[kPlHeaderNullValues] = KTA_PL_SUM(a.nulls), words[kPlBadHeaders] = KTA_PL_SUM(a.bad);
    words[kPlHeaderWireBytes] = KTA_PL_SUM(a.wire);
#undef KTA_PL_SUM
    const uint32_t slot = one ? lane : sub;                                   // the first word this lane adds; the second is kPlL behind it
    uint64_t lo = 0, hi = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPlPartitionSums; k++) {
        lo = slot == k ? words[k] : lo;
        if (k >= kPlL) hi = slot == k - kPlL ? words[k] : hi;
    }
    if (one) {
        unsigned long long *pw = vec + (size_t)kPlPartitionWords * (uint32_t)p0;
        if (lane < kPlPartitionSums && lo) atomicAdd(pw + lane, (unsigned long long)lo);
    } else if (a.part >= 0) {
        unsigned long long *pw = vec + (size_t)kPlPartitionWords * (uint32_t)a.part;
        if (lo) atomicAdd(pw + sub, (unsigned long long)lo);
        if (hi) atomicAdd(pw + kPlL + sub, (unsigned long long)hi);
    }
    a.part = -1, a.since = 0, a.with = 0, a.bad = 0;
#pragma unroll
    for (uint32_t c = 0; c < kPlClasses; c++) a.cls[c] = 0;
    a.bytes[0] = a.bytes[1] = a.bytes[2] = 0;
    a.headers = a.keyb = a.valb = a.nulls = a.wire = 0;
}

// One slot of the id cache added to its cell of both rows of the table — T, B and T for every set bit of the id: one add per
// touched word — and emptied; every lane calls it with the same slot, between barriers.
__device__ __forceinline__ void payload_flush_id(uint32_t id, uint64_t t, uint64_t bytes, unsigned long long *table, uint32_t lane)
{
    if (lane < kPlCellWords) {
        const uint64_t v = lane == kPlCellT ? t : lane == kPlCellB ? bytes : (((id >> (lane - kPlCellBits)) & 1u) ? t : 0ull);
        if (v) {
#pragma unroll
            for (uint32_t row = 0; row < kPlRows; row++)
                atomicAdd(table + ((size_t)row * kPlCells + payload_cell(row, id)) * kPlCellWords + lane, (unsigned long long)v);
        }
    }
}

// The ids that lanes hand over (`give`: id, t records, b bytes), one pass per DISTINCT id of the wave, into the workgroup's id
// cache; a slot that holds another id goes to the table first.  Every lane calls it.
__device__ __forceinline__ void payload_drain_ids(bool give, uint32_t id, uint32_t t, uint64_t b, uint32_t *s_id, unsigned long long *s_id_t,
                                                  unsigned long long *s_id_b, unsigned long long *table, uint32_t lane)
{
    uint64_t pending;
    while ((pending = KTA_BALLOT64(give)) != 0ull) {
        const uint32_t leader = KTA_UNI((uint32_t)__builtin_ctzll(pending));
        const uint32_t id0 = KTA_READLANE(id, leader);
        const bool same = give && id == id0;
        const uint64_t records = wave_sum(same ? (uint64_t)t : 0ull), bytes = wave_sum(same ? b : 0ull);
        const uint32_t slot = payload_fmix32(id0) & (kPlIdSlots - 1u);
        const uint32_t held = s_id[slot];
        const uint64_t held_t = s_id_t[slot], held_b = s_id_b[slot];
        const bool other = held_t != 0ull && held != id0;                      // (uniform)
        if (other) payload_flush_id(held, held_t, held_b, table, lane);
        __syncthreads();
        if (lane == 0) s_id[slot] = id0, s_id_t[slot] = (other ? 0ull : held_t) + records, s_id_b[slot] = (other ? 0ull : held_b) + bytes;
        __syncthreads();
        give = give && !same;
    }
}

// grid: the number of workgroups; workgroup w takes the batches 4 q .. 4 q + 3 for q = w, w + grid, ...
__global__ __launch_bounds__(64) KTA_WAVES_PER_EU(3, 8) void kta_payload(const uint4 *blocks, const kta_kafka_batch_desc *descs, uint64_t n_batches, uint32_t P,
                                                  FilterSpec f, const uint32_t *bitmap, unsigned long long *vec, uint32_t grid)
{
    namespace rec = kta::rec;
    constexpr int G = kPlG;
    constexpr uint32_t W = kPlW, R = kPlR, L = kPlL;
    __shared__ uint4 s_win[G][W / 16 + 1];        // the walk's arrays (kta_record_walk.h: WalkLds)
    __shared__ uint32_t s_start[G][R + 1];
    __shared__ uint64_t s_next[G];
    __shared__ uint32_t s_found[G], s_first_incomplete[G], s_first_bad[G];
    __shared__ uint32_t s_hist[G][kPlHistBins];
    __shared__ uint32_t s_id[kPlIdSlots];
    __shared__ unsigned long long s_id_t[kPlIdSlots], s_id_b[kPlIdSlots];   // T == 0: the slot is empty
    const WalkLds<G, W, R> lds{s_win, s_start, s_next, s_found, s_first_incomplete, s_first_bad};
    const uint32_t lane = threadIdx.x, g = lane / L, sub = lane % L;
    const uint8_t *win = reinterpret_cast<const uint8_t *>(s_win[g]);
    s_hist[g][sub] = 0u;
    if (lane < kPlIdSlots) s_id[lane] = 0u, s_id_t[lane] = 0ull, s_id_b[lane] = 0ull;
    PayloadAcc acc;
    acc.part = -1, acc.since = 0, acc.with = 0, acc.bad = 0;
#pragma unroll
    for (uint32_t c = 0; c < kPlClasses; c++) acc.cls[c] = 0;
    acc.bytes[0] = acc.bytes[1] = acc.bytes[2] = 0;
    acc.headers = acc.keyb = acc.valb = acc.nulls = acc.wire = 0;
    uint32_t no_headers = 0;                            // this lane's records in bin 0 of the histogram (s_hist holds the other bins)
    uint32_t c_id = 0, c_t = 0;                         // this lane's schema id: c_t records (0: none) of c_b value bytes, in registers
    uint64_t c_b = 0;
    unsigned long long *table = vec + payload_table_at(P);
    __syncthreads();
  for (uint64_t quad = blockIdx.x; quad * G < n_batches; quad += grid) {      // (uniform)
    WalkBatch bt = walk_batch(descs, quad * G + g, n_batches, P, f, bitmap);
    // the accumulators hold one partition: another one first sends them to the vector (every lane takes part); so does a
    // lane whose 32-bit counts are half full
    if (__any((bt.counted && acc.part >= 0 && acc.part != bt.partition) || acc.since >= 0x80000000u)) payload_flush_acc(acc, vec, lane);
    if (__any(no_headers >= 0x80000000u)) {                                    // (s_hist's words are 32 bits wide as well)
        if (no_headers) atomicAdd(&s_hist[g][0], no_headers);
        no_headers = 0;
        __syncthreads();
        if (s_hist[g][sub]) atomicAdd(vec + payload_hist_at(P) + sub, (unsigned long long)s_hist[g][sub]);
        s_hist[g][sub] = 0u;
        __syncthreads();
    }
    if (bt.counted) acc.part = bt.partition;
    while (__any(bt.run)) {
        const WalkRound rd = walk_open(blocks, bt, lds, lane);
        const uint64_t wbase = rd.wbase;
        const uint32_t limit = rd.limit;
        // this lane's record of the round, held until the round knows how far it commits
        bool hdr_bad = false;
        uint32_t cls = 0, id = 0, hcount_bin = 0;
        uint64_t vb = 0, hcount = 0, hkeyb = 0, hvalb = 0, hnulls = 0, wire = 0;
        BlockSrc src{blocks, ~0ull, make_uint4(0, 0, 0, 0)};
        const WalkRecord wr = walk_record(bt, rd, lds, f, src, lane);
        const bool have = wr.counts;
        if (have) {
            const rec::Record &r = wr.r;
            const uint64_t value = wr.value;
            const uint32_t rec_end = wr.rec_end;
            const uint64_t rec_end_abs = wbase + rec_end;
            vb = r.val_len > 0 ? (uint64_t)r.val_len : 0ull;
            const uint64_t vrel = value - wbase;
            const uint32_t need = vb >= 5 ? 5u : (vb ? 1u : 0u);
            uint32_t head[5] = {0xFFu, 0u, 0u, 0u, 0u};
            if (need == 0u) {
            } else if (vrel + need <= limit) {                                 // the head lies inside the window: two reads (what
                const uint32_t *w32 = reinterpret_cast<const uint32_t *>(win);           // lies behind `limit` decides nothing)
                const uint32_t w0 = rec::window_bytes4(w32, (uint32_t)vrel), w1 = rec::window_bytes4(w32, (uint32_t)vrel + 4u);
                head[0] = w0 & 0xFFu, head[1] = (w0 >> 8) & 0xFFu, head[2] = (w0 >> 16) & 0xFFu, head[3] = w0 >> 24, head[4] = w1 & 0xFFu;
            } else {
#pragma unroll
                for (uint32_t q = 0; q < 5; q++)
                    if (q < need) head[q] = src.at(value + q);
            }
            cls = payload_class(r.val_len, head[0]);
            id = payload_schema_id(head[1], head[2], head[3], head[4]);
            const uint64_t hpos = value + vb;
            wire = rec_end_abs - hpos;
            if (wire == 1 && hpos - wbase < limit && win[(uint32_t)(hpos - wbase)] == 0u) {
                // no headers: the one byte 0, inside the window
            } else if (rec_end <= limit) {                                     // the record lies inside the window: walked in LDS
                WindowSrc ws{win, wbase};
                const PayloadHeaders h = payload_walk_headers(ws, hpos, rec_end_abs);
                hdr_bad = h.bad, hcount = h.count, hkeyb = h.key_bytes, hvalb = h.value_bytes, hnulls = h.null_values;
            } else {
                const PayloadHeaders h = payload_walk_headers(src, hpos, rec_end_abs);
                hdr_bad = h.bad, hcount = h.count, hkeyb = h.key_bytes, hvalb = h.value_bytes, hnulls = h.null_values;
            }
            hcount_bin = payload_hist_bin(hcount);
        }
        __syncthreads();
        bool give = false;                                                     // this lane hands its id over: its record carries another
        uint32_t g_id = 0, g_t = 0;
        uint64_t g_b = 0;
        if (bt.run) {
            const WalkCommit cm = walk_commit(lds, g);
            if (have && sub < cm.commit) {
                acc.since++;
#pragma unroll
                for (uint32_t c = 0; c < kPlClasses; c++) acc.cls[c] += cls == c ? 1u : 0u;                       // (registers: no indexing)
#pragma unroll
                for (uint32_t c = kPlFramed; c < kPlClasses; c++) acc.bytes[c - kPlFramed] += cls == c ? vb : 0ull;
                if (cls == kPlFramed) {                                        // a real topic has a handful of ids: the lane keeps one
                    give = c_t != 0u && (c_id != id || c_t >= 0x80000000u);
                    if (give) g_id = c_id, g_t = c_t, g_b = c_b, c_t = 0u, c_b = 0ull;
                    c_id = id, c_t++, c_b += vb;
                }
                if (hdr_bad) acc.bad++;
                else {
                    acc.with += hcount != 0, acc.headers += hcount, acc.keyb += hkeyb, acc.valb += hvalb, acc.nulls += hnulls, acc.wire += wire;
                    if (hcount_bin == 0u) no_headers++;
                    else atomicAdd(&s_hist[g][hcount_bin], 1u);
                }
            }
            walk_advance(bt, rd, lds, g, cm);
        }
        payload_drain_ids(give, g_id, g_t, g_b, s_id, s_id_t, s_id_b, table, lane);
        __syncthreads();
    }
  }
    __syncthreads();
    payload_flush_acc(acc, vec, lane);
    payload_drain_ids(c_t != 0u, c_id, c_t, c_b, s_id, s_id_t, s_id_b, table, lane);
    if (no_headers) atomicAdd(&s_hist[g][0], no_headers);
    __syncthreads();
    for (uint32_t slot = 0; slot < kPlIdSlots; slot++)                         // (uniform)
        if (s_id_t[slot] != 0ull) payload_flush_id(s_id[slot], s_id_t[slot], s_id_b[slot], table, lane);
    const uint32_t in_bin = s_hist[g][sub];
    if (in_bin) atomicAdd(vec + payload_hist_at(P) + sub, (unsigned long long)in_bin);
}

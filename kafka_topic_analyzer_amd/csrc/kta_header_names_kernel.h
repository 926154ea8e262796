// kta_header_names_kernel.h — the header-name section's kernel (kta_header_names, KTA_FLAG_HEADER_NAMES).
// kta_header_names.hip includes this file INSIDE its unnamed namespace, behind kta_decode_coop.h (pin, load_block,
// KTA_READLANE); beside kta_wave_src.h it has no includes of its own: the including file has included kta_filter.h, kta_kafka.h,
// kta_header_names.h and kta_records.h (at file scope) and provides the HIP runtime — or, for the CPU suite,
// tests/native/wave_emu.h (tests/native/header_names_emu.cpp, tests/test_header_names_emu.py): the kernel below is then the
// very source the GPU runs.  What the kernel does is said at the top of kta_header_names.hip.  The walk of a batch — the
// descriptor, the window, the chain, the parse, the commit rule, the advance — is kta_record_walk.h's, statement for
// statement, kept here as text: over that header this kernel measured up to 1.8 % slower (profiles/record_walk_bench_ab.jsonl).
#pragma once

#ifndef KTA_BALLOT64    // the lanes (of those that call it together) whose predicate holds.  (wave_emu.h: a meeting point.)
#define KTA_BALLOT64(p) ((uint64_t)__builtin_amdgcn_ballot_w64(p))
#endif

#include "kta_wave_src.h"

constexpr int kHnG = 4;                         // batches per wave
constexpr uint32_t kHnW = 3072;                 // window bytes
constexpr uint32_t kHnR = 16;                   // records per round of a group
constexpr uint32_t kHnL = 64 / kHnG;            // lanes per batch
constexpr uint32_t kHnNLoad = kHnW / (kHnL * 16);
constexpr uint32_t kHnPer = kHnW / 1024;
constexpr uint32_t kHnWavesPerCu = 10;          // resident workgroups per CU (14.5 KiB of LDS each; the grid is that many per CU at most)
constexpr uint32_t kHnCacheSlots = 64;          // the workgroup's cache of names, keyed by hash, in LDS
constexpr uint32_t kHnSinceMax = 1u << 24;      // a lane's occurrences in the cache since its last flush stay below twice this:
                                                // 64 lanes keep a slot's 32-bit T and Z below 2^31
enum HnInfoWord : uint32_t { kHnInfoSpills = 0, kHnInfoClaims = 1, kHnInfoCacheFlushes = 2, kHnInfoWords = 4 };
static_assert(kHnR == kHnL && kHnL == kWsL && kta::rec::line_windows(kHnW), "one parse round; KiB loads");
static_assert(kHnCellWords <= 64 && kHnCacheSlots == 64, "a lane per word in the flush; a lane per slot when the cache is cleared");

// The workgroup's name cache: tag 0 an empty slot, else 2^32 | hash (claimed with a compare-and-swap); T and Z count at
// most one an occurrence, L and V are byte sums.
struct HnCache {
    unsigned long long *tag, *l, *v;
    uint32_t *t, *z;
};
// What a lane keeps in registers: the globals' words it has seen, its occurrences in the cache since the last flush, and
// the work counters.
struct HnLane {
    uint64_t occ, nameb, valb, nulls, with, looked;
    uint32_t since, spills, claims;
};

// The exemplar of hash h: the name slots of its two cells, each claimed by whoever finds it empty — the fields written
// with plain stores, a fence, then `state` published.  A slot in any other state is left alone: the first writer wins.
template <class Src>
__device__ __forceinline__ void hn_capture(Src &src, uint64_t name, uint64_t name_len, uint32_t h, kta::HnSlot *names)
{
#pragma unroll
    for (uint32_t row = 0; row < kPlRows; row++) {
        kta::HnSlot *s = names + row * kPlCells + payload_cell(row, h);
        if (atomicCAS(&s->state, (uint32_t)kHnEmpty, (uint32_t)kHnClaimed) != (uint32_t)kHnEmpty) continue;
        s->hash = h, s->name_len = name_len < 0xFFFFFFFFull ? (uint32_t)name_len : 0xFFFFFFFFu, s->reserved = 0u;
        uint32_t *w = reinterpret_cast<uint32_t *>(s->bytes);
        for (uint32_t q = 0; q < kHnExemplarBytes / 4; q++) {
            uint32_t word = 0;
            for (uint32_t b = 0; b < 4; b++)
                if (4 * q + b < name_len) word |= src.at(name + 4 * q + b) << (8 * b);
            w[q] = word;
        }
        __threadfence();
        atomicExch(&s->state, (uint32_t)kHnPublished);
    }
}

// One occurrence (the rule: kta_header_names.h's hn_add_occurrence).  Into the cache slot of its hash when the slot is
// empty or holds that hash; when it holds another, or `direct`, straight to the table's two cells: exact either way.
template <class Src>
__device__ __forceinline__ void hn_emit(Src &src, uint64_t name, uint64_t name_len, long long val_len, bool direct, const HnCache &c, HnLane &st,
                                        unsigned long long *table, kta::HnSlot *names)
{
    uint32_t h = kHnFnvInit;
    for (uint64_t i = 0; i < name_len; i++) h = hn_fnv_byte(h, src.at(name + i));
    const uint64_t vb = val_len > 0 ? (uint64_t)val_len : 0ull;
    const uint32_t z = val_len < 0 ? 1u : 0u;
    st.occ++, st.nameb += name_len, st.valb += vb, st.nulls += z;
    const uint32_t slot = payload_fmix32(h) >> 26;                            // (the bits that row 1's cell does not use)
    const unsigned long long want = (1ull << 32) | h;
    const unsigned long long held = direct ? ~0ull : atomicCAS(&c.tag[slot], 0ull, want);
    if (held == 0ull || held == want) {
        atomicAdd(&c.t[slot], 1u);
        atomicAdd(&c.l[slot], (unsigned long long)name_len);
        if (vb) atomicAdd(&c.v[slot], (unsigned long long)vb);
        if (z) atomicAdd(&c.z[slot], 1u);
        if (held == 0ull) {
            st.claims++;
            hn_capture(src, name, name_len, h, names);
        }
        return;
    }
    st.spills++;
#pragma unroll
    for (uint32_t row = 0; row < kPlRows; row++) {
        unsigned long long *cell = table + ((size_t)row * kPlCells + payload_cell(row, h)) * kHnCellWords;
        atomicAdd(cell + kHnCellT, 1ull);
        if (name_len) atomicAdd(cell + kHnCellL, (unsigned long long)name_len);
        if (vb) atomicAdd(cell + kHnCellV, (unsigned long long)vb);
        if (z) atomicAdd(cell + kHnCellZ, 1ull);
        for (uint32_t b = 0; b < 32; b++)
            if ((h >> b) & 1u) atomicAdd(cell + kHnCellBits + b, 1ull);
    }
    hn_capture(src, name, name_len, h, names);
}

// Every used slot of the cache added to its cell of both rows — T, L, V, Z and T for every set bit of the hash, a lane per
// word: one add per touched word — and the cache emptied.  Every lane calls it; no lane emits meanwhile.
__device__ __forceinline__ void hn_flush_cache(const HnCache &c, unsigned long long *table, uint32_t lane)
{
    __syncthreads();
    for (uint32_t slot = 0; slot < kHnCacheSlots; slot++) {                   // (uniform)
        const unsigned long long tag = c.tag[slot];
        if (tag == 0ull) continue;
        const uint32_t h = (uint32_t)tag;
        const uint64_t t = c.t[slot];
        if (lane < kHnCellWords) {
            const uint64_t v = lane == kHnCellT   ? t
                               : lane == kHnCellL ? (uint64_t)c.l[slot]
                               : lane == kHnCellV ? (uint64_t)c.v[slot]
                               : lane == kHnCellZ ? (uint64_t)c.z[slot]
                                                  : (((h >> (lane - kHnCellBits)) & 1u) ? t : 0ull);
            if (v) {
#pragma unroll
                for (uint32_t row = 0; row < kPlRows; row++)
                    atomicAdd(table + ((size_t)row * kPlCells + payload_cell(row, h)) * kHnCellWords + lane, (unsigned long long)v);
            }
        }
    }
    __syncthreads();
    c.tag[lane] = 0ull, c.l[lane] = 0ull, c.v[lane] = 0ull, c.t[lane] = 0u, c.z[lane] = 0u;
    __syncthreads();
}

// grid: the number of workgroups; workgroup w takes the batches 4 q .. 4 q + 3 for q = w, w + grid, ...
__global__ __launch_bounds__(64) KTA_WAVES_PER_EU(2, 8) void kta_header_names(const uint4 *blocks, const kta_kafka_batch_desc *descs, uint64_t n_batches,
                                                                            uint32_t P, FilterSpec f, const uint32_t *bitmap, unsigned long long *vec,
                                                                            kta::HnSlot *names, unsigned long long *info, uint32_t grid)
{
    namespace rec = kta::rec;
    constexpr int G = kHnG;
    constexpr uint32_t W = kHnW, R = kHnR, L = kHnL, NLOAD = kHnNLoad, PER = kHnPer;
    __shared__ uint4 s_win[G][W / 16 + 1];        // + 1: the register paths read whole dwords up to 16 bytes ahead
    __shared__ uint32_t s_start[G][R + 1];
    __shared__ uint64_t s_next[G];
    __shared__ uint32_t s_found[G], s_first_incomplete[G], s_first_bad[G];
    __shared__ unsigned long long s_tag[kHnCacheSlots], s_l[kHnCacheSlots], s_v[kHnCacheSlots];
    __shared__ uint32_t s_t[kHnCacheSlots], s_z[kHnCacheSlots];
    const uint32_t lane = threadIdx.x, g = lane / L, sub = lane % L;
    const uint8_t *win = reinterpret_cast<const uint8_t *>(s_win[g]);
    const HnCache cache{s_tag, s_l, s_v, s_t, s_z};
    s_tag[lane] = 0ull, s_l[lane] = 0ull, s_v[lane] = 0ull, s_t[lane] = 0u, s_z[lane] = 0u;
    HnLane st;
    st.occ = st.nameb = st.valb = st.nulls = st.with = st.looked = 0ull;
    st.since = st.spills = st.claims = 0u;
    uint32_t cache_flushes = 0;
    unsigned long long *table = vec + kHnGlobals;
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
    bool run = counted && j < total;                      // uniform inside a group
    while (__any(run)) {
        if (__any(st.since >= kHnSinceMax)) {             // a slot's 32-bit counts could come near 2^31: the cache goes to the table
            hn_flush_cache(cache, table, lane);
            st.since = 0u;
            cache_flushes += lane == 0 ? 1u : 0u;
        }
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
        // VALIDATE: this lane's record of the round and its header section, held until the round knows how far it commits
        bool have = false, in_window = false;
        uint64_t hpos = 0, hend = 0, hcount = 0;
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
                uint64_t value = wbase + r.after;                              // where the value's bytes begin
                if (verdict == rec::REC_VALUE_LENGTH_OUTSIDE) {                // behind a key of the window's size
                    verdict = payload_varlong(src, value, rec_end_abs, r.val_len) ? rec::value_fits(r.val_len, value - wbase, rec_end) : rec::REC_BAD;
                }
                if (verdict == rec::REC_INCOMPLETE) atomicMin(&s_first_incomplete[g], k);
                else if (verdict != rec::REC_OK) atomicMin(&s_first_bad[g], k);
                else if (filter_time_passes(f, ts_base + (r.ts_delta & ts_mask))) {
                    hpos = value + (r.val_len > 0 ? (uint64_t)r.val_len : 0ull);
                    hend = rec_end_abs;
                    in_window = rec_end <= limit;
                    if (hend - hpos == 1 && hpos - wbase < limit && win[(uint32_t)(hpos - wbase)] == 0u) {
                        have = true;                                           // no headers: the one byte 0, inside the window
                    } else if (in_window) {                                    // the record lies inside the window: walked in LDS
                        WindowSrc ws{win, wbase};
                        const PayloadHeaders h = payload_walk_headers(ws, hpos, hend);
                        have = !h.bad, hcount = h.count;
                    } else {
                        const PayloadHeaders h = payload_walk_headers(src, hpos, hend);
                        have = !h.bad, hcount = h.count;
                    }
                }
            }
        }
        __syncthreads();
        // COMMIT, then VISIT: only the records in front of the round's first incomplete and first bad one, only good sections
        if (run) {
            const uint32_t found = s_found[g], first_inc = s_first_incomplete[g], first_bad = s_first_bad[g];
            const uint32_t done = first_inc < found ? first_inc : found;
            const uint32_t commit = first_bad < done ? first_bad : done;
            if (have && sub < commit) {
                st.looked++, st.with += hcount != 0;
                if (hcount) {
                    const bool direct = hcount >= kHnSinceMax;                 // (a record of 2^24 headers and more goes past the cache)
                    if (!direct) st.since += (uint32_t)hcount;
                    auto visit = [&](auto &src) {
                        payload_visit_headers(src, hpos, hend, [&](uint64_t name, uint64_t name_len, long long val_len) {
                            hn_emit(src, name, name_len, val_len, direct, cache, st, table, names);
                        });
                    };
                    if (in_window) {
                        WindowSrc ws{win, wbase};
                        visit(ws);
                    } else {
                        BlockSrc src{blocks, ~0ull, make_uint4(0, 0, 0, 0)};
                        visit(src);
                    }
                }
            }
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
    hn_flush_cache(cache, table, lane);
    const uint64_t sums[kHnGlobalSums] = {wave_sum(st.occ), wave_sum(st.nameb), wave_sum(st.valb), wave_sum(st.nulls), wave_sum(st.with), wave_sum(st.looked)};
    const uint64_t spills = wave_sum(st.spills), claims = wave_sum(st.claims), flushes = wave_sum(cache_flushes);
    uint64_t mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kHnGlobalSums; k++) mine = lane == k ? sums[k] : mine;
    if (lane < kHnGlobalSums && mine) atomicAdd(vec + lane, (unsigned long long)mine);
    const uint64_t work = lane == kHnInfoSpills ? spills : lane == kHnInfoClaims ? claims : lane == kHnInfoCacheFlushes ? flushes : 0ull;
    if (lane < kHnInfoWords && work) atomicAdd(info + lane, (unsigned long long)work);
}

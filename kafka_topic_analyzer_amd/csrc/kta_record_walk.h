// kta_record_walk.h — the walk over the records of a decoded batch, for the kernels behind the decode kernel: the batch as a
// group of 64 / G lanes holds it, a round's window, chain and parse, the commit rule and the advance.  kta_payload_kernel.h
// walks with it.  kta_header_names_kernel.h and kta_value_bytes_kernel.h hold the same statements as text of their own: over
// this header both measured 1-2 % slower than their own text on some legs (profiles/record_walk_bench_ab.jsonl),
// so a change of the framing rule is made here and in those two.  Why the walk has this shape — a window through LDS, the
// wave's KiB loads, the leader's chain, a record per lane — is said in kta_decode_coop.h, whose kernel keeps its own copy
// (NT parse rounds, a flag for the first bad record, the small-window loads).  Included INSIDE the including file's
// unnamed namespace, behind kta_decode_coop.h (pin, load_block, KTA_READLANE) and kta_wave_src.h (BlockSrc); no includes of
// its own: the including file has included kta_filter.h, kta_kafka.h, kta_payload.h and kta_records.h at file scope.
// <G, W, R>: batches per wave, window bytes, records per round of a group; one parse round (R lanes a group), KiB loads.
//
// A round of a kernel, every lane:   walk_open (two barriers)  ->  walk_record  ->  a barrier of the kernel's  ->
// walk_commit, what the kernel does with its committed record, walk_advance  ->  a barrier of the kernel's.
#pragma once

// The batch of this lane's group: what its descriptor says, and how far the walk has come (pos, j, run).
struct WalkBatch {
    uint64_t end, pos;          // the records section ends here; the next record to take begins here
    int64_t ts_base, ts_mask;   // a record's timestamp: ts_base + (its delta & ts_mask)
    uint32_t total, j;          // the records the batch promises; those done
    int32_t partition;
    bool counted;               // the batch: status 0, partition in [0, P) and in the filter's set
    bool run;                   // the batch has records left to take (uniform inside a group)
};

// Batch b of the call (b >= n_batches: none, nothing to run).
__device__ __forceinline__ WalkBatch walk_batch(const kta_kafka_batch_desc *descs, uint64_t b, uint64_t n_batches, uint32_t P, const FilterSpec &f,
                                                const uint32_t *bitmap)
{
    WalkBatch bt{0, 0, 0, 0, 0, 0, 0, false, false};
    if (b < n_batches) {
        const kta_kafka_batch_desc &d = descs[b];
        bt.end = d.payload_end; bt.pos = d.payload_off;
        const bool append_time = (d.flags & KTA_KB_LOG_APPEND_TIME) != 0;   // every record carries maxTimestamp
        bt.ts_base = append_time ? d.max_ts_ms : d.base_ts_ms;
        bt.ts_mask = append_time ? 0 : -1;
        bt.total = d.n_records > 0 ? (uint32_t)d.n_records : 0u; bt.partition = d.partition;
        bt.counted = d.status == 0 && (uint32_t)bt.partition < P &&
                     (!f.parts || ((bitmap[(uint32_t)bt.partition >> 5] >> ((uint32_t)bt.partition & 31u)) & 1u));
    }
    bt.run = bt.counted && bt.j < bt.total;
    return bt;
}

// The kernel's LDS arrays of the walk (__shared__ declarations of the kernel: their order there is the LDS layout).
template <int G, uint32_t W, uint32_t R>
struct WalkLds {
    uint4 (*win)[W / 16 + 1];           // + 1: the register paths read whole dwords up to 16 bytes ahead
    uint32_t (*start)[R + 1];           // record starts relative to the window base; [found]: where the last one ends
    uint64_t *next;                     // absolute position after the last chained record
    uint32_t *found, *first_incomplete, *first_bad;
};

// A round's window: its base in the blob, the valid bytes in it, the batch's end seen from its base, whether it reaches that end.
struct WalkRound {
    uint64_t wbase;
    uint32_t limit, end_rel;
    bool to_the_end;
};

// A round's opening: the windows of the wave's G groups loaded into LDS, the record starts of this group's window chained by
// its first lane.  Every lane calls it; two barriers.  A batch whose count promises more records than it holds stops running.
template <int G, uint32_t W, uint32_t R>
__device__ __forceinline__ WalkRound walk_open(const uint4 *blocks, WalkBatch &bt, const WalkLds<G, W, R> &s, uint32_t lane)
{
    namespace rec = kta::rec;
    constexpr uint32_t L = 64 / G, NLOAD = W / (L * 16), PER = W / 1024;
    static_assert(R == L && rec::line_windows(W), "one parse round; KiB loads");
    const uint32_t g = lane / L, sub = lane % L;
    const uint8_t *win = reinterpret_cast<const uint8_t *>(s.win[g]);
    WalkRound rd{0, 0, 0, false};
    uint64_t load_base = 0;                               // a group that does not run reads the blob's first block into its own window
    uint32_t load_bytes = 16;
    if (bt.run && bt.pos >= bt.end) bt.run = false;       // (the count promises more records than the batch holds: nothing more)
    if (bt.run) {
        rd.wbase = rec::window_base(bt.pos, W);
        const uint64_t span = ((bt.end + 15) & ~15ull) - rd.wbase, rest = bt.end - rd.wbase;
        const uint32_t wbytes = span < W ? (uint32_t)span : W;             // a multiple of 16, at least 16
        rd.to_the_end = rest <= wbytes;
        rd.limit = rd.to_the_end ? (uint32_t)rest : wbytes;
        rd.end_rel = rest < 0xF0000000ull ? (uint32_t)rest : 0xF0000000u;
        load_base = rd.wbase; load_bytes = wbytes;
        if (sub == 0) { s.first_bad[g] = R + 1; s.first_incomplete[g] = R; }
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
        for (uint32_t u = 0; u < NLOAD; u++) s.win[u / PER][(u % PER) * 64 + lane] = stage[u];
    }
    __syncthreads();
    if (bt.run && sub == 0) {                                                  // chain the length prefixes
        const uint32_t *w32 = reinterpret_cast<const uint32_t *>(win);
        const uint32_t want = bt.total - bt.j < R ? bt.total - bt.j : R;
        uint32_t k = 0, cur = (uint32_t)(bt.pos - rd.wbase);
        uint64_t next = 0;
        if (rec::chain(w32, rd.limit, want, s.start[g], k, cur)) {             // a length of three bytes or more: byte by byte
            uint32_t off = cur;
            long long len;
            if (rec::window_varlong(win, off, rd.limit, len)) {
                const uint64_t rec_end = rd.wbase + off + (uint64_t)len;
                if (len < 0 || rec_end > bt.end) s.first_bad[g] = k;
                else { s.start[g][k++] = cur; next = rec_end; }
            } else if (rd.to_the_end) {
                s.first_bad[g] = k;                                            // ran into the end of the batch
            }                                                                  // (else it straddles the window: next round)
        }
        if (!next) next = rd.wbase + cur;
        const uint64_t next_rel = next - rd.wbase;
        s.start[g][k] = next_rel < 0xFFFFFFFFull ? (uint32_t)next_rel : 0xFFFFFFFFu;
        s.found[g] = k;
        s.next[g] = next;
    }
    __syncthreads();
    return rd;
}

// This lane's record of the round: parsed, judged — the round's first incomplete and first bad record noted in LDS — and
// passed through the time filter.  counts: the record counts, should the round commit it; then r is the record, value where
// its value's bytes begin in the blob and rec_end its end relative to the window base.  A value length that lies outside
// the window is read through src, which keeps the block for what the caller reads next.
struct WalkRecord {
    bool counts;
    kta::rec::Record r;
    uint64_t value;
    uint32_t rec_end;
};
template <int G, uint32_t W, uint32_t R>
__device__ __forceinline__ WalkRecord walk_record(const WalkBatch &bt, const WalkRound &rd, const WalkLds<G, W, R> &s, const FilterSpec &f, BlockSrc &src,
                                                  uint32_t lane)
{
    namespace rec = kta::rec;
    constexpr uint32_t L = 64 / G;
    const uint32_t g = lane / L, sub = lane % L;
    const uint8_t *win = reinterpret_cast<const uint8_t *>(s.win[g]);
    WalkRecord w;
    w.counts = false, w.value = 0, w.rec_end = 0;
    if (bt.run && sub < s.found[g]) {
        const uint32_t k = sub;
        const uint32_t start = s.start[g][k], rec_end = s.start[g][k + 1];
        if (rec_end > rd.end_rel) {                                            // the record overruns the batch
            atomicMin(&s.first_bad[g], k);
        } else {
            const uint64_t rec_end_abs = rd.wbase + rec_end;
            uint32_t verdict = rec::parse_record(win, start, rec_end, rd.limit, w.r);
            w.value = rd.wbase + w.r.after;                                    // where the value's bytes begin
            w.rec_end = rec_end;
            if (verdict == rec::REC_VALUE_LENGTH_OUTSIDE) {                    // behind a key of the window's size
                verdict = payload_varlong(src, w.value, rec_end_abs, w.r.val_len) ? rec::value_fits(w.r.val_len, w.value - rd.wbase, rec_end) : rec::REC_BAD;
            }
            if (verdict == rec::REC_INCOMPLETE) atomicMin(&s.first_incomplete[g], k);
            else if (verdict != rec::REC_OK) atomicMin(&s.first_bad[g], k);
            else if (filter_time_passes(f, bt.ts_base + (w.r.ts_delta & bt.ts_mask))) w.counts = true;
        }
    }
    return w;
}

// How far the round commits, behind the barrier that follows walk_record: the records in front of the round's first incomplete
// one are done (those behind are redone next round), and of them the ones in front of its first bad one are committed.
struct WalkCommit {
    uint32_t found, done, commit;
    bool ends;                          // bad framing, or no progress (a truncated batch): the batch ends here
};
template <int G, uint32_t W, uint32_t R>
__device__ __forceinline__ WalkCommit walk_commit(const WalkLds<G, W, R> &s, uint32_t g)
{
    const uint32_t found = s.found[g], first_inc = s.first_incomplete[g], first_bad = s.first_bad[g];
    const uint32_t done = first_inc < found ? first_inc : found;
    return WalkCommit{found, done, first_bad < done ? first_bad : done, first_bad <= done || done == 0};
}

// The batch moved behind the round's done records; a group that runs calls it.
template <int G, uint32_t W, uint32_t R>
__device__ __forceinline__ void walk_advance(WalkBatch &bt, const WalkRound &rd, const WalkLds<G, W, R> &s, uint32_t g, const WalkCommit &c)
{
    if (c.ends) {
        bt.run = false;
    } else {
        bt.j += c.done;
        bt.pos = c.done < c.found ? rd.wbase + s.start[g][c.done] : s.next[g];   // records >= done are redone
        bt.run = bt.j < bt.total;
    }
}

// kta_kernels.hip — hand-written gfx950 (MI355X / CDNA4) kernels for the per-record
// metric-accumulation hot path of kafka-topic-analyzer: the metrics scan (K1, K1p), the fold of its partial rows (K5),
// the tile expansion and the result vector's initialisation, with their launchers.  Integer/byte work, HBM-bound:
// no MFMA.  wave = 64 lanes, 256-thread workgroups, 16 B/lane coalesced loads,
// LDS-staged per-workgroup partial counters, deterministic integer reductions.
// (The single-kernel alive-table family is kta_alive_table.hip.)
//
// Reference semantics (paths under /root/reference):
//   kta_metrics_scan   src/metric.rs:207-252  MessageMetrics::handle_message
#include "kta_kernels.h"
#include "kta_fold.h"
#include "kta_lean_blocks.h"
#include "kta_plane_pack.h"

#include <limits.h>
#include <type_traits>

namespace kta {

// ---------------------------------------------------------------------------------------
// K1  metrics scan
// ---------------------------------------------------------------------------------------
//
// Input: four columns, 20 B/record (partition i32, key_len i32, val_len i32, ts_ms i64).
// Each lane owns 4 consecutive records per tile (one int4 from each i32 column, two
// longlong2 from the timestamp column: 5 x 16 B loads, fully coalesced: a wave reads
// 3 x 1 KiB + 2 KiB contiguous).  A tile is 256 lanes x 4 records; tiles are dealt
// round-robin to workgroups, and the next tile's loads are issued before the current
// tile is accumulated (register double buffer) to keep HBM requests in flight.
//
// Accumulation: per-partition partial counters live in LDS, replicated 2^rep_log2 times
// (replica = lane & (R-1)) so records of one partition that sit in the same wave do not
// serialise on one LDS address (a Kafka consumer delivers per-partition runs, and small
// P is common).  Three non-returning 64-bit LDS atomics per record — or per QUAD when the
// lane's four consecutive records share a partition (inside a per-partition run they do):
//     A += 1 | tombstone << 21 | key_null << 42      (three 21-bit counts in one word)
//     K += key_len (Some)      V += val_len (Some)
// LDS partials are flushed to this workgroup's row of the partial workspace every 2^18
// records (so the 21-bit fields cannot overflow) and at the end; a second tiny kernel
// folds the rows.  No floating point anywhere; integer adds commute, so results are
// independent of scheduling.
//
// Tile-compact batches (TILED, kta_hip.h): the tiles are the layout's own (KTA_TILE_RECORDS = this kernel's 1024),
// taken at their allocation positions, and records outside [rec0, rec0 + n) are masked per record (no scalar tail).
// The tile's header (one uniform load) picks the loads: a compact tile is read as one uint2 of u16 partitions and
// one int4 of i32 timestamp offsets per lane next to the two int4 length loads — 14 B per record, every
// instruction a fully coalesced wave-wide stream (512 B or 1 KiB) — and a raw tile as above.  The compact values
// travel in the raw registers of the Quad (p.xy, t0) and are widened when the tile is accumulated.
// The same header's `lens` picks the length loads, independently: a u16 tile (keyless allocations only) gives a lane
// the four key lengths and the four value lengths of its records in ONE int4 of the key_len column — 10 B per record
// with compact partitions and timestamps — which rides in the Quad's k registers and is widened (0xFFFF -> -1) when the
// tile is accumulated.
//
// The accumulating scan of a tile-compact batch without additive outputs — the flagship's — is a kernel of its own,
// kta_metrics_scan_packed (K1p below): the same loads and tile deal, two atomics per record into packed words, a second,
// full-width level of partials in LDS, one row write at the end.
//
// Globals: min/max of ts_ms (-1 => 0 first, metric.rs:209) — the division by 1000
// (metric.rs:210) is monotone, so it is applied once to the extrema on the host — and
// min/max of key+value size over non-tombstones (metric.rs:249-251), both carried in
// registers and reduced with wave shuffles at the end.

constexpr uint32_t kCntBits = 21;
constexpr uint64_t kCntMask = (1ull << kCntBits) - 1;
constexpr uint32_t kFlushTiles = 256;          // 256 tiles x 1024 records = 2^18 records
#ifndef KTA_SCAN_PREFETCH
#define KTA_SCAN_PREFETCH 1
#endif
// Diagnostic build (tools/build_variant.sh <tag> -DKTA_PACKED_LOADS_ONLY=1): kta_metrics_scan_packed does its loads and
// the register work, no LDS accumulation — the HBM bound of its own loads.  Its results are not the scan's.
#ifndef KTA_PACKED_LOADS_ONLY
#define KTA_PACKED_LOADS_ONLY 0
#endif
constexpr int kTilePrefetch = KTA_SCAN_PREFETCH;   // TILED: tiles a workgroup loads ahead of the one it accumulates (1 or 2)
static_assert(kTilePrefetch == 1 || kTilePrefetch == 2, "the prefetch ring has two or three slots");
// kta_metrics_scan_packed has a prefetch distance of its own (a summarised tile has 24 B per lane in flight, not 40).
#ifndef KTA_PACKED_PREFETCH
#define KTA_PACKED_PREFETCH 1
#endif
constexpr int kPackedPrefetch = KTA_PACKED_PREFETCH;
static_assert(kPackedPrefetch == 1 || kPackedPrefetch == 2, "the prefetch ring has two or three slots");

struct Quad {
    int4 p, k, v;
    longlong2 t0, t1;
    long long base;    // TILED: the tile's ts_base
    uint32_t compact;  // TILED: bit 0 = p.xy hold four u16 partitions, t0 four i32 timestamp offsets;
                       //        bit 1 = k holds four u16 key lengths (k.xy) and four u16 value lengths (k.zw)
                       //        bit 2 (with bit 0; kta_metrics_scan_packed only) = the tile is summarised: every record of
                       //        it counts, its timestamp offsets were NOT loaded, and t0.x / t0.y hold what the tile gives
                       //        the earliest / the latest timestamp (uniform; from its kta_tile_sum)
};
constexpr uint32_t kQuadCompact = 1u, kQuadLens16 = 2u, kQuadSummed = 4u;

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v2i __attribute__((ext_vector_type(2)));
typedef long long v2l __attribute__((ext_vector_type(2)));
static_assert(KTA_TILE_RECORDS == 4u * kWG, "a layout tile is one scan tile: 256 lanes x 4 records");

// NT: non-temporal loads (the columns are streamed exactly once; keep them out of L2/MALL)
template <bool NT>
__device__ __forceinline__ void load_quad(Quad &q, const ScanColumns &c, uint64_t qi)
{
    if (NT) {
        const v4i p = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(c.partition) + qi);
        const v4i k = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(c.key_len) + qi);
        const v4i v = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(c.val_len) + qi);
        const v2l t0 = __builtin_nontemporal_load(reinterpret_cast<const v2l *>(c.ts_ms) + 2 * qi);
        const v2l t1 = __builtin_nontemporal_load(reinterpret_cast<const v2l *>(c.ts_ms) + 2 * qi + 1);
        q.p = make_int4(p.x, p.y, p.z, p.w);
        q.k = make_int4(k.x, k.y, k.z, k.w);
        q.v = make_int4(v.x, v.y, v.z, v.w);
        q.t0 = make_longlong2(t0.x, t0.y);
        q.t1 = make_longlong2(t1.x, t1.y);
    } else {
        q.p = reinterpret_cast<const int4 *>(c.partition)[qi];
        q.k = reinterpret_cast<const int4 *>(c.key_len)[qi];
        q.v = reinterpret_cast<const int4 *>(c.val_len)[qi];
        q.t0 = reinterpret_cast<const longlong2 *>(c.ts_ms)[2 * qi];
        q.t1 = reinterpret_cast<const longlong2 *>(c.ts_ms)[2 * qi + 1];
    }
    q.compact = 0u;
}

template <bool NT>
__device__ __forceinline__ int4 load16(const void *col, uint64_t i)   // 16-byte unit i of a column
{
    if (NT) {
        const v4i x = __builtin_nontemporal_load(reinterpret_cast<const v4i *>(col) + i);
        return make_int4(x.x, x.y, x.z, x.w);
    }
    return reinterpret_cast<const int4 *>(col)[i];
}

// TILED: the lane's 4 records of allocation tile T.  One header load picks the length loads (lens) and the partition /
// timestamp loads (mode).
// SUM (kta_metrics_scan_packed; n: the batch's records, pc = min(P, KTA_COMPACT_PART_NONE)): the timestamps of a tile are
// not loaded iff its summary is VALID, its header COMPACT, it lies wholly inside [rec0, rec0 + n) and its largest
// partition counts — then every record of it counts and the tile's extrema are the summary's (kta_tile.h).  Uniform per
// workgroup and tile, and decided here because the loads run a tile ahead of the accumulation.
// What a VALID summary s beside the COMPACT header h gives the earliest (lo) and the latest (hi) timestamp:
__device__ __forceinline__ void tile_sum_extrema(const kta_tile_hdr &h, const kta_tile_sum &s, long long &lo, long long &hi)
{
    // a counted record without a timestamp is t = 0 (metric.rs:209); ts_base + ts_span is modular, as tile_unpack_ts
    const bool timed = (s.flags & KTA_TILE_SUM_TIMED) != 0, untimed = (s.flags & KTA_TILE_SUM_UNTIMED) != 0;
    lo = timed ? (long long)h.ts_base : LLONG_MAX;
    hi = timed ? (long long)((uint64_t)h.ts_base + s.ts_span) : LLONG_MIN;
    lo = (untimed && 0ll < lo) ? 0ll : lo;
    hi = (untimed && 0ll > hi) ? 0ll : hi;
}
// The rule itself, from uniform values alone (h: a COMPACT header): whether tile T is summarised for this scan, and if
// so what it gives the earliest (lo) and the latest (hi) timestamp.
__device__ __forceinline__ bool tile_summed(const kta_tile_hdr &h, const kta_tile_sum &s, uint64_t T, const ScanColumns &c, uint64_t n,
                                            uint32_t pc, long long &lo, long long &hi)
{
    const uint64_t first = T * KTA_TILE_RECORDS;
    if (!((s.flags & KTA_TILE_SUM_VALID) && first >= c.rec0 && first + KTA_TILE_RECORDS <= c.rec0 + n && s.part_max < pc)) return false;
    tile_sum_extrema(h, s, lo, hi);
    return true;
}

// TILED: the lane's four records of a tile lie at a .. a + 3 of the batch (a wraps where the tile begins below rec0);
// bit j = record j is one of the batch's n
__device__ __forceinline__ uint32_t quad_valid(uint64_t a, uint64_t n)
{
    uint32_t valid = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) valid |= (a + j < n) ? 1u << j : 0u;
    return valid;
}

template <bool NT, bool SUM = false>
__device__ __forceinline__ void load_tile_quad(Quad &q, const ScanColumns &c, uint64_t T, uint32_t tid, uint64_t n = 0, uint32_t pc = 0)
{
    const kta_tile_hdr h = c.hdr[T];
    const kta_tile_sum sm = SUM ? c.sum[T] : kta_tile_sum{0, 0, 0};   // (with the header: both uniform loads go out first)
    const uint64_t qi = T * (KTA_TILE_RECORDS / 4) + tid;
    const bool lens16 = h.lens == KTA_TILE_LENS_U16;
    q.k = load16<NT>(c.key_len, qi);     // u16 tile: group tid, both lengths of the lane's four records
    if (!lens16) q.v = load16<NT>(c.val_len, qi);
    if (h.mode != KTA_TILE_COMPACT) {
        q.p = load16<NT>(c.partition, qi);
        const int4 a = load16<NT>(c.ts_ms, 2 * qi), b = load16<NT>(c.ts_ms, 2 * qi + 1);
        q.t0.x = (long long)(((uint64_t)(uint32_t)a.y << 32) | (uint32_t)a.x);
        q.t0.y = (long long)(((uint64_t)(uint32_t)a.w << 32) | (uint32_t)a.z);
        q.t1.x = (long long)(((uint64_t)(uint32_t)b.y << 32) | (uint32_t)b.x);
        q.t1.y = (long long)(((uint64_t)(uint32_t)b.w << 32) | (uint32_t)b.z);
        q.compact = lens16 ? kQuadLens16 : 0u;
        return;
    }
    const uint64_t ci = T * (KTA_TILE_RECORDS / 2) + tid;   // the tile's first half, in 8-byte / 16-byte units
    v2i p;
    if (NT) p = __builtin_nontemporal_load(reinterpret_cast<const v2i *>(c.partition) + ci);
    else p = reinterpret_cast<const v2i *>(c.partition)[ci];
    q.p.x = p.x;
    q.p.y = p.y;
    if (SUM) {
        long long lo, hi;
        if (tile_summed(h, sm, T, c, n, pc, lo, hi)) {
            q.t0.x = lo;
            q.t0.y = hi;
            q.compact = kQuadCompact | kQuadSummed | (lens16 ? kQuadLens16 : 0u);
            return;
        }
    }
    const int4 o = load16<NT>(c.ts_ms, ci);
    q.t0.x = (long long)(((uint64_t)(uint32_t)o.y << 32) | (uint32_t)o.x);
    q.t0.y = (long long)(((uint64_t)(uint32_t)o.w << 32) | (uint32_t)o.z);
    q.base = h.ts_base;
    q.compact = kQuadCompact | (lens16 ? kQuadLens16 : 0u);
}

// the quad's partitions and raw timestamps, whichever form it was loaded in
__device__ __forceinline__ void quad_part_ts(const Quad &q, uint32_t (&p)[4], long long (&t)[4])
{
    if (q.compact & kQuadCompact) {
        uint32_t u[4];
        int32_t o[4];
        tile_u16x4((uint32_t)q.p.x, (uint32_t)q.p.y, u);
        tile_i32x4(q.t0.x, q.t0.y, o);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            p[j] = (uint32_t)tile_unpack_part(u[j]);
            t[j] = tile_unpack_ts(o[j], q.base);
        }
    } else {
        p[0] = (uint32_t)q.p.x, p[1] = (uint32_t)q.p.y, p[2] = (uint32_t)q.p.z, p[3] = (uint32_t)q.p.w;
        t[0] = q.t0.x, t[1] = q.t0.y, t[2] = q.t1.x, t[3] = q.t1.y;
    }
}

// the quad's lengths as i32, whichever form they were loaded in
// (half a u16 group: two dwords are four key lengths, or four value lengths)
__device__ __forceinline__ int4 widen_lens4(int32_t w0, int32_t w1)
{
    uint32_t u[4];
    tile_u16x4((uint32_t)w0, (uint32_t)w1, u);
    return make_int4(tile_unpack_len(u[0]), tile_unpack_len(u[1]), tile_unpack_len(u[2]), tile_unpack_len(u[3]));
}
template <bool TILED>
__device__ __forceinline__ void quad_lens(const Quad &q, int4 &k, int4 &v)
{
    k = q.k;
    v = q.v;
    if (TILED && (q.compact & kQuadLens16)) {   // (the raw layout has no such tiles: its instantiations keep their code)
        k = widen_lens4(q.k.x, q.k.y);
        v = widen_lens4(q.k.z, q.k.w);
    }
}

// A lane's extrema and bad-partition count; a new one has seen nothing.
struct LaneState {
    long long tmin = LLONG_MAX, tmax = LLONG_MIN;
    uint32_t smin = 0xFFFFFFFFu;   // never a real size (max real size is 2^32-2)
    uint32_t smax = 0u;
    uint32_t bad = 0u;
};

constexpr uint32_t kHistBuckets = 34; // [0] None, [1] length 0, [2+k] 2^k <= length < 2^(k+1)
constexpr uint32_t kHistReps = 16;    // lane-replicated LDS counters per bucket

__device__ __forceinline__ uint32_t size_bucket(uint32_t is_null, uint32_t len)
{
    return is_null ? 0u : (len == 0u ? 1u : 2u + (31u - (uint32_t)__clz((int)len)));
}

// What one record contributes, derived in registers.
struct Rec {
    uint32_t part, tomb, knull, ks, vs;
    long long t;
    bool ok;
};

__device__ __forceinline__ Rec make_rec(uint32_t part, int32_t kl, int32_t vl, long long ts, uint32_t P, bool valid)
{
    Rec r;
    r.part = part;
    r.ok = valid && (part < P);           // unsigned compare also rejects negative ids
    r.tomb = (uint32_t)vl >> 31;          // payload None  (metric.rs:241-244)
    r.knull = (uint32_t)kl >> 31;         // key None      (metric.rs:227-230)
    r.ks = r.knull ? 0u : (uint32_t)kl;
    r.vs = r.tomb ? 0u : (uint32_t)vl;
    r.t = (ts == -1ll) ? 0ll : ts;        // to_millis() None -> unwrap_or(0)  (metric.rs:209)
    return r;
}

// global extrema in registers (metric.rs:56-72) + the bad-partition count
__device__ __forceinline__ void lane_extrema(const Rec &r, bool valid, LaneState &st)
{
    st.bad += (valid && !r.ok) ? 1u : 0u;
    if (r.ok) {
        st.tmin = r.t < st.tmin ? r.t : st.tmin;
        st.tmax = r.t > st.tmax ? r.t : st.tmax;
        if (!r.tomb) {                     // metric.rs:249-251
            const uint32_t sz = r.ks + r.vs; // < 2^32: both < 2^31
            st.smin = min(st.smin, sz);
            st.smax = max(st.smax, sz);
        }
    }
}

struct ScanLds {
    unsigned long long *A, *K, *V;     // counters
    long long *X;                      // ANALYTICS: [4][slots] signed-max arrays [~ts, ts, ~size, size]
    uint32_t *H;                       // ANALYTICS: [2][34][16] histogram counters
    uint32_t slots;
};

// LDS side of ONE record.
template <int VARIANT, bool ANALYTICS>
__device__ __forceinline__ void lds_record(const Rec &r, const ScanLds &L, uint32_t rep_log2, uint32_t rep)
{
    if (VARIANT == 9) return; // diagnostic: loads + register work only
    const uint32_t slot = (r.part << rep_log2) | rep;
    const unsigned long long a = 1ull | ((unsigned long long)r.tomb << kCntBits) |
                                 ((unsigned long long)r.knull << (2 * kCntBits));
    if (r.ok) {
        atomicAdd(&L.A[slot], a);
        atomicAdd(&L.K[slot], (unsigned long long)r.ks);
        atomicAdd(&L.V[slot], (unsigned long long)r.vs);
    }
    if (ANALYTICS && r.ok) {
        atomicMax(&L.X[slot], ~r.t);
        atomicMax(&L.X[L.slots + slot], r.t);
        if (!r.tomb) {
            const long long sz = (long long)(r.ks + r.vs);
            atomicMax(&L.X[2 * L.slots + slot], ~sz);
            atomicMax(&L.X[3 * L.slots + slot], sz);
        }
    }
}

template <bool ANALYTICS>
__device__ __forceinline__ void lds_histograms(const Rec &r, const ScanLds &L)
{
    if (ANALYTICS && r.ok) {
        const uint32_t hr = threadIdx.x & (kHistReps - 1u);
        atomicAdd(&L.H[size_bucket(r.knull, r.ks) * kHistReps + hr], 1u);
        atomicAdd(&L.H[(kHistBuckets + size_bucket(r.tomb, r.vs)) * kHistReps + hr], 1u);
    }
}

// TIMELINE (kta_set_timeline; no reference counterpart): records, tombstones and bytes per time bucket of every counted
// record, in LDS rows of {count word (records | tombstones << kCntBits, as the counters pack them), bytes}, flushed
// with the counters (so the 21-bit fields cannot overflow) by a device-scope atomicAdd of every non-zero row into the
// live vector.  Rows: 0 no timestamp (ts < 0), 1 before the origin, 2 + k bucket k, n + 2 after the window.
struct TimelineLds {
    unsigned long long *C, *B;         // [n_buckets + 3] count words, bytes
};

// The row of a record with raw timestamp ts, d = ts - origin (mod 2^64, exact when ts >= origin).  No 64-bit division:
// the float estimate d * (1 / width) of k = floor(d / width) is off by at most one (d / width < 1024 here and the
// three float roundings cost a relative 2^-22 at most, an absolute 2^-12), and one multiply-compare moves it to k:
// exact for every int64 timestamp.
__device__ __forceinline__ uint32_t timeline_row(long long ts, unsigned long long d, const TimelineArgs &a)
{
    if (ts < 0) return 0u;
    if (ts < a.origin) return 1u;
    if (d >= a.span) return a.n_buckets + 2u;
    uint32_t k = (uint32_t)((float)d * a.inv_width);
    k = min(k, a.n_buckets - 1u);
    const unsigned long long kw = (unsigned long long)k * a.width;
    if (kw > d) k--;
    else if (d - kw >= a.width) k++;
    return 2u + k;
}

__device__ __forceinline__ unsigned long long timeline_count(uint32_t records, uint32_t tombs)
{
    return (unsigned long long)records | ((unsigned long long)tombs << kCntBits);
}

// The quad's records on the timeline.  Kafka timestamps ascend inside a partition, so an ordered topic puts a whole
// wave into one bucket, and 64 same-address LDS atomics would serialise: the lane's quad is combined in registers
// (as accumulate_quad does for partitions), a wave whose quads all share one row is reduced across the wave and
// issues one pair of atomics, and only a scattered wave pays per-record atomics.
__device__ __forceinline__ void timeline_quad(const Quad &q, const Rec (&r)[4], const long long (&ts)[4],
                                              const TimelineArgs &a, const TimelineLds &T)
{
    unsigned long long d[4];
    if (q.compact & kQuadCompact) {
        // compact tile: ts = ts_base + o, so d = (ts_base - origin) + o with the difference taken once per tile
        const unsigned long long db = (unsigned long long)q.base - (unsigned long long)a.origin;
        int32_t o[4];
        tile_i32x4(q.t0.x, q.t0.y, o);
#pragma unroll
        for (int j = 0; j < 4; j++) d[j] = db + (unsigned long long)(long long)o[j];
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) d[j] = (unsigned long long)ts[j] - (unsigned long long)a.origin;
    }
    uint32_t row[4], by[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        row[j] = timeline_row(ts[j], d[j], a);
        by[j] = r[j].ks + r[j].vs;     // < 2^32: both < 2^31
    }
    const bool quni = r[0].ok && r[1].ok && r[2].ok && r[3].ok && row[0] == row[1] && row[0] == row[2] &&
                      row[0] == row[3];
    const uint32_t tombs = r[0].tomb + r[1].tomb + r[2].tomb + r[3].tomb;
    const unsigned long long bytes = (unsigned long long)by[0] + by[1] + by[2] + by[3];
    const uint32_t first = __builtin_amdgcn_readfirstlane(quni ? row[0] : 0xFFFFFFFFu);
    if (__ballot(quni && row[0] == first) == __ballot(1)) {   // (wave-uniform) every quad of the wave in one row
        uint32_t c = 4u | (tombs << 16);                     // a wave's 256 records: two 16-bit fields
        unsigned long long b = bytes;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            c += __shfl_xor(c, off);
            b += __shfl_xor(b, off);
        }
        if ((threadIdx.x & 63u) == 0u) {
            atomicAdd(&T.C[first], timeline_count(c & 0xFFFFu, c >> 16));
            atomicAdd(&T.B[first], b);
        }
        return;
    }
    if (quni) {
        atomicAdd(&T.C[row[0]], timeline_count(4u, tombs));
        atomicAdd(&T.B[row[0]], bytes);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (r[j].ok) {
            atomicAdd(&T.C[row[j]], timeline_count(1u, r[j].tomb));
            atomicAdd(&T.B[row[j]], (unsigned long long)by[j]);
        }
}

// The lane's 4 consecutive records of a tile.  A Kafka consumer delivers per-partition runs, so the
// four usually share a partition: then their contributions are combined in registers and cost one
// set of LDS atomics instead of four (4x fewer same-address conflicts inside a run).
// valid: bit j = record j of the quad is one of the batch's
template <int VARIANT, bool ANALYTICS, bool TIMELINE = false, bool TILED = false>
__device__ __forceinline__ void accumulate_quad(const Quad &q, uint32_t valid, uint32_t P, uint32_t rep_log2,
                                                uint32_t rep, const ScanLds &L, LaneState &st,
                                                const TimelineArgs &ta = TimelineArgs{}, const TimelineLds &T = TimelineLds{})
{
    uint32_t pt[4];
    long long ts[4];
    int4 k, v;
    quad_part_ts(q, pt, ts);
    quad_lens<TILED>(q, k, v);
    Rec r[4] = {make_rec(pt[0], k.x, v.x, ts[0], P, valid & 1u),
                make_rec(pt[1], k.y, v.y, ts[1], P, (valid >> 1) & 1u),
                make_rec(pt[2], k.z, v.z, ts[2], P, (valid >> 2) & 1u),
                make_rec(pt[3], k.w, v.w, ts[3], P, (valid >> 3) & 1u)};
#pragma unroll
    for (int j = 0; j < 4; j++) lane_extrema(r[j], (valid >> j) & 1u, st);
    if (VARIANT == 9) {
        st.smax = max(st.smax, r[0].part + r[1].part + r[2].part + r[3].part); // keep the loads alive
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) lds_histograms<ANALYTICS>(r[j], L);
    if (TIMELINE) timeline_quad(q, r, ts, ta, T);
    const bool uniform = r[0].ok && r[1].ok && r[2].ok && r[3].ok && r[0].part == r[1].part && r[0].part == r[2].part &&
                         r[0].part == r[3].part;
    if (uniform) {
        const uint32_t slot = (r[0].part << rep_log2) | rep;
        const uint32_t tombs = r[0].tomb + r[1].tomb + r[2].tomb + r[3].tomb;
        const uint32_t knulls = r[0].knull + r[1].knull + r[2].knull + r[3].knull;
        atomicAdd(&L.A[slot], 4ull | ((unsigned long long)tombs << kCntBits) |
                                  ((unsigned long long)knulls << (2 * kCntBits)));
        atomicAdd(&L.K[slot], (unsigned long long)r[0].ks + r[1].ks + r[2].ks + r[3].ks);
        atomicAdd(&L.V[slot], (unsigned long long)r[0].vs + r[1].vs + r[2].vs + r[3].vs);
        if (ANALYTICS) {
            long long nt = LLONG_MIN, tx = LLONG_MIN, ns = LLONG_MIN, sx = LLONG_MIN;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                nt = ~r[j].t > nt ? ~r[j].t : nt;
                tx = r[j].t > tx ? r[j].t : tx;
                if (!r[j].tomb) {
                    const long long sz = (long long)(r[j].ks + r[j].vs);
                    ns = ~sz > ns ? ~sz : ns;
                    sx = sz > sx ? sz : sx;
                }
            }
            atomicMax(&L.X[slot], nt);
            atomicMax(&L.X[L.slots + slot], tx);
            if (tombs < 4u) {
                atomicMax(&L.X[2 * L.slots + slot], ns);
                atomicMax(&L.X[3 * L.slots + slot], sx);
            }
        }
        return;
    }
    // interleaved partitions: per-record atomics, spread over the replicas
#pragma unroll
    for (int j = 0; j < 4; j++) lds_record<VARIANT, ANALYTICS>(r[j], L, rep_log2, rep);
}

// The workgroup's extrema and bad-partition count into the globals of its partial row: wave shuffle tree, then the
// four waves through LDS.  The end of every scan kernel.
// MERGE: the row holds the globals of another kernel's workgroup already (kta_metrics_scan_packed_rest): fold into them.
template <bool MERGE = false>
__device__ __forceinline__ void write_scan_globals(const LaneState &st, long long (&s_red)[kWG / 64][6], uint64_t *row, uint32_t P,
                                                   uint32_t tid)
{
    long long tmin = st.tmin, tmax = st.tmax;
    long long smin = (long long)st.smin, smax = (long long)st.smax, bad = (long long)st.bad;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const long long a = __shfl_xor(tmin, off), b = __shfl_xor(tmax, off);
        const long long cmin = __shfl_xor(smin, off), cmax = __shfl_xor(smax, off);
        const long long d = __shfl_xor(bad, off);
        tmin = a < tmin ? a : tmin;
        tmax = b > tmax ? b : tmax;
        smin = cmin < smin ? cmin : smin;
        smax = cmax > smax ? cmax : smax;
        bad += d;
    }
    const uint32_t wave = tid >> 6;
    if ((tid & 63u) == 0u) {
        s_red[wave][0] = tmin; s_red[wave][1] = tmax; s_red[wave][2] = smin;
        s_red[wave][3] = smax; s_red[wave][4] = bad;
    }
    __syncthreads();
    if (tid == 0) {
        for (uint32_t w = 1; w < kWG / 64; w++) {
            tmin = s_red[w][0] < tmin ? s_red[w][0] : tmin;
            tmax = s_red[w][1] > tmax ? s_red[w][1] : tmax;
            smin = s_red[w][2] < smin ? s_red[w][2] : smin;
            smax = s_red[w][3] > smax ? s_red[w][3] : smax;
            bad += s_red[w][4];
        }
        uint64_t *g = row + (uint64_t)P * kScanCols;
        if (MERGE) {   // (the row's smallest size is LLONG_MAX where there was none: above every size)
            const long long gtmin = (long long)g[SG_TMIN], gtmax = (long long)g[SG_TMAX];
            const long long gsmin = (long long)g[SG_SMIN], gsmax = (long long)g[SG_SMAX];
            tmin = gtmin < tmin ? gtmin : tmin;
            tmax = gtmax > tmax ? gtmax : tmax;
            smin = gsmin < smin ? gsmin : smin;
            smax = gsmax > smax ? gsmax : smax;
            bad += (long long)g[SG_BAD];
        }
        g[SG_TMIN] = (uint64_t)tmin;
        g[SG_TMAX] = (uint64_t)tmax;
        g[SG_SMIN] = (smin == 0xFFFFFFFFll) ? (uint64_t)LLONG_MAX : (uint64_t)smin;
        g[SG_SMAX] = (uint64_t)smax;
        g[SG_BAD] = (uint64_t)bad;
        g[SG_NREC] = 0;
        g[6] = 0;
        g[7] = 0;
    }
}

// ANALYTICS (opt-in, no reference counterpart — the additive outputs named by the project brief):
// log2 histograms of key and value sizes and per-partition timestamp / message-size extrema, kept
// in additional LDS arrays (extrema as signed-max arrays of [~ts, ts, ~size, size], histograms as
// u32 counters replicated 16x by lane) and flushed with the counters.
// TIMELINE: the kernel takes one more argument, the TimelineArgs (Extra = TimelineArgs; the timeline rows follow
// the other LDS arrays).  Instantiated for the accumulating, non-temporal scan only: raw and tiled, with and without
// analytics.  Without it (Extra empty) the kernel has the parameters and the code of before.
__device__ __forceinline__ TimelineArgs timeline_args() { return TimelineArgs{}; }
__device__ __forceinline__ TimelineArgs timeline_args(const TimelineArgs &a) { return a; }

template <int VARIANT, bool NT, bool ANALYTICS, bool TILED, typename... Extra>
__global__ __launch_bounds__(kWG) void kta_metrics_scan(ScanColumns c, uint64_t n, uint32_t P,
                                                        uint32_t rep_log2,
                                                        uint64_t *__restrict__ partials,
                                                        uint32_t row_len, Extra... extra)
{
    constexpr bool TIMELINE = sizeof...(Extra) != 0;
    const TimelineArgs ta = timeline_args(extra...);
    extern __shared__ unsigned long long lds[];
    __shared__ long long s_red[kWG / 64][6];

    const uint32_t tid = threadIdx.x;
    const uint32_t slots = P << rep_log2;
    const uint32_t n_arrays = 3u;
    unsigned long long *sA = lds;
    unsigned long long *sK = lds + slots;
    unsigned long long *sV = lds + 2 * slots;
    long long *sX = reinterpret_cast<long long *>(lds + n_arrays * slots);          // ANALYTICS: [4][slots]
    uint32_t *sH = reinterpret_cast<uint32_t *>(lds + (n_arrays + 4) * slots);      // ANALYTICS: [2][34][16]
    const ScanLds L{sA, sK, sV, sX, sH, slots};
    // TIMELINE: [n_buckets + 3] count words, then as many byte sums, after the arrays above
    const uint32_t tl_rows = TIMELINE ? ta.n_buckets + 3u : 0u;
    unsigned long long *sT = lds + (n_arrays + (ANALYTICS ? 4u : 0u)) * slots +
                             (ANALYTICS ? 2u * kHistBuckets * kHistReps / 2u : 0u);
    const TimelineLds T{sT, sT + tl_rows};

    for (uint32_t i = tid; i < n_arrays * slots; i += kWG) lds[i] = 0ull;
    if (ANALYTICS) {
        for (uint32_t i = tid; i < 4 * slots; i += kWG) sX[i] = LLONG_MIN;
        for (uint32_t i = tid; i < 2 * kHistBuckets * kHistReps; i += kWG) sH[i] = 0u;
    }
    if (TIMELINE)
        for (uint32_t i = tid; i < 2 * tl_rows; i += kWG) sT[i] = 0ull;
    __syncthreads();

    const uint32_t rep = tid & ((1u << rep_log2) - 1u);
    LaneState st;

    uint64_t *row = partials + (uint64_t)blockIdx.x * row_len;
    bool first_flush = true;

    auto flush = [&]() {
        __syncthreads();
        for (uint32_t p = tid; p < P; p += kWG) {
            unsigned long long a = 0, k = 0, v = 0;
            for (uint32_t r = 0; r < (1u << rep_log2); r++) {
                const uint32_t s = (p << rep_log2) | r;
                a += sA[s];
                k += sK[s];
                v += sV[s];
                sA[s] = 0ull;
                sK[s] = 0ull;
                sV[s] = 0ull;
            }
            uint64_t *o = row + (uint64_t)p * kScanCols;
            const uint64_t c0 = a & kCntMask, c1 = (a >> kCntBits) & kCntMask,
                           c2 = (a >> (2 * kCntBits)) & kCntMask;
            if (first_flush) {
                o[0] = c0; o[1] = c1; o[2] = c2; o[3] = k; o[4] = v;
            } else {
                o[0] += c0; o[1] += c1; o[2] += c2; o[3] += k; o[4] += v;
            }
            if (ANALYTICS) {
                long long *x = reinterpret_cast<long long *>(row + (uint64_t)P * kScanCols + kScanGlobals) + 4ull * p;
                for (uint32_t j = 0; j < 4; j++) {
                    long long m = LLONG_MIN;
                    for (uint32_t r = 0; r < (1u << rep_log2); r++) {
                        const uint32_t s = j * slots + ((p << rep_log2) | r);
                        m = sX[s] > m ? sX[s] : m;
                        sX[s] = LLONG_MIN;
                    }
                    x[j] = (first_flush || m > x[j]) ? m : x[j];
                }
            }
        }
        if (ANALYTICS) {
            uint64_t *hrow = row + (uint64_t)P * kScanCols + kScanGlobals + 4ull * P;
            for (uint32_t bkt = tid; bkt < 2 * kHistBuckets; bkt += kWG) {
                uint64_t t = 0;
                for (uint32_t r = 0; r < kHistReps; r++) {
                    t += sH[bkt * kHistReps + r];
                    sH[bkt * kHistReps + r] = 0u;
                }
                hrow[bkt] = first_flush ? t : hrow[bkt] + t;
            }
        }
        if (TIMELINE) {
            unsigned long long *tv = reinterpret_cast<unsigned long long *>(ta.vec);
            for (uint32_t i = tid; i < tl_rows; i += kWG) {
                const unsigned long long a = T.C[i];
                if (a == 0ull) continue;
                const unsigned long long b = T.B[i];
                T.C[i] = 0ull;
                T.B[i] = 0ull;
                const unsigned long long tombs = (a >> kCntBits) & kCntMask;
                atomicAdd(&tv[(uint64_t)i * kTimelineCols], a & kCntMask);
                if (tombs) atomicAdd(&tv[(uint64_t)i * kTimelineCols + 1], tombs);
                if (b) atomicAdd(&tv[(uint64_t)i * kTimelineCols + 2], b);
            }
        }
        first_flush = false;
        __syncthreads();
    };

    uint32_t since_flush = 0;
    Quad cur, nxt;
    if (TILED) {
        // allocation tiles [t0, t0 + ntiles) hold the batch; record a of the allocation is the batch's iff a - rec0 < n
        const uint64_t t0 = c.rec0 / KTA_TILE_RECORDS;
        const uint64_t ntiles = (c.rec0 + n + KTA_TILE_RECORDS - 1) / KTA_TILE_RECORDS - t0;
        // prefetch ring: the loads of the tile kTilePrefetch deals ahead are issued before the current tile is accumulated;
        // the slots rotate by moves (cur <- nxt <- nx2), and a slot past the last tile is never loaded nor accumulated
        uint64_t tile = blockIdx.x;
        Quad nx2;
        if (tile < ntiles) load_tile_quad<NT>(cur, c, t0 + tile, tid);
        if (kTilePrefetch == 2 && tile + gridDim.x < ntiles) load_tile_quad<NT>(nxt, c, t0 + tile + gridDim.x, tid);
        while (tile < ntiles) { // uniform per workgroup
            const uint64_t ntile = tile + gridDim.x;
            const uint64_t ahead = tile + (uint64_t)kTilePrefetch * gridDim.x;
            if (ahead < ntiles) load_tile_quad<NT>(kTilePrefetch == 2 ? nx2 : nxt, c, t0 + ahead, tid);

            const uint64_t a = (t0 + tile) * KTA_TILE_RECORDS + 4u * tid - c.rec0;   // (wraps below rec0)
            const uint32_t valid = quad_valid(a, n);
            accumulate_quad<VARIANT, ANALYTICS, TIMELINE, true>(cur, valid, P, rep_log2, rep, L, st, ta, T);

            if (++since_flush == kFlushTiles) {
                flush();
                since_flush = 0;
            }
            cur = nxt;
            if (kTilePrefetch == 2) nxt = nx2;
            tile = ntile;
        }
    } else {
        const uint64_t nquads = n >> 2;
        const uint64_t ntiles = (nquads + kWG - 1) / kWG;
        uint64_t tile = blockIdx.x;

        uint64_t qi = tile * kWG + tid;
        bool cur_valid = (tile < ntiles) && (qi < nquads);
        if (cur_valid) load_quad<NT>(cur, c, qi);

        while (tile < ntiles) { // uniform per workgroup
            const uint64_t ntile = tile + gridDim.x;
            const uint64_t nqi = ntile * kWG + tid;
            const bool nxt_valid = (ntile < ntiles) && (nqi < nquads);
            if (nxt_valid) load_quad<NT>(nxt, c, nqi);

            accumulate_quad<VARIANT, ANALYTICS, TIMELINE>(cur, cur_valid ? 0xFu : 0u, P, rep_log2, rep, L, st, ta, T);

            if (++since_flush == kFlushTiles) {
                flush();
                since_flush = 0;
            }
            cur = nxt;
            cur_valid = nxt_valid;
            tile = ntile;
        }
    }

    // tail (raw layout): the last n % 4 records, scalar, by the first lanes of workgroup 0
    if (!TILED && blockIdx.x == 0) {
        const uint64_t i = ((n >> 2) << 2) + tid;
        const bool v = (tid < 3) && (i < n);
        const uint64_t ii = v ? i : 0;
        if (tid < 64) {
            uint32_t p = 0; int32_t kl = 0, vl = 0; long long ts = 0;
            if (v) { p = (uint32_t)c.partition[ii]; kl = c.key_len[ii]; vl = c.val_len[ii]; ts = c.ts_ms[ii]; }
            const Rec r = make_rec(p, kl, vl, ts, P, v);
            lane_extrema(r, v, st);
            lds_histograms<ANALYTICS>(r, L);
            lds_record<VARIANT, ANALYTICS>(r, L, rep_log2, rep);
            if (TIMELINE && r.ok) {
                const uint32_t tr = timeline_row(ts, (unsigned long long)ts - (unsigned long long)ta.origin, ta);
                atomicAdd(&T.C[tr], timeline_count(1u, r.tomb));
                atomicAdd(&T.B[tr], (unsigned long long)(r.ks + r.vs));
            }
        }
    }

    flush();
    write_scan_globals(st, s_red, row, P, tid);
}

// ---------------------------------------------------------------------------------------
// K1p  metrics scan of a tile-compact batch, packed accumulation (no analytics, no timeline)
// ---------------------------------------------------------------------------------------
// The same loads, tile deal, prefetch ring and partial row as kta_metrics_scan<0, NT, false, true>; what differs is
// where a record's five sums go.  Two levels of partials in LDS:
//   front  W1, W2 [P << rep_log2], replicated by lane, updated with TWO 64-bit atomics per record (or quad):
//              W1 += 1 | tomb << 16 | (u64)key_size << 32        W2 += key_null | (u64)value_size << 32
//          (a u16-lens tile: its sizes are below 2^16; the dwords are built independently, no 64-bit shift).
//          A tile whose lengths are i32 adds its counts to the low dwords alone and its two sizes, with two more
//          atomics, straight to the back level: exact for every i32 length, and such tiles are rare.
//   back   B [kScanCols][P], full-width u64, unreplicated.  Every kFrontFlushTiles tiles of the workgroup, between
//          two barriers, thread p sums and zeroes partition p's replicas and adds the fields to its own five words
//          with plain adds (accumulation and flush never overlap, so the i32 tiles' atomics are safe too).
// The row of the partial workspace is written once, from the back level, at the end of the kernel.
// Summarised tiles (kta_tile_sum, kta_tile.h): where the producer's summary says that every record of a whole compact tile
// counts, the tile's timestamp offsets are not loaded (6 B per record instead of 10) and its two extrema come from the
// summary (load_tile_quad<NT, true>, kQuadSummed); any other tile is read as before.
// Between two front flushes a slot takes at most the workgroup's kFrontRecords records, so no field carries into
// its neighbour:
constexpr uint32_t kFrontFlushTiles = 32;
constexpr uint64_t kFrontRecords = (uint64_t)kFrontFlushTiles * KTA_TILE_RECORDS;   // 2^15
static_assert(kFrontRecords <= 0xFFFFu, "count, tombstones and null keys of a front interval fit 16 bits");
static_assert(kFrontRecords + (kFrontRecords << 16) <= 0xFFFFFFFFull, "count | tombstones << 16 stays in W1's low dword");
static_assert(kFrontRecords * (KTA_COMPACT_LEN_NONE - 1u) < (1ull << 31), "a front interval's u16 sizes sum below 2^31");
// The plane form has words, bounds and an interval of its own (kta_plane_pack.h): one 64-bit add per record of count, raw
// key sum and raw value sum, whose fields hold the 8192 records that ONE slot takes in min(kFrontFlushTiles, 8 R) tiles
// — kFrontFlushTiles with four replicas or more, 16 tiles with two, 8 with one.  The 6-byte form, the rest kernel and
// the kernel without summaries keep kFrontFlushTiles and the two adds above.
static_assert(kPlaneTileRecords == KTA_TILE_RECORDS && kPlaneKeyNone == KTA_PLANE_KEY_NONE && kPlaneValNone == KTA_COMPACT_LEN_NONE,
              "kta_plane_pack.h restates the tile's constants");
static_assert(plane_slot_records(0, kFrontFlushTiles) <= kPlaneSlotRecords && plane_slot_records(1, kFrontFlushTiles) <= kPlaneSlotRecords &&
              plane_slot_records(2, kFrontFlushTiles) <= kPlaneSlotRecords && plane_slot_records(6, kFrontFlushTiles) <= kPlaneSlotRecords,
              "a slot of the plane form takes at most kPlaneSlotRecords records between two flushes");

struct PackedLds {
    unsigned long long *W1, *W2;       // front level
    unsigned long long *B;             // back level: column c of partition p at B[c * P + p]
};

__device__ __forceinline__ unsigned long long pack_dwords(uint32_t lo, uint32_t hi)
{
    return ((unsigned long long)hi << 32) | lo;
}

// The lane's 4 consecutive records of a tile (accumulate_quad's job).  The tile's two forms (q.compact) are uniform per
// workgroup.  Extrema without branches: a record that does not count contributes the neutral value.
// Here: the lengths' half — sizes, size extrema and the LDS adds — of records whose partitions pt and ok are known.
template <bool LENS16>
__device__ __forceinline__ void packed_quad_lens(const Quad &q, const uint32_t (&pt)[4], const bool (&ok)[4], uint32_t P,
                                                 uint32_t rep_log2, uint32_t rep, const PackedLds &L, LaneState &st)
{
    uint32_t tomb[4], knull[4], ks[4], vs[4];
    if (LENS16) {
        uint32_t ku[4], vu[4];
        tile_u16x4((uint32_t)q.k.x, (uint32_t)q.k.y, ku);
        tile_u16x4((uint32_t)q.k.z, (uint32_t)q.k.w, vu);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            knull[j] = ku[j] == KTA_COMPACT_LEN_NONE;
            tomb[j] = vu[j] == KTA_COMPACT_LEN_NONE;
            ks[j] = knull[j] ? 0u : ku[j];
            vs[j] = tomb[j] ? 0u : vu[j];
        }
    } else {
        const int32_t kl[4] = {q.k.x, q.k.y, q.k.z, q.k.w}, vl[4] = {q.v.x, q.v.y, q.v.z, q.v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            knull[j] = (uint32_t)kl[j] >> 31;      // as make_rec
            tomb[j] = (uint32_t)vl[j] >> 31;
            ks[j] = knull[j] ? 0u : (uint32_t)kl[j];
            vs[j] = tomb[j] ? 0u : (uint32_t)vl[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {                  // metric.rs:249-251
        const bool sized = ok[j] && !tomb[j];
        const uint32_t sz = ks[j] + vs[j];         // < 2^32: both < 2^31
        st.smin = min(st.smin, sized ? sz : 0xFFFFFFFFu);
        st.smax = max(st.smax, sized ? sz : 0u);
    }
#if KTA_PACKED_LOADS_ONLY
    st.bad += pt[0] ^ pt[1] ^ pt[2] ^ pt[3];   // (keeps the partition loads alive)
    return;
#endif
    const bool uniform = ok[0] && ok[1] && ok[2] && ok[3] && pt[0] == pt[1] && pt[0] == pt[2] && pt[0] == pt[3];
    if (uniform) {
        const uint32_t slot = (pt[0] << rep_log2) | rep;
        const uint32_t tombs = tomb[0] + tomb[1] + tomb[2] + tomb[3];
        const uint32_t knulls = knull[0] + knull[1] + knull[2] + knull[3];
        if (LENS16) {
            atomicAdd(&L.W1[slot], pack_dwords(4u | (tombs << 16), ks[0] + ks[1] + ks[2] + ks[3]));
            atomicAdd(&L.W2[slot], pack_dwords(knulls, vs[0] + vs[1] + vs[2] + vs[3]));
        } else {
            atomicAdd(&L.W1[slot], (unsigned long long)(4u | (tombs << 16)));
            atomicAdd(&L.W2[slot], (unsigned long long)knulls);
            atomicAdd(&L.B[3u * P + pt[0]], (unsigned long long)ks[0] + ks[1] + ks[2] + ks[3]);
            atomicAdd(&L.B[4u * P + pt[0]], (unsigned long long)vs[0] + vs[1] + vs[2] + vs[3]);
        }
        return;
    }
    // interleaved partitions: per-record atomics, spread over the replicas
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (!ok[j]) continue;
        const uint32_t slot = (pt[j] << rep_log2) | rep;
        if (LENS16) {
            atomicAdd(&L.W1[slot], pack_dwords(1u | (tomb[j] << 16), ks[j]));
            atomicAdd(&L.W2[slot], pack_dwords(knull[j], vs[j]));
        } else {
            atomicAdd(&L.W1[slot], (unsigned long long)(1u | (tomb[j] << 16)));
            atomicAdd(&L.W2[slot], (unsigned long long)knull[j]);
            atomicAdd(&L.B[3u * P + pt[j]], (unsigned long long)ks[j]);
            atomicAdd(&L.B[4u * P + pt[j]], (unsigned long long)vs[j]);
        }
    }
}

// FORM: the tile's two forms when the caller knows them (kQuadCompact | kQuadLens16), else -1: read from the quad.
// SUM: the kernel reads summaries (the other instantiation never sees a summarised quad and keeps the code of before).
template <int FORM, bool SUM>
__device__ __forceinline__ void packed_quad(const Quad &q, uint32_t valid, uint32_t P, uint32_t rep_log2, uint32_t rep,
                                            const PackedLds &L, LaneState &st)
{
    const uint32_t form = FORM >= 0 ? (uint32_t)FORM : q.compact;
    uint32_t pt[4];
    bool ok[4];
    if (SUM && (form & kQuadSummed)) {
        // A summarised tile (load_tile_quad): every record counts, and the tile's extrema came with the quad — uniform
        // values, and min / max are idempotent, so every lane folds them.
        tile_u16x4((uint32_t)q.p.x, (uint32_t)q.p.y, pt);
#pragma unroll
        for (int j = 0; j < 4; j++) ok[j] = true;
        st.tmin = q.t0.x < st.tmin ? q.t0.x : st.tmin;
        st.tmax = q.t0.y > st.tmax ? q.t0.y : st.tmax;
    } else if (form & kQuadCompact) {
        // The lane's least and largest offset first, one 64-bit ts_base + offset each per tile.  Offsets lie in [0, 2^31)
        // and KTA_COMPACT_TS_NONE is INT32_MIN: above every offset as u32, below every one as i32, so it drops out of
        // the unsigned min and the signed max by itself, and so does a record that does not count once it is given that
        // value.  A counted record without a timestamp is t = 0 (metric.rs:209).
        static_assert(KTA_COMPACT_TS_NONE == INT32_MIN, "the sentinel is neutral for min as u32 and for max as i32");
        const uint32_t pc = min(P, (uint32_t)KTA_COMPACT_PART_NONE);   // the u16 marker of -1 is no partition, whatever P
        int32_t o[4];
        tile_u16x4((uint32_t)q.p.x, (uint32_t)q.p.y, pt);
        tile_i32x4(q.t0.x, q.t0.y, o);
        uint32_t lo = (uint32_t)KTA_COMPACT_TS_NONE;
        int32_t hi = KTA_COMPACT_TS_NONE;
        bool none = false;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            ok[j] = ((valid >> j) & 1u) && pt[j] < pc;
            const int32_t oj = ok[j] ? o[j] : KTA_COMPACT_TS_NONE;
            lo = min(lo, (uint32_t)oj);
            hi = max(hi, oj);
            none = none || (ok[j] && o[j] == KTA_COMPACT_TS_NONE);
        }
        const bool timed = hi >= 0;
        const long long tlo = (long long)((uint64_t)q.base + lo), thi = (long long)((uint64_t)q.base + (uint32_t)hi);
        st.tmin = (timed && tlo < st.tmin) ? tlo : st.tmin;
        st.tmax = (timed && thi > st.tmax) ? thi : st.tmax;
        st.tmin = (none && 0ll < st.tmin) ? 0ll : st.tmin;
        st.tmax = (none && 0ll > st.tmax) ? 0ll : st.tmax;
    } else {
        const long long ts[4] = {q.t0.x, q.t0.y, q.t1.x, q.t1.y};
        pt[0] = (uint32_t)q.p.x, pt[1] = (uint32_t)q.p.y, pt[2] = (uint32_t)q.p.z, pt[3] = (uint32_t)q.p.w;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            ok[j] = ((valid >> j) & 1u) && pt[j] < P;   // unsigned compare also rejects negative ids
            const long long t = (ts[j] == -1ll) ? 0ll : ts[j];
            st.tmin = (ok[j] && t < st.tmin) ? t : st.tmin;
            st.tmax = (ok[j] && t > st.tmax) ? t : st.tmax;
        }
    }
    if (!(SUM && (form & kQuadSummed))) {
#pragma unroll
        for (int j = 0; j < 4; j++) st.bad += (((valid >> j) & 1u) && !ok[j]) ? 1u : 0u;
    }
    if (form & kQuadLens16) packed_quad_lens<true>(q, pt, ok, P, rep_log2, rep, L, st);
    else packed_quad_lens<false>(q, pt, ok, P, rep_log2, rep, L, st);
}

// A keyless allocation's tiles are compact with u16 lengths unless a value does not fit: straight code for that form,
// summarised and not, and one copy with the branches for the others.
template <bool SUM>
__device__ __forceinline__ void accumulate_packed(const Quad &q, uint32_t valid, uint32_t P, uint32_t rep_log2, uint32_t rep,
                                                  const PackedLds &L, LaneState &st)
{
    constexpr uint32_t both = kQuadCompact | kQuadLens16, summed = both | kQuadSummed;
    if (SUM && q.compact == summed) packed_quad<(int)summed, SUM>(q, valid, P, rep_log2, rep, L, st);
    else if ((q.compact & both) == both) packed_quad<(int)both, SUM>(q, valid, P, rep_log2, rep, L, st);
    else packed_quad<-1, SUM>(q, valid, P, rep_log2, rep, L, st);
}

// ---- the lean loop of the summarised compact / u16 tiles (SUM kernels) ---------------------------------------------
// The flagship's tiles are all of one kind: compact, u16 lengths, summarised.  Such a tile needs no per-record mask, no
// bad-partition count and no timestamps: 6 vector registers per lane (a Quad has 20) and two uniform extrema.  The lean
// loop keeps a ring of such slots, unrolled (no rotation moves); which tiles it takes it knows 64 steps at a time, from
// two ballots over the tiles' headers, summaries and marks (kta_lean_blocks.h), so a step holds no load but the tile's.
// Any other tile (cut by rec0 or n, raw, i32 lengths, part_max >= pc, no VALID summary) is left to the loop of before:
// see the kernel.
// Plane tiles (kta_tile.h: a marked tile) go through the same loop in their own form (lean_run<NT, true>): the lane's
// four records are the four dwords partition | key << 8 | val << 16 of the tile's plane — one 16-byte load, 4 B per
// record in one stream, 4 vector registers per slot.  A ring holds tiles of ONE form, so that the wait for a slot is
// exact; a workgroup that meets a summarised tile of the other form drains its ring and goes on in the other
// instantiation (see packed_scan_lean), so a batch that mixes both keeps every summarised tile here.
#ifndef KTA_LEAN_PREFETCH
#define KTA_LEAN_PREFETCH 2   // (swept with the plan's workgroups per CU, both forms: profiles/lean_blocks_scan.jsonl)
#endif
constexpr int kLeanPrefetch = KTA_LEAN_PREFETCH;   // tiles the lean loop loads ahead of the one it accumulates (1, 2 or 3)
static_assert(kLeanPrefetch >= 1 && kLeanPrefetch <= 3, "the lean ring has two, three or four slots");

struct LeanSlot {
    v2i p;    // four u16 partitions
    int4 k;   // four u16 key lengths (x, y), four u16 value lengths (z, w)
};
struct PlaneSlot {
    int4 w;   // four plane words
};
constexpr uint64_t kTileColBytes = (uint64_t)KTA_TILE_RECORDS * 4u;   // a tile's own bytes of an i32 column

// Whether the lean loop takes a tile (uniform) and in which form: tile_summed's rule with `whole` — the tile lies
// wholly inside the batch — worked out by the caller from 32-bit tile indices (a 64-bit compare is a vector
// instruction).  mark: the tile's, 0 where the marks are ignored.  A marked tile is a plane tile whatever the form of
// its lengths; any other needs u16 lengths.  A taken tile's extrema are tile_sum_extrema's.
__device__ __forceinline__ void lean_tile(const kta_tile_hdr &h, const kta_tile_sum &s, uint32_t mark, bool whole, uint32_t pc,
                                          bool &lean, bool &plane)
{
    const bool summed = whole && (s.flags & KTA_TILE_SUM_VALID) && s.part_max < pc && h.mode == KTA_TILE_COMPACT;
    plane = summed && mark == 1u;
    lean = summed && !plane && h.lens == KTA_TILE_LENS_U16;
}

// the tile's base is uniform, the lane's byte offsets (8 * tid, 16 * tid) constant over the loop
// B: the first byte the form reads of the tile in its column — T * kTileColBytes of an i32 column, twice that and the
// plane's offset of ts_ms — which the loop advances by a constant stride
template <bool NT>
__device__ __forceinline__ void lean_load(LeanSlot &s, const ScanColumns &c, uint64_t B, uint32_t off8, uint32_t off16)
{
    const char *pb = reinterpret_cast<const char *>(c.partition) + B;
    const char *kb = reinterpret_cast<const char *>(c.key_len) + B;
    const v2i *pp = reinterpret_cast<const v2i *>(pb + off8);
    const v4i *kp = reinterpret_cast<const v4i *>(kb + off16);
    s.p = NT ? __builtin_nontemporal_load(pp) : *pp;
    const v4i k = NT ? __builtin_nontemporal_load(kp) : *kp;
    s.k = make_int4(k.x, k.y, k.z, k.w);
}
template <bool NT>
__device__ __forceinline__ void lean_load(PlaneSlot &s, const ScanColumns &c, uint64_t B, uint32_t, uint32_t off16)
{
    const char *tb = reinterpret_cast<const char *>(c.ts_ms) + B;   // (B: of the tile's plane, kTilePlaneOffset included)
    const v4i *wp = reinterpret_cast<const v4i *>(tb + off16);
    const v4i w = NT ? __builtin_nontemporal_load(wp) : *wp;
    s.w = make_int4(w.x, w.y, w.z, w.w);
}

// packed_quad_lens<true> of four records that all count; the timestamps' extrema are the caller's (uniform)
// (pt: the partitions; ku / vu: the lengths as stored, knull / tomb: whether they are the form's marker of -1)
__device__ __forceinline__ void lean_quad_add(const uint32_t (&pt)[4], const uint32_t (&ku)[4], const uint32_t (&vu)[4],
                                              const uint32_t (&knull)[4], const uint32_t (&tomb)[4], uint32_t rep_log2, uint32_t rep,
                                              const PackedLds &L, LaneState &st)
{
    uint32_t ks[4], vs[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        ks[j] = knull[j] ? 0u : ku[j];
        vs[j] = tomb[j] ? 0u : vu[j];
    }
    uint32_t lo[4], hi[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {                  // metric.rs:249-251
        const uint32_t sz = ks[j] + vs[j];
        lo[j] = tomb[j] ? 0xFFFFFFFFu : sz;
        hi[j] = tomb[j] ? 0u : sz;
    }
    st.smin = min(min(min(lo[0], lo[1]), min(lo[2], lo[3])), st.smin);
    st.smax = max(max(max(hi[0], hi[1]), max(hi[2], hi[3])), st.smax);
#if KTA_PACKED_LOADS_ONLY
    st.bad += pt[0] ^ pt[1] ^ pt[2] ^ pt[3];   // (keeps the partition loads alive)
    return;
#endif
    if (pt[0] == pt[1] && pt[0] == pt[2] && pt[0] == pt[3]) {
        const uint32_t slot = (pt[0] << rep_log2) | rep;
        const uint32_t tombs = tomb[0] + tomb[1] + tomb[2] + tomb[3];
        const uint32_t knulls = knull[0] + knull[1] + knull[2] + knull[3];
        atomicAdd(&L.W1[slot], pack_dwords(4u | (tombs << 16), ks[0] + ks[1] + ks[2] + ks[3]));
        atomicAdd(&L.W2[slot], pack_dwords(knulls, vs[0] + vs[1] + vs[2] + vs[3]));
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t slot = (pt[j] << rep_log2) | rep;
        atomicAdd(&L.W1[slot], pack_dwords(1u | (tomb[j] << 16), ks[j]));
        atomicAdd(&L.W2[slot], pack_dwords(knull[j], vs[j]));
    }
}
__device__ __forceinline__ void lean_quad(const LeanSlot &s, uint32_t rep_log2, uint32_t rep, const PackedLds &L, LaneState &st)
{
    uint32_t pt[4], ku[4], vu[4], tomb[4], knull[4];
    tile_u16x4((uint32_t)s.p.x, (uint32_t)s.p.y, pt);
    tile_u16x4((uint32_t)s.k.x, (uint32_t)s.k.y, ku);
    tile_u16x4((uint32_t)s.k.z, (uint32_t)s.k.w, vu);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        knull[j] = ku[j] == KTA_COMPACT_LEN_NONE;
        tomb[j] = vu[j] == KTA_COMPACT_LEN_NONE;
    }
    lean_quad_add(pt, ku, vu, knull, tomb, rep_log2, rep, L, st);
}
// A plane slot: four words partition | key << 8 | val << 16 (kta_tile.h).  RAW sums: the lengths are added as stored,
// 0xFF for a key of -1 and 0xFFFF for a value of -1 included, and front_flush(raw) subtracts the markers by the
// interval's counts of null keys and tombstones — no select per record.  No size extrema either: the tile's producer
// wrote them (kta_tile.h) and packed_scan_lean folds them behind the loop.
// ONE 64-bit add per record (or uniform quad): count, raw key sum and raw value sum share W1's word, and the two flag
// counts go with a 32-bit add to the low dword of W2, executed only by the lanes that have a flag (kta_plane_pack.h:
// the word, its bounds and the shorter interval they ask of a plan with fewer than four replicas).
__device__ __forceinline__ void plane_add(const PackedLds &L, uint32_t slot, const PlaneAdd &a)
{
    atomicAdd(&L.W1[slot], plane_word(a));
    if (a.flags) atomicAdd(reinterpret_cast<uint32_t *>(&L.W2[slot]), a.flags);   // (little endian: the low dword)
}
__device__ __forceinline__ void lean_quad(const PlaneSlot &s, uint32_t rep_log2, uint32_t rep, const PackedLds &L, LaneState &st)
{
    const uint32_t w[4] = {(uint32_t)s.w.x, (uint32_t)s.w.y, (uint32_t)s.w.z, (uint32_t)s.w.w};
#if KTA_PACKED_LOADS_ONLY
    st.bad += w[0] ^ w[1] ^ w[2] ^ w[3];   // (keeps the loads alive)
    return;
#endif
    uint32_t pt[4], ku[4], vu[4], tomb[4], knull[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        pt[j] = w[j] & 0xFFu;
        ku[j] = (w[j] >> 8) & 0xFFu;
        vu[j] = w[j] >> 16;
        knull[j] = ku[j] == KTA_PLANE_KEY_NONE;
        tomb[j] = vu[j] == KTA_COMPACT_LEN_NONE;
    }
    if (pt[0] == pt[1] && pt[0] == pt[2] && pt[0] == pt[3]) {
        const uint32_t slot = (pt[0] << rep_log2) | rep;
        const uint32_t tombs = tomb[0] + tomb[1] + tomb[2] + tomb[3];
        const uint32_t knulls = knull[0] + knull[1] + knull[2] + knull[3];
        plane_add(L, slot, plane_pack(4u, ku[0] + ku[1] + ku[2] + ku[3], vu[0] + vu[1] + vu[2] + vu[3], knulls, tombs));
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) plane_add(L, (pt[j] << rep_log2) | rep, plane_pack(1u, ku[j], vu[j], knull[j], tomb[j]));
}

// The workgroup of every packed scan kernel: its LDS words, carved out of the dynamic LDS and zeroed, its lane state,
// the front flush and the row.
struct PackedWg {
    PackedLds L;
    uint32_t P, rep_log2, rep, tid;
    LaneState st;

    __device__ __forceinline__ PackedWg(unsigned long long *lds, uint32_t P_, uint32_t rep_log2_) : P(P_), rep_log2(rep_log2_)
    {
        tid = threadIdx.x;
        const uint32_t slots = P << rep_log2;
        L = PackedLds{lds, lds + slots, lds + 2 * slots};
        for (uint32_t i = tid; i < 2 * slots + kScanCols * P; i += kWG) lds[i] = 0ull;
        __syncthreads();
        rep = tid & ((1u << rep_log2) - 1u);
    }
    // front level into back level: thread p sums and zeroes partition p's replicas, between two barriers
    // raw: the interval's records were plane records, added in the plane's words and with their markers
    // (lean_quad(PlaneSlot), kta_plane_pack.h): every replica is unpacked on its own — only a single slot's fields are
    // bounded — and the null keys' 0xFF and the tombstones' 0xFFFF leave the two size sums here, by the interval's own
    // counts.  One rule per interval: a workgroup that changes form flushes first (packed_scan_lean).
    __device__ __forceinline__ void front_flush(bool raw = false) const
    {
        __syncthreads();
        if (raw) {
            for (uint32_t p = tid; p < P; p += kWG) {
                PlaneSums sums;
                for (uint32_t r = 0; r < (1u << rep_log2); r++) {
                    const uint32_t s = (p << rep_log2) | r;
                    plane_unpack(sums, L.W1[s], L.W2[s]);
                    L.W1[s] = 0ull;
                    L.W2[s] = 0ull;
                }
                plane_corrected(sums);
                L.B[p] += sums.cnt;
                L.B[P + p] += sums.tb;
                L.B[2u * P + p] += sums.kn;
                L.B[3u * P + p] += sums.ks;
                L.B[4u * P + p] += sums.vs;
            }
            __syncthreads();
            return;
        }
        for (uint32_t p = tid; p < P; p += kWG) {
            unsigned long long w1 = 0, w2 = 0;   // (the replicas' sum obeys the same bound: it is the workgroup's records)
            for (uint32_t r = 0; r < (1u << rep_log2); r++) {
                const uint32_t s = (p << rep_log2) | r;
                w1 += L.W1[s];
                w2 += L.W2[s];
                L.W1[s] = 0ull;
                L.W2[s] = 0ull;
            }
            L.B[p] += w1 & 0xFFFFull;
            L.B[P + p] += (w1 >> 16) & 0xFFFFull;
            L.B[2u * P + p] += w2 & 0xFFFFFFFFull;
            L.B[3u * P + p] += w1 >> 32;
            L.B[4u * P + p] += w2 >> 32;
        }
        __syncthreads();
    }
    // the row, from the back level (behind the last front_flush).  MERGE: added to what another kernel's workgroup wrote.
    template <bool MERGE = false>
    __device__ __forceinline__ void write_row(uint64_t *row, long long (&s_red)[kWG / 64][6]) const
    {
        for (uint32_t p = tid; p < P; p += kWG)        // (thread p's own words of the back level)
#pragma unroll
            for (uint32_t j = 0; j < kScanCols; j++) {
                uint64_t &o = row[(uint64_t)p * kScanCols + j];
                if (MERGE) o += L.B[j * P + p];
                else o = L.B[j * P + p];
            }
        write_scan_globals<MERGE>(st, s_red, row, P, tid);
    }
};

// The lean kernel of a summary-reading scan (kta_metrics_scan_packed<NT, true>); kta_metrics_scan_packed_rest is launched
// behind it with the same grid.
// Its loop (lean_run) takes the summarised tiles of one form — plane tiles, or compact / u16 tiles (lean_tile) —
// through a ring of slots, unrolled.  The workgroup's steps are classified a block of 64 at a time: lane l of every
// wave loads header, summary, mark and size words of step 64 b + l (vector loads, requested a block ahead), applies
// lean_tile and votes; the two ballots, through lean_block, are the block's masks, and a lane whose bit stays folds its
// tile's extrema.  Every decision is then made from uniform values.  A tile that does not qualify is not accumulated here.  Its step — tile = workgroup + step x grid
// — goes on the row's list (kLeanListed steps at most, in three of the row's globals that no fold reads) and the ring
// goes on behind it; where the list is full the workgroup ends at that tile and hands it and all that follow over.
// The workgroup of the same index in kta_metrics_scan_packed_rest takes the listed tiles and the handed-over ones
// through the loop over whole Quads and adds them to the row; with an empty list it reads three words and ends.  So a
// cut first or last tile, or one raw tile in a thousand, leaves its workgroup in the lean loop, and a batch of which no
// tile qualifies runs in the loop it ran in before.
constexpr uint32_t kLeanListed = 4;
constexpr uint32_t kScanListA = 5, kScanHandover = 6, kScanListB = 7;   // (SG_NREC's word, unused by the scans, and the two behind it)
// entry i of the list (a step + 1, 0: none): four 32-bit halves of two row words, filled in ascending order
__device__ __forceinline__ uint32_t lean_list_entry(uint64_t list_a, uint64_t list_b, uint32_t i)
{
    return (uint32_t)((i < 2 ? list_a : list_b) >> (32u * (i & 1u)));
}

// A lane's side words of one tile: header, summary (as its two dwords: taking the u16 fields apart belongs to the use,
// not to the load), mark and the two size words.
struct LeanSide {
    kta_tile_hdr h;
    uint2 s;
    uint32_t m, z0, z1;
};
// Tile T's (vector loads: T differs by lane).  No load is left out where the batch has no marks — it reads a summary's
// bytes instead, and lean_tile is given a mark of 0: every path then has the same loads in flight.
__device__ __forceinline__ void lean_side_load(LeanSide &sd, const ScanColumns &c, uint64_t T)
{
    const uint32_t *mp = c.mark ? c.mark : reinterpret_cast<const uint32_t *>(c.sum);
    const uint32_t *zp = c.mark ? c.size : reinterpret_cast<const uint32_t *>(c.sum);
    sd.h = c.hdr[T];
    sd.s = reinterpret_cast<const uint2 *>(c.sum)[T];
    sd.m = mp[T];
    sd.z0 = zp[2u * T];
    sd.z1 = zp[2u * T + 1u];
}

// What a workgroup of the lean kernel carries from one run of the loop to the next: uniform but for `side`.
// Steps and tiles are counted in 32 bits: launch_metrics_scan keeps a batch of 2^31 tiles out.
struct LeanRun {
    LeanBlocks b;                       // the end of this kernel's steps, the list and the handover (kta_lean_blocks.h)
    uint32_t step = 0;                  // the next step to accumulate: tile = workgroup + step x grid
    uint32_t open_at = 0;               // the first step of the next block to open; the blocks below it are open
    uint64_t pm = 0, lm = 0;            // the open block's plane and lean masks, bit l = step open_at - 64 + l
    uint32_t whole_lo = 0, whole_hi = 0;   // tiles [whole_lo, whole_hi) lie wholly inside the batch
    uint32_t since_flush = 0;
    LeanSide side;                      // the lane's side words of step open_at + lane, requested a block ahead
};

// One run of the lean loop over tiles of one form (PLANE: plane tiles, else compact / u16 tiles), from r.step on, until
// this kernel's steps end or a summarised tile of the OTHER form comes up: r.step is then that tile's, the ring is
// dropped, and the caller goes on in the other instantiation.
// Between two block openings the loop holds no scalar load and no LDS read: a step is a bit of the block's mask and an
// address that advances by the grid's stride.  The ring's loads go out whatever the bit says (of a tile that is not
// taken they fetch bytes of the tile's own that nobody uses; past the workgroup's last tile the address stays where it
// is, so nothing past the batch's last tile is read): a slot is then waited for behind the same number of younger loads
// on every path, and the wait can let those stay in flight.
template <bool NT, bool PLANE>
__device__ __forceinline__ void lean_run(PackedWg &wg, LeanRun &r, const ScanColumns &c, uint64_t t0, uint32_t last, uint32_t pc,
                                         uint32_t rep_log2)
{
    using Slot = typename std::conditional<PLANE, PlaneSlot, LeanSlot>::type;
    constexpr uint64_t kUnit = PLANE ? 2u * kTileColBytes : kTileColBytes;   // a tile's bytes of the column the form reads
    const uint32_t tid = wg.tid, lane = tid & 63u;
    const uint32_t G = gridDim.x;
    const uint64_t stride = (uint64_t)G * kUnit;
    const uint32_t interval = PLANE ? plane_interval_tiles(rep_log2, kFrontFlushTiles) : kFrontFlushTiles;   // (uniform)
    uint32_t itile = 0;                       // the tile the next load reads, and its first byte in the form's column
    uint64_t ibyte = 0;
    auto seek = [&](uint32_t step) {
        const uint64_t tile = blockIdx.x + (uint64_t)step * G;
        itile = tile < last ? (uint32_t)tile : last;
        ibyte = (t0 + itile) * kUnit + (PLANE ? kTilePlaneOffset : 0u);
    };
    auto issue = [&](Slot &s) {
        lean_load<NT>(s, c, ibyte, 8u * tid, 16u * tid);
        const uint32_t next = itile + G;      // (both below 2^31)
        const bool adv = next <= last;
        itile = adv ? next : itile;
        ibyte += adv ? stride : 0ull;
    };
    auto take = [&](const Slot &s, bool v) {
        if (v) {
            lean_quad(s, rep_log2, wg.rep, wg.L, wg.st);
            if (++r.since_flush == interval) {
                wg.front_flush(PLANE);
                r.since_flush = 0;
            }
        }
    };
    // the lane's side words of step base + lane (the tile index clamped, not the load skipped)
    auto side_request = [&](uint32_t base) {
        const uint64_t tile = blockIdx.x + (uint64_t)(base + lane) * G;
        lean_side_load(r.side, c, t0 + (tile < last ? tile : last));
    };
    // Open the block at r.open_at (= r.step): classify its 64 steps from the side words, one per lane, apply the block
    // rule (lean_block), fold the extrema of the tiles that stay in a mask — min and max are idempotent, so every wave
    // folds — and request the side words of the block behind it, whose latency 64 steps hide.
    auto open_block = [&]() {
        const uint32_t base = r.open_at;
        const uint64_t tile = blockIdx.x + (uint64_t)(base + lane) * G;
        const kta_tile_sum sm{r.side.s.x, (uint16_t)(r.side.s.y & 0xFFFFu), (uint16_t)(r.side.s.y >> 16)};
        bool lean, plane;
        lean_tile(r.side.h, sm, c.mark ? r.side.m : 0u, tile >= r.whole_lo && tile < r.whole_hi, pc, lean, plane);
        r.pm = __ballot(plane);
        r.lm = __ballot(lean);
        lean_block(r.b, base, kLeanListed, r.pm, r.lm);
        const bool tp = (r.pm >> lane) & 1ull, tl = (r.lm >> lane) & 1ull;
        long long lo, hi;
        tile_sum_extrema(r.side.h, sm, lo, hi);
        wg.st.tmin = ((tp || tl) && lo < wg.st.tmin) ? lo : wg.st.tmin;
        wg.st.tmax = ((tp || tl) && hi > wg.st.tmax) ? hi : wg.st.tmax;
        wg.st.smin = min(wg.st.smin, tp ? r.side.z0 : 0xFFFFFFFFu);   // (c.size is there wherever c.mark is)
        wg.st.smax = max(wg.st.smax, tp ? r.side.z1 : 0u);
        r.open_at = base + kLeanBlockSteps;
        side_request(r.open_at);
    };
    // The steps of this run in the open block from r.step on — up to the first of the other form, the block's end or
    // r.b.end — and their bits of this form's mask, bit 0 = r.step.
    auto span = [&](uint64_t &mine) {
        const uint32_t pos = r.step - (r.open_at - kLeanBlockSteps);
        const uint64_t a = (PLANE ? r.pm : r.lm) >> pos, o = (PLANE ? r.lm : r.pm) >> pos;
        uint32_t cnt = o ? (uint32_t)__builtin_ctzll(o) : kLeanBlockSteps - pos;
        cnt = min(cnt, r.b.end - r.step);
        mine = cnt < kLeanBlockSteps ? a & ((1ull << cnt) - 1ull) : a;
        return cnt;
    };
    // the ring, unrolled over four steps whatever its depth (no rotation moves; a block is 16 such bodies): the slots
    // a, b, c hold the kLeanPrefetch tiles in flight
    Slot a, b, cc, d;
    auto body = [&](uint64_t &m) {
        if (kLeanPrefetch == 3) {
            issue(d), take(a, (uint32_t)m & 1u);
            issue(a), take(b, (uint32_t)m & 2u);
            issue(b), take(cc, (uint32_t)m & 4u);
            issue(cc), take(d, (uint32_t)m & 8u);
        } else if (kLeanPrefetch == 2) {
            issue(cc), take(a, (uint32_t)m & 1u);
            issue(d), take(b, (uint32_t)m & 2u);
            issue(a), take(cc, (uint32_t)m & 4u);
            issue(b), take(d, (uint32_t)m & 8u);
        } else {
            issue(b), take(a, (uint32_t)m & 1u);
            issue(a), take(b, (uint32_t)m & 2u);
            issue(b), take(a, (uint32_t)m & 4u);
            issue(a), take(b, (uint32_t)m & 8u);
        }
        m >>= 4;
    };
    if (r.step != r.open_at) {
        // The run begins inside an open block (behind a run of the other form): single steps up to a multiple of four.
        uint64_t mine;
        uint32_t cnt = span(mine);
        const bool ends = cnt < r.open_at - r.step;
        while ((r.step & 3u) && cnt) {
            Slot x;
            seek(r.step);
            issue(x);
            take(x, mine & 1u);
            mine >>= 1;
            r.step++, cnt--;
        }
        if (!cnt && ends) return;
    }
    seek(r.step);
    issue(a);
    if (kLeanPrefetch >= 2) issue(b);
    if (kLeanPrefetch == 3) issue(cc);
    while (r.step < r.b.end) {
        uint64_t mine;
        uint32_t cnt, nb;
        const bool opens = r.step == r.open_at;
        if (opens) {
            // (the first body of a block has the next block's side loads behind the ring's: a copy of its own, whose
            // waits count them; every later body waits as if there were none)
            open_block();
            cnt = span(mine);
            if (!cnt) break;
            nb = (cnt + 3u) / 4u - 1u;
            body(mine);
        } else {
            cnt = span(mine);
            if (!cnt) break;
            nb = (cnt + 3u) / 4u;
        }
        for (; nb; nb--) body(mine);
        // (the last body may have stepped past the run's steps: their bits are 0, and the slots hold no tile)
        r.step += cnt;
        if (r.step != r.open_at) break;
    }
}

template <bool NT>
__device__ __forceinline__ void packed_scan_lean(const ScanColumns &c, uint64_t n, uint32_t P, uint32_t rep_log2,
                                                 uint64_t *__restrict__ partials, uint32_t row_len, unsigned long long *lds,
                                                 long long (&s_red)[kWG / 64][6])
{
    PackedWg wg(lds, P, rep_log2);
    const uint32_t tid = wg.tid;
    // allocation tiles [t0, t0 + ntiles) hold the batch; record a of the allocation is the batch's iff a - rec0 < n
    const uint64_t t0 = c.rec0 / KTA_TILE_RECORDS;
    const uint64_t ntiles = (c.rec0 + n + KTA_TILE_RECORDS - 1) / KTA_TILE_RECORDS - t0;
    const uint32_t pc = min(P, (uint32_t)KTA_COMPACT_PART_NONE);
    LeanRun r;
    r.b.end = lean_steps(blockIdx.x, gridDim.x, ntiles);
    r.whole_lo = c.rec0 % KTA_TILE_RECORDS ? 1u : 0u;
    r.whole_hi = (uint32_t)((c.rec0 + n) / KTA_TILE_RECORDS - t0);
    const uint32_t last = (uint32_t)ntiles - 1u;
    // Runs of the two forms in turn (r.b.end > 0: there is a tile to clamp to).  A run that begins at a tile of the
    // other form ends at once, and the other one takes that tile, so every turn but the first takes a tile.  With marks
    // the plane form goes first: the flagship's tiles are all marked.
    bool plane = c.mark != nullptr;
    if (r.b.end) {
        // the first block's side words, before any run
        const uint64_t tile = blockIdx.x + (uint64_t)(tid & 63u) * gridDim.x;
        lean_side_load(r.side, c, t0 + (tile < last ? tile : last));
    }
    while (r.step < r.b.end) {
        if (plane) lean_run<NT, true>(wg, r, c, t0, last, pc, rep_log2);
        else lean_run<NT, false>(wg, r, c, t0, last, pc, rep_log2);
        // A front interval holds records of one form, so that front_flush has one rule for it: the run's last interval
        // is flushed before a run of the other form adds to the same slots (and the last run's before the row is read).
        if (r.since_flush) {
            wg.front_flush(plane);
            r.since_flush = 0;
        }
        plane = !plane;
    }
    // (every run flushed its last interval, and thread p reads from the back level the words it wrote there itself)
    uint64_t *row = partials + (uint64_t)blockIdx.x * row_len;
    wg.write_row(row, s_red);
    if (tid == 0) {   // (behind the zeroes write_scan_globals put there)
        uint64_t *g = row + (uint64_t)P * kScanCols;
        g[kScanListA] = r.b.list_a;
        g[kScanHandover] = r.b.handover;
        g[kScanListB] = r.b.list_b;
    }
}

// SUM = true: the lean kernel.  SUM = false: the packed scan's loop over whole Quads, for a batch without summaries and
// for scan_variant bit 32.
template <bool NT, bool SUM>
__global__ __launch_bounds__(kWG) void kta_metrics_scan_packed(ScanColumns c, uint64_t n, uint32_t P, uint32_t rep_log2,
                                                               uint64_t *__restrict__ partials, uint32_t row_len)
{
    extern __shared__ unsigned long long lds[];
    __shared__ long long s_red[kWG / 64][6];

    if constexpr (SUM) {
        packed_scan_lean<NT>(c, n, P, rep_log2, partials, row_len, lds, s_red);
        return;
    }
    PackedWg wg(lds, P, rep_log2);
    const uint32_t tid = wg.tid;
    // allocation tiles [t0, t0 + ntiles) hold the batch; record a of the allocation is the batch's iff a - rec0 < n
    const uint64_t t0 = c.rec0 / KTA_TILE_RECORDS;
    const uint64_t ntiles = (c.rec0 + n + KTA_TILE_RECORDS - 1) / KTA_TILE_RECORDS - t0;
    // the prefetch ring of kta_metrics_scan
    uint32_t since_flush = 0;
    uint64_t tile = blockIdx.x;
    const uint32_t pc = min(P, (uint32_t)KTA_COMPACT_PART_NONE);
    Quad cur, nxt, nx2;
    if (tile < ntiles) load_tile_quad<NT, SUM>(cur, c, t0 + tile, tid, n, pc);
    if (kPackedPrefetch == 2 && tile + gridDim.x < ntiles) load_tile_quad<NT, SUM>(nxt, c, t0 + tile + gridDim.x, tid, n, pc);
    while (tile < ntiles) { // uniform per workgroup
        const uint64_t ntile = tile + gridDim.x;
        const uint64_t ahead = tile + (uint64_t)kPackedPrefetch * gridDim.x;
        if (ahead < ntiles) load_tile_quad<NT, SUM>(kPackedPrefetch == 2 ? nx2 : nxt, c, t0 + ahead, tid, n, pc);

        const uint64_t a = (t0 + tile) * KTA_TILE_RECORDS + 4u * tid - c.rec0;   // (wraps below rec0)
        const uint32_t valid = quad_valid(a, n);
        accumulate_packed<SUM>(cur, valid, P, rep_log2, wg.rep, wg.L, wg.st);

        if (++since_flush == kFrontFlushTiles) {
            wg.front_flush();
            since_flush = 0;
        }
        cur = nxt;
        if (kPackedPrefetch == 2) nxt = nx2;
        tile = ntile;
    }
    wg.front_flush();
    wg.write_row(partials + (uint64_t)blockIdx.x * row_len, s_red);
}
// The lean kernel, specialised for its register budget alone (the body is the template's SUM branch): left to itself
// the compiler spends some 100 vector registers on it — the loop needs about 60 — and five workgroups of a CU, the
// plan's, would not be resident together.  kLeanWavesPerSimd waves per SIMD: 96 registers.
#ifndef KTA_LEAN_WAVES
#define KTA_LEAN_WAVES 5
#endif
constexpr int kLeanWavesPerSimd = KTA_LEAN_WAVES;
#define KTA_LEAN_KERNEL(NT)                                                                                                    \
    template <>                                                                                                                \
    __global__ __launch_bounds__(kWG, kLeanWavesPerSimd) void kta_metrics_scan_packed<NT, true>(                               \
        ScanColumns c, uint64_t n, uint32_t P, uint32_t rep_log2, uint64_t *__restrict__ partials, uint32_t row_len)           \
    {                                                                                                                          \
        extern __shared__ unsigned long long lds[];                                                                            \
        __shared__ long long s_red[kWG / 64][6];                                                                               \
        packed_scan_lean<NT>(c, n, P, rep_log2, partials, row_len, lds, s_red);                                                \
    }
KTA_LEAN_KERNEL(true)
KTA_LEAN_KERNEL(false)
#undef KTA_LEAN_KERNEL

// The tiles the lean kernel's workgroup of the same index left (see there): the listed ones, then every tile from the
// handed-over step on, through the loop over Quads with one tile loaded ahead; added to the row.
// The tiles are read WITHOUT their summaries, as kta_metrics_scan_packed<NT, false> reads them — right for every tile,
// 4 B per record more for a summarised one among the handed-over, and the faster loop where nothing is summarised (the
// summary-reading loop over Quads was 5 % slower there): the listed tiles never are, and the handed-over ones rarely.
template <bool NT>
__global__ __launch_bounds__(kWG) void kta_metrics_scan_packed_rest(ScanColumns c, uint64_t n, uint32_t P, uint32_t rep_log2,
                                                                    uint64_t *__restrict__ partials, uint32_t row_len)
{
    extern __shared__ unsigned long long lds[];
    __shared__ long long s_red[kWG / 64][6];

    uint64_t *row = partials + (uint64_t)blockIdx.x * row_len;
    uint64_t *g = row + (uint64_t)P * kScanCols;
    const uint64_t list_a = g[kScanListA], list_b = g[kScanListB], handover = g[kScanHandover];   // uniform
    if ((list_a | list_b | handover) == 0) return;   // (write_scan_globals zeroes the three words, behind barriers)

    PackedWg wg(lds, P, rep_log2);
    const uint32_t tid = wg.tid;
    const uint64_t t0 = c.rec0 / KTA_TILE_RECORDS;
    const uint64_t ntiles = (c.rec0 + n + KTA_TILE_RECORDS - 1) / KTA_TILE_RECORDS - t0;
    const uint32_t pc = min(P, (uint32_t)KTA_COMPACT_PART_NONE);
    uint32_t since_flush = 0;
    Quad cur, nxt;
    // Listed steps that end right before the handed-over one are taken with it (a batch of which no tile qualifies lists
    // its first four tiles and hands over the fifth: the ring then starts at the first).
    uint64_t first = handover;   // the step the ring starts at, + 1
    uint32_t nlist = 0;
    for (uint32_t li = 0; li < kLeanListed; li++) nlist += lean_list_entry(list_a, list_b, li) != 0u;
    while (first > 1 && nlist > 0 && lean_list_entry(list_a, list_b, nlist - 1u) == (uint32_t)(first - 1)) {
        first--;
        nlist--;
    }
    // the other listed tiles, one at a time (four at most, in ascending order)
    for (uint32_t li = 0; li < nlist; li++) {
        const uint64_t tile = blockIdx.x + (uint64_t)(lean_list_entry(list_a, list_b, li) - 1u) * gridDim.x;
        load_tile_quad<NT, false>(cur, c, t0 + tile, tid, n, pc);
        const uint64_t a = (t0 + tile) * KTA_TILE_RECORDS + 4u * tid - c.rec0;   // (wraps below rec0)
        const uint32_t valid = quad_valid(a, n);
        accumulate_packed<false>(cur, valid, P, rep_log2, wg.rep, wg.L, wg.st);   // (four tiles: no front flush is due)
        since_flush++;
    }
    // the handed-over tiles, through the ring of Quads: kta_metrics_scan_packed<NT, false>'s loop
    uint64_t tile = first ? blockIdx.x + (first - 1) * gridDim.x : ntiles;
    if (tile < ntiles) load_tile_quad<NT, false>(cur, c, t0 + tile, tid, n, pc);
    while (tile < ntiles) { // uniform per workgroup
        const uint64_t ntile = tile + gridDim.x;
        if (ntile < ntiles) load_tile_quad<NT, false>(nxt, c, t0 + ntile, tid, n, pc);

        const uint64_t a = (t0 + tile) * KTA_TILE_RECORDS + 4u * tid - c.rec0;   // (wraps below rec0)
        const uint32_t valid = quad_valid(a, n);
        accumulate_packed<false>(cur, valid, P, rep_log2, wg.rep, wg.L, wg.st);

        if (++since_flush == kFrontFlushTiles) {
            wg.front_flush();
            since_flush = 0;
        }
        cur = nxt;
        tile = ntile;
    }
    wg.front_flush();
    wg.write_row<true>(row, s_red);   // (added to the lean kernel's)
}

// ---------------------------------------------------------------------------------------
// K5  fold partial rows into the persistent counter vector
// ---------------------------------------------------------------------------------------
// The body is kta_fold.h's.  grid = (column blocks, row groups of kta_fold_groups.h); each thread folds one column of its
// group's rows.
__global__ __launch_bounds__(kWG) void kta_fold_partials(const uint64_t *__restrict__ partials,
                                                         uint32_t rows, uint32_t P,
                                                         uint64_t *__restrict__ vec, uint32_t row_len,
                                                         uint64_t *__restrict__ avec)
{
    const uint32_t col = blockIdx.x * kWG + threadIdx.x;
    if (col >= row_len) return;
    uint32_t r0, r1;
    fold_group_rows(blockIdx.y, rows, r0, r1);   // (launch_fold_partials: gridDim.y = fold_groups(rows))
    fold_rows(partials, r0, r1, P, vec, row_len, avec, col);
}

// launch_tiles_to_raw: one workgroup per tile, grid-strided over the allocation tiles that overlap [lo, hi).  what bit 0:
// compact partitions / timestamps become raw; bit 1: u16 lengths become i32.  A tile wholly inside the range only changes
// its header unless `keep` (the producer that follows overwrites all of its records; a key-reading pass that follows
// needs them: keep); one the range cuts is expanded in place — every lane reads its 4 records before any lane writes, the
// compact halves and the u16 groups overlap the raw positions of the tile's first records.
__global__ __launch_bounds__(kWG) void kta_tiles_to_raw(int32_t *__restrict__ partition, int64_t *__restrict__ ts_ms,
                                                        int32_t *__restrict__ key_len, int32_t *__restrict__ val_len,
                                                        kta_tile_hdr *__restrict__ hdr, uint64_t lo, uint64_t hi,
                                                        uint32_t what, uint32_t keep)
{
    const uint64_t t0 = lo / KTA_TILE_RECORDS, t1 = (hi + KTA_TILE_RECORDS - 1) / KTA_TILE_RECORDS;
    const uint32_t tid = threadIdx.x;
    for (uint64_t T = t0 + blockIdx.x; T < t1; T += gridDim.x) {
        const kta_tile_hdr h = hdr[T];
        const bool dm = (what & 1u) && h.mode == KTA_TILE_COMPACT, dl = (what & 2u) && h.lens == KTA_TILE_LENS_U16;
        if (!dm && !dl) continue;   // (uniform)
        const uint64_t first = T * KTA_TILE_RECORDS;
        if (keep || first < lo || first + KTA_TILE_RECORDS > hi) {
            int32_t p[4];
            long long t[4];
            int4 g = make_int4(0, 0, 0, 0);
            if (dm) {
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) tile_record_h<false>(partition, ts_ms, h, T, first + 4u * tid + j, p[j], t[j]);
            }
            if (dl) g = reinterpret_cast<const int4 *>(key_len)[first / 4 + tid];
            __syncthreads();
            if (dm) {
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) {
                    partition[first + 4u * tid + j] = p[j];
                    ts_ms[first + 4u * tid + j] = t[j];
                }
            }
            if (dl) {
                reinterpret_cast<int4 *>(key_len)[first / 4 + tid] = widen_lens4(g.x, g.y);
                reinterpret_cast<int4 *>(val_len)[first / 4 + tid] = widen_lens4(g.z, g.w);
            }
        }
        __syncthreads();
        if (tid == 0) {
            if (dm) {
                hdr[T].ts_base = 0;
                hdr[T].mode = KTA_TILE_RAW;
            }
            if (dl) hdr[T].lens = KTA_TILE_LENS_I32;
        }
        __syncthreads();
    }
}

__global__ void kta_init_vector(uint64_t *vec, uint32_t P, uint64_t *avec)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nc = P * 7;
    if (i < nc) vec[i] = 0;
    if (avec) {
        if (i < 2 * kHistBuckets) avec[i] = 0;
        if (i < 4 * P) avec[2 * kHistBuckets + i] = (uint64_t)LLONG_MIN;
    }
    if (i == 0) {
        uint64_t *g = vec + nc;
        g[0] = 0; g[1] = 0; g[2] = 0; g[3] = 0;  // SUM globals
        g[4] = (uint64_t)~LLONG_MAX;             // ~min ts: nothing seen
        g[5] = (uint64_t)LLONG_MIN;              // max ts
        g[6] = (uint64_t)~LLONG_MAX;             // ~smallest: u64::MAX in the reference (metric.rs:42)
        g[7] = 0;                                // largest (metric.rs:41)
    }
}

// ---------------------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------------------

ScanPlan plan_scan(uint32_t P, uint64_t n, int cu_count, int req_workgroups, int req_variant, bool analytics, bool tiled,
                   uint32_t timeline_buckets)
{
    ScanPlan pl;
    // req_variant: low bits 0 = accumulate, 9 = loads only (diagnostic); +16 = non-temporal loads; +32 = no tile summaries;
    // +64 = ignore the plane marks (a summarised tile is read in its u16 form)
    const int base = req_variant & 15;
    pl.summaries = (req_variant & 32) == 0;
    pl.planes = (req_variant & 64) == 0;
    const bool timeline = timeline_buckets != 0u;
    pl.analytics = analytics;
    pl.nontemporal = (analytics || timeline) ? true : (req_variant & 16) != 0;
    pl.variant = (analytics || timeline) ? 0u : (base == 9 ? 9u : 0u);
    pl.timeline_rows = timeline ? timeline_buckets + 3u : 0u;
    // the packed scan (kta_metrics_scan_packed): accumulating, tile-compact, no additive outputs — as long as its 56 B
    // per partition (unreplicated) fit a workgroup's LDS; the few P beyond that keep kta_metrics_scan's 24 B
    pl.packed = tiled && !analytics && !timeline && pl.variant == 0u &&
                P * (16u + kScanCols * 8u) + 256u <= 160u * 1024u;
    const uint32_t arrays = pl.packed ? 2u : 3u + (analytics ? 4u : 0u);
    const uint32_t hist_bytes = analytics ? 2u * kHistBuckets * kHistReps * 4u : 0u;
    // LDS budget per workgroup: 32 KiB (4 workgroups = 16 waves per CU can be resident); the
    // analytics kernel carries 7 arrays and gets 64 KiB (2 workgroups per CU) to keep the replication.
    // Tile-compact analytics: 48 KiB, so that 3 workgroups per CU are resident (2^30 records of config 4: 4.89 ms with
    // 64 KiB and 2 per CU, 3.33 with 48 KiB, 3.34 with 40, 3.62 with 32 KiB and 5 per CU).
    // The timeline's rows (16 B each, 16.05 KiB at 1024 buckets) come out of the same budget: the replication backs
    // off, the workgroups per CU stay.
    const uint32_t budget_kib = analytics ? (tiled ? 48u : 64u) : 32u;
    const uint32_t tl_bytes = pl.timeline_rows * 16u;
    // (packed: two front arrays, replicated, and the back level's five words per partition: 16 P R + 40 P bytes)
    const uint32_t fixed = hist_bytes + tl_bytes + (pl.packed ? P * kScanCols * 8u : 0u);
    const uint32_t budget_slots = budget_kib * 1024u > fixed ? (budget_kib * 1024u - fixed) / (8u * arrays) : 0u;
    uint32_t rep_log2 = 0;
    while (rep_log2 < 6 && (P << (rep_log2 + 1)) <= budget_slots) rep_log2++;
    pl.rep_log2 = rep_log2;
    pl.lds_bytes = (P << rep_log2) * 8u * arrays + fixed;
    pl.row_len = scan_row_len(P, analytics);
    const uint64_t ntiles = ((n >> 2) + kWG - 1) / kWG;
    // Raw layout: 3 workgroups (12 waves) per CU saturate HBM (measured: 2-3 per CU best, more is slower), and
    // every workgroup is resident at once, so the static round-robin tile deal stays balanced.
    // (a workgroup needing more than 40 KiB of LDS only fits twice per CU: use 2 per CU then)
    // Tile-compact layout: a lane has 56 B of a tile in flight instead of 80, and 3 per CU leave HBM short of
    // requests (2^30 records of config 4: 2.85 ms at 3 per CU, 2.44 at 4, 2.32 at 5, 2.66 at 6, 2.96 at 7) — 5 per
    // CU, as far as the LDS of 160 KiB per CU lets them all be resident.  The plane form (4 B per record, 16 B per lane
    // in flight) was swept again and keeps both (profiles/plane_scan.jsonl).
    uint32_t per_cu = pl.lds_bytes > 40u * 1024u ? 2u : 3u;
    if (tiled) {
        const uint32_t fit = (160u * 1024u) / (pl.lds_bytes + 256u);
        per_cu = fit < 5u ? (fit > 0u ? fit : 1u) : 5u;
    }
    uint64_t wgs = req_workgroups > 0 ? (uint64_t)req_workgroups : (uint64_t)cu_count * per_cu;
    if (wgs > ntiles) wgs = ntiles;
    if (wgs < 1) wgs = 1;
    pl.workgroups = (uint32_t)wgs;
    return pl;
}

// One scan kernel on the plan's grid.  More than 48 KiB of dynamic LDS must be opted into, per kernel.
template <typename... Extra>
static hipError_t launch_scan_kernel(void (*kernel)(ScanColumns, uint64_t, uint32_t, uint32_t, uint64_t *, uint32_t, Extra...),
                                     const ScanPlan &pl, const ScanColumns &c, uint64_t n, uint32_t P, uint64_t *partials,
                                     hipStream_t s, const Extra &...extra)
{
    if (pl.lds_bytes > 48u * 1024u) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)pl.lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3(pl.workgroups), dim3(kWG), pl.lds_bytes, s, c, n, P, pl.rep_log2, partials, pl.row_len,
                       extra...);
    return hipGetLastError();
}

hipError_t launch_metrics_scan(const ScanPlan &pl, const ScanColumns &c, uint64_t n, uint32_t P,
                               uint64_t *partials, hipStream_t s, const TimelineArgs *tl)
{
    if (pl.timeline_rows && (!tl || tl->n_buckets + 3u != pl.timeline_rows)) return hipErrorInvalidValue;
    const bool tiled = c.hdr != nullptr, nt = pl.nontemporal;
    const auto launch = [&](auto kernel, const ScanColumns &cols, const auto &...extra) {
        return launch_scan_kernel(kernel, pl, cols, n, P, partials, s, extra...);
    };
    if (pl.timeline_rows) {   // (plan_scan: accumulating, non-temporal)
        if (pl.analytics)
            return tiled ? launch(kta_metrics_scan<0, true, true, true, TimelineArgs>, c, *tl)
                         : launch(kta_metrics_scan<0, true, true, false, TimelineArgs>, c, *tl);
        return tiled ? launch(kta_metrics_scan<0, true, false, true, TimelineArgs>, c, *tl)
                     : launch(kta_metrics_scan<0, true, false, false, TimelineArgs>, c, *tl);
    }
    if (pl.analytics) return tiled ? launch(kta_metrics_scan<0, true, true, true>, c) : launch(kta_metrics_scan<0, true, true, false>, c);
    if (pl.packed) {
        if (!tiled) return hipErrorInvalidValue;
        ScanColumns cs = c;
        if (!pl.summaries) cs.sum = nullptr;
        if (!pl.planes || !cs.sum) cs.mark = nullptr;
        if (!cs.mark) cs.size = nullptr;
        // (the lean kernel counts the batch's tiles, and a few grids ahead of them, in 32 bits)
        if ((c.rec0 % KTA_TILE_RECORDS + n) / KTA_TILE_RECORDS >= (1ull << 31)) cs.sum = nullptr, cs.mark = nullptr, cs.size = nullptr;
        if (!cs.sum) return nt ? launch(kta_metrics_scan_packed<true, false>, cs) : launch(kta_metrics_scan_packed<false, false>, cs);
        // the lean kernel, then — same grid, same rows — the tiles its workgroups left (none, where every tile is
        // summarised, compact and u16: a workgroup of the second kernel then reads one word and ends)
        const hipError_t el = nt ? launch(kta_metrics_scan_packed<true, true>, cs) : launch(kta_metrics_scan_packed<false, true>, cs);
        if (el != hipSuccess) return el;
        return nt ? launch(kta_metrics_scan_packed_rest<true>, cs) : launch(kta_metrics_scan_packed_rest<false>, cs);
    }
    if (pl.variant == 9) {
        if (nt) return tiled ? launch(kta_metrics_scan<9, true, false, true>, c) : launch(kta_metrics_scan<9, true, false, false>, c);
        return tiled ? launch(kta_metrics_scan<9, false, false, true>, c) : launch(kta_metrics_scan<9, false, false, false>, c);
    }
    if (nt) return tiled ? launch(kta_metrics_scan<0, true, false, true>, c) : launch(kta_metrics_scan<0, true, false, false>, c);
    return tiled ? launch(kta_metrics_scan<0, false, false, true>, c) : launch(kta_metrics_scan<0, false, false, false>, c);
}

hipError_t launch_fold_partials(const uint64_t *partials, uint32_t rows, uint32_t P, uint64_t *vec,
                                uint32_t row_len, uint64_t *avec, hipStream_t s)
{
    dim3 grid((row_len + kWG - 1) / kWG, fold_groups(rows)), block(kWG);   // (the kernel takes the rows of group blockIdx.y)
    hipLaunchKernelGGL(kta_fold_partials, grid, block, 0, s, partials, rows, P, vec, row_len, avec);
    return hipGetLastError();
}

hipError_t launch_tiles_to_raw(int32_t *partition, int64_t *ts_ms, int32_t *key_len, int32_t *val_len, kta_tile_hdr *hdr,
                               uint64_t lo, uint64_t hi, uint32_t what, bool keep, hipStream_t s)
{
    if (lo >= hi) return hipSuccess;
    const uint64_t tiles = (hi + KTA_TILE_RECORDS - 1) / KTA_TILE_RECORDS - lo / KTA_TILE_RECORDS;
    const uint32_t grid = (uint32_t)(tiles < 8192 ? tiles : 8192);
    hipLaunchKernelGGL(kta_tiles_to_raw, dim3(grid), dim3(kWG), 0, s, partition, ts_ms, key_len, val_len, hdr, lo, hi, what,
                       keep ? 1u : 0u);
    return hipGetLastError();
}

hipError_t launch_init_vector(uint64_t *vec, uint32_t P, uint64_t *avec, hipStream_t s)
{
    const uint32_t n = P * 7 + 1;
    hipLaunchKernelGGL(kta_init_vector, dim3((n + 255) / 256), dim3(256), 0, s, vec, P, avec);
    return hipGetLastError();
}

} // namespace kta

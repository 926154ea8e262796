// kta_tile.h — the tile-compact layout of device batches (include/kta_hip.h states the format; this is its code), once:
// which values fit the compact forms, how a value is packed and widened, where record i's u16 / i32 sits in a tile's
// bytes, the whole-tile host pack and unpack, and the device readers of a record's partition and timestamp.  Everything
// but the device readers compiles as plain C++ (tests/native/tile_codec.cpp) as well as under hipcc, host and device:
// no HIP runtime call, no LDS.  The sentinels of the compact forms are named in this file only.
#pragma once

#include <stdint.h>
#include <string.h>

#include "kta_hip.h"

#ifdef __HIPCC__
#define KTA_TILE_HD __host__ __device__
#else
#define KTA_TILE_HD
#endif

namespace kta {

// ---- which values fit ---------------------------------------------------------------------------------------------
KTA_TILE_HD inline bool tile_part_fits(int32_t p) { return p >= -1 && p < (int32_t)KTA_COMPACT_PART_NONE; }
KTA_TILE_HD inline bool tile_len_fits(int32_t l) { return l >= -1 && l < (int32_t)KTA_COMPACT_LEN_NONE; }
// lo / hi: the least and the largest of a tile's timestamps other than -1 (lo > hi: it has none, and its base is 0).
// Compact when they span less than 2^31 ms; *base is then what the offsets count from.
KTA_TILE_HD inline bool tile_ts_fits(int64_t lo, int64_t hi, int64_t *base)
{
    *base = lo <= hi ? lo : 0;
    return lo > hi || (uint64_t)hi - (uint64_t)lo <= (uint64_t)INT32_MAX;
}

// ---- a tile's summary (kta_tile_sum, kta_hip.h) -------------------------------------------------------------------
// The one rule of validity: a summary is trusted only next to a KTA_TILE_COMPACT header; whoever writes a COMPACT header
// writes that tile's summary in the same step; and the summary is VALID only if that step wrote all KTA_TILE_RECORDS
// records of the tile — the partial last tile of a fill gets a zero summary ("none").  A header that turns RAW
// (kta_tiles_to_raw) needs nothing more, and widening the lengths leaves partitions and timestamps, so the summary, as
// they are.
// The one address rule: the summaries of an allocation of ntiles tiles lie behind its ntiles headers, in the same device
// allocation (alloc_device_batch), entry t next to header t.
KTA_TILE_HD inline kta_tile_sum *tile_sums_behind(kta_tile_hdr *hdr, uint64_t ntiles)
{
    return reinterpret_cast<kta_tile_sum *>(hdr + ntiles);
}
static_assert(sizeof(kta_tile_sum) == 8 && sizeof(kta_tile_hdr) == 16, "a summary is one 8-byte word behind 16-byte headers");
// The summary of a compact tile of m records: lo / hi as tile_ts_fits takes them, part_max the largest STORED u16 partition
// (tile_pack_part) and untimed (a timestamp of -1) over the m records.
KTA_TILE_HD inline kta_tile_sum tile_summary(int64_t lo, int64_t hi, uint32_t part_max, bool untimed, uint64_t m)
{
    kta_tile_sum s{0, 0, 0};
    if (m != KTA_TILE_RECORDS) return s;
    const bool timed = lo <= hi;
    s.ts_span = timed ? (uint32_t)((uint64_t)hi - (uint64_t)lo) : 0u;
    s.part_max = (uint16_t)part_max;
    s.flags = (uint16_t)(KTA_TILE_SUM_VALID | (timed ? KTA_TILE_SUM_TIMED : 0u) | (untimed ? KTA_TILE_SUM_UNTIMED : 0u));
    return s;
}

// ---- a tile's scan plane (kta_hip.h) ------------------------------------------------------------------------------
// A compact tile uses the first half of its 8 KiB of the ts_ms column; the plane is the second half: one dword per
// record — partition | key << 8 | val << 16 — all that the metrics scan needs of a record whose timestamps the summary
// covers, in one stream.  It repeats what the u16 / i32 forms hold; every other reader keeps reading those.
// Which records fit: a partition in [0, 256) (no sentinel: a tile with an id of -1 has no plane), a key length in
// [-1, 255) (0xFF is -1), a value length under tile_len_fits' rule (0xFFFF is -1).
// The mark: a tile has a plane exactly when its mark is 1.  The rule of validity is the summaries' with one more
// sentence: a mark is trusted only next to a KTA_TILE_COMPACT header and a VALID summary; whoever writes a tile's
// summary writes its mark, 0 or 1, in the same step, and the plane before it.  The mark is 1 only for a compact tile of
// all KTA_TILE_RECORDS records of which every one fits.  A header that turns RAW needs nothing more; widening the
// lengths touches neither the ts_ms bytes nor the values.  The plane does not depend on `lens`: keyed allocations have
// planes too.
// The address rule: the marks, a u32 per tile, lie behind the summaries in the same device allocation.
constexpr uint32_t KTA_PLANE_PARTS = 256u, KTA_PLANE_KEY_NONE = 0xFFu;
constexpr uint32_t kTilePlaneOffset = KTA_TILE_RECORDS * 4u;   // the plane's first byte among the tile's bytes of ts_ms
KTA_TILE_HD inline uint32_t *tile_marks_behind(kta_tile_hdr *hdr, uint64_t ntiles)
{
    return reinterpret_cast<uint32_t *>(tile_sums_behind(hdr, ntiles) + ntiles);
}
// The size extrema: two u32 per tile, size_min and size_max — the least and the largest key_len + val_len over the
// tile's records that have a value (val_len != -1; a key of -1 counts as 0), 0xFFFFFFFF / 0 where it has none: what the
// metrics scan would otherwise find record by record.  The rule of validity: the two words are trusted only where the
// tile's mark is 1 (so only where the mark itself is trusted); whoever writes a mark of 1 writes the tile's two words in
// the same step, before the mark.  A mark that is cleared, a header that turns RAW and widened lengths need nothing more.
// The address rule: the words lie behind the marks in the same device allocation, tile t's at [2 t] and [2 t + 1].
constexpr uint32_t kTileSizeMinNone = 0xFFFFFFFFu, kTileSizeMaxNone = 0u;
KTA_TILE_HD inline uint32_t *tile_sizes_behind(kta_tile_hdr *hdr, uint64_t ntiles)
{
    return tile_marks_behind(hdr, ntiles) + ntiles;
}
constexpr uint64_t kTileSideBytes = sizeof(kta_tile_hdr) + sizeof(kta_tile_sum) + sizeof(uint32_t) + 2 * sizeof(uint32_t);   // header, summary, mark, size extrema
// a record's share of its tile's size extrema (of a record that fits the plane): folded with min into lo, with max into hi
KTA_TILE_HD inline void tile_size_fold(int32_t k, int32_t v, uint32_t &lo, uint32_t &hi)
{
    if (v == -1) return;
    const uint32_t sz = (uint32_t)(k == -1 ? 0 : k) + (uint32_t)v;
    lo = sz < lo ? sz : lo;
    hi = sz > hi ? sz : hi;
}
KTA_TILE_HD inline bool tile_plane_fits(int32_t p, int32_t k, int32_t v)
{
    return p >= 0 && p < (int32_t)KTA_PLANE_PARTS && k >= -1 && k < (int32_t)KTA_PLANE_KEY_NONE && tile_len_fits(v);
}
// (of a record that fits: -1 is all ones, so the masks make the sentinels)
KTA_TILE_HD inline uint32_t tile_plane_pack(int32_t p, int32_t k, int32_t v)
{
    return (uint32_t)p | (((uint32_t)k & 0xFFu) << 8) | ((uint32_t)v << 16);
}
KTA_TILE_HD inline int32_t tile_plane_part(uint32_t w) { return (int32_t)(w & 0xFFu); }
KTA_TILE_HD inline int32_t tile_plane_key(uint32_t w) { return ((w >> 8) & 0xFFu) == KTA_PLANE_KEY_NONE ? -1 : (int32_t)((w >> 8) & 0xFFu); }
KTA_TILE_HD inline int32_t tile_plane_val(uint32_t w) { return (w >> 16) == KTA_COMPACT_LEN_NONE ? -1 : (int32_t)(w >> 16); }
// byte of the tile's own bytes of the ts_ms column where the word of record j of the tile sits
KTA_TILE_HD inline uint32_t tile_plane_at(uint32_t j) { return kTilePlaneOffset + 4u * j; }

// ---- one value ----------------------------------------------------------------------------------------------------
KTA_TILE_HD inline uint16_t tile_pack_part(int32_t p) { return p == -1 ? (uint16_t)KTA_COMPACT_PART_NONE : (uint16_t)p; }
KTA_TILE_HD inline int32_t tile_unpack_part(uint32_t u) { return u == KTA_COMPACT_PART_NONE ? -1 : (int32_t)u; }
// (modular: base + offset is exact for every pair the fit rule admits, INT64_MIN + 1 .. INT64_MAX included)
KTA_TILE_HD inline int32_t tile_pack_ts(int64_t t, int64_t base)
{
    return t == -1 ? KTA_COMPACT_TS_NONE : (int32_t)((uint64_t)t - (uint64_t)base);
}
KTA_TILE_HD inline int64_t tile_unpack_ts(int32_t o, int64_t base)
{
    return o == KTA_COMPACT_TS_NONE ? -1 : (int64_t)((uint64_t)base + (uint64_t)(int64_t)o);
}
KTA_TILE_HD inline uint16_t tile_pack_len(int32_t l) { return (uint16_t)l; }   // (-1 -> KTA_COMPACT_LEN_NONE)
KTA_TILE_HD inline int32_t tile_unpack_len(uint32_t u) { return u == KTA_COMPACT_LEN_NONE ? -1 : (int32_t)u; }

// ---- where a value sits -------------------------------------------------------------------------------------------
// Compact partition / timestamp offset of record i (an allocation index) of allocation tile `tile`: element
// i + tile * KTA_TILE_RECORDS of the column seen as u16 / i32 — the first half of the tile's own bytes.
KTA_TILE_HD inline uint64_t tile_compact_at(uint64_t i, uint64_t tile) { return i + tile * KTA_TILE_RECORDS; }
// u16 lengths: the tile's bytes of the key_len column are 256 groups of {4 key lengths, 4 value lengths}; the u16 slot
// of record j of the tile (0 .. 1023) among the tile's 2048
KTA_TILE_HD inline uint32_t tile_klen_slot(uint32_t j) { return (j / 4u) * 8u + j % 4u; }
KTA_TILE_HD inline uint32_t tile_vlen_slot(uint32_t j) { return tile_klen_slot(j) + 4u; }
// The word-level forms of a lane's four consecutive records: four u16 are two dwords (the partitions; a group's key
// lengths are its dwords 0 and 1, its value lengths 2 and 3), four i32 offsets two 8-byte words.
KTA_TILE_HD inline void tile_u16x4(uint32_t w0, uint32_t w1, uint32_t (&u)[4])
{
    u[0] = w0 & 0xFFFFu, u[1] = w0 >> 16, u[2] = w1 & 0xFFFFu, u[3] = w1 >> 16;
}
KTA_TILE_HD inline uint32_t tile_u16x2_word(uint16_t a, uint16_t b) { return (uint32_t)a | ((uint32_t)b << 16); }
KTA_TILE_HD inline void tile_i32x4(long long w0, long long w1, int32_t (&o)[4])
{
    o[0] = (int32_t)(uint32_t)w0, o[1] = (int32_t)(uint32_t)((uint64_t)w0 >> 32);
    o[2] = (int32_t)(uint32_t)w1, o[3] = (int32_t)(uint32_t)((uint64_t)w1 >> 32);
}

// ---- a whole tile on the host (kta_batch_from_raw / kta_batch_to_raw) ---------------------------------------------
// Records [0, m), m <= KTA_TILE_RECORDS, of raw columns p / t / k / v into one tile's images — part, ts, klen, vlen: the
// tile's own KTA_TILE_RECORDS elements of each column, what is not written keeps its value — and the tile's header.
// lens16: the allocation has no key columns, so the lengths may take the u16 form.  klen == null: the lengths are not
// the caller's business (a keyed allocation takes them with a plain copy), k / v are not read and lens stays 0.
// sum (may be null): the tile's summary — zero unless the tile is compact and m is the whole tile.
inline kta_tile_hdr tile_pack_host(const int32_t *p, const int64_t *t, const int32_t *k, const int32_t *v, uint64_t m, bool lens16,
                                   int32_t *part, int64_t *ts, int32_t *klen, int32_t *vlen, kta_tile_sum *sum = nullptr)
{
    kta_tile_hdr h{0, KTA_TILE_RAW, KTA_TILE_LENS_I32};
    int64_t lo = INT64_MAX, hi = INT64_MIN, base = 0;
    bool fits = true, untimed = false;
    uint32_t part_max = 0;
    if (sum) *sum = kta_tile_sum{0, 0, 0};
    for (uint64_t j = 0; j < m; j++) {
        fits = fits && tile_part_fits(p[j]);
        untimed = untimed || t[j] == -1;
        if (t[j] == -1) continue;
        lo = t[j] < lo ? t[j] : lo;
        hi = t[j] > hi ? t[j] : hi;
    }
    if (tile_ts_fits(lo, hi, &base) && fits) {
        uint16_t *p16 = reinterpret_cast<uint16_t *>(part);
        int32_t *o32 = reinterpret_cast<int32_t *>(ts);
        for (uint64_t j = 0; j < m; j++) {
            p16[tile_compact_at(j, 0)] = tile_pack_part(p[j]);
            o32[tile_compact_at(j, 0)] = tile_pack_ts(t[j], base);
            part_max = tile_pack_part(p[j]) > part_max ? tile_pack_part(p[j]) : part_max;
        }
        h.ts_base = base;
        h.mode = KTA_TILE_COMPACT;
        if (sum) *sum = tile_summary(lo, hi, part_max, untimed, m);
    } else {
        memcpy(part, p, m * 4);
        memcpy(ts, t, m * 8);
    }
    if (!klen) return h;
    bool u16 = lens16;
    for (uint64_t j = 0; j < m && u16; j++) u16 = tile_len_fits(k[j]) && tile_len_fits(v[j]);
    if (u16) {
        uint16_t *g16 = reinterpret_cast<uint16_t *>(klen);
        for (uint64_t j = 0; j < m; j++) {
            g16[tile_klen_slot((uint32_t)j)] = tile_pack_len(k[j]);
            g16[tile_vlen_slot((uint32_t)j)] = tile_pack_len(v[j]);
        }
        h.lens = KTA_TILE_LENS_U16;
    } else {
        memcpy(klen, k, m * 4);
        memcpy(vlen, v, m * 4);
    }
    return h;
}

// The reverse: records [j0, j1) of the tile whose images and header these are, as raw values in p / t / k / v [0, j1 - j0).
// klen == null: partition and timestamp only (vlen is not read for a u16 tile either: its bytes are unused).
inline void tile_unpack_host(const kta_tile_hdr &h, const int32_t *part, const int64_t *ts, const int32_t *klen, const int32_t *vlen,
                             uint64_t j0, uint64_t j1, int32_t *p, int64_t *t, int32_t *k, int32_t *v)
{
    const uint16_t *p16 = reinterpret_cast<const uint16_t *>(part), *g16 = reinterpret_cast<const uint16_t *>(klen);
    const int32_t *o32 = reinterpret_cast<const int32_t *>(ts);
    for (uint64_t j = j0; j < j1; j++) {
        const bool compact = h.mode == KTA_TILE_COMPACT;
        p[j - j0] = compact ? tile_unpack_part(p16[tile_compact_at(j, 0)]) : part[j];
        t[j - j0] = compact ? tile_unpack_ts(o32[tile_compact_at(j, 0)], h.ts_base) : ts[j];
        if (!klen) continue;
        const bool u16 = h.lens == KTA_TILE_LENS_U16;
        k[j - j0] = u16 ? tile_unpack_len(g16[tile_klen_slot((uint32_t)j)]) : klen[j];
        v[j - j0] = u16 ? tile_unpack_len(g16[tile_vlen_slot((uint32_t)j)]) : vlen[j];
    }
}

// The plane of the tile that tile_pack_host packed from the same records with header h: the mark, and — iff it is 1 —
// the plane's words in bytes [kTilePlaneOffset, 2 kTilePlaneOffset) of the tile's ts image and (sizes, may be null) the
// tile's two size extrema; nothing else is written.
inline uint32_t tile_plane_host(const kta_tile_hdr &h, const int32_t *p, const int32_t *k, const int32_t *v, uint64_t m, int64_t *ts,
                                uint32_t *sizes = nullptr)
{
    if (h.mode != KTA_TILE_COMPACT || m != KTA_TILE_RECORDS) return 0u;
    for (uint64_t j = 0; j < m; j++)
        if (!tile_plane_fits(p[j], k[j], v[j])) return 0u;
    unsigned char *plane = reinterpret_cast<unsigned char *>(ts);
    uint32_t lo = kTileSizeMinNone, hi = kTileSizeMaxNone;
    for (uint64_t j = 0; j < m; j++) {
        const uint32_t w = tile_plane_pack(p[j], k[j], v[j]);
        memcpy(plane + tile_plane_at((uint32_t)j), &w, 4);
        tile_size_fold(k[j], v[j], lo, hi);
    }
    if (sizes) sizes[0] = lo, sizes[1] = hi;
    return 1u;
}

#ifdef __HIPCC__
// ---- device readers -----------------------------------------------------------------------------------------------
// Partition id and (TS) raw timestamp of record i (an allocation index) of a tile-compact batch.
// (tile_record_h: the header h of allocation tile `tile` is already loaded.  A record of another tile reads in-bounds
// garbage — for records the caller masks.)
template <bool NT, bool TS = true>
__device__ __forceinline__ void tile_record_h(const int32_t *part, const int64_t *ts, const kta_tile_hdr &h, uint64_t tile,
                                              uint64_t i, int32_t &p, long long &t)
{
    if (h.mode == KTA_TILE_COMPACT) {
        const uint64_t ci = tile_compact_at(i, tile);
        const uint16_t *p16 = reinterpret_cast<const uint16_t *>(part) + ci;
        p = tile_unpack_part(NT ? __builtin_nontemporal_load(p16) : *p16);
        if (TS) {
            const int32_t *t32 = reinterpret_cast<const int32_t *>(ts) + ci;
            t = tile_unpack_ts(NT ? __builtin_nontemporal_load(t32) : *t32, h.ts_base);
        }
    } else {
        p = NT ? __builtin_nontemporal_load(part + i) : part[i];
        if (TS) t = NT ? __builtin_nontemporal_load(ts + i) : ts[i];
    }
}

template <bool NT, bool TS = true>
__device__ __forceinline__ void tile_record(const int32_t *part, const int64_t *ts, const kta_tile_hdr *hdr, uint64_t i,
                                            int32_t &p, long long &t)
{
    const uint64_t tile = i / KTA_TILE_RECORDS;
    tile_record_h<NT, TS>(part, ts, hdr[tile], tile, i, p, t);
}

// A wave step — `len` consecutive records from allocation index a0 on — usually lies in one layout tile: the header of
// the step's first tile is loaded once for the step (step_tile; on: the step has records at all).  step_tile_record reads
// a record's partition and timestamp through it where the step lies in that one tile (a step that straddles two looks
// every record's header up), step_tile_part a record's partition alone (its mode is the cached one where the record
// lies in the first tile).
struct StepTile {
    kta_tile_hdr h;
    uint64_t tile;
    bool one;
};
__device__ __forceinline__ StepTile step_tile(const kta_tile_hdr *hdr, uint64_t a0, uint32_t len, bool on)
{
    StepTile s{};
    s.tile = a0 / KTA_TILE_RECORDS;
    if (hdr && on) {
        s.one = (a0 + len - 1) / KTA_TILE_RECORDS == s.tile;
        s.h = hdr[s.tile];
    }
    return s;
}
template <bool NT, bool TS = true>
__device__ __forceinline__ void step_tile_record(const StepTile &s, const int32_t *part, const int64_t *ts, const kta_tile_hdr *hdr,
                                                 uint64_t i, int32_t &p, long long &t)
{
    if (s.one) tile_record_h<NT, TS>(part, ts, s.h, i / KTA_TILE_RECORDS, i, p, t);
    else tile_record<NT, TS>(part, ts, hdr, i, p, t);
}
template <bool NT>
__device__ __forceinline__ int32_t step_tile_part(const StepTile &s, const int32_t *part, const kta_tile_hdr *hdr, uint64_t i)
{
    const uint64_t tile = i / KTA_TILE_RECORDS;
    const kta_tile_hdr h{0, tile == s.tile ? s.h.mode : hdr[tile].mode, KTA_TILE_LENS_I32};
    int32_t p;
    long long no_ts;
    tile_record_h<NT, false>(part, nullptr, h, tile, i, p, no_ts);
    return p;
}
#endif

} // namespace kta

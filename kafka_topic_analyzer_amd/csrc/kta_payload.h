// kta_payload.h — the payload section (KTA_FLAG_PAYLOAD, include/kta_hip.h): the one statement of what a record of a Kafka
// v2 batch adds to the section's vector — its value's class, its schema-registry id, its headers —, the layout of that
// vector, the identities between its words and the read-off of the schema ids.  Shared by the kernel (kta_payload.hip), the
// host functions that read, merge and restate the vector (kta_api.hip), the renderer (host/report.cpp) and the stand-alone
// check (tests/native/payload_check.cpp): plain C++, no HIP header.  No reference counterpart.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define KTA_PL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define KTA_PL_HD inline
#endif

namespace kta {

// ---- the vector: u64[24 P + 16 + 2 * 1024 * 34], every word a SUM ------------------------------------------------------
//   [24 p, 24 p + 24)                          partition p's words (PayloadWord)
//   [24 P, 24 P + 16)                          headers per record over the topic: bins 0 .. 14 and >= 15 (records with
//                                              bad headers are in no bin)
//   [24 P + 16 + (1024 r + c) 34, .. + 34)     cell c of row r of the schema-id table: T records, B value bytes, 32 bit counters
enum PayloadWord : uint32_t {
    kPlRecords = 0,
    kPlClass = 1,            // five counts: null, empty, framed, json, other (PayloadClass)
    kPlClassBytes = 6,       // five value-byte sums, the same order (null and empty: 0)
    kPlWithHeaders = 11, kPlHeaders, kPlHeaderKeyBytes, kPlHeaderValueBytes, kPlHeaderNullValues, kPlBadHeaders, kPlHeaderWireBytes,
    kPlPartitionSums = 18,   // words 18..23 are zero
    kPlPartitionWords = 24
};
enum PayloadClass : uint32_t { kPlNull = 0, kPlEmpty, kPlFramed, kPlJson, kPlOther, kPlClasses = 5 };
constexpr uint32_t kPlHistBins = 16;
constexpr uint32_t kPlRows = 2;
constexpr uint32_t kPlCells = 1024;
constexpr uint32_t kPlCellT = 0, kPlCellB = 1, kPlCellBits = 2, kPlCellWords = 34;
constexpr uint32_t kPlTableWords = kPlRows * kPlCells * kPlCellWords;   // 69 632
constexpr uint32_t kPlVarintMax = 10;                                    // bytes of the longest varint

KTA_PL_HD size_t payload_hist_at(uint32_t P) { return (size_t)kPlPartitionWords * P; }
KTA_PL_HD size_t payload_table_at(uint32_t P) { return payload_hist_at(P) + kPlHistBins; }
KTA_PL_HD size_t payload_len(uint32_t P) { return payload_table_at(P) + kPlTableWords; }

// murmur3's finaliser (kta_fnv.h's fmix32, which is device code): a bijection of u32
KTA_PL_HD uint32_t payload_fmix32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}
// The cell of id x in row r: row 0 by the id's low bits (ids that span fewer than 1024 consecutive values never share
// one), row 1 by its hash.
KTA_PL_HD uint32_t payload_cell(uint32_t row, uint32_t id) { return (row == 0 ? id : payload_fmix32(id)) & (kPlCells - 1u); }
KTA_PL_HD size_t payload_cell_at(uint32_t P, uint32_t row, uint32_t cell)
{
    return payload_table_at(P) + ((size_t)row * kPlCells + cell) * kPlCellWords;
}

// ---- THE RULE, part 1: the class of a value -----------------------------------------------------------------------------
// val_len: -1 null.  b0: the value's first byte (read only when val_len >= 1).  Only bytes of the record decide.
KTA_PL_HD uint32_t payload_class(long long val_len, uint32_t b0)
{
    if (val_len < 0) return kPlNull;
    if (val_len == 0) return kPlEmpty;
    if (val_len >= 5 && b0 == 0x00u) return kPlFramed;    // Confluent wire format: magic 0, then the schema id
    if (b0 == (uint32_t)'{' || b0 == (uint32_t)'[') return kPlJson;
    return kPlOther;
}
// The schema id of a framed value: bytes 1..4, big endian.
KTA_PL_HD uint32_t payload_schema_id(uint32_t b1, uint32_t b2, uint32_t b3, uint32_t b4) { return (b1 << 24) | (b2 << 16) | (b3 << 8) | b4; }

// ---- THE RULE, part 2: the headers of a record --------------------------------------------------------------------------
// headersCount varint | count x (keyLen varint | key | valueLen varint (-1: null) | value), from `pos` to the record's end
// `end` (from its length prefix).  Src::at(p) is the byte at position p; the walk reads no byte at or behind `end`.
// BAD: a negative count, a negative key length, a value length below -1, a varint that runs on past ten bytes, a field that
// overruns the record, a walk that does not end exactly at `end` — and so a section that is absent (pos == end).
struct PayloadHeaders {
    bool bad;
    uint64_t count, key_bytes, value_bytes, null_values;
};

template <class Src>
KTA_PL_HD bool payload_varlong(Src &src, uint64_t &pos, uint64_t end, long long &out)
{
    unsigned long long v = 0;
    for (uint32_t i = 0; i < kPlVarintMax; i++) {
        if (pos >= end) return false;
        const uint32_t b = src.at(pos++);
        const uint32_t shift = 7u * i;
        v |= (unsigned long long)(b & 0x7Fu) << (shift < 64u ? shift : 63u);
        if (!(b & 0x80u)) {
            out = (long long)(v >> 1) ^ -(long long)(v & 1ull);
            return true;
        }
    }
    return false;
}

template <class Src>
KTA_PL_HD PayloadHeaders payload_walk_headers(Src &src, uint64_t pos, uint64_t end)
{
    PayloadHeaders h;
    h.bad = true, h.count = 0, h.key_bytes = 0, h.value_bytes = 0, h.null_values = 0;
    long long count;
    if (!payload_varlong(src, pos, end, count) || count < 0) return h;
    uint64_t keyb = 0, valb = 0, nulls = 0;
    for (long long i = 0; i < count; i++) {                       // every header takes two bytes at least: the loop ends
        long long kl, vl;
        if (!payload_varlong(src, pos, end, kl) || kl < 0 || (uint64_t)kl > end - pos) return h;
        pos += (uint64_t)kl, keyb += (uint64_t)kl;
        if (!payload_varlong(src, pos, end, vl) || vl < -1) return h;
        if (vl < 0) { nulls++; continue; }
        if ((uint64_t)vl > end - pos) return h;
        pos += (uint64_t)vl, valb += (uint64_t)vl;
    }
    if (pos != end) return h;
    h.bad = false, h.count = (uint64_t)count, h.key_bytes = keyb, h.value_bytes = valb, h.null_values = nulls;
    return h;
}

// The same walk, VISITING: visit(name position, name length, value length or -1 for a null value) for every header, in the
// section's order.  For a section that payload_walk_headers found good (the header-name section, kta_header_names.h: validate,
// then visit); on any other it returns false where the walk above returns bad, having visited the headers in front of that place.
template <class Src, class Visit>
KTA_PL_HD bool payload_visit_headers(Src &src, uint64_t pos, uint64_t end, Visit &&visit)
{
    long long count;
    if (!payload_varlong(src, pos, end, count) || count < 0) return false;
    for (long long i = 0; i < count; i++) {
        long long kl, vl;
        if (!payload_varlong(src, pos, end, kl) || kl < 0 || (uint64_t)kl > end - pos) return false;
        const uint64_t name = pos;
        pos += (uint64_t)kl;
        if (!payload_varlong(src, pos, end, vl) || vl < -1 || (vl > 0 && (uint64_t)vl > end - pos)) return false;
        visit(name, (uint64_t)kl, vl);
        pos += vl > 0 ? (uint64_t)vl : 0;
    }
    return pos == end;
}

KTA_PL_HD uint32_t payload_hist_bin(uint64_t headers) { return headers < kPlHistBins - 1u ? (uint32_t)headers : kPlHistBins - 1u; }

// ---- what one record adds (host form; the kernel adds the same words from registers) ------------------------------------
// A counted record: its batch's descriptor has status 0 after the decode, its framing (length prefix .. value) is good and
// so is that of every record in front of it in the batch, its partition lies in [0, P) and it passes the context's filter.
// wire: the bytes from the headersCount varint to the record's end.  A record with bad headers adds 1 to kPlBadHeaders and
// nothing to any other header word or to the histogram; its value counts all the same.
struct PayloadBytes {            // a byte source over memory
    const uint8_t *p;
    uint32_t at(uint64_t i) const { return p[i]; }
};

inline void payload_add(uint64_t *vec, uint32_t P, uint32_t partition, long long val_len, const uint8_t *value, const PayloadHeaders &h,
                        uint64_t wire)
{
    uint64_t *w = vec + (size_t)kPlPartitionWords * partition;
    const uint32_t cls = payload_class(val_len, val_len >= 1 ? value[0] : 0u);
    const uint64_t vb = val_len > 0 ? (uint64_t)val_len : 0;
    w[kPlRecords]++, w[kPlClass + cls]++, w[kPlClassBytes + cls] += vb;
    if (cls == kPlFramed) {
        const uint32_t id = payload_schema_id(value[1], value[2], value[3], value[4]);
        for (uint32_t r = 0; r < kPlRows; r++) {
            uint64_t *c = vec + payload_cell_at(P, r, payload_cell(r, id));
            c[kPlCellT]++, c[kPlCellB] += vb;
            for (uint32_t b = 0; b < 32; b++) c[kPlCellBits + b] += (id >> b) & 1u;
        }
    }
    if (h.bad) {
        w[kPlBadHeaders]++;
        return;
    }
    w[kPlWithHeaders] += h.count != 0, w[kPlHeaders] += h.count, w[kPlHeaderKeyBytes] += h.key_bytes, w[kPlHeaderValueBytes] += h.value_bytes;
    w[kPlHeaderNullValues] += h.null_values, w[kPlHeaderWireBytes] += wire;
    vec[payload_hist_at(P) + payload_hist_bin(h.count)]++;
}

// The records of one batch's payload [pos, end) of `bytes` (uncompressed, or inflated), n_records of them, as the decode
// walks them: length varint | attributes | timestampDelta | offsetDelta | keyLength | key | valueLength | value | headers.
// The walk stops at the first record whose framing fails; the records in front of it count.  passes(ts_delta): the filter.
// record(val_len, value position, position behind the value, the record's end) for every record that counts.
template <class Passes, class OnRecord>
inline void payload_records_host(const uint8_t *bytes, uint64_t pos, uint64_t end, uint64_t n_records, Passes passes, OnRecord record)
{
    PayloadBytes src{bytes};
    for (uint64_t r = 0; r < n_records; r++) {
        long long len, ts_delta, offset_delta, key_len, val_len;
        if (!payload_varlong(src, pos, end, len) || len < 0 || (uint64_t)len > end - pos) return;
        const uint64_t rec_end = pos + (uint64_t)len;
        if (pos >= rec_end) return;
        pos++;                                                   // the attributes byte
        if (!payload_varlong(src, pos, rec_end, ts_delta) || !payload_varlong(src, pos, rec_end, offset_delta) ||
            !payload_varlong(src, pos, rec_end, key_len))
            return;
        if (key_len < -1 || (key_len > 0 && (uint64_t)key_len > rec_end - pos)) return;
        pos += key_len > 0 ? (uint64_t)key_len : 0;
        if (pos >= rec_end || !payload_varlong(src, pos, rec_end, val_len)) return;
        if (val_len < -1 || (val_len > 0 && (uint64_t)val_len > rec_end - pos)) return;
        const uint64_t value = pos, after = pos + (val_len > 0 ? (uint64_t)val_len : 0);
        if (passes(ts_delta)) record(val_len, value, after, rec_end);
        pos = rec_end;
    }
}

template <class Passes>
inline void payload_batch_host(uint64_t *vec, uint32_t P, uint32_t partition, const uint8_t *bytes, uint64_t pos, uint64_t end, uint64_t n_records,
                               Passes passes)
{
    PayloadBytes src{bytes};
    payload_records_host(bytes, pos, end, n_records, passes, [&](long long val_len, uint64_t value, uint64_t after, uint64_t rec_end) {
        payload_add(vec, P, partition, val_len, bytes + value, payload_walk_headers(src, after, rec_end), rec_end - after);
    });
}

// ---- the identities between the words of one vector --------------------------------------------------------------------
// counters: NULL, or the counter vector (kta_hip.h: [P][KTA_N_COUNTERS]-prefix, total at word 0 and tombstones at word 1 of
// a partition's `stride` words) of the same unfiltered run without failed batches: records == total_messages (which
// includes the tombstones) and null == tombstones, per partition.
inline bool payload_identities_hold(const uint64_t *vec, uint32_t P, const uint64_t *counters = nullptr, size_t stride = 0)
{
    uint64_t records = 0, with = 0, bad = 0, framed = 0, framed_bytes = 0;
    for (uint32_t p = 0; p < P; p++) {
        const uint64_t *w = vec + (size_t)kPlPartitionWords * p;
        uint64_t classes = 0;
        for (uint32_t c = 0; c < kPlClasses; c++) classes += w[kPlClass + c];
        if (classes != w[kPlRecords] || w[kPlClassBytes + kPlNull] || w[kPlClassBytes + kPlEmpty]) return false;
        for (uint32_t k = kPlPartitionSums; k < kPlPartitionWords; k++)
            if (w[k]) return false;
        records += w[kPlRecords], with += w[kPlWithHeaders], bad += w[kPlBadHeaders];
        framed += w[kPlClass + kPlFramed], framed_bytes += w[kPlClassBytes + kPlFramed];
        if (counters && (w[kPlRecords] != counters[stride * p] || w[kPlClass + kPlNull] != counters[stride * p + 1])) return false;
    }
    const uint64_t *hist = vec + payload_hist_at(P);
    uint64_t in_hist = 0;
    for (uint32_t b = 0; b < kPlHistBins; b++) in_hist += hist[b];
    if (in_hist != records - bad || hist[0] != records - with - bad) return false;
    for (uint32_t r = 0; r < kPlRows; r++) {
        uint64_t t = 0, b = 0;
        for (uint32_t c = 0; c < kPlCells; c++) {
            const uint64_t *cell = vec + payload_cell_at(P, r, c);
            t += cell[kPlCellT], b += cell[kPlCellB];
            for (uint32_t k = 0; k < 32; k++)
                if (cell[kPlCellBits + k] > cell[kPlCellT]) return false;
        }
        if (t != framed || b != framed_bytes) return false;
    }
    return true;
}

// ---- the read-off of the schema ids -------------------------------------------------------------------------------------
// The table is an invertible Bloom lookup table of two rows.  A cell is PURE when T > 0, every bit counter is 0 or T, and the
// id so spelled maps to this cell in this row: it then holds that id alone (two ids in a cell differ in a bit, whose counter
// lies strictly between 0 and T) and gives its records and bytes exactly.  A recovered id is peeled — its T, B and bit
// counts subtracted from its cell in the other row — and the rows are looked at again until nothing changes.  What then
// remains in row 0 is "records in cells that hold several ids": reported, never guessed at.
struct PayloadSchemaId {
    uint32_t id;
    uint64_t records, bytes;
};

// (bits: the cell's 32 bit counters; the words in front of them are sums that a key adds to, word 0 its T)
inline bool payload_cell_pure(const uint64_t *cell, uint32_t row, uint32_t index, uint32_t &id, uint32_t bits = kPlCellBits)
{
    const uint64_t t = cell[kPlCellT];
    if (t == 0) return false;
    id = 0;
    for (uint32_t k = 0; k < 32; k++) {
        const uint64_t c = cell[bits + k];
        if (c != 0 && c != t) return false;
        if (c) id |= 1u << k;
    }
    return payload_cell(row, id) == index;
}

// The peel of a two-row table t[kPlRows][kPlCells][CW] (T, CW - 33 further sums, 32 bit counters) in place: found(id, cell) for
// every recovered id, with the cell that spelled it, before the id is subtracted from both rows.  also_pure(cell): what a
// table asks of a pure cell beyond the above.  What remains in the rows is what could not be told apart.
template <uint32_t CW, class AlsoPure, class Found>
inline void payload_peel(uint64_t *t, AlsoPure also_pure, Found found)
{
    auto cell_of = [&](uint32_t row, uint32_t c) { return t + ((size_t)row * kPlCells + c) * CW; };
    for (bool changed = true; changed;) {
        changed = false;
        for (uint32_t row = 0; row < kPlRows; row++)
            for (uint32_t c = 0; c < kPlCells; c++) {
                uint64_t *cell = cell_of(row, c);
                uint32_t id;
                if (!payload_cell_pure(cell, row, c, id, CW - 32u) || !also_pure(cell)) continue;
                uint64_t *other = cell_of(1u - row, payload_cell(1u - row, id));
                bool fits = true;                                               // (always, in a vector the rule wrote)
                for (uint32_t k = 0; k < CW && fits; k++) fits = other[k] >= cell[k];
                if (!fits) continue;
                found(id, (const uint64_t *)cell);
                for (uint32_t k = 0; k < CW; k++) other[k] -= cell[k], cell[k] = 0;
                changed = true;
            }
    }
}

// Sorted by records (most first), then bytes, then id.
inline std::vector<PayloadSchemaId> payload_schema_ids(const uint64_t *vec, uint32_t P, uint64_t *unresolved_records, uint64_t *unresolved_bytes)
{
    std::vector<uint64_t> t(vec + payload_table_at(P), vec + payload_table_at(P) + kPlTableWords);
    std::vector<PayloadSchemaId> out;
    payload_peel<kPlCellWords>(t.data(), [](const uint64_t *) { return true; },
                               [&](uint32_t id, const uint64_t *cell) { out.push_back(PayloadSchemaId{id, cell[kPlCellT], cell[kPlCellB]}); });
    uint64_t ur = 0, ub = 0;
    for (uint32_t c = 0; c < kPlCells; c++) ur += t[(size_t)c * kPlCellWords + kPlCellT], ub += t[(size_t)c * kPlCellWords + kPlCellB];
    if (unresolved_records) *unresolved_records = ur;
    if (unresolved_bytes) *unresolved_bytes = ub;
    std::sort(out.begin(), out.end(), [](const PayloadSchemaId &a, const PayloadSchemaId &b) {
        return a.records != b.records ? a.records > b.records : a.bytes != b.bytes ? a.bytes > b.bytes : a.id < b.id;
    });
    return out;
}

} // namespace kta

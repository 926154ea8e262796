// kta_header_names.h — the header-name section (KTA_FLAG_HEADER_NAMES, include/kta_hip.h): the one statement of what a header
// occurrence of a record of a Kafka v2 batch adds to the section's vector and to its name table, the layout of both, the
// identities between the vector's words and the read-off of the names.  Which records count, the header grammar and what a
// BAD section is are kta_payload.h's (payload_records_host, payload_walk_headers, payload_visit_headers); so are the cell
// mapping (payload_cell) and the peel (payload_peel).  Shared by the kernel (kta_header_names.hip), the host functions
// (kta_api.hip), the renderer (host/report.cpp) and the stand-alone check (tests/native/header_names_check.cpp): plain C++, no
// HIP header.  No reference counterpart.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "kta_payload.h"

namespace kta {

// ---- the vector: u64[8 + 2 * 1024 * 36], independent of P, every word a SUM ---------------------------------------------
//   [0, 8)                              the globals (HnGlobal); words 6 and 7 are zero
//   [8 + (1024 r + c) 36, .. + 36)      cell c of row r: T occurrences, L name bytes, V value bytes, Z null values, 32 bit counters
enum HnGlobal : uint32_t { kHnOccurrences = 0, kHnNameBytes, kHnValueBytes, kHnNullValues, kHnWithHeaders, kHnLooked, kHnGlobalSums = 6, kHnGlobals = 8 };
constexpr uint32_t kHnCellT = 0, kHnCellL = 1, kHnCellV = 2, kHnCellZ = 3, kHnCellBits = 4, kHnCellWords = 36;
constexpr uint32_t kHnTableWords = kPlRows * kPlCells * kHnCellWords;   // 73 728
constexpr uint32_t kHnWords = kHnGlobals + kHnTableWords;                // 73 736
constexpr uint32_t kHnSlots = kPlRows * kPlCells;                        // the name table's slots: one per cell
constexpr uint32_t kHnExemplarBytes = 48;
enum HnSlotState : uint32_t { kHnEmpty = 0, kHnClaimed = 1, kHnPublished = 2 };

// A slot of the name table (kta_hip.h's kta_header_name): slot 1024 r + c belongs to cell c of row r.  Published, it holds
// the first min(name_len, 48) bytes of ONE occurrence's name whose hash is `hash` and maps to that cell in that row.
struct HnSlot {
    uint32_t hash, name_len, state, reserved;
    uint8_t bytes[kHnExemplarBytes];
};
static_assert(sizeof(HnSlot) == 64, "a slot is 64 bytes");

KTA_PL_HD size_t hn_cell_at(uint32_t row, uint32_t cell) { return kHnGlobals + ((size_t)row * kPlCells + cell) * kHnCellWords; }

// The name's hash: the reference's FNV-32 variant over the name's bytes (kta_fnv.h holds the device's fast forms of the same
// chain for keys; kta_header_names.hip asserts that the constants agree).  An empty name hashes to the offset basis.
constexpr uint32_t kHnFnvInit = 0x811c9dc5u, kHnFnvMul = 0x811c9dc5u;
KTA_PL_HD uint32_t hn_fnv_byte(uint32_t h, uint32_t b) { return (h ^ b) * kHnFnvMul; }

// ---- THE RULE: what one header occurrence adds (host form; the kernel adds the same words through its cache) -------------
inline void hn_add_occurrence(uint64_t *vec, HnSlot *table, const uint8_t *name, uint64_t name_len, long long val_len)
{
    uint32_t h = kHnFnvInit;
    for (uint64_t i = 0; i < name_len; i++) h = hn_fnv_byte(h, name[i]);
    const uint64_t vb = val_len > 0 ? (uint64_t)val_len : 0, z = val_len < 0 ? 1u : 0u;
    vec[kHnOccurrences]++, vec[kHnNameBytes] += name_len, vec[kHnValueBytes] += vb, vec[kHnNullValues] += z;
    for (uint32_t r = 0; r < kPlRows; r++) {
        const uint32_t cell = payload_cell(r, h);
        uint64_t *c = vec + hn_cell_at(r, cell);
        c[kHnCellT]++, c[kHnCellL] += name_len, c[kHnCellV] += vb, c[kHnCellZ] += z;
        for (uint32_t b = 0; b < 32; b++) c[kHnCellBits + b] += (h >> b) & 1u;
        if (table && table[r * kPlCells + cell].state == kHnEmpty) {          // the first writer wins
            HnSlot &s = table[r * kPlCells + cell];
            s.hash = h, s.name_len = name_len < 0xFFFFFFFFull ? (uint32_t)name_len : 0xFFFFFFFFu, s.reserved = 0;
            memset(s.bytes, 0, sizeof s.bytes);
            memcpy(s.bytes, name, (size_t)std::min<uint64_t>(name_len, kHnExemplarBytes));
            s.state = kHnPublished;
        }
    }
}

// The records of one batch's payload (as payload_batch_host takes them): a counted record with good headers is looked at.
template <class Passes>
inline void hn_batch_host(uint64_t *vec, HnSlot *table, const uint8_t *bytes, uint64_t pos, uint64_t end, uint64_t n_records, Passes passes)
{
    PayloadBytes src{bytes};
    payload_records_host(bytes, pos, end, n_records, passes, [&](long long, uint64_t, uint64_t after, uint64_t rec_end) {
        const PayloadHeaders h = payload_walk_headers(src, after, rec_end);
        if (h.bad) return;
        vec[kHnLooked]++, vec[kHnWithHeaders] += h.count != 0;
        payload_visit_headers(src, after, rec_end, [&](uint64_t name, uint64_t name_len, long long val_len) {
            hn_add_occurrence(vec, table, bytes + name, name_len, val_len);
        });
    });
}

// ---- the identities between the words of one vector --------------------------------------------------------------------
// payload: NULL, or the payload vector (kta_payload.h, P partitions) of the same run.
inline bool hn_identities_hold(const uint64_t *vec, const uint64_t *payload = nullptr, uint32_t P = 0)
{
    if (vec[kHnGlobalSums] || vec[kHnGlobalSums + 1]) return false;
    for (uint32_t r = 0; r < kPlRows; r++) {
        uint64_t sums[kHnCellBits] = {0, 0, 0, 0};
        for (uint32_t c = 0; c < kPlCells; c++) {
            const uint64_t *cell = vec + hn_cell_at(r, c);
            for (uint32_t k = 0; k < kHnCellBits; k++) sums[k] += cell[k];
            for (uint32_t k = 0; k < 32; k++)
                if (cell[kHnCellBits + k] > cell[kHnCellT]) return false;
        }
        if (sums[kHnCellT] != vec[kHnOccurrences] || sums[kHnCellL] != vec[kHnNameBytes] || sums[kHnCellV] != vec[kHnValueBytes] ||
            sums[kHnCellZ] != vec[kHnNullValues])
            return false;
    }
    if (vec[kHnWithHeaders] > vec[kHnLooked] || vec[kHnNullValues] > vec[kHnOccurrences]) return false;
    if (payload) {
        uint64_t headers = 0, keyb = 0, valb = 0, nulls = 0, with = 0, records = 0, bad = 0;
        for (uint32_t p = 0; p < P; p++) {
            const uint64_t *w = payload + (size_t)kPlPartitionWords * p;
            headers += w[kPlHeaders], keyb += w[kPlHeaderKeyBytes], valb += w[kPlHeaderValueBytes], nulls += w[kPlHeaderNullValues];
            with += w[kPlWithHeaders], records += w[kPlRecords], bad += w[kPlBadHeaders];
        }
        if (vec[kHnOccurrences] != headers || vec[kHnNameBytes] != keyb || vec[kHnValueBytes] != valb || vec[kHnNullValues] != nulls ||
            vec[kHnWithHeaders] != with || vec[kHnLooked] != records - bad)
            return false;
    }
    return true;
}

// ---- the read-off of the names -----------------------------------------------------------------------------------------
// kta_payload.h's peel over this table; a cell is pure only if, beyond that, its L is a multiple of its T (one name has one
// length).  A listed hash has its exact occurrences, name length (L / T), value bytes and null values; its name when a
// published slot of either of its cells holds that hash.  What remains in row 0 is the remainder: never guessed at.
struct HnListed {
    uint32_t hash;
    uint64_t occurrences, name_len, value_bytes, null_values;
    const HnSlot *name;          // nullptr: no exemplar
};

inline std::vector<HnListed> hn_list(const uint64_t *vec, const HnSlot *table, uint64_t *unresolved_occurrences, uint64_t *unresolved_value_bytes)
{
    std::vector<uint64_t> t(vec + kHnGlobals, vec + kHnWords);
    std::vector<HnListed> out;
    payload_peel<kHnCellWords>(t.data(), [](const uint64_t *cell) { return cell[kHnCellL] % cell[kHnCellT] == 0; },
                               [&](uint32_t h, const uint64_t *cell) {
                                   const HnSlot *name = nullptr;
                                   for (uint32_t r = 0; r < kPlRows && table && !name; r++) {
                                       const HnSlot *s = table + r * kPlCells + payload_cell(r, h);
                                       if (s->state == kHnPublished && s->hash == h) name = s;
                                   }
                                   out.push_back(HnListed{h, cell[kHnCellT], cell[kHnCellL] / cell[kHnCellT], cell[kHnCellV], cell[kHnCellZ], name});
                               });
    uint64_t uo = 0, uv = 0;
    for (uint32_t c = 0; c < kPlCells; c++) uo += t[(size_t)c * kHnCellWords + kHnCellT], uv += t[(size_t)c * kHnCellWords + kHnCellV];
    if (unresolved_occurrences) *unresolved_occurrences = uo;
    if (unresolved_value_bytes) *unresolved_value_bytes = uv;
    std::sort(out.begin(), out.end(), [](const HnListed &a, const HnListed &b) {
        return a.occurrences != b.occurrences ? a.occurrences > b.occurrences : a.value_bytes != b.value_bytes ? a.value_bytes > b.value_bytes : a.hash < b.hash;
    });
    return out;
}

} // namespace kta

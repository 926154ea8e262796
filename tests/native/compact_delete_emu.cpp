// compact_delete_emu.cpp — test infrastructure: the KEPT instantiation of the segment pass's wave step
// (csrc/kta_segments_wave.h, seg_wave_step<true>: the kept-apply kernel's own source) compiled for the host over
// tests/native/wave_emu.h and run with its 64 lanes as fibers.  tests/test_compact_delete_emu.py compares every lane's
// state, every row it closes and the final tables with the sequential loop.
#include "wave_emu.h"

#include "kta_compact_delete.h"

// (as tests/native/segments_emu.cpp: the order point is a meeting of its own)
#define KTA_SEG_LDS_ORDER() ((void)wave_emu::ballot(false, __LINE__))

namespace {
#include "kta_segments_wave.h"
}

extern "C" {

// n_instr instructions of 64 records each (partition, key_len, val_len, class byte: n_instr * 64 values) share the tables
// run[P][4] = {L, B, T, K} (in: the seed, out: the final table) and nxt[P] (out only: made from the seed here, as the apply
// kernel makes it).  at[n_instr * 64][6]: what every lane got — its four words, closes, row — all ones for a lane that does
// not take part.  counters[2]: instructions on the one-partition path, colliding groups.  order, seed: wave_emu::launch.
// Returns 0; -2: the emulator reports divergent meeting points.
int kta_emu_kept(const int32_t *partition, const int32_t *key_len, const int32_t *val_len, const uint8_t *cls, uint32_t n_instr, uint32_t P, uint64_t S,
                 uint32_t M, uint32_t overhead, uint64_t *run, uint64_t *nxt, uint64_t *at_out, uint32_t *counters, int order, uint32_t seed,
                 char *err_out, uint64_t err_cap)
{
    std::vector<uint64_t> table(run, run + (size_t)P * kta::kSegWords), next(P);
    for (uint32_t p = 0; p < P; p++) next[p] = kta::segments_next_boundary(table[(size_t)p * kta::kSegWords + kta::kKeptB], S, M);
    std::vector<uint8_t> tag(P, 0xEE);
    const char *err = wave_emu::launch(1, order, seed, [&] {
        const uint32_t lane = threadIdx.x;
        uint32_t n_one = 0, n_groups = 0;
        for (uint32_t j = 0; j < n_instr; j++) {
            const size_t i = (size_t)j * 64 + lane;
            const bool on = seg_takes_part(partition[i], P);
            const uint64_t z = kta::segments_record_size(overhead, key_len[i], val_len[i]);
            const bool live = cls[i] == kta::kKeptClassLive, tomb = cls[i] == kta::kKeptClassTombstone;
            SegAt at;
            at.closes = false;
            seg_wave_step<true>(table.data(), next.data(), tag.data(), lane, on, (uint32_t)partition[i], z, tomb, live || tomb ? z : 0ull, S, M, at,
                                n_one, n_groups, live);
            uint64_t *o = at_out + i * 6;
            for (uint32_t k = 0; k < 6; k++) o[k] = ~0ull;
            if (on) {
                for (uint32_t k = 0; k < kta::kSegWords; k++) o[k] = at.v[k];
                o[4] = at.closes ? 1u : 0u, o[5] = at.closes ? at.row : 0u;
            }
        }
        if (lane == 0) counters[0] = n_one, counters[1] = n_groups;
    });
    if (err) {
        if (err_out && err_cap) snprintf(err_out, err_cap, "%s", err);
        return -2;
    }
    for (size_t e = 0; e < (size_t)P * kta::kSegWords; e++) run[e] = table[e];
    for (uint32_t p = 0; p < P; p++) nxt[p] = next[p];
    return 0;
}

} // extern "C"

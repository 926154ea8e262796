// kta_lean_blocks.h — the block rule of the lean scan kernel (kta_kernels.hip: packed_scan_lean), once.
// A workgroup's step s is tile workgroup + s x grid.  A block is 64 consecutive steps; lane l of a wave classifies step
// 64 b + l (lean_tile) and the wave's two ballots are the block's plane mask and lean mask.  lean_block below makes of
// them the masks of the tiles the lean kernel takes, and applies the list rule to the others — the tiles inside the
// workgroup's range that are in neither mask — in step order: the first `max_listed` others of the workgroup go on the
// list (four 32-bit halves of two words, a step + 1 each, filled in ascending order); the next one is handed over: the
// lean kernel's steps end there, and kta_metrics_scan_packed_rest takes that step and all that follow.
// Plain C++ as well as HIP, host and device (tests/native/lean_blocks_check.cpp): no HIP runtime call, no LDS.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define KTA_LEAN_HD __host__ __device__
#else
#define KTA_LEAN_HD
#endif

namespace kta {

constexpr uint32_t kLeanBlockSteps = 64;

// What a workgroup carries from block to block (uniform).
struct LeanBlocks {
    uint32_t end = 0;                   // this kernel's steps end here: the workgroup's steps, or the handed-over step
    uint32_t listed = 0;                // entries on the list
    uint64_t list_a = 0, list_b = 0;    // the list: four steps + 1, 32 bits each
    uint32_t handover = 0;              // the step the rest kernel takes everything from, + 1
};

// The steps of workgroup `wg` of `grid` over a batch of `ntiles` tiles (below 2^31): tiles wg, wg + grid, ...
KTA_LEAN_HD inline uint32_t lean_steps(uint32_t wg, uint32_t grid, uint64_t ntiles)
{
    return wg < ntiles ? (uint32_t)((ntiles - 1u - wg) / grid) + 1u : 0u;
}

// The block that begins at step `base` (a multiple of 64, below s.end).  In: the ballots of the lanes' classes, whatever
// the lanes past the end voted.  Out: the steps the lean kernel takes in either form — a tile past s.end, a listed tile
// and everything from the handed-over step on are in neither.
KTA_LEAN_HD inline void lean_block(LeanBlocks &s, uint32_t base, uint32_t max_listed, uint64_t &plane, uint64_t &lean)
{
    const uint32_t left = s.end > base ? s.end - base : 0u;
    const uint64_t in = left >= kLeanBlockSteps ? ~0ull : (1ull << left) - 1ull;
    plane &= in;
    lean &= in & ~plane;
    uint64_t others = in & ~(plane | lean);
    while (others) {
        const uint32_t l = (uint32_t)__builtin_ctzll(others);
        others &= others - 1ull;
        const uint32_t step = base + l;
        if (s.listed == max_listed) {
            const uint64_t before = (1ull << l) - 1ull;
            s.handover = step + 1u;
            s.end = step;
            plane &= before;
            lean &= before;
            return;
        }
        const uint64_t e = (uint64_t)(step + 1u) << (32u * (s.listed & 1u));
        if (s.listed < 2) s.list_a |= e;
        else s.list_b |= e;
        s.listed++;
    }
}

}   // namespace kta

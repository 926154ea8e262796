// kta_wave_src.h — what the kernels that walk record bytes behind the decode kernel share (kta_payload_kernel.h,
// kta_header_names_kernel.h, kta_value_bytes_kernel.h) beside the walk itself (kta_record_walk.h: the payload kernel's; the
// other two keep its statements as their own text): the two byte
// sources of the header walks (kta_payload.h's Src) and the sums over a group of sixteen lanes and over the wave.  Included
// INSIDE the including file's unnamed namespace, as those three are; no includes of its own.  kWsL: the lanes per batch.
#pragma once

constexpr uint32_t kWsL = 16;

// A byte source over the blob: aligned 16-byte loads, one block cached (payload_walk_headers' Src).
struct BlockSrc {
    const uint4 *blocks;
    uint64_t cached_idx;
    uint4 cached;
    __device__ __forceinline__ uint32_t at(uint64_t pos)
    {
        const uint64_t bi = pos >> 4;
        if (bi != cached_idx) {
            cached = blocks[bi];
            cached_idx = bi;
        }
        const uint32_t w = (uint32_t)(pos >> 2) & 3u;
        const uint32_t word = w == 0 ? cached.x : (w == 1 ? cached.y : (w == 2 ? cached.z : cached.w));
        return (word >> ((uint32_t)(pos & 3u) * 8u)) & 0xFFu;
    }
};

// The same over the window in LDS, for a record that lies inside it.
struct WindowSrc {
    const uint8_t *win;
    uint64_t wbase;
    __device__ __forceinline__ uint32_t at(uint64_t pos) const { return win[(uint32_t)(pos - wbase)]; }
};

__device__ __forceinline__ uint64_t group_sum(uint64_t v)   // over the kWsL lanes of a group (aligned, a power of two)
{
#pragma unroll
    for (int m = (int)kWsL / 2; m >= 1; m >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, m);
    return v;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, m);
    return v;
}

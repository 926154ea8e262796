// kta_fnv.h — the reference's FNV-32 variant (src/fnv32.rs:76-101) on gfx950: the byte chain, the 16-byte and four-keys
// forms and the hash of a key whose first 16 bytes were prefetched, and fmix32, which the sketches put behind it.  Shared by
// the alive-key pass (kta_alive.hip), the key sketch (kta_sketch.hip) and the hot-key sketch (kta_hot.hip) through the keyed
// record stream (kta_key_stream.h); device code only, every helper inlined into its caller.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kta {

namespace {

constexpr uint32_t kFnvInit = 0x811c9dc5u;   // fnv32.rs:80
constexpr uint32_t kFnvMul = 0x811c9dc5u;    // fnv32.rs:97: the multiplier is the offset basis, not the FNV prime

__device__ __forceinline__ uint32_t fmix32(uint32_t x)   // murmur3's finaliser: a bijection
{
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ uint32_t fnv_byte(uint32_t h, uint32_t b) { return (h ^ b) * kFnvMul; }

// h ^ byte N of w in ONE instruction: gfx9's sub-dword addressing selects the byte inside the xor.  (Left to itself
// the compiler does that for byte 3 only; bytes 1 and 2 cost a shift and an and-xor each — a quarter of the chain.)
#define KTA_XOR_BYTE(N)                                                                                         \
    __device__ __forceinline__ uint32_t xor_byte##N(uint32_t h, uint32_t w)                                      \
    {                                                                                                           \
        uint32_t r;                                                                                             \
        asm("v_xor_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_" #N    \
            : "=v"(r)                                                                                           \
            : "v"(h), "v"(w));                                                                                  \
        return r;                                                                                               \
    }
KTA_XOR_BYTE(0)
KTA_XOR_BYTE(1)
KTA_XOR_BYTE(2)
KTA_XOR_BYTE(3)
#undef KTA_XOR_BYTE

__device__ __forceinline__ uint32_t fnv_word(uint32_t h, uint32_t w)
{
    h = xor_byte0(h, w) * kFnvMul;
    h = xor_byte1(h, w) * kFnvMul;
    h = xor_byte2(h, w) * kFnvMul;
    return xor_byte3(h, w) * kFnvMul;
}

__device__ __forceinline__ uint32_t fnv_16(uint32_t h, const uint4 &v)
{
    return fnv_word(fnv_word(fnv_word(fnv_word(h, v.x), v.y), v.z), v.w);
}

// Four 16-byte keys at once, their chains interleaved (one chain is 32 dependent instructions).
__device__ __forceinline__ void fnv_16x4(uint32_t (&h)[4], const uint4 (&k)[4])
{
    const uint32_t w[4][4] = {{k[0].x, k[0].y, k[0].z, k[0].w}, {k[1].x, k[1].y, k[1].z, k[1].w},
                              {k[2].x, k[2].y, k[2].z, k[2].w}, {k[3].x, k[3].y, k[3].z, k[3].w}};
#pragma unroll
    for (int j = 0; j < 4; j++) h[j] = kFnvInit;
#pragma unroll
    for (int d = 0; d < 4; d++) {
#pragma unroll
        for (int j = 0; j < 4; j++) h[j] = xor_byte0(h[j], w[j][d]) * kFnvMul;
#pragma unroll
        for (int j = 0; j < 4; j++) h[j] = xor_byte1(h[j], w[j][d]) * kFnvMul;
#pragma unroll
        for (int j = 0; j < 4; j++) h[j] = xor_byte2(h[j], w[j][d]) * kFnvMul;
#pragma unroll
        for (int j = 0; j < 4; j++) h[j] = xor_byte3(h[j], w[j][d]) * kFnvMul;
    }
}

// FNV of `len` more bytes at k (any alignment), continuing from h.  gfx950 runs in unaligned access mode,
// so the body is 16-byte loads at the key's own address; only the last 1..3 bytes go through aligned
// dwords that overlap the key (never a byte beyond the 4-byte word that holds the key's end).
__device__ __forceinline__ uint32_t fnv32_more(uint32_t h, const uint8_t *k, uint32_t len)
{
    while (len >= 16u) {
        uint4 v;
        __builtin_memcpy(&v, k, 16);
        h = fnv_16(h, v);
        k += 16;
        len -= 16u;
    }
    if (len >= 8u) {
        uint2 v;
        __builtin_memcpy(&v, k, 8);
        h = fnv_word(fnv_word(h, v.x), v.y);
        k += 8;
        len -= 8u;
    }
    if (len >= 4u) {
        uint32_t v;
        __builtin_memcpy(&v, k, 4);
        h = fnv_word(h, v);
        k += 4;
        len -= 4u;
    }
    if (len) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(k);
        const uint32_t *w = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
        const uint32_t skip = (uint32_t)(a & 3u);
        uint64_t two = w[0];
        if (skip + len > 4u) two |= (uint64_t)w[1] << 32;
        two >>= 8u * skip;
        for (uint32_t j = 0; j < len; j++) {
            h = fnv_byte(h, (uint32_t)two & 0xFFu);
            two >>= 8;
        }
    }
    return h;
}

// FNV of a key whose first 16 bytes are in registers
__device__ __forceinline__ uint32_t fnv32_prefetched(const uint4 &k16, const uint8_t *key, uint32_t len)
{
    if (len == 16u) return fnv_16(kFnvInit, k16);
    if (len > 16u) return fnv32_more(fnv_16(kFnvInit, k16), key + 16, len - 16u);
    const uint32_t w[4] = {k16.x, k16.y, k16.z, k16.w};
    uint32_t h = kFnvInit;
#pragma unroll
    for (uint32_t d = 0; d < 3; d++)
        if (len >= 4u * (d + 1u)) h = fnv_word(h, w[d]);
    const uint32_t q = len >> 2;
    uint32_t tw = q == 0u ? w[0] : (q == 1u ? w[1] : (q == 2u ? w[2] : w[3]));
    for (uint32_t t = len & 3u; t > 0u; t--) {
        h = fnv_byte(h, tw & 0xFFu);
        tw >>= 8;
    }
    return h;
}

} // namespace

} // namespace kta

// kta_key_stream.h — the keyed record stream of the passes that hash every key (pass 1 of the alive-key pass, both states:
// kta_alive.hip; the key sketch: kta_sketch.hip; the hot keys: kta_hot.hip), once: a wave step is 256 records, instruction j
// of it takes the records 64 j + lane, the first 16 bytes of every key are requested a step before they are hashed, and a
// wave whose keys are all 16 bytes long hashes four of them with interleaved chains.  Device code only, every helper
// inlined into its caller.
#pragma once

#include "kta_fnv.h"
#include "kta_kernels.h"

namespace kta {

namespace {

typedef uint32_t v4u_any __attribute__((ext_vector_type(4), aligned(1)));   // 16 key bytes at any address (unaligned access mode)

// The first 16 bytes of the four keys of a lane's step (key None or empty: the blob's first bytes, not used).
// Unconditional: key_bytes is readable for 16 bytes past the last key.  NT: non-temporal loads.
template <bool NT>
__device__ __forceinline__ void prefetch_keys4(const uint8_t *key_bytes, const int32_t (&kl)[4], const uint32_t (&ko)[4], uint4 (&keys)[4])
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const v4u_any *a = reinterpret_cast<const v4u_any *>(key_bytes + (kl[j] > 0 ? ko[j] : 0u));
        const v4u_any kk = NT ? __builtin_nontemporal_load(a) : *a;
        keys[j] = make_uint4(kk.x, kk.y, kk.z, kk.w);
    }
}

// h[j] = the reference's FNV-32 of key j (fnv32.rs:92-101; key None or empty: the offset basis), from the prefetched bytes
__device__ __forceinline__ void hash_keys4(uint32_t (&h)[4], const uint4 (&keys)[4], const uint8_t *key_bytes, const int32_t (&kl)[4],
                                           const uint32_t (&ko)[4])
{
    if (__all(kl[0] == 16 && kl[1] == 16 && kl[2] == 16 && kl[3] == 16)) {
        fnv_16x4(h, keys);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) h[j] = kl[j] > 0 ? fnv32_prefetched(keys[j], key_bytes + ko[j], (uint32_t)kl[j]) : kFnvInit;
    }
}

// What the sketches read of a step's records: key length, key offset, partition.
struct KeyedCols {
    int32_t kl[4];       // -1: key None, or no record
    uint32_t ko[4];
    int32_t pt[4];
};

// Step `step` (of nsteps, STEP records each) of the n records of c.  Every load is unconditional — the index clamped
// into the batch, the result masked —, so that a wave requests its next step's columns before it hashes this one's.
// (The scalars come by reference, as the lambdas this replaces captured them: by value the compiler kept two more vector
// registers in both kernels, and the key sketch's eight waves per SIMD have 64.)
template <uint32_t STEP>
__device__ __forceinline__ void load_keyed_cols(const SketchColumns &c, const uint64_t &step, const uint64_t &nsteps, const uint64_t &n, const uint32_t &lane, KeyedCols &r)
{
    static_assert(STEP == 256, "four instructions of 64 lanes");
    const bool ok = step < nsteps;
    const StepTile st = step_tile(c.hdr, c.rec0 + step * STEP, STEP, ok);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint64_t i = step * STEP + 64u * j + lane;
        const bool in = ok && i < n;
        const uint64_t ic = in ? i : n - 1;
        r.kl[j] = __builtin_nontemporal_load(c.key_len + ic);
        r.ko[j] = __builtin_nontemporal_load(c.key_off + ic);
        if (c.hdr) r.pt[j] = step_tile_part<true>(st, c.partition, c.hdr, c.rec0 + ic);
        else r.pt[j] = __builtin_nontemporal_load(c.partition + ic);
        r.kl[j] = in ? r.kl[j] : -1;
    }
}

} // namespace

} // namespace kta

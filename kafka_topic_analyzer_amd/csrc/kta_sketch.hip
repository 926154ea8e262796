// kta_sketch.hip — the opt-in key sketch (KTA_FLAG_KEY_SKETCH, include/kta_hip.h): one HyperLogLog register array per
// partition over the reference's FNV-32 of every keyed record (src/fnv32.rs:76-101, the hash the -c pass uses), so that
// "distinct keys" means what -c means by a key.  No reference counterpart.
//
//   kta_key_sketch        streams partition (u16 in compact tiles), key_len, key_off and the key bytes once — the 16-byte
//                         prefetch and the all-16-byte-keys form of the alive pass's pass 1 (kta_fnv.h) — and raises
//                         M[p][x >> 20] to rho(x << 12) for x = fmix32(fnv(key)).  A record reaches memory only past two
//                         filters: its group's floor in LDS (the least register of 4096 >> group_shift registers of its
//                         partition, refreshed before every launch), then a read of the register itself.  What is left
//                         takes an atomicMax, after the lanes of the wave that share the first such lane's register are
//                         combined into one.  Registers only grow, so a stale floor or read costs an atomic, never an
//                         update: the registers are exact whatever the filters see.
//   kta_key_sketch_floor  floors[p][g] = min of the group's registers (u8)
//   kta_key_sketch_widen  the u32 live registers into the u64 snapshot (one register per word: what the collectives reduce)
#include "kta_key_stream.h"

#include <algorithm>

namespace kta {

namespace {

constexpr int kSketchThreads = 256;
constexpr uint32_t kSketchStep = 256;            // records of one wave step: instruction j of it takes the records 64 j + lane
constexpr int kSketchWgPerCu = 8;

__global__ __launch_bounds__(kSketchThreads) void kta_key_sketch(SketchColumns c, uint64_t n, uint32_t P, uint32_t *regs,
                                                                  const uint8_t *__restrict__ floors, uint32_t group_shift,
                                                                  unsigned long long *stats)
{
    __shared__ uint8_t s_floor[kSketchFloorBytes];
    __shared__ unsigned long long s_cnt[3];
    const uint32_t nfloor = P << (KTA_SKETCH_LOG2 - group_shift);
    for (uint32_t e = threadIdx.x; e < nfloor; e += kSketchThreads) s_floor[e] = floors[e];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0ull;
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nsteps = (n + kSketchStep - 1) / kSketchStep;
    const uint64_t waves = (uint64_t)gridDim.x * (kSketchThreads / 64);
    uint64_t step = (uint64_t)blockIdx.x * (kSketchThreads / 64) + (threadIdx.x >> 6);
    uint32_t n_keyed = 0, n_read = 0, n_atomic = 0;   // (wave-uniform: popcounts of ballots)

    KeyedCols cur;
    load_keyed_cols<kSketchStep>(c, step, nsteps, n, lane, cur);
    while (step < nsteps) {
        uint4 keys[4];
        prefetch_keys4<false>(c.key_bytes, cur.kl, cur.ko, keys);
        const uint64_t next = step + waves;
        KeyedCols nxt;
        load_keyed_cols<kSketchStep>(c, next, nsteps, n, lane, nxt);
        uint32_t h[4];
        hash_keys4(h, keys, c.key_bytes, cur.kl, cur.ko);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            // key Some (the empty key included) in a partition the metrics handler counts
            const bool keyed = cur.kl[j] >= 0 && (uint32_t)cur.pt[j] < P;
            const uint32_t x = fmix32(h[j]);
            const uint32_t reg = x >> (32 - KTA_SKETCH_LOG2);
            const uint32_t w = x << KTA_SKETCH_LOG2;
            const uint32_t rho = w == 0u ? (33u - KTA_SKETCH_LOG2) : (uint32_t)__builtin_clz(w) + 1u;
            const uint32_t p = keyed ? (uint32_t)cur.pt[j] : 0u;
            const bool pass = keyed && rho > s_floor[(p << (KTA_SKETCH_LOG2 - group_shift)) | (reg >> group_shift)];
            const uint64_t idx = (uint64_t)p * kSketchRegs + reg;
            bool need = false;
            if (pass) need = rho > __hip_atomic_load(regs + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            n_keyed += (uint32_t)__popcll(__ballot(keyed));
            n_read += (uint32_t)__popcll(__ballot(pass));
            const unsigned long long m = __ballot(need);
            if (m) {
                // the lanes on the first needing lane's register: one atomic with their largest rho (one key repeated)
                const int leader = __ffsll((long long)m) - 1;
                const uint64_t lidx = __shfl(idx, leader);
                const bool same = need && idx == lidx;
                uint32_t r = same ? rho : 0u;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) r = max(r, (uint32_t)__shfl_xor(r, off));
                if ((int)lane == leader) atomicMax(regs + lidx, r);
                if (need && !same) atomicMax(regs + idx, rho);
                n_atomic += 1u + (uint32_t)__popcll(__ballot(need && !same));
            }
        }
        cur = nxt;
        step = next;
    }
    if (lane == 0) {
        atomicAdd(&s_cnt[0], (unsigned long long)n_keyed);
        atomicAdd(&s_cnt[1], (unsigned long long)n_read);
        atomicAdd(&s_cnt[2], (unsigned long long)n_atomic);
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(stats + threadIdx.x, s_cnt[threadIdx.x]);
}

__global__ __launch_bounds__(256) void kta_key_sketch_floor(const uint32_t *__restrict__ regs, uint32_t P, uint32_t group_shift,
                                                            uint8_t *__restrict__ floors)
{
    const uint64_t nout = (uint64_t)P << (KTA_SKETCH_LOG2 - group_shift);
    const uint32_t per = 1u << group_shift;   // registers of a group, contiguous
    for (uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < nout; o += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t *g = regs + o * per;
        uint32_t m = 0xFFFFFFFFu;
        if (per >= 4u) {
            for (uint32_t k = 0; k < per; k += 4u) {
                const uint4 v = *reinterpret_cast<const uint4 *>(g + k);
                m = min(m, min(min(v.x, v.y), min(v.z, v.w)));
            }
        } else {
            for (uint32_t k = 0; k < per; k++) m = min(m, g[k]);
        }
        floors[o] = (uint8_t)m;   // (registers are at most 21)
    }
}

__global__ __launch_bounds__(256) void kta_key_sketch_widen(const uint32_t *__restrict__ regs, uint64_t n, uint64_t *__restrict__ out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = regs[i];
}

} // namespace

hipError_t launch_key_sketch(const SketchColumns &c, uint64_t n, uint32_t P, uint32_t *regs, const uint8_t *floors,
                             uint64_t *stats, int cu_count, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    const uint64_t waves = (n + kSketchStep - 1) / kSketchStep;
    const uint64_t want = (waves + kSketchThreads / 64 - 1) / (kSketchThreads / 64);
    const uint64_t cap = (uint64_t)(cu_count > 0 ? cu_count : 256) * kSketchWgPerCu;
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    hipLaunchKernelGGL(kta_key_sketch, dim3(grid), dim3(kSketchThreads), 0, s, c, n, P, regs, floors, sketch_group_shift(P),
                       reinterpret_cast<unsigned long long *>(stats));
    return hipGetLastError();
}

hipError_t launch_key_sketch_floor(const uint32_t *regs, uint32_t P, uint8_t *floors, hipStream_t s)
{
    const uint32_t shift = sketch_group_shift(P);
    const uint64_t nout = (uint64_t)P << (KTA_SKETCH_LOG2 - shift);
    const uint32_t grid = (uint32_t)std::min<uint64_t>((nout + 255) / 256, 4096);
    hipLaunchKernelGGL(kta_key_sketch_floor, dim3(grid), dim3(256), 0, s, regs, P, shift, floors);
    return hipGetLastError();
}

hipError_t launch_key_sketch_widen(const uint32_t *regs, uint64_t n, uint64_t *out, hipStream_t s)
{
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(kta_key_sketch_widen, dim3(grid), dim3(256), 0, s, regs, n, out);
    return hipGetLastError();
}

} // namespace kta

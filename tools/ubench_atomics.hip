// Developer microbenchmark (not product code): throughput of 64-bit atomicMax on random slots of a
// table, by memory scope and working-set size.  Informs the alive-key pass design.
//   ubench_atomics lds : instead, the rate of non-returning LDS adds (ds_add_u64 / ds_add_u32) in the metrics scan's
//   geometry: 256 partitions x 4 lane replicas, 5 workgroups of 4 waves per CU; and the two forms of
//   a plane record's adds, per record: two ds_add_u64 (W1 and W2), or one ds_add_u64 and a ds_add_u32 that a random
//   tenth of the lanes executes (kta_plane_pack.h).
#include <string.h>
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <vector>

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

template <int SCOPE, bool RET>
__global__ __launch_bounds__(256) void k_atomic(unsigned long long *table, uint64_t mask, uint64_t n, uint64_t seed,
                                                unsigned long long *sink)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    unsigned long long acc = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const uint64_t slot = mix64(seed + i) & mask;
        const unsigned long long v = (i << 1) | 1ull;
        if (RET) acc += __hip_atomic_fetch_max(&table[slot], v, __ATOMIC_RELAXED, SCOPE);
        else (void)__hip_atomic_fetch_max(&table[slot], v, __ATOMIC_RELAXED, SCOPE);
    }
    if (RET && acc == 0x1234567) *sink = acc;
}

// plain (non-atomic) read-modify-write for comparison
__global__ __launch_bounds__(256) void k_plain(unsigned long long *table, uint64_t mask, uint64_t n, uint64_t seed)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const uint64_t slot = mix64(seed + i) & mask;
        const unsigned long long v = (i << 1) | 1ull;
        if (table[slot] < v) table[slot] = v;
    }
}

// LDS adds on the scan's slots: slot = part << 2 | lane & 3 with `part` random in [0, 256) (MODE 0), or slot = thread
// (MODE 1: no two lanes of a wave on one bank beyond what the width itself costs).  Each lane cycles through 16 slots it
// drew before the timed loop, so the loop body is the adds and a counter.  T = unsigned long long or uint32_t.
constexpr int kLdsSlots = 1024, kLdsDraws = 16;
template <typename T, int MODE>
__global__ __launch_bounds__(256) void k_lds_add(uint32_t iters, uint64_t seed, unsigned long long *sink)
{
    __shared__ T tab[kLdsSlots];
    for (uint32_t i = threadIdx.x; i < kLdsSlots; i += 256) tab[i] = 0;
    uint32_t slot[kLdsDraws];
#pragma unroll
    for (int j = 0; j < kLdsDraws; j++) {
        const uint32_t part = (uint32_t)mix64(seed + ((uint64_t)blockIdx.x * 256 + threadIdx.x) * kLdsDraws + j) & 255u;
        slot[j] = MODE == 0 ? (part << 2 | (threadIdx.x & 3u)) : ((threadIdx.x + 64u * j) & (kLdsSlots - 1));
    }
    __syncthreads();
    for (uint32_t it = 0; it < iters; it++) {
#pragma unroll
        for (int j = 0; j < kLdsDraws; j++)
            (void)__hip_atomic_fetch_add(&tab[slot[j]], (T)(it | 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    unsigned long long acc = 0;
    for (uint32_t i = threadIdx.x; i < kLdsSlots; i += 256) acc += tab[i];
    if (acc == 0x1234567) *sink = acc;
}

// A plane record's adds on the scan's slots, two tables as the front level has them.  FORM 0: two ds_add_u64, W1[slot]
// and W2[slot].  FORM 1: one ds_add_u64 to W1[slot] and one ds_add_u32 to the low dword of W2[slot], executed by the
// lanes whose draw carries a flag — a random tenth, drawn with the slots before the timed loop.
template <int FORM>
__global__ __launch_bounds__(256) void k_lds_pair(uint32_t iters, uint64_t seed, unsigned long long *sink)
{
    __shared__ unsigned long long w1[kLdsSlots], w2[kLdsSlots];
    for (uint32_t i = threadIdx.x; i < kLdsSlots; i += 256) w1[i] = 0, w2[i] = 0;
    uint32_t slot[kLdsDraws], flagged = 0;
#pragma unroll
    for (int j = 0; j < kLdsDraws; j++) {
        const uint64_t d = mix64(seed + ((uint64_t)blockIdx.x * 256 + threadIdx.x) * kLdsDraws + j);
        slot[j] = ((uint32_t)d & 255u) << 2 | (threadIdx.x & 3u);
        flagged |= (uint32_t)((d >> 32) % 10u == 0u) << j;
    }
    __syncthreads();
    for (uint32_t it = 0; it < iters; it++) {
#pragma unroll
        for (int j = 0; j < kLdsDraws; j++) {
            (void)__hip_atomic_fetch_add(&w1[slot[j]], (unsigned long long)(it | 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (FORM == 0)
                (void)__hip_atomic_fetch_add(&w2[slot[j]], (unsigned long long)(it | 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else if ((flagged >> j) & 1u)
                (void)__hip_atomic_fetch_add(reinterpret_cast<uint32_t *>(&w2[slot[j]]), it | 1u, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    __syncthreads();
    unsigned long long acc = 0;
    for (uint32_t i = threadIdx.x; i < kLdsSlots; i += 256) acc += w1[i] + w2[i];
    if (acc == 0x1234567) *sink = acc;
}

static int lds_main()
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { printf("no device\n"); return 1; }
    const int cus = prop.multiProcessorCount, per_cu = 5;
    const double mhz = prop.clockRate / 1e3;
    unsigned long long *sink;
    hipMalloc(&sink, 8);
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    const uint32_t iters = 4096;
    printf("LDS adds, non-returning: %d CUs x %d workgroups x 4 waves, %u x %d instructions per wave, clock %.0f MHz\n", cus,
           per_cu, iters, kLdsDraws, mhz);
    const char *names[6] = {"ds_add_u64 scan slots (random part << 2 | lane & 3)", "ds_add_u64 slot = thread",
                            "ds_add_u32 scan slots (random part << 2 | lane & 3)", "ds_add_u32 slot = thread",
                            "record: ds_add_u64 + ds_add_u64, scan slots", "record: ds_add_u64 + ds_add_u32 by a tenth of the lanes"};
    for (int mode = 0; mode < 6; mode++) {
        float best = 1e9;
        for (int rep = 0; rep < 4; rep++) {
            hipEventRecord(a);
            switch (mode) {
            case 0: hipLaunchKernelGGL((k_lds_add<unsigned long long, 0>), dim3(cus * per_cu), dim3(256), 0, 0, iters, 7 + rep, sink); break;
            case 1: hipLaunchKernelGGL((k_lds_add<unsigned long long, 1>), dim3(cus * per_cu), dim3(256), 0, 0, iters, 7 + rep, sink); break;
            case 2: hipLaunchKernelGGL((k_lds_add<uint32_t, 0>), dim3(cus * per_cu), dim3(256), 0, 0, iters, 7 + rep, sink); break;
            case 3: hipLaunchKernelGGL((k_lds_add<uint32_t, 1>), dim3(cus * per_cu), dim3(256), 0, 0, iters, 7 + rep, sink); break;
            case 4: hipLaunchKernelGGL((k_lds_pair<0>), dim3(cus * per_cu), dim3(256), 0, 0, iters, 7 + rep, sink); break;
            default: hipLaunchKernelGGL((k_lds_pair<1>), dim3(cus * per_cu), dim3(256), 0, 0, iters, 7 + rep, sink); break;
            }
            hipEventRecord(b);
            if (hipEventSynchronize(b) != hipSuccess) { printf("kernel failed\n"); return 1; }
            float ms; hipEventElapsedTime(&ms, a, b);
            if (rep > 0 && ms < best) best = ms;   // (the first launch of each kernel loads its code)
        }
        const double per_cu_insts = (double)per_cu * 4 * iters * kLdsDraws;
        const double ns = best * 1e6 / per_cu_insts;
        printf("%-56s %8.3f ms  %6.2f ns per wave %s per CU = %5.1f cycles at %.0f MHz\n", names[mode], best, ns,
               mode < 4 ? "instruction" : "record", ns * mhz / 1e3, mhz);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "lds")) return lds_main();
    const uint64_t n = 1ull << 26;
    unsigned long long *table, *sink;
    const uint64_t max_slots = 1ull << 32;
    if (hipMalloc(&table, max_slots * 8) != hipSuccess) { printf("alloc failed\n"); return 1; }
    hipMalloc(&sink, 8);
    hipMemset(table, 0, max_slots * 8);
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    const int grid = 256 * 8;
    for (int log2slots : {14, 17, 20, 23, 26, 29, 32}) {
        const uint64_t mask = (1ull << log2slots) - 1;
        for (int mode = 0; mode < 5; mode++) {
            float best = 1e9;
            for (int rep = 0; rep < 3; rep++) {
                hipEventRecord(a);
                switch (mode) {
                case 0: hipLaunchKernelGGL((k_atomic<__HIP_MEMORY_SCOPE_AGENT, false>), dim3(grid), dim3(256), 0, 0, table, mask, n, 7 + rep, sink); break;
                case 1: hipLaunchKernelGGL((k_atomic<__HIP_MEMORY_SCOPE_AGENT, true>), dim3(grid), dim3(256), 0, 0, table, mask, n, 7 + rep, sink); break;
                case 2: hipLaunchKernelGGL((k_atomic<__HIP_MEMORY_SCOPE_WORKGROUP, false>), dim3(grid), dim3(256), 0, 0, table, mask, n, 7 + rep, sink); break;
                case 3: hipLaunchKernelGGL((k_atomic<__HIP_MEMORY_SCOPE_WORKGROUP, true>), dim3(grid), dim3(256), 0, 0, table, mask, n, 7 + rep, sink); break;
                default: hipLaunchKernelGGL(k_plain, dim3(grid), dim3(256), 0, 0, table, mask, n, 7 + rep); break;
                }
                hipEventRecord(b);
                hipEventSynchronize(b);
                float ms; hipEventElapsedTime(&ms, a, b);
                if (ms < best) best = ms;
            }
            const char *names[5] = {"agent-scope atomicMax (no return)", "agent-scope atomicMax (returning)",
                                    "workgroup-scope atomicMax (no return; L2-local, NOT cross-XCD coherent)",
                                    "workgroup-scope atomicMax (returning)", "plain load/compare/store (racy)"};
            printf("slots=2^%-2d (%8.1f MB)  %-72s %7.3f ms  %6.2f G/s\n", log2slots, (double)(8ull << log2slots) / 1e6,
                   names[mode], best, n / best / 1e6);
        }
    }
    return 0;
}

// kta_alive_table.hip — the single-kernel alive-table family for gfx950 (MI355X / CDNA4): one kernel hashes a record's
// key and updates the 2^32-slot last-writer-wins table (alive_variant 0 / 1 / 2, the ablation pair 8 / 9), and the
// kernels that count, export, import and walk the table and its written list for the multi-GPU exchange (kta_comm.hip).
// The partitioned alive-key pass is kta_alive.hip.
//
// Reference semantics (paths under /root/reference):
//   kta_alive_update   src/metric.rs:289-304  LogCompactionInMemoryMetrics::handle_message
//                      src/metric.rs:256-260  fnv1a        src/fnv32.rs:92-101  FnvHasher::write
//   kta_alive_count    src/metric.rs:282-284  sum_all_alive
#include "kta_fnv.h"
#include "kta_kernels.h"

#include <limits.h>

namespace kta {

// ---------------------------------------------------------------------------------------
// K2 + K3  FNV + last-writer-wins alive table
// ---------------------------------------------------------------------------------------
// fnv32.rs:92-101: h = 0x811c9dc5; for each byte: h ^= byte; h *= 0x811c9dc5 (wrapping).
// The multiplier is the offset basis, not the FNV prime (kFnvInit, kFnvMul: kta_fnv.h).

__device__ __forceinline__ uint32_t fnv_step(uint32_t h, uint32_t byte) { return (h ^ byte) * kFnvMul; }

// Hash `len` bytes starting at byte pointer k (any alignment) with aligned 4-byte loads.
// Reads only whole dwords that overlap the key, so it may touch up to 3 bytes before and
// after the key inside the same 4-byte words (the key blob is allocated padded to 16 B).
__device__ __forceinline__ uint32_t fnv32_global(const uint8_t *k, uint32_t len)
{
    uint32_t h = kFnvInit;
    if (len == 0) return h;
    const uintptr_t a = reinterpret_cast<uintptr_t>(k);
    const uint32_t *w = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
    uint32_t skip = (uint32_t)(a & 3u);
    uint32_t word = *w++;
    word >>= 8u * skip;
    uint32_t avail = 4u - skip;
    while (true) {
        const uint32_t take = len < avail ? len : avail;
        if (take == 4u) {
            h = fnv_step(h, word & 0xFFu);
            h = fnv_step(h, (word >> 8) & 0xFFu);
            h = fnv_step(h, (word >> 16) & 0xFFu);
            h = fnv_step(h, word >> 24);
        } else {
            for (uint32_t j = 0; j < take; j++) {
                h = fnv_step(h, word & 0xFFu);
                word >>= 8;
            }
        }
        len -= take;
        if (len == 0) break;
        word = *w++;
        avail = 4u;
    }
    return h;
}

// table[h] = max(table[h], ((seq+1) << 1) | alive): the entry with the largest sequence
// number is the last writer in consumption order, which is exactly what sequential
// BitSet insert/remove leaves behind (metric.rs:273-280, 291-303).  0 == never written.
__global__ __launch_bounds__(kWG) void kta_alive_update(AliveColumns c, uint64_t n, uint64_t base_seq,
                                                        unsigned long long *__restrict__ table, WrittenList wl)
{
    const uint64_t stride = (uint64_t)gridDim.x * kWG;
    for (uint64_t i = (uint64_t)blockIdx.x * kWG + threadIdx.x; i < n; i += stride) {
        const int32_t kl = c.key_len[i];
        if (kl < 0) continue; // key None: ignored (metric.rs:302)
        const uint32_t h = fnv32_global(c.key_bytes + c.key_off[i], (uint32_t)kl);
        const uint64_t s = c.seq ? c.seq[i] : base_seq + i;
        const unsigned long long v = ((unsigned long long)(s + 1) << 1) | (c.val_len[i] >= 0 ? 1ull : 0ull);
        note_new_slot(wl, atomicMax(&table[h], v) == 0ull, h);
    }
}

// Variant with a RUNNING alive count.  atomicMax returns the previous entry; when this record
// replaces it (v > old) the number of alive slots changes by flag(v) - flag(old).  Updates to one
// address are serialised by the memory-side atomic unit, so over any interleaving the deltas
// telescope to flag(final) - flag(initial): the running sum is exactly sum_all_alive()
// (metric.rs:282-284) without scanning the 32 GiB table.
__global__ __launch_bounds__(kWG) void kta_alive_update_counting(AliveColumns c, uint64_t n, uint64_t base_seq,
                                                                 unsigned long long *__restrict__ table,
                                                                 long long *__restrict__ running, WrittenList wl)
{
    __shared__ long long s_w[kWG / 64];
    const uint64_t stride = (uint64_t)gridDim.x * kWG;
    long long delta = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kWG + threadIdx.x; i < n; i += stride) {
        const int32_t kl = c.key_len[i];
        if (kl < 0) continue;
        const uint32_t h = fnv32_global(c.key_bytes + c.key_off[i], (uint32_t)kl);
        const uint64_t s = c.seq ? c.seq[i] : base_seq + i;
        const unsigned long long v = ((unsigned long long)(s + 1) << 1) | (c.val_len[i] >= 0 ? 1ull : 0ull);
        const unsigned long long old = atomicMax(&table[h], v);
        note_new_slot(wl, old == 0ull, h);
        if (v > old) delta += (long long)(v & 1ull) - (long long)(old & 1ull);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) delta += __shfl_xor(delta, off);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = delta;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0;
        for (int w = 0; w < kWG / 64; w++) t += s_w[w];
        if (t) atomicAdd(reinterpret_cast<unsigned long long *>(running), (unsigned long long)t);
    }
}

// Variant 2: the counting kernel with a pre-read and the batch walked from its END.  A record only needs
// the table if no later record owns its slot yet; walking the batch backwards lets the LAST record of a
// key arrive first, so the earlier ones (a compacted topic repeats its keys) find a larger entry with a
// plain load and skip the memory-side atomic, which is the scarce resource (section 3.3 of DESIGN.md).
// Exactness does not depend on the order or on what the load sees: entries only grow, so `seen >= v`
// proves that a later record has already been applied, and a stale smaller value merely costs the atomic.
__global__ __launch_bounds__(kWG) void kta_alive_update_filtered(AliveColumns c, uint64_t n, uint64_t base_seq,
                                                                 unsigned long long *__restrict__ table,
                                                                 long long *__restrict__ running,
                                                                 const uint32_t *__restrict__ only_if, WrittenList wl)
{
    __shared__ long long s_w[kWG / 64];
    if (only_if && *only_if == 0u) return;   // stands in for the partitioned pass only when that gave the batch up
    const uint64_t stride = (uint64_t)gridDim.x * kWG;
    long long delta = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * kWG + threadIdx.x; j < n; j += stride) {
        const uint64_t i = n - 1 - j;                      // highest sequence numbers first
        const int32_t kl = c.key_len[i];
        if (kl < 0) continue;
        const uint32_t h = fnv32_global(c.key_bytes + c.key_off[i], (uint32_t)kl);
        const uint64_t s = c.seq ? c.seq[i] : base_seq + i;
        const unsigned long long v = ((unsigned long long)(s + 1) << 1) | (c.val_len[i] >= 0 ? 1ull : 0ull);
        const unsigned long long seen = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen >= v) continue;
        const unsigned long long old = atomicMax(&table[h], v);
        note_new_slot(wl, old == 0ull, h);
        if (v > old) delta += (long long)(v & 1ull) - (long long)(old & 1ull);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) delta += __shfl_xor(delta, off);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = delta;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0;
        for (int w = 0; w < kWG / 64; w++) t += s_w[w];
        if (t) atomicAdd(reinterpret_cast<unsigned long long *>(running), (unsigned long long)t);
    }
}

// Ablation kernels (alive_variant 8 / 9): hash only (h -> scratch) and table update only
// (h <- scratch).  Used to attribute time; the pair is also a valid two-phase implementation.
__global__ __launch_bounds__(kWG) void kta_alive_hash_only(AliveColumns c, uint64_t n, uint32_t *__restrict__ hout)
{
    const uint64_t stride = (uint64_t)gridDim.x * kWG;
    for (uint64_t i = (uint64_t)blockIdx.x * kWG + threadIdx.x; i < n; i += stride) {
        const int32_t kl = c.key_len[i];
        hout[i] = kl < 0 ? 0u : fnv32_global(c.key_bytes + c.key_off[i], (uint32_t)kl);
    }
}

__global__ __launch_bounds__(kWG) void kta_alive_apply_only(AliveColumns c, uint64_t n, uint64_t base_seq,
                                                            const uint32_t *__restrict__ hin,
                                                            unsigned long long *__restrict__ table, WrittenList wl)
{
    const uint64_t stride = (uint64_t)gridDim.x * kWG;
    for (uint64_t i = (uint64_t)blockIdx.x * kWG + threadIdx.x; i < n; i += stride) {
        if (c.key_len[i] < 0) continue;
        const uint64_t s = c.seq ? c.seq[i] : base_seq + i;
        const unsigned long long v = ((unsigned long long)(s + 1) << 1) | (c.val_len[i] >= 0 ? 1ull : 0ull);
        note_new_slot(wl, atomicMax(&table[hin[i]], v) == 0ull, hin[i]);
    }
}

__global__ __launch_bounds__(kWG) void kta_fnv32(const uint8_t *key_bytes, const uint32_t *key_off,
                                                 const int32_t *key_len, uint64_t n, uint32_t *out)
{
    const uint64_t i = (uint64_t)blockIdx.x * kWG + threadIdx.x;
    if (i >= n) return;
    const int32_t kl = key_len[i];
    out[i] = kl < 0 ? 0u : fnv32_global(key_bytes + key_off[i], (uint32_t)kl);
}

// K4: popcount of the alive bits.  16 B/lane streaming read of the u64 table.
__global__ __launch_bounds__(kWG) void kta_alive_count(const ulonglong2 *__restrict__ table2,
                                                       uint64_t n_pairs, unsigned long long *out)
{
    __shared__ unsigned long long s_w[kWG / 64];
    const uint64_t stride = (uint64_t)gridDim.x * kWG;
    unsigned long long cnt = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kWG + threadIdx.x; i < n_pairs; i += stride) {
        const ulonglong2 e = table2[i];
        cnt += (e.x & 1ull) + (e.y & 1ull);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kWG / 64; w++) t += s_w[w];
        if (t) atomicAdd(out, t);
    }
}

// Alive bits of the slots [lo, hi) only (any bounds): what the owner of a hash range counts after the
// hash-range exchange of a multi-GPU run.  8 B/lane.
__global__ __launch_bounds__(kWG) void kta_alive_count_span(const uint64_t *__restrict__ table, uint64_t lo,
                                                            uint64_t hi, unsigned long long *out)
{
    __shared__ unsigned long long s_w[kWG / 64];
    const uint64_t stride = (uint64_t)gridDim.x * kWG;
    unsigned long long cnt = 0;
    for (uint64_t i = lo + (uint64_t)blockIdx.x * kWG + threadIdx.x; i < hi; i += stride) cnt += table[i] & 1ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kWG / 64; w++) t += s_w[w];
        if (t) atomicAdd(out, t);
    }
}

// The same, but only when the written list is no longer complete (see launch_written_alive_count).
__global__ __launch_bounds__(kWG) void kta_alive_count_span_if_overflowed(WrittenList wl, const uint64_t *__restrict__ table, uint64_t lo,
                                                                          uint64_t hi, unsigned long long *out)
{
    __shared__ unsigned long long s_w[kWG / 64];
    if (*wl.n <= wl.cap) return;
    const uint64_t stride = (uint64_t)gridDim.x * kWG;
    unsigned long long cnt = 0;
    for (uint64_t i = lo + (uint64_t)blockIdx.x * kWG + threadIdx.x; i < hi; i += stride) cnt += table[i] & 1ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kWG / 64; w++) t += s_w[w];
        if (t) atomicAdd(out, t);
    }
}

// Compact export of the entries ever written (value != 0): (slot u32, value u64) pairs.  A shard's
// table holds at most one entry per distinct key hash it has seen, so this is what partition-sharded
// GPUs exchange instead of the 32 GiB table.  Each workgroup sweeps a contiguous slab, stages hits in
// LDS and reserves output space with ONE device atomic per flush (not per hit).
constexpr uint32_t kExportStage = 2048;

__global__ __launch_bounds__(kWG) void kta_alive_export(const unsigned long long *__restrict__ table,
                                                        uint64_t n_slots, uint32_t slot_base,
                                                        uint32_t *__restrict__ out_slots,
                                                        unsigned long long *__restrict__ out_vals,
                                                        unsigned long long *__restrict__ counter, uint64_t cap)
{
    __shared__ uint32_t s_slot[kExportStage];
    __shared__ unsigned long long s_val[kExportStage];
    __shared__ uint32_t s_n;
    __shared__ unsigned long long s_base;
    const uint64_t per = (n_slots + gridDim.x - 1) / gridDim.x;
    const uint64_t lo = (uint64_t)blockIdx.x * per;
    const uint64_t hi = lo + per < n_slots ? lo + per : n_slots;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    for (uint64_t base = lo; base < hi; base += kWG * 4) {     // uniform trip count per workgroup
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint64_t i = base + (uint64_t)u * kWG + threadIdx.x;
            const unsigned long long v = i < hi ? table[i] : 0ull;
            if (v) {
                const uint32_t at = atomicAdd(&s_n, 1u);         // LDS counter; stage holds 2048 >= 4 * 256
                s_slot[at] = slot_base + (uint32_t)i;
                s_val[at] = v;
            }
        }
        __syncthreads();
        const uint32_t n = s_n;
        if (n > kExportStage - kWG * 4 || base + kWG * 4 >= hi) {  // flush when the next round might overflow
            if (threadIdx.x == 0 && n) s_base = atomicAdd(counter, (unsigned long long)n);
            __syncthreads();
            for (uint32_t k = threadIdx.x; k < n; k += kWG)
                if (s_base + k < cap) {
                    out_slots[s_base + k] = s_slot[k];
                    out_vals[s_base + k] = s_val[k];
                }
            __syncthreads();
            if (threadIdx.x == 0) s_n = 0;
        }
        __syncthreads();
    }
}

// Merge foreign entries: table[slot] = max(table[slot], value), keeping the running alive count exact
// (same telescoping argument as kta_alive_update_counting).
__global__ __launch_bounds__(kWG) void kta_alive_import(const uint32_t *__restrict__ slots,
                                                        const unsigned long long *__restrict__ vals, uint64_t n,
                                                        unsigned long long *__restrict__ table,
                                                        long long *__restrict__ running, WrittenList wl)
{
    __shared__ long long s_w[kWG / 64];
    const uint64_t stride = (uint64_t)gridDim.x * kWG;
    long long delta = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kWG + threadIdx.x; i < n; i += stride) {
        const unsigned long long v = vals[i];
        if (!v) continue;
        const unsigned long long old = atomicMax(&table[slots[i]], v);
        note_new_slot(wl, old == 0ull, slots[i]);
        if (v > old) delta += (long long)(v & 1ull) - (long long)(old & 1ull);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) delta += __shfl_xor(delta, off);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = delta;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0;
        for (int w = 0; w < kWG / 64; w++) t += s_w[w];
        if (t) atomicAdd(reinterpret_cast<unsigned long long *>(running), (unsigned long long)t);
    }
}

// number of entries ever written (value != 0)
__global__ __launch_bounds__(kWG) void kta_alive_count_written(const ulonglong2 *__restrict__ table2, uint64_t n_pairs,
                                                               unsigned long long *out)
{
    __shared__ unsigned long long s_w[kWG / 64];
    const uint64_t stride = (uint64_t)gridDim.x * kWG;
    unsigned long long cnt = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kWG + threadIdx.x; i < n_pairs; i += stride) {
        const ulonglong2 e = table2[i];
        cnt += (e.x != 0ull) + (e.y != 0ull);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kWG / 64; w++) t += s_w[w];
        if (t) atomicAdd(out, t);
    }
}

// entries ever written in the slots [lo, hi) (any bounds)
__global__ __launch_bounds__(kWG) void kta_alive_count_written_span(const uint64_t *__restrict__ table, uint64_t lo,
                                                                    uint64_t hi, unsigned long long *out)
{
    __shared__ unsigned long long s_w[kWG / 64];
    const uint64_t stride = (uint64_t)gridDim.x * kWG;
    unsigned long long cnt = 0;
    for (uint64_t i = lo + (uint64_t)blockIdx.x * kWG + threadIdx.x; i < hi; i += stride) cnt += table[i] != 0ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kWG / 64; w++) t += s_w[w];
        if (t) atomicAdd(out, t);
    }
}

// table -> bitmap: one wave turns 64 consecutive entries into one u64 of bits via ballot.
__global__ __launch_bounds__(kWG) void kta_alive_bitmap(const unsigned long long *__restrict__ table,
                                                        uint64_t n_slots,
                                                        unsigned long long *__restrict__ bitmap64)
{
    const uint64_t stride = (uint64_t)gridDim.x * kWG;
    for (uint64_t i = (uint64_t)blockIdx.x * kWG + threadIdx.x; i < n_slots; i += stride) {
        const unsigned long long m = __ballot((table[i] & 1ull) != 0ull);
        if ((threadIdx.x & 63u) == 0u) bitmap64[i >> 6] = m;
    }
}

// ---------------------------------------------------------------------------------------
// launch wrappers
// ---------------------------------------------------------------------------------------

hipError_t launch_alive_update(const AliveColumns &c, uint64_t n, uint64_t base_seq, uint64_t *table,
                               int workgroups, int variant, uint32_t *scratch, int64_t *running, hipStream_t s,
                               const uint32_t *only_if, const WrittenList &wl)
{
    uint64_t wgs = (n + kWG - 1) / kWG;
    const uint64_t cap = workgroups > 0 ? (uint64_t)workgroups : 256ull * 8ull;
    if (wgs > cap) wgs = cap;
    if (wgs < 1) wgs = 1;
    unsigned long long *t = reinterpret_cast<unsigned long long *>(table);
    if (variant == 8 && scratch) {
        hipLaunchKernelGGL(kta_alive_hash_only, dim3((uint32_t)wgs), dim3(kWG), 0, s, c, n, scratch);
    } else if (variant == 9 && scratch) {
        hipLaunchKernelGGL(kta_alive_apply_only, dim3((uint32_t)wgs), dim3(kWG), 0, s, c, n, base_seq, scratch, t, wl);
    } else if (variant == 2 && running) {
        hipLaunchKernelGGL(kta_alive_update_filtered, dim3((uint32_t)wgs), dim3(kWG), 0, s, c, n, base_seq, t,
                           reinterpret_cast<long long *>(running), only_if, wl);
    } else if (variant == 1 && running) {
        hipLaunchKernelGGL(kta_alive_update_counting, dim3((uint32_t)wgs), dim3(kWG), 0, s, c, n, base_seq, t,
                           reinterpret_cast<long long *>(running), wl);
    } else {
        hipLaunchKernelGGL(kta_alive_update, dim3((uint32_t)wgs), dim3(kWG), 0, s, c, n, base_seq, t, wl);
    }
    return hipGetLastError();
}

hipError_t launch_alive_count(const uint64_t *table, uint64_t n_slots, uint64_t *out, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(out, 0, sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kta_alive_count, dim3(256 * 8), dim3(kWG), 0, s,
                       reinterpret_cast<const ulonglong2 *>(table), n_slots / 2,
                       reinterpret_cast<unsigned long long *>(out));
    return hipGetLastError();
}

hipError_t launch_alive_count_span(const uint64_t *table, uint64_t lo, uint64_t hi, uint64_t *out, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(out, 0, sizeof(uint64_t), s);
    if (e != hipSuccess || lo >= hi) return e;
    hipLaunchKernelGGL(kta_alive_count_span, dim3(256 * 8), dim3(kWG), 0, s, table, lo, hi,
                       reinterpret_cast<unsigned long long *>(out));
    return hipGetLastError();
}

hipError_t launch_alive_count_written_span(const uint64_t *table, uint64_t lo, uint64_t hi, uint64_t *out, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(out, 0, sizeof(uint64_t), s);
    if (e != hipSuccess || lo >= hi) return e;
    hipLaunchKernelGGL(kta_alive_count_written_span, dim3(256 * 8), dim3(kWG), 0, s, table, lo, hi,
                       reinterpret_cast<unsigned long long *>(out));
    return hipGetLastError();
}

hipError_t launch_alive_count_written(const uint64_t *table, uint64_t n_slots, uint64_t *out, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(out, 0, sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kta_alive_count_written, dim3(256 * 8), dim3(kWG), 0, s,
                       reinterpret_cast<const ulonglong2 *>(table), n_slots / 2,
                       reinterpret_cast<unsigned long long *>(out));
    return hipGetLastError();
}

hipError_t launch_alive_export(const uint64_t *table, uint64_t n_slots, uint32_t *out_slots, uint64_t *out_vals,
                               uint64_t *counter, uint64_t cap, hipStream_t s)
{
    return launch_alive_export_span(table, 0, n_slots, out_slots, out_vals, counter, cap, s);
}

hipError_t launch_alive_export_span(const uint64_t *table, uint64_t lo, uint64_t hi, uint32_t *out_slots,
                                    uint64_t *out_vals, uint64_t *counter, uint64_t cap, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(counter, 0, sizeof(uint64_t), s);
    if (e != hipSuccess || lo >= hi) return e;
    const uint64_t n_slots = hi - lo;
    hipLaunchKernelGGL(kta_alive_export, dim3(256 * 16), dim3(kWG), 0, s,
                       reinterpret_cast<const unsigned long long *>(table + lo), n_slots, (uint32_t)lo, out_slots,
                       reinterpret_cast<unsigned long long *>(out_vals),
                       reinterpret_cast<unsigned long long *>(counter), cap);
    return hipGetLastError();
}

hipError_t launch_alive_import(const uint32_t *slots, const uint64_t *vals, uint64_t n, uint64_t *table,
                               int64_t *running, const WrittenList &wl, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    uint64_t wgs = (n + kWG - 1) / kWG;
    if (wgs > 256 * 8) wgs = 256 * 8;
    hipLaunchKernelGGL(kta_alive_import, dim3((uint32_t)wgs), dim3(kWG), 0, s, slots,
                       reinterpret_cast<const unsigned long long *>(vals), n,
                       reinterpret_cast<unsigned long long *>(table), reinterpret_cast<long long *>(running), wl);
    return hipGetLastError();
}

// ---- the exchange over the written list -----------------------------------------------------------------
constexpr int kMaxOwners = 64;

// The list's length is read on the device (the host does not wait for it): a list that overflowed its capacity says so
// in *overflow, and the counts then cover its first `cap` entries only — the host, which reads the flag together with the
// counts, falls back to the sweeps.
__global__ __launch_bounds__(kWG) void kta_written_count(WrittenList wl, uint32_t nranks, unsigned long long *counts, unsigned long long *overflow)
{
    __shared__ uint32_t s_c[kMaxOwners];
    if (threadIdx.x < kMaxOwners) s_c[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t have = *wl.n, n = have < wl.cap ? have : wl.cap;
    if (blockIdx.x == 0 && threadIdx.x == 0 && have > wl.cap) *overflow = 1ull;
    for (uint64_t i = (uint64_t)blockIdx.x * kWG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kWG)
        atomicAdd(&s_c[(uint32_t)(((uint64_t)wl.slots[i] * nranks) >> 32)], 1u);
    __syncthreads();
    if (threadIdx.x < nranks && s_c[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)s_c[threadIdx.x]);
}

// Every workgroup takes a contiguous piece of the list, counts its entries per owner in LDS, reserves their places
// in the owners' lists with ONE device atomic per owner, and writes (slot, table[slot]).
__global__ __launch_bounds__(kWG) void kta_written_export(WrittenList wl, const unsigned long long *__restrict__ table,
                                                          uint32_t nranks, uint32_t skip_rank,
                                                          const unsigned long long *__restrict__ owner_at,
                                                          unsigned long long *__restrict__ cursors, uint32_t *__restrict__ out_slots,
                                                          unsigned long long *__restrict__ out_vals)
{
    __shared__ uint32_t s_c[kMaxOwners];
    __shared__ unsigned long long s_base[kMaxOwners];
    const uint64_t have = *wl.n, n = have < wl.cap ? have : wl.cap;     // (the length is read on the device, as in kta_written_count)
    const uint64_t per = (n + gridDim.x - 1) / gridDim.x;
    const uint64_t lo = (uint64_t)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    constexpr uint64_t kChunk = (uint64_t)kWG * 8;
    for (uint64_t c0 = lo; c0 < hi; c0 += kChunk) {                    // uniform trip count per workgroup
        if (threadIdx.x < kMaxOwners) s_c[threadIdx.x] = 0;
        __syncthreads();
        uint32_t slot[8], own[8], at[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint64_t i = c0 + (uint64_t)u * kWG + threadIdx.x;
            slot[u] = i < hi ? wl.slots[i] : 0u;
            own[u] = i < hi ? (uint32_t)(((uint64_t)slot[u] * nranks) >> 32) : skip_rank;
            at[u] = own[u] != skip_rank ? atomicAdd(&s_c[own[u]], 1u) : 0u;
        }
        __syncthreads();
        if (threadIdx.x < nranks && s_c[threadIdx.x]) s_base[threadIdx.x] = atomicAdd(&cursors[threadIdx.x], (unsigned long long)s_c[threadIdx.x]);
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (own[u] == skip_rank) continue;
            const unsigned long long k = owner_at[own[u]] + s_base[own[u]] + at[u];
            out_slots[k] = slot[u];
            out_vals[k] = table[slot[u]];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kWG) void kta_written_alive_count(WrittenList wl, const unsigned long long *__restrict__ table,
                                                               uint64_t lo, uint64_t hi, unsigned long long *out)
{
    __shared__ unsigned long long s_w[kWG / 64];
    unsigned long long cnt = 0;
    const uint64_t len = *wl.n;                           // (may have grown by the import that ran just before)
    if (len > wl.cap) return;                             // the list is not complete: kta_alive_count_span_if_overflowed counts
    for (uint64_t i = (uint64_t)blockIdx.x * kWG + threadIdx.x; i < len; i += (uint64_t)gridDim.x * kWG) {
        const uint64_t slot = wl.slots[i];
        if (slot >= lo && slot < hi) cnt += table[slot] & 1ull;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kWG / 64; w++) t += s_w[w];
        if (t) atomicAdd(out, t);
    }
}

hipError_t launch_written_count(const WrittenList &wl, int nranks, uint64_t *counts, uint64_t *overflow, hipStream_t s)
{
    // (one LDS counter per owner: kta_comm.hip takes the sweeps — launch_alive_count_written_span / _export_span — for more
    // than kMaxOwners ranks and never comes here with them)
    if (nranks > kMaxOwners) return hipErrorInvalidValue;
    // (the grid does not depend on the list's length, which only the device knows: 4 workgroups per CU walk it)
    hipLaunchKernelGGL(kta_written_count, dim3(1024), dim3(kWG), 0, s, wl, (uint32_t)nranks,
                       reinterpret_cast<unsigned long long *>(counts), reinterpret_cast<unsigned long long *>(overflow));
    return hipGetLastError();
}

hipError_t launch_written_export(const WrittenList &wl, const uint64_t *table, int nranks, int skip_rank,
                                 const uint64_t *owner_at, uint64_t *cursors, uint32_t *out_slots, uint64_t *out_vals, hipStream_t s)
{
    if (nranks > kMaxOwners) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kta_written_export, dim3(1024), dim3(kWG), 0, s, wl, reinterpret_cast<const unsigned long long *>(table),
                       (uint32_t)nranks, (uint32_t)skip_rank, reinterpret_cast<const unsigned long long *>(owner_at),
                       reinterpret_cast<unsigned long long *>(cursors), out_slots, reinterpret_cast<unsigned long long *>(out_vals));
    return hipGetLastError();
}

// The owner's count of its hash range over the written list — or, when the list has overflowed by now (the import may
// have added to it; only the device knows), over the range itself: both kernels are launched, one of them returns at once.
hipError_t launch_written_alive_count(const WrittenList &wl, const uint64_t *table, uint64_t lo, uint64_t hi,
                                      uint64_t *out, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(out, 0, sizeof(uint64_t), s);
    if (e != hipSuccess || lo >= hi) return e;
    hipLaunchKernelGGL(kta_written_alive_count, dim3(1024), dim3(kWG), 0, s, wl,
                       reinterpret_cast<const unsigned long long *>(table), lo, hi, reinterpret_cast<unsigned long long *>(out));
    hipLaunchKernelGGL(kta_alive_count_span_if_overflowed, dim3(256 * 8), dim3(kWG), 0, s, wl, table, lo, hi,
                       reinterpret_cast<unsigned long long *>(out));
    return hipGetLastError();
}

hipError_t launch_alive_bitmap(const uint64_t *table, uint64_t n_slots, uint32_t *bitmap, hipStream_t s)
{
    hipLaunchKernelGGL(kta_alive_bitmap, dim3(256 * 8), dim3(kWG), 0, s,
                       reinterpret_cast<const unsigned long long *>(table), n_slots,
                       reinterpret_cast<unsigned long long *>(bitmap));
    return hipGetLastError();
}

hipError_t launch_fnv32(const uint8_t *key_bytes, const uint32_t *key_off, const int32_t *key_len,
                        uint64_t n, uint32_t *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(kta_fnv32, dim3((uint32_t)((n + kWG - 1) / kWG)), dim3(kWG), 0, s, key_bytes,
                       key_off, key_len, n, out);
    return hipGetLastError();
}

} // namespace kta

// kta_record_batches.hip — the record-batch section (KTA_FLAG_RECORD_BATCHES, include/kta_hip.h): what the batch headers of
// a decode call say, accumulated into the section's live vector.  The rule, the vector's layout and the counted-batch
// predicate are kta_record_batches.h's.  No reference counterpart.
//
//   kta_record_batches   One lane per batch, 256-thread workgroups, a grid-stride loop over at most two workgroups per CU
//                     (so the flush below is bounded by the grid, not by the batches).  A lane loads its 88-byte descriptor
//                     and the header bytes 12..50 of its batch one by one — byte_off has no alignment — and forms the
//                     batch's RbBatch in registers.
//                     Codec words: u64[500] in LDS, seven ds_add_u64 per batch.  Producer sketch: u32[1024] in LDS, one
//                     ds_max_u32 per idempotent batch.  Partition words: when the counted lanes of a wave instruction all
//                     hold one partition (a ballot; the normal case, a blob is one partition), the 13 sums and 4 maxima are
//                     reduced across the wave with __shfl_xor and lanes 0..12 and 16..19 issue one device atomic each on
//                     consecutive words; otherwise every counted lane issues its own.  Integer adds and maxima commute: the
//                     vector is bit-exact whatever the schedule.  At the end the workgroup adds its non-zero LDS words to the
//                     vector (atomicAdd / atomicMax on u64).
#include <hip/hip_runtime.h>

#include "kta_internal.h"
#include "kta_record_batches.h"

namespace kta {

namespace {

constexpr uint32_t kRbThreads = 256;

__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, m, 64);
    return v;
}
__device__ __forceinline__ uint64_t wave_max(uint64_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(kRbThreads) void kta_record_batches(const kta_kafka_batch_desc *descs, uint64_t n, const uint8_t *blob,
                                                                 uint64_t blob_len, uint32_t P, RbFilter f, unsigned long long *vec)
{
    __shared__ unsigned long long s_codec[kRbCodecTable];
    __shared__ uint32_t s_regs[kRbSketchRegs];
    for (uint32_t e = threadIdx.x; e < kRbCodecTable; e += kRbThreads) s_codec[e] = 0ull;
    for (uint32_t e = threadIdx.x; e < kRbSketchRegs; e += kRbThreads) s_regs[e] = 0u;
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * kRbThreads;
    // (the loop's bound is wave-uniform: every lane of a wave runs the same iterations, so the ballots and shuffles below
    // see the whole wave; a lane past the end holds no batch)
    const uint64_t wave0 = (uint64_t)blockIdx.x * kRbThreads + (threadIdx.x & ~63u);
    for (uint64_t w = wave0; w < n; w += stride) {
        const uint64_t i = w + lane;
        bool counted = false;
        int32_t partition = -1;
        RbBatch b = rb_failed_batch();
        if (i < n) {
            const kta_kafka_batch_desc d = descs[i];
            partition = d.partition;
            counted = rb_counted(f, P, d.partition, d.base_ts_ms, d.max_ts_ms);
            if (counted && d.status == 0 && rb_header_inside(d.byte_off, blob_len)) b = rb_batch(d, rb_fields(blob + d.byte_off));
        }
        if (counted && !b.failed) {
            unsigned long long *cw = s_codec + b.codec * kRbCodecWords;
            atomicAdd(cw + kRbCodecBatches, 1ull);
            atomicAdd(cw + kRbCodecRecords, (unsigned long long)b.sums[kRbRecords]);
            atomicAdd(cw + kRbCodecRecbytes, (unsigned long long)b.recbytes);
            atomicAdd(cw + kRbCodecPayload, (unsigned long long)b.sums[kRbPayload]);
            atomicAdd(cw + kRbCodecHistRecords + rb_bin(b.sums[kRbRecords]), 1ull);
            atomicAdd(cw + kRbCodecHistWire + rb_bin(b.sums[kRbWire]), 1ull);
            atomicAdd(cw + kRbCodecHistSpan + rb_bin(b.sums[kRbSpanMs]), 1ull);
            if (b.idempotent) atomicMax(s_regs + b.reg, b.rank);
        }
        const unsigned long long m = __ballot(counted);
        if (m == 0ull) continue;                                 // (uniform)
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
        const int32_t p0 = __builtin_amdgcn_readlane(partition, leader);
        if (__ballot(counted && partition != p0) == 0ull) {      // (uniform) one partition: reduce, then one atomic per word
            uint64_t mine = 0;
#pragma unroll
            for (uint32_t k = 0; k < kRbPartitionSums; k++) {
                const uint64_t t = wave_sum(counted ? b.sums[k] : 0ull);
                if (lane == k) mine = t;
            }
#pragma unroll
            for (uint32_t k = 0; k < kRbMaxWords; k++) {
                const uint64_t t = wave_max(counted ? b.maxima[k] : 0ull);
                if (lane == 16u + k) mine = t;
            }
            if (mine) {
                if (lane < kRbPartitionSums) atomicAdd(vec + (size_t)kRbPartitionWords * (uint32_t)p0 + lane, (unsigned long long)mine);
                else atomicMax(vec + rb_max_at(P, (uint32_t)p0) + (lane - 16u), (unsigned long long)mine);
            }
        } else if (counted) {                                    // mixed partitions (rare): the lane's own atomics
            unsigned long long *pw = vec + (size_t)kRbPartitionWords * (uint32_t)partition;
#pragma unroll
            for (uint32_t k = 0; k < kRbPartitionSums; k++)
                if (b.sums[k]) atomicAdd(pw + k, (unsigned long long)b.sums[k]);
            unsigned long long *mw = vec + rb_max_at(P, (uint32_t)partition);
#pragma unroll
            for (uint32_t k = 0; k < kRbMaxWords; k++)
                if (b.maxima[k]) atomicMax(mw + k, (unsigned long long)b.maxima[k]);
        }
    }
    __syncthreads();
    unsigned long long *codecs = vec + rb_codec_at(P, 0), *regs = vec + rb_sketch_at(P);
    for (uint32_t e = threadIdx.x; e < kRbCodecTable; e += kRbThreads) {
        const unsigned long long v = s_codec[e];
        if (v) atomicAdd(codecs + e, v);
    }
    for (uint32_t e = threadIdx.x; e < kRbSketchRegs; e += kRbThreads) {
        const uint32_t v = s_regs[e];
        if (v) atomicMax(regs + e, (unsigned long long)v);
    }
}

} // namespace

hipError_t launch_record_batches(const BlobPassArgs &a, uint32_t *workgroups, hipStream_t s)
{
    const uint64_t n = a.n;
    *workgroups = 0;
    if (n == 0) return hipSuccess;
    if (!a.descs || !a.blob || !a.vec || a.P == 0) return hipErrorInvalidValue;
    const uint64_t want = (n + kRbThreads - 1) / kRbThreads;
    const uint64_t cap = 2ull * (uint64_t)(a.cu_count > 0 ? a.cu_count : 256);
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    hipLaunchKernelGGL(kta_record_batches, dim3(grid), dim3(kRbThreads), 0, s, a.descs, n, a.blob, a.blob_len, a.P,
                       RbFilter{a.from_ms, a.to_ms, a.bitmap}, reinterpret_cast<unsigned long long *>(a.vec));
    *workgroups = grid;
    return hipGetLastError();
}

} // namespace kta

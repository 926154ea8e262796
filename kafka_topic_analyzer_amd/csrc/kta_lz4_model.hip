// kta_lz4_model.hip — the compression what-if (KTA_FLAG_COMPRESS_WHATIF, include/kta_hip.h): the bytes a defined LZ4
// compressor would leave of every batch's records section, per partition and by the batch's current codec, accumulated into
// the section's live vector.  The compressor, the frame, the vector's layout and the identities are kta_lz4_model.h's; which
// batches count is kta_record_batches.h's rb_counted and the descriptor's status.  No reference counterpart.
//
//   kta_lz4_model A wave is a workgroup and takes every grid-th batch, of those the counted ones, and a batch's blocks of at
//                 most 65536 bytes one after the other.  The table T[4096] lies in LDS, 16 KiB a wave; an entry is
//                 epoch << 16 | position and one of another epoch reads as the zero a block begins with, so nothing is
//                 cleared between blocks (a batch of 2 KiB would clear 16 KiB); after 65535 blocks the table is zeroed.
//                 STRIDE: lane l takes position i + l — an unaligned dword from the blob, the hash, the entry, the
//                 candidate's dword, and where they agree a short extension of its own, dword by dword (kCwLaneSteps).  A
//                 ballot gives the hits; the greedy walk runs over the mask in scalar registers, reading the chosen lane's
//                 candidate and length; a match that reached the lane's cap goes on with the whole wave, 64 lanes by 4 bytes
//                 a step.  Then every lane inserts its position with an LDS atomicMax, and a barrier parts the stride from
//                 the next one's lookups.  The lookups of a stride see the table as it stood before it, and the highest
//                 position of a hash wins: the sizes are lz4m_block's whatever the lanes' order.
//                 The words of the wave's partition and codec are held in registers, every lane alike, and go to the vector
//                 with 64-bit atomics, a lane a word, when either changes and at the end.  The grid is at most eight
//                 workgroups per CU.  Integer adds commute: the vector is bit-exact whatever the schedule.
#include <hip/hip_runtime.h>

#include "kta_internal.h"
#include "kta_kafka.h"
#include "kta_lz4_model.h"
#include "kta_record_batches.h"

#ifndef KTA_WAVES_PER_EU
#define KTA_WAVES_PER_EU(least, most) __attribute__((amdgpu_waves_per_eu(least, most)))
#endif

namespace kta {

namespace {

#include "kta_lz4_model_kernel.h"

} // namespace

hipError_t launch_lz4_model(const BlobPassArgs &a, uint32_t *workgroups, hipStream_t s)
{
    const uint64_t n = a.n;
    *workgroups = 0;
    if (n == 0) return hipSuccess;
    if (!a.descs || !a.blob || !a.vec || a.P == 0) return hipErrorInvalidValue;
    // as many workgroups as are resident at once, each over every grid-th batch: the flushes are bounded by the grid and
    // the partitions' changes, not by the batches
    const uint64_t cap = kCwWavesPerCu * (uint64_t)(a.cu_count > 0 ? a.cu_count : 256);
    const uint32_t grid = (uint32_t)(n < cap ? n : cap);
    hipLaunchKernelGGL(kta_lz4_model<kCwEpochs>, dim3(grid), dim3(64), 0, s, a.blob, a.descs, n, a.P, RbFilter{a.from_ms, a.to_ms, a.bitmap},
                       reinterpret_cast<unsigned long long *>(a.vec), grid);
    *workgroups = grid;
    return hipGetLastError();
}

} // namespace kta

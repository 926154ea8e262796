// kta_payload.hip — the payload section (KTA_FLAG_PAYLOAD, include/kta_hip.h): the value classes, schema-registry ids and
// record headers of the records of a decode call, accumulated into the section's live vector.  The rule, the vector's
// layout and the header walk are kta_payload.h's.  No reference counterpart.
//
//   kta_payload   The decode kernel's shape (kta_decode_coop.h, <4, 3 KiB, 16>): a wave is a workgroup and takes four
//                 batches, sixteen lanes each.  A window of the batch goes through LDS (a KiB per wave instruction,
//                 non-temporal), the group's first lane chains the length prefixes (kta::rec::chain), the lanes parse a
//                 record each (kta::rec::parse_record).  New per lane: the value's first five bytes from the window when
//                 they lie inside it, else from global memory; a record whose header section is the one byte 0 inside the
//                 window is done; a record inside the window has its headers walked in LDS, any other in global memory
//                 through a cached 16-byte block, bounded by the record's end (payload_walk_headers over two byte
//                 sources).  Nothing is stored per record.
//                 A round COMMITS the records in front of its first incomplete and its first bad record, so a batch
//                 counts up to its first record with bad framing, as the host statement does.
//                 The grid is at most twelve workgroups per CU; a workgroup takes every grid-th four batches.
//                 Accumulation: the partition words in registers per lane, for one partition at a time; when the partition
//                 changes and at the workgroup's end they are summed over the wave (over each group when the wave holds
//                 several partitions) with __shfl_xor and added with one device atomicAdd per non-zero word.  The histogram:
//                 bin 0 in a register, the others in LDS per group (u32[16]), added at the end.  The schema-id table: a lane
//                 keeps one id with its records and bytes in registers; a record with another id hands the old one over, the
//                 wave loops over the DISTINCT ids handed over (first pending lane, a ballot of the lanes with its id) into
//                 a sixteen-slot id cache in LDS, and a slot goes to the table — lanes 0..33 add T, B and T for every set bit
//                 of the id, once per row: one add per touched word — when another id needs it and at the end.  Integer adds
//                 commute: the vector is bit-exact whatever the schedule.
#include <hip/hip_runtime.h>

#include "kta_filter.h"
#include "kta_internal.h"
#include "kta_kafka.h"
#include "kta_payload.h"
#include "kta_records.h"

namespace kta {

namespace {

#include "kta_decode_coop.h"   // pin, load_block, KTA_READLANE (the decode kernel itself is not instantiated here)
#include "kta_payload_kernel.h"

} // namespace

hipError_t launch_payload(const BlobPassArgs &a, uint32_t *workgroups, hipStream_t s)
{
    const uint64_t n = a.n;
    const uint32_t P = a.P;
    *workgroups = 0;
    if (n == 0) return hipSuccess;
    if (!a.descs || !a.blob || !a.vec || P == 0 || ((uintptr_t)a.blob & 15u)) return hipErrorInvalidValue;
    // as many workgroups as are resident at once (12 waves per CU: 142 registers, 12.9 KiB of LDS), each over every grid-th four
    // batches: the flushes at a workgroup's end are bounded by the grid, not by the batches
    const uint64_t want = (n + kPlG - 1) / kPlG, cap = kPlWavesPerCu * (uint64_t)(a.cu_count > 0 ? a.cu_count : 256);
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    hipLaunchKernelGGL(kta_payload, dim3(grid), dim3(64), 0, s, reinterpret_cast<const uint4 *>(a.blob), a.descs, n, P,
                       FilterSpec{a.from_ms, a.to_ms, P, a.bitmap ? 1u : 0u}, a.bitmap, reinterpret_cast<unsigned long long *>(a.vec), grid);
    *workgroups = grid;
    return hipGetLastError();
}

} // namespace kta

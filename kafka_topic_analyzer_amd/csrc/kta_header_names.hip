// kta_header_names.hip — the header-name section (KTA_FLAG_HEADER_NAMES, include/kta_hip.h): a census of the header names of
// the records of a decode call, accumulated into the section's live vector and its name table.  The rule, the vector's
// layout and the read-off are kta_header_names.h's; which records count, the header grammar and the cell mapping are
// kta_payload.h's.  No reference counterpart.
//
//   kta_header_names   The decode kernel's shape (kta_decode_coop.h, <4, 3 KiB, 16>), as kta_payload has it: a wave is a
//                 workgroup and takes four batches, sixteen lanes each; a window of the batch goes through LDS, the group's
//                 first lane chains the length prefixes (kta::rec::chain), the lanes parse a record each
//                 (kta::rec::parse_record).  A round has three steps between barriers.
//                 VALIDATE: a lane walks its record's header section with payload_walk_headers — in LDS when the record lies
//                 inside the window, else in global memory through a cached 16-byte block — and keeps good / bad, the count
//                 and where the section lies; a section that is the one byte 0 inside the window is done.
//                 COMMIT: the round commits the records in front of its first incomplete and its first bad record; records
//                 at or behind the first incomplete one are redone next round, those at or behind the first bad one dropped.
//                 VISIT: a lane whose record is committed and whose section was good walks it a second time with
//                 payload_visit_headers over the same byte source and emits every occurrence: the name's FNV chain byte by
//                 byte, then the workgroup's cache of 64 names in LDS, keyed by hash — the slot (six bits of fmix32 that row 1's
//                 cell does not use) is claimed with a 64-bit compare-and-swap of 2^32 | hash, and T, L, V, Z are added with LDS
//                 atomics by whichever lanes hold that name.  A lane that finds the slot held by another hash adds the
//                 occurrence straight to the table's two cells (up to 2 x 36 device atomics): exact either way.  The lane
//                 that claims a slot (and a lane that spills) tries the name slots of its two cells: compare-and-swap on
//                 `state`, the fields with plain stores, a fence, then `state` published.
//                 The cache goes to the table at the workgroup's end, and before a lane has put 2^24 occurrences into it
//                 (64 lanes: a slot's 32-bit T and Z stay below 2^31; a single record of 2^24 headers goes past the cache):
//                 a lane per word, T for every set bit of the hash, once per row.  The six globals are kept in registers,
//                 summed over the wave and added once.  The grid is at most ten workgroups per CU; a workgroup takes every
//                 grid-th four batches, so the flushes are bounded by the grid.  Integer adds commute: the vector is
//                 bit-exact whatever the schedule; which occurrence's bytes a name slot holds is not.
#include <hip/hip_runtime.h>

#include "kta_filter.h"
#include "kta_fnv.h"
#include "kta_header_names.h"
#include "kta_internal.h"
#include "kta_kafka.h"
#include "kta_records.h"

namespace kta {

namespace {

static_assert(kHnFnvInit == kFnvInit && kHnFnvMul == kFnvMul, "the name hash is the -c hash: kta_header_names.h and kta_fnv.h");

#include "kta_decode_coop.h"   // pin, load_block, KTA_READLANE (the decode kernel itself is not instantiated here)
#include "kta_header_names_kernel.h"

} // namespace

hipError_t launch_header_names(const BlobPassArgs &a, uint32_t *workgroups, hipStream_t s)
{
    const uint64_t n = a.n;
    const uint32_t P = a.P;
    *workgroups = 0;
    if (n == 0) return hipSuccess;
    if (!a.descs || !a.blob || !a.vec || !a.names || !a.info || P == 0 || ((uintptr_t)a.blob & 15u)) return hipErrorInvalidValue;
    // as many workgroups as are resident at once, each over every grid-th four batches: the flushes at a workgroup's end are
    // bounded by the grid, not by the batches
    const uint64_t want = (n + kHnG - 1) / kHnG, cap = kHnWavesPerCu * (uint64_t)(a.cu_count > 0 ? a.cu_count : 256);
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    hipLaunchKernelGGL(kta_header_names, dim3(grid), dim3(64), 0, s, reinterpret_cast<const uint4 *>(a.blob), a.descs, n, P,
                       FilterSpec{a.from_ms, a.to_ms, P, a.bitmap ? 1u : 0u}, a.bitmap, reinterpret_cast<unsigned long long *>(a.vec),
                       static_cast<HnSlot *>(a.names), reinterpret_cast<unsigned long long *>(a.info), grid);
    *workgroups = grid;
    return hipGetLastError();
}

} // namespace kta

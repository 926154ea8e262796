// kta_value_bytes.hip — the value-byte section (KTA_FLAG_VALUE_BYTES, include/kta_hip.h): a histogram of the bytes of the
// values of the records of a decode call, per partition, accumulated into the section's live vector.  The rule, the vector's
// layout and the read-off are kta_value_bytes.h's; which records count and the record grammar are kta_payload.h's and
// kta_records.h's.  No reference counterpart.
//
//   kta_value_bytes   The decode kernel's shape (kta_decode_coop.h, <4, 3 KiB, 16>), as kta_payload has it: a wave is a
//                 workgroup and takes four batches, sixteen lanes each; a window of the batch goes through LDS, the group's
//                 first lane chains the length prefixes (kta::rec::chain), the lanes parse a record each
//                 (kta::rec::parse_record) and keep where its value begins and how long it is.
//                 COMMIT: the round commits the records in front of its first incomplete and its first bad record; records
//                 at or behind the first incomplete one are redone next round, those at or behind the first bad one dropped.
//                 The lane of a committed record counts it in registers (records, values, bytes) and hands its value to the
//                 group through LDS.
//                 VALUES: the group's committed values are taken one after the other, the same step of the loop in all four
//                 groups.  The sixteen lanes of the group read what lies inside the window in dwords from LDS, a lane per
//                 dword, and what lies behind the window in 16-byte blocks from the blob, a lane per block — a value of 1 MiB
//                 too; no lane walks a value byte by byte.  A byte is one LDS atomic add to the group's 256 32-bit bins; a
//                 dword of four equal bytes is one add of 4 (kVbCombineDword: values of one byte send every lane to one LDS
//                 address; measured, DESIGN §3.5n: all zero over random costs 3.4 x with every byte its own add, 1.15 x so;
//                 the form that combines whichever bytes of a dword are equal costs 0.3 ms on every law and is kept, with
//                 the plain one, for tools/bench_value_bytes.py alone).  A repeat compares a byte with the one
//                 in front of it: inside the dword, else the last byte of the dword in front, read from where the dword was
//                 read (LDS or the blob) — never a byte in front of the value's first.  Repeats are kept in registers.
//                 FLUSH: the bins and the registers go to the vector with 64-bit atomics when a group's partition changes,
//                 before a group has put more than FLUSH bytes into its bins (a bin could take them all: FLUSH = 2^31 keeps a
//                 32-bit bin from wrapping; a longer value is taken in slices of FLUSH bytes) and at the kernel's end.  When
//                 the four groups hold one partition their bins are summed first: 256 + 4 adds a workgroup.  The grid is at
//                 most eight workgroups per CU; a workgroup takes every grid-th four batches, so the flushes are bounded
//                 by the grid.  Integer adds commute: the vector is bit-exact whatever the schedule.
#include <hip/hip_runtime.h>

#include "kta_filter.h"
#include "kta_internal.h"
#include "kta_kafka.h"
#include "kta_records.h"
#include "kta_value_bytes.h"

namespace kta {

namespace {

#include "kta_decode_coop.h"   // pin, load_block, KTA_READLANE (the decode kernel itself is not instantiated here)
#include "kta_value_bytes_kernel.h"

} // namespace

hipError_t launch_value_bytes(const BlobPassArgs &a, uint32_t *workgroups, hipStream_t s)
{
    const kta_kafka_batch_desc *descs = a.descs;
    const uint64_t n = a.n;
    const uint32_t P = a.P, *bitmap = a.bitmap;
    const int variant = a.variant;
    *workgroups = 0;
    if (n == 0) return hipSuccess;
    if (!descs || !a.blob || !a.vec || !a.info || P == 0 || ((uintptr_t)a.blob & 15u)) return hipErrorInvalidValue;
    // as many workgroups as are resident at once, each over every grid-th four batches: the flushes at a workgroup's end are
    // bounded by the grid, not by the batches
    const uint64_t want = (n + kVbG - 1) / kVbG, cap = kVbWavesPerCu * (uint64_t)(a.cu_count > 0 ? a.cu_count : 256);
    const uint32_t grid = (uint32_t)(want < cap ? want : cap);
    const FilterSpec spec{a.from_ms, a.to_ms, P, bitmap ? 1u : 0u};
    const uint4 *blocks = reinterpret_cast<const uint4 *>(a.blob);
    unsigned long long *v = reinterpret_cast<unsigned long long *>(a.vec), *work = reinterpret_cast<unsigned long long *>(a.info);
    if (variant == 1)                           // tools/bench_value_bytes.py's A/B switches: every byte its own LDS add
        hipLaunchKernelGGL((kta_value_bytes<kVbFlushBytes, kVbCombineNone>), dim3(grid), dim3(64), 0, s, blocks, descs, n, P, spec, bitmap, v, work, grid);
    else if (variant == 2)                      // ... equal bytes of a dword added once, whichever they are
        hipLaunchKernelGGL((kta_value_bytes<kVbFlushBytes, kVbCombinePairs>), dim3(grid), dim3(64), 0, s, blocks, descs, n, P, spec, bitmap, v, work, grid);
    else
        hipLaunchKernelGGL((kta_value_bytes<kVbFlushBytes, kVbCombineDword>), dim3(grid), dim3(64), 0, s, blocks, descs, n, P, spec, bitmap, v, work, grid);
    *workgroups = grid;
    return hipGetLastError();
}

} // namespace kta

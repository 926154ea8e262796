// lz4_model_emu.cpp — test infrastructure: kta_lz4_model (csrc/kta_lz4_model_kernel.h, the kernel's own source) compiled for
// the host over tests/native/wave_emu.h and run workgroup by workgroup, 64 lanes as fibers.  A program of its own
// (tests/test_lz4_model_emu.py builds and runs it): it reads a case file, runs the kernel and writes the vector, and beside
// it the vector the host statement (kta_lz4_model.h: compress_whatif_add over the same descriptors) gives.
//
// The blob is handed to the kernel as the device sees it — 64 readable bytes behind its end, poisoned — between two pages
// without access: a read outside [0, padded length) ends the program with a signal.  The vector lies in front of such a page
// as well, so an add behind its end does too.
//
// Case file: as tests/native/value_bytes_emu.cpp's.  Output file: the kernel's vector u64[8 P + 20] | the host statement's.
// A third argument: the grid (workgroups; default and at most one per batch).  The kernel is instantiated with kEmuEpochs
// tags, so that a workgroup's table runs out of them, and is zeroed, on inputs of a few blocks.
#include "wave_emu.h"

#include <sys/mman.h>
#include <unistd.h>

#include "../../include/kta_kafka.h"
#include "kta_lz4_model.h"
#include "kta_record_batches.h"

// one OS thread: the atomic that wave_emu.h does not have is a plain operation as well
static inline uint32_t atomicMax(uint32_t *p, uint32_t v)
{
    const uint32_t old = *p;
    if (v > old) *p = v;
    return old;
}

constexpr uint32_t kEmuEpochs = 4;   // the tags 1, 2, 3: the fourth block of a workgroup begins with a zeroed table

namespace kta {
namespace {
#include "kta_lz4_model_kernel.h"
}
}

// `bytes` bytes that end at a page without access (and begin behind one when `front`)
static uint8_t *guarded(size_t bytes, bool front)
{
    const size_t page = (size_t)sysconf(_SC_PAGESIZE), body = (bytes + page - 1) / page * page;
    uint8_t *m = (uint8_t *)mmap(nullptr, body + 2 * page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m == MAP_FAILED) return nullptr;
    mprotect(m, page, PROT_NONE);
    mprotect(m + page + body, page, PROT_NONE);
    return front && bytes % page == 0 ? m + page : m + page + body - bytes;
}

int main(int argc, char **argv)
{
    if (argc < 3 || argc > 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t n_batches = 0, blob_len = 0;
    uint32_t P = 0, order = 0, seed = 0, parts = 0;
    int64_t from_ms = 0, to_ms = 0;
    bool ok = fread(&n_batches, 8, 1, f) == 1 && fread(&blob_len, 8, 1, f) == 1 && fread(&P, 4, 1, f) == 1 && fread(&order, 4, 1, f) == 1 &&
              fread(&seed, 4, 1, f) == 1 && fread(&parts, 4, 1, f) == 1 && fread(&from_ms, 8, 1, f) == 1 && fread(&to_ms, 8, 1, f) == 1;
    if (!ok || P == 0 || P > 4096) return 2;
    std::vector<uint32_t> bitmap((P + 31) / 32);
    std::vector<kta_kafka_batch_desc> descs(n_batches);
    ok = fread(bitmap.data(), 4, bitmap.size(), f) == bitmap.size() && fread(descs.data(), sizeof(kta_kafka_batch_desc), n_batches, f) == n_batches;
    const size_t padded = blob_len + 64;
    uint8_t *blob = guarded(padded, false);
    if (!ok || !blob) return 2;
    memset(blob, 0xA5, padded);
    if (fread(blob, 1, blob_len, f) != blob_len) return 2;
    fclose(f);
    const size_t words = kta::compress_whatif_len(P);
    unsigned long long *vec = (unsigned long long *)guarded(words * 8, false);
    if (!vec) return 2;
    memset(vec, 0, words * 8);
    const uint32_t asked = argc >= 4 ? (uint32_t)atoi(argv[3]) : 0u;
    const uint32_t grid = asked > 0 && asked < n_batches ? asked : (uint32_t)(n_batches ? n_batches : 1);   // fewer: a workgroup takes several
    const kta::RbFilter filter{from_ms, to_ms, parts ? bitmap.data() : nullptr};
    const char *err = wave_emu::launch(grid, (int)order, seed, [&] { kta::kta_lz4_model<kEmuEpochs>(blob, descs.data(), n_batches, P, filter, vec, grid); });
    if (err) {
        fprintf(stderr, "%s\n", err);
        return 3;
    }
    // the host statement over the same descriptors
    std::vector<uint64_t> want(words, 0);
    for (const kta_kafka_batch_desc &d : descs) {
        if (d.status != 0 || !kta::rb_counted(filter, P, d.partition, d.base_ts_ms, d.max_ts_ms)) continue;
        kta::compress_whatif_add(want.data(), P, (uint32_t)d.partition, kta::compress_whatif_codec(d.flags), d.batch_bytes, blob + d.payload_off,
                                 d.payload_end > d.payload_off ? d.payload_end - d.payload_off : 0);
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(vec, 8, words, f) != words || fwrite(want.data(), 8, words, f) != words) return 2;
    fclose(f);
    printf("OK %u workgroups\n", grid);
    return 0;
}

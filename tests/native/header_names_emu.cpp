// header_names_emu.cpp — test infrastructure: kta_header_names (csrc/kta_header_names_kernel.h, the kernel's own source)
// compiled for the host over tests/native/wave_emu.h and run workgroup by workgroup, 64 lanes as fibers.  A program of its
// own (tests/test_header_names_emu.py builds and runs it): it reads a case file, runs the kernel and writes the vector, the
// name table and the work counters.
//
// The blob is handed to the kernel as the device sees it — 16-byte aligned, 64 readable bytes behind its end, poisoned —
// between two pages without access: a read outside [0, padded length) ends the program with a signal.  The vector and the
// name table lie in front of such a page as well, so an add or a store behind their ends does too.
//
// Case file: as tests/native/payload_emu.cpp's.  Output file: the vector u64[73736] | the name table [2048][64 bytes] |
// u64[4] work counters.  A third argument: the grid (workgroups; default and at most one per four batches).
#include "wave_emu.h"

#include <sys/mman.h>
#include <unistd.h>

#include "../../include/kta_kafka.h"
#include "kta_filter.h"
#include "kta_header_names.h"
#include "kta_records.h"

// one OS thread: the atomics that wave_emu.h does not have are plain operations as well
static inline uint32_t atomicAdd(uint32_t *p, uint32_t v)
{
    const uint32_t old = *p;
    *p = old + v;
    return old;
}
static inline unsigned long long atomicCAS(unsigned long long *p, unsigned long long expect, unsigned long long v)
{
    const unsigned long long old = *p;
    if (old == expect) *p = v;
    return old;
}
static inline uint32_t atomicCAS(uint32_t *p, uint32_t expect, uint32_t v)
{
    const uint32_t old = *p;
    if (old == expect) *p = v;
    return old;
}
static inline uint32_t atomicExch(uint32_t *p, uint32_t v)
{
    const uint32_t old = *p;
    *p = v;
    return old;
}
static inline void __threadfence() {}

namespace kta {
namespace {
#include "kta_decode_coop.h"
#include "kta_header_names_kernel.h"
}
}

// `bytes` bytes that end at a page without access (and begin behind one when `front`); 16-byte aligned when bytes % 16 == 0
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
    if (argc != 3 && argc != 4) return 2;
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
    const size_t padded = ((blob_len + 15) & ~15ull) + 64;
    uint8_t *blob = guarded(padded, true);
    if (!ok || !blob) return 2;
    memset(blob, 0xA5, padded);
    if (fread(blob, 1, blob_len, f) != blob_len) return 2;
    fclose(f);
    const size_t words = kta::kHnWords;
    unsigned long long *vec = (unsigned long long *)guarded(words * 8, false);
    kta::HnSlot *names = (kta::HnSlot *)guarded(kta::kHnSlots * sizeof(kta::HnSlot), false);
    if (!vec || !names) return 2;
    memset(vec, 0, words * 8);
    memset(names, 0, kta::kHnSlots * sizeof(kta::HnSlot));
    unsigned long long info[kta::kHnInfoWords] = {0, 0, 0, 0};
    const uint32_t quads = (uint32_t)((n_batches + kta::kHnG - 1) / kta::kHnG);
    const uint32_t grid = argc == 4 && (uint32_t)atoi(argv[3]) > 0 && (uint32_t)atoi(argv[3]) < quads ? (uint32_t)atoi(argv[3]) : quads;   // fewer: a workgroup takes several fours
    const kta::FilterSpec spec{from_ms, to_ms, P, parts};
    const char *err = wave_emu::launch(grid, (int)order, seed, [&] {
        kta::kta_header_names(reinterpret_cast<const uint4 *>(blob), descs.data(), n_batches, P, spec, bitmap.data(), vec, names, info, grid);
    });
    if (err) {
        fprintf(stderr, "%s\n", err);
        return 3;
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(vec, 8, words, f) != words || fwrite(names, sizeof(kta::HnSlot), kta::kHnSlots, f) != kta::kHnSlots ||
        fwrite(info, 8, kta::kHnInfoWords, f) != kta::kHnInfoWords)
        return 2;
    fclose(f);
    printf("OK %u workgroups\n", grid);
    return 0;
}

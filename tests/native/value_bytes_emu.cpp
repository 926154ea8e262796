// value_bytes_emu.cpp — test infrastructure: kta_value_bytes (csrc/kta_value_bytes_kernel.h, the kernel's own source) compiled
// for the host over tests/native/wave_emu.h and run workgroup by workgroup, 64 lanes as fibers.  A program of its own
// (tests/test_value_bytes_emu.py builds and runs it): it reads a case file, runs the kernel and writes the vector and the work
// counters.  The kernel is instantiated with a flush threshold of kEmuFlush bytes, so that the flush in the middle of a pass
// runs on inputs of a few KiB.
//
// The blob is handed to the kernel as the device sees it — 16-byte aligned, 64 readable bytes behind its end, poisoned —
// between two pages without access: a read outside [0, padded length) ends the program with a signal.  The vector lies in
// front of such a page as well, so an add behind its end does too.
//
// Case file: as tests/native/payload_emu.cpp's.  Output file: the vector u64[264 P] | u64[4] work counters.  A third
// argument: the grid (workgroups; default and at most one per four batches).  A fourth: the kernel's form of combining equal
// bytes, as KTA_VALUE_BYTES_VARIANT numbers them (0 the default; 1 every byte on its own; 2 all pairs of a dword).
#include "wave_emu.h"

#include <sys/mman.h>
#include <unistd.h>

#include "../../include/kta_kafka.h"
#include "kta_filter.h"
#include "kta_records.h"
#include "kta_value_bytes.h"

// one OS thread: the atomics that wave_emu.h does not have are plain operations as well
static inline uint32_t atomicAdd(uint32_t *p, uint32_t v)
{
    const uint32_t old = *p;
    *p = old + v;
    return old;
}

constexpr uint32_t kEmuFlush = 3000;   // bytes: below a window, so that a flush also falls between the values of one round

namespace kta {
namespace {
#include "kta_decode_coop.h"
#include "kta_value_bytes_kernel.h"
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
    if (argc < 3 || argc > 5) return 2;
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
    const size_t words = kta::value_bytes_len(P);
    unsigned long long *vec = (unsigned long long *)guarded(words * 8, false);
    if (!vec) return 2;
    memset(vec, 0, words * 8);
    unsigned long long info[kta::kVbInfoWords] = {0, 0, 0, 0};
    const uint32_t quads = (uint32_t)((n_batches + kta::kVbG - 1) / kta::kVbG);
    const uint32_t asked = argc >= 4 ? (uint32_t)atoi(argv[3]) : 0u;
    const uint32_t grid = asked > 0 && asked < quads ? asked : quads;   // fewer: a workgroup takes several fours
    const int variant = argc == 5 ? atoi(argv[4]) : 0;
    const kta::FilterSpec spec{from_ms, to_ms, P, parts};
    const char *err = wave_emu::launch(grid, (int)order, seed, [&] {
        const uint4 *blocks = reinterpret_cast<const uint4 *>(blob);
        if (variant == 1)
            kta::kta_value_bytes<kEmuFlush, kta::kVbCombineNone>(blocks, descs.data(), n_batches, P, spec, bitmap.data(), vec, info, grid);
        else if (variant == 2)
            kta::kta_value_bytes<kEmuFlush, kta::kVbCombinePairs>(blocks, descs.data(), n_batches, P, spec, bitmap.data(), vec, info, grid);
        else
            kta::kta_value_bytes<kEmuFlush, kta::kVbCombineDword>(blocks, descs.data(), n_batches, P, spec, bitmap.data(), vec, info, grid);
    });
    if (err) {
        fprintf(stderr, "%s\n", err);
        return 3;
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(vec, 8, words, f) != words || fwrite(info, 8, kta::kVbInfoWords, f) != kta::kVbInfoWords) return 2;
    fclose(f);
    printf("OK %u workgroups\n", grid);
    return 0;
}

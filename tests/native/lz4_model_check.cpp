// lz4_model_check.cpp — test infrastructure: csrc/kta_lz4_model.h, the model compressor's own source, in a program of its
// own that tests/test_lz4_model_host.py builds with AddressSanitizer + UBSan and runs directly.  Every frame is written into
// a heap buffer of exactly its size (a byte behind it is a finding), inflated again with csrc/kta_lz4.h and compared; the
// counted size equals the written one; a buffer that is too small is filled to its end and no further.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "kta_lz4.h"
#include "kta_lz4_model.h"

static uint64_t g_rng = 0x243F6A8885A308D3ull;
static uint32_t next()
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33);
}

static int check(const std::vector<uint8_t> &src, const char *what)
{
    std::vector<uint32_t> table(kta::kLz4mTable, 0xFFFFFFFFu);   // (any content: a block clears it)
    kta::Lz4mCount size;
    const kta::Lz4mUnit u = kta::lz4m_frame(src.data(), src.size(), table.data(), size);
    if (u.frame_bytes != size.n || u.blocks != kta::lz4m_blocks(src.size()) || u.stored_blocks > u.blocks || u.match_bytes > src.size() ||
        u.match_bytes < 4 * u.sequences || u.frame_bytes > src.size() + 11 + 4 * u.blocks) {
        printf("%s: the unit's words\n", what);
        return 1;
    }
    std::vector<uint8_t> frame(size.n);
    kta::Lz4mEmit out{frame.data(), frame.size()};
    const kta::Lz4mUnit w = kta::lz4m_frame(src.data(), src.size(), table.data(), out);
    if (out.n != size.n || w.sequences != u.sequences || w.match_bytes != u.match_bytes) {
        printf("%s: written %llu, counted %llu\n", what, (unsigned long long)out.n, (unsigned long long)size.n);
        return 1;
    }
    std::vector<uint8_t> back(src.size() + 1);
    const int64_t got = kta::lz4_inflate(frame.data(), frame.size(), back.data(), src.size());
    if (got != (int64_t)src.size() || (!src.empty() && memcmp(back.data(), src.data(), src.size()) != 0)) {
        printf("%s: inflates to %lld bytes of %llu\n", what, (long long)got, (unsigned long long)src.size());
        return 1;
    }
    if (frame.size() > 8) {                                       // a destination that is too small
        std::vector<uint8_t> small(frame.size() - 5);
        kta::Lz4mEmit cut{small.data(), small.size()};
        kta::lz4m_frame(src.data(), src.size(), table.data(), cut);
        if (cut.n != size.n || memcmp(small.data(), frame.data(), small.size()) != 0) {
            printf("%s: the short destination\n", what);
            return 1;
        }
    }
    return 0;
}

int main()
{
    const size_t lengths[] = {0, 1, 12, 13, 16, 64, 65, 75, 76, 77, 140, 4096, 65535, 65536, 65537, 65536 + 12, 65536 + 13, 3 * 65536 + 5};
    int bad = 0;
    for (size_t n : lengths) {
        for (int law = 0; law < 6; law++) {
            std::vector<uint8_t> src(n);
            const uint32_t period = law == 1 ? 1 : law == 2 ? 3 : law == 3 ? 24 : 64;
            for (size_t k = 0; k < n; k++)
                src[k] = law == 0 ? 0 : law <= 4 ? (uint8_t)(0x41 + (k % period) * 7 % 26) : (uint8_t)next();
            if (law == 4)                                         // a few words, many short matches
                for (size_t k = 0; k < n; k++) src[k] = (uint8_t)("user action click view "[(k + (k / 23) * (next() % 3)) % 23]);
            char what[64];
            snprintf(what, sizeof what, "length %zu, law %d", n, law);
            bad += check(src, what);
        }
    }
    if (kta::lz4m_hc() != 0x82) printf("HC %02x\n", kta::lz4m_hc()), bad++;
    if (kta::lz4m_ext(14) != 0 || kta::lz4m_ext(15) != 1 || kta::lz4m_ext(269) != 1 || kta::lz4m_ext(270) != 2) printf("ext\n"), bad++;
    if (bad) return 1;
    printf("OK\n");
    return 0;
}

// tile_summary.cpp — csrc/kta_tile.h's host pack of one tile with its summary (kta_tile_sum) behind a C interface, next to
// the entry without one (tests/native/tile_codec.cpp's call), compiled with plain g++ for tests/test_tile_summary_host.py
// (no HIP, no GPU).
#include "kta_tile.h"

extern "C" {

void kta_tile_summary_pack(const int32_t *p, const int64_t *t, const int32_t *k, const int32_t *v, uint64_t m, int lens16, int32_t *part,
                           int64_t *ts, int32_t *klen, int32_t *vlen, kta_tile_hdr *hdr, kta_tile_sum *sum)
{
    *hdr = kta::tile_pack_host(p, t, k, v, m, lens16 != 0, part, ts, klen, vlen, sum);
}

// the existing codec entry: no summary asked for
void kta_tile_summary_pack_plain(const int32_t *p, const int64_t *t, const int32_t *k, const int32_t *v, uint64_t m, int lens16,
                                 int32_t *part, int64_t *ts, int32_t *klen, int32_t *vlen, kta_tile_hdr *hdr)
{
    *hdr = kta::tile_pack_host(p, t, k, v, m, lens16 != 0, part, ts, klen, vlen);
}

}

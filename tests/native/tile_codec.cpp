// tile_codec.cpp — csrc/kta_tile.h's host pack and unpack of one tile behind a C interface, compiled with plain g++ for
// tests/test_tile_codec_host.py (no HIP, no GPU).
#include "kta_tile.h"

extern "C" {

// klen / vlen null: the lengths are left out (kta_tile.h)
void kta_tile_codec_pack(const int32_t *p, const int64_t *t, const int32_t *k, const int32_t *v, uint64_t m, int lens16, int32_t *part,
                         int64_t *ts, int32_t *klen, int32_t *vlen, kta_tile_hdr *hdr)
{
    *hdr = kta::tile_pack_host(p, t, k, v, m, lens16 != 0, part, ts, klen, vlen);
}

void kta_tile_codec_unpack(const kta_tile_hdr *hdr, const int32_t *part, const int64_t *ts, const int32_t *klen, const int32_t *vlen,
                           uint64_t j0, uint64_t j1, int32_t *p, int64_t *t, int32_t *k, int32_t *v)
{
    kta::tile_unpack_host(*hdr, part, ts, klen, vlen, j0, j1, p, t, k, v);
}

}

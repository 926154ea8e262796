// tile_summary.cpp — csrc/kta_tile.h's host pack of one tile with its summary (kta_tile_sum) behind a C interface, next to
// the entry without one (tests/native/tile_codec.cpp's call) and the tile's scan plane, compiled with plain g++ for
// tests/test_tile_summary_host.py and tests/test_device_batch_model.py (no HIP, no GPU).
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

// the scan plane of the tile that kta_tile_summary_pack packed from the same records into the ts image `ts` with header
// *hdr: -> the mark; the plane's words go to bytes [4096, 8192) of ts and the two size extrema to sizes, iff it is 1
// (tests/test_device_batch_model.py: plane_definition against this)
uint32_t kta_tile_summary_plane(const kta_tile_hdr *hdr, const int32_t *p, const int32_t *k, const int32_t *v, uint64_t m, int64_t *ts,
                                uint32_t *sizes)
{
    return kta::tile_plane_host(*hdr, p, k, v, m, ts, sizes);
}

}

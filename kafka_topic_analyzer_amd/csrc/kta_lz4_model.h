// kta_lz4_model.h — the compression what-if (KTA_FLAG_COMPRESS_WHATIF, include/kta_hip.h): the one statement of the MODEL
// COMPRESSOR, a defined LZ4 compressor whose output size says what `compression.type=lz4` would leave of a batch, of the
// section's vector, of the identities between its words.  Same source on the host (kta_api.hip, host/report.cpp, the CPU
// suite) and on the device (kta_lz4_model_kernel.h uses the costs, the hash and the layout; its schedule of 64 lanes is
// held against lz4m_block below, bit for bit).  Plain C++, no HIP header.  No reference counterpart.
//
// UNIT.  A batch's inflated records section, the bytes [payload_off, payload_end) of its descriptor: what a producer
// compresses.  It is cut into independent blocks of at most 65536 bytes, as an LZ4 frame with block independence has them.
// FRAME.  04 22 4D 18 | FLG 0x60 | BD 0x40 | HC (7 bytes); per block a u32 LE size and min(model(block), block length)
// bytes — a block that does not shrink is stored, bit 31 of its size set —; an end mark of 4 zero bytes.  No checksums, no
// content size.
// BLOCK b[0, n).  The LZ4 block grammar: the last 5 bytes are literals, no match starts behind n - 12, a block of n < 13 is
// literals only.  A sequence costs 1 + ext(ll) + ll + 2 + ext(m - 4), the closing literals 1 + ext(ll) + ll; ext(x) = 0 for
// x < 15, else 1 + (x - 15) / 255.
// MATCH FINDER.  A table T[4096] of positions, all zero at the block's start; h(p) = (le32(b + p) * 2654435761u) >> 20.  The
// cursor i starts at 1, the anchor a at 0.  While i <= n - 12, one STRIDE:
//   1. the stride is the positions p = i .. min(i + 63, n - 12);
//   2. every position looks up c(p) = T[h(p)] in the table AS IT STOOD BEFORE THE STRIDE;
//   3. p HITS when c(p) < p and le32(b + c) == le32(b + p);
//   4. the stride is walked left to right with q = i: the first hit p >= q becomes a match, extended while p + m < n - 5 and
//      b[c + m] == b[p + m]; the literals [a, p) and the match are emitted, a = q = p + m; repeated until no hit >= q remains;
//   5. every position of the stride is then inserted, T[h(p)] = max(T[h(p)], p): the highest position of a hash wins;
//   6. i = max(i + stride length, q).
// Then the literals [a, n).  Nothing in 1 .. 6 depends on the order in which the positions of a stride are looked at: 64 lanes
// can take one each.  (Inserting before looking up — a candidate inside the own stride — reads better on paper and compresses
// 2.4 x worse: a position would find itself or a neighbour that the walk then skips.)
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KTA_LZ4M_HD __host__ __device__ inline
#else
#define KTA_LZ4M_HD inline
#endif

namespace kta {

constexpr uint32_t kLz4mBlock = 65536;       // bytes of a block at most
constexpr uint32_t kLz4mTable = 4096;        // entries of T
constexpr uint32_t kLz4mStride = 64;         // positions of a stride at most
constexpr uint32_t kLz4mMinMatchBlock = 13;  // a shorter block is literals only
constexpr uint32_t kLz4mMatchLimit = 12;     // no match starts behind n - 12
constexpr uint32_t kLz4mLastLiterals = 5;    // the last bytes of a block are literals
constexpr uint32_t kLz4mFrameHead = 7, kLz4mBlockHead = 4, kLz4mEndMark = 4;
constexpr uint32_t kLz4mFlg = 0x60, kLz4mBd = 0x40;

KTA_LZ4M_HD uint32_t lz4m_le32(const uint8_t *p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);   // (little-endian hosts and the device)
    return v;
}
KTA_LZ4M_HD uint32_t lz4m_hash(uint32_t v) { return (v * 2654435761u) >> 20; }
KTA_LZ4M_HD uint32_t lz4m_ext(uint32_t x) { return x < 15u ? 0u : 1u + (x - 15u) / 255u; }
KTA_LZ4M_HD uint32_t lz4m_sequence_cost(uint32_t ll, uint32_t m) { return 1u + lz4m_ext(ll) + ll + 2u + lz4m_ext(m - 4u); }
KTA_LZ4M_HD uint32_t lz4m_closing_cost(uint32_t ll) { return 1u + lz4m_ext(ll) + ll; }
KTA_LZ4M_HD uint64_t lz4m_blocks(uint64_t n) { return (n + kLz4mBlock - 1) / kLz4mBlock; }

// xxHash32 of a short input (fewer than 16 bytes), seed 0: the frame descriptor's HC is its second byte.
KTA_LZ4M_HD uint32_t lz4m_xxh32_short(const uint8_t *p, uint32_t n)
{
    uint32_t h = 374761393u + n;
    uint32_t k = 0;
    for (; k + 4 <= n; k += 4) {
        h += lz4m_le32(p + k) * 3266489917u;
        h = ((h << 17) | (h >> 15)) * 668265263u;
    }
    for (; k < n; k++) {
        h += p[k] * 374761393u;
        h = ((h << 11) | (h >> 21)) * 2654435761u;
    }
    h ^= h >> 15, h *= 2246822519u, h ^= h >> 13, h *= 3266489917u, h ^= h >> 16;
    return h;
}
KTA_LZ4M_HD uint8_t lz4m_hc()
{
    const uint8_t d[2] = {(uint8_t)kLz4mFlg, (uint8_t)kLz4mBd};
    return (uint8_t)(lz4m_xxh32_short(d, 2) >> 8);
}

// ---- the output policies: count only, or emit bytes ---------------------------------------------------------------------
struct Lz4mCount {
    uint64_t n = 0;
    KTA_LZ4M_HD void put(uint8_t) { n++; }
    KTA_LZ4M_HD void copy(const uint8_t *, uint64_t len) { n += len; }
};
struct Lz4mEmit {   // n counts on behind cap: the caller sees what the frame needs
    uint8_t *dst;
    uint64_t cap;
    uint64_t n = 0;
    KTA_LZ4M_HD void put(uint8_t v)
    {
        if (n < cap) dst[n] = v;
        n++;
    }
    KTA_LZ4M_HD void copy(const uint8_t *src, uint64_t len)
    {
        for (uint64_t k = 0; k < len; k++) put(src[k]);
    }
};

template <class Out> KTA_LZ4M_HD void lz4m_put_ext(Out &out, uint32_t x)   // the bytes behind a token's 15
{
    if (x < 15u) return;
    x -= 15u;
    for (; x >= 255u; x -= 255u) out.put(255);
    out.put((uint8_t)x);
}
template <class Out> KTA_LZ4M_HD void lz4m_put_sequence(Out &out, const uint8_t *lit, uint32_t ll, uint32_t offset, uint32_t m)
{
    out.put((uint8_t)(((ll < 15u ? ll : 15u) << 4) | (m - 4u < 15u ? m - 4u : 15u)));
    lz4m_put_ext(out, ll);
    out.copy(lit, ll);
    out.put((uint8_t)(offset & 0xFFu)), out.put((uint8_t)(offset >> 8));
    lz4m_put_ext(out, m - 4u);
}
template <class Out> KTA_LZ4M_HD void lz4m_put_closing(Out &out, const uint8_t *lit, uint32_t ll)
{
    out.put((uint8_t)((ll < 15u ? ll : 15u) << 4));
    lz4m_put_ext(out, ll);
    out.copy(lit, ll);
}

struct Lz4mMatches {
    uint64_t sequences, match_bytes;
};

// ---- THE DEFINITION: model(block) ---------------------------------------------------------------------------------------
// b[0, n), n <= 65536; T: kLz4mTable words of the caller's (any content).  The block's bytes go to `out`; mt counts on.
template <class Out> KTA_LZ4M_HD void lz4m_block(const uint8_t *b, uint32_t n, uint32_t *T, Out &out, Lz4mMatches &mt)
{
    uint32_t a = 0;
    if (n >= kLz4mMinMatchBlock) {
        for (uint32_t k = 0; k < kLz4mTable; k++) T[k] = 0;
        const uint32_t last = n - kLz4mMatchLimit, lim = n - kLz4mLastLiterals;
        uint32_t i = 1;
        while (i <= last) {
            const uint32_t len = last - i + 1 < kLz4mStride ? last - i + 1 : kLz4mStride;
            uint32_t c[kLz4mStride];
            for (uint32_t l = 0; l < len; l++) c[l] = T[lz4m_hash(lz4m_le32(b + i + l))];        // 2: the table before the stride
            uint32_t q = i;
            for (uint32_t l = 0; l < len; l++) {                                                // 4: left to right
                const uint32_t p = i + l, cc = c[l];
                if (p < q || !(cc < p && lz4m_le32(b + cc) == lz4m_le32(b + p))) continue;      // 3
                uint32_t m = 4;
                while (p + m < lim && b[cc + m] == b[p + m]) m++;
                lz4m_put_sequence(out, b + a, p - a, p - cc, m);
                mt.sequences++, mt.match_bytes += m;
                a = q = p + m;
            }
            for (uint32_t l = 0; l < len; l++) {                                                // 5
                const uint32_t p = i + l, h = lz4m_hash(lz4m_le32(b + p));
                if (T[h] < p) T[h] = p;
            }
            i = i + len > q ? i + len : q;                                                      // 6
        }
    }
    lz4m_put_closing(out, b + a, n - a);
}

// ---- the frame of one unit ----------------------------------------------------------------------------------------------
struct Lz4mUnit {
    uint64_t blocks, stored_blocks, frame_bytes, sequences, match_bytes;
};

// src[0, n): a records section.  The frame's bytes go to `out` (Lz4mCount: only counted).  T as lz4m_block's.
template <class Out> KTA_LZ4M_HD Lz4mUnit lz4m_frame(const uint8_t *src, uint64_t n, uint32_t *T, Out &out)
{
    Lz4mUnit u{0, 0, 0, 0, 0};
    const uint64_t before = out.n;
    out.put(0x04), out.put(0x22), out.put(0x4D), out.put(0x18), out.put((uint8_t)kLz4mFlg), out.put((uint8_t)kLz4mBd), out.put(lz4m_hc());
    for (uint64_t pos = 0; pos < n; pos += kLz4mBlock) {
        const uint32_t bn = n - pos < kLz4mBlock ? (uint32_t)(n - pos) : kLz4mBlock;
        Lz4mCount size;
        Lz4mMatches mt{0, 0};
        lz4m_block(src + pos, bn, T, size, mt);
        const bool stored = size.n >= bn;                   // does not shrink: stored
        const uint32_t word = stored ? (bn | 0x80000000u) : (uint32_t)size.n;
        for (int k = 0; k < 4; k++) out.put((uint8_t)(word >> (8 * k)));
        if (stored) {
            out.copy(src + pos, bn);
        } else {
            Lz4mMatches again{0, 0};
            lz4m_block(src + pos, bn, T, out, again);
        }
        u.blocks++, u.stored_blocks += stored ? 1u : 0u, u.sequences += mt.sequences, u.match_bytes += mt.match_bytes;
    }
    for (int k = 0; k < 4; k++) out.put(0);
    u.frame_bytes = out.n - before;
    return u;
}

// ---- the vector: u64[8 P + 20], every word a SUM ------------------------------------------------------------------------
//   [8 p, 8 p + 8)             partition p: batches, blocks, stored_blocks, raw_bytes, now_bytes, model_bytes, sequences,
//                              match_bytes
//   8 P + 4 c .. 8 P + 4 c + 3 the batches whose CURRENT codec is c (0 none, 1 gzip, 2 snappy, 3 lz4, 4 zstd): batches,
//                              raw_bytes, now_bytes, model_bytes
// raw_bytes: payload_end - payload_off, the records section inflated.  now_bytes: batch_bytes - 61, the records section as it
// lies on disk.  model_bytes: the frame's bytes.  sequences: matches; match_bytes: the bytes they cover.
enum CompressWhatifWord : uint32_t {
    kCwBatches = 0, kCwBlocks, kCwStoredBlocks, kCwRawBytes, kCwNowBytes, kCwModelBytes, kCwSequences, kCwMatchBytes,
    kCwPartitionWords = 8,
    kCwCodecBatches = 0, kCwCodecRawBytes, kCwCodecNowBytes, kCwCodecModelBytes,
    kCwCodecWords = 4,
    kCwCodecs = 5,
    kCwGlobals = kCwCodecs * kCwCodecWords
};
constexpr uint32_t kCwBatchHeader = 61;   // (KTA_KAFKA_BATCH_HEADER: on neither side of the comparison)

KTA_LZ4M_HD size_t compress_whatif_len(uint32_t P) { return (size_t)kCwPartitionWords * P + kCwGlobals; }
// The codec of a descriptor's flags (KTA_KB_GZIP 16, KTA_KB_SNAPPY 4, KTA_KB_LZ4 8, KTA_KB_ZSTD 32), in Kafka's numbering.
KTA_LZ4M_HD uint32_t compress_whatif_codec(uint32_t flags) { return (flags & 16u) ? 1u : (flags & 4u) ? 2u : (flags & 8u) ? 3u : (flags & 32u) ? 4u : 0u; }
inline const char *compress_whatif_codec_name(uint32_t c) { return c == 0 ? "none" : c == 1 ? "gzip" : c == 2 ? "snappy" : c == 3 ? "lz4" : "zstd"; }

// What one counted batch adds (host form; the kernel adds the same words from registers).  recs[0, n): its records section,
// inflated; batch_bytes: the descriptor's.
inline void compress_whatif_add(uint64_t *vec, uint32_t P, uint32_t partition, uint32_t codec, uint32_t batch_bytes, const uint8_t *recs, uint64_t n)
{
    uint32_t T[kLz4mTable];
    Lz4mCount out;
    const Lz4mUnit u = lz4m_frame(recs, n, T, out);
    const uint64_t now = batch_bytes > kCwBatchHeader ? batch_bytes - kCwBatchHeader : 0;
    uint64_t *w = vec + (size_t)kCwPartitionWords * partition, *c = vec + (size_t)kCwPartitionWords * P + (size_t)kCwCodecWords * codec;
    w[kCwBatches]++, w[kCwBlocks] += u.blocks, w[kCwStoredBlocks] += u.stored_blocks, w[kCwRawBytes] += n, w[kCwNowBytes] += now;
    w[kCwModelBytes] += u.frame_bytes, w[kCwSequences] += u.sequences, w[kCwMatchBytes] += u.match_bytes;
    c[kCwCodecBatches]++, c[kCwCodecRawBytes] += n, c[kCwCodecNowBytes] += now, c[kCwCodecModelBytes] += u.frame_bytes;
}

// The sum over the partitions.
inline void compress_whatif_topic(const uint64_t *vec, uint32_t P, uint64_t out[kCwPartitionWords])
{
    for (uint32_t k = 0; k < kCwPartitionWords; k++) out[k] = 0;
    for (uint32_t p = 0; p < P; p++)
        for (uint32_t k = 0; k < kCwPartitionWords; k++) out[k] += vec[(size_t)kCwPartitionWords * p + k];
}

// ---- the identities between the words of one vector ---------------------------------------------------------------------
// The codec table's sums equal the partitions' sums; per partition stored_blocks <= blocks, match_bytes <= raw_bytes,
// model_bytes <= raw_bytes + 11 batches + 4 blocks (every block stored at worst), match_bytes >= 4 sequences.
inline bool compress_whatif_identities_hold(const uint64_t *vec, uint32_t P)
{
    uint64_t topic[kCwPartitionWords], codecs[kCwCodecWords] = {0, 0, 0, 0};
    compress_whatif_topic(vec, P, topic);
    for (uint32_t c = 0; c < kCwCodecs; c++)
        for (uint32_t k = 0; k < kCwCodecWords; k++) codecs[k] += vec[(size_t)kCwPartitionWords * P + (size_t)kCwCodecWords * c + k];
    if (codecs[kCwCodecBatches] != topic[kCwBatches] || codecs[kCwCodecRawBytes] != topic[kCwRawBytes] || codecs[kCwCodecNowBytes] != topic[kCwNowBytes] ||
        codecs[kCwCodecModelBytes] != topic[kCwModelBytes])
        return false;
    for (uint32_t p = 0; p < P; p++) {
        const uint64_t *w = vec + (size_t)kCwPartitionWords * p;
        if (w[kCwStoredBlocks] > w[kCwBlocks] || w[kCwMatchBytes] > w[kCwRawBytes] ||
            w[kCwModelBytes] > w[kCwRawBytes] + 11u * w[kCwBatches] + 4u * w[kCwBlocks] || w[kCwMatchBytes] < 4u * w[kCwSequences])
            return false;
    }
    return true;
}

} // namespace kta

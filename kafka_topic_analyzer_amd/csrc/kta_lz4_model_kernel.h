// kta_lz4_model_kernel.h — the compression what-if's kernel (kta_lz4_model, KTA_FLAG_COMPRESS_WHATIF).  kta_lz4_model.hip
// includes this file INSIDE its unnamed namespace; it has no includes of its own: the including file has included
// kta_kafka.h, kta_record_batches.h and kta_lz4_model.h (at file scope) and provides the HIP runtime — or, for the CPU
// suite, tests/native/wave_emu.h (tests/native/lz4_model_emu.cpp, tests/test_lz4_model_emu.py): the kernel below is then
// the very source the GPU runs.  What the kernel does is said at the top of kta_lz4_model.hip.
#pragma once

#ifndef KTA_BALLOT64    // the lanes (of those that call it together) whose predicate holds.  (wave_emu.h: a meeting point.)
#define KTA_BALLOT64(p) ((uint64_t)__builtin_amdgcn_ballot_w64(p))
#endif
#ifndef KTA_UNI         // a value every lane holds alike, moved to a scalar register (the emulator: the value)
#define KTA_UNI(v) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(v)))
#endif
#ifndef KTA_READLANE
#define KTA_READLANE(v, l) ((uint32_t)__builtin_amdgcn_readlane((int)(v), (int)(l)))
#endif

constexpr uint32_t kCwWavesPerCu = 8;       // resident workgroups per CU (16 KiB of LDS each; the grid is that many per CU at most)
constexpr uint32_t kCwLaneSteps = 4;        // a lane extends its own hit by this many dwords behind the first four bytes
constexpr uint32_t kCwEpochBits = 16;       // a table entry: epoch << 16 | position (a position is below 65536)
constexpr uint32_t kCwEpochs = 1u << kCwEpochBits;   // the tags 1 .. kCwEpochs - 1, then the table is zeroed
constexpr uint32_t kCwPositionMask = (1u << kCwEpochBits) - 1u;
static_assert(kLz4mBlock <= (1u << 16) && kLz4mStride == 64, "a position fits 16 bits; a lane a position");

// How many of the four bytes at b[c + off ..] and b[p + off ..] agree from the first on, among those in front of lim (a
// match ends in front of lim = n - 5, so the dwords lie inside the block).  c < p.
__device__ __forceinline__ uint32_t cw_agree(const uint8_t *b, uint32_t c, uint32_t p, uint32_t off, uint32_t lim)
{
    if (p + off >= lim) return 0u;
    const uint32_t room = lim - (p + off);
    const uint32_t x = kta::lz4m_le32(b + c + off) ^ kta::lz4m_le32(b + p + off);
    const uint32_t eq = x ? (uint32_t)__builtin_ctz(x) >> 3 : 4u;
    return eq < room ? eq : room;
}

// What a wave holds in registers (every lane the same) for the batches of ONE partition and ONE codec since the last flush.
struct CwAcc {
    int32_t part;      // -1: nothing yet
    uint32_t codec;
    uint64_t w[kta::kCwPartitionWords];
};

__device__ __forceinline__ void cw_flush(CwAcc &a, uint32_t P, unsigned long long *vec, uint32_t lane)
{
    if (a.part >= 0) {
        uint64_t mine = 0;
#pragma unroll
        for (uint32_t k = 0; k < kta::kCwPartitionWords; k++) mine = lane == k ? a.w[k] : mine;
        // lanes 8 .. 11: the codec's batches, raw_bytes, now_bytes, model_bytes
        mine = lane == 8 ? a.w[kta::kCwBatches] : lane == 9 ? a.w[kta::kCwRawBytes] : lane == 10 ? a.w[kta::kCwNowBytes] : lane == 11 ? a.w[kta::kCwModelBytes] : mine;
        if (lane < kta::kCwPartitionWords && mine) atomicAdd(vec + (size_t)kta::kCwPartitionWords * (uint32_t)a.part + lane, (unsigned long long)mine);
        if (lane >= 8 && lane < 12 && mine)
            atomicAdd(vec + (size_t)kta::kCwPartitionWords * P + (size_t)kta::kCwCodecWords * a.codec + (lane - 8), (unsigned long long)mine);
    }
    a.part = -1, a.codec = 0;
#pragma unroll
    for (uint32_t k = 0; k < kta::kCwPartitionWords; k++) a.w[k] = 0;
}

// model(block) of b[0, n) by the wave: its size, and the matches added to seqs / mbytes.  Every lane returns the same.
// s_T: the wave's table; epoch: this block's tag, above every tag the table holds (or the table is all zero).
__device__ __forceinline__ uint32_t cw_block(const uint8_t *b, uint32_t n, uint32_t *s_T, uint32_t epoch, uint32_t lane, uint64_t &seqs, uint64_t &mbytes)
{
    uint32_t a = 0, cost = 0;
    if (n >= kta::kLz4mMinMatchBlock) {
        const uint32_t last = n - kta::kLz4mMatchLimit, lim = n - kta::kLz4mLastLiterals, tag = epoch << kCwEpochBits;
        uint32_t i = 1;
        while (i <= last) {                                                    // (uniform)
            const uint32_t p = i + lane;
            const bool active = p <= last;
            uint32_t v = 0, h = 0, c = 0, m = 0;
            bool hit = false, capped = false;
            if (active) {
                v = kta::lz4m_le32(b + p);
                h = kta::lz4m_hash(v);
                const uint32_t e = s_T[h];
                c = (e >> kCwEpochBits) == epoch ? (e & kCwPositionMask) : 0u; // an entry of an earlier block is the zero it began with
                hit = c < p && kta::lz4m_le32(b + c) == v;
            }
            if (hit) {                                                         // a short extension of the lane's own
                m = 4;
                capped = true;
#pragma unroll 1
                for (uint32_t k = 0; k < kCwLaneSteps; k++) {
                    const uint32_t eq = cw_agree(b, c, p, m, lim);
                    m += eq;
                    if (eq < 4u) { capped = false; break; }
                }
            }
            uint64_t hits = KTA_BALLOT64(hit);                                 // (the lookups lie in front of it, the inserts behind it)
            uint32_t q = i;
            while (hits) {                                                     // the greedy walk (uniform)
                const uint32_t j = KTA_UNI((uint32_t)__builtin_ctzll(hits));
                const uint32_t pj = i + j, cj = KTA_READLANE(c, j);
                uint32_t mj = KTA_READLANE(m, j);
                if (KTA_READLANE(capped ? 1u : 0u, j)) {                       // the wave goes on, 64 lanes by 4 bytes a step
                    for (;;) {
                        const uint32_t eq = cw_agree(b, cj, pj, mj + 4u * lane, lim);
                        const uint64_t ends = KTA_BALLOT64(eq < 4u);
                        if (!ends) { mj += 256u; continue; }
                        const uint32_t f = KTA_UNI((uint32_t)__builtin_ctzll(ends));
                        mj += 4u * f + KTA_READLANE(eq, f);
                        break;
                    }
                }
                cost += kta::lz4m_sequence_cost(pj - a, mj);
                seqs++, mbytes += mj;
                a = q = pj + mj;
                const uint32_t skip = q - i;                                   // the hits in front of q are skipped
                hits = skip >= 64u ? 0ull : hits & ~((1ull << skip) - 1ull);
            }
            if (active) atomicMax(&s_T[h], tag | p);                           // the highest position of a hash wins
            const uint32_t len = last - i + 1u < kta::kLz4mStride ? last - i + 1u : kta::kLz4mStride;
            i = i + len > q ? i + len : q;
            __syncthreads();                                                   // the inserts, in front of the next stride's lookups
        }
    }
    return cost + kta::lz4m_closing_cost(n - a);
}

// grid: the number of workgroups; workgroup w takes the batches w, w + grid, ... and of them those that count.
// EPOCHS: the tags a table takes before it is zeroed (kCwEpochs; the CPU suite instantiates it small).
template <uint32_t EPOCHS>
__global__ __launch_bounds__(64) KTA_WAVES_PER_EU(2, 8) void kta_lz4_model(const uint8_t *blob, const kta_kafka_batch_desc *descs, uint64_t n_batches, uint32_t P,
                                                                         kta::RbFilter f, unsigned long long *vec, uint32_t grid)
{
    static_assert(EPOCHS >= 2 && EPOCHS <= kCwEpochs, "a tag fits the entry's upper half");
    __shared__ uint32_t s_T[kta::kLz4mTable];
    const uint32_t lane = threadIdx.x;
    for (uint32_t k = lane; k < kta::kLz4mTable; k += 64) s_T[k] = 0u;
    uint32_t epoch = 0;
    CwAcc acc{-1, 0, {0, 0, 0, 0, 0, 0, 0, 0}};
    __syncthreads();
    for (uint64_t bi = blockIdx.x; bi < n_batches; bi += grid) {              // (uniform)
        const kta_kafka_batch_desc &d = descs[bi];
        const int32_t partition = d.partition;
        if (d.status != 0 || !kta::rb_counted(f, P, partition, d.base_ts_ms, d.max_ts_ms)) continue;
        const uint64_t off = d.payload_off, raw = d.payload_end > off ? d.payload_end - off : 0ull;
        const uint32_t codec = kta::compress_whatif_codec(d.flags);
        if (acc.part >= 0 && (acc.part != partition || acc.codec != codec)) cw_flush(acc, P, vec, lane);
        acc.part = partition, acc.codec = codec;
        uint64_t frame = kta::kLz4mFrameHead + kta::kLz4mEndMark, blocks = 0, stored = 0;
        for (uint64_t pos = 0; pos < raw; pos += kta::kLz4mBlock) {            // (uniform)
            const uint32_t bn = raw - pos < kta::kLz4mBlock ? (uint32_t)(raw - pos) : kta::kLz4mBlock;
            if (++epoch == EPOCHS) {                                        // the tags are used up: the table begins again
                __syncthreads();
                for (uint32_t k = lane; k < kta::kLz4mTable; k += 64) s_T[k] = 0u;
                epoch = 1;
                __syncthreads();
            }
            const uint32_t cost = cw_block(blob + off + pos, bn, s_T, epoch, lane, acc.w[kta::kCwSequences], acc.w[kta::kCwMatchBytes]);
            frame += kta::kLz4mBlockHead + (cost < bn ? cost : bn);
            blocks++, stored += cost >= bn ? 1u : 0u;
        }
        acc.w[kta::kCwBatches]++, acc.w[kta::kCwBlocks] += blocks, acc.w[kta::kCwStoredBlocks] += stored, acc.w[kta::kCwRawBytes] += raw;
        acc.w[kta::kCwNowBytes] += d.batch_bytes > kta::kCwBatchHeader ? d.batch_bytes - kta::kCwBatchHeader : 0u;
        acc.w[kta::kCwModelBytes] += frame;
    }
    cw_flush(acc, P, vec, lane);
}

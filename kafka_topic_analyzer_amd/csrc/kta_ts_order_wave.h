// kta_ts_order_wave.h — the wave step of the timestamp-order pass (KTA_FLAG_TS_ORDER, include/kta_hip.h): one instruction
// of a wave holds 64 consecutive records, lane order is record order, and every timestamped lane needs
//   prev = max(run[p], the timestamps of the lower lanes of its partition)        (-1: none; timestamps are >= 0)
// after which run[p] holds the instruction's maximum as well.  (Included by kta_ts_order.hip and, compiled for the host
// over tests/native/wave_emu.h, by tests/native/ts_order_emu.cpp: the CPU suite runs this text.)
//
//   one partition   every timestamped lane has the first one's partition (a readlane compare and a ballot: Kafka delivers
//                   per-partition runs): one wave-wide exclusive prefix maximum, seeded with run[p]; the last lane writes.
//   general         every lane writes its number into a per-wave byte table at its partition and reads it back (LDS
//                   operations of one wave are performed in program order): a lane that reads another's number shares its
//                   partition with it.  Each such partition is resolved as a group — a ballot of its lanes, a prefix
//                   maximum in which the other lanes hold the identity -1 —, one group per turn of a loop that removes at
//                   least one lane from the ballot it runs on.  The lanes left over are alone in their partitions and read
//                   and write run[p] themselves.  Which lane of a group wins the byte does not matter: all the others lose.
#pragma once

#ifndef KTA_READLANE
#define KTA_READLANE(v, l) ((uint32_t)__builtin_amdgcn_readlane((int)(v), (int)(l)))
#endif
#ifndef KTA_BALLOT64
#define KTA_BALLOT64(p) ((uint64_t)__builtin_amdgcn_ballot_w64(p))
#endif
#ifndef KTA_SHFL_UP
#define KTA_SHFL_UP(v, off) __shfl_up((v), (off))
#endif
// between the LDS operations of two instructions of a wave whose order matters (the hardware keeps a wave's LDS
// operations in program order; this keeps the compiler from moving them)
#ifndef KTA_TSO_LDS_ORDER
#define KTA_TSO_LDS_ORDER() asm volatile("" ::: "memory")
#endif

// a record that takes part: counted by the metrics handler (partition in [0, P)) with a timestamp that is available
__device__ __forceinline__ bool tso_timestamped(int32_t p, long long ts, uint32_t P) { return (uint32_t)p < P && ts >= 0; }

__device__ __forceinline__ long long tso_max(long long a, long long b) { return a > b ? a : b; }

__device__ __forceinline__ long long tso_shfl_up(long long v, uint32_t off)
{
    const uint32_t lo = KTA_SHFL_UP((uint32_t)(unsigned long long)v, off);
    const uint32_t hi = KTA_SHFL_UP((uint32_t)((unsigned long long)v >> 32), off);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// v of every lane -> *incl = max of lanes [0, lane], returns max of lanes [0, lane) (-1 for lane 0: v >= -1 everywhere)
__device__ __forceinline__ long long tso_prefix_max(uint32_t lane, long long v, long long *incl)
{
    long long a = v;
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const long long t = tso_shfl_up(a, off);
        if (lane >= off) a = tso_max(a, t);
    }
    *incl = a;
    const long long ex = tso_shfl_up(a, 1);
    return lane == 0 ? -1 : ex;
}

// One instruction.  run: the wave's table i64[P] (LDS), tag: the wave's byte table u8[P] (LDS; any contents).  on: the lane
// holds a timestamped record of partition p with timestamp ts (p and ts of the other lanes are not looked at).  Returns
// prev (-1 for a lane that is not on).  n_one / n_groups (the same on every lane) count the instructions that took the
// one-partition path and the colliding groups resolved.  Every lane of the wave must call it.
__device__ __forceinline__ long long tso_wave_step(long long *run, uint8_t *tag, uint32_t lane, bool on, uint32_t p, long long ts,
                                                   uint32_t &n_one, uint32_t &n_groups)
{
    const uint64_t live = KTA_BALLOT64(on);
    if (live == 0) return -1;
    const long long v = on ? ts : -1;
    const uint32_t p0 = KTA_READLANE(p, (uint32_t)__builtin_ctzll(live));
    long long prev = -1;
    if (KTA_BALLOT64(on && p != p0) == 0) {
        long long incl;
        const long long ex = tso_prefix_max(lane, v, &incl);
        const long long seed = run[p0];
        if (on) prev = tso_max(seed, ex);
        KTA_TSO_LDS_ORDER();
        if (lane == 63) run[p0] = tso_max(seed, incl);
        KTA_TSO_LDS_ORDER();
        n_one++;
        return prev;
    }
    if (on) tag[p] = (uint8_t)lane;
    KTA_TSO_LDS_ORDER();
    const uint32_t seen = on ? (uint32_t) * static_cast<const volatile uint8_t *>(tag + p) : lane;
    KTA_TSO_LDS_ORDER();
    uint64_t todo = KTA_BALLOT64(on && seen != lane);   // lost their byte to another lane of their partition
    uint64_t grouped = 0;
    while (todo) {                                      // (wave-uniform) one trip per colliding partition
        const uint32_t pg = KTA_READLANE(p, (uint32_t)__builtin_ctzll(todo));
        const bool in = on && p == pg;
        const uint64_t grp = KTA_BALLOT64(in);
        long long incl;
        const long long ex = tso_prefix_max(lane, in ? ts : -1, &incl);
        const long long seed = run[pg];
        if (in) prev = tso_max(seed, ex);
        KTA_TSO_LDS_ORDER();
        if (lane == 63) run[pg] = tso_max(seed, incl);
        KTA_TSO_LDS_ORDER();
        grouped |= grp;
        todo &= ~grp;
        n_groups++;
    }
    if (on && !((grouped >> lane) & 1ull)) {            // alone in its partition
        prev = run[p];
        run[p] = tso_max(prev, ts);
    }
    KTA_TSO_LDS_ORDER();
    return prev;
}

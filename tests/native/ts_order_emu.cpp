// ts_order_emu.cpp — test infrastructure: the wave step of the timestamp-order pass (csrc/kta_ts_order_wave.h, the apply
// kernel's own source) compiled for the host over tests/native/wave_emu.h and run with its 64 lanes as fibers.
// tests/test_ts_order_emu.py compares every lane's `prev` and the final table with the sequential loop.
#include "wave_emu.h"

// The step orders the LDS operations of consecutive instructions of one wave; the hardware keeps them in program order.
// Here the lanes run one after the other between two meeting points, so the order point is a meeting of its own (the
// emulator has none without a value: a ballot of nothing).
#define KTA_TSO_LDS_ORDER() ((void)wave_emu::ballot(false, __LINE__))

namespace {
#include "kta_ts_order_wave.h"
}

extern "C" {

// n_instr instructions of 64 records each (partition, ts_ms: n_instr * 64 values) share the table run[P] (in: the seed,
// out: the final table).  prev[n_instr * 64]: what every lane got (-1 for a lane that is not timestamped).
// counters[2]: instructions on the one-partition path, colliding groups.  order, seed: wave_emu::launch.
// Returns 0; -2: the emulator reports divergent meeting points.
int kta_emu_ts_order(const int32_t *partition, const int64_t *ts_ms, uint32_t n_instr, uint32_t P, int64_t *run, int64_t *prev,
                     uint32_t *counters, int order, uint32_t seed, char *err_out, uint64_t err_cap)
{
    std::vector<long long> table(run, run + P);
    std::vector<uint8_t> tag(P, 0xEE);
    const char *err = wave_emu::launch(1, order, seed, [&] {
        const uint32_t lane = threadIdx.x;
        uint32_t n_one = 0, n_groups = 0;
        for (uint32_t j = 0; j < n_instr; j++) {
            const int32_t p = partition[(size_t)j * 64 + lane];
            const long long ts = (long long)ts_ms[(size_t)j * 64 + lane];
            prev[(size_t)j * 64 + lane] = (int64_t)tso_wave_step(table.data(), tag.data(), lane, tso_timestamped(p, ts, P), (uint32_t)p, ts, n_one, n_groups);
        }
        if (lane == 0) counters[0] = n_one, counters[1] = n_groups;
    });
    if (err) {
        if (err_out && err_cap) snprintf(err_out, err_cap, "%s", err);
        return -2;
    }
    for (uint32_t p = 0; p < P; p++) run[p] = (int64_t)table[p];
    return 0;
}

} // extern "C"

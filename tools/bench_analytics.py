"""What KTA_FLAG_ANALYTICS costs the metrics scan: config 4 (256 partitions, 2^30 records by default) resident in HBM
on one GPU, scan + fold timed with the library's timing hooks (kta_set_timing / kta_kernel_time_stats), once by a
context without analytics and once by one with them, on the same box in the same process and the same records.

    python tools/bench_analytics.py [--log2-records 30] [--steps 10] [--warmup 3]

Prints one JSON line per leg (ms per pass of scan + fold, records/s, TB/s of the 20 B per record the scan reads,
fraction of the 8 TB/s HBM roofline) and a last line with the ratio of the two legs.  Both legs' reference counters are
compared (the analytics arm must not change them)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import kafka_topic_analyzer_amd as kta  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-records", type=int, default=30)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()

BYTES_PER_RECORD = 20            # partition, key_len, val_len (i32) + ts_ms (i64)
ROOFLINE_TBS = 8.0
n, P = 1 << args.log2_records, 256
spec, _ = kta.synth_preset("c4")
owner = kta.HipMetricHandler(P)
batch = owner.device_batch_alloc(n)
owner.synth_fill_device(spec, 0, n, batch)
owner.sync()


def leg(analytics):
    with kta.HipMetricHandler(P, analytics=analytics) as h:
        for _ in range(args.warmup):
            h.submit_device(batch, n, 0, which=1)
        h.sync()
        h.kernel_time_stats()                                    # drain what the warm-up recorded
        h.set_timing(True)
        for _ in range(args.steps):
            h.submit_device(batch, n, 0, which=1)
        avg, launches = h.kernel_time_stats()
        h.set_timing(False)
        ms = (avg[0] * launches[0] + avg[1] * launches[1]) / args.steps
        _, counters = h.finish()
    tbs = n * BYTES_PER_RECORD / (ms * 1e-3) / 1e12
    line = {"tool": "bench_analytics", "leg": "analytics" if analytics else "plain", "config": "c4", "partitions": P,
            "records": n, "steps": args.steps, "scan_launches_per_step": launches[0] / args.steps,
            "ms": round(ms, 4), "records_per_s": round(n / (ms * 1e-3)), "TBps": round(tbs, 3),
            "roofline_frac": round(tbs / ROOFLINE_TBS, 4)}
    print(json.dumps(line), flush=True)
    return line, counters


plain, c_plain = leg(False)
anal, c_anal = leg(True)
print(json.dumps({"tool": "bench_analytics", "ratio_analytics_over_plain_ms": round(anal["ms"] / plain["ms"], 4),
                  "counters_equal": bool(np.array_equal(c_plain, c_anal))}), flush=True)
owner.device_batch_free(batch)
owner.close()

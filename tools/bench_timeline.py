"""What the timeline (kta_set_timeline) costs the metrics scan: config 4 (256 partitions, 2^30 records by default)
resident in HBM on one GPU as tile-compact batches, scan + fold timed with the library's timing hooks (kta_set_timing /
kta_kernel_time_stats) by three contexts — no timeline, a timeline (W = 10 s, 1024 buckets from ts_base - 30 min), a
timeline and the analytics — under two timestamp laws: c4's own (+-1 h of jitter: the buckets scatter inside a wave) and
c4 with ts_jitter_ms = 0 (ordered: a wave lands in one bucket, the contention case).  The legs alternate, round after
round, in one process on one box, over the same records.

    python tools/bench_timeline.py [--log2-records 30] [--steps 10] [--warmup 3] [--rounds 2]

Prints one JSON line per leg and round (ms per pass of scan + fold, records/s, TB/s of the 20 B per record the
reference columns hold, fraction of the 8 TB/s HBM roofline) and per law a last line with the best-of-rounds ratios to
the plain leg.  Every leg's reference counters are compared with the plain leg's (the timeline must not change them)."""
import argparse
import copy
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
ap.add_argument("--rounds", type=int, default=2)
args = ap.parse_args()

BYTES_PER_RECORD = 20
ROOFLINE_TBS = 8.0
n, P = 1 << args.log2_records, 256
base, _ = kta.synth_preset("c4")
TL = (int(base.ts_base_ms) - 30 * 60 * 1000, 10_000, 1024)
LEGS = (("plain", False, None), ("timeline", False, TL), ("timeline+analytics", True, TL))


def leg(batch, law, name, analytics, tl, rnd):
    with kta.HipMetricHandler(P, analytics=analytics, timeline=tl) as h:
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
        rows = int((h.timeline()[:, 0] != 0).sum()) if tl else 0
    tbs = n * BYTES_PER_RECORD / (ms * 1e-3) / 1e12
    line = {"tool": "bench_timeline", "law": law, "leg": name, "round": rnd, "config": "c4", "partitions": P,
            "records": n, "steps": args.steps, "scan_launches_per_step": launches[0] / args.steps, "ms": round(ms, 4),
            "records_per_s": round(n / (ms * 1e-3)), "TBps": round(tbs, 3), "roofline_frac": round(tbs / ROOFLINE_TBS, 4),
            "nonzero_timeline_rows": rows}
    print(json.dumps(line), flush=True)
    return ms, counters


for law in ("c4", "c4_ordered"):
    spec = copy.copy(base)
    if law == "c4_ordered":
        spec.ts_jitter_ms = 0
    owner = kta.HipMetricHandler(P)
    batch = owner.device_batch_alloc(n)
    owner.synth_fill_device(spec, 0, n, batch)
    owner.sync()
    best, counters = {}, {}
    for rnd in range(args.rounds):
        for name, analytics, tl in LEGS:
            ms, c = leg(batch, law, name, analytics, tl, rnd)
            best[name] = min(best.get(name, ms), ms)
            counters[name] = c
    print(json.dumps({"tool": "bench_timeline", "law": law,
                      "ratio_timeline_over_plain_ms": round(best["timeline"] / best["plain"], 4),
                      "ratio_timeline_analytics_over_plain_ms": round(best["timeline+analytics"] / best["plain"], 4),
                      "counters_equal": all(np.array_equal(counters["plain"], c) for c in counters.values())}), flush=True)
    owner.device_batch_free(batch)
    owner.close()

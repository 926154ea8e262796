"""What the timestamp-order pass (KTA_FLAG_TS_ORDER) costs: 2^30 records (by default) resident in HBM on one GPU as keyless
tile-compact batches, the metrics handler (which = 1) timed by wall clock around whole passes over all batches, by a
context without the flag (the scan alone) and one with it (scan + the pass), alternated round after round in one process.
Three laws:

    c4          config 4 as it is: random partitions, +-1 h jitter, nearly every record late (the general path, the histogram)
    c4-ordered  config 4 with KTA_PART_RUNS, run length 500, ts_jitter_ms = 0: the one-partition path, nothing late
    c3          config 3

    python tools/bench_ts_order.py [--log2-records 30] [--log2-batch 27] [--steps 5] [--warmup 1] [--rounds 2]
                                   [--laws c4,c4-ordered,c3] [--pass-only]

Prints one JSON line per law, leg and round, and per law a last line: the pass's share (best scan + pass minus best scan
alone), its TB/s of algorithmic bytes (2 x (2 + 4) B per record: both record kernels read partition and timestamp of a
compact tile) and fraction of the 8 TB/s roofline, the late records, and the pass's work counters of one warm pass
(kta_ts_order_info).  --pass-only runs the second leg alone, for a `rocprofv3 --kernel-trace --stats` run of its own."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import kafka_topic_analyzer_amd as kta  # noqa: E402
from kafka_topic_analyzer_amd import _native as N  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-records", type=int, default=30)
ap.add_argument("--log2-batch", type=int, default=27)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--laws", default="c4,c4-ordered,c3")
ap.add_argument("--pass-only", action="store_true")
args = ap.parse_args()

ROOFLINE_TBS = 8.0
n = 1 << args.log2_records
INFO = ("launches", "chunks", "instructions", "one_partition", "groups")


def law_spec(law):
    spec, _ = kta.synth_preset("c3" if law == "c3" else "c4")
    if law == "c4-ordered":
        spec.part_mode, spec.part_run_len, spec.ts_jitter_ms = N.KTA_PART_RUNS, 500, 0
    return spec


def run_leg(h, on, batches, per):
    for _ in range(args.warmup):
        for i, b in enumerate(batches):
            h.submit_device(b, per, i * per, which=1)
    h.sync()
    before = h.ts_order_info() if on else None
    t0 = time.perf_counter()
    for _ in range(args.steps):
        for i, b in enumerate(batches):
            h.submit_device(b, per, i * per, which=1)
    h.sync()
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    work = None
    if on:
        after = h.ts_order_info()
        work = {k: (after[k] - before[k]) // args.steps for k in INFO}
        work["chunk_records"] = after["chunk_records"]
    return ms, work


for law in args.laws.split(","):
    spec = law_spec(law)
    P = int(spec.n_partitions)
    per = min(n, 1 << args.log2_batch)
    owner = kta.HipMetricHandler(P)
    batches = []
    for lo in range(0, n, per):
        b = owner.device_batch_alloc(per)
        owner.synth_fill_device(spec, lo, per, b)
        batches.append(b)
    owner.sync()
    alg_bytes = n * 2 * (2 + 4)
    legs = (("scan+ts_order", True),) if args.pass_only else (("scan", False), ("scan+ts_order", True))
    best, work = {}, None
    with kta.HipMetricHandler(P) as plain, kta.HipMetricHandler(P, ts_order=True) as tso:
        for rnd in range(args.rounds):
            for name, on in legs:
                ms, w = run_leg(tso if on else plain, on, batches, per)
                work = w or work
                best[name] = min(best.get(name, ms), ms)
                print(json.dumps({"tool": "bench_ts_order", "law": law, "leg": name, "round": rnd, "partitions": P, "records": n,
                                  "batches": len(batches), "steps": args.steps, "ms": round(ms, 4),
                                  "records_per_s": round(n / (ms * 1e-3))}), flush=True)
        # one pass over the topic from a fresh state: the law's own figures
        tso.reset()
        for i, b in enumerate(batches):
            tso.submit_device(b, per, i * per, which=1)
        v = tso.ts_order()
    line = {"tool": "bench_ts_order", "law": law, "records": n, "partitions": P, "algorithmic_bytes_per_record": 12,
            "best_ms": {k: round(x, 4) for k, x in best.items()}, "work_per_pass": work, "timed": v["timed"],
            "late": int(v["late"].sum()), "max_late_ms": int(v["max_late_ms"].max())}
    if "scan" in best:
        d = best["scan+ts_order"] - best["scan"]
        tbs = alg_bytes / (d * 1e-3) / 1e12 if d > 0 else None
        line.update({"pass_ms": round(d, 4), "pass_TBps": tbs and round(tbs, 3), "pass_roofline_frac": tbs and round(tbs / ROOFLINE_TBS, 4),
                     "roofline_ms": round(alg_bytes / (ROOFLINE_TBS * 1e12) * 1e3, 4),
                     "ratio_scan_pass_over_scan": round(best["scan+ts_order"] / best["scan"], 4)})
    print(json.dumps(line), flush=True)
    for b in batches:
        owner.device_batch_free(b)
    owner.close()

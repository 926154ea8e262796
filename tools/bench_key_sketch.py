"""What the key sketch (KTA_FLAG_KEY_SKETCH) costs: 2^30 records (by default) resident in HBM on one GPU as tile-compact
batches, the metrics handler (which = 1) timed by wall clock around whole passes over all batches, by a context without
the flag (the scan alone) and one with it (scan + sketch), alternated round after round in one process.  Two shapes:

    c3   16 B keys, 64 partitions, 10 M distinct keys (batches of 2^27 records)
    c4   config 4's mixed key lengths 8..200 B, 256 partitions, 100 M distinct keys (batches of 2^25 records)

    python tools/bench_key_sketch.py [--log2-records 30] [--steps 5] [--warmup 1] [--rounds 2] [--shapes c3,c4]
                                     [--sketch-only]

Prints one JSON line per shape, leg and round, and per shape a last line: the sketch's share (best scan + sketch minus
best scan alone), its TB/s of algorithmic bytes (partition 2 B in a compact tile + key_len 4 + key_off 4 + the key bytes)
and fraction of the 8 TB/s roofline, and the sketch kernel's work counters of one warm pass (kta_key_sketch_info: keyed
records, reads of a register past the LDS floor, atomics).  --sketch-only runs the sketch leg alone (one context, no
alternation), for a `rocprofv3 --kernel-trace --stats` run of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import kafka_topic_analyzer_amd as kta  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-records", type=int, default=30)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--shapes", default="c3,c4")
ap.add_argument("--sketch-only", action="store_true")
args = ap.parse_args()

ROOFLINE_TBS = 8.0
n = 1 << args.log2_records
SHAPES = {"c3": (27, 16), "c4": (25, 72)}   # log2 records per batch, key bytes per record allotted


def run_leg(h, batches, per):
    for _ in range(args.warmup):
        for i, b in enumerate(batches):
            h.submit_device(b, per, i * per, which=1)
    h.sync()
    before = h.key_sketch_info() if h.key_sketch_on else None
    t0 = time.perf_counter()
    for _ in range(args.steps):
        for i, b in enumerate(batches):
            h.submit_device(b, per, i * per, which=1)
    h.sync()
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    work = None
    if before:
        after = h.key_sketch_info()
        work = {k: (after[k] - before[k]) // args.steps for k in ("keyed", "reads", "atomics", "launches")}
    return ms, work


for shape in args.shapes.split(","):
    spec, _ = kta.synth_preset(shape)
    P = int(spec.n_partitions)
    log2_per, kb_per = SHAPES[shape]
    per = min(n, 1 << log2_per)
    owner = kta.HipMetricHandler(P)
    batches, key_bytes = [], 0
    for lo in range(0, n, per):
        b = owner.device_batch_alloc(per, kb_per * per + 16)
        key_bytes += owner.synth_fill_device(spec, lo, per, b)
        batches.append(b)
    owner.sync()
    alg_bytes = n * (2 + 4 + 4) + key_bytes
    legs = (("scan+sketch", True),) if args.sketch_only else (("scan", False), ("scan+sketch", True))
    best, work = {}, None
    with kta.HipMetricHandler(P) as plain, kta.HipMetricHandler(P, key_sketch=True) as sk:
        for rnd in range(args.rounds):
            for name, on in legs:
                ms, w = run_leg(sk if on else plain, batches, per)
                work = w or work
                best[name] = min(best.get(name, ms), ms)
                print(json.dumps({"tool": "bench_key_sketch", "shape": shape, "leg": name, "round": rnd, "partitions": P,
                                  "records": n, "batches": len(batches), "steps": args.steps, "ms": round(ms, 4),
                                  "records_per_s": round(n / (ms * 1e-3))}), flush=True)
        _, c = plain.finish() if not args.sketch_only else sk.finish()
        est, topic = kta.estimate_distinct_keys(sk.key_sketch(), P)
    line = {"tool": "bench_key_sketch", "shape": shape, "records": n, "mean_key_bytes": round(key_bytes / n, 3),
            "algorithmic_bytes_per_record": round(alg_bytes / n, 3), "best_ms": {k: round(v, 4) for k, v in best.items()},
            "sketch_work_per_pass": work, "topic_estimate": round(topic)}
    if "scan" in best:
        d = best["scan+sketch"] - best["scan"]
        tbs = alg_bytes / (d * 1e-3) / 1e12 if d > 0 else None
        line.update({"sketch_ms": round(d, 4), "sketch_TBps": tbs and round(tbs, 3),
                     "sketch_roofline_frac": tbs and round(tbs / ROOFLINE_TBS, 4),
                     "ratio_scan_sketch_over_scan": round(best["scan+sketch"] / best["scan"], 4)})
    print(json.dumps(line), flush=True)
    for b in batches:
        owner.device_batch_free(b)
    owner.close()

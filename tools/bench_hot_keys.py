"""What the hot-key sketch (KTA_FLAG_HOT_KEYS) costs: 2^30 records (by default) resident in HBM on one GPU as tile-compact
batches, the metrics handler (which = 1) timed by wall clock around whole passes over all batches, by a context without a
flag (the scan alone), one with the key sketch (scan + kta_key_sketch: the yardstick) and one with the hot keys (scan +
kta_hot_keys), alternated round after round in one process.  Shapes:

    c3    16 B keys, 64 partitions, 10 M distinct keys (batches of 2^27 records)
    c4    config 4's mixed key lengths 8..200 B, 256 partitions, 100 M distinct keys (batches of 2^25 records)
    one   the c3 shape with one key
    k40   the c3 shape with 40 keys
    zipf  16 B keys drawn from 2^20 keys by a Zipf law (s = 1.1), one batch of 2^26 records built on the host and
          submitted 2^30 / 2^26 times per pass (its key bytes are the 16 MiB table of the distinct keys, so the key
          reads of this shape mostly hit the caches)

    python tools/bench_hot_keys.py [--log2-records 30] [--steps 5] [--warmup 1] [--rounds 2]
                                   [--shapes c3,c4,one,k40,zipf] [--hot-only]

Prints one JSON line per shape, leg and round, and per shape a last line: the pass's share (best scan + hot keys minus
best scan alone), its TB/s of algorithmic bytes (partition 2 B in a compact tile + key_len 4 + key_off 4 + the key
bytes) and fraction of the 8 TB/s roofline, the same for the key sketch, the ratio of the two, and the pass's work
counters of one warm pass (kta_hot_keys_info).  --hot-only runs the hot-key leg alone (one context, no alternation),
for a `rocprofv3 --kernel-trace --stats` run of its own."""
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
ap.add_argument("--shapes", default="c3,c4,one,k40,zipf")
ap.add_argument("--hot-only", action="store_true")
args = ap.parse_args()

ROOFLINE_TBS = 8.0
n = 1 << args.log2_records
SHAPES = {"c3": ("c3", 27, 16, None), "c4": ("c4", 25, 72, None), "one": ("c3", 27, 16, 1), "k40": ("c3", 27, 16, 40),
          "zipf": ("c3", 26, 16, None)}   # preset, log2 records per batch, key bytes per record allotted, distinct keys
INFO = ("keyed", "groups", "flushes", "launches", "exemplars", "workgroups")


def zipf_columns(per, P, keys_log2=20, s=1.1, seed=5):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, (1 << keys_log2) + 1) ** s
    ids = np.searchsorted(np.cumsum(w / w.sum()), rng.random(per)).clip(0, (1 << keys_log2) - 1)
    ids = rng.permutation(1 << keys_log2)[ids]                 # the heavy keys anywhere in the table
    return {"partition": (ids % P).astype(np.int32), "key_len": np.full(per, 16, np.int32),
            "val_len": np.full(per, 100, np.int32), "ts_ms": np.full(per, 1_600_000_000_000, np.int64),
            "key_off": (ids * 16).astype(np.uint32),
            "key_bytes": rng.integers(0, 256, size=16 << keys_log2, dtype=np.uint8)}


def run_leg(h, batches, per, reps):
    def one_pass():
        for r in range(reps):
            for i, b in enumerate(batches):
                h.submit_device(b, per, (r * len(batches) + i) * per, which=1)
    for _ in range(args.warmup):
        one_pass()
    h.sync()
    before = h.hot_keys_info() if h.hot_keys_on else None
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one_pass()
    h.sync()
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    work = None
    if before:
        after = h.hot_keys_info()
        work = {k: (after[k] - before[k]) // args.steps for k in INFO}
    return ms, work


for shape in args.shapes.split(","):
    preset, log2_per, kb_per, distinct = SHAPES[shape]
    spec, _ = kta.synth_preset(preset)
    if distinct:
        spec.n_distinct_keys = distinct
    P = int(spec.n_partitions)
    per = min(n, 1 << log2_per)
    owner = kta.HipMetricHandler(P)
    batches, key_bytes, reps = [], 0, 1
    if shape == "zipf":
        b, _ = owner.upload_batch(zipf_columns(per, P), with_keys=True)
        batches, key_bytes, reps = [b], 16 * n, n // per
    else:
        for lo in range(0, n, per):
            b = owner.device_batch_alloc(per, kb_per * per + 16)
            key_bytes += owner.synth_fill_device(spec, lo, per, b)
            batches.append(b)
    owner.sync()
    alg_bytes = n * (2 + 4 + 4) + key_bytes
    legs = (("scan+hot", "hot"),) if args.hot_only else (("scan", "plain"), ("scan+sketch", "sketch"), ("scan+hot", "hot"))
    best, work = {}, None
    with kta.HipMetricHandler(P) as plain, kta.HipMetricHandler(P, key_sketch=True) as sk, \
            kta.HipMetricHandler(P, hot_keys=True) as hot:
        ctxs = {"plain": plain, "sketch": sk, "hot": hot}
        for rnd in range(args.rounds):
            for name, which in legs:
                ms, w = run_leg(ctxs[which], batches, per, reps)
                work = w or work
                best[name] = min(best.get(name, ms), ms)
                print(json.dumps({"tool": "bench_hot_keys", "shape": shape, "leg": name, "round": rnd, "partitions": P,
                                  "records": n, "batches": len(batches) * reps, "steps": args.steps, "ms": round(ms, 4),
                                  "records_per_s": round(n / (ms * 1e-3))}), flush=True)
        found, keyed = kta.recover_hot_keys(hot.hot_keys(), 5)
    line = {"tool": "bench_hot_keys", "shape": shape, "records": n, "mean_key_bytes": round(key_bytes / n, 3),
            "algorithmic_bytes_per_record": round(alg_bytes / n, 3), "best_ms": {k: round(v, 4) for k, v in best.items()},
            "hot_work_per_pass": work, "reported": len(found), "heaviest_share": round(found[0][1] / keyed, 5) if found else None}
    if "scan" in best:
        for leg, tag in (("scan+hot", "hot"), ("scan+sketch", "sketch")):
            d = best[leg] - best["scan"]
            tbs = alg_bytes / (d * 1e-3) / 1e12 if d > 0 else None
            line.update({tag + "_ms": round(d, 4), tag + "_TBps": tbs and round(tbs, 3),
                         tag + "_roofline_frac": tbs and round(tbs / ROOFLINE_TBS, 4)})
        if line["sketch_ms"] > 0:
            line["hot_over_sketch"] = round(line["hot_ms"] / line["sketch_ms"], 3)
    print(json.dumps(line), flush=True)
    for b in batches:
        owner.device_batch_free(b)
    owner.close()

"""What the partitioner pass (KTA_FLAG_PARTITIONER) costs: records resident in HBM on one GPU as tile-compact batches,
the metrics handler (which = 1) timed by wall clock around whole passes over all batches, by a context without a flag
(the scan alone), one with the key sketch (scan + kta_key_sketch), one with the hot keys (scan + kta_hot_keys) — the two
yardsticks — and one with the partitioner (scan + kta_partitioner), alternated round after round in ONE process.  Shapes:

    c3    16 B keys, 64 partitions, 10 M distinct keys, 2^30 records (batches of 2^27)
    c4    config 4's mixed key lengths 8..200 B, 256 partitions, 100 M distinct keys, 2^30 records (batches of 2^25)
    one   the c3 shape with one key, 2^26 records

    python tools/bench_partitioner.py [--log2-records 30] [--steps 5] [--warmup 1] [--rounds 2] [--shapes c3,c4,one]
                                      [--repartition Q] [--pass-only]

Prints one JSON line per shape, leg and round, and per shape a last line: each pass's share (best scan + pass minus best
scan alone), the partitioner's TB/s of algorithmic bytes (partition 2 B in a compact tile + key_len 4 + key_off 4 +
val_len 4 + the key bytes) and its fraction of the 8 TB/s roofline, its ns per record, its ratio to the two yardsticks and
its work counters of one warm pass (kta_partitioner_info).  --pass-only runs the partitioner leg alone (one context, no
alternation), for a `rocprofv3 --kernel-trace --stats` run of its own.  Only legs of one process compare."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import kafka_topic_analyzer_amd as kta  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-records", type=int, default=30)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--shapes", default="c3,c4,one")
ap.add_argument("--repartition", type=int, default=0, help="the what-if partition count Q (0: the topic's P)")
ap.add_argument("--pass-only", action="store_true")
args = ap.parse_args()

ROOFLINE_TBS = 8.0
# preset, log2 records at most, log2 records per batch, key bytes per record allotted, distinct keys
SHAPES = {"c3": ("c3", 30, 27, 16, None), "c4": ("c4", 30, 25, 72, None), "one": ("c3", 26, 26, 16, 1)}
INFO = ("keyed_records", "launches", "partition_adds", "target_adds", "workgroups")


def run_leg(h, batches, per, is_pass):
    def one_pass():
        for i, b in enumerate(batches):
            h.submit_device(b, per, i * per, which=1)
    for _ in range(args.warmup):
        one_pass()
    h.sync()
    before = h.partitioner_info() if is_pass else None
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one_pass()
    h.sync()
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    work = None
    if before:
        after = h.partitioner_info()
        work = {k: (after[k] - before[k]) // args.steps for k in INFO}
        work["lds_bytes"] = after["lds_bytes"]
    return ms, work


for shape in args.shapes.split(","):
    preset, log2_max, log2_per, kb_per, distinct = SHAPES[shape]
    spec, _ = kta.synth_preset(preset)
    if distinct:
        spec.n_distinct_keys = distinct
    P = int(spec.n_partitions)
    Q = args.repartition or P
    n = 1 << min(args.log2_records, log2_max)
    per = min(n, 1 << log2_per)
    owner = kta.HipMetricHandler(P)
    batches, key_bytes = [], 0
    for lo in range(0, n, per):
        b = owner.device_batch_alloc(per, kb_per * per + 16)
        key_bytes += owner.synth_fill_device(spec, lo, per, b)
        batches.append(b)
    owner.sync()
    alg_bytes = n * (2 + 4 + 4 + 4) + key_bytes
    legs = (("scan+partitioner", "part"),) if args.pass_only else \
        (("scan", "plain"), ("scan+sketch", "sketch"), ("scan+hot", "hot"), ("scan+partitioner", "part"))
    best, work = {}, None
    with kta.HipMetricHandler(P) as plain, kta.HipMetricHandler(P, key_sketch=True) as sk, \
            kta.HipMetricHandler(P, hot_keys=True) as hot, kta.HipMetricHandler(P, partitioner=True, repartition=Q) as part:
        ctxs = {"plain": plain, "sketch": sk, "hot": hot, "part": part}
        for rnd in range(args.rounds):
            for name, which in legs:
                ms, w = run_leg(ctxs[which], batches, per, which == "part")
                work = w or work
                best[name] = min(best.get(name, ms), ms)
                print(json.dumps({"tool": "bench_partitioner", "shape": shape, "leg": name, "round": rnd, "partitions": P,
                                  "repartition": Q, "records": n, "batches": len(batches), "steps": args.steps,
                                  "ms": round(ms, 4), "records_per_s": round(n / (ms * 1e-3))}), flush=True)
        v = part.partitioner()
    line = {"tool": "bench_partitioner", "shape": shape, "records": n, "partitions": P, "repartition": Q,
            "mean_key_bytes": round(key_bytes / n, 3), "algorithmic_bytes_per_record": round(alg_bytes / n, 3),
            "best_ms": {k: round(x, 4) for k, x in best.items()}, "partitioner_work_per_pass": work,
            "placed_share": round(int(v["placed"].sum()) / max(int(v["checked"].sum()), 1), 5)}
    if "scan" in best:
        for leg, tag in (("scan+partitioner", "partitioner"), ("scan+sketch", "sketch"), ("scan+hot", "hot")):
            line[tag + "_ms"] = round(best[leg] - best["scan"], 4)
        d = line["partitioner_ms"]
        if d > 0:
            tbs = alg_bytes / (d * 1e-3) / 1e12
            line.update({"partitioner_TBps": round(tbs, 3), "partitioner_roofline_frac": round(tbs / ROOFLINE_TBS, 4),
                         "partitioner_ns_per_record": round(d * 1e6 / n, 5)})
        for tag in ("sketch", "hot"):
            if line[tag + "_ms"] > 0:
                line["partitioner_over_" + tag] = round(d / line[tag + "_ms"], 3)
    print(json.dumps(line), flush=True)
    for b in batches:
        owner.device_batch_free(b)
    owner.close()

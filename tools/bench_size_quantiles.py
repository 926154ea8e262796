"""What the size-percentile pass (KTA_FLAG_SIZE_QUANTILES) costs: config 4's records resident in HBM on one GPU as keyless
tile-compact batches (6 B per record for this pass), the metrics handler (which = 1) timed by wall clock around whole passes
over all batches, alternated round after round in ONE process:

    scan256 / scan12              a context without the flag, 256 and 12 partitions: the plain step
    scan+sizeq256                 256 partitions: ceil(256 / S) slices as the grid's second dimension
    scan+sizeq256-serial          the same, one launch per slice (KTA_SIZEQ_VARIANT=1)
    scan+loads256                 the same grid, the loads alone (KTA_SIZEQ_VARIANT=9)
    scan+sizeq12 / scan+loads12   the same records with a 12-partition handler: one slice (partitions 12 .. 255 are
                                  counted as bad-partition records and binned nowhere)

    python tools/bench_size_quantiles.py [--log2-records 30] [--steps 5] [--warmup 1] [--rounds 3] [--slice S]

Prints one JSON line per leg and round, and a last line: each pass's share (best scan + pass minus best scan alone), the
pass's own bound (the loads-only share: slices x 6 B per record at the rate the loads run at), how far above it the pass
stands, and the plan and the LDS adds of one warm pass (kta_size_quantiles_info).  Only legs of one process compare."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import kafka_topic_analyzer_amd as kta  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-records", type=int, default=30)
ap.add_argument("--log2-batch", type=int, default=25)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--slice", type=int, default=0, help="a forced S (0: the plan's)")
args = ap.parse_args()

BYTES_PER_RECORD = 6   # u16 partition + u16 key_len + u16 val_len of a compact tile with u16 lengths


def context(P, sizeq, variant=0):
    """KTA_SIZEQ_VARIANT is read when the context is created"""
    os.environ["KTA_SIZEQ_VARIANT"] = str(variant)
    h = kta.HipMetricHandler(P, size_quantiles=sizeq)
    os.environ.pop("KTA_SIZEQ_VARIANT")
    if sizeq and args.slice:
        h.set_size_quantiles_slice(args.slice)
    return h


def run_leg(h, batches, per):
    def one_pass():
        for i, b in enumerate(batches):
            h.submit_device(b, per, i * per, which=1)
    for _ in range(args.warmup):
        one_pass()
    h.sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one_pass()
    h.sync()
    return (time.perf_counter() - t0) * 1e3 / args.steps


spec, _ = kta.synth_preset("c4")
n = 1 << args.log2_records
per = min(n, 1 << args.log2_batch)
owner = kta.HipMetricHandler(int(spec.n_partitions))
batches = []
for lo in range(0, n, per):
    b = owner.device_batch_alloc(per, 0)
    owner.synth_fill_device(spec, lo, per, b)
    batches.append(b)
owner.sync()

LEGS = (("scan256", 256, False, 0), ("scan+sizeq256", 256, True, 0), ("scan+sizeq256-serial", 256, True, 1), ("scan+loads256", 256, True, 9),
        ("scan12", 12, False, 0), ("scan+sizeq12", 12, True, 0), ("scan+loads12", 12, True, 9))
ctxs = {name: context(P, sizeq, variant) for name, P, sizeq, variant in LEGS}
best = {}
for rnd in range(args.rounds):
    for name, P, _, _ in LEGS:
        ms = run_leg(ctxs[name], batches, per)
        best[name] = min(best.get(name, ms), ms)
        print(json.dumps({"tool": "bench_size_quantiles", "leg": name, "round": rnd, "partitions": P, "records": n, "batches": len(batches),
                          "steps": args.steps, "ms": round(ms, 4), "records_per_s": round(n / (ms * 1e-3))}), flush=True)
line = {"tool": "bench_size_quantiles", "records": n, "best_ms": {k: round(x, 4) for k, x in best.items()}}
for tag, P in (("256", 256), ("12", 12)):
    h = ctxs["scan+sizeq" + tag]
    before = h.size_quantiles_info()
    for i, b in enumerate(batches):
        h.submit_device(b, per, i * per, which=1)
    info = h.size_quantiles_info()
    info["lds_adds"] -= before["lds_adds"]
    d, ld = best["scan+sizeq" + tag] - best["scan" + tag], best["scan+loads" + tag] - best["scan" + tag]
    line["sizeq%s_plan_and_work" % tag] = info
    line["sizeq%s_ms" % tag], line["loads%s_ms" % tag] = round(d, 4), round(ld, 4)
    if ld > 0 and d > 0:
        line["loads%s_TBps" % tag] = round(info["slices"] * BYTES_PER_RECORD * n / (ld * 1e-3) / 1e12, 3)
        line["sizeq%s_over_its_loads" % tag] = round(d / ld, 3)
        line["sizeq%s_ns_per_record" % tag] = round(d * 1e6 / n, 5)
line["sizeq256_serial_ms"] = round(best["scan+sizeq256-serial"] - best["scan256"], 4)
print(json.dumps(line), flush=True)
for h in ctxs.values():
    h.close()
for b in batches:
    owner.device_batch_free(b)
owner.close()

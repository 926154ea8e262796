"""The metrics scan of config 4 on its own, in the shapes bench.py does not offer: 2^30 records (by default) resident in HBM
on one GPU as keyless tile-compact batches, reset + scan + fold per step, the scan and the fold timed with the library's
timing hooks (kta_set_timing / kta_kernel_time_stats; the scan's pair spans every kernel the scan launches), the step
by wall clock around the timed steps.

    python tools/bench_scan.py [--lib FILE] [--scan-variant V] [--workgroups-per-cu W] [--handler-partitions P]
                               [--cut] [--part-mode random|runs] [--long-key BYTES] [--steps 20] [--preroll 155] [--tag TEXT]

--lib: another build of the library (tools/build_variant.sh).  --handler-partitions 200: a handler of 200 partitions over
config 4's 256, so that no tile's summary applies.  --cut: the batch viewed from record 4 to n - 37 — a cut first and last
tile around summarised ones.  --scan-variant 80 (16 + 64): the plane marks are ignored, every summarised tile is read in
its u16 form (`plane`: off).  --long-key 300: config 4's longest key length becomes 300 bytes, which no scan plane holds
(`marked_tiles`: how many of the batch's `tiles` have a plane).  One JSON line."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--log2-records", type=int, default=30)
ap.add_argument("--scan-variant", type=int, default=16)
ap.add_argument("--workgroups-per-cu", type=int, default=0)
ap.add_argument("--handler-partitions", type=int, default=256)
ap.add_argument("--cut", action="store_true")
ap.add_argument("--part-mode", choices=["random", "runs"], default="random")
ap.add_argument("--long-key", type=int, default=0)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--preroll", type=int, default=155)
ap.add_argument("--tag", default="")
args = ap.parse_args()
if args.lib:
    os.environ["KTA_LIB_PATH"] = os.path.abspath(args.lib)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402
import kafka_topic_analyzer_amd as kta  # noqa: E402
from kafka_topic_analyzer_amd import _native as N  # noqa: E402

n, P = 1 << args.log2_records, args.handler_partitions
spec, _ = kta.synth_preset("c4")
if args.part_mode == "runs":
    spec.part_mode, spec.part_run_len = N.KTA_PART_RUNS, 500
if args.long_key:
    spec.key_lens[spec.n_key_lens - 1] = args.long_key
cus = torch.cuda.get_device_properties(0).multi_processor_count
with kta.HipMetricHandler(P) as h:
    h.set_tuning(scan_workgroups=args.workgroups_per_cu * cus, scan_variant=args.scan_variant)
    batch = h.device_batch_alloc(n)
    h.synth_fill_device(spec, 0, n, batch)
    marks = h.batch_tile_planes(batch, n)
    lo, m = (4, n - 4 - 37) if args.cut else (0, n)
    view = kta.KtaBatch()
    for f, sz in (("partition", 4), ("key_len", 4), ("val_len", 4), ("ts_ms", 8)):
        setattr(view, f, getattr(batch, f) + lo * sz)
    b = view if args.cut else batch

    def step():
        h.reset()
        h.submit_device(b, m, 0, which=1)

    for _ in range(args.preroll):
        step()
    h.sync()
    h.kernel_time_stats()                                    # drain what the pre-roll recorded
    h.set_timing(True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    h.sync()
    wall = (time.perf_counter() - t0) * 1e3 / args.steps
    avg, launches = h.kernel_time_stats()
    h.set_timing(False)
    res, _ = h.finish(allow_bad_partition=True)
    print(json.dumps({"tool": "bench_scan", "tag": args.tag, "lib": args.lib, "records": m, "handler_partitions": P,
                      "part_mode": args.part_mode, "cut": args.cut, "long_key": args.long_key, "scan_variant": args.scan_variant,
                      "plane": "off" if args.scan_variant & 64 else "on", "tiles": int(marks.size), "marked_tiles": int(marks.sum()),
                      "workgroups_per_cu": args.workgroups_per_cu or "plan", "steps": args.steps, "preroll_steps": args.preroll,
                      "kernel_ms": round(avg[0], 4), "fold_kernel_ms": round(avg[1], 4), "ms_per_step_wall": round(wall, 4),
                      "overall_count": int(res.overall_count), "bad_partition_records": int(res.bad_partition_records)}), flush=True)
    h.device_batch_free(batch)

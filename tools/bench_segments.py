"""What the segment pass of the retention what-if (kta_set_segments) costs, next to the timestamp-order pass measured in the
same call: 2^30 records (by default) resident in HBM on one GPU as keyless tile-compact batches, the metrics handler
(which = 1) timed by wall clock around whole passes over all batches, by a context without any pass (the scan alone), one
with KTA_FLAG_TS_ORDER, and one with segments for every S given — alternated round after round in one process.  Three laws:

    c4          config 4 as it is: random partitions
    c4-ordered  config 4 with KTA_PART_RUNS, run length 500, ts_jitter_ms = 0: the one-partition path
    c3          config 3

    python tools/bench_segments.py [--log2-records 30] [--log2-batch 27] [--steps 5] [--warmup 1] [--rounds 2]
                                   [--laws c4,c4-ordered,c3] [--segment-bytes 1073741824,auto] [--rows 1024]

S = 1 GiB is a broker's default segment.bytes: all but a handful of chunks close no row and the apply kernel leaves them at
once.  S = auto exposes the wave step: the smallest S at which no partition outgrows its M rows within one pass over the
topic (from a probe pass's totals), so that rows close in nearly every chunk of every pass — a fixed small S such as 4 KiB
fills the M rows within the first batch, after which nothing closes and every chunk is skipped.  Every timed pass starts
from a reset context (the reset and a wait are outside the clock), for the same reason, in every leg.  Prints one JSON line per law, leg and round, and
per law a last line: every pass's share (best scan + pass minus best scan alone), the segment pass's TB/s of algorithmic
bytes — (2 + 4 + 4) B per record of a compact tile with u16 lengths, read by the chunk sums and again by the apply kernel
in the chunks it does not skip — and fraction of the 8 TB/s roofline, and the pass's work counters of one warm pass
(kta_segments_info)."""
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
ap.add_argument("--segment-bytes", default="1073741824,auto")
ap.add_argument("--rows", type=int, default=1024)
args = ap.parse_args()

ROOFLINE_TBS = 8.0
RECORD_BYTES = 2 + 4 + 4     # partition u16, timestamp offset i32, a u16 key length and a u16 value length
n = 1 << args.log2_records
INFO = ("chunks", "launches", "chunks_applied", "chunks_skipped", "groups")


def law_spec(law):
    spec, _ = kta.synth_preset("c3" if law == "c3" else "c4")
    if law == "c4-ordered":
        spec.part_mode, spec.part_run_len, spec.ts_jitter_ms = N.KTA_PART_RUNS, 500, 0
    return spec


def run_leg(h, seg, batches, per):
    for _ in range(args.warmup):
        for i, b in enumerate(batches):
            h.submit_device(b, per, i * per, which=1)
    h.sync()
    ms, work = 0.0, None
    for _ in range(args.steps):
        h.reset()
        h.sync()
        t0 = time.perf_counter()
        for i, b in enumerate(batches):
            h.submit_device(b, per, i * per, which=1)
        h.sync()
        ms += (time.perf_counter() - t0) * 1e3 / args.steps
    if seg:   # (of the last pass: the counters start at every reset)
        info = h.segments_info()
        work = {k: info[k] for k in INFO}
        work["chunk_records"] = info["chunk_records"]
    return ms, work


for law in args.laws.split(","):
    spec = law_spec(law)
    P = int(spec.n_partitions)
    M = min(args.rows, (1 << 20) // P)
    per = min(n, 1 << args.log2_batch)
    owner = kta.HipMetricHandler(P)
    batches = []
    for lo in range(0, n, per):
        b = owner.device_batch_alloc(per)
        owner.synth_fill_device(spec, lo, per, b)
        batches.append(b)
    owner.sync()
    sizes = []
    for s in args.segment_bytes.split(","):
        if s != "auto":
            sizes.append(int(s))
            continue
        with kta.HipMetricHandler(P, segments=(1 << 40, 2, 0)) as probe:   # the partitions' bytes of one pass
            for i, b in enumerate(batches):
                probe.submit_device(b, per, i * per, which=1)
            sizes.append(int(probe.segments()["totals"][:, 1].max()) // (M - 2) + 1)
    legs = {"scan": kta.HipMetricHandler(P), "scan+ts_order": kta.HipMetricHandler(P, ts_order=True)}
    for S in sizes:
        legs["scan+segments(S=%d)" % S] = kta.HipMetricHandler(P, segments=(S, M, 0))
    best, work = {}, {}
    for rnd in range(args.rounds):
        for name, h in legs.items():
            ms, w = run_leg(h, "segments" in name, batches, per)
            if w:
                work[name] = w
            best[name] = min(best.get(name, ms), ms)
            print(json.dumps({"tool": "bench_segments", "law": law, "leg": name, "round": rnd, "partitions": P, "records": n,
                              "batches": len(batches), "steps": args.steps, "ms": round(ms, 4),
                              "records_per_s": round(n / (ms * 1e-3))}), flush=True)
    line = {"tool": "bench_segments", "law": law, "records": n, "partitions": P, "rows_per_partition": M,
            "best_ms": {k: round(x, 4) for k, x in best.items()}, "pass_ms": {}, "segments": {}}
    for name in legs:
        if name == "scan":
            continue
        d = best[name] - best["scan"]
        line["pass_ms"][name] = round(d, 4)
        if "segments" not in name:
            continue
        w = work[name]
        read = n * RECORD_BYTES * (1.0 + (w["chunks_applied"] / w["chunks"] if w["chunks"] else 0.0))
        tbs = read / (d * 1e-3) / 1e12 if d > 0 else None
        # one pass over the topic from a fresh state: the rows closed
        h = legs[name]
        h.reset()
        for i, b in enumerate(batches):
            h.submit_device(b, per, i * per, which=1)
        g = h.segments()["globals"]
        line["segments"][name] = {"work_per_pass": w, "algorithmic_bytes": int(read), "pass_TBps": tbs and round(tbs, 3),
                                  "pass_roofline_frac": tbs and round(tbs / ROOFLINE_TBS, 4),
                                  "roofline_ms": round(read / (ROOFLINE_TBS * 1e12) * 1e3, 4), "rows_closed": int(g[2]),
                                  "ratio_to_ts_order": round(d / (best["scan+ts_order"] - best["scan"]), 4)
                                  if best["scan+ts_order"] > best["scan"] else None}
    print(json.dumps(line), flush=True)
    for h in legs.values():
        h.close()
    for b in batches:
        owner.device_batch_free(b)
    owner.close()

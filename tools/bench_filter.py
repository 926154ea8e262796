"""What the record filter (kta_set_filter) costs and saves: config 4 (256 partitions) resident in HBM on one GPU as keyless
tile-compact batches of 2^26 records (the filter's slice), the metrics handler (which = 1)
timed by wall clock around whole passes over all batches.  ONE context takes every leg — kta_reset, then kta_set_filter,
which a context accepts again after a reset — so the tiles' summaries are the context's own, and the legs alternate round
after round in one process:

    unfiltered   no filter: the yardstick, the step of a context that was never filtered
    everything   a window over every timestamp: every whole tile passes by its summary, every slice is handed on as it is
    eighth       a window over about 1/8 of the timestamps' range
    nothing      a window before every timestamp: every whole tile is rejected from its 24 bytes of header and summary
    partition    one partition of the 256, no window: every tile is read, about 1/256 of the records pass

    python tools/bench_filter.py [--log2-records 30] [--steps 5] [--warmup 1] [--rounds 3] [--out profiles/filter_bench.jsonl]
                                 [--jitter-ms J] [--ts-missing-permille M] [--append]

Config 4 stamps record i with base + i * 10 us and a jitter of +- one hour, and leaves one timestamp in a thousand out: a
tile's 1024 timestamps then span about two hours whatever the window, and most tiles hold a record without a timestamp, so
summaries decide few of its tiles.  --jitter-ms 0 --ts-missing-permille 0 gives the same topic with timestamps in log order
(what a broker's LogAppendTime produces), where they decide nearly all; --append adds that run's lines to --out.

Prints (and writes to --out) one JSON line per leg and round — step ms, kta_filter_info of one step, the fraction of tiles
decided by summary — and a last line with the best step of every leg next to the unfiltered one.  filter_bytes_per_record_seen
is the filter's own algorithmic traffic per record it was shown, from kta_filter_info: 24 B per tile decided by summary;
6 B per record of a tile the count kernel read (u16 partition + i32 timestamp offset); per passing record that the scatter
moved 6 + 4 B read (the u16 lengths) and 20 B written; a slice handed on as it is moves nothing.  The passes behind the
filter then read the scratch batch (20 B per passing record, raw layout) or, for a slice handed on, the tiles as always."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import kafka_topic_analyzer_amd as kta  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-records", type=int, default=30)
ap.add_argument("--log2-batch", type=int, default=26)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--jitter-ms", type=int, default=None)
ap.add_argument("--ts-missing-permille", type=int, default=None)
ap.add_argument("--append", action="store_true")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "filter_bench.jsonl"))
args = ap.parse_args()

n = 1 << args.log2_records
per = min(n, 1 << args.log2_batch)
spec, _ = kta.synth_preset("c4")
P = int(spec.n_partitions)
if args.jitter_ms is not None:
    spec.ts_jitter_ms = args.jitter_ms
if args.ts_missing_permille is not None:
    spec.ts_missing_permille = args.ts_missing_permille
TOPIC = {"ts_jitter_ms": int(spec.ts_jitter_ms), "ts_missing_permille": int(spec.ts_missing_permille)}
lo = int(spec.ts_base_ms) - int(spec.ts_jitter_ms) - 1
hi = int(spec.ts_base_ms) + (n * int(spec.ts_step_us)) // 1000 + int(spec.ts_jitter_ms) + 1
span = hi - lo
LEGS = [("unfiltered", (None, None, None)), ("everything", (lo - 10**6, hi + 10**6, None)),
        ("eighth", (lo + span * 3 // 8, lo + span * 4 // 8, None)), ("nothing", (1, 2, None)), ("partition", (None, None, [7]))]
INFO = ("seen", "passed", "tiles_summary_none", "tiles_summary_all", "tiles_read", "slices")
out_lines = []


def emit(line):
    print(json.dumps(line), flush=True)
    out_lines.append(json.dumps(line))


with kta.HipMetricHandler(P) as h:
    batches = []
    for first in range(0, n, per):
        b = h.device_batch_alloc(per, 0)
        h.synth_fill_device(spec, first, per, b)
        batches.append(b)
    h.sync()

    def one_pass():
        for i, b in enumerate(batches):
            h.submit_device(b, per, i * per, which=1)

    best, last = {}, {}
    for rnd in range(args.rounds):
        for name, (frm, to, parts) in LEGS:
            h.reset()
            h.set_filter(frm, to, parts)
            for _ in range(args.warmup):
                one_pass()
            h.sync()
            before = h.filter_info()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                one_pass()
            h.sync()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            after = h.filter_info()
            info = {k: (after[k] - before[k]) // args.steps for k in INFO}
            tiles = info["tiles_summary_none"] + info["tiles_summary_all"] + info["tiles_read"]
            handed_on = info["passed"] == info["seen"]
            moved = 0 if handed_on else info["passed"]
            fbytes = 24 * tiles + 6 * 1024 * info["tiles_read"] + moved * (6 + 4 + 20)
            res, _ = h.finish()
            line = {"tool": "bench_filter", **TOPIC, "leg": name, "round": rnd, "partitions": P, "records": n, "batches": len(batches),
                    "steps": args.steps, "ms": round(ms, 4), "records_seen_per_s": round(n / (ms * 1e-3)), "filter_info": info,
                    "summary_tile_fraction": round((tiles - info["tiles_read"]) / tiles, 6) if tiles else None,
                    "filter_bytes_per_record_seen": round(fbytes / n, 4) if tiles else 0.0,
                    "records_counted": int(res.overall_count)}
            best[name] = min(best.get(name, ms), ms)
            last[name] = line
            emit(line)
    base = best["unfiltered"]
    emit({"tool": "bench_filter", **TOPIC, "summary": True, "records": n, "partitions": P, "batch_records": per,
          "best_ms": {k: round(v, 4) for k, v in best.items()},
          "over_unfiltered": {k: round(v / base, 4) for k, v in best.items()},
          "passed_fraction": {k: round(last[k]["filter_info"]["passed"] / n, 6) if k != "unfiltered" else 1.0 for k in best},
          "summary_tile_fraction": {k: last[k]["summary_tile_fraction"] for k in best if k != "unfiltered"},
          "filter_bytes_per_record_seen": {k: last[k]["filter_bytes_per_record_seen"] for k in best if k != "unfiltered"}})
    h.sync()
    for b in batches:
        h.device_batch_free(b)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a" if args.append else "w") as f:
    f.write("\n".join(out_lines) + "\n")

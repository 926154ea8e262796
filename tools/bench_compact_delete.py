"""What the compact,delete what-if (kta_set_compact_delete) adds to the compaction replay: config 3's shape as
tools/bench_compaction.py builds it — the sequence-numbered table (32 GiB), device-resident tile-compact batches with a seq
column, 16-byte keys, 64 partitions, 10 M distinct keys, 10 % tombstones — on one GPU, in ONE process, for every S given
(1 GiB, a broker's default segment.bytes, and `auto` as tools/bench_segments.py defines it: the smallest S at which no
partition outgrows its M rows within one pass, so that rows close in nearly every chunk).  Three legs, alternated
`--rounds` times:

    replay_off    the replay with the switch off: kta_compaction_survivors alone, as before
    replay_on     the replay with the switch on: the instantiation that also stores the class column, then the kept-row
                  triple (chunk sums, prefix, apply in flagged chunks)
    segment_pass  a first-pass segment pass: the metrics handler (which = 1) of a context with segments minus the same pass
                  of a context without (the scan alone), each from a reset context

    python tools/bench_compact_delete.py [--records 251658240] [--batches 5] [--steps 3] [--warmup 1] [--rounds 2]
                                         [--segment-bytes 1073741824,auto] [--rows 1024]

Every replay leg starts from a reset context and an untimed first pass (which = 3).  Prints one JSON line per S, leg and
round, and per S a last line: the best of every leg, replay_on - replay_off next to the segment pass — what the first
exceeds the second by is the class bytes' write and read (1 B per record each way) and the apply in flagged chunks —, the
kept-row kernels' work counters of one replay (kta_compact_delete_info), and the verdict of kta_compact_delete_whatif on the
three vectors (the identities hold)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import kafka_topic_analyzer_amd as kta  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--records", type=int, default=15 << 24, help="records per batch (bench.py's --alive-records)")
ap.add_argument("--batches", type=int, default=5)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--segment-bytes", default="1073741824,auto")
ap.add_argument("--rows", type=int, default=1024)
args = ap.parse_args()

spec, _ = kta.synth_preset("c3")
P, per = 64, args.records
M = min(args.rows, (1 << 20) // P)
owner = kta.HipMetricHandler(P)
batches = []
for k in range(args.batches):
    b = owner.device_batch_alloc(per, per * 16, with_seq=True)
    owner.synth_fill_device(spec, k * per, per, b)
    batches.append(b)
owner.sync()
n = per * len(batches)


def one_pass(h, which):
    for b in batches:
        h.submit_device(b, per, 0, which=which)
    h.sync()


def timed_passes(h, which):
    """the best of --steps passes of the metrics handler, each from a reset context (the reset and a wait outside the clock)"""
    for _ in range(args.warmup):
        one_pass(h, which)
    times = []
    for _ in range(args.steps):
        h.reset()
        h.sync()
        t0 = time.perf_counter()
        one_pass(h, which)
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def timed_replays(h, on):
    """reset, the switch, an untimed first pass, then --warmup + --steps replays"""
    h.reset()
    h.set_compact_delete(on)
    one_pass(h, 3)
    h.finish()

    def replay():
        with h.compaction_replay():
            for b in batches:
                h.submit_device(b, per, 0)
        h.sync()

    for _ in range(args.warmup):
        replay()
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        replay()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


sizes = []
for s in args.segment_bytes.split(","):
    if s != "auto":
        sizes.append(int(s))
        continue
    with kta.HipMetricHandler(P, segments=(1 << 40, 2, 0)) as probe:   # the partitions' bytes of one pass
        one_pass(probe, 1)
        sizes.append(int(probe.segments()["totals"][:, 1].max()) // (M - 2) + 1)

scan = kta.HipMetricHandler(P)
for S in sizes:
    cfg = (S, M, 0)
    best, work, verdict = {}, None, None
    with kta.HipMetricHandler(P, count_alive_keys=True, compaction=True, segments=cfg) as h, kta.HipMetricHandler(P, segments=cfg) as seg:
        for rnd in range(args.rounds):
            for leg in ("replay_off", "replay_on", "segment_pass"):
                if leg == "segment_pass":
                    with_seg, without = timed_passes(seg, 1), timed_passes(scan, 1)
                    times = [round(min(with_seg) - min(without), 4)]
                    extra = {"scan_with_segments_ms": [round(t, 4) for t in with_seg], "scan_ms": [round(t, 4) for t in without]}
                else:
                    times = timed_replays(h, leg == "replay_on")
                    extra = {}
                    if leg == "replay_on":
                        work = h.compact_delete_info()                              # (of the last replay: the counters start with each)
                        sv, kv, cv = h.segments()["vector"], h.compact_delete()["vector"], h.compaction()["vector"]
                        w = kta.compact_delete_whatif(sv, kv, cv, P, M, 0)      # raises when an identity fails
                        verdict = {"identities_hold": True, "rows_closed": int(h.compact_delete()["globals"][2]),
                                   "records": int(w[P][0]), "compacted_records": int(w[P][2])}
                ms = min(times)
                best[leg] = min(best.get(leg, ms), ms)
                print(json.dumps(dict({"tool": "bench_compact_delete", "segment_bytes": S, "leg": leg, "round": rnd, "records": n,
                                       "batches": len(batches), "partitions": P, "steps": args.steps, "ms": round(ms, 4),
                                       "ms_all": [round(t, 4) for t in times]}, **extra)), flush=True)
    added = best["replay_on"] - best["replay_off"]
    print(json.dumps({"tool": "bench_compact_delete", "shape": "c3 law, table state, seq column, 16 B keys, 10M distinct, 10% tombstones",
                      "segment_bytes": S, "rows_per_partition": M, "records": n, "partitions": P,
                      "best_ms": {k: round(v, 4) for k, v in best.items()},
                      "replay_off_G_records_per_s": round(n / (best["replay_off"] * 1e-3) / 1e9, 3),
                      "replay_on_G_records_per_s": round(n / (best["replay_on"] * 1e-3) / 1e9, 3),
                      "replay_on_minus_off_ms": round(added, 4), "segment_pass_ms": round(best["segment_pass"], 4),
                      "on_over_off_plus_segment_pass": round(best["replay_on"] / (best["replay_off"] + best["segment_pass"]), 4),
                      "class_column_bytes": 2 * n, "work_per_replay": work, "whatif": verdict}), flush=True)
scan.close()
for b in batches:
    owner.device_batch_free(b)
owner.close()

"""What the compaction what-if (KTA_FLAG_COMPACTION) costs: the replay of config 3's shape as bench.py's alive_pass_table
leg builds it — the sequence-numbered table (32 GiB), device-resident tile-compact batches with a seq column, 16-byte keys,
64 partitions, 10 M distinct keys, 10 % tombstones — on one GPU, in ONE process:

    first pass   the alive-key handler alone (which = 2) over every batch, timed by wall clock: the pass that leaves the table
    replay       kta_compaction_replay(on), every batch again (kta_compaction_survivors), off; `--steps` times

    python tools/bench_compaction.py [--records 251658240] [--batches 5] [--steps 3] [--warmup 1]

Prints one JSON line: ms per replay, G records/s, the bytes streamed per record (partition 2 B in a compact tile + key_len
4 + key_off 4 + val_len 4 + seq 8 + the key bytes, next to ONE random 8-byte table read per keyed record: a 64-byte line
of its own), the first pass's time in the same call for comparison, the pass's work counters of one replay
(kta_compaction_info) and the identity live survivors == alive keys.  Hold the G records/s against
`tools/ubench_scatter reads` of the same box: one such read per keyed record is what bounds the pass."""
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
args = ap.parse_args()

spec, _ = kta.synth_preset("c3")
P, per = 64, args.records
with kta.HipMetricHandler(P, count_alive_keys=True, compaction=True) as h:
    batches, key_bytes = [], 0
    for k in range(args.batches):
        b = h.device_batch_alloc(per, per * 16, with_seq=True)
        key_bytes += h.synth_fill_device(spec, k * per, per, b)
        batches.append(b)
    h.sync()
    n = per * len(batches)
    t0 = time.perf_counter()
    for b in batches:
        h.submit_device(b, per, 0, which=2)
    h.sync()
    first_ms = (time.perf_counter() - t0) * 1e3
    res, _ = h.finish()

    def replay():
        with h.compaction_replay():
            for b in batches:
                h.submit_device(b, per, 0)
        h.sync()

    for _ in range(args.warmup):
        replay()
    before = h.compaction_info()
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        replay()
        times.append((time.perf_counter() - t0) * 1e3)
    after = h.compaction_info()
    v = h.compaction()
    ms = min(times)
    streamed = n * (2 + 4 + 4 + 4 + 8) + key_bytes
    work = {k: (after[k] - before[k]) // args.steps for k in ("keyed_records", "launches", "workgroups", "lds_adds")}
    work["lds_bytes"] = after["lds_bytes"]
    live = int(v["live_records"].sum()) + v["live_outside"]
    assert v["unknown"] == 0 and v["replayed"] == n and live == res.alive_keys, (v["unknown"], v["replayed"], live, res.alive_keys)
    print(json.dumps({"tool": "bench_compaction", "shape": "c3 law, table state, seq column, 16 B keys, 10M distinct, 10% tombstones",
                      "records": n, "batches": len(batches), "partitions": P, "steps": args.steps,
                      "replay_ms": round(ms, 4), "replay_ms_all": [round(t, 4) for t in times],
                      "replay_G_records_per_s": round(n / (ms * 1e-3) / 1e9, 3),
                      "streamed_bytes_per_record": round(streamed / n, 3), "streamed_TBps": round(streamed / (ms * 1e-3) / 1e12, 3),
                      "table_reads_per_record": round(work["keyed_records"] / n, 4),
                      "first_pass_ms": round(first_ms, 4), "first_pass_G_records_per_s": round(n / (first_ms * 1e-3) / 1e9, 3),
                      "replay_over_first_pass": round(ms / first_ms, 3), "work_per_replay": work,
                      "alive_keys": int(res.alive_keys), "live_survivors": live,
                      "tombstones_kept": int(v["tombstone_records"].sum()),
                      "records_reclaimed_share": round(1 - (live + int(v["tombstone_records"].sum())) / n, 5)}), flush=True)
    for b in batches:
        h.device_batch_free(b)

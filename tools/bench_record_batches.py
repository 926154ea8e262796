"""What the record-batch pass (KTA_FLAG_RECORD_BATCHES) costs a decode step, on the GPU: kta_kafka_decode_device over the
bench's raw logs of c4 records — batches of 60 records (~16 KiB, 4 M records) and of 8 (~2 KiB, 2 M records), resident in
HBM — with the flag off and on, the two contexts alternated ROUNDS times in one process.  A step is one decode call; a round
times STEPS of them between two synchronisations (host clock).  Per shape one JSON line: the median step of either side, the
ratio on / off with the spread of the rounds, the host's time inside the calls (the enqueue: a step cannot be shorter), the
pass's own kernel time (kta_record_batches_info under kta_set_timing, event
pairs, taken in rounds of their own) beside the decode kernel's, and the bytes the pass reads as a share of the log.

    python tools/bench_record_batches.py [--rounds 5] [--steps 30] [--out profiles/record_batches_bench.jsonl]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((60, 4_000_000, "~16 KiB"), (8, 2_000_000, "~2 KiB"))
PASS_BYTES_PER_BATCH = 88 + 64   # the descriptor, and the 64-byte lines the header bytes 12..50 touch (one, sometimes two)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import kafka_topic_analyzer_amd as kta
    from kafka_topic_analyzer_amd import _native as N
    lib = N.load()
    spec, _ = kta.synth_preset("c4")
    lines = []
    for rpb, n, label in SHAPES:
        ln = C.c_uint64()
        lib.kta_kafka_encode_synth_host(C.byref(spec), 0, n, rpb, None, 0, C.byref(ln))
        buf = np.zeros(ln.value + 64, np.uint8)
        lib.kta_kafka_encode_synth_host(C.byref(spec), 0, n, rpb, buf.ctypes.data, ln.value, C.byref(ln))
        cap = n // rpb + 2
        descs = (N.KtaKafkaBatchDesc * cap)()
        st = N.KtaKafkaIndexStats()
        assert lib.kta_kafka_index_host(buf.ctypes.data_as(C.c_char_p), ln.value, 0, 0, 0, 0, descs, cap, C.byref(st)) == 0
        sides = {}
        for on in (False, True):
            h = kta.HipMetricHandler(256, record_batches=on)
            blob = h.device_batch_alloc((ln.value + 3) // 4 + 32)
            h._check(lib.kta_copy_to_device(h._ctx, blob.partition, buf.ctypes.data, (ln.value + 63) // 64 * 64))
            out = h.device_batch_alloc(n, 16)
            sides[on] = (h, blob, out)

        def step(on):
            h, blob, out = sides[on]
            h._check(lib.kta_kafka_decode_device(h._ctx, blob.partition, ln.value, descs, st.n_batches, n, C.byref(out), None, None))

        for on in (False, True):                       # warm up this shape on both sides
            for _ in range(5):
                step(on)
            sides[on][0].sync()
        ms, enqueue = {False: [], True: []}, {False: [], True: []}
        for _ in range(args.rounds):
            for on in (False, True):
                h = sides[on][0]
                h.sync()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(on)
                t1 = time.perf_counter()               # the host is done enqueueing: what it spent inside the calls
                h.sync()
                ms[on].append((time.perf_counter() - t0) / args.steps * 1e3)
                enqueue[on].append((t1 - t0) / args.steps * 1e3)
        # kernel times, event pairs around each kernel: rounds of their own (recording events is host work)
        kernel = {}
        for on in (False, True):
            h = sides[on][0]
            h.set_timing(True)
            for _ in range(args.steps):
                step(on)
            h.sync()
            a, c = (C.c_float * 2)(), (C.c_uint64 * 2)()
            h._check(lib.kta_kafka_time_stats(h._ctx, C.byref(a), C.byref(c)))
            kernel[on] = {"decode_kernel_ms": float(a[1])}
            if on:
                info = h.record_batches_info()
                kernel[on].update(pass_kernel_ms=info["kernel_ms"], pass_workgroups=info["workgroups"], pass_launches_timed=info["timed"])
                d = h.get_record_batches()
                steps_run = info["launches"]
                assert int(d["partitions"][0][0]) == st.n_batches * steps_run and int(d["partitions"][0][1]) == n * steps_run
            h.set_timing(False)
        ratios = [b / a for a, b in zip(ms[False], ms[True])]
        line = {"bench": "record_batches", "batch": label, "records_per_batch": rpb, "records": n, "batches": int(st.n_batches),
                "raw_log_bytes": int(ln.value), "rounds": args.rounds, "steps_per_round": args.steps,
                "step_ms_off": statistics.median(ms[False]), "step_ms_on": statistics.median(ms[True]),
                "step_ms_off_rounds": ms[False], "step_ms_on_rounds": ms[True],
                "ratio_on_over_off": statistics.median(ratios), "ratio_min": min(ratios), "ratio_max": max(ratios),
                "off_spread": max(ms[False]) / min(ms[False]),
                "host_enqueue_ms_off": statistics.median(enqueue[False]), "host_enqueue_ms_on": statistics.median(enqueue[True]),
                "pass_bytes_share_of_log": PASS_BYTES_PER_BATCH * st.n_batches / ln.value, **kernel[False], "on": kernel[True]}
        print(json.dumps(line), flush=True)
        lines.append(line)
        for h, blob, out in sides.values():
            h.device_batch_free(out)
            h.device_batch_free(blob)
            h.close()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

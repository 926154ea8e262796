"""What the header-name pass (KTA_FLAG_HEADER_NAMES) costs a decode step, on the GPU: tools/bench_payload.py's workload —
kta_kafka_decode_device over the bench's raw log of c4 records, 4 M records in uncompressed batches of 60 (~16 KiB), resident in
HBM — with 0, 1 and 5 headers behind every record, with the flag off and on, the contexts alternated ROUNDS times in one
process; a third context with KTA_FLAG_PAYLOAD instead gives the payload pass's cost on the same bytes in the same rounds.  A
step is one decode call; a round times STEPS of them between two synchronisations (host clock).  Per blob one JSON line: the
median step of each side and the ratios to the flag-off side, the passes' own kernel times (kta_header_names_info,
kta_payload_info under kta_set_timing, event pairs, taken in rounds of their own) beside the decode kernel's of the same process
(kta_kafka_time_stats), the header-name pass over the payload pass, and the pass's work: occurrences per run, names listed, cache
claims and spills.

    python tools/bench_header_names.py [--records 4000000] [--rounds 5] [--steps 20] [--out profiles/header_names_bench.jsonl]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_payload import HEADERS, RPB, with_headers  # noqa: E402  (the same workload)

FIVE = HEADERS + [(b"correlation-id", b"7f3c2a1e-9b4d-4c6f-8a2b-5d1e0f9c8b7a")]
SIDES = ("off", "header_names", "payload")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=4_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import kafka_topic_analyzer_amd as kta
    from kafka_topic_analyzer_amd import _native as N
    lib = N.load()
    spec, _ = kta.synth_preset("c4")
    n = args.records
    ln = C.c_uint64()
    lib.kta_kafka_encode_synth_host_ex(C.byref(spec), 0, n, RPB, 0, None, 0, C.byref(ln))
    buf = np.zeros(ln.value + 64, np.uint8)
    lib.kta_kafka_encode_synth_host_ex(C.byref(spec), 0, n, RPB, 0, buf.ctypes.data, ln.value, C.byref(ln))
    plain = buf[:ln.value].tobytes()
    lines = []
    for label, headers in (("0 headers per record", []), ("1 header per record", HEADERS[:1]), ("5 headers per record", FIVE)):
        raw = with_headers(lib, plain, headers) if headers else plain
        cap = n // RPB + 2
        descs = (N.KtaKafkaBatchDesc * cap)()
        st = N.KtaKafkaIndexStats()
        inflate_at = (len(raw) + 127) & ~63
        assert lib.kta_kafka_index_host(raw, len(raw), 0, 0, 0, inflate_at, descs, cap, C.byref(st)) == 0
        buf = np.zeros(inflate_at + 64, np.uint8)
        buf[:len(raw)] = np.frombuffer(raw, np.uint8)
        sides = {}
        for side in SIDES:
            h = kta.HipMetricHandler(256, header_names=side == "header_names", payload=side == "payload")
            blob = h.device_batch_alloc((inflate_at + st.inflate_bytes + 3) // 4 + 64)
            h._check(lib.kta_copy_to_device(h._ctx, blob.partition, buf.ctypes.data, inflate_at))
            out = h.device_batch_alloc(n, 16)
            sides[side] = (h, blob, out)

        def step(side):
            h, blob, out = sides[side]
            h._check(lib.kta_kafka_decode_device(h._ctx, blob.partition, len(raw), descs, st.n_batches, n, C.byref(out), None, None))

        for side in SIDES:                             # warm up this blob on every side
            for _ in range(3):
                step(side)
            sides[side][0].sync()
        ms = {side: [] for side in SIDES}
        for _ in range(args.rounds):
            for side in SIDES:
                h = sides[side][0]
                h.sync()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(side)
                h.sync()
                ms[side].append((time.perf_counter() - t0) / args.steps * 1e3)
        kernel = {}
        for side in SIDES:                             # kernel times, event pairs around each kernel: rounds of their own
            h = sides[side][0]
            h.set_timing(True)
            for _ in range(args.steps):
                step(side)
            h.sync()
            a, c = (C.c_float * 2)(), (C.c_uint64 * 2)()
            h._check(lib.kta_kafka_time_stats(h._ctx, C.byref(a), C.byref(c)))
            kernel[side] = {"decode_kernel_ms": float(a[1])}
            if side == "header_names":
                info, d = h.header_names_info(), h.header_names()
                runs = info["launches"]
                assert d["looked"] == n * runs and d["occurrences"] == n * runs * len(headers) and kta.header_names_identities(d["vector"]), d
                assert d["names"]["unresolved_occurrences"] == 0 and len(d["names"]["names"]) == len(headers)
                kernel[side].update(pass_kernel_ms=info["kernel_ms"], pass_workgroups=info["workgroups"], pass_launches_timed=info["timed"],
                                    pass_over_decode_kernel=info["kernel_ms"] / float(a[1]), occurrences_per_run=d["occurrences"] // runs,
                                    names_listed=len(d["names"]["names"]), cache_claims_per_run=info["claims"] / runs, spills=info["spills"],
                                    cache_flushes=info["cache_flushes"])
            elif side == "payload":
                info = h.payload_info()
                kernel[side].update(pass_kernel_ms=info["kernel_ms"], pass_workgroups=info["workgroups"], pass_over_decode_kernel=info["kernel_ms"] / float(a[1]))
            h.set_timing(False)
        line = {"bench": "header_names", "blob": label, "records_per_batch": RPB, "records": n, "batches": int(st.n_batches), "raw_log_bytes": len(raw),
                "rounds": args.rounds, "steps_per_round": args.steps}
        for side in SIDES:
            line["step_ms_" + side] = statistics.median(ms[side])
            line["step_ms_%s_rounds" % side] = ms[side]
        for side in SIDES[1:]:
            ratios = [b / a for a, b in zip(ms["off"], ms[side])]
            line["ratio_%s_over_off" % side] = {"median": statistics.median(ratios), "min": min(ratios), "max": max(ratios)}
        line["pass_kernel_header_names_over_payload"] = kernel["header_names"]["pass_kernel_ms"] / kernel["payload"]["pass_kernel_ms"]
        line.update(off=kernel["off"], header_names=kernel["header_names"], payload=kernel["payload"])
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

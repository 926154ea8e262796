"""What the compression what-if's pass (KTA_FLAG_COMPRESS_WHATIF) costs, on the GPU: kta_kafka_decode_device over a raw log of
4 M c4 records in uncompressed batches of 60 (~16 KiB) from the synthetic encoder, resident in HBM, under its two value laws —
the bench's patterned values (a 24-byte period) and its text (words, numbers, punctuation) —, by a context with
KTA_FLAG_COMPRESS_WHATIF and KTA_FLAG_VALUE_BYTES both on, so that the same call times both passes on the same blob
(kta_compress_whatif_info, kta_value_bytes_info under kta_set_timing: event pairs around each kernel), and by a context with
neither for the step without them.  Per law one JSON line: the two passes' kernel times, GB/s of inflated bytes for either,
their ratio, the what-if's rate over the link rate the committed bench line gives for raw_log_e2e (52.1 GB/s of raw log over
PCIe), the decode kernel's time, the steps with and without the passes, and the section's own figures (model ratio, match share).
The device's vector is checked against the host rule on the log's first batches.

    python tools/bench_compress_whatif.py [--records 4000000] [--steps 10] [--out profiles/compress_whatif_bench.jsonl]"""
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

RPB = 60
LINK_GBPS = 52.1                         # BENCH_r06.json: raw_log_e2e, metrics, raw_log_GBps
CHECK_BATCHES = 2000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=4_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import kafka_topic_analyzer_amd as kta
    from kafka_topic_analyzer_amd import _native as N
    lib = N.load()
    spec, _ = kta.synth_preset("c4")
    lines = []
    for law, flag in (("patterned", 0), ("text", 0x200)):
        ln = C.c_uint64()
        lib.kta_kafka_encode_synth_host_ex(C.byref(spec), 0, args.records, RPB, 0x100 | flag, None, 0, C.byref(ln))
        raw_np = np.zeros(ln.value + 128, np.uint8)
        assert lib.kta_kafka_encode_synth_host_ex(C.byref(spec), 0, args.records, RPB, 0x100 | flag, raw_np.ctypes.data, ln.value, C.byref(ln)) == 0
        raw = raw_np[:ln.value].tobytes()
        n_batches = (args.records + RPB - 1) // RPB
        descs = (N.KtaKafkaBatchDesc * (n_batches + 2))()
        st = N.KtaKafkaIndexStats()
        inflate_at = (len(raw) + 127) & ~63
        assert lib.kta_kafka_index_host(raw, len(raw), 0, 0, 0, inflate_at, descs, n_batches + 2, C.byref(st)) == 0
        assert st.n_batches == n_batches and st.n_records == args.records
        buf = np.zeros(inflate_at + 64, np.uint8)
        buf[:len(raw)] = raw_np[:len(raw)]
        sides = {}
        for side in ("off", "on"):
            h = kta.HipMetricHandler(256, value_bytes=side == "on", compress_whatif=side == "on")
            blob = h.device_batch_alloc((inflate_at + st.inflate_bytes + 3) // 4 + 64)
            h._check(lib.kta_copy_to_device(h._ctx, blob.partition, buf.ctypes.data, inflate_at))
            out = h.device_batch_alloc(args.records, 16)
            sides[side] = (h, blob, out)

        def step(side, batches=None):
            h, blob, out = sides[side]
            nb = st.n_batches if batches is None else batches
            nbytes = len(raw) if batches is None else int(descs[batches].byte_off)
            nrec = args.records if batches is None else batches * RPB
            h._check(lib.kta_kafka_decode_device(h._ctx, blob.partition, nbytes, descs, nb, nrec, C.byref(out), None, None))

        # the device against the host rule, on the log's first batches
        check = min(CHECK_BATCHES, n_batches - 1)
        step("on", check)
        got = sides["on"][0].compress_whatif()["vector"]
        want = kta.compress_whatif_host(raw[:int(descs[check].byte_off)], 0, 256)
        assert np.array_equal(got, want) and kta.compress_whatif_identities(got, 256), law
        sides["on"][0].reset()
        ms = {}
        for side in ("off", "on"):
            h = sides[side][0]
            step(side)
            h.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(side)
            h.sync()
            ms[side] = (time.perf_counter() - t0) / args.steps * 1e3
        h = sides["on"][0]
        h.reset()
        h.set_timing(True)
        for _ in range(args.steps):
            step("on")
        h.sync()
        a, c = (C.c_float * 2)(), (C.c_uint64 * 2)()
        h._check(lib.kta_kafka_time_stats(h._ctx, C.byref(a), C.byref(c)))
        cw, vb, d = h.compress_whatif_info(), h.value_bytes_info(), h.compress_whatif()
        topic = {k: int(v) for k, v in zip(kta.COMPRESS_WHATIF_COLUMNS, d["topic"])}
        inflated = topic["raw_bytes"] // args.steps
        line = {"bench": "compress_whatif", "law": law, "records_per_batch": RPB, "records": args.records, "batches": int(st.n_batches),
                "raw_log_bytes": len(raw), "inflated_bytes": inflated, "steps": args.steps, "checked_batches": check,
                "step_ms_off": ms["off"], "step_ms_on": ms["on"], "decode_kernel_ms": float(a[1]),
                "compress_whatif_kernel_ms": cw["kernel_ms"], "compress_whatif_workgroups": cw["workgroups"],
                "value_bytes_kernel_ms": vb["kernel_ms"],
                "compress_whatif_gb_per_s": inflated / cw["kernel_ms"] / 1e6, "value_bytes_gb_per_s": inflated / vb["kernel_ms"] / 1e6,
                "compress_whatif_over_value_bytes": cw["kernel_ms"] / vb["kernel_ms"],
                "link_gb_per_s": LINK_GBPS, "compress_whatif_rate_over_link": inflated / cw["kernel_ms"] / 1e6 / LINK_GBPS,
                "model_ratio": topic["raw_bytes"] / topic["model_bytes"], "match_share": topic["match_bytes"] / topic["raw_bytes"],
                "sequences_per_batch": topic["sequences"] / topic["batches"], "stored_blocks": topic["stored_blocks"]}
        print(json.dumps(line), flush=True)
        lines.append(line)
        for h, blob, out in sides.values():
            h.device_batch_free(out)
            h.device_batch_free(blob)
            h.close()
        del raw, raw_np, buf
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

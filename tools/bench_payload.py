"""What the payload pass (KTA_FLAG_PAYLOAD) costs a decode step, on the GPU: kta_kafka_decode_device over the bench's raw log
of c4 records — 4 M records in batches of 60 (~16 KiB), resident in HBM — uncompressed, as zstd batches (libzstd level 3
through pyarrow, as bench.py makes them) and uncompressed with 4 headers behind every record, with the flag off and on, the two
contexts alternated ROUNDS times in one process.  A step is one decode call; a round times STEPS of them between two
synchronisations (host clock).  Per blob one JSON line: the median step of either side and their ratio, the pass's own kernel
time (kta_payload_info under kta_set_timing, event pairs, taken in rounds of their own) beside the decode kernel's of the same
process (kta_kafka_time_stats) and their ratio — the yardstick: the pass streams the same windows and stores nothing per
record —, and the bytes the pass reads: the windows (the batches' record bytes), the descriptors and the header sections it
walks in global memory.

    python tools/bench_payload.py [--records 4000000] [--rounds 5] [--steps 20] [--out profiles/payload_bench.jsonl]"""
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
from bench import _recompress_batches  # noqa: E402  (zstd batches exactly as the benchmark's raw-log legs have them)

RPB = 60
HEADERS = [(b"traceparent", b"00-0af7651916cd43dd8448eb211c80319c-b7ad6b7169203331-01"), (b"ce_type", b"com.example.order.created"),
           (b"ce_source", b"/orders/eu-west"), (b"retries", None)]


def _varint(v):
    z, out = v << 1, bytearray()
    while True:
        b = z & 0x7F
        z >>= 7
        out.append(b | 0x80 if z else b)
        if not z:
            return bytes(out)


def with_headers(lib, raw, headers):
    """The uncompressed v2 batches of `raw` with `headers` behind every record (their header sections are the byte 0)."""
    block = _varint(len(headers)) + b"".join(_varint(len(k)) + k + (b"\x01" if v is None else _varint(len(v)) + v) for k, v in headers)
    grow, out, pos = len(block) - 1, [], 0
    raw = bytes(raw)
    while pos + 61 <= len(raw):
        total = 12 + int.from_bytes(raw[pos + 8:pos + 12], "big")
        b, recs, p = raw[pos:pos + total], [], 61
        while p < total:
            n = b[p]
            nb = 1
            if n & 0x80:
                n = (n & 0x7F) | (b[p + 1] & 0x7F) << 7
                nb = 2
                if b[p + 1] & 0x80:
                    n |= b[p + 2] << 14
                    nb = 3
            n >>= 1
            assert b[p + nb + n - 1] == 0
            recs += [_varint(n + grow), b[p + nb:p + nb + n - 1], block]
            p += nb + n
        body = b"".join(recs)
        after_crc = b[21:61] + body
        crc = lib.kta_crc32c_host(after_crc, len(after_crc))
        out.append(b[0:8] + (49 + len(body)).to_bytes(4, "big") + b[12:17] + crc.to_bytes(4, "big") + after_crc)
        pos += total
    return b"".join(out)


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

    def synth(codec):
        ln = C.c_uint64()
        lib.kta_kafka_encode_synth_host_ex(C.byref(spec), 0, n, RPB, codec, None, 0, C.byref(ln))
        buf = np.zeros(ln.value + 64, np.uint8)
        lib.kta_kafka_encode_synth_host_ex(C.byref(spec), 0, n, RPB, codec, buf.ctypes.data, ln.value, C.byref(ln))
        return buf[:ln.value].tobytes()

    plain = synth(0)
    blobs = [("uncompressed", plain), ("zstd", _recompress_batches(lib, synth(0x100), 4)), ("uncompressed, 4 headers per record", with_headers(lib, plain, HEADERS))]
    del plain
    lines = []
    for label, raw in blobs:
        cap = n // RPB + 2
        descs = (N.KtaKafkaBatchDesc * cap)()
        st = N.KtaKafkaIndexStats()
        inflate_at = (len(raw) + 127) & ~63
        assert lib.kta_kafka_index_host(raw, len(raw), 0, 0, 0, inflate_at, descs, cap, C.byref(st)) == 0
        buf = np.zeros(inflate_at + 64, np.uint8)
        buf[:len(raw)] = np.frombuffer(raw, np.uint8)
        window_bytes = sum(descs[i].payload_end - descs[i].payload_off for i in range(st.n_batches))   # (a bound for zstd: the index's)
        sides = {}
        for on in (False, True):
            h = kta.HipMetricHandler(256, payload=on)
            blob = h.device_batch_alloc((inflate_at + st.inflate_bytes + 3) // 4 + 64)
            h._check(lib.kta_copy_to_device(h._ctx, blob.partition, buf.ctypes.data, inflate_at))
            out = h.device_batch_alloc(n, 16)
            sides[on] = (h, blob, out)

        def step(on):
            h, blob, out = sides[on]
            h._check(lib.kta_kafka_decode_device(h._ctx, blob.partition, len(raw), descs, st.n_batches, n, C.byref(out), None, None))

        for on in (False, True):                       # warm up this blob on both sides
            for _ in range(3):
                step(on)
            sides[on][0].sync()
        ms = {False: [], True: []}
        for _ in range(args.rounds):
            for on in (False, True):
                h = sides[on][0]
                h.sync()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(on)
                h.sync()
                ms[on].append((time.perf_counter() - t0) / args.steps * 1e3)
        kernel = {}
        for on in (False, True):                       # kernel times, event pairs around each kernel: rounds of their own
            h = sides[on][0]
            h.set_timing(True)
            for _ in range(args.steps):
                step(on)
            h.sync()
            a, c = (C.c_float * 2)(), (C.c_uint64 * 2)()
            h._check(lib.kta_kafka_time_stats(h._ctx, C.byref(a), C.byref(c)))
            kernel[on] = {"decode_kernel_ms": float(a[1])}
            if on:
                info = h.payload_info()
                d = h.get_payload()
                part, runs = d["partitions"][0], info["launches"]
                assert int(part[0]) == n * runs and kta.payload_identities(d["vector"], 256), (int(part[0]), n, runs)
                walked = int(part[17]) - int(d["headers_hist"][0])      # header sections of more than the byte 0
                kernel[on].update(pass_kernel_ms=info["kernel_ms"], pass_workgroups=info["workgroups"], pass_launches_timed=info["timed"],
                                  pass_over_decode_kernel=info["kernel_ms"] / float(a[1]),
                                  pass_bytes={"windows": int(window_bytes), "descriptors": 88 * int(st.n_batches), "header_sections": walked // runs},
                                  classes_per_run=[int(x) // runs for x in part[1:6]], schema_ids=len(d["schema_ids"]["ids"]))
            h.set_timing(False)
        ratios = [b / a for a, b in zip(ms[False], ms[True])]
        line = {"bench": "payload", "blob": label, "records_per_batch": RPB, "records": n, "batches": int(st.n_batches), "raw_log_bytes": len(raw),
                "rounds": args.rounds, "steps_per_round": args.steps, "step_ms_off": statistics.median(ms[False]),
                "step_ms_on": statistics.median(ms[True]), "step_ms_off_rounds": ms[False], "step_ms_on_rounds": ms[True],
                "ratio_on_over_off": statistics.median(ratios), "ratio_min": min(ratios), "ratio_max": max(ratios), **kernel[False], "on": kernel[True]}
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

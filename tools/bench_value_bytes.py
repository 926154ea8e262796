"""What the value-byte pass (KTA_FLAG_VALUE_BYTES) costs a decode step, on the GPU: kta_kafka_decode_device over a raw log of
4 M records in uncompressed batches of 60 (~16 KiB: 61 bytes of batch header, records of 9 framing bytes around a 256-byte
value), resident in HBM, under three value laws — uniformly random bytes, JSON-like text, all zero — with the flag off, on
(a dword of four equal bytes is one LDS add), on with every byte its own LDS add (KTA_VALUE_BYTES_VARIANT=1, read when a context
is created), on with whichever bytes of a dword are equal added once (KTA_VALUE_BYTES_VARIANT=2) and with KTA_FLAG_PAYLOAD instead (the neighbour: the pass that walks the same
records but reads five bytes of a value), the contexts alternated ROUNDS times in one process.  A step is one decode call; a
round times STEPS of them between two synchronisations (host clock).  Per law one JSON line: the median step of each side and
the ratios to the flag-off side, the passes' own kernel times (kta_value_bytes_info, kta_payload_info under kta_set_timing,
event pairs, taken in rounds of their own) beside the decode kernel's of the same process (kta_kafka_time_stats), the blob's
bytes over the pass kernel's time in GB/s, and the floor: the blob's bytes over 6.3 TB/s, the HBM rate the metrics scan
reaches.  A last line states the all-zero law over the random law, the cost of skew, for the three forms.

    python tools/bench_value_bytes.py [--records 4000000] [--rounds 5] [--steps 20] [--out profiles/value_bytes_bench.jsonl]"""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RPB, VALUE = 60, 256
RECORD = 9 + VALUE                       # length varint (2) | attributes | tsDelta | offsetDelta | key -1 | value length varint (2) | value | headers 0
BATCH = 61 + RPB * RECORD
HBM_RATE = 6.3e12                        # bytes / s: what the metrics scan reaches
SIDES = ("off", "value_bytes", "value_bytes_single", "value_bytes_pairs", "payload")
T0 = 1_600_000_000_000


def _varint(v):
    z, out = (v << 1) ^ (v >> 63), bytearray()
    while True:
        b = z & 0x7F
        z >>= 7
        out.append(b | (0x80 if z else 0))
        if not z:
            return bytes(out)


def log_of(lib, n_batches, values):
    """The raw log: n_batches v2 batches of RPB records; values: uint8 [n_batches][RPB][VALUE]."""
    rows = np.zeros((n_batches, BATCH), np.uint8)
    head = struct.pack(">qiibIhiqqqhii", 0, BATCH - 12, 0, 2, 0, 0, RPB - 1, T0, T0, -1, -1, -1, RPB)
    assert len(head) == 61
    rows[:, :61] = np.frombuffer(head, np.uint8)
    rows[:, :8] = (np.arange(n_batches, dtype=np.uint64) * RPB).astype(">u8").view(np.uint8).reshape(n_batches, 8)
    recs = rows[:, 61:].reshape(n_batches, RPB, RECORD)
    for r in range(RPB):
        framing = _varint(RECORD - 2) + b"\x00\x00" + _varint(r) + _varint(-1) + _varint(VALUE)
        assert len(framing) == 8
        recs[:, r, :8] = np.frombuffer(framing, np.uint8)
    recs[:, :, 8:8 + VALUE] = values
    for b in range(n_batches):                                                # CRC-32C over attributes .. end
        crc = lib.kta_crc32c_host(rows[b, 21:].tobytes(), BATCH - 21)
        rows[b, 17:21] = np.frombuffer(struct.pack(">I", crc & 0xFFFFFFFF), np.uint8)
    return rows.reshape(-1)


def values_of(law, n_batches, rng):
    if law == "random":
        return rng.integers(0, 256, (n_batches, RPB, VALUE), dtype=np.uint8)
    if law == "zero":
        return np.zeros((n_batches, RPB, VALUE), np.uint8)
    pool = []
    for i in range(4096):                                                     # JSON-like text: 4096 documents of 256 bytes
        doc = ('{"order_id":%d,"customer":"user-%05d","items":[{"sku":"A-%04d","qty":%d,"price":%d.%02d}],"status":"%s","note":"'
               % (10 ** 9 + 7919 * i, i * 13 % 100000, i % 10000, i % 9 + 1, i % 500, i % 100, ("created", "paid", "shipped")[i % 3])).encode()
        doc += (b"lorem ipsum dolor sit amet consectetur adipiscing elit sed do eiusmod tempor " * 4)[i % 17:]
        pool.append(np.frombuffer(doc[:VALUE - 2] + b'"}', np.uint8))
    pool = np.stack(pool)
    return pool[rng.integers(0, len(pool), (n_batches, RPB))]


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
    n_batches = (args.records + RPB - 1) // RPB
    n = n_batches * RPB
    rng = np.random.default_rng(12)
    lines, kernels = [], {}
    for law in ("random", "json", "zero"):
        values = values_of(law, n_batches, rng)
        raw_np = log_of(lib, n_batches, values)
        raw = raw_np.tobytes()
        want_bins = np.bincount(values.reshape(-1), minlength=256).astype(np.uint64)
        del values
        descs = (N.KtaKafkaBatchDesc * (n_batches + 2))()
        st = N.KtaKafkaIndexStats()
        inflate_at = (len(raw) + 127) & ~63
        assert lib.kta_kafka_index_host(raw, len(raw), 0, 0, 0, inflate_at, descs, n_batches + 2, C.byref(st)) == 0
        assert st.n_batches == n_batches and st.n_records == n
        buf = np.zeros(inflate_at + 64, np.uint8)
        buf[:len(raw)] = raw_np
        sides = {}
        for side in SIDES:
            os.environ["KTA_VALUE_BYTES_VARIANT"] = {"value_bytes_single": "1", "value_bytes_pairs": "2"}.get(side, "0")
            h = kta.HipMetricHandler(256, value_bytes=side.startswith("value_bytes"), payload=side == "payload")
            blob = h.device_batch_alloc((inflate_at + st.inflate_bytes + 3) // 4 + 64)
            h._check(lib.kta_copy_to_device(h._ctx, blob.partition, buf.ctypes.data, inflate_at))
            out = h.device_batch_alloc(n, 16)
            sides[side] = (h, blob, out)
        os.environ.pop("KTA_VALUE_BYTES_VARIANT", None)

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
            if side.startswith("value_bytes"):
                info, d = h.value_bytes_info(), h.value_bytes()
                runs = info["launches"]
                w = d["partitions"][0]
                assert np.array_equal(w[:256], want_bins * np.uint64(runs)) and w[258] == np.uint64(n * VALUE * runs) and w[256] == np.uint64(n * runs), law
                assert kta.value_bytes_identities(d["vector"], 256)
                kernel[side].update(pass_kernel_ms=info["kernel_ms"], pass_workgroups=info["workgroups"], mid_flushes=info["mid_flushes"],
                                    pass_over_decode_kernel=info["kernel_ms"] / float(a[1]), blob_gb_per_s=len(raw) / info["kernel_ms"] / 1e6,
                                    entropy_bits=d["topic"]["entropy_bits"], repeats_share=d["topic"]["repeats"] / d["topic"]["bytes"],
                                    value_class=d["topic"]["class"])
            elif side == "payload":
                info = h.payload_info()
                kernel[side].update(pass_kernel_ms=info["kernel_ms"], pass_workgroups=info["workgroups"], pass_over_decode_kernel=info["kernel_ms"] / float(a[1]))
            h.set_timing(False)
        line = {"bench": "value_bytes", "law": law, "records_per_batch": RPB, "value_bytes_per_record": VALUE, "records": n, "batches": int(st.n_batches),
                "raw_log_bytes": len(raw), "hbm_floor_ms": len(raw) / HBM_RATE * 1e3, "rounds": args.rounds, "steps_per_round": args.steps}
        for side in SIDES:
            line["step_ms_" + side] = statistics.median(ms[side])
            line["step_ms_%s_rounds" % side] = ms[side]
        for side in SIDES[1:]:
            ratios = [b / a for a, b in zip(ms["off"], ms[side])]
            line["ratio_%s_over_off" % side] = {"median": statistics.median(ratios), "min": min(ratios), "max": max(ratios)}
        line["pass_kernel_value_bytes_over_payload"] = kernel["value_bytes"]["pass_kernel_ms"] / kernel["payload"]["pass_kernel_ms"]
        line["pass_kernel_over_hbm_floor"] = kernel["value_bytes"]["pass_kernel_ms"] / line["hbm_floor_ms"]
        line.update({side: kernel[side] for side in SIDES})
        print(json.dumps(line), flush=True)
        lines.append(line)
        kernels[law] = kernel
        for h, blob, out in sides.values():
            h.device_batch_free(out)
            h.device_batch_free(blob)
            h.close()
        del raw, raw_np, buf
    skew = {"bench": "value_bytes", "cost_of_skew": "the pass kernel under the all-zero law over the random law",
            "a_dword_of_one_byte_combined": kernels["zero"]["value_bytes"]["pass_kernel_ms"] / kernels["random"]["value_bytes"]["pass_kernel_ms"],
            "every_byte_its_own_add": kernels["zero"]["value_bytes_single"]["pass_kernel_ms"] / kernels["random"]["value_bytes_single"]["pass_kernel_ms"],
            "all_pairs_of_a_dword": kernels["zero"]["value_bytes_pairs"]["pass_kernel_ms"] / kernels["random"]["value_bytes_pairs"]["pass_kernel_ms"]}
    print(json.dumps(skew), flush=True)
    lines.append(skew)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

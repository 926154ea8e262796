"""The payload kernel's own source on the CPU (no GPU needed): csrc/kta_payload_kernel.h compiled over tests/native/wave_emu.h
(tests/native/payload_emu.cpp, a program of its own) and run with the lanes in ascending, descending and pseudo-random
order; its vector must be np.array_equal to the restatement (tests/payload_py.py).  The blob lies between pages without
access, so a read outside what the device may read ends the program.  The cases are those of tests/test_gpu_payload.py that a
single launch can show: window edges, large values and keys, every bad header kind, value classes and ids, interleaved
partitions, LogAppendTime and the record filter, failed batches, compressed batches (inflated here by the encoder's bytes)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from kafka_topic_analyzer_amd import _native as N
import payload_blobs as B
import payload_py as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc")
P = 4
T0 = B.T0


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("payload_emu") / "payload_emu")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                        "-I", os.path.join(ROOT, "tests", "native"), os.path.join(ROOT, "tests", "native", "payload_emu.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _image(blob, raw, partition, partitions=None, failed=()):
    """(descriptors, the device's buffer after the inflate kernels): compressed batches' records at their payload_off"""
    lib, st = N.load(), N.KtaKafkaIndexStats()
    cap = max(len(R.batches_of(blob)), 1)
    descs = (N.KtaKafkaBatchDesc * cap)()
    inflate_at = (len(blob) + 127) & ~63
    assert lib.kta_kafka_index_host(blob, len(blob), partition, 0, 0, inflate_at, descs, cap, C.byref(st)) == N.KTA_OK
    image = bytearray(blob) + bytes(inflate_at - len(blob) + st.inflate_bytes)
    for i in range(st.n_batches):
        d = descs[i]
        if partitions is not None:
            d.partition = partitions[i]
        if d.byte_off in failed:
            d.status = 2
        elif d.payload_off != d.byte_off + 61:                                       # a compressed batch: as the inflate kernel leaves it
            rec = raw[d.byte_off]
            assert d.payload_off + len(rec) <= len(image)
            image[d.payload_off:d.payload_off + len(rec)] = rec
            d.payload_end = d.payload_off + len(rec)
    return descs, st.n_batches, bytes(image)


def _run(emu, tmp_path, blob, raw, partition=1, partitions=None, failed=(), flt=None, orders=(0, 1, 2), grid=0):
    descs, n, image = _image(blob, raw, partition, partitions, failed)
    lo, hi, parts = flt or (None, None, None)
    bitmap = [0] * ((P + 31) // 32)
    for p in parts or ():
        bitmap[p >> 5] |= 1 << (p & 31)
    out = None
    for order in orders:
        case, res = tmp_path / "case.bin", tmp_path / "vec.bin"
        case.write_bytes(struct.pack("<QQIIIIqq", n, len(image), P, order, 77 + order, 1 if parts is not None else 0,
                                     -2 ** 63 if lo is None else lo, 2 ** 63 - 1 if hi is None else hi) +
                         struct.pack("<%dI" % len(bitmap), *bitmap) + bytes(descs)[:88 * n] + image)
        r = subprocess.run([emu, str(case), str(res), str(grid)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("OK "), (order, r.returncode, r.stdout[-300:], r.stderr[-1000:])
        vec = np.fromfile(str(res), np.uint64)
        assert out is None or np.array_equal(out, vec), order
        out = vec
    return out


def _check(emu, tmp_path, blob, raw, partition=1, failed=(), flt=None, **kw):   # kw: orders, grid
    got = _run(emu, tmp_path, blob, raw, partition, failed=failed, flt=flt, **kw)
    want = R.restate([(blob, partition, raw, set(failed))], P, flt)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:20]
    assert all(ok for _, ok in R.identities(got, P))
    return got


@pytest.mark.parametrize("n", [1, 3, 4, 5, 9, 65])
def test_batch_counts_around_a_wave(emu, tmp_path, n):
    blob, raw = B.mixed(n, 5, seed=n)
    _check(emu, tmp_path, blob, raw)
    if n > 8:
        _check(emu, tmp_path, blob, raw, grid=2, orders=(2,))                          # two workgroups take turns


def test_more_ids_than_the_cache_has_slots_and_ids_that_share_a_slot(emu, tmp_path):
    recs = [B.record(i, B.framed(700 + (i * 37) % 100, b"b" * (i % 5))) for i in range(400)]   # 100 ids through 16 slots, again and again
    blob, raw = B.join([B.batch(40 * b, recs[40 * b:40 * b + 40]) for b in range(10)])
    got = _check(emu, tmp_path, blob, raw, grid=1, orders=(2,))
    assert len(R.schema_ids(got, P)[0]) == 100


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_records_per_batch_around_a_round(emu, tmp_path, n):
    blob, raw = B.join([B.batch(0, B.mixed_records(n, seed=n)), B.batch(n, B.mixed_records(n + 1, seed=3))])
    assert _check(emu, tmp_path, blob, raw)[R.PW + R.RECORDS] == 2 * n + 1


@pytest.mark.parametrize("value", [B.framed(0x01020304, b"tail"), b'{"json":true}', b"other"], ids=["framed", "json", "other"])
def test_a_value_at_every_offset_around_the_windows_end(emu, tmp_path, value):
    blob, raw, n = B.window_edges(value)
    assert _check(emu, tmp_path, blob, raw, orders=(2,))[R.PW + R.RECORDS] == n


def test_values_larger_than_the_window_long_records_and_a_long_key(emu, tmp_path):
    recs = B.large_records()
    blob, raw = B.join([B.batch(0, recs), B.batch(7, recs[2:3] + recs[:1] + B.mixed_records(20)), B.batch(40, recs, compression="snappy")])
    _check(emu, tmp_path, blob, raw, orders=(1,))


def test_every_bad_header_kind_first_in_the_middle_and_last(emu, tmp_path):
    good = [B.record(i, B.framed(9), headers=[(b"a", b"bc"), (b"", None)]) for i in range(19)]
    out = []
    for kind in sorted(B.BAD_HEADERS):
        for place in (0, 9, 18):
            recs = list(good)
            recs[place] = B.record(place, b'{"v":1}', raw_headers=B.BAD_HEADERS[kind])
            out.append(B.batch(19 * len(out), recs))
    blob, raw = B.join(out)
    got = _check(emu, tmp_path, blob, raw)
    assert got[R.PW + R.BAD] == 3 * len(B.BAD_HEADERS) and got[R.PW + R.HEADERS] == 2 * 18 * 3 * len(B.BAD_HEADERS)


def test_header_counts_classes_and_ids(emu, tmp_path):
    recs = [B.record(i, b"v", headers=[(b"h%d" % k, b"x" * (k % 4)) for k in range(n)]) for i, n in enumerate((0, 1, 14, 15, 16, 200))]
    recs += [B.record(6, b"v", headers=[(b"K" * 300, b"V" * 300), (b"", None)])]
    values = [None, b"", b"\x00", b"{", b"x", b"\x00abc", b"[abc", b"\x00abcd", b"{abcd", b"xabcd"] + [B.framed(i, b"") for i in (0, 1, 0x7FFFFFFF, 0xFFFFFFFF)]
    wave = [B.batch(100 + 16 * g, [B.record(i, B.framed(90000 + 16 * g + i, b"b" * i)) for i in range(16)]) for g in range(4)]   # 64 ids in one wave
    blob, raw = B.join(wave + [B.batch(0, recs), B.batch(9, [B.record(i, v) for i, v in enumerate(values)]),
                               B.batch(30, [B.record(i, B.framed(31, b"same")) for i in range(40)])])
    got = _check(emu, tmp_path, blob, raw)
    ids, ur, _ = R.schema_ids(got, P)
    assert len(ids) == 64 + 4 + 1 + 1 and ur == 0 and ids[0] == (31, 40, 360)


def test_interleaved_partitions_failed_batches_and_partitions_outside_the_range(emu, tmp_path):
    batches = [B.batch(5 * i, B.mixed_records(5, seed=i), compression=(None, "snappy")[i % 2]) for i in range(30)]
    blob, raw = B.join(batches)
    parts = [(i * 7 + i // 5) % (P + 2) - 1 for i in range(30)]
    failed = {sorted(raw)[4], sorted(raw)[11]}
    want = R.restate([(b, p, {0: r}, set()) for i, ((b, r), p) in enumerate(zip(batches, parts)) if sorted(raw)[i] not in failed], P)
    assert want[:R.PW * P:R.PW].all()
    for grid in (0, 1, 3):                                                             # a workgroup per four batches; one and three for all of them
        got = _run(emu, tmp_path, blob, raw, partitions=parts, failed=failed, grid=grid, orders=(2,) if grid else (0, 1, 2))
        assert np.array_equal(got, want), grid


@pytest.mark.parametrize("flt", [(T0 + 4000, None, None), (None, T0 + 4000, None), (T0 + 3, T0 + 9, (1, 3)), (None, None, (0,)), (None, None, (1,))])
def test_log_append_time_batches_and_the_record_filter(emu, tmp_path, flt):
    out = [B.batch(12 * b, B.mixed_records(12, seed=b), attributes=0x08 if b % 2 else 0, max_ts=T0 + 5000) for b in range(6)]
    blob, raw = B.join(out)
    got = _check(emu, tmp_path, blob, raw, flt=(flt[0], flt[1], None if flt[2] is None else set(flt[2])), orders=(2,))
    assert bool(got.any()) == (flt[2] is None or 1 in flt[2])


def test_a_record_with_bad_framing_ends_its_batch_where_the_host_statement_ends_it(emu, tmp_path):
    recs = [B.record(i, B.framed(i)) for i in range(40)]
    out = []
    for place in (0, 3, 15, 16, 17, 39):                                               # first, inside a round, at its edges, last
        r = list(recs)
        broken = bytearray(r[place])
        broken[0] += 100                                                               # a length that overruns the batch
        r[place] = bytes(broken)
        out.append(B.batch(0, r))
    negative = list(recs)
    negative[5] = b"\x01" + recs[5][1:]                                                # a negative length
    out.append(B.batch(0, negative))
    out.append(B.batch(0, recs[:7], count=9))                                          # the count promises more than the batch holds
    blob, raw = B.join(out)
    got = _check(emu, tmp_path, blob, raw)
    assert got[R.PW + R.RECORDS] == 0 + 3 + 15 + 16 + 17 + 39 + 5 + 7

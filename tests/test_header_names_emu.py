"""The header-name kernel's own source on the CPU (no GPU needed): csrc/kta_header_names_kernel.h compiled over
tests/native/wave_emu.h (tests/native/header_names_emu.cpp, a program of its own) and run with the lanes in ascending,
descending and pseudo-random order; its vector must be np.array_equal to the restatement (tests/header_names_py.py) and to the
host rule (kta_header_names_host), and every published slot of its name table must hold a name that occurred.  The blob lies
between pages without access, so a read outside what the device may read ends the program."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import header_names_blobs as HB
import header_names_py as H
import payload_blobs as B
import payload_py as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc")
P = 4
T0 = B.T0


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("header_names_emu") / "header_names_emu")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                        "-I", os.path.join(ROOT, "tests", "native"), os.path.join(ROOT, "tests", "native", "header_names_emu.cpp"), "-o", exe],
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
            image[d.payload_off:d.payload_off + len(rec)] = rec
            d.payload_end = d.payload_off + len(rec)
    return descs, st.n_batches, bytes(image)


def _run(emu, tmp_path, blob, raw, partition=1, partitions=None, failed=(), flt=None, orders=(0, 1, 2), grid=0):
    """(vector, name table, work counters) — the vector the same under every order"""
    descs, n, image = _image(blob, raw, partition, partitions, failed)
    lo, hi, parts = flt or (None, None, None)
    bitmap = [0] * ((P + 31) // 32)
    for p in parts or ():
        bitmap[p >> 5] |= 1 << (p & 31)
    out = None
    for order in orders:
        case, res = tmp_path / "case.bin", tmp_path / "out.bin"
        case.write_bytes(struct.pack("<QQIIIIqq", n, len(image), P, order, 77 + order, 1 if parts is not None else 0,
                                     -2 ** 63 if lo is None else lo, 2 ** 63 - 1 if hi is None else hi) +
                         struct.pack("<%dI" % len(bitmap), *bitmap) + bytes(descs)[:88 * n] + image)
        r = subprocess.run([emu, str(case), str(res), str(grid)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("OK "), (order, r.returncode, r.stdout[-300:], r.stderr[-1000:])
        data = res.read_bytes()
        vec = np.frombuffer(data[:8 * H.WORDS], np.uint64)
        table = np.frombuffer(data[8 * H.WORDS:8 * H.WORDS + 64 * 2048], kta.HEADER_NAME_DTYPE)
        info = np.frombuffer(data[8 * H.WORDS + 64 * 2048:], np.uint64)
        assert out is None or np.array_equal(out[0], vec), order
        out = (vec, table, info)
    return out


def _check(emu, tmp_path, blob, raw, partition=1, failed=(), flt=None, **kw):   # kw: orders, grid
    got, table, info = _run(emu, tmp_path, blob, raw, partition, failed=failed, flt=flt, **kw)
    seen = {}
    want = H.restate([(blob, partition, raw, set(failed))], P, flt, seen=seen)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:20]
    if flt is None and not failed:
        assert np.array_equal(got, kta.header_names_host(blob, partition, P)[0])   # the host rule
    assert all(ok for _, ok in H.identities(got)) and kta.header_names_identities(got)
    H.check_table(table, seen)
    return got, table, info


@pytest.mark.parametrize("n", [1, 3, 4, 5, 9, 65])
def test_batch_counts_around_a_wave(emu, tmp_path, n):
    blob, raw = B.mixed(n, 5, seed=n)
    _check(emu, tmp_path, blob, raw)
    if n > 8:
        _check(emu, tmp_path, blob, raw, grid=2, orders=(2,))                          # two workgroups take turns


@pytest.mark.parametrize("n", [15, 16, 17])
def test_records_per_batch_around_a_round(emu, tmp_path, n):
    blob, raw = B.join([B.batch(0, B.mixed_records(n, seed=n)), B.batch(n, B.mixed_records(n + 1, seed=3))])
    assert _check(emu, tmp_path, blob, raw)[0][H.LOOKED] == 2 * n + 1


@pytest.mark.parametrize("field", ["name", "value"])
def test_a_name_and_a_value_astride_the_windows_end(emu, tmp_path, field):
    blob, raw, n = HB.astride(field)
    got, table, _ = _check(emu, tmp_path, blob, raw, orders=(2,))
    assert got[H.LOOKED] == n
    blob, raw, n = B.window_edges(b"", tail=((b"a-name-of-12", b"its value"), (b"null", None)))
    assert _check(emu, tmp_path, blob, raw, orders=(1,))[0][H.LOOKED] == n


def test_long_names_empty_names_and_names_of_48_and_49_bytes(emu, tmp_path):
    recs = B.large_records()
    recs += [B.record(7, b"v", headers=[(b"e" * 48, b"1"), (b"f" * 49, b"2"), (b"e" * 48, None)])]   # the same name twice in one record
    blob, raw = B.join([B.batch(0, recs), B.batch(7, recs[2:3] + recs[:1] + B.mixed_records(20)), B.batch(40, recs, compression="snappy")])
    got, table, _ = _check(emu, tmp_path, blob, raw, orders=(1, 2))
    names = H.table_names(table)
    found, uo, _ = H.list_names(got)
    assert uo == 0 and {h for h, *_ in found} == {H.fnv1a(n) for n in (b"trace-id", b"k" * 300, b"", b"e" * 48, b"f" * 49, b"h0", b"h1", b"h2")}
    assert names[H.fnv1a(b"e" * 48)] == b"e" * 48 and names[H.fnv1a(b"f" * 49)] == b"f" * 48 and names[H.fnv1a(b"")] == b""
    slot = [e for e in table if e["state"] == 2 and e["hash"] == H.fnv1a(b"k" * 300)]
    assert slot and all(e["name_len"] == 300 for e in slot)


def test_hot_names_in_every_lane_and_64_names_in_one_wave(emu, tmp_path):
    blob, raw = HB.hot_wave()
    got, _, info = _check(emu, tmp_path, blob, raw, grid=1)
    assert info[0] == 0 and info[1] == 3                                               # no spill; a claim per name
    blob, raw, names = HB.distinct_names(64, per_record=1)
    got, table, _ = _check(emu, tmp_path, blob, raw, grid=1, orders=(2,))
    assert len(H.list_names(got)[0]) == 64


def test_200_names_in_one_workgroup_run_the_spill_path(emu, tmp_path):
    blob, raw, names = HB.distinct_names(200)
    assert H.list_names(H.restate([(blob, 1, raw, set())], P))[1] == 0                # the input leaves no remainder
    got, table, info = _check(emu, tmp_path, blob, raw, grid=1)
    assert info[0] > 0 and 0 < info[1] <= 64 and info[0] + info[1] == 200              # every name occurs once: it claims a slot or spills
    found, uo, _ = H.list_names(got)
    assert uo == 0 and {h for h, *_ in found} == {H.fnv1a(n) for n in names}
    H.check_missing(table, names)                                                      # a name without its exemplar found both its slots taken


def test_names_that_share_cells(emu, tmp_path):
    one, both = HB.colliding_names()
    for pair, listed in ((one, True), (both, False)):
        recs = [B.record(i, b"v", headers=[(pair[i % 2], b"x" * (i % 3)), (b"other", None)]) for i in range(20)]
        blob, raw = B.join([B.batch(0, recs)])
        got, _, _ = _check(emu, tmp_path, blob, raw, orders=(2,))
        found, uo, uv = H.list_names(got)
        got_list = kta.header_names_list(got)
        assert [f[:5] for f in got_list["names"]] == found and (got_list["unresolved_occurrences"], got_list["unresolved_value_bytes"]) == (uo, uv)
        hashes = {h for h, *_ in found}
        assert ({H.fnv1a(n) for n in pair} <= hashes) == listed
        assert (uo, uv) == ((0, 0) if listed else (20, sum(i % 3 for i in range(20))))


def test_every_bad_header_kind_adds_nothing(emu, tmp_path):
    good = [B.record(i, B.framed(9), headers=[(b"a", b"bc"), (b"", None)]) for i in range(19)]
    out = []
    for kind in sorted(B.BAD_HEADERS):
        for place in (0, 9, 18):
            recs = list(good)
            recs[place] = B.record(place, b'{"v":1}', raw_headers=B.BAD_HEADERS[kind])
            out.append(B.batch(19 * len(out), recs))
    blob, raw = B.join(out)
    got, _, _ = _check(emu, tmp_path, blob, raw)
    k = 3 * len(B.BAD_HEADERS)
    assert got[H.LOOKED] == 18 * k and got[H.OCC] == 2 * 18 * k and got[H.NULLS] == 18 * k


def test_interleaved_partitions_failed_batches_and_partitions_outside_the_range(emu, tmp_path):
    batches = [B.batch(5 * i, B.mixed_records(5, seed=i), compression=(None, "snappy")[i % 2]) for i in range(30)]
    blob, raw = B.join(batches)
    parts = [(i * 7 + i // 5) % (P + 2) - 1 for i in range(30)]
    failed = {sorted(raw)[4], sorted(raw)[11]}
    want = H.restate([(b, p, {0: r}, set()) for i, ((b, r), p) in enumerate(zip(batches, parts)) if sorted(raw)[i] not in failed], P)
    assert want[H.OCC]
    for grid in (0, 1, 3):
        got = _run(emu, tmp_path, blob, raw, partitions=parts, failed=failed, grid=grid, orders=(2,) if grid else (0, 1, 2))[0]
        assert np.array_equal(got, want), grid


@pytest.mark.parametrize("flt", [(T0 + 4000, None, None), (None, T0 + 4000, None), (T0 + 3, T0 + 9, (1, 3)), (None, None, (0,)), (None, None, (1,))])
def test_log_append_time_batches_and_the_record_filter(emu, tmp_path, flt):
    out = [B.batch(12 * b, B.mixed_records(12, seed=b), attributes=0x08 if b % 2 else 0, max_ts=T0 + 5000) for b in range(6)]
    blob, raw = B.join(out)
    got = _check(emu, tmp_path, blob, raw, flt=(flt[0], flt[1], None if flt[2] is None else set(flt[2])), orders=(2,))[0]
    assert bool(got.any()) == (flt[2] is None or 1 in flt[2])


def test_a_record_with_bad_framing_ends_its_batch_where_the_host_statement_ends_it(emu, tmp_path):
    recs = [B.record(i, B.framed(i), headers=[(b"n%d" % (i % 3), b"v")]) for i in range(40)]
    out = []
    for place in (0, 3, 15, 16, 17, 39):                                               # first, inside a round, at its edges, last
        r = list(recs)
        broken = bytearray(r[place])
        broken[0] += 100                                                               # a length that overruns the batch
        r[place] = bytes(broken)
        out.append(B.batch(0, r))
    out.append(B.batch(0, recs[:7], count=9))                                          # the count promises more than the batch holds
    blob, raw = B.join(out)
    assert _check(emu, tmp_path, blob, raw)[0][H.OCC] == 0 + 3 + 15 + 16 + 17 + 39 + 7

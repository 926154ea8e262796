"""The value-byte kernel's own source on the CPU (no GPU needed): csrc/kta_value_bytes_kernel.h compiled over
tests/native/wave_emu.h (tests/native/value_bytes_emu.cpp, a program of its own) with a flush threshold of 3000 bytes, and run
with the lanes in ascending, descending and pseudo-random order; its vector must be np.array_equal to the restatement
(tests/value_bytes_py.py) and to the host rule (kta_value_bytes_host), and where the input holds more than 3000 value bytes in
one group the bins must have been flushed in the middle of the pass.  The blob lies between pages without access, so a read
outside what the device may read ends the program.  Every input of tests/test_gpu_value_bytes.py but the value of 1 MiB."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import payload_blobs as B
import payload_py as R
import record_batches_blobs as RB
import value_bytes_blobs as VB
import value_bytes_py as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc")
P = 4
T0 = B.T0
FLUSH = 3000
CODECS = [c for c in B.CODECS if c != "zstd" or RB.have_zstd()]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("value_bytes_emu") / "value_bytes_emu")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                        "-I", os.path.join(ROOT, "tests", "native"), os.path.join(ROOT, "tests", "native", "value_bytes_emu.cpp"), "-o", exe],
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


def _run(emu, tmp_path, blob, raw, partition=1, partitions=None, failed=(), flt=None, orders=(0, 1, 2), grid=0, single=0):   # single: the kernel's form of combining (value_bytes_emu.cpp)
    """(vector, work counters) — the vector the same under every order"""
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
        r = subprocess.run([emu, str(case), str(res), str(grid), str(single)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("OK "), (order, r.returncode, r.stdout[-300:], r.stderr[-1000:])
        data = res.read_bytes()
        vec = np.frombuffer(data[:8 * V.words(P)], np.uint64)
        info = np.frombuffer(data[8 * V.words(P):], np.uint64)
        assert out is None or np.array_equal(out[0], vec), order
        out = (vec, info)
    return out


def _check(emu, tmp_path, blob, raw, partition=1, failed=(), flt=None, **kw):   # kw: orders, grid, single
    got, info = _run(emu, tmp_path, blob, raw, partition, failed=failed, flt=flt, **kw)
    want = V.restate([(blob, partition, raw, set(failed))], P, flt)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:20]
    if flt is None and not failed:
        assert np.array_equal(got, kta.value_bytes_host(blob, partition, P))          # the host rule
    assert all(ok for _, ok in V.identities(got, P)) and kta.value_bytes_identities(got, P)
    return got, info


def _w(v, p=1):
    return v[V.PW * p:V.PW * (p + 1)]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 64, 65])
def test_batch_counts_around_a_wave(emu, tmp_path, n):
    blob, raw = B.mixed(n, 5, seed=n)
    _check(emu, tmp_path, blob, raw)
    if n > 8:
        _check(emu, tmp_path, blob, raw, grid=2, orders=(2,))                          # two workgroups take turns
        _check(emu, tmp_path, blob, raw, orders=(1,), single=1)                        # every byte its own add
        _check(emu, tmp_path, blob, raw, orders=(0,), single=2)                        # all pairs of a dword


@pytest.mark.parametrize("n", [15, 16, 17])
def test_records_per_batch_around_a_round(emu, tmp_path, n):
    blob, raw = B.join([B.batch(0, B.mixed_records(n, seed=n)), B.batch(n, B.mixed_records(n + 1, seed=3))])
    assert _w(_check(emu, tmp_path, blob, raw)[0])[V.RECORDS] == 2 * n + 1


def test_value_lengths_around_a_dword_a_block_and_a_window_flush_in_the_middle_of_the_pass(emu, tmp_path):
    blob, raw = VB.lengths()
    got, info = _check(emu, tmp_path, blob, raw, orders=(0, 2))
    assert info[0] > 2 * 65539 // FLUSH                                               # the two long values alone take that many slices
    got1, info1 = _check(emu, tmp_path, blob, raw, orders=(1,), grid=3, single=1)
    assert info1[0] > 0 and np.array_equal(got, got1)
    small, small_raw = VB.lengths((None, 0, 1, 2, 3, 4, 5, 15, 16, 17))
    assert _check(emu, tmp_path, small, small_raw, orders=(2,))[1][0] == 0             # below the threshold: no flush but the last


def test_a_marker_astride_the_windows_end_and_values_at_every_alignment(emu, tmp_path):
    blob, raw, where = VB.astride()
    assert len(where) == 16
    got, _ = _check(emu, tmp_path, blob, raw, orders=(2,))
    assert all(_w(got)[b] >= 16 for b in range(0x41, 0x51))
    blob, raw, starts = VB.alignments()
    assert starts == set(range(16))
    _check(emu, tmp_path, blob, raw, orders=(1, 2))
    for value in (b"other", B.framed(7, b"tail")):
        blob, raw, n = B.window_edges(value)
        assert _w(_check(emu, tmp_path, blob, raw, orders=(2,))[0])[V.RECORDS] == n


def test_every_byte_value_at_every_position_of_a_dword(emu, tmp_path):
    blob, raw, residues = VB.every_byte_at_every_position()
    assert residues == {0, 1, 2, 3}
    got, _ = _check(emu, tmp_path, blob, raw, orders=(0, 2))
    assert (_w(got)[:256] >= 12).all()
    _check(emu, tmp_path, blob, raw, orders=(1,), single=1)
    _check(emu, tmp_path, blob, raw, orders=(2,), single=2)


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_one_byte_in_all_64_lanes_at_once(emu, tmp_path, byte):
    blob, raw = VB.one_byte_in_every_lane(byte)
    got, _ = _check(emu, tmp_path, blob, raw, grid=1)
    for variant in (1, 2):
        assert np.array_equal(_check(emu, tmp_path, blob, raw, grid=1, orders=(2,), single=variant)[0], got)
    w = _w(got)
    assert w[byte] == w[V.BYTES] == sum(40 + i for i in range(16)) * 4 and w[V.REPEATS] == w[V.BYTES] - w[V.VALUES] and w[V.VALUES] == 64


def test_repeats_astride_every_seam_and_neighbours_outside_the_value(emu, tmp_path):
    blob, raw, at = VB.seams()
    got, info = _check(emu, tmp_path, blob, raw)
    assert _w(got)[V.REPEATS] == len(at) > 100 and info[0] >= 2                        # the slices' seams among them
    _check(emu, tmp_path, blob, raw, orders=(2,), single=1)
    _check(emu, tmp_path, blob, raw, orders=(1,), single=2)
    blob, raw = VB.neighbours_outside_the_value()
    assert _w(_check(emu, tmp_path, blob, raw)[0])[V.REPEATS] == 1
    (const, const_raw), (alt, alt_raw) = VB.constant_and_alternating()
    w = _w(_check(emu, tmp_path, const, const_raw, orders=(2,))[0])
    assert w[V.REPEATS] == w[V.BYTES] - w[V.VALUES] > 0
    w = _w(_check(emu, tmp_path, alt, alt_raw, orders=(2,))[0])
    assert w[V.REPEATS] == 0 and w[V.BYTES] > 2000


def test_large_records_and_a_key_of_the_windows_size(emu, tmp_path):
    recs = B.large_records()
    blob, raw = B.join([B.batch(0, recs), B.batch(7, recs[2:3] + recs[:1] + B.mixed_records(20)), B.batch(40, recs, compression="snappy")])
    got, info = _check(emu, tmp_path, blob, raw, orders=(1, 2))
    assert info[0] > 0 and _w(got)[ord("w")] == 2 * 70000


def test_interleaved_partitions_failed_batches_and_partitions_outside_the_range(emu, tmp_path):
    batches = [B.batch(5 * i, B.mixed_records(5, seed=i) + [B.record(5 + k, VB.plain(1600 + i, i + k)) for k in range(2)], compression=(None, "snappy")[i % 2]) for i in range(30)]
    blob, raw = B.join(batches)
    parts = [(i * 7 + i // 5) % (P + 2) - 1 for i in range(30)]
    failed = {sorted(raw)[4], sorted(raw)[11]}
    want = V.restate([(b, p, {0: r}, set()) for i, ((b, r), p) in enumerate(zip(batches, parts)) if sorted(raw)[i] not in failed], P)
    assert want[V.BYTES::V.PW].all()
    for grid in (0, 1, 3):
        got, info = _run(emu, tmp_path, blob, raw, partitions=parts, failed=failed, grid=grid, orders=(2,) if grid else (0, 1, 2))
        assert np.array_equal(got, want), grid
        assert grid != 1 or (info[0] > 0 and info[1] > 0)                              # one workgroup: its bins overflow and change partitions


def test_every_codec_forged_counts_and_corrupt_streams(emu, tmp_path):
    blob, raw = B.mixed(3 * len(CODECS), 30, seed=2, compression=CODECS)
    _check(emu, tmp_path, blob, raw, partition=0, orders=(2,))
    out = [B.batch(0, B.mixed_records(9))]
    out.append((RB.patch(B.batch(9, B.mixed_records(3, seed=1))[0], count=1000), b""))  # a forged count: the device fails the batch
    for comp in [c for c in CODECS if c]:                                              # a stream that does not inflate
        b, r = B.batch(20, B.mixed_records(30, seed=2), compression=comp)
        out.append((RB.corrupt_stream(b, comp), r))
    out.append(B.batch(90, B.mixed_records(5, seed=3), compression="snappy"))
    blob, raw = B.join(out)
    got, _ = _check(emu, tmp_path, blob, raw, failed=set(sorted(raw)[1:-1]), orders=(2,))
    assert _w(got)[V.RECORDS] == 14


@pytest.mark.parametrize("flt", [(T0 + 4000, None, None), (None, T0 + 4000, None), (T0 + 3, T0 + 9, (1, 3)), (None, None, (0,)), (None, None, (1,))])
def test_log_append_time_batches_and_the_record_filter(emu, tmp_path, flt):
    out = [B.batch(12 * b, B.mixed_records(12, seed=b), attributes=0x08 if b % 2 else 0, max_ts=T0 + 5000) for b in range(6)]
    blob, raw = B.join(out)
    got = _check(emu, tmp_path, blob, raw, flt=(flt[0], flt[1], None if flt[2] is None else set(flt[2])), orders=(2,))[0]
    assert bool(got.any()) == (flt[2] is None or 1 in flt[2])


def test_a_record_with_bad_framing_ends_its_batch_where_the_host_statement_ends_it(emu, tmp_path):
    recs = [B.record(i, b"value-%d" % i) for i in range(40)]
    out = []
    for place in (0, 3, 15, 16, 17, 39):                                               # first, inside a round, at its edges, last
        r = list(recs)
        broken = bytearray(r[place])
        broken[0] += 100                                                               # a length that overruns the batch
        r[place] = bytes(broken)
        out.append(B.batch(0, r))
    out.append(B.batch(0, recs[:7], count=9))                                          # the count promises more than the batch holds
    blob, raw = B.join(out)
    assert _w(_check(emu, tmp_path, blob, raw)[0])[V.RECORDS] == 0 + 3 + 15 + 16 + 17 + 39 + 7

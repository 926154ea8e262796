"""GPU tests of the value-byte section (KTA_FLAG_VALUE_BYTES; no reference counterpart): the live vector that kta_value_bytes
accumulates from the records of every decode call is np.array_equal to the restatement (tests/value_bytes_py.py: np.bincount of
the encoder's own values) and its identities hold.  The kernel's geometry: 4 batches per wave (= workgroup), 16 lanes per
batch, windows of 3 KiB on 128-byte lines, 16 records per round; a value is read in dwords from the window and in 16-byte
blocks behind it.

    batch counts      1; 3 / 4 / 5; 64 / 65
    records / batch   15 / 16 / 17
    value lengths     null, 0, 1 .. 5, 15 / 16 / 17, 3071 / 3072 / 3073, 3 * 3072 + 1, 65 539; one value of 1 MiB
    window edges      a 16-byte marker whose first byte lies at every offset 3056 .. 3071 of its window; values that begin at
                      every position mod 16; payload_blobs' window edges
    bytes             all 256 byte values at every position mod 4, in the window and behind it; 0x00 / 0xFF alone in all 64 lanes
    repeats           a pair astride every seam (inside a dword, dword to dword, lane to lane, window to blob, block to block);
                      a first byte that equals the byte in front of the value; constant and alternating values
    partitions        interleaved batch by batch in one call; outside [0, P)
    codecs, failures  all five codecs in one blob; a forged count, streams that do not inflate, a failed CRC; LogAppendTime
                      batches and the record filter
    composition       kta_kafka_consume in chunks, kta_reset, the snapshot; a compaction replay; every opt-in pass at once with
                      the cross-identities to the payload section; two ranks over tests/mock_rccl.cpp
    kta-analyzer      kta.value_bytes=1 alone and with kta.gpus=2,kta.oversubscribe=1, against the golden text"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import payload_blobs as B
import payload_py as R
import record_batches_blobs as RB
import value_bytes_blobs as VB
import value_bytes_py as V
from helpers import NOW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
GOLDEN = os.path.join(ROOT, "tests", "golden", "value_bytes_cli_section.txt")
P = 4
T0 = B.T0
CODECS = [c for c in B.CODECS if c != "zstd" or RB.have_zstd()]


def _index(blob, partition):
    lib, st = N.load(), N.KtaKafkaIndexStats()
    cap = max(len(R.batches_of(blob)), 1)
    descs = (N.KtaKafkaBatchDesc * cap)()
    assert lib.kta_kafka_index_host(blob, len(blob), partition, 0, 0, (len(blob) + 127) & ~63, descs, cap, C.byref(st)) == N.KTA_OK
    return descs, st


def _decode(h, blob, partition=0, partitions=None):
    """One kta_kafka_decode_device call over the whole blob.  partitions: one per descriptor, instead of `partition`."""
    lib = N.load()
    descs, st = _index(blob, partition)
    if partitions is not None:
        assert len(partitions) == st.n_batches
        for i, p in enumerate(partitions):
            descs[i].partition = p
    out = h.device_batch_alloc(max(st.n_records, 1), 0)
    buf_bytes = ((len(blob) + 127) & ~63) + st.inflate_bytes + 128
    dev = h.device_batch_alloc(buf_bytes // 4 + 1)                 # a column serves as the raw byte buffer
    arr = np.frombuffer(blob + b"\0" * ((-len(blob)) % 4), dtype=np.uint8).copy()
    h._check(lib.kta_copy_to_device(h._ctx, dev.partition, arr.ctypes.data, arr.nbytes))
    h._check(lib.kta_kafka_decode_device(h._ctx, dev.partition, len(blob), descs, st.n_batches, st.n_records, C.byref(out), None, None))
    vec = h.value_bytes()["vector"].copy()                         # (waits for the compute stream before the buffers go)
    h.device_batch_free(out)
    h.device_batch_free(dev)
    return vec, descs, st


def _consume(h, blob, partition):
    st = N.KtaKafkaIndexStats()
    h._check(N.load().kta_kafka_consume(h._ctx, blob, len(blob), partition, C.byref(st)))
    return st


def _holds(v, P_=P, payload=None, counters=None):
    bad = [n for n, ok in V.identities(v, P_, payload, counters) if not ok]
    assert not bad, bad
    assert kta.value_bytes_identities(v, P_, payload, counters)


def _one_call(blob, raw, partition=1, failed=()):
    """the blob through one decode call; (the partition's 264 words, info), the vector checked against the restatement"""
    with kta.HipMetricHandler(P, now=NOW, value_bytes=True) as h:
        got, descs, st = _decode(h, blob, partition)
        info = h.value_bytes_info()
    want = V.restate([(blob, partition, raw, set(failed))], P)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:20]
    _holds(got)
    assert info["launches"] == 1 and info["batches"] == st.n_batches and info["workgroups"] == (st.n_batches + 3) // 4 and info["mid_flushes"] == 0
    return got[V.PW * partition:V.PW * (partition + 1)], st


# ------------------------------------------------------------------------------------------ batch counts, records, lengths
@pytest.mark.parametrize("n", [1, 3, 4, 5, 64, 65])
def test_group_and_wave_edges(n):
    blob, raw = B.mixed(n, 5, seed=n)
    _, st = _one_call(blob, raw, partition=2)
    assert st.n_batches == n


@pytest.mark.parametrize("n", [15, 16, 17])
def test_records_per_batch_around_a_round(n):
    blob, raw = B.join([B.batch(0, B.mixed_records(n, seed=n)), B.batch(n, B.mixed_records(n + 1, seed=3))])
    assert _one_call(blob, raw)[0][V.RECORDS] == 2 * n + 1


def test_value_lengths_around_a_dword_a_block_and_a_window():
    blob, raw = VB.lengths()
    w, _ = _one_call(blob, raw)
    assert w[V.BYTES] > 4 * 65539 and w[V.RECORDS] > w[V.VALUES]


def test_one_value_of_1_mib():
    big = VB.plain(1 << 20, 5)
    blob, raw = B.join([B.batch(0, [B.record(0, b"before"), B.record(1, big, key=b"key"), B.record(2, b"after")]),
                        B.batch(3, [B.record(0, b"\x00" * (1 << 20), key=None)])])
    w, _ = _one_call(blob, raw)
    assert w[V.BYTES] == 2 * (1 << 20) + 11 and w[0] >= (1 << 20) + 4096 and w[V.REPEATS] == (1 << 20) - 1


# ------------------------------------------------------------------------------------------ window edges, alignments, bytes
def test_a_marker_astride_the_windows_end_and_values_at_every_alignment():
    blob, raw, where = VB.astride()
    assert len(where) == 16
    w, _ = _one_call(blob, raw)
    assert all(w[b] >= 16 for b in range(0x41, 0x51))
    blob, raw, starts = VB.alignments()
    assert starts == set(range(16))
    _one_call(blob, raw)
    for value in (b"other", B.framed(7, b"tail")):
        blob, raw, n = B.window_edges(value)
        assert _one_call(blob, raw)[0][V.RECORDS] == n


def test_every_byte_value_at_every_position_of_a_dword():
    blob, raw, residues = VB.every_byte_at_every_position()
    assert residues == {0, 1, 2, 3}
    w, _ = _one_call(blob, raw)
    assert (w[:256] >= 12).all()


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_one_byte_in_all_64_lanes_at_once(byte):
    blob, raw = VB.one_byte_in_every_lane(byte)
    w, st = _one_call(blob, raw)
    assert st.n_batches == 4 and w[byte] == w[V.BYTES] == sum(40 + i for i in range(16)) * 4
    assert w[V.REPEATS] == w[V.BYTES] - w[V.VALUES] and w[V.VALUES] == 64


# ------------------------------------------------------------------------------------------ repeats
def test_repeats_astride_every_seam_and_neighbours_outside_the_value():
    blob, raw, at = VB.seams()
    assert _one_call(blob, raw)[0][V.REPEATS] == len(at) > 100
    blob, raw = VB.neighbours_outside_the_value()
    assert _one_call(blob, raw)[0][V.REPEATS] == 1                                    # the byte in front of a value never counts
    (const, const_raw), (alt, alt_raw) = VB.constant_and_alternating()
    w, _ = _one_call(const, const_raw)
    assert w[V.REPEATS] == w[V.BYTES] - w[V.VALUES] > 0
    w, _ = _one_call(alt, alt_raw)
    assert w[V.REPEATS] == 0 and w[V.BYTES] > 2000


def test_values_larger_than_the_window_long_records_and_a_long_key():
    recs = B.large_records()
    blob, raw = B.join([B.batch(0, recs), B.batch(7, recs[2:3] + recs[:1] + B.mixed_records(20)), B.batch(40, recs, compression="lz4")])
    assert _one_call(blob, raw)[0][ord("w")] == 2 * 70000


# ------------------------------------------------------------------------------------------ partitions, codecs, failures
def test_interleaved_partitions_and_partitions_outside_the_range():
    batches = [B.batch(5 * i, B.mixed_records(5, seed=i) + [B.record(5, VB.plain(700 + i, i))]) for i in range(90)]
    blob, _ = B.join(batches)
    parts = [(i * 7 + i // 5) % (P + 2) - 1 for i in range(90)]                       # -1 and P among them: left out entirely
    with kta.HipMetricHandler(P, now=NOW, value_bytes=True) as h:
        got, _, _ = _decode(h, blob, partitions=parts)                                # one call, a wave holds four partitions
    want = V.restate([(b, p, {0: r}, set()) for (b, r), p in zip(batches, parts)], P)
    assert np.array_equal(got, want) and want[V.BYTES::V.PW].all() and want[V.RECORDS::V.PW].sum() < 6 * 90
    _holds(got)


def test_more_batches_than_resident_workgroups_take_turns_and_change_partitions():
    kinds = [B.batch(3 * k, B.mixed_records(3, seed=k) + [B.record(3, VB.plain(50 + k, k))]) for k in range(5)]
    n = 5 * 4000
    blob = b"".join(b for b, _ in kinds) * (n // 5)
    parts = [(i // 7) % (P + 1) for i in range(n)]                                   # P among them: left out
    with kta.HipMetricHandler(P, now=NOW, value_bytes=True) as h:
        got, _, st = _decode(h, blob, partitions=parts)
        info = h.value_bytes_info()
    assert st.n_batches == n and info["workgroups"] < n // 4 and info["workgroups"] % 8 == 0
    want = np.zeros(V.words(P), np.uint64)
    for k, (b, r) in enumerate(kinds):
        for p in range(P):
            want += np.uint64(sum(1 for i in range(k, n, 5) if parts[i] == p)) * V.restate([(b, p, {0: r}, set())], P)
    assert np.array_equal(got, want) and want[V.RECORDS::V.PW].all()
    _holds(got)


def test_all_codecs_in_one_blob():
    blob, raw = B.mixed(3 * len(CODECS), 30, seed=2, compression=CODECS)
    _one_call(blob, raw, partition=0)
    assert {b["codec"] for b in R.batches_of(blob)} == set(range(len(CODECS)))


def test_forged_counts_and_corrupt_streams_add_nothing():
    out = [B.batch(0, B.mixed_records(9))]
    out.append((RB.patch(B.batch(9, B.mixed_records(3, seed=1))[0], count=1000), b""))   # a forged count
    for comp in [c for c in CODECS if c]:                                              # a stream that does not inflate
        b, raw = B.batch(20, B.mixed_records(30, seed=2), compression=comp)
        out.append((RB.corrupt_stream(b, comp), raw))
    out.append(B.batch(90, B.mixed_records(5, seed=3), compression="snappy"))
    blob, raw = B.join(out)
    assert _one_call(blob, raw, failed=set(sorted(raw)[1:-1]))[0][V.RECORDS] == 14


def test_a_failed_batch_under_check_crcs_adds_nothing():
    good, (b, raw) = B.batch(0, B.mixed_records(3)), B.batch(3, B.mixed_records(4, seed=8))
    bad = b[:70] + bytes([b[70] ^ 1]) + b[71:]                                      # one bit inside the CRC's range (a timestamp delta)
    blob = good[0] + bad + good[0]
    raws = {0: good[1], len(good[0]): raw, len(good[0]) + len(bad): good[1]}
    with kta.HipMetricHandler(P, now=NOW, value_bytes=True) as h:
        h._check(N.load().kta_kafka_set_check_crcs(h._ctx, 1))
        got, _, _ = _decode(h, blob, 0)
    assert np.array_equal(got, V.restate([(blob, 0, raws, {len(good[0])})], P)) and got[V.RECORDS] == 6


@pytest.mark.parametrize("flt", [None, (T0 + 4000, None, None), (None, T0 + 4000, None), (T0 + 3, T0 + 9, None), (T0 + 3, None, (1, 3)), (None, None, (0,))])
def test_log_append_time_batches_and_the_record_filter(flt):
    sets = []
    for p in range(P):
        out = []
        for b in range(6):                                                           # create time: T0 + the record's delta; append time: max_ts
            recs = B.mixed_records(12, seed=10 * p + b)
            out.append(B.batch(12 * b, recs, attributes=0x08 if b % 2 else 0, max_ts=T0 + 5000, compression=CODECS[b % len(CODECS)]))
        blob, raw = B.join(out)
        sets.append((blob, p, raw, set()))
    want = V.restate(sets, P, None if flt is None else (flt[0], flt[1], None if flt[2] is None else set(flt[2])))
    with kta.HipMetricHandler(P, now=NOW, value_bytes=True) as h:
        if flt is not None:
            h.set_filter(*flt)
        for blob, p, _, _ in sets:
            _consume(h, blob, p)
        got = h.value_bytes()["vector"]
    assert np.array_equal(got, want)
    _holds(got)
    whole = V.restate(sets, P)
    assert (flt is None) == bool(np.array_equal(want, whole)) and 0 < want[V.RECORDS::V.PW].sum() <= whole[V.RECORDS::V.PW].sum()


# ------------------------------------------------------------------------------------------ submission paths
def test_consume_in_chunks_accumulates_resets_and_snapshots():
    blob, raw = B.mixed(300, 6, seed=21)
    other, other_raw = B.mixed(40, 4, seed=22)
    want = V.restate([(blob, 2, raw, set())], P)
    with kta.HipMetricHandler(P, now=NOW, value_bytes=True) as h:
        h._check(N.load().kta_kafka_configure(h._ctx, 8192, 3))                     # a few dozen batches per staging blob
        st = _consume(h, blob, 2)
        assert st.n_batches == 300 and h.value_bytes_info()["launches"] > 5
        got = h.value_bytes()
        assert np.array_equal(got["vector"], want) and got["topic"] == V.summary(V.topic(want, P)) | {"entropy_bits": got["topic"]["entropy_bits"]}
        h.finish()
        _holds(got["vector"], counters=h.result_vector_host())                      # records == total_messages
        assert np.array_equal(h.exchange_value_bytes()["vector"], want) and np.array_equal(h.value_bytes()["vector"], want)
        _consume(h, other, 0)                                                       # a second call accumulates
        both = V.restate([(blob, 2, raw, set()), (other, 0, other_raw, set())], P)
        assert np.array_equal(h.value_bytes()["vector"], both)
        assert np.array_equal(h.exchange_value_bytes()["vector"], want)             # the snapshot is finish()'s
        h.reset()
        assert not h.value_bytes()["vector"].any() and h.value_bytes_info()["mid_flushes"] == 0
        _consume(h, other, 0)
        assert np.array_equal(h.value_bytes()["vector"], V.restate([(other, 0, other_raw, set())], P))


def test_a_compaction_replay_counts_nothing_twice():
    blob, raw = B.mixed(100, 5, seed=41)
    want = V.restate([(blob, 1, raw, set())], P)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True, value_bytes=True) as h:
        _consume(h, blob, 1)
        h.finish()
        launches = h.value_bytes_info()["launches"]
        with h.compaction_replay():
            _consume(h, blob, 1)
        assert h.value_bytes_info()["launches"] == launches                         # the pass is skipped
        assert np.array_equal(h.value_bytes()["vector"], want)


EVERYTHING = dict(count_alive_keys=True, analytics=True, key_sketch=True, hot_keys=True, ts_order=True, partitioner=True, compaction=True,
                  size_quantiles=True, timeline=(T0, 1000, 8), segments=(4096, 4, 70), compact_delete=True, record_batches=True, payload=True,
                  header_names=True)
OTHER_SECTIONS = ("analytics", "timeline", "key_sketch", "hot_keys", "ts_order", "partitioner", "size_quantiles", "segments", "get_record_batches",
                  "get_payload", "header_names")


def _flat(x):
    if isinstance(x, dict) and "vector" in x:
        return np.asarray(x["vector"]).reshape(-1)
    if isinstance(x, dict):
        return np.concatenate([np.asarray(x[k]).reshape(-1).view(np.uint64) for k in sorted(x)])
    return np.asarray(x).reshape(-1)


def test_every_pass_on_at_once_and_no_side_effects_on_the_others():
    sets = [B.mixed(60, 4, seed=50 + p) + (p,) for p in range(P)]
    want = V.restate([(blob, p, raw, set()) for blob, raw, p in sets], P)
    state = {}
    for on in (False, True):
        with kta.HipMetricHandler(P, now=NOW, value_bytes=on, **EVERYTHING) as h:
            for blob, _, p in sets:
                _consume(h, blob, p)
            h.finish()
            state[on] = {s: _flat(getattr(h, s)()).copy() for s in OTHER_SECTIONS}
            state[on]["counters"] = h.result_vector_host()
            if on:
                got = h.value_bytes()["vector"]
                assert np.array_equal(got, want)
                _holds(got, payload=state[on]["get_payload"], counters=state[on]["counters"])   # the identities between the sections
            else:
                for call in (h.value_bytes, h.exchange_value_bytes, h.value_bytes_info, h.value_bytes_vector, h.value_bytes_result_vector):
                    with pytest.raises(kta.KtaError, match="KTA_FLAG_VALUE_BYTES"):
                        call()
    for name in state[True]:
        assert np.array_equal(state[True][name], state[False][name]), name


# ------------------------------------------------------------------------------------------ two ranks
@pytest.fixture(scope="module")
def mock_rccl(tmp_path_factory):
    lib = tmp_path_factory.mktemp("mock") / "libmock_rccl.so"
    r = subprocess.run(["timeout", "-k", "10", "600", "/opt/rocm/bin/hipcc", "-O1", "-shared", "-fPIC", "-std=c++17",
                        os.path.join(ROOT, "tests", "mock_rccl.cpp"), "-o", str(lib), "-lrt", "-lpthread"],
                       capture_output=True, text=True, timeout=660)
    assert r.returncode == 0, r.stderr[-2000:]
    return str(lib)


_EXCHANGE_WORKER = r'''
import ctypes as C, os, sys, threading
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import value_bytes_py as V
import payload_blobs as B
from helpers import NOW

P, nranks = 5, 2
sets = []
for p in range(P):
    blob, raw = B.mixed(20 + 7 * p, 6, seed=80 + p, compression=[None, "snappy", "lz4"])
    sets.append((blob, p, raw, set()))
want = V.restate(sets, P)
assert want[V.BYTES::V.PW].all() and all(ok for _, ok in V.identities(want, P))
uid = kta.HipMetricHandler.comm_unique_id()
def run(rank):
    try:
        h = kta.HipMetricHandler(P, now=NOW, value_bytes=True)
        h.comm_create(nranks, rank, uid)
        mine = [s for s in sets if s[1] % nranks == rank]
        for blob, p, raw, failed in mine:
            st = N.KtaKafkaIndexStats()
            h._check(N.load().kta_kafka_consume(h._ctx, blob, len(blob), p, C.byref(st)))
        h.exchange()
        assert np.array_equal(h.exchange_value_bytes()["vector"], want), (rank, "exchanged")
        assert np.array_equal(h.value_bytes()["vector"], V.restate(mine, P)), (rank, "own")
        h.exchange()
        assert np.array_equal(h.exchange_value_bytes()["vector"], want), (rank, "again")
        h.sync()
        h.comm_destroy(); h.close()
    except BaseException as e:
        print("rank %d: %r" % (rank, e), file=sys.stderr, flush=True)
        os._exit(2)        # the other rank would wait in its collective for ever
ts = [threading.Thread(target=run, args=(r,)) for r in range(nranks)]
[t.start() for t in ts]; [t.join() for t in ts]
print("OK")
'''


def test_exchange_on_two_ranks_ends_with_the_unsharded_vector(tmp_path, mock_rccl):
    script = tmp_path / "exchange_worker.py"
    script.write_text(_EXCHANGE_WORKER)
    env = dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=330, env=env)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.stdout[-2000:], r.stderr[-3000:])


# ------------------------------------------------------------------------------------------ the CLI
def _cli(*args, env=None):
    return subprocess.run(["timeout", "-k", "10", "240", CLI, *args], capture_output=True, text=True, timeout=270, env=env)


def _normalise(text):
    text = re.sub(r"Scanning took: \d+ seconds", "Scanning took: 3 seconds", text)
    return re.sub(r"Estimated Msg/s: \d+", "Estimated Msg/s: 133", text)


def test_cli_prints_the_section_alone_and_on_two_ranks(tmp_path, mock_rccl):
    sets, files = [], []
    for p in range(2):
        blob, raw = B.mixed(40 + 10 * p, 6, seed=60 + p, compression=[None, "snappy", "lz4", "gzip"])
        path = tmp_path / ("%d.log" % p)
        path.write_bytes(blob)
        files.append(str(path))
        sets.append((blob, p, raw, set()))
    src = "segment://" + ",".join(files)
    v = V.restate(sets, 2)
    assert V.decimals_clear_of_a_tie(v, 2)
    want = open(GOLDEN).read()
    assert want == V.section(v, 2) == kta.render_value_bytes(v, 2)
    plain = _cli("-t", "seg", "-b", src)
    one = _cli("-t", "seg", "-b", src, "--librdkafka", "kta.value_bytes=1")
    assert plain.returncode == 0 and one.returncode == 0, one.stderr
    assert "Value bytes:" not in plain.stdout
    at = one.stdout.index("Value bytes: a byte histogram")
    assert one.stdout[at:] == want and _normalise(one.stdout[:at]) == _normalise(plain.stdout)
    both = _cli("-t", "seg", "-b", src, "--librdkafka", "kta.value_bytes=1,kta.headers=1,kta.payload=1")
    assert both.returncode == 0, both.stderr
    assert both.stdout.endswith(want) and both.stdout.index("Payload: value formats") < both.stdout.index("Header names: a census") < both.stdout.index("Value bytes:")
    # two ranks, both on the one reachable GPU, RCCL replaced by tests/mock_rccl.cpp (real RCCL refuses two ranks on one device)
    ranks = _cli("-t", "seg", "-b", src, "--librdkafka", "kta.value_bytes=1,kta.gpus=2,kta.oversubscribe=1", env=dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl))
    assert ranks.returncode == 0, ranks.stderr
    assert ranks.stdout.endswith(want)
    flt = _cli("-t", "seg", "-b", src, "-c", "--librdkafka", "kta.value_bytes=1,kta.partitions=1")
    assert flt.returncode == 0, flt.stderr
    assert flt.stdout.endswith(V.section(V.restate(sets, 2, (None, None, {1})), 2))

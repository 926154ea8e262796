"""GPU tests of the header-name section (KTA_FLAG_HEADER_NAMES; no reference counterpart): the live vector that kta_header_names
accumulates from the records of every decode call is np.array_equal to the restatement (tests/header_names_py.py, which walks
the encoder's own record bytes), and every published slot of the name table holds a name that occurred.  The kernel's
geometry is the payload kernel's: 4 batches per wave (= workgroup), 16 lanes per batch, windows of 3 KiB, 16 records per round;
its cache holds 64 names per workgroup.

    batch counts      1; 3 / 4 / 5; 64 / 65
    records / batch   15 / 16 / 17
    window edges      a 16-byte name and a 16-byte value with the window's end behind each of their bytes; window_edges with a
                      name in its tail; large_records(): a 300-byte name, an empty name with a null value, hs * 5
    names             48 and 49 bytes (the exemplar full, and truncated with its length kept); the same name twice in a record;
                      a few names hot in all 64 lanes; 64 distinct names in one wave; 200 distinct names in one workgroup (the
                      spill path ran, by the work counter); a pair that shares its row-0 cell (both listed) and a pair that
                      shares both cells (neither listed, the remainder their sums)
    nothing           every bad header kind; partitions outside [0, P); forged counts and corrupt streams
    filter            the cases of test_gpu_payload.py's last parametrisation
    submission        kta_kafka_consume in chunks, kta_reset, the snapshot; a compaction replay; every opt-in pass on at once
    exchange          two ranks over tests/mock_rccl.cpp
    kta-analyzer      kta.headers=1 alone, with kta.payload=1, and with kta.gpus=2,kta.oversubscribe=1

A test that asserts that names are listed uses at most 200 distinct names and first asserts on the CPU that the restatement's
peel leaves no remainder for its input."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import header_names_blobs as HB
import header_names_py as H
import payload_blobs as B
import payload_py as R
import record_batches_blobs as RB
from helpers import NOW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
P = 4
T0 = B.T0
CODECS = [c for c in B.CODECS if c != "zstd" or RB.have_zstd()]


def _decode(h, blob, partition=0, partitions=None):
    """One kta_kafka_decode_device call over the whole blob.  partitions: one per descriptor, instead of `partition`."""
    lib, st = N.load(), N.KtaKafkaIndexStats()
    cap = max(len(R.batches_of(blob)), 1)
    descs = (N.KtaKafkaBatchDesc * cap)()
    assert lib.kta_kafka_index_host(blob, len(blob), partition, 0, 0, (len(blob) + 127) & ~63, descs, cap, C.byref(st)) == N.KTA_OK
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
    got = h.header_names()                                         # (waits for the compute stream before the buffers go)
    h.device_batch_free(out)
    h.device_batch_free(dev)
    return got, st


def _consume(h, blob, partition):
    st = N.KtaKafkaIndexStats()
    h._check(N.load().kta_kafka_consume(h._ctx, blob, len(blob), partition, C.byref(st)))
    return st


def _holds(v, payload=None):
    bad = [n for n, ok in H.identities(v, payload, P) if not ok]
    assert not bad, bad
    assert kta.header_names_identities(v, payload, P if payload is not None else 0)


def _run(blob, raw, partition=1, failed=(), listed=None):
    seen = {}
    want = H.restate([(blob, partition, raw, set(failed))], P, seen=seen)
    if listed is not None:
        assert len(seen) <= 200 and H.list_names(want)[1] == 0                         # the input's own peel: no remainder
    with kta.HipMetricHandler(P, now=NOW, header_names=True) as h:
        got, st = _decode(h, blob, partition)
        table = h.header_name_table()
        info = h.header_names_info()
    v = got["vector"]
    assert np.array_equal(v, want), np.flatnonzero(v != want)[:20]
    _holds(v)
    H.check_table(table, seen)
    if listed is not None:
        found = H.list_names(v)
        assert found[1] == 0 and {h_ for h_, *_ in found[0]} == {H.fnv1a(n) for n in listed}
        assert [f[:5] for f in got["names"]["names"]] == found[0] and got["names"]["unresolved_occurrences"] == 0
    return v, table, info, st


# ------------------------------------------------------------------------------------------ batch counts, records
@pytest.mark.parametrize("n", [1, 3, 4, 5, 64, 65])
def test_group_and_wave_edges(n):
    blob, raw = B.mixed(n, 5, seed=n)
    v, _, info, st = _run(blob, raw, 2)
    assert st.n_batches == n and info["launches"] == 1 and info["batches"] == n and info["workgroups"] == (n + 3) // 4


@pytest.mark.parametrize("n", [15, 16, 17])
def test_records_per_batch_around_a_round(n):
    blob, raw = B.join([B.batch(0, B.mixed_records(n, seed=n)), B.batch(n, B.mixed_records(n + 1, seed=3))])
    v, _, _, st = _run(blob, raw)
    assert v[H.LOOKED] == 2 * n + 1 == st.n_records


# ------------------------------------------------------------------------------------------ window edges
@pytest.mark.parametrize("field", ["name", "value"])
def test_a_name_and_a_value_astride_the_windows_end(field):
    blob, raw, n = HB.astride(field)
    v, table, _, _ = _run(blob, raw, listed=[bytes(range(0x41, 0x51)) if field == "name" else b"n", b"null"])
    assert v[H.LOOKED] == n


def test_window_edges_with_a_name_in_the_tail():
    blob, raw, n = B.window_edges(b"", tail=((b"a-name-of-12", b"its value"), (b"null", None)))
    assert _run(blob, raw, listed=[b"a-name-of-12", b"null"])[0][H.LOOKED] == n


def test_large_records_long_names_and_names_of_48_and_49_bytes():
    recs = B.large_records()
    recs += [B.record(7, b"v", headers=[(b"e" * 48, b"1"), (b"f" * 49, b"2"), (b"e" * 48, None)])]   # the same name twice in one record
    blob, raw = B.join([B.batch(0, recs), B.batch(7, recs[2:3] + recs[:1] + B.mixed_records(20)), B.batch(40, recs, compression="lz4")])
    v, table, _, _ = _run(blob, raw, listed=[b"trace-id", b"k" * 300, b"", b"e" * 48, b"f" * 49, b"h0", b"h1", b"h2"])
    names = H.table_names(table)
    assert names[H.fnv1a(b"e" * 48)] == b"e" * 48 and names[H.fnv1a(b"f" * 49)] == b"f" * 48 and names[H.fnv1a(b"")] == b""
    slot = [e for e in table if e["state"] == 2 and e["hash"] == H.fnv1a(b"k" * 300)]
    assert slot and all(e["name_len"] == 300 for e in slot)
    text = kta.render_header_names(v, table)
    assert text == H.section(v, names) and "f" * 48 + "..." in text and "k" * 48 + "..." in text


# ------------------------------------------------------------------------------------------ the cache
def test_a_few_names_hot_in_all_lanes():
    blob, raw = HB.hot_wave(8, 16)                                                     # two waves of 64 records, three names on each
    v, _, info, _ = _run(blob, raw, listed=[b"traceparent", b"correlation-id", b"__replicated-from"])
    assert v[H.OCC] == 3 * 128 and info["spills"] == 0 and info["claims"] == 3 * 2


def test_64_distinct_names_in_one_wave():
    blob, raw, names = HB.distinct_names(64, per_record=1)
    v, _, info, st = _run(blob, raw, listed=names)
    assert st.n_batches == 4 and info["workgroups"] == 1 and info["spills"] + info["claims"] == 64


def test_200_distinct_names_in_one_workgroup_run_the_spill_path():
    blob, raw, names = HB.distinct_names(200, per_record=4, per_batch=13)             # 50 records in 4 batches: one workgroup
    v, table, info, st = _run(blob, raw, listed=names)
    assert st.n_batches == 4 and info["workgroups"] == 1
    assert info["spills"] >= 200 - 64 and info["spills"] + info["claims"] == 200      # the cache has 64 slots: the rest went past it
    H.check_missing(table, names)                                                      # a name without its exemplar found both its slots taken


def test_names_that_share_cells():
    one, both = HB.colliding_names()
    assert H.cell(0, H.fnv1a(one[0])) == H.cell(0, H.fnv1a(one[1])) and H.cell(1, H.fnv1a(one[0])) != H.cell(1, H.fnv1a(one[1]))
    assert all(H.cell(r, H.fnv1a(both[0])) == H.cell(r, H.fnv1a(both[1])) for r in (0, 1)) and H.fnv1a(both[0]) != H.fnv1a(both[1])
    recs = [B.record(i, b"v", headers=[(one[i % 2], b"x" * (i % 3)), (b"other", None)]) for i in range(20)]
    blob, raw = B.join([B.batch(0, recs)])
    _run(blob, raw, listed=[one[0], one[1], b"other"])                                 # both are listed exactly
    recs = [B.record(i, b"v", headers=[(both[i % 2], b"x" * (i % 3)), (b"other", None)]) for i in range(20)]
    blob, raw = B.join([B.batch(0, recs)])
    v, table, _, _ = _run(blob, raw)
    read = kta.header_names_list(v, table)
    assert [n[0] for n in read["names"]] == [H.fnv1a(b"other")] and read["names"][0][5] == b"other"   # neither is listed
    assert (read["unresolved_occurrences"], read["unresolved_value_bytes"]) == (20, sum(i % 3 for i in range(20))) == H.list_names(v)[1:]


# ------------------------------------------------------------------------------------------ what adds nothing
def test_every_bad_header_kind_adds_nothing():
    good = [B.record(i, B.framed(9), headers=[(b"a", b"bc"), (b"", None)]) for i in range(19)]      # more than a round
    out = []
    for kind in sorted(B.BAD_HEADERS):
        for place in (0, 9, 18):
            recs = list(good)
            recs[place] = B.record(place, b'{"v":1}', raw_headers=B.BAD_HEADERS[kind])
            out.append(B.batch(19 * len(out), recs))
    blob, raw = B.join(out)
    v, _, _, _ = _run(blob, raw, listed=[b"a", b""])
    k = 3 * len(B.BAD_HEADERS)
    assert (v[H.LOOKED], v[H.OCC], v[H.NULLS], v[H.NAMEB], v[H.VALB]) == (18 * k, 36 * k, 18 * k, 18 * k, 36 * k)


def test_interleaved_partitions_and_partitions_outside_the_range():
    batches = [B.batch(5 * i, B.mixed_records(5, seed=i)) for i in range(90)]
    blob, _ = B.join(batches)
    parts = [(i * 7 + i // 5) % (P + 2) - 1 for i in range(90)]                       # -1 and P among them: left out entirely
    with kta.HipMetricHandler(P, now=NOW, header_names=True) as h:
        got, _ = _decode(h, blob, partitions=parts)
    want = H.restate([(b, p, {0: r}, set()) for (b, r), p in zip(batches, parts)], P)
    whole = H.restate([(b, 0, {0: r}, set()) for b, r in batches], P)
    assert np.array_equal(got["vector"], want) and 0 < want[H.LOOKED] < whole[H.LOOKED]


def test_forged_counts_and_corrupt_streams_add_nothing():
    out = [B.batch(0, B.mixed_records(9))]
    out.append((RB.patch(B.batch(9, B.mixed_records(3, seed=1))[0], count=1000), b""))           # forged count
    for comp in [c for c in CODECS if c]:                                                      # a stream that does not inflate
        b, raw = B.batch(20, B.mixed_records(30, seed=2), compression=comp)
        out.append((RB.corrupt_stream(b, comp), raw))
    out.append(B.batch(90, B.mixed_records(5, seed=3), compression="snappy"))
    blob, raw = B.join(out)
    v, _, _, _ = _run(blob, raw, failed=set(sorted(raw)[1:-1]))
    assert v[H.LOOKED] == 14


# ------------------------------------------------------------------------------------------ filter
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
    want = H.restate(sets, P, None if flt is None else (flt[0], flt[1], None if flt[2] is None else set(flt[2])))
    with kta.HipMetricHandler(P, now=NOW, header_names=True) as h:
        if flt is not None:
            h.set_filter(*flt)
        for blob, p, _, _ in sets:
            _consume(h, blob, p)
        got = h.header_names()["vector"]
    assert np.array_equal(got, want)
    _holds(got)
    whole = H.restate(sets, P)
    assert (flt is None) == bool(np.array_equal(want, whole)) and 0 < want[H.LOOKED] <= whole[H.LOOKED]


# ------------------------------------------------------------------------------------------ submission paths
def test_consume_in_chunks_accumulates_resets_and_snapshots():
    blob, raw = B.mixed(300, 6, seed=21)
    other, other_raw = B.mixed(40, 4, seed=22)
    seen = {}
    want = H.restate([(blob, 2, raw, set())], P, seen=seen)
    with kta.HipMetricHandler(P, now=NOW, header_names=True) as h:
        h._check(N.load().kta_kafka_configure(h._ctx, 8192, 3))                     # a few dozen batches per staging blob
        st = _consume(h, blob, 2)
        assert st.n_batches == 300 and h.header_names_info()["launches"] > 5
        assert np.array_equal(h.header_names()["vector"], want)
        h.finish()
        assert np.array_equal(h.exchange_header_names()["vector"], want) and np.array_equal(h.header_names()["vector"], want)
        H.check_table(h.header_name_table(), seen)
        assert len(H.table_names(h.header_name_table())) == 3
        _consume(h, other, 0)                                                       # a second call accumulates
        both = H.restate([(blob, 2, raw, set()), (other, 0, other_raw, set())], P)
        assert np.array_equal(h.header_names()["vector"], both)
        assert np.array_equal(h.exchange_header_names()["vector"], want)            # the snapshot is finish()'s
        h.reset()
        assert not h.header_names()["vector"].any() and not h.header_name_table()["state"].any()
        assert h.header_names_info()["claims"] == 0
        _consume(h, other, 0)
        assert np.array_equal(h.header_names()["vector"], H.restate([(other, 0, other_raw, set())], P))


def test_a_compaction_replay_counts_nothing_twice():
    blob, raw = B.mixed(100, 5, seed=41)
    want = H.restate([(blob, 1, raw, set())], P)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True, header_names=True) as h:
        _consume(h, blob, 1)
        h.finish()
        launches = h.header_names_info()["launches"]
        with h.compaction_replay():
            _consume(h, blob, 1)
        assert h.header_names_info()["launches"] == launches
        assert np.array_equal(h.header_names()["vector"], want)


EVERYTHING = dict(count_alive_keys=True, analytics=True, key_sketch=True, hot_keys=True, ts_order=True, partitioner=True, compaction=True,
                  size_quantiles=True, timeline=(T0, 1000, 8), segments=(4096, 4, 70), compact_delete=True, record_batches=True, payload=True)
OTHER_SECTIONS = ("analytics", "timeline", "key_sketch", "hot_keys", "ts_order", "partitioner", "size_quantiles", "segments", "get_record_batches",
                  "get_payload")


def _flat(x):
    if isinstance(x, dict) and "vector" in x:
        return np.asarray(x["vector"]).reshape(-1)
    if isinstance(x, dict):
        return np.concatenate([np.asarray(x[k]).reshape(-1).view(np.uint64) for k in sorted(x)])
    return np.asarray(x).reshape(-1)


def test_every_pass_on_at_once_and_no_side_effects_on_the_others():
    sets = [B.mixed(60, 4, seed=50 + p) + (p,) for p in range(P)]
    want = H.restate([(blob, p, raw, set()) for blob, raw, p in sets], P)
    state = {}
    for on in (False, True):
        with kta.HipMetricHandler(P, now=NOW, header_names=on, **EVERYTHING) as h:
            for blob, _, p in sets:
                _consume(h, blob, p)
            h.finish()
            state[on] = {s: _flat(getattr(h, s)()).copy() for s in OTHER_SECTIONS}
            state[on]["counters"] = h.result_vector_host()
            if on:
                got = h.header_names()["vector"]
                assert np.array_equal(got, want)
                _holds(got, payload=state[on]["get_payload"])                       # the identities between the two sections
            else:
                for call in (h.header_names, h.exchange_header_names, h.header_name_table, h.header_names_info, h.header_names_vector,
                             h.header_names_result_vector):
                    with pytest.raises(kta.KtaError, match="KTA_FLAG_HEADER_NAMES"):
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
import header_names_py as H
import payload_blobs as B
from helpers import NOW

P, nranks = 5, 2
sets = []
for p in range(P):
    blob, raw = B.mixed(20 + 7 * p, 6, seed=80 + p, compression=[None, "snappy", "lz4"])
    sets.append((blob, p, raw, set()))
want = H.restate(sets, P)
assert want[H.OCC] and all(ok for _, ok in H.identities(want))
uid = kta.HipMetricHandler.comm_unique_id()
def run(rank):
    try:
        h = kta.HipMetricHandler(P, now=NOW, header_names=True)
        h.comm_create(nranks, rank, uid)
        mine = [s for s in sets if s[1] % nranks == rank]
        for blob, p, raw, failed in mine:
            st = N.KtaKafkaIndexStats()
            h._check(N.load().kta_kafka_consume(h._ctx, blob, len(blob), p, C.byref(st)))
        h.exchange()
        assert np.array_equal(h.exchange_header_names()["vector"], want), (rank, "exchanged")
        assert np.array_equal(h.header_names()["vector"], H.restate(mine, P)), (rank, "own")
        h.exchange()
        assert np.array_equal(h.exchange_header_names()["vector"], want), (rank, "again")
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


def test_cli_prints_the_section_alone_with_payload_and_on_two_ranks(tmp_path, mock_rccl):
    sets, files = [], []
    for p in range(2):
        recs_sets = B.mixed(40 + 10 * p, 6, seed=60 + p, compression=[None, "snappy", "lz4", "gzip"])
        path = tmp_path / ("%d.log" % p)
        path.write_bytes(recs_sets[0])
        files.append(str(path))
        sets.append((recs_sets[0], p, recs_sets[1], set()))
    src = "segment://" + ",".join(files)
    seen = {}
    v = H.restate(sets, 2, seen=seen)
    assert H.list_names(v)[1] == 0 and len(seen) <= 200                               # the input's own peel: no remainder
    want = H.section(v, {h: min(names) for h, names in seen.items()})
    plain = _cli("-t", "seg", "-b", src)
    one = _cli("-t", "seg", "-b", src, "--librdkafka", "kta.headers=1")
    assert plain.returncode == 0 and one.returncode == 0, one.stderr
    assert "Header names:" not in plain.stdout
    at = one.stdout.index("Header names: a census")
    assert one.stdout[at:] == want and _normalise(one.stdout[:at]) == _normalise(plain.stdout)
    assert "| h0 " in want and "n/a" not in want
    two = _cli("-t", "seg", "-b", src, "--librdkafka", "kta.headers=1,kta.payload=1")
    assert two.returncode == 0, two.stderr
    assert two.stdout.endswith(want) and two.stdout.index("Payload: value formats") < two.stdout.index("Header names: a census")
    # two ranks, both on the one reachable GPU, RCCL replaced by tests/mock_rccl.cpp (real RCCL refuses two ranks on one device)
    ranks = _cli("-t", "seg", "-b", src, "--librdkafka", "kta.headers=1,kta.gpus=2,kta.oversubscribe=1", env=dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl))
    assert ranks.returncode == 0, ranks.stderr
    assert ranks.stdout.endswith(want)
    flt = _cli("-t", "seg", "-b", src, "-c", "--librdkafka", "kta.headers=1,kta.partitions=1")
    assert flt.returncode == 0, flt.stderr
    assert flt.stdout.endswith(H.section(H.restate(sets, 2, (None, None, {1})), {h: min(names) for h, names in seen.items()}))

"""GPU tests of the payload section (KTA_FLAG_PAYLOAD; no reference counterpart): the live vector that kta_payload accumulates
from the records of every decode call is np.array_equal to the restatement (tests/payload_py.py, which walks the encoder's own
record bytes).  The kernel's geometry: 4 batches per wave (= workgroup), 16 lanes per batch, windows of 3 KiB on 128-byte
lines, 16 records per round.

    batch counts      1; 3 / 4 / 5 and 7 / 8 / 9 (group of lanes, wave and workgroup are all 4 batches); 63 / 64 / 65; 257; 20 000
                      (more fours than the grid has workgroups: they take turns), the partition changing every 7 batches
    records / batch   1; 15 / 16 / 17 (lanes per group, and one more than a round holds); 33
    byte offsets      byte_off at every residue mod 16
    window edges      a value whose first byte lies at every offset 3064 .. 3079 of its window (the last valid byte, the head
                      astride the end, the value length astride the end); a value larger than the window with headers behind
                      it; records of 8 KiB and more; a null value followed by headers; a key of the window's size
    headers           0, 1, 14, 15, 16 and 200 of them; a null value, an empty key, a 300-byte key; every bad kind first, in the
                      middle and last in a batch
    value classes     every class at lengths 0, 1, 4, 5; ids 0, 1, 2^31 - 1, 2^32 - 1; 64 distinct ids in one wave; one id
                      throughout; a pair that collides in both rows of the table
    codecs, flags     all five codecs in one blob; LogAppendTime batches with and without a time filter
    partitions        interleaved batch by batch in one call; outside [0, P); a forged count, streams that do not inflate, a bad
                      CRC under check.crcs: nothing
    submission        kta_kafka_consume in chunks; two calls accumulate; kta_reset; get after finish; a compaction replay;
                      every opt-in pass on at once; counters and every other section identical with the flag on and off
    kta-analyzer      kta.payload=1 on a two-partition segment:// fixture, behind the unchanged report"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import payload_blobs as B
import payload_py as R
import record_batches_blobs as RB
from helpers import NOW
from test_payload_host import double_collision

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
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
    vec = h.get_payload()["vector"].copy()                         # (waits for the compute stream before the buffers go)
    h.device_batch_free(out)
    h.device_batch_free(dev)
    return vec, descs, st


def _consume(h, blob, partition):
    st = N.KtaKafkaIndexStats()
    h._check(N.load().kta_kafka_consume(h._ctx, blob, len(blob), partition, C.byref(st)))
    return st


def _holds(v, P_=P, counters=None):
    bad = [n for n, ok in R.identities(v, P_, counters) if not ok]
    assert not bad, bad
    assert kta.payload_identities(v, P_, counters)


def _one_call(blob, raw, partition=1, failed=()):
    """the blob through one decode call; the vector, checked against the restatement"""
    with kta.HipMetricHandler(P, now=NOW, payload=True) as h:
        got, descs, st = _decode(h, blob, partition)
    want = R.restate([(blob, partition, raw, set(failed))], P)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:20]
    _holds(got)
    return got, descs, st


# ------------------------------------------------------------------------------------------ batch counts, records, offsets
@pytest.mark.parametrize("n", [1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 257])
def test_group_wave_and_workgroup_edges(n):
    blob, raw = B.mixed(n, 5, seed=n)
    with kta.HipMetricHandler(P, now=NOW, payload=True) as h:
        got, _, st = _decode(h, blob, 2)
        info = h.payload_info()
    assert st.n_batches == n and info["launches"] == 1 and info["batches"] == n and info["workgroups"] == (n + 3) // 4
    assert np.array_equal(got, R.restate([(blob, 2, raw, set())], P))
    _holds(got)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_records_per_batch_around_a_round(n):
    blob, raw = B.join([B.batch(0, B.mixed_records(n, seed=n)), B.batch(n, B.mixed_records(n + 1, seed=3))])
    got, _, st = _one_call(blob, raw)
    assert got[R.PW + R.RECORDS] == 2 * n + 1 == st.n_records


def test_byte_off_at_every_residue_mod_16():
    blob, raw = B.mixed(80, 3, seed=5)
    got, descs, st = _one_call(blob, raw)
    assert {descs[i].byte_off % 16 for i in range(st.n_batches)} == set(range(16))


def test_more_batches_than_resident_workgroups_take_turns_and_change_partitions():
    """the grid is twelve workgroups per CU at most: beyond that a workgroup takes every grid-th four batches, keeps its sums
    in registers and sends them to the vector when the partition changes and at its end"""
    kinds = [B.batch(3 * k, B.mixed_records(3, seed=k)) for k in range(5)]
    n = 5 * 4000
    blob = b"".join(b for b, _ in kinds) * (n // 5)
    parts = [(i // 7) % (P + 1) for i in range(n)]                                   # P among them: left out
    with kta.HipMetricHandler(P, now=NOW, payload=True) as h:
        got, _, st = _decode(h, blob, partitions=parts)
        info = h.payload_info()
    assert st.n_batches == n and info["workgroups"] < n // 4 and info["workgroups"] % 12 == 0
    want = np.zeros(R.words(P), np.uint64)
    for k, (b, r) in enumerate(kinds):
        for p in range(P):
            want += np.uint64(sum(1 for i in range(k, n, 5) if parts[i] == p)) * R.restate([(b, p, {0: r}, set())], P)
    assert np.array_equal(got, want) and want[:R.PW * P:R.PW].all()
    _holds(got)


# ------------------------------------------------------------------------------------------ window edges
@pytest.mark.parametrize("value", [B.framed(0x01020304, b"tail"), b'{"json":true}', b"other"], ids=["framed", "json", "other"])
def test_a_value_at_every_offset_around_the_windows_end(value):
    """batch by batch, the second record's value begins at offset 3064 .. 3079 of the batch's first window: its first byte is
    the window's last valid byte (3071), its head lies astride the end, its length varint lies astride the end or behind it"""
    blob, raw, n = B.window_edges(value)
    got, _, _ = _one_call(blob, raw)
    assert got[R.PW + R.RECORDS] == n == 16 * 6 and got[R.PW + R.BAD] == 0


def test_values_larger_than_the_window_long_records_and_a_long_key():
    recs = B.large_records()
    blob, raw = B.join([B.batch(0, recs), B.batch(7, recs[2:3] + recs[:1] + B.mixed_records(20)), B.batch(40, recs, compression="lz4")])
    got, _, _ = _one_call(blob, raw)
    ids = dict((i, (n, b)) for i, n, b in kta.payload_schema_ids(got, P)["ids"])
    assert ids[42] == (3, 3 * 5005) and ids[43] == (2, 2 * 70005) and ids[44] == (2, 20) and got[R.PW + R.CLASS + R.NULL] >= 3


# ------------------------------------------------------------------------------------------ headers
def test_header_counts_null_values_empty_and_long_keys():
    recs = [B.record(i, b"v", headers=[(b"h%d" % k, b"x" * (k % 4)) for k in range(n)]) for i, n in enumerate((0, 1, 14, 15, 16, 200))]
    recs += [B.record(6, b"v", headers=[(b"nul", None)]), B.record(7, b"v", headers=[(b"", b"empty-key")]),
             B.record(8, b"v", headers=[(b"K" * 300, b"V" * 300), (b"", None)])]
    blob, raw = B.join([B.batch(0, recs), B.batch(9, recs[::-1], compression="snappy")])
    got, _, _ = _one_call(blob, raw)
    hist = got[R.PW * P:R.PW * P + R.HIST]
    assert hist.tolist() == [2, 6, 2] + [0] * 11 + [2, 6] and got[R.PW + R.HEADERS] == 2 * (1 + 14 + 15 + 16 + 200 + 1 + 1 + 2)
    assert got[R.PW + R.HNULL] == 4 and got[R.PW + R.WITH] == 16


@pytest.mark.parametrize("kind", sorted(B.BAD_HEADERS))
def test_every_bad_header_kind_first_in_the_middle_and_last(kind):
    good = [B.record(i, B.framed(9), headers=[(b"a", b"bc"), (b"", None)]) for i in range(19)]      # more than a round
    out = []
    for place in (0, 9, 18):
        recs = list(good)
        recs[place] = B.record(place, b'{"v":1}', raw_headers=B.BAD_HEADERS[kind])
        out.append(B.batch(19 * len(out), recs))
    blob, raw = B.join(out)
    got, _, _ = _one_call(blob, raw)
    w = got[R.PW:2 * R.PW]
    assert (w[R.RECORDS], w[R.BAD], w[R.CLASS + R.JSON], w[R.CLASS + R.FRAMED]) == (57, 3, 3, 54)
    assert (w[R.WITH], w[R.HEADERS], w[R.HKEY], w[R.HVAL], w[R.HNULL], w[R.WIRE]) == (54, 108, 54, 108, 54, 54 * 8)   # the neighbours alone


# ------------------------------------------------------------------------------------------ value classes, ids
def test_every_class_at_lengths_0_1_4_5_and_the_edge_ids():
    values = [None, b"", b"\x00", b"{", b"[", b"x", b"\x00abc", b"{abc", b"[abc", b"xabc", b"\x00abcd", b"{abcd", b"[abcd", b"xabcd", b"\x01\x00\x00\x00\x01"]
    values += [B.framed(i, b"") for i in (0, 1, 0x7FFFFFFF, 0xFFFFFFFF)] + [B.framed(0xFFFFFFFF, b"more")]
    blob, raw = B.join([B.batch(0, [B.record(i, v) for i, v in enumerate(values)])])
    got, _, _ = _one_call(blob, raw)
    w = got[R.PW:2 * R.PW]
    assert w[R.CLASS:R.CLASS + 5].tolist() == [1, 1, 6, 6, 6] and w[R.CLASS + R.OTHER] == 6          # 0x00 with four bytes is `other`
    read = kta.payload_schema_ids(got, P)
    assert sorted(read["ids"]) == sorted([(0, 1, 5), (1, 1, 5), (0x7FFFFFFF, 1, 5), (0xFFFFFFFF, 2, 14), (0x61626364, 1, 5)])
    assert read["unresolved_records"] == 0


def test_sixty_four_distinct_ids_in_one_wave_one_id_throughout_and_a_double_collision():
    wave = [B.batch(16 * g, [B.record(i, B.framed(90000 + 16 * g + i, b"b" * i)) for i in range(16)]) for g in range(4)]
    blob, raw = B.join(wave)
    got, _, st = _one_call(blob, raw)
    assert st.n_batches == 4 and len(kta.payload_schema_ids(got, P)["ids"]) == 64
    blob, raw = B.join([B.batch(0, [B.record(i, B.framed(31, b"same")) for i in range(200)])] * 5)
    got, _, _ = _one_call(blob, raw)
    assert kta.payload_schema_ids(got, P)["ids"] == [(31, 1000, 9000)]
    a, b = double_collision()
    blob, raw = B.join([B.batch(0, [B.record(i, B.framed((a, b, 99)[i % 3], b"z" * (i % 3))) for i in range(30)])])
    got, _, _ = _one_call(blob, raw)
    read = kta.payload_schema_ids(got, P)
    assert read["ids"] == [(99, 10, 70)] and read["unresolved_records"] == 20 and read["unresolved_bytes"] == 10 * 5 + 10 * 6
    assert (read["ids"], read["unresolved_records"], read["unresolved_bytes"]) == R.schema_ids(got, P)


# ------------------------------------------------------------------------------------------ codecs, flags, filter
def test_all_codecs_in_one_blob():
    blob, raw = B.mixed(3 * len(CODECS), 30, seed=2, compression=CODECS)
    got, _, _ = _one_call(blob, raw, partition=0)
    assert {b["codec"] for b in R.batches_of(blob)} == set(range(len(CODECS)))


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
    want = R.restate(sets, P, None if flt is None else (flt[0], flt[1], None if flt[2] is None else set(flt[2])))
    with kta.HipMetricHandler(P, now=NOW, payload=True) as h:
        if flt is not None:
            h.set_filter(*flt)
        for blob, p, _, _ in sets:
            _consume(h, blob, p)
        got = h.get_payload()["vector"]
    assert np.array_equal(got, want)
    _holds(got)
    whole = R.restate(sets, P)
    assert (flt is None) == bool(np.array_equal(want, whole)) and 0 < want[:R.PW * P:R.PW].sum() <= whole[:R.PW * P:R.PW].sum()


# ------------------------------------------------------------------------------------------ partitions, failures
def test_interleaved_partitions_and_partitions_outside_the_range():
    batches = [B.batch(5 * i, B.mixed_records(5, seed=i)) for i in range(90)]
    blob, _ = B.join(batches)
    parts = [(i * 7 + i // 5) % (P + 2) - 1 for i in range(90)]                       # -1 and P among them: left out entirely
    with kta.HipMetricHandler(P, now=NOW, payload=True) as h:
        got, _, _ = _decode(h, blob, partitions=parts)                                # one call, a wave holds four partitions
    want = R.restate([(b, p, {0: r}, set()) for (b, r), p in zip(batches, parts)], P)
    assert np.array_equal(got, want) and want[:R.PW * P:R.PW].all() and want[:R.PW * P:R.PW].sum() < 450
    _holds(got)


def test_forged_counts_and_corrupt_streams_add_nothing():
    out, failed = [B.batch(0, B.mixed_records(9))], set()
    forged = RB.patch(B.batch(9, B.mixed_records(3, seed=1))[0], count=1000)                     # forged count
    out.append((forged, b""))
    for comp in [c for c in CODECS if c]:                                                      # a stream that does not inflate
        b, raw = B.batch(20, B.mixed_records(30, seed=2), compression=comp)
        out.append((RB.corrupt_stream(b, comp), raw))
    out.append(B.batch(90, B.mixed_records(5, seed=3), compression="snappy"))
    blob, raw = B.join(out)
    failed = set(sorted(raw)[1:-1])
    got, _, _ = _one_call(blob, raw, failed=failed)
    assert got[R.PW + R.RECORDS] == 14


def test_a_bad_crc_under_check_crcs_adds_nothing():
    good, (b, raw) = B.batch(0, B.mixed_records(3)), B.batch(3, B.mixed_records(4, seed=8))
    bad = b[:70] + bytes([b[70] ^ 1]) + b[71:]                                      # one bit inside the CRC's range (a timestamp delta)
    blob = good[0] + bad + good[0]
    raws = {0: good[1], len(good[0]): raw, len(good[0]) + len(bad): good[1]}
    with kta.HipMetricHandler(P, now=NOW, payload=True) as h:
        h._check(N.load().kta_kafka_set_check_crcs(h._ctx, 1))
        got, _, _ = _decode(h, blob, 0)
    assert np.array_equal(got, R.restate([(blob, 0, raws, {len(good[0])})], P)) and got[R.RECORDS] == 6
    with kta.HipMetricHandler(P, now=NOW, payload=True) as h:                       # check.crcs off: the batch is delivered
        got, _, _ = _decode(h, blob, 0)
    assert np.array_equal(got, R.restate([(blob, 0, raws, set())], P)) and got[R.RECORDS] == 10


# ------------------------------------------------------------------------------------------ submission paths
def test_consume_in_chunks_accumulates_resets_and_snapshots():
    blob, raw = B.mixed(300, 6, seed=21)
    other, other_raw = B.mixed(40, 4, seed=22)
    want = R.restate([(blob, 2, raw, set())], P)
    with kta.HipMetricHandler(P, now=NOW, payload=True) as h:
        h._check(N.load().kta_kafka_configure(h._ctx, 8192, 3))                     # a few dozen batches per staging blob
        st = _consume(h, blob, 2)
        assert st.n_batches == 300 and h.payload_info()["launches"] > 5
        got = h.get_payload()["vector"]
        assert np.array_equal(got, want)
        h.finish()
        _holds(got, counters=h.result_vector_host())                                # records == total_messages, null == tombstones
        assert np.array_equal(h.exchange_payload()["vector"], want) and np.array_equal(h.get_payload()["vector"], want)
        _consume(h, other, 0)                                                       # a second call accumulates
        both = R.restate([(blob, 2, raw, set()), (other, 0, other_raw, set())], P)
        assert np.array_equal(h.get_payload()["vector"], both)
        assert np.array_equal(h.exchange_payload()["vector"], want)                 # the snapshot is finish()'s
        h.reset()
        assert not h.get_payload()["vector"].any()
        _consume(h, other, 0)
        assert np.array_equal(h.get_payload()["vector"], R.restate([(other, 0, other_raw, set())], P))


def test_a_compaction_replay_counts_no_record_twice():
    blob, raw = B.mixed(100, 5, seed=41)
    want = R.restate([(blob, 1, raw, set())], P)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True, payload=True) as h:
        _consume(h, blob, 1)
        h.finish()
        launches = h.payload_info()["launches"]
        with h.compaction_replay():
            _consume(h, blob, 1)
        assert h.compaction()["replayed"] == int(want[R.PW + R.RECORDS])
        assert h.payload_info()["launches"] == launches
        assert np.array_equal(h.get_payload()["vector"], want)


EVERYTHING = dict(count_alive_keys=True, analytics=True, key_sketch=True, hot_keys=True, ts_order=True, partitioner=True, compaction=True,
                  size_quantiles=True, timeline=(T0, 1000, 8), segments=(4096, 4, 70), compact_delete=True, record_batches=True)
OTHER_SECTIONS = ("analytics", "timeline", "key_sketch", "hot_keys", "ts_order", "partitioner", "size_quantiles", "segments", "get_record_batches")


def _flat(x):
    if isinstance(x, dict) and "vector" in x:
        return np.asarray(x["vector"]).reshape(-1)
    if isinstance(x, dict):
        return np.concatenate([np.asarray(x[k]).reshape(-1).view(np.uint64) for k in sorted(x)])
    return np.asarray(x).reshape(-1)


def test_every_pass_on_at_once_and_no_side_effects_on_the_others():
    sets = [B.mixed(60, 4, seed=50 + p) + (p,) for p in range(P)]
    want = R.restate([(blob, p, raw, set()) for blob, raw, p in sets], P)
    state = {}
    for on in (False, True):
        with kta.HipMetricHandler(P, now=NOW, payload=on, **EVERYTHING) as h:
            for blob, _, p in sets:
                _consume(h, blob, p)
            res, counters = h.finish()
            state[on] = {s: _flat(getattr(h, s)()).copy() for s in OTHER_SECTIONS}
            state[on]["counters"] = h.result_vector_host()
            state[on]["alive"] = res.alive_keys
            if on:
                got = h.get_payload()["vector"]
                assert np.array_equal(got, want)
                _holds(got, counters=state[on]["counters"])
            else:
                for call in (h.get_payload, h.exchange_payload, h.payload_info, h.payload_vector, h.payload_result_vector):
                    with pytest.raises(kta.KtaError, match="KTA_FLAG_PAYLOAD"):
                        call()
    for name in state[True]:
        assert np.array_equal(state[True][name], state[False][name]), name


# ------------------------------------------------------------------------------------------ the CLI
def _cli(*args):
    return subprocess.run(["timeout", "-k", "10", "240", CLI, *args], capture_output=True, text=True, timeout=270)


def _normalise(text):
    text = re.sub(r"Scanning took: \d+ seconds", "Scanning took: 3 seconds", text)
    return re.sub(r"Estimated Msg/s: \d+", "Estimated Msg/s: 133", text)


def test_cli_prints_the_section_behind_the_unchanged_report(tmp_path):
    sets, files = [], []
    for p in range(2):
        blob, raw = B.mixed(40 + 10 * p, 6, seed=60 + p, compression=[None, "snappy", "lz4", "gzip"])
        path = tmp_path / ("%d.log" % p)
        path.write_bytes(blob)
        files.append(str(path))
        sets.append((blob, p, raw, set()))
    src = "segment://" + ",".join(files)
    sizes = np.zeros(7 * 2 + 8, np.uint64)
    want = kta.render_payload(R.restate(sets, 2, sizes=sizes), 2, sizes)
    plain = _cli("-t", "seg", "-b", src)
    one = _cli("-t", "seg", "-b", src, "--librdkafka", "kta.payload=1")
    assert plain.returncode == 0 and one.returncode == 0, one.stderr
    assert "Payload:" not in plain.stdout
    at = one.stdout.index("Payload: value formats")
    assert one.stdout[at:] == want and _normalise(one.stdout[:at]) == _normalise(plain.stdout)
    assert "Schema id" in want and "n/a" not in want
    # with -c and the compaction what-if (the source is read twice, the records counted once), beside other sections, filtered
    many = _cli("-t", "seg", "-b", src, "-c", "--librdkafka", "kta.payload=1,kta.record_batches=1,kta.compaction=1,kta.percentiles=1,kta.partitions=1")
    assert many.returncode == 0, many.stderr
    sizes1 = np.zeros(7 * 2 + 8, np.uint64)
    want1 = kta.render_payload(R.restate(sets, 2, (None, None, {1}), sizes=sizes1), 2, sizes1)
    assert many.stdout.endswith(want1) and "Compaction what-if" in many.stdout and "Record batches:" in many.stdout

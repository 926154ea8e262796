"""GPU tests of the record-batch section (KTA_FLAG_RECORD_BATCHES; no reference counterpart): the live vector that
kta_record_batches accumulates from the descriptors and headers of every decode call is np.array_equal to the restatement
(tests/record_batches_py.py, which parses the blob itself and takes every inflated size from the encoder's own record bytes)

    batch counts      1; 63 / 64 / 65 (wave edge); 255 / 256 / 257 (workgroup edge); 3 000 batches of odd sizes, byte_off at
                      every residue mod 16
    partition mix     one partition per call (the wave-uniform path) and partitions interleaved batch by batch inside one
                      kta_kafka_decode_device call (the per-lane path)
    field edges       n_records 1, 2^k - 1, 2^k; spans 0, 1, >= 2^31, max_ts < base_ts; producer ids -1, 0, 2^63 - 1;
                      lastOffsetDelta + 1 above and below the count; leader epochs -1 and 5
    codecs, flags     all five codecs in one blob; LogAppendTime and transactional bits
    failed batches    a forged count, a corrupted compressed stream, a bad CRC under check.crcs: `failed` only
    submission        kta_kafka_consume in chunks = one decode call; two calls accumulate; kta_reset; get after finish
    composition       a filter (set, window, both); -c with a compaction replay; every opt-in pass on at once
    no side effects   every other section and the counters identical with the flag on and off
    kta-analyzer      kta.record_batches=1 on a two-partition segment:// fixture, behind the unchanged report"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import record_batches_blobs as B
import record_batches_py as R
from helpers import NOW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
P = 4
T0 = 1_600_000_000_000


def _index(blob, partition):
    lib, st = N.load(), N.KtaKafkaIndexStats()
    cap = max(len(R.parse(blob)), 1)
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
    vec = h.get_record_batches()["vector"].copy()                  # (waits for the compute stream before the buffers go)
    h.device_batch_free(out)
    h.device_batch_free(dev)
    return vec, descs, st


def _consume(h, blob, partition):
    st = N.KtaKafkaIndexStats()
    h._check(N.load().kta_kafka_consume(h._ctx, blob, len(blob), partition, C.byref(st)))
    return st


def _all_hold(v, P_=P, records=None):
    bad = [n for n, ok in R.identities(v, P_, records) if not ok]
    assert not bad, bad
    assert kta.record_batches_identities(v, P_)


# ------------------------------------------------------------------------------------------ batch counts
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_wave_and_workgroup_edges(n):
    blob, raw = B.mixed(n, n)
    with kta.HipMetricHandler(P, now=NOW, record_batches=True) as h:
        got, _, st = _decode(h, blob, 2)
        info = h.record_batches_info()
    assert st.n_batches == n and info["launches"] == 1 and info["batches"] == n and info["workgroups"] == (n + 255) // 256
    assert np.array_equal(got, R.restate([(blob, 2, raw, set())], P))
    _all_hold(got)


def test_three_thousand_batches_at_every_alignment():
    blob, raw = B.mixed(11, 3000)
    with kta.HipMetricHandler(P, now=NOW, record_batches=True) as h:
        got, descs, st = _decode(h, blob, 1)
    assert st.n_batches == 3000 and {descs[i].byte_off % 16 for i in range(3000)} == set(range(16))
    assert np.array_equal(got, R.restate([(blob, 1, raw, set())], P))
    _all_hold(got)


# ------------------------------------------------------------------------------------------ partition mix
def test_uniform_and_interleaved_partitions_give_the_restatements_vector():
    blob, raw = B.mixed(5, 700)
    n = len(R.parse(blob))
    parts = [(i * 7 + i // 5) % (P + 2) - 1 for i in range(n)]          # -1 and P among them: left out entirely
    with kta.HipMetricHandler(P, now=NOW, record_batches=True) as h:
        mixed, _, _ = _decode(h, blob, partitions=parts)                 # one call, a wave holds every partition
    want = R.restate_parts(blob, parts, P, raw)
    assert np.array_equal(mixed, want)
    _all_hold(mixed)
    assert want[[16 * p for p in range(P)]].all() and want[:16 * P:16].sum() < n
    # the same batches, one partition per call: the wave-uniform path ends with the same vector
    cut = [b["pos"] for b in R.parse(blob)] + [len(blob)]
    with kta.HipMetricHandler(P, now=NOW, record_batches=True) as h:
        for p in range(P):
            own = [i for i in range(n) if parts[i] == p]
            sub = b"".join(blob[cut[i]:cut[i + 1]] for i in own)
            got, _, _ = _decode(h, sub, p)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------ field edges
def _edge_batches():
    out, off = [], 0
    for n in (1, 2, 3, 4, 7, 8, 255, 256, 1023, 1024):                  # 2^k - 1 and 2^k: both sides of a histogram bin
        out.append(B.batch(off, n, T0, value_len=3, key=False))
        off += n
    for base, mx in ((T0, T0), (T0, T0 + 1), (T0, T0 + 2 ** 31 - 1), (T0, T0 + 2 ** 31), (T0, T0 + 2 ** 40), (T0 + 500, T0), (0, 2 ** 62),
                     (-1, -1)):
        out.append(B.batch(off, 2, base, max_ts=mx, ts_step=0))
        off += 2
    for pid in (-1, 0, 2 ** 63 - 1, 1, -2 ** 63):
        out.append(B.batch(off, 1, T0, producer_id=pid))
        off += 1
    for n, lod in ((5, 4), (5, 40), (5, 2), (1, 2 ** 31 - 1), (3, -1)):  # a compacted batch, a lying one, the extremes
        out.append(B.batch(off, n, T0, last_offset_delta=lod))
        off += 50
    for epoch in (-1, 5, 0, 2 ** 31 - 1):
        out.append(B.batch(off, 1, T0, epoch=epoch))
        off += 1
    for attrs in (0x08, 0x10, 0x18, 0x40):
        out.append(B.batch(off, 2, T0, attributes=attrs))
        off += 2
    return B.join(out)


def test_field_edges():
    blob, raw = _edge_batches()
    with kta.HipMetricHandler(P, now=NOW, record_batches=True) as h:
        got, _, st = _decode(h, blob, 3)
    want = R.restate([(blob, 3, raw, set())], P)
    assert np.array_equal(got, want)
    _all_hold(got)
    d = kta.split_record_batches(got, P)
    assert d["maxima"][3].tolist() == [1024, int(d["maxima"][3][1]), 2 ** 31, 2 ** 31 - 1] and d["partitions"][3][R.FAILED] == 0
    hist = d["hist_records"][0]
    assert hist[8] == 1 and hist[9] == 1 and hist[10] == 1 and hist[11] == 1       # 255 | 256 | 1023 | 1024: both sides of a bin
    assert d["hist_span"][0][31] == 4 and d["hist_span"][0][0] >= 2               # clamped spans; span 0 and max_ts < base_ts


def test_all_five_codecs_in_one_blob_and_the_flag_bits():
    pytest.importorskip("pyarrow")
    if not B.have_zstd():
        pytest.skip("pyarrow without zstd")
    out, off = [], 0
    for i, comp in enumerate(B.CODECS * 3):
        out.append(B.batch(off, 6 + i, T0 + i, value_len=40 + 3 * i, compression=comp, attributes=(0x08, 0x10, 0x18)[i % 3], producer_id=i % 4))
        off += 6 + i
    blob, raw = B.join(out)
    with kta.HipMetricHandler(P, now=NOW, record_batches=True) as h:
        got, _, _ = _decode(h, blob, 0)
    assert np.array_equal(got, R.restate([(blob, 0, raw, set())], P))
    _all_hold(got)
    d = kta.split_record_batches(got, P)
    assert d["codecs"][:, 0].tolist() == [3] * 5 and d["partitions"][0][R.LOG_APPEND] == 10 and d["partitions"][0][R.TRANSACTIONAL] == 10
    assert (d["codecs"][1:, 3] > d["codecs"][1:, 2]).all() and round(d["producers"]) == 4   # every codec compressed; 4 producers


# ------------------------------------------------------------------------------------------ failed batches
def _codecs_here():
    return [c for c in B.CODECS if c is not None and (c != "zstd" or B.have_zstd())]


def test_forged_count_and_corrupt_streams_add_to_failed_only():
    out, failed = [B.batch(0, 4, T0, producer_id=3)], set()
    failed.add(len(out))
    out.append((B.patch(B.batch(4, 2, T0, producer_id=77, epoch=9)[0], count=1000), 0))          # forged count
    for comp in _codecs_here():                                                                # a stream that does not inflate
        b, raw = B.batch(10, 30, T0, value_len=50, compression=comp, producer_id=78, epoch=9)
        failed.add(len(out))
        out.append((B.corrupt_stream(b, comp), raw))
    out.append(B.batch(90, 5, T0 + 9, compression="snappy"))
    blob, raw = B.join(out)
    with kta.HipMetricHandler(P, now=NOW, record_batches=True) as h:
        got, descs, st = _decode(h, blob, 1)
    want = R.restate([(blob, 1, raw, failed)], P)
    assert np.array_equal(got, want)
    _all_hold(got)
    d = kta.split_record_batches(got, P)
    assert d["partitions"][1][R.FAILED] == len(failed) and d["partitions"][1][R.BATCHES] == 2
    assert d["maxima"][1][2] == 1 and round(d["producers"]) == 1                    # epoch 9 and producers 77, 78 left no trace


def test_bad_crc_with_check_crcs_on_adds_to_failed_only():
    good, (b, raw) = B.batch(0, 3, T0), B.batch(3, 3, T0 + 5, producer_id=5)
    bad = b[:70] + bytes([b[70] ^ 1]) + b[71:]                                      # one bit inside the CRC's range
    blob, raws = good[0] + bad + good[0], [good[1], raw, good[1]]
    with kta.HipMetricHandler(P, now=NOW, record_batches=True) as h:
        h._check(N.load().kta_kafka_set_check_crcs(h._ctx, 1))
        got, _, _ = _decode(h, blob, 0)
    assert np.array_equal(got, R.restate([(blob, 0, raws, {1})], P))
    assert got[R.FAILED] == 1 and got[R.BATCHES] == 2 and got[R.IDEMPOTENT] == 0
    with kta.HipMetricHandler(P, now=NOW, record_batches=True) as h:               # check.crcs off: the batch is delivered
        got, _, _ = _decode(h, blob, 0)
    assert got[R.FAILED] == 0 and got[R.BATCHES] == 3 and got[R.IDEMPOTENT] == 1


# ------------------------------------------------------------------------------------------ submission paths
def test_consume_in_chunks_accumulates_resets_and_snapshots():
    blob, raw = B.mixed(21, 900)
    other, other_raw = B.mixed(22, 130)
    want = R.restate([(blob, 2, raw, set())], P)
    with kta.HipMetricHandler(P, now=NOW, record_batches=True) as h:
        one, _, _ = _decode(h, blob, 2)
    assert np.array_equal(one, want)
    with kta.HipMetricHandler(P, now=NOW, record_batches=True) as h:
        h._check(N.load().kta_kafka_configure(h._ctx, 8192, 3))                     # ~60 batches per staging blob
        st = _consume(h, blob, 2)
        assert st.n_batches == 900 and h.record_batches_info()["launches"] > 10
        got = h.get_record_batches()["vector"]
        assert np.array_equal(got, want)
        res, counters = h.finish()
        _all_hold(got, records=int(counters[:, N.KTA_C_TOTAL].sum()))               # every record delivered, tombstones included
        assert np.array_equal(h.exchange_record_batches()["vector"], want) and np.array_equal(h.get_record_batches()["vector"], want)
        _consume(h, other, 0)                                                       # a second call accumulates
        both = R.restate([(blob, 2, raw, set()), (other, 0, other_raw, set())], P)
        assert np.array_equal(h.get_record_batches()["vector"], both)
        assert np.array_equal(h.exchange_record_batches()["vector"], want)          # the snapshot is finish()'s
        h.reset()
        assert not h.get_record_batches()["vector"].any()
        _consume(h, other, 0)
        assert np.array_equal(h.get_record_batches()["vector"], R.restate([(other, 0, other_raw, set())], P))


# ------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize("flt", [(None, None, (0, 2)), (T0 + 1000, T0 + 3000, None), (T0 + 1000, None, (1, 2, 3)), (None, T0 + 1000, (3,))])
def test_with_a_filter_the_batches_that_overlap_the_window_are_counted(flt):
    sets = []
    for p in range(P):
        blob, raw = B.mixed(30 + p, 500)                                            # base_ts = T0 + 10 i, spans of a few ms
        sets.append((blob, p, raw, set()))
    lo, hi, parts = flt
    want = R.restate(sets, P, (lo, hi, None if parts is None else set(parts)))
    with kta.HipMetricHandler(P, now=NOW, record_batches=True) as h:
        h.set_filter(lo, hi, parts)
        for blob, p, _, _ in sets:
            _consume(h, blob, p)
        got = h.get_record_batches()["vector"]
    assert np.array_equal(got, want)
    _all_hold(got)
    whole = R.restate(sets, P)
    assert 0 < want[:16 * P:16].sum() < whole[:16 * P:16].sum()


def test_a_compaction_replay_counts_no_batch_twice():
    blob, raw = B.mixed(41, 300)
    want = R.restate([(blob, 1, raw, set())], P)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True, record_batches=True) as h:
        _consume(h, blob, 1)
        h.finish()
        launches = h.record_batches_info()["launches"]
        with h.compaction_replay():
            _consume(h, blob, 1)
        assert h.compaction()["replayed"] == int(want[16 + R.RECORDS])
        assert h.record_batches_info()["launches"] == launches
        assert np.array_equal(h.get_record_batches()["vector"], want)


EVERYTHING = dict(count_alive_keys=True, analytics=True, key_sketch=True, hot_keys=True, ts_order=True, partitioner=True, compaction=True,
                  size_quantiles=True, timeline=(T0, 1000, 8), segments=(4096, 4, 70), compact_delete=True)
OTHER_SECTIONS = ("analytics", "timeline", "key_sketch", "hot_keys", "ts_order", "partitioner", "size_quantiles", "segments")


def _flat(x):
    if isinstance(x, dict) and "vector" in x:
        return np.asarray(x["vector"]).reshape(-1)
    if isinstance(x, dict):
        return np.concatenate([np.asarray(x[k]).reshape(-1).view(np.uint64) for k in sorted(x)])
    return np.asarray(x).reshape(-1)


def test_every_pass_on_at_once_and_no_side_effects_on_the_others():
    sets = [B.mixed(50 + p, 200) + (p,) for p in range(P)]
    want = R.restate([(blob, p, raw, set()) for blob, raw, p in sets], P)
    state = {}
    for on in (False, True):
        with kta.HipMetricHandler(P, now=NOW, record_batches=on, **EVERYTHING) as h:
            for blob, _, p in sets:
                _consume(h, blob, p)
            res, counters = h.finish()
            state[on] = {s: _flat(getattr(h, s)()).copy() for s in OTHER_SECTIONS}
            state[on]["counters"] = h.result_vector_host()
            state[on]["alive"] = res.alive_keys
            if on:
                got = h.get_record_batches()["vector"]
                assert np.array_equal(got, want)
                _all_hold(got, records=int(counters[:, N.KTA_C_TOTAL].sum()))
            else:
                with pytest.raises(kta.KtaError, match="KTA_FLAG_RECORD_BATCHES"):
                    h.get_record_batches()
                with pytest.raises(kta.KtaError, match="KTA_FLAG_RECORD_BATCHES"):
                    h.record_batches_info()
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
        blob, raw = B.mixed(60 + p, 150 + 40 * p, codecs=[None, "snappy", "lz4", "gzip"])
        control = B.batch(10 ** 6, 1, T0, attributes=0x20)[0]
        blob, raw = blob + control, raw + [0]
        path = tmp_path / ("%d.log" % p)
        path.write_bytes(blob)
        files.append(str(path))
        sets.append((blob, p, raw, set()))
    src = "segment://" + ",".join(files)
    want = kta.render_record_batches(R.restate(sets, 2), 2, skipped=[2, 0, 0])
    plain = _cli("-t", "seg", "-b", src)
    one = _cli("-t", "seg", "-b", src, "--librdkafka", "kta.record_batches=1")
    assert plain.returncode == 0 and one.returncode == 0, one.stderr
    assert "Record batches" not in plain.stdout
    at = one.stdout.index("Record batches: what the batch headers")
    assert one.stdout[at:] == want and _normalise(one.stdout[:at]) == _normalise(plain.stdout)
    assert "control batches (2)" in want
    # with -c and the compaction what-if (the source is read twice, the batches counted once), beside other sections, filtered
    many = _cli("-t", "seg", "-b", src, "-c", "--librdkafka", "kta.record_batches=1,kta.compaction=1,kta.percentiles=1,kta.partitions=1")
    assert many.returncode == 0, many.stderr
    want1 = kta.render_record_batches(R.restate(sets, 2, (None, None, {1})), 2, filtered=True, skipped=[2, 0, 0])
    assert many.stdout.endswith(want1) and "Compaction what-if" in many.stdout and "Record filter" in many.stdout

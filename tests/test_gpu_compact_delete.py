"""GPU tests of the compact,delete what-if (kta_set_compact_delete): the kept vector the compaction replay writes, bit for
bit against the sequential restatement (tests/compact_delete_py.py), with the identities between the first pass's segment
vector, the replay's kept vector and the replay's compaction vector asserted in every test — on every submission path,
tile form and layout, across batches and resets, at the chunk and wave-count switches, with the switch off, and through
the CLI.  Every input is first shown, on the CPU, to exercise the feature."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import compact_delete_py as CD
import compaction_py as CP
import filter_py as F
import kafka_format as KF
import segments_py as SP
from helpers import NOW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
BASE = 1_600_000_000_000
METRIC = ("partition", "key_len", "val_len", "ts_ms")


def _topic(seed, n, P, outside=0.02, max_val=60):
    """keys of 1 to 24 bytes from a pool of about n / 8, 10 % tombstones, 5 % null keys, a few records outside [0, P)"""
    rng = np.random.default_rng(seed)
    pool = max(n // 8, 1)
    pool_len = rng.integers(1, 25, pool)
    pool_bytes = rng.integers(0, 256, (pool, 24), dtype=np.uint8)
    kid = rng.integers(0, pool, n)
    key_len = pool_len[kid].astype(np.int32)
    key_len[rng.random(n) < 0.05] = -1
    kl = np.maximum(key_len, 0).astype(np.int64)
    off = np.zeros(n, np.int64)
    off[1:] = np.cumsum(kl)[:-1]
    blob = np.zeros(int(kl.sum()) + 16, np.uint8)                                   # (readable 16 bytes past the last key)
    for i in np.flatnonzero(kl):
        blob[off[i]:off[i] + kl[i]] = pool_bytes[kid[i], :kl[i]]
    part = rng.integers(0, P, n).astype(np.int32)
    m = rng.random(n) < outside
    part[m] = np.where(rng.random(int(m.sum())) < 0.5, -1, P)
    val_len = rng.integers(0, max_val, n).astype(np.int32)
    val_len[rng.random(n) < 0.10] = -1
    ts = BASE + np.arange(n, dtype=np.int64) * 10 + rng.integers(-500, 501, n)
    ts[rng.random(n) < 0.02] = -1
    return {"partition": part, "key_len": key_len, "val_len": val_len, "ts_ms": ts, "key_off": off.astype(np.uint32), "key_bytes": blob}


def _cut(cols, lo, hi):
    return {k: (v if k == "key_bytes" else v[lo:hi]) for k, v in cols.items()}


def _want(cols, P, cfg, seq=None):
    """(segment vector, kept vector, compaction vector) of a first pass and a replay over the same records"""
    seg = SP.segments_vector(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"], P, *cfg)
    cls = CD.classes(cols, seq)
    return seg, CD.kept_vector(cols, P, *cfg, cls=cls), CP.vector(cols, P, seq), cls


def _exercises(want, P, M, closes=True):
    """the restatement alone: a survivor in a closed row, a superseded record, a closed row"""
    seg, kept, comp, cls = want
    k = CD.split(kept, P, M)
    superseded = int(CP.split(comp, P)["replayed"]) - int(CP.split(comp, P)["unkeyed"]) - sum(1 for c in cls if c > 0)
    assert superseded > 0 and not any(c < 0 for c in cls)
    if closes:
        assert int(k["globals"][2]) > 0 and int((k["rows"][:, :, 0] + k["rows"][:, :, 2]).max()) > 0
    assert CD.identities_hold(seg, kept, comp, P, M)


def _handler(P, cfg, **kw):
    return kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True, segments=cfg, compact_delete=True, **kw)


def _round(h, feed, want, P, M):
    """feed(replay) hands the records over: a first pass, a replay; all three vectors are `want`, and the identities hold"""
    feed(False)
    h.finish(allow_bad_partition=True)
    with h.compaction_replay():
        feed(True)
    return _hold(h, want, P, M)


def _hold(h, want, P, M):
    seg, kept, comp = h.segments()["vector"], h.compact_delete()["vector"], h.compaction()["vector"]
    assert np.array_equal(seg, want[0])
    assert np.array_equal(comp, want[2])
    assert np.array_equal(kept, want[1]), np.flatnonzero(kept != want[1])[:8]
    assert CD.identities_hold(seg, kept, comp, P, M)
    now = int(BASE + 10**6)
    got = kta.compact_delete_whatif(seg, kept, comp, P, M, now, 10**5, 1000)         # (the library's own check of the identities)
    assert np.array_equal(got, np.array(CD.whatif_formula(seg, kept, P, M, now, 10**5, 1000), np.uint64))
    return kept


def _submit(h, cols, base_seq=None):
    h.submit_columns(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"], cols["key_off"], cols["key_bytes"], base_seq=base_seq)


def _device_feed(h, cols, base_seq=0):
    b, nb = h.upload_batch(cols, with_keys=True)
    return b, (lambda replay: h.submit_device(b, nb, base_seq))


def _free(h, *batches):
    h.sync()
    for b in batches:
        h.device_batch_free(b)


# ------------------------------------------------------------------------------------------ small shapes
@pytest.mark.parametrize("n", [64, 65])
@pytest.mark.parametrize("P", [1, 3, 64])
def test_small_shapes_host_and_device_batches(P, n):
    cfg, M = (7, 1024, 2), 1024                                                    # (rows enough for every record to close one)
    cols = _topic(1000 * P + n, n, P, outside=0.05 if P > 1 else 0.0)
    want = _want(cols, P, cfg)
    _exercises(want, P, M)
    with _handler(P, cfg) as h:
        h.set_segments_chunk(64)
        _round(h, lambda replay: _submit(h, cols, base_seq=0), want, P, M)
        h.reset()
        b, feed = _device_feed(h, cols)
        _round(h, feed, want, P, M)
        assert h.compact_delete_info()["chunks"] == -(-n // 64)
        _free(h, b)


# ------------------------------------------------------------------------------------------ S extremes
@functools.lru_cache(maxsize=None)
def _medium():
    P, n = 5, 6000
    return P, n, _topic(7, n, P)


def test_s_of_one_byte_every_record_closes_a_row():
    P, n, cols = _medium()
    n = 2000
    cols = _cut(cols, 0, n)
    M = 1 << 15                                                                     # (more rows than a partition has bytes)
    cfg = (1, M, 1)
    want = _want(cols, P, cfg)
    _exercises(want, P, M)
    k = CD.split(want[1], P, M)
    assert int(k["globals"][2]) == int(k["globals"][0]) > n // 2 and int(k["totals"][:, 1].max()) < M - 1
    with _handler(P, cfg) as h:
        b, feed = _device_feed(h, cols)
        _round(h, feed, want, P, M)
        info = h.compact_delete_info()
        assert info["chunks_applied"] == info["chunks"] > 0
        _free(h, b)


def test_s_of_2_to_the_40_no_record_closes_a_row():
    P, n, cols = _medium()
    M = 8
    cfg = (1 << 40, M, 0)
    want = _want(cols, P, cfg)
    _exercises(want, P, M, closes=False)
    _exercises(_want(cols, P, (700, 64, 0)), P, 64)                                 # (the same records do close rows at a smaller S)
    assert not CD.split(want[1], P, M)["rows"].any() and CD.split(want[1], P, M)["totals"][:, 3].all()
    with _handler(P, cfg) as h:
        b, feed = _device_feed(h, cols)
        _round(h, feed, want, P, M)
        info = h.compact_delete_info()
        assert info["chunks_applied"] == 0 and info["chunks"] > 0 and info["launches"] == 3
        _free(h, b)


# ------------------------------------------------------------------------------------------ carry, reset
def test_carry_across_three_batches_and_a_second_replay_after_reset():
    P, n, cols = _medium()
    M = 64
    cfg = (900, M, 3)
    want = _want(cols, P, cfg)
    _exercises(want, P, M)
    with _handler(P, cfg) as h:
        for cuts in ((64, 65), (1023, 4097)):
            h.reset()
            parts = [_cut(cols, lo, hi) for lo, hi in zip((0,) + cuts, cuts + (n,))]
            los = (0,) + cuts
            bs = [h.upload_batch(c, with_keys=True) for c in parts]

            def feed(replay):
                for (b, nb), lo in zip(bs, los):
                    h.submit_device(b, nb, lo)

            _round(h, feed, want, P, M)
            with h.compaction_replay():                                             # a second replay starts from zero
                empty = h.compact_delete()
                assert list(empty["globals"]) == [0, 0, 0, 900, M, 3, 0, 0] and not empty["vector"][:-8].any()
                feed(True)
            _hold(h, want, P, M)
            _free(h, *[b for b, _ in bs])
        h.reset()                                                                   # the state is cleared, the switch and the configuration kept
        got = h.compact_delete()
        assert list(got["globals"]) == [0, 0, 0, 900, M, 3, 0, 0] and not got["vector"][:-8].any()
        assert h.compact_delete_info() == {"launches": 0, "chunks": 0, "chunks_applied": 0, "scratch_bytes": h.compact_delete_info()["scratch_bytes"]}
        half = _cut(cols, 0, 2500)
        _round(h, lambda replay: _submit(h, half, base_seq=0), _want(half, P, cfg), P, M)


# ------------------------------------------------------------------------------------------ tile forms, layouts, a view, a seq column
def _view(b, lo):
    v = N.KtaBatch()
    for f, sz in (("partition", 4), ("key_len", 4), ("val_len", 4), ("ts_ms", 8), ("key_off", 4)):
        setattr(v, f, getattr(b, f) + lo * sz)
    v.key_bytes = b.key_bytes
    return v


def test_every_tile_form_both_layouts_a_view_and_a_seq_column():
    import torch
    P, n = 6, 5 * 1024 + 5
    cols = _topic(30, n, P)
    cols["val_len"][1024 + 77] = 65535                                              # tile 1: lengths that do not fit u16
    cols["ts_ms"][2 * 1024 + 5] = BASE + 2**32                                      # tile 2: raw partitions and timestamps
    cols["val_len"][3 * 1024 + 9] = 70000                                           # tile 3: both
    cols["ts_ms"][3 * 1024 + 10] = BASE + 2**33
    M = 300
    cfg = (4096, M, 5)
    want = _want(cols, P, cfg)
    _exercises(want, P, M)
    with _handler(P, cfg) as h:
        for chunk in (0, 64):                                                       # a keyed allocation: compact and raw tiles, i32 lengths
            h.reset()
            h.set_segments_chunk(chunk)
            b, feed = _device_feed(h, cols)
            _round(h, feed, want, P, M)
        lo, hi = 4, n - 37                                                          # a view cut inside tiles
        sub = _cut(cols, lo, hi)
        h.reset()
        _round(h, lambda replay: h.submit_device(_view(b, lo), hi - lo, 0), _want(sub, P, cfg), P, M)
        _free(h, b)
        # a keyless allocation (u16 lengths where they fit) handed over with key columns of the caller's own
        h.reset()
        kb, nb = h.upload_batch({k: cols[k] for k in METRIC})
        dev = {"key_off": torch.from_numpy(cols["key_off"].view(np.int32)).cuda(), "key_bytes": torch.from_numpy(cols["key_bytes"]).cuda()}
        torch.cuda.synchronize()
        v = N.KtaBatch()
        for f in METRIC:
            setattr(v, f, getattr(kb, f))
        v.key_off, v.key_bytes = dev["key_off"].data_ptr(), dev["key_bytes"].data_ptr()
        _round(h, lambda replay: h.submit_device(v, nb, 0), want, P, M)
        _free(h, kb)
        h.reset()                                                                   # the raw layout: host batches through the staging ring
        _round(h, lambda replay: _submit(h, cols, base_seq=0), want, P, M)
    seq = np.random.default_rng(9).permutation(n).astype(np.uint64) * np.uint64(3) + np.uint64(10)
    want_seq = _want(cols, P, cfg, seq)
    assert not np.array_equal(want_seq[1], want[1])
    _exercises(want_seq, P, M)
    with _handler(P, cfg, seq_column=True) as h:
        b, nb = h.upload_batch(dict(cols, seq=seq), with_keys=True)
        _round(h, lambda replay: h.submit_device(b, nb, 12345), want_seq, P, M)     # (base_seq is not looked at)
        _free(h, b)


# ------------------------------------------------------------------------------------------ a closing chunk beside skipped ones
def test_a_closing_chunk_and_skipped_chunks_together():
    P, n = 4, 4096
    cols = _topic(11, n, P, outside=0.0, max_val=40)
    cand = np.flatnonzero(np.array(CD.classes(cols)) > 0)                            # (last writers: they stay so with another value length)
    at = np.array([int(cand[cand >= lo][0]) for lo in (100, 900, 2100, 2400)])      # partition 0 crosses S = 2^30 once, at the third: chunk 8
    assert at[2] // 256 == 8 and at[3] // 256 > 8
    cols["partition"][cols["partition"] == 0] = 1
    cols["partition"][at] = 0
    cols["val_len"][at] = (1 << 29) - 100
    M = 4
    cfg = (1 << 30, M, 0)
    want = _want(cols, P, cfg)
    _exercises(want, P, M)
    k = CD.split(want[1], P, M)
    assert int(k["globals"][2]) == 1 and int(k["rows"][0][0][1]) > 1 << 30 and int(k["rows"][0][0][0]) == 3 and int(k["totals"][0][0]) == 4
    with _handler(P, cfg) as h:
        h.set_segments_chunk(256)
        b, feed = _device_feed(h, cols)
        _round(h, feed, want, P, M)
        info = h.compact_delete_info()
        assert info["chunks"] == 16 and info["chunks_applied"] == 1 and info["launches"] == 3 and info["scratch_bytes"] >= n
        assert h.segments_info()["chunks_applied"] == 1
        _free(h, b)


# ------------------------------------------------------------------------------------------ submission paths
def test_staging_ring_in_several_batches_and_handle_message():
    P, n, cols = _medium()
    M = 64
    cfg = (900, M, 3)
    want = _want(cols, P, cfg)
    _exercises(want, P, M)
    with _handler(P, cfg, batch_capacity=1 << 10, key_bytes_capacity=1 << 16) as h:
        _round(h, lambda replay: _submit(h, cols, base_seq=0), want, P, M)           # six staging batches
        assert h.compact_delete_info()["launches"] >= 3 * 6
    sub = _cut(cols, 0, 2000)
    kb = cols["key_bytes"].tobytes()

    def feed(replay):
        if replay:
            h.replay_messages(sub)
            return
        for i in range(2000):
            kl = int(cols["key_len"][i])
            key = None if kl < 0 else kb[int(cols["key_off"][i]):int(cols["key_off"][i]) + kl]
            h.handle_message(kta.Message(int(cols["partition"][i]), int(cols["ts_ms"][i]), key, int(cols["val_len"][i])))

    want_sub = _want(sub, P, cfg)
    _exercises(want_sub, P, M)
    with _handler(P, cfg, batch_capacity=1 << 9) as h:
        _round(h, feed, want_sub, P, M)


def test_kafka_decode_consumed_twice():
    lib = N.load()
    P = 2
    rng = np.random.default_rng(8)
    blobs, recs = [], []
    for p in range(P):
        rows = []
        for i in range(300):
            key = None if i % 19 == 0 else b"user-%d" % int(rng.integers(0, 40))
            val = None if i % 10 == 0 else bytes(int(rng.integers(0, 300)))
            rows.append((i, key, val, []))
        blobs.append((b"".join(KF.encode_batch(lo, rows[lo:lo + 40], BASE) for lo in range(0, len(rows), 40)), p))
        recs += [(p, k, None if v is None else len(v)) for _, k, v, _ in rows]
    blob, off = b"", []
    for _, k, _ in recs:
        off.append(len(blob))
        blob += k or b""
    cols = {"partition": np.array([r[0] for r in recs], np.int32), "key_len": np.array([-1 if r[1] is None else len(r[1]) for r in recs], np.int32),
            "val_len": np.array([-1 if r[2] is None else r[2] for r in recs], np.int32), "ts_ms": np.full(len(recs), BASE, np.int64),
            "key_off": np.array(off, np.uint32), "key_bytes": np.frombuffer(blob + b"\0", np.uint8)}
    M = 100
    cfg = (2000, M, 70)

    def consume(replay):
        for blob, part in blobs:
            st = N.KtaKafkaIndexStats()
            h._check(lib.kta_kafka_consume(h._ctx, blob, len(blob), part, C.byref(st)))

    with _handler(P, cfg) as h:
        consume(False)
        h.finish()
        cols["ts_ms"] = None                                                        # the decoded timestamps: only H + 1 of the segment vector has them
        seg = h.segments()["vector"]
        with h.compaction_replay():
            consume(True)
        kept, comp = h.compact_delete()["vector"], h.compaction()["vector"]
    cls = CD.classes(cols)
    want_kept, want_comp = CD.kept_vector(cols, P, *cfg, cls=cls), CP.vector(cols, P)
    k = CD.split(want_kept, P, M)
    assert int(k["globals"][2]) > 3 and int(k["rows"][:, :, 0].max()) > 0 and int(k["rows"][:, :, 2].max()) > 0 and cls.count(0) > 100
    assert np.array_equal(kept, want_kept) and np.array_equal(comp, want_comp)
    assert CD.identities_hold(seg, kept, comp, P, M)
    kta.compact_delete_whatif(seg, kept, comp, P, M, BASE + 10, 5, 100)


def test_filtered_context_replays_the_passing_records():
    P, n, cols = _medium()
    frm, to, parts = BASE + 5_000, BASE + 45_000, [0, 2, 3]
    idx = np.nonzero(F.passes(cols["partition"], cols["ts_ms"], P, frm, to, parts))[0]
    assert 500 < len(idx) < n // 2
    taken = F.take(cols, idx, with_seq=True)
    M = 64
    cfg = (900, M, 3)
    want = _want(taken, P, cfg, taken["seq"])
    _exercises(want, P, M)
    with _handler(P, cfg) as h:
        h.set_filter(frm, to, parts)
        h.set_filter_slice(1024)
        b, feed = _device_feed(h, cols)
        _round(h, feed, want, P, M)
        assert int(h.compaction()["replayed"]) == len(idx)
        _free(h, b)


# ------------------------------------------------------------------------------------------ P at the wave-count switches and the bound
@pytest.mark.parametrize("P", [1024, 2048])
def test_partition_counts_at_the_apply_kernels_wave_count_switches(P):
    assert kta.compact_delete_max_partitions() == 2048
    n, M = 8192, 8
    cols = _topic(P, n, P, max_val=300)
    cfg = (300, M, 3)
    want = _want(cols, P, cfg)
    _exercises(want, P, M)
    with _handler(P, cfg) as h:
        h.set_segments_chunk(1024)
        b, feed = _device_feed(h, cols)
        _round(h, feed, want, P, M)
        _free(h, b)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals():
    P = 4
    cols = _topic(3, 500, P)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, alive_table=True, segments=(100, 8, 0)) as h:
        with pytest.raises(kta.KtaError, match="KTA_FLAG_COMPACTION"):
            h.set_compact_delete(True)
    with pytest.raises(kta.KtaError, match="KTA_FLAG_COMPACTION"):
        kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, segments=(100, 8, 0), compact_delete=True)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True) as h:
        with pytest.raises(kta.KtaError, match="kta_set_segments"):
            h.set_compact_delete(True)
        for fn in (h.compact_delete_info, lambda: h._check(h._lib.kta_get_compact_delete(h._ctx, np.zeros(8, np.uint64).ctypes.data, 8))):
            with pytest.raises(kta.KtaError, match="kta_set_compact_delete"):
                fn()
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True, segments=(100, 8, 0)) as h:
        _submit(h, cols, base_seq=0)
        with pytest.raises(kta.KtaError, match="handed records"):
            h.set_compact_delete(True)
        h.reset()
        h.set_compact_delete(True)                                                  # after a reset it is taken
        with pytest.raises(kta.KtaError, match="KTA_FLAG_COMPACTION"):
            h.comm_create(2, 0, bytes(128))
        with pytest.raises(kta.KtaError, match="words"):
            h._check(h._lib.kta_get_compact_delete(h._ctx, np.zeros(8, np.uint64).ctypes.data, 8))
        h.set_segments(200, 8, 0)                                                   # another configuration turns the switch off
        with pytest.raises(kta.KtaError, match="kta_set_compact_delete"):
            h.compact_delete()
    # 2049 partitions: the segment pass's own bound refuses first; 2048 is taken (test above)
    with pytest.raises(kta.KtaError, match="at most 2048 partitions"):
        kta.HipMetricHandler(2049, count_alive_keys=True, now=NOW, compaction=True, segments=(100, 2, 0), compact_delete=True)
    with kta.HipMetricHandler(2049, count_alive_keys=True, now=NOW, compaction=True) as h:
        with pytest.raises(kta.KtaError):
            h.set_compact_delete(True)


# ------------------------------------------------------------------------------------------ the switch off
def test_the_switch_off_replays_to_the_vectors_it_always_wrote():
    P, n, cols = _medium()
    M = 64
    cfg = (900, M, 3)
    want = _want(cols, P, cfg)
    got = {}
    for on in (False, True):
        with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True, segments=cfg, compact_delete=on) as h:
            b, feed = _device_feed(h, cols)
            feed(False)
            res, c = h.finish(allow_bad_partition=True)
            with h.compaction_replay():
                feed(True)
            res2, c2 = h.finish(allow_bad_partition=True)
            got[on] = (bytes(res), c, h.segments()["vector"], h.compaction()["vector"], h.compaction_info(), h.segments_info())
            assert bytes(res) == bytes(res2) and np.array_equal(c, c2)
            if on:
                _hold(h, want, P, M)
                h.set_segments_chunk(0)
            else:
                with pytest.raises(kta.KtaError, match="kta_set_compact_delete"):
                    h.compact_delete()
            _free(h, b)
    for a, b in zip(got[False], got[True]):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    assert np.array_equal(got[False][2], want[0]) and np.array_equal(got[False][3], want[2])
    # switched on and then off again before the first record: the replay leaves the kept vector zero
    with _handler(P, cfg) as h:
        h.set_compact_delete(False)
        b, feed = _device_feed(h, cols)
        feed(False)
        h.finish(allow_bad_partition=True)
        with h.compaction_replay():
            feed(True)
        assert np.array_equal(h.compaction()["vector"], want[2])
        h.reset()
        h.set_compact_delete(True)
        empty = h.compact_delete()
        assert list(empty["globals"]) == [0, 0, 0, 900, M, 3, 0, 0] and not empty["vector"][:-8].any()
        _free(h, b)


# ------------------------------------------------------------------------------------------ every opt-in at once
def test_every_opt_in_at_once_the_replay_touches_none_of_the_others():
    P, n, cols = _medium()
    cols = dict(cols, partition=np.clip(cols["partition"], 0, P - 1))
    tl = (BASE - 10**6, 10_000, 40)
    M = 64
    cfg = (900, M, 3)
    want = _want(cols, P, cfg)
    _exercises(want, P, M)
    with _handler(P, cfg, batch_capacity=1 << 11, key_bytes_capacity=1 << 17, analytics=True, timeline=tl, key_sketch=True, hot_keys=True,
                  ts_order=True, partitioner=True, size_quantiles=True) as h:
        def snapshot():
            res, c = h.finish()
            return [bytes(res), c, h.exchange_partitioner()["vector"], h.exchange_key_sketch(), h.exchange_timeline(),
                    h.exchange_ts_order()["vector"], h.exchange_hot_keys(), h.exchange_size_quantiles()["vector"], h.exchange_segments()["vector"],
                    h.partitioner()["vector"], h.key_sketch(), h.timeline(), h.ts_order()["vector"], h.hot_keys(), h.segments()["vector"],
                    str({k: np.asarray(v).tolist() for k, v in sorted(h.exchange_analytics().items())}).encode()]
        _submit(h, cols, base_seq=0)
        before = snapshot()
        with h.compaction_replay():
            _submit(h, cols, base_seq=0)
        after = snapshot()
        for x, y in zip(before, after):
            assert x == y if isinstance(x, bytes) else np.array_equal(x, y)
        _hold(h, want, P, M)


# ------------------------------------------------------------------------------------------ the CLI
def _cli(*args):
    return subprocess.run(["timeout", "-k", "10", "240", CLI, *args], capture_output=True, text=True, timeout=270)


def _normalise(text):
    text = re.sub(r"Scanning took: \d+ seconds", "Scanning took: 3 seconds", text)
    return re.sub(r"Estimated Msg/s: \d+", "Estimated Msg/s: 133", text)


def test_cli_section_on_a_synthetic_topic_and_nothing_without_the_knob():
    sp, _ = kta.synth_preset("c2")
    n, P = 20000, int(sp.n_partitions)
    src = "synthetic://c2?records=%d" % n
    cols = kta.synth_fill_host(sp, 0, n, with_keys=True)
    M = min(1024, (1 << 20) // P)
    S, overhead, now_s = 16 << 10, 70, int(cols["ts_ms"].max()) // 1000 + 5
    want = _want(cols, P, (S, M, overhead))
    _exercises(want, P, M)
    span = int(cols["ts_ms"].max() - cols["ts_ms"][cols["ts_ms"] >= 0].min()) // 1000
    rms_s = max(span // 2, 1)
    both = "kta.compaction=1,kta.segments=16k,kta.segments.overhead=70,kta.retention.now=%d,kta.retention.ms=%ds,kta.retention.bytes=64k" % (now_s, rms_s)
    section = CD.section(want[0], want[1], want[2], P, M, now_s * 1000, rms_s * 1000, 64 << 10)
    assert " time " in section or " size " in section                               # (the policy does cut something)
    plain = _cli("-t", "t", "-b", src, "-c", "--librdkafka", both)
    assert plain.returncode == 0 and "Compact,delete" not in plain.stdout, plain.stderr
    off = _cli("-t", "t", "-b", src, "-c", "--librdkafka", both + ",kta.compact_delete=0")
    assert off.returncode == 0 and _normalise(off.stdout) == _normalise(plain.stdout)
    r = _cli("-t", "t", "-b", src, "-c", "--librdkafka", both + ",kta.compact_delete=1,kta.from=0")
    assert r.returncode == 0, r.stderr
    out = r.stdout
    assert out.index("Compaction what-if:") < out.index("Retention what-if:") < out.index("Compact,delete what-if:") < out.index("Record filter:")
    r = _cli("-t", "t", "-b", src, "-c", "--librdkafka", both + ",kta.compact_delete=1")
    assert r.returncode == 0, r.stderr
    at = r.stdout.index("Compact,delete what-if:")
    assert r.stdout[at:] == section and _normalise(r.stdout[:at]) == _normalise(plain.stdout)

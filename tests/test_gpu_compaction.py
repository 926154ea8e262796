"""GPU tests of the compaction what-if (KTA_FLAG_COMPACTION: a replay of the first pass's records against the last-writer
table adds up, per partition, the records and bytes log compaction would keep; no reference counterpart), the vector
bit-identical to the independent restatement in tests/compaction_py.py:

    the topic            60 000 random records, P = 6: null and empty keys, 30 % tombstones, key lengths 0..300, partitions -1
                         and P + 3, and a pair of distinct 8-byte keys of one FNV hash in different partitions
    entry paths          the staging ring, kta_handle_message / kta_replay_messages, raw and tile-compact device batches,
                         views cut inside tiles, batches in reverse order with base_seq, a seq column that neither ascends nor
                         is consecutive — each: first pass, replay, the vector, the three identities, finish unchanged
    small shapes         n around the wave, the step and the tile; P in {1, 6, 256, 257, the limit}; 16-byte keys
    contention           2^20 records of one key, of two keys alternating, of distinct keys, of keys that all end deleted
    mismatch             base_seq shifted, half the records, a replay run twice
    behaviour            refusals, kta_reset, the calls of a context without the flag, kta_comm_create with 2 ranks
    with the filter      a filtered context against an unfiltered one handed the passing records with the numbers they kept
    every opt-in         their vectors after the replay are their vectors before it
    the Kafka decode     raw log segments consumed twice
    kta-analyzer         -c kta.compaction=1 on synthetic://, segment:// and dump://; nothing changes without the key"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import compaction_py as CP
import filter_py as F
import kafka_format as KF
import key_sketch_py as KS
from helpers import NOW, random_cols

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
LIMIT = 4096


def _colliding_pair():
    """Two distinct 8-byte keys of one FNV hash, found by hashing 2^18 random keys (about eight pairs expected)."""
    for seed in range(50, 60):
        keys = np.random.default_rng(seed).integers(0, 256, size=(1 << 18, 8), dtype=np.uint8)
        h = np.full(len(keys), 0x811C9DC5, np.uint64)
        for j in range(8):
            h = ((h ^ keys[:, j].astype(np.uint64)) * np.uint64(0x811C9DC5)) & np.uint64(0xFFFFFFFF)
        order = np.argsort(h, kind="stable")
        same = np.nonzero(h[order][1:] == h[order][:-1])[0]
        for s in same:
            a, b = keys[order[s]].tobytes(), keys[order[s + 1]].tobytes()
            if a != b:
                assert KS.fnv1a(a) == KS.fnv1a(b)
                return a, b
    raise AssertionError("no colliding pair among 10 * 2^18 keys")


def _append(cols, records):
    """cols + [(partition, key, val_len)] at the end."""
    blob = cols["key_bytes"].tobytes()
    add = {"partition": [], "key_len": [], "val_len": [], "ts_ms": [], "key_off": []}
    for p, key, vl in records:
        add["partition"].append(p), add["key_len"].append(len(key)), add["val_len"].append(vl)
        add["ts_ms"].append(1_600_000_000_000), add["key_off"].append(len(blob))
        blob += key
    out = {k: np.concatenate([cols[k], np.array(v, cols[k].dtype)]) for k, v in add.items()}
    out["key_bytes"] = np.frombuffer(blob, np.uint8).copy()
    return out


def _cols(seed, n=60000, P=6, key_space=9000, max_key=300):
    rng = np.random.default_rng(seed)
    cols = random_cols(rng, n, P, key_space=key_space, null_key=0.1, empty_key=0.03, tomb=0.3, max_key=max_key)
    cols["partition"][rng.random(n) < 0.02] = -1            # a damaged batch's records
    cols["partition"][rng.random(n) < 0.02] = P + 3          # out of range
    return cols


@pytest.fixture(scope="module")
def topic():
    """The records of the entry-path tests, their hashes and their vector, computed once."""
    P = 6
    a, b = _colliding_pair()
    cols = _append(_cols(1), [(0, a, 11), (1, b, 13)])      # the pair at the end: a is superseded by b
    h = CP.hashes(cols)
    return {"P": P, "cols": cols, "h": h, "pair": (a, b), "want": CP.vector(cols, P, h=h), "n": len(cols["partition"])}


def _submit(h, cols, base_seq=None):
    h.submit_columns(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"], cols["key_off"], cols["key_bytes"], base_seq=base_seq)


def _part(cols, lo, hi):
    return {k: (v if k == "key_bytes" else v[lo:hi]) for k, v in cols.items()}


def _identities(v, res, counters):
    assert int(v["live_records"].sum()) + v["live_outside"] == res.alive_keys
    assert v["unknown"] == 0
    assert (v["live_records"] + v["tombstone_records"] <= counters[:, N.KTA_C_KEY_NON_NULL]).all()


def _first_pass_and_replay(h, feed, want, P):
    """feed(replay) hands the records over; -> the vector as a dict, checked against `want`, the identities, and the finish
    results before and after the replay."""
    feed(False)
    res, c = h.finish(allow_bad_partition=True)
    with h.compaction_replay():
        feed(True)
    got = h.compaction()
    assert np.array_equal(got["vector"], want)
    res2, c2 = h.finish(allow_bad_partition=True)
    assert bytes(res) == bytes(res2) and np.array_equal(c, c2) and res.alive_keys == res2.alive_keys
    _identities(got, res, c)
    assert int(got["replayed"]) == int(c[:, N.KTA_C_TOTAL].sum()) + res.bad_partition_records
    assert kta.render_compaction(got["vector"], h.result_vector_host(), P) == CP.section(got["vector"], h.result_vector_host(), P)
    return got


def test_the_input_exercises_every_class(topic):
    cols, h, P, n = topic["cols"], topic["h"], topic["P"], topic["n"]
    k = CP.survivors(cols, np.arange(n, dtype=np.uint64), CP.last_writers(cols, np.arange(n, dtype=np.uint64), h), h)
    keyed, vl, part = cols["key_len"] >= 0, cols["val_len"], cols["partition"]
    for p in range(P):
        here = part == p
        assert ((k == 1) & (vl >= 0) & here).any() and ((k == 1) & (vl < 0) & here).any() and ((k == 0) & keyed & here).any(), p
    assert not (k == -1).any() and (~keyed).any()
    v = CP.split(topic["want"], P)
    assert v["unkeyed"] > 0 and v["live_outside"] > 0 and v["tombstones_outside"] > 0
    a, b = topic["pair"]
    assert a != b and h[n - 2] == h[n - 1] and part[n - 2] != part[n - 1] and k[n - 2] == 0 and k[n - 1] == 1
    kl = cols["key_len"][keyed]
    assert {int(x) for x in np.unique(kl % 4)} == {0, 1, 2, 3} and (kl > 16).any() and (kl == 0).any() and kl.max() > 250


# ------------------------------------------------------------------------------------------ entry paths
def test_staging_ring_in_several_batches(topic):
    P, cols = topic["P"], topic["cols"]
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, batch_capacity=1 << 13, key_bytes_capacity=1 << 17, compaction=True) as h:
        _first_pass_and_replay(h, lambda replay: _submit(h, cols, base_seq=0), topic["want"], P)
        info = h.compaction_info()
        assert info["keyed_records"] == int((cols["key_len"] >= 0).sum()) and info["launches"] >= 8 and info["workgroups"] >= info["launches"]
        survivors = int(topic["want"][:CP.WORDS * P:CP.WORDS].sum()), int(topic["want"][3:CP.WORDS * P:CP.WORDS].sum())
        assert info["lds_adds"] == 3 * survivors[0] + 2 * survivors[1] and info["lds_bytes"] == 32 * P * 32 and info["reserved"] == 0


def test_handle_message_then_replay_messages(topic):
    P, cols = topic["P"], topic["cols"]
    sub = _part(cols, 0, 3000)
    kb = cols["key_bytes"].tobytes()

    def feed(replay):
        if replay:
            h.replay_messages(sub)
            return
        for i in range(3000):
            kl = int(cols["key_len"][i])
            key = None if kl < 0 else kb[int(cols["key_off"][i]):int(cols["key_off"][i]) + kl]
            h.handle_message(kta.Message(int(cols["partition"][i]), int(cols["ts_ms"][i]), key, int(cols["val_len"][i])))

    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, batch_capacity=1 << 10, compaction=True) as h:
        _first_pass_and_replay(h, feed, CP.vector(sub, P, h=topic["h"][:3000]), P)
        # the numbering of the first pass goes on where it was: 3000 more records are newer than all before
        h.replay_messages(_part(cols, 3000, 6000))
        res, c = h.finish(allow_bad_partition=True)
        with h.compaction_replay():
            h.replay_messages(_part(cols, 0, 6000))
        got = h.compaction()
        assert np.array_equal(got["vector"], CP.vector(_part(cols, 0, 6000), P, h=topic["h"][:6000]))
        _identities(got, res, c)


def test_raw_layout_device_batch_whatever_which_says(topic):
    import torch
    P, cols, n = topic["P"], topic["cols"], topic["n"]
    dev = {k: torch.from_numpy(np.ascontiguousarray(cols[k])).cuda() for k in ("partition", "key_len", "val_len", "ts_ms")}
    dev["key_off"] = torch.from_numpy(cols["key_off"].view(np.int32)).cuda()
    kb = np.zeros(len(cols["key_bytes"]) + 16, np.uint8)     # readable 16 bytes past the last key
    kb[:len(cols["key_bytes"])] = cols["key_bytes"]
    dev["key_bytes"] = torch.from_numpy(kb).cuda()
    torch.cuda.synchronize()
    b = N.KtaBatch()
    for k, t in dev.items():
        setattr(b, k, t.data_ptr())
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True) as h:
        _first_pass_and_replay(h, lambda replay: h.submit_device(b, n, 0, which=3), topic["want"], P)
        for which in (1, 2):
            with h.compaction_replay():
                h.submit_device(b, n, 0, which=which)
            assert np.array_equal(h.compaction()["vector"], topic["want"]), which
        h.sync()


def test_tile_compact_device_batch_whole_and_as_views_cut_inside_tiles(topic):
    P, cols, n = topic["P"], topic["cols"], topic["n"]
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True) as h:
        b, nb = h.upload_batch(cols, with_keys=True)
        assert nb == n
        cuts = ((0, 1036), (1036, 2 * 1024 + 4), (2 * 1024 + 4, n))      # (a view's columns stay 16-byte aligned)

        def views(replay):
            for lo, hi in cuts:
                v = N.KtaBatch()
                v.partition, v.key_len, v.val_len = b.partition + 4 * lo, b.key_len + 4 * lo, b.val_len + 4 * lo
                v.ts_ms, v.key_off, v.key_bytes = b.ts_ms + 8 * lo, b.key_off + 4 * lo, b.key_bytes
                h.submit_device(v, hi - lo, lo)

        _first_pass_and_replay(h, lambda replay: h.submit_device(b, n, 0), topic["want"], P)
        with h.compaction_replay():          # the whole batch's table, the views' replay
            views(True)
        assert np.array_equal(h.compaction()["vector"], topic["want"])
        h.reset()
        _first_pass_and_replay(h, views, topic["want"], P)
        h.sync()
        h.device_batch_free(b)


def test_batches_in_reverse_order_with_explicit_base_seq(topic):
    P, cols, n = topic["P"], topic["cols"], topic["n"]
    los = list(range(0, n, 7000))[::-1]

    def feed(replay):
        for lo in los:
            _submit(h, _part(cols, lo, min(lo + 7000, n)), base_seq=lo)

    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, batch_capacity=1 << 13, key_bytes_capacity=1 << 20, alive_table=True,
                              compaction=True) as h:
        _first_pass_and_replay(h, feed, topic["want"], P)


def test_seq_column_that_neither_ascends_nor_is_consecutive(topic):
    P, cols, n = topic["P"], topic["cols"], topic["n"]
    seq = np.random.default_rng(9).permutation(n).astype(np.uint64) * np.uint64(3) + np.uint64(10)
    want = CP.vector(cols, P, seq, h=topic["h"])
    assert not np.array_equal(want, topic["want"])
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, seq_column=True, compaction=True) as h:
        b, nb = h.upload_batch(dict(cols, seq=seq), with_keys=True)
        _first_pass_and_replay(h, lambda replay: h.submit_device(b, nb, 12345), want, P)      # (base_seq is not looked at)
        h.sync()
        h.device_batch_free(b)


# ------------------------------------------------------------------------------------------ small shapes
def _small(n, P, seed, max_key=23, key_space=50):
    cols = random_cols(np.random.default_rng(seed), n, P, key_space=key_space, null_key=0.1, empty_key=0.1, tomb=0.3, max_key=max_key)
    kb = cols["key_bytes"].tobytes() + b"seven b"           # the last record's key, 7 bytes, ends the blob
    cols["key_off"][n - 1], cols["key_len"][n - 1], cols["partition"][n - 1] = len(kb) - 7, 7, P - 1
    cols["key_bytes"] = np.frombuffer(kb, np.uint8)
    return cols


def _device_round(h, cols, P, want=None):
    b, nb = h.upload_batch(cols, with_keys=True)
    got = _first_pass_and_replay(h, lambda replay: h.submit_device(b, nb, 0), CP.vector(cols, P) if want is None else want, P)
    h.sync()
    h.device_batch_free(b)
    return got


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4 * 1024 + 7])
def test_small_shapes_the_last_key_ends_key_bytes(n):
    P = 3
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True) as h:
        got = _device_round(h, _small(n, P, 100 + n), P)
        assert got["replayed"] == n and int(got["live_records"][P - 1]) >= 1     # the last record survives


@pytest.mark.parametrize("P", [1, 6, 256, 257, LIMIT])
def test_partition_counts_up_to_the_limit(P):
    n = 4 * 1024 + 7
    cols = _small(n, P, 200 + P, key_space=3000)
    cols["partition"][::97] = P                                 # just outside
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True) as h:
        assert h.compaction_info()["lds_bytes"] == 32 * P * (32 if P <= 16 else 2 if P == 256 else 1)
        got = _device_round(h, cols, P)
        assert got["live_outside"] + got["tombstones_outside"] > 0


def test_the_limit_plus_one_is_refused():
    assert kta.compaction_max_partitions() == LIMIT
    with pytest.raises(kta.KtaError, match="KTA_FLAG_COMPACTION admits at most %d" % LIMIT):
        kta.HipMetricHandler(LIMIT + 1, count_alive_keys=True, now=NOW, compaction=True)


def test_all_keys_16_bytes_the_four_chain_path():
    P, n, K = 4, 1025, 200
    rng = np.random.default_rng(11)
    keys = rng.integers(0, 256, size=(K, 16), dtype=np.uint8)
    kid = rng.integers(0, K, n)
    cols = {"partition": rng.integers(0, P, n).astype(np.int32), "key_len": np.full(n, 16, np.int32),
            "val_len": np.where(rng.random(n) < 0.3, -1, rng.integers(0, 500, n)).astype(np.int32),
            "ts_ms": np.full(n, 1_600_000_000_000, np.int64), "key_off": (16 * np.arange(n)).astype(np.uint32),
            "key_bytes": keys[kid].reshape(-1).copy()}          # the last key ends key_bytes
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True) as h:
        got = _device_round(h, cols, P)
        assert int(got["live_records"].sum() + got["tombstone_records"].sum()) == len(np.unique(kid))


# ------------------------------------------------------------------------------------------ contention and extremes
def _repeat_keys(keys, parts, n, val_len=10):
    """n records cycling through `keys` (16 bytes each) lane by lane."""
    k = len(keys)
    blob = np.frombuffer(b"".join(keys), np.uint8)
    i = np.arange(n) % k
    return {"partition": np.asarray(parts, np.int32)[i], "key_len": np.full(n, 16, np.int32),
            "val_len": np.full(n, val_len, np.int32), "ts_ms": np.full(n, 1_600_000_000_000, np.int64),
            "key_off": (16 * i).astype(np.uint32), "key_bytes": blob}


def test_one_key_throughout_one_survivor():
    n, P = 1 << 20, 3
    cols = _repeat_keys([b"the one hot key!"], [2], n)
    want = np.zeros(CP.words(P), np.uint64)
    want[CP.WORDS * 2:CP.WORDS * 2 + 3] = (1, 16, 10)
    want[CP.WORDS * P + CP.REPLAYED] = n
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True) as h:
        got = _device_round(h, cols, P, want)
        info = h.compaction_info()
        assert info["keyed_records"] == n and info["lds_adds"] == 3 and int(got["live_records"].sum()) == 1


def test_two_keys_alternating():
    n, P = 1 << 20, 5
    keys = [b"key number one ..", b"key number two .."]
    cols = _repeat_keys([k[:16] for k in keys], [1, 4], n)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True) as h:
        got = _device_round(h, cols, P)
        assert got["live_records"].tolist() == [0, 1, 0, 0, 1] and h.compaction_info()["lds_adds"] == 6


def test_2e20_distinct_16_byte_keys_every_record_survives():
    sp, _ = kta.synth_preset("c3")
    sp.n_distinct_keys, sp.key_null_permille, sp.key_empty_permille = 0, 0, 0
    n, P = 1 << 20, int(sp.n_partitions)
    cols = kta.synth_fill_host(sp, 0, n, with_keys=True)
    assert (cols["key_len"] == 16).all()
    h32 = CP.hashes(cols)
    want = CP.vector(cols, P, h=h32)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True) as h:
        got = _device_round(h, cols, P, want)
        kept = int(got["live_records"].sum() + got["tombstone_records"].sum())
        assert kept == len(np.unique(h32)) and kept > n - 300      # (two keys of one 32-bit hash are one key: about 2^40 / 2^33 pairs)


def test_every_keys_last_record_a_tombstone_no_live_survivors():
    n, P, K = 1 << 20, 4, 1 << 14
    rng = np.random.default_rng(12)
    keys = rng.integers(0, 256, size=(K, 16), dtype=np.uint8)
    kid = np.concatenate([rng.integers(0, K, n - K), rng.permutation(K)])
    cols = {"partition": (kid % P).astype(np.int32), "key_len": np.full(n, 16, np.int32),
            "val_len": np.concatenate([rng.integers(0, 100, n - K), np.full(K, -1)]).astype(np.int32),
            "ts_ms": np.full(n, 1_600_000_000_000, np.int64), "key_off": (16 * kid).astype(np.uint32), "key_bytes": keys.reshape(-1).copy()}
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True) as h:
        got = _device_round(h, cols, P)
        assert not got["live_records"].any() and not got["live_value_bytes"].any()
        assert int(got["tombstone_records"].sum()) == len(np.unique(CP.hashes(_part(cols, n - K, n)))) and h.finish()[0].alive_keys == 0


# ------------------------------------------------------------------------------------------ mismatch
def test_a_replay_that_does_not_match_and_a_replay_run_twice(topic):
    P, cols, n = topic["P"], topic["cols"], topic["n"]
    table = CP.last_writers(cols, np.arange(n, dtype=np.uint64), topic["h"])
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True) as h:
        b, nb = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, nb, 0)
        res, c = h.finish(allow_bad_partition=True)
        cv = h.result_vector_host()
        with h.compaction_replay():
            h.submit_device(b, nb, 7)                        # base_seq shifted by + 7
        got = h.compaction()
        assert np.array_equal(got["vector"], CP.vector(cols, P, np.arange(n, dtype=np.uint64) + np.uint64(7), table, h=topic["h"]))
        assert got["unknown"] > 0 and got["replayed"] == n
        with pytest.raises(kta.KtaError) as e:
            kta.render_compaction(got["vector"], cv, P)
        assert e.value.code == N.KTA_ERR_INVALID and "did not match" in e.value.text
        half = n // 2
        with h.compaction_replay():
            h.submit_device(b, half, 0)                      # half the records
        got = h.compaction()
        assert np.array_equal(got["vector"], CP.vector(_part(cols, 0, half), P, None, table, h=topic["h"][:half]))
        assert got["replayed"] == half and got["unknown"] == 0
        with pytest.raises(kta.KtaError) as e:
            kta.render_compaction(got["vector"], cv, P)
        assert "replayed %d of %d records" % (half, n) in e.value.text
        for _ in range(2):                                   # off, on again: zeroed on entry
            h.compaction_replay(True)
            h.compaction_replay(True)                        # (the mode it is in: nothing happens)
            h.submit_device(b, nb, 0)
            h.compaction_replay(False)
            assert np.array_equal(h.compaction()["vector"], topic["want"])
        res2, c2 = h.finish(allow_bad_partition=True)
        assert bytes(res) == bytes(res2) and np.array_equal(c, c2)
        h.sync()
        h.device_batch_free(b)


# ------------------------------------------------------------------------------------------ behaviour
def test_refusals_reset_and_calls_without_the_flag():
    P = 4
    cols = _cols(3, n=5000, P=P, key_space=600)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True) as h:
        b, n = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, n, 0)
        _, c0 = h.finish(allow_bad_partition=True)
        nokeys = N.KtaBatch()
        nokeys.partition, nokeys.key_len, nokeys.val_len, nokeys.ts_ms = b.partition, b.key_len, b.val_len, b.ts_ms
        h.submit_device(nokeys, n, n, which=1)               # outside replay mode the metrics handler needs no keys
        launches = h.compaction_info()["launches"]
        h.compaction_replay(True)
        for which in (1, 2, 3):
            with pytest.raises(kta.KtaError, match=r"key columns missing \(KTA_FLAG_COMPACTION\)"):
                h.submit_device(nokeys, n, 0, which=which)
        assert not h.compaction()["vector"].any() and h.compaction_info()["launches"] == launches == 0
        h.submit_device(b, n, 0)
        assert np.array_equal(h.compaction()["vector"], CP.vector(cols, P))
        h.reset()                                            # zeroes the vector and leaves replay mode
        assert not h.compaction()["vector"].any() and h.compaction_info()["launches"] == 0
        h.submit_device(b, n, 0)                             # a first pass again: the counters count, the vector stays zero
        _, c1 = h.finish(allow_bad_partition=True)
        assert np.array_equal(c0, c1) and not h.compaction()["vector"].any()
        with pytest.raises(kta.KtaError, match="KTA_FLAG_COMPACTION"):
            h.comm_create(2, 0, bytes(128))
        h.sync()
        h.device_batch_free(b)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, alive_table=True) as h:
        for fn in (h.compaction, h.compaction_info, lambda: h.compaction_replay(True), lambda: h.compaction_replay(False)):
            with pytest.raises(kta.KtaError, match="KTA_FLAG_COMPACTION"):
                fn()
    with pytest.raises(kta.KtaError, match="KTA_FLAG_COMPACTION needs count_alive_keys"):
        kta.HipMetricHandler(P, now=NOW, compaction=True)


# ------------------------------------------------------------------------------------------ with the filter
def test_filtered_context_replays_the_passing_records_with_the_numbers_they_kept(topic):
    P, cols, n = topic["P"], topic["cols"], topic["n"]
    frm, to, parts = 1_600_000_000_000 - 300_000_000, 1_600_000_000_000 + 500_000_000, [0, 2, 3, 5]
    idx = np.nonzero(F.passes(cols["partition"], cols["ts_ms"], P, frm, to, parts))[0]
    assert 1000 < len(idx) < n // 2
    taken = F.take(cols, idx, with_seq=True)
    want = CP.vector(taken, P, taken["seq"])
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True) as h, \
            kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True) as plain:
        h.set_filter(frm, to, parts)
        h.set_filter_slice(8192)
        b, nb = h.upload_batch(cols, with_keys=True)
        got = _first_pass_and_replay(h, lambda replay: h.submit_device(b, nb, 0), want, P)
        assert got["replayed"] == len(idx)
        pb, pn = plain.upload_batch(taken, with_keys=True)
        same = _first_pass_and_replay(plain, lambda replay: plain.submit_device(pb, pn, 0), want, P)
        assert np.array_equal(got["vector"], same["vector"])
        for x, bb in ((h, b), (plain, pb)):
            x.sync()
            x.device_batch_free(bb)


# ------------------------------------------------------------------------------------------ every opt-in at once
def test_every_opt_in_at_once_the_replay_touches_none_of_them():
    P, n = 6, 30000
    cols = _cols(5, n=n, P=P, key_space=4000, max_key=64)
    cols["partition"] = np.clip(cols["partition"], 0, P - 1)
    tl = (1_600_000_000_000 - 10**9, 50_000_000, 40)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, batch_capacity=1 << 13, key_bytes_capacity=1 << 19, analytics=True,
                              timeline=tl, key_sketch=True, hot_keys=True, ts_order=True, partitioner=True, compaction=True) as h:
        def snapshot():
            res, c = h.finish()
            return [bytes(res), c, h.exchange_partitioner()["vector"], h.exchange_key_sketch(), h.exchange_timeline(),
                    h.exchange_ts_order()["vector"], h.exchange_hot_keys(), h.partitioner()["vector"], h.key_sketch(), h.timeline(),
                    h.ts_order()["vector"], h.hot_keys(),
                    str({k: np.asarray(v).tolist() for k, v in sorted(h.exchange_analytics().items())}).encode()]
        _submit(h, cols, base_seq=0)
        before = snapshot()
        with h.compaction_replay():
            _submit(h, cols, base_seq=0)
        got = h.compaction()
        assert np.array_equal(got["vector"], CP.vector(cols, P))
        after = snapshot()
        for x, y in zip(before, after):
            assert x == y if isinstance(x, bytes) else np.array_equal(x, y)
        assert before[2].any() and before[3].any() and before[4].any() and before[6].any()


# ------------------------------------------------------------------------------------------ the Kafka decode
def _segments(P, per_partition=300):
    """-> ([(blob, partition)], columns of the records in consumption order)"""
    rng = np.random.default_rng(8)
    blobs, recs = [], []
    for p in range(P):
        rows = []
        for i in range(per_partition):
            key = None if i % 11 == 0 else (b"" if i % 53 == 0 else b"user-%d" % int(rng.integers(0, 120)))
            val = None if i % 7 == 0 else bytes(int(rng.integers(0, 300)))
            rows.append((i, key, val, []))
        blob = b"".join(KF.encode_batch(lo, rows[lo:lo + 40], 1_600_000_000_000) for lo in range(0, len(rows), 40))
        blobs.append((blob, p))
        recs += [(p, k, None if v is None else len(v)) for _, k, v, _ in rows]
    blob, off = b"", []
    for _, k, _ in recs:
        off.append(len(blob))
        blob += k or b""
    cols = {"partition": np.array([r[0] for r in recs], np.int32),
            "key_len": np.array([-1 if r[1] is None else len(r[1]) for r in recs], np.int32),
            "val_len": np.array([-1 if r[2] is None else r[2] for r in recs], np.int32), "key_off": np.array(off, np.uint32),
            "key_bytes": np.frombuffer(blob + b"\0", np.uint8)}
    return blobs, cols


def test_kafka_decode_consumed_twice():
    lib = N.load()
    P = 2
    blobs, cols = _segments(P)
    want = CP.vector(cols, P)
    assert CP.split(want, P)["tombstone_records"].all() and CP.split(want, P)["live_records"].all()

    def consume(replay):
        for blob, part in blobs:
            st = N.KtaKafkaIndexStats()
            h._check(lib.kta_kafka_consume(h._ctx, blob, len(blob), part, C.byref(st)))

    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True) as h:
        _first_pass_and_replay(h, consume, want, P)


# ------------------------------------------------------------------------------------------ the CLI
def _cli(*args):
    return subprocess.run(["timeout", "-k", "10", "240", CLI, *args], capture_output=True, text=True, timeout=270)


def _normalise(text):
    text = re.sub(r"Scanning took: \d+ seconds", "Scanning took: 3 seconds", text)
    return re.sub(r"Estimated Msg/s: \d+", "Estimated Msg/s: 133", text)


def _split(stdout):
    at = stdout.index("Compaction what-if:")
    return stdout[:at], stdout[at:]


def _check_cli(src, cols, P, extra=""):
    want = CP.section(CP.vector(cols, P), CP.counters(cols, P), P)
    plain = _cli("-t", "t", "-b", src, "-c", *(["--librdkafka", extra] if extra else []))
    assert plain.returncode == 0 and "Compaction" not in plain.stdout, plain.stderr
    r = _cli("-t", "t", "-b", src, "-c", "--librdkafka", "kta.compaction=1" + ("," + extra if extra else ""))
    assert r.returncode == 0, r.stderr
    report, section = _split(r.stdout)
    assert section == want and _normalise(report) == _normalise(plain.stdout)
    alive = int(re.search(r"^Alive keys: (\d+)$", report, flags=re.M).group(1))
    v = CP.split(CP.vector(cols, P), P)
    assert alive == int(v["live_records"].sum()) + v["live_outside"]
    off = _cli("-t", "t", "-b", src, "-c", "--librdkafka", "kta.compaction=0" + ("," + extra if extra else ""))
    assert off.returncode == 0 and _normalise(off.stdout) == _normalise(plain.stdout)
    return r


def test_cli_section_on_a_synthetic_topic_and_its_dump(tmp_path):
    sp, _ = kta.synth_preset("c2")
    n, P = 100000, int(sp.n_partitions)
    cols = kta.synth_fill_host(sp, 0, n, with_keys=True)
    _check_cli("synthetic://c2?records=%d" % n, cols, P)
    _check_cli("synthetic://c2?records=%d" % n, cols, P, extra="kta.batch=8192")       # several staging batches
    path = str(tmp_path / "c2.dump")
    w = _cli("-t", "t", "-b", "synthetic://c2?records=%d" % n, "-c", "--librdkafka", "kta.write_dump=" + path)
    assert w.returncode == 0, w.stderr
    _check_cli("dump://" + path, cols, P, extra="kta.batch=8192")
    # after the partitioner section, before the filter section
    both = _cli("-t", "t", "-b", "synthetic://c2?records=%d" % n, "-c", "--librdkafka", "kta.partitioner=murmur2,kta.compaction=1,kta.from=0")
    assert both.returncode == 0, both.stderr
    assert both.stdout.index("Partitioner check:") < both.stdout.index("Compaction what-if:") < both.stdout.index("Record filter:")
    taken = F.take(cols, np.nonzero(F.passes(cols["partition"], cols["ts_ms"], P, 0, None))[0], with_seq=True)     # (no timestamp: not in the window)
    assert len(taken["partition"]) < n
    assert _split(both.stdout)[1].startswith(CP.section(CP.vector(taken, P, taken["seq"]), CP.counters(taken, P), P))


def test_cli_section_on_raw_kafka_log_segments(tmp_path):
    P = 2
    blobs, cols = _segments(P)
    files = []
    for blob, p in blobs:
        path = tmp_path / ("%020d.%d.log" % (0, p))
        path.write_bytes(blob)
        files.append(str(path))
    _check_cli("segment://" + ",".join(files), cols, P)

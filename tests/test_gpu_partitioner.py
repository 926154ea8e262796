"""GPU tests of the partitioner pass (KTA_FLAG_PARTITIONER: Kafka's murmur2 of every keyed record, the records on the
partition the Java default partitioner gives their key and the what-if spread over Q partitions; no reference counterpart),
the vector bit-exact against the independent restatement in tests/partitioner_py.py:

    random columns           null and empty keys, tombstones, bad partitions, key lengths 0..300, half of the keyed records
                             placed by murmur2, Q in {1, 6, 7, 1000}: the staging ring, kta_handle_message,
                             kta_replay_messages, raw and tile-compact device batches, views; the counters identical to a
                             context without the flag; which == 2 touches nothing
    small shapes             n around the wave, the step and the tile; the last key ends key_bytes
    limits                   P = Q = the limit; limit + 1 refused; kta_set_repartition after a batch refused, after kta_reset not
    contention               one key 2^22 times (P = Q = 1 and 256), two keys alternating, 2^22 distinct 16-byte keys
    behaviour                a batch without key columns refused, kta_reset, the calls of a context without the flag
    with -c                  which == 3: the fused pass still taken, the alive count the oracle's; every opt-in at once
    the Kafka decode         raw log segments, zero-copy keys
    kta_exchange             the RCCL test double, 2 and 3 ranks, with and without -c
    kta-analyzer             kta.partitioner=murmur2 on segment:// (placed by murmur2, and a fifth moved), synthetic:// with
                             kta.repartition, kta.per_message=1 and kta.gpus=2; nothing changes without the key"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import hot_keys_py as HK
import kafka_format as KF
import key_sketch_py as KS
import partitioner_py as R
import timeline_py as T
import ts_order_py as TS
from helpers import NOW, random_cols
from oracle_c import Oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
LIMIT = 4096


def _cols(seed, n=60000, P=6, key_space=9000):
    """random_cols with damaged and out-of-range partitions, about half of the keyed records moved to murmur2 % P."""
    rng = np.random.default_rng(seed)
    cols = random_cols(rng, n, P, key_space=key_space, null_key=0.15, empty_key=0.05, tomb=0.3, max_key=300)
    h = R.hashes(cols)
    move = (rng.random(n) < 0.5) & (cols["key_len"] >= 0)
    cols["partition"][move] = ((h[move] & np.uint32(0x7FFFFFFF)) % np.uint32(P)).astype(np.int32)
    cols["partition"][rng.random(n) < 0.02] = -1            # a damaged batch's records
    cols["partition"][rng.random(n) < 0.02] = P + 3          # out of range
    return cols, h


@pytest.fixture(scope="module")
def topic():
    """The 60 000 records of the entry-path tests, their hashes and their vectors for every Q, computed once."""
    P = 6
    cols, h = _cols(1)
    return {"P": P, "cols": cols, "h": h, "want": {Q: R.vector(cols, P, Q, h=h) for Q in (1, 6, 7, 1000)}}


def _submit(h, cols):
    h.submit_columns(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"], cols["key_off"], cols["key_bytes"])


def _identities(v, counters):
    assert np.array_equal(v["checked"], counters[:, N.KTA_C_KEY_NON_NULL])
    assert int(v["target_records"].sum()) == int(v["checked"].sum())
    assert (v["placed"] <= v["checked"]).all()


def test_the_input_exercises_every_path(topic):
    cols, h, P = topic["cols"], topic["h"], topic["P"]
    keyed = (cols["key_len"] >= 0) & (cols["partition"] >= 0) & (cols["partition"] < P)
    kl = cols["key_len"][keyed]
    assert {int(x) for x in np.unique(kl % 4)} == {0, 1, 2, 3} and (kl > 16).any() and (kl == 0).any() and kl.max() > 250
    assert (h[keyed] >> np.uint32(31)).any() and not (h[keyed] >> np.uint32(31)).all()
    assert (cols["key_len"] < 0).any() and (cols["val_len"] < 0).any()
    assert (cols["partition"] == -1).any() and (cols["partition"] == P + 3).any()
    v = kta.split_partitioner(topic["want"][6], P, 6)
    assert 0 < int(v["placed"].sum()) < int(v["checked"].sum()) and (v["placed"] > 0).all()


@pytest.mark.parametrize("Q", [1, 6, 7, 1000])
def test_staging_ring_in_several_batches_bit_exact_and_counters_unchanged(topic, Q):
    P, cols, want = topic["P"], topic["cols"], topic["want"][Q]
    with kta.HipMetricHandler(P, now=NOW, batch_capacity=1 << 13, key_bytes_capacity=1 << 17, partitioner=True,
                              repartition=None if Q == P else Q) as h, \
            kta.HipMetricHandler(P, now=NOW, batch_capacity=1 << 13) as plain:
        for x in (h, plain):
            _submit(x, cols)
        got = h.partitioner()
        assert np.array_equal(got["vector"], want)
        res, c = h.finish(allow_bad_partition=True)
        res0, c0 = plain.finish(allow_bad_partition=True)
        assert np.array_equal(c, c0) and bytes(res) == bytes(res0)
        _identities(got, c)
        assert np.array_equal(h.exchange_partitioner()["vector"], want)
        info = h.partitioner_info()
        assert info["keyed_records"] == int(got["checked"].sum()) and info["launches"] >= 8
        assert 0 < info["partition_adds"] <= info["keyed_records"] and 0 < info["target_adds"] <= info["keyed_records"]
        if Q == 1:
            assert info["target_adds"] * 16 < info["keyed_records"]      # one target: a wave's lanes add as one or two groups


def test_handle_message_and_replay_messages(topic):
    P, cols = topic["P"], topic["cols"]
    sub = {k: v[:3000] for k, v in cols.items() if k != "key_bytes"}
    sub["key_bytes"] = cols["key_bytes"]
    want_sub = R.vector(sub, P, 7, h=topic["h"][:3000])
    with kta.HipMetricHandler(P, now=NOW, batch_capacity=1 << 10, partitioner=True, repartition=7) as h:
        kb = cols["key_bytes"].tobytes()
        for i in range(3000):
            kl = int(cols["key_len"][i])
            key = None if kl < 0 else kb[int(cols["key_off"][i]):int(cols["key_off"][i]) + kl]
            h.handle_message(kta.Message(int(cols["partition"][i]), int(cols["ts_ms"][i]), key, int(cols["val_len"][i])))
        assert np.array_equal(h.partitioner()["vector"], want_sub)
        h.reset()
        assert not h.partitioner()["vector"].any()
        h.replay_messages(cols)
        assert np.array_equal(h.partitioner()["vector"], topic["want"][7])           # (kta_reset kept Q)


def test_tile_compact_device_batch_views_and_which_2(topic):
    P, cols, want = topic["P"], topic["cols"], topic["want"][6]
    with kta.HipMetricHandler(P, now=NOW, partitioner=True) as h:
        b, n = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, n, 0, which=1)
        assert np.array_equal(h.partitioner()["vector"], want)
        h.reset()
        cut = 1000 + 36                                     # (a view's columns stay 16-byte aligned)
        for lo, hi in ((0, cut), (cut, 2 * 1024 + 4), (2 * 1024 + 4, n)):
            v = N.KtaBatch()
            v.partition, v.key_len, v.val_len = b.partition + 4 * lo, b.key_len + 4 * lo, b.val_len + 4 * lo
            v.ts_ms, v.key_off, v.key_bytes = b.ts_ms + 8 * lo, b.key_off + 4 * lo, b.key_bytes
            h.submit_device(v, hi - lo, 0, which=1)
        assert np.array_equal(h.partitioner()["vector"], want)
        h.reset()
        h.submit_device(b, n, 0, which=2)                   # the alive-key handler alone: not the pass's records
        assert not h.partitioner()["vector"].any()
        h.sync()
        h.device_batch_free(b)
    # a view into a KEYLESS allocation (u16 lengths in its tiles) with key columns of the caller's own
    with kta.HipMetricHandler(P, now=NOW, partitioner=True, repartition=7) as h:
        small = {k: (v.copy() if k == "key_bytes" else v[:20000].copy()) for k, v in cols.items()}
        small["val_len"] = np.minimum(small["val_len"], 60000).astype(np.int32)
        keyless, n = h.upload_batch(small, with_keys=False)
        keyed, _ = h.upload_batch(small, with_keys=True)
        lo = 1024 + 512 + 4
        v = N.KtaBatch()
        v.partition, v.key_len, v.val_len = keyless.partition + 4 * lo, keyless.key_len + 4 * lo, keyless.val_len + 4 * lo
        v.ts_ms, v.key_off, v.key_bytes = keyless.ts_ms + 8 * lo, keyed.key_off + 4 * lo, keyed.key_bytes
        h.submit_device(v, n - lo, 0, which=1)
        tail = {k: (x if k == "key_bytes" else x[lo:]) for k, x in small.items()}
        assert np.array_equal(h.partitioner()["vector"], R.vector(tail, P, 7, h=topic["h"][lo:20000]))
        h.sync()
        h.device_batch_free(keyless)
        h.device_batch_free(keyed)


def test_raw_layout_device_batch(topic):
    import torch
    P, cols = topic["P"], topic["cols"]
    dev = {k: torch.from_numpy(np.ascontiguousarray(cols[k])).cuda() for k in ("partition", "key_len", "val_len", "ts_ms")}
    dev["key_off"] = torch.from_numpy(cols["key_off"].view(np.int32)).cuda()
    kb = np.zeros(len(cols["key_bytes"]) + 16, np.uint8)     # readable 16 bytes past the last key
    kb[:len(cols["key_bytes"])] = cols["key_bytes"]
    dev["key_bytes"] = torch.from_numpy(kb).cuda()
    torch.cuda.synchronize()
    b = N.KtaBatch()
    for k, t in dev.items():
        setattr(b, k, t.data_ptr())
    with kta.HipMetricHandler(P, now=NOW, partitioner=True, repartition=1000) as h:
        h.submit_device(b, len(cols["partition"]), 0, which=1)
        assert np.array_equal(h.partitioner()["vector"], topic["want"][1000])
        h.sync()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 257, 1023, 1025])
def test_small_shapes_the_last_key_ends_key_bytes(n):
    P, Q = 3, 5
    rng = np.random.default_rng(100 + n)
    cols = random_cols(rng, max(n, 1), P, key_space=50, null_key=0.1, empty_key=0.1, max_key=23)
    cols = {k: (v if k == "key_bytes" else v[:n]) for k, v in cols.items()}
    if n:
        kb = cols["key_bytes"].tobytes() + b"seven b"       # the last record's key, 7 bytes, ends the blob
        cols["key_off"][n - 1], cols["key_len"][n - 1], cols["partition"][n - 1] = len(kb) - 7, 7, 1
        cols["key_bytes"] = np.frombuffer(kb, np.uint8)
    want = R.vector(cols, P, Q) if n else np.zeros(R.words(P, Q), np.uint64)
    with kta.HipMetricHandler(P, now=NOW, partitioner=True, repartition=Q) as h:
        if n:
            b, nb = h.upload_batch(cols, with_keys=True)
            h.submit_device(b, nb, 0, which=1)
        got = h.partitioner()
        assert np.array_equal(got["vector"], want)
        _identities(got, h.finish()[1])
        h.sync()
        if n:
            h.device_batch_free(b)


def test_limits():
    assert kta.partitioner_max_partitions() == LIMIT
    rng = np.random.default_rng(7)
    cols = random_cols(rng, 20000, LIMIT, key_space=5000, null_key=0.1, max_key=40)
    with kta.HipMetricHandler(LIMIT, now=NOW, partitioner=True) as h:
        assert h.partitioner_info()["lds_bytes"] == 20 * LIMIT
        b, n = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, n, 0, which=1)
        got = h.partitioner()
        assert np.array_equal(got["vector"], R.vector(cols, LIMIT, LIMIT))
        _identities(got, h.finish()[1])
        with pytest.raises(kta.KtaError, match="handed records"):
            h.set_repartition(5)
        assert np.array_equal(h.partitioner()["vector"], got["vector"])
        h.reset()
        with pytest.raises(kta.KtaError, match=r"\[1, %d\]" % LIMIT):
            h.set_repartition(LIMIT + 1)
        with pytest.raises(kta.KtaError):
            h.set_repartition(0)
        h.set_repartition(5)
        h.submit_device(b, n, 0, which=1)
        assert np.array_equal(h.partitioner()["vector"], R.vector(cols, LIMIT, 5))
        h.sync()
        h.device_batch_free(b)
    with pytest.raises(kta.KtaError, match="KTA_FLAG_PARTITIONER admits at most %d" % LIMIT):
        kta.HipMetricHandler(LIMIT + 1, now=NOW, partitioner=True)
    with pytest.raises(kta.KtaError):
        kta.HipMetricHandler(4, now=NOW, partitioner=True, repartition=LIMIT + 1)
    # a mid-sized plan: 1024-thread workgroups, two to a CU
    cols = random_cols(rng, 30000, 700, key_space=5000, null_key=0.1, max_key=40)
    with kta.HipMetricHandler(700, now=NOW, partitioner=True, repartition=3000) as h:
        b, n = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, n, 0, which=1)
        assert np.array_equal(h.partitioner()["vector"], R.vector(cols, 700, 3000))
        h.sync()
        h.device_batch_free(b)


def _repeat_keys(keys, parts, n, val_len=10):
    """n records cycling through `keys` (16 bytes each) lane by lane."""
    k = len(keys)
    blob = np.frombuffer(b"".join(keys), np.uint8)
    i = np.arange(n) % k
    return {"partition": np.asarray(parts, np.int32)[i], "key_len": np.full(n, 16, np.int32),
            "val_len": np.full(n, val_len, np.int32), "ts_ms": np.full(n, 1_600_000_000_000, np.int64),
            "key_off": (16 * i).astype(np.uint32), "key_bytes": blob}


def _expect_repeated(keys, parts, n, P, Q, val_len=10):
    v = np.zeros(R.words(P, Q), np.uint64)
    for j, (k, p) in enumerate(zip(keys, parts)):
        cnt = n // len(keys) + (1 if j < n % len(keys) else 0)
        t = R.to_positive(R.murmur2(k))
        v[2 * p] += cnt
        v[2 * p + 1] += cnt * (t % P == p)
        v[2 * P + 2 * (t % Q)] += cnt
        v[2 * P + 2 * (t % Q) + 1] += cnt * (16 + val_len)
    return v


@pytest.mark.parametrize("P,Q", [(1, 1), (256, 256)])
def test_contention_one_key(P, Q):
    n = 1 << 22
    key = b"the one hot key!"
    p = R.to_positive(R.murmur2(key)) % P
    with kta.HipMetricHandler(P, now=NOW, partitioner=True, repartition=None if Q == P else Q) as h:
        b, nb = h.upload_batch(_repeat_keys([key], [p], n), with_keys=True)
        h.submit_device(b, nb, 0, which=1)
        got = h.partitioner()
        assert np.array_equal(got["vector"], _expect_repeated([key], [p], n, P, Q))
        assert int(got["placed"][p]) == n
        info = h.partitioner_info()
        assert info["keyed_records"] == n and info["partition_adds"] == n // 64 and info["target_adds"] == n // 64
        h.sync()
        h.device_batch_free(b)


def test_contention_two_keys_alternating_lane_by_lane():
    n, P, Q = 1 << 22, 5, 9
    keys = [b"key number one ..", b"key number two .."]
    keys = [k[:16] for k in keys]
    parts = [R.to_positive(R.murmur2(keys[0])) % P, (R.to_positive(R.murmur2(keys[1])) + 1) % P]   # one placed, one not
    with kta.HipMetricHandler(P, now=NOW, partitioner=True, repartition=Q) as h:
        b, nb = h.upload_batch(_repeat_keys(keys, parts, n), with_keys=True)
        h.submit_device(b, nb, 0, which=1)
        got = h.partitioner()
        assert np.array_equal(got["vector"], _expect_repeated(keys, parts, n, P, Q))
        assert int(got["placed"].sum()) == n // 2
        info = h.partitioner_info()
        assert info["partition_adds"] <= n // 32 and info["target_adds"] <= n // 32       # two groups per instruction
        h.sync()
        h.device_batch_free(b)


def test_2e22_distinct_16_byte_keys_the_interleaved_path():
    sp, _ = kta.synth_preset("c3")
    sp.n_distinct_keys, sp.key_null_permille, sp.key_empty_permille = 0, 0, 0
    n, P, Q = 1 << 22, int(sp.n_partitions), 48
    cols = kta.synth_fill_host(sp, 0, n, with_keys=True)
    assert (cols["key_len"] == 16).all()
    want = R.vector(cols, P, Q)
    with kta.HipMetricHandler(P, now=NOW, partitioner=True, repartition=Q) as h:
        b, nb = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, nb, 0, which=1)
        got = h.partitioner()
        assert np.array_equal(got["vector"], want)
        assert int(got["checked"].sum()) == n and (got["target_records"] > 0).all()
        h.sync()
        h.device_batch_free(b)


def test_refusal_reset_and_calls_without_the_flag():
    P = 4
    cols, _ = _cols(3, n=5000, P=P)
    with kta.HipMetricHandler(P, now=NOW, partitioner=True) as h:
        b, n = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, n, 0, which=1)
        v0, c0 = h.partitioner()["vector"], h.finish(allow_bad_partition=True)[1]
        assert v0.any()
        nokeys = N.KtaBatch()
        nokeys.partition, nokeys.key_len, nokeys.val_len, nokeys.ts_ms = b.partition, b.key_len, b.val_len, b.ts_ms
        for which in (1, 3):
            with pytest.raises(kta.KtaError, match=r"key columns missing \(KTA_FLAG_PARTITIONER\)"):
                h.submit_device(nokeys, n, 0, which=which)
        assert np.array_equal(h.partitioner()["vector"], v0) and np.array_equal(h.finish(allow_bad_partition=True)[1], c0)
        h.reset()
        assert not h.partitioner()["vector"].any()
        h.finish(allow_bad_partition=True)
        assert not h.exchange_partitioner()["vector"].any()
        with pytest.raises(kta.KtaError):
            h.replay_messages({k: v for k, v in cols.items() if k not in ("key_off", "key_bytes")})
        h.sync()
        h.device_batch_free(b)
    with kta.HipMetricHandler(P, now=NOW) as h:
        for fn in (h.partitioner, h.exchange_partitioner, h.partitioner_result_vector, h.partitioner_info,
                   lambda: h.set_repartition(3)):
            with pytest.raises(kta.KtaError, match="KTA_FLAG_PARTITIONER"):
                fn()


def test_with_c_the_fused_pass_is_still_taken_and_every_opt_in_at_once():
    sp, _ = kta.synth_preset("c3")
    n, P = 1 << 21, 64
    cols = kta.synth_fill_host(sp, 0, n, with_keys=True)
    o = Oracle(NOW, count_alive_keys=True)
    o.run_soa(cols)
    want = R.vector(cols, P, 100)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, partitioner=True, repartition=100) as h:
        b, nb = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, nb, 0, which=3)
        res, c = h.finish()
        info = h.alive_pass_info()
        assert info["fused"] > 0 and info["scanned"] == 0
        assert np.array_equal(c, o.counters(P)) and res.alive_keys == o.alive_keys()
        assert np.array_equal(h.exchange_partitioner()["vector"], want)
        h.sync()
        h.device_batch_free(b)
    tl = (int(sp.ts_base_ms), 1_000, 40)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, batch_capacity=1 << 20, key_bytes_capacity=1 << 25,
                              analytics=True, timeline=tl, key_sketch=True, hot_keys=True, ts_order=True, partitioner=True,
                              repartition=100) as h:
        _submit(h, cols)
        res, c = h.finish()
        assert np.array_equal(c, o.counters(P)) and res.alive_keys == o.alive_keys()
        assert np.array_equal(h.exchange_partitioner()["vector"], want)
        assert np.array_equal(h.exchange_key_sketch(), KS.sketch(cols, P))
        assert np.array_equal(h.exchange_timeline(), T.timeline_vector(cols, P, *tl))
        assert np.array_equal(h.exchange_ts_order()["vector"], TS.vector_of(P, cols["partition"], cols["ts_ms"]))
        assert np.array_equal(h.exchange_hot_keys().reshape(-1), np.asarray(HK.vector(cols, P)).reshape(-1))


def test_kafka_decode_zero_copy_keys():
    from kafka_cases import random_record_set
    lib = N.load()
    rng = np.random.default_rng(42)
    P, Q = 4, 9
    blobs, recs = [], []
    for fetch in range(6):
        part = fetch % P
        blob, (pl, klen, vlen, ts, keys), _ = random_record_set(rng, 50, partition=part, key_space=300, with_noise=False)
        blobs.append((blob, part))
        recs += [(part, k, v) for k, v in zip(keys, vlen)]
    want = np.zeros(R.words(P, Q), np.uint64)
    for p, k, v in recs:
        if k is None:
            continue
        t = R.to_positive(R.murmur2(bytes(k)))
        want[2 * p] += 1
        want[2 * p + 1] += t % P == p
        want[2 * P + 2 * (t % Q)] += 1
        want[2 * P + 2 * (t % Q) + 1] += len(k) + max(int(v), 0)
    assert want[1:2 * P:2].any()
    with kta.HipMetricHandler(P, now=NOW, partitioner=True, repartition=Q) as h:
        for blob, part in blobs:
            st = N.KtaKafkaIndexStats()
            h._check(lib.kta_kafka_consume(h._ctx, blob, len(blob), part, C.byref(st)))
        assert np.array_equal(h.partitioner()["vector"], want)


# ------------------------------------------------------------------------------------------ kta_exchange, test double
@pytest.fixture(scope="module")
def mock_rccl(tmp_path_factory):
    lib = tmp_path_factory.mktemp("mock") / "libmock_rccl.so"
    r = subprocess.run(["timeout", "-k", "10", "600", "/opt/rocm/bin/hipcc", "-O1", "-shared", "-fPIC", "-std=c++17",
                        os.path.join(ROOT, "tests", "mock_rccl.cpp"), "-o", str(lib), "-lrt", "-lpthread"],
                       capture_output=True, text=True, timeout=660)
    assert r.returncode == 0, r.stderr[-2000:]
    return str(lib)


_EXCHANGE_WORKER = r'''
import os, sys, threading
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import kafka_topic_analyzer_amd as kta
import partitioner_py as R
from helpers import NOW, random_cols

P, Q = 7, 11
rng = np.random.default_rng(31)
cols = random_cols(rng, 80000, P, key_space=20000, tomb=0.3, max_key=64)
n = len(cols["partition"])
cols["seq"] = np.arange(n, dtype=np.uint64)
half = n // 2
hashes = R.hashes(cols)

def subset(idx):
    kl = np.maximum(cols["key_len"][idx], 0).astype(np.int64)
    off = np.zeros(len(idx), np.int64)
    off[1:] = np.cumsum(kl)[:-1]
    kb = np.zeros(max(int(kl.sum()), 1), np.uint8)
    src = cols["key_off"][idx].astype(np.int64)
    for j in np.nonzero(kl)[0]:
        kb[off[j]:off[j] + kl[j]] = cols["key_bytes"][src[j]:src[j] + kl[j]]
    return {"partition": cols["partition"][idx], "key_len": cols["key_len"][idx], "val_len": cols["val_len"][idx],
            "ts_ms": cols["ts_ms"][idx], "key_off": off.astype(np.uint32), "key_bytes": kb[:max(int(kl.sum()), 1)],
            "seq": cols["seq"][idx]}

vec = lambda idx: R.vector({k: (v if k == "key_bytes" else v[idx]) for k, v in cols.items()}, P, Q, h=hashes[idx])
want = {"first": vec(np.arange(half)), "all": vec(np.arange(n))}

for nranks in (2, 3):
    for with_c in (False, True):
        uid = kta.HipMetricHandler.comm_unique_id()
        errors = []
        def run(rank):
            try:
                h = kta.HipMetricHandler(P, count_alive_keys=with_c, now=NOW, seq_column=with_c, partitioner=True, repartition=Q)
                h.comm_create(nranks, rank, uid)
                mine = cols["partition"] % nranks == rank
                for stage, idx in (("first", np.arange(half)[mine[:half]]), ("all", np.arange(half, n)[mine[half:]])):
                    sh = subset(idx)
                    if not with_c:
                        del sh["seq"]
                    b, nb = h.upload_batch(sh, with_keys=True)
                    h.submit_device(b, nb, 0)
                    h.exchange()
                    assert np.array_equal(h.exchange_partitioner()["vector"], want[stage]), (nranks, with_c, rank, stage, "exchanged")
                    own = np.nonzero(mine[:half if stage == "first" else n])[0]
                    assert np.array_equal(h.partitioner()["vector"], vec(own)), (nranks, with_c, rank, stage, "own")
                    h.exchange()
                    assert np.array_equal(h.exchange_partitioner()["vector"], want[stage]), (nranks, with_c, rank, stage, "again")
                    h.sync()
                    h.device_batch_free(b)
                h.comm_destroy(); h.close()
            except BaseException as e:
                errors.append((rank, repr(e)))
                print("rank %d: %r" % (rank, e), file=sys.stderr, flush=True)
                os._exit(2)        # the other ranks would wait in their collectives for ever
        ts = [threading.Thread(target=run, args=(r,)) for r in range(nranks)]
        [t.start() for t in ts]; [t.join() for t in ts]
        assert not errors, errors
        print("ranks", nranks, "-c" if with_c else "", "OK", flush=True)
print("OK")
'''


def test_exchange_partitioner_on_two_and_three_ranks_with_and_without_c(tmp_path, mock_rccl):
    script = tmp_path / "exchange_worker.py"
    script.write_text(_EXCHANGE_WORKER)
    env = dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(script), ROOT], capture_output=True, text=True,
                       timeout=330, env=env)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count(" OK") == 4


# ------------------------------------------------------------------------------------------ the CLI
def _cli(*args, env=None, cwd=None):
    return subprocess.run(["timeout", "-k", "10", "240", CLI, *args], capture_output=True, text=True, timeout=270,
                          env=env, cwd=cwd)


def _normalise(text):
    text = re.sub(r"Scanning took: \d+ seconds", "Scanning took: 3 seconds", text)
    return re.sub(r"Estimated Msg/s: \d+", "Estimated Msg/s: 133", text)


def _split(stdout):
    at = stdout.index("Partitioner check:")
    return stdout[:at], stdout[at:]


def _segment_files(tmp_path, P, moved):
    """A test producer that places keyed records by murmur2 (file k is partition k); `moved`: every fifth keyed record goes
    to the next partition instead.  -> (files, [(partition, key | None, value length | None)])"""
    rng = np.random.default_rng(8)
    per = [[] for _ in range(P)]
    keyed = 0
    for i in range(600):
        key = None if i % 11 == 0 else (b"" if i % 53 == 0 else b"user-%d" % int(rng.integers(0, 150)))
        val = None if i % 7 == 0 else bytes(int(rng.integers(0, 300)))
        if key is None:
            p = i % P
        else:
            p = R.to_positive(R.murmur2(key)) % P
            keyed += 1
            if moved and keyed % 5 == 0:
                p = (p + 1) % P
        per[p].append((i, key, val, []))
    files, recs = [], []
    for p in range(P):
        blob = b""
        for lo in range(0, len(per[p]), 40):
            blob += KF.encode_batch(lo, per[p][lo:lo + 40], 1_600_000_000_000)
        path = tmp_path / ("%s%020d.log" % ("m" if moved else "p", p))
        path.write_bytes(blob)
        files.append(str(path))
        recs += [(p, k, None if v is None else len(v)) for _, k, v, _ in per[p]]
    return files, recs


def _recs_cols(recs):
    blob, off = b"", []
    for _, k, _ in recs:
        off.append(len(blob))
        blob += k or b""
    return {"partition": np.array([r[0] for r in recs], np.int32),
            "key_len": np.array([-1 if r[1] is None else len(r[1]) for r in recs], np.int32),
            "val_len": np.array([-1 if r[2] is None else r[2] for r in recs], np.int32), "key_off": np.array(off, np.uint32),
            "key_bytes": np.frombuffer(blob + b"\0", np.uint8)}


@pytest.mark.parametrize("moved", [False, True])
def test_cli_section_on_raw_kafka_log_segments(tmp_path, moved):
    P = 4
    files, recs = _segment_files(tmp_path, P, moved)
    cols = _recs_cols(recs)
    want = R.section(R.vector(cols, P, P), R.counters(cols, P), P, P)
    r = _cli("-t", "seg", "-b", "segment://" + ",".join(files), "--librdkafka", "kta.partitioner=murmur2")
    assert r.returncode == 0, r.stderr
    report, section = _split(r.stdout)
    assert section == want
    if moved:
        assert "80." in section and "only partly keyed" in section
    else:
        assert "All keyed records lie on murmur2's partition" in section
    plain = _cli("-t", "seg", "-b", "segment://" + ",".join(files))
    assert plain.returncode == 0 and _normalise(plain.stdout) == _normalise(report) and "Partitioner" not in plain.stdout


def test_cli_section_single_sharded_per_message_and_nothing_without_the_key(mock_rccl):
    src = "synthetic://c2?records=250000"
    sp, _ = kta.synth_preset("c2")
    cols = kta.synth_fill_host(sp, 0, 250000, with_keys=True)
    P, Q = int(sp.n_partitions), 12
    want = R.section(R.vector(cols, P, Q), R.counters(cols, P), P, Q)
    knobs = "kta.partitioner=murmur2,kta.repartition=12"
    plain = _cli("-t", "c2", "-b", src)
    assert plain.returncode == 0 and "Partitioner" not in plain.stdout and "murmur2" not in plain.stdout, plain.stderr
    one = _cli("-t", "c2", "-b", src, "--librdkafka", knobs)
    assert one.returncode == 0, one.stderr
    report, section = _split(one.stdout)
    assert section == want and _normalise(report) == _normalise(plain.stdout)
    same_q = _cli("-t", "c2", "-b", src, "--librdkafka", "kta.partitioner=murmur2")
    assert same_q.returncode == 0 and _split(same_q.stdout)[1] == R.section(R.vector(cols, P, P), R.counters(cols, P), P, P)
    # after every other section, the hot keys included; those print what they print without the key
    others = "kta.analytics=1,kta.timeline=1h,kta.distinct_keys=1,kta.ts_order=1,kta.hot_keys=5"
    without = _cli("-t", "c2", "-b", src, "--librdkafka", others)
    both = _cli("-t", "c2", "-b", src, "--librdkafka", others + "," + knobs)
    assert without.returncode == 0 and both.returncode == 0, both.stderr
    rep2, sec2 = _split(both.stdout)
    assert sec2 == want and _normalise(rep2) == _normalise(without.stdout) and "Hot keys" in rep2
    env = dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl)
    for c in ([], ["-c"]):
        many = _cli("-t", "c2", "-b", src, *c, "--librdkafka", knobs + ",kta.gpus=2,kta.batch=32768,kta.oversubscribe=1", env=env)
        assert many.returncode == 0, (c, many.stderr[-2000:])
        assert many.stdout.count("Partitioner check:") == 1 and _split(many.stdout)[1] == want, c
    pm = _cli("-t", "c2", "-b", src, "--librdkafka", knobs + ",kta.per_message=1,kta.batch=4096")
    assert pm.returncode == 0, pm.stderr
    assert _split(pm.stdout)[1] == want

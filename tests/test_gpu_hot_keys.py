"""GPU tests of the hot-key sketch (KTA_FLAG_HOT_KEYS: a topic-wide vector of sums that names the heaviest keys; no
reference counterpart), every vector bit-exact against the independent numpy restatement in tests/hot_keys_py.py:

    random columns           null and empty keys, tombstones, bad partitions, key lengths 0..300: the staging ring,
                             kta_handle_message, kta_replay_messages, raw and tile-compact device batches, views cut
                             inside a tile, which = 2; the counters identical to a context without the flag
    planted keys             2^20 records, keys at 10 %, 3 % and 1 % (one of 40 bytes, one empty) over 200 000 others:
                             reported, within their bounds, with their bytes as exemplars
    contention, overflow     one key 2^26 times; two keys alternating lane by lane, 2^24 records, every workgroup of the
                             large launches flushing its LDS counters mid-stream
    behaviour                a batch without key columns refused, kta_reset, the calls of a context without the flag
    composition              -c with which == 3: the fused pass still taken, the alive count the oracle's; all five
                             opt-ins at once
    the Kafka decode         raw log segments, zero-copy keys
    kta_exchange             the RCCL test double, 2 and 3 ranks, with and without -c, exchanged twice
    kta-analyzer             kta.hot_keys=K on synthetic://, kta.gpus=2, kta.per_message=1 and segment://"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import hot_keys_py as H
import key_sketch_py as K
import timeline_py as T
from helpers import NOW, random_cols
from oracle_c import Oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")


def _cols(seed, n=60000, P=6):
    rng = np.random.default_rng(seed)
    cols = random_cols(rng, n, P, key_space=9000, null_key=0.15, empty_key=0.05, tomb=0.3, max_key=300)
    cols["partition"][rng.random(n) < 0.02] = -1            # a damaged batch's records
    cols["partition"][rng.random(n) < 0.02] = P + 3          # out of range
    return cols


def _n_keyed(cols, P):
    return int(((cols["partition"] >= 0) & (cols["partition"] < P) & (cols["key_len"] >= 0)).sum())


def _pack(keys):
    """(key_len, key_off, key_bytes) columns of a list of keys (None: a null key)."""
    kl = np.array([-1 if k is None else len(k) for k in keys], np.int32)
    lens = np.maximum(kl, 0).astype(np.int64)
    off = np.zeros(len(keys), np.int64)
    off[1:] = np.cumsum(lens)[:-1]
    kb = np.frombuffer(b"".join(k or b"" for k in keys) + b"\0", np.uint8)
    return kl, off.astype(np.uint32), kb


def test_random_columns_every_entry_path_bit_exact():
    P = 6
    cols = _cols(1)
    assert set(np.unique(cols["key_len"] % 16)) > {0, 1, 3} and cols["key_len"].max() > 250
    want = H.vector(cols, P)
    keyed = _n_keyed(cols, P)
    assert int(want[0, :, 0].sum()) == int(want[1, :, 0].sum()) == keyed and keyed > 40000
    # the staging ring (several batches), against a context without the flag fed the same records
    with kta.HipMetricHandler(P, now=NOW, batch_capacity=1 << 13, key_bytes_capacity=1 << 17, hot_keys=True) as h, \
            kta.HipMetricHandler(P, now=NOW, batch_capacity=1 << 13) as plain:
        for x in (h, plain):
            x.submit_columns(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"], cols["key_off"],
                             cols["key_bytes"])
        assert np.array_equal(h.hot_keys(), want)
        res, c = h.finish(allow_bad_partition=True)
        res0, c0 = plain.finish(allow_bad_partition=True)
        assert np.array_equal(c, c0) and bytes(res) == bytes(res0)
        assert np.array_equal(h.exchange_hot_keys(), want)
        info = h.hot_keys_info()
        assert info["keyed"] == keyed and info["launches"] >= 8 and 0 < info["groups"] <= keyed
        assert kta.recover_hot_keys(h.exchange_hot_keys(), 10) == H.recover(want, 10)
    # kta_handle_message (one message at a time) and kta_replay_messages
    sub = {k: v[:3000] for k, v in cols.items() if k != "key_bytes"}
    sub["key_bytes"] = cols["key_bytes"]
    want_sub = H.vector(sub, P)
    with kta.HipMetricHandler(P, now=NOW, batch_capacity=1 << 10, hot_keys=True) as h:
        kb = cols["key_bytes"].tobytes()
        for i in range(3000):
            kl = int(cols["key_len"][i])
            key = None if kl < 0 else kb[int(cols["key_off"][i]):int(cols["key_off"][i]) + kl]
            h.handle_message(kta.Message(int(cols["partition"][i]), int(cols["ts_ms"][i]), key, int(cols["val_len"][i])))
        assert np.array_equal(h.hot_keys(), want_sub)
        h.reset()
        assert not h.hot_keys().any()
        h.replay_messages(cols)
        assert np.array_equal(h.hot_keys(), want)
    # tile-compact device batches, views cut inside a tile (which = 1 for the metrics handler alone)
    with kta.HipMetricHandler(P, now=NOW, hot_keys=True) as h:
        b, n = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, n, 0, which=1)
        assert np.array_equal(h.hot_keys(), want)
        h.reset()
        cut = 1000 + 36                                     # (a view's columns stay 16-byte aligned)
        for lo, hi in ((0, cut), (cut, 2 * 1024 + 4), (2 * 1024 + 4, n)):
            v = N.KtaBatch()
            v.partition, v.key_len, v.val_len = b.partition + 4 * lo, b.key_len + 4 * lo, b.val_len + 4 * lo
            v.ts_ms, v.key_off, v.key_bytes = b.ts_ms + 8 * lo, b.key_off + 4 * lo, b.key_bytes
            h.submit_device(v, hi - lo, 0, which=1)
        assert np.array_equal(h.hot_keys(), want)
        h.reset()
        h.submit_device(b, n, 0, which=2)                   # the alive-key handler alone: not the sketch's records
        assert not h.hot_keys().any() and h.hot_keys_info()["keyed"] == 0
        h.sync()
        h.device_batch_free(b)


def test_raw_layout_device_batch():
    import torch
    P = 6
    cols = _cols(2, n=40000)
    want = H.vector(cols, P)
    dev = {k: torch.from_numpy(np.ascontiguousarray(cols[k])).cuda() for k in ("partition", "key_len", "val_len", "ts_ms")}
    dev["key_off"] = torch.from_numpy(cols["key_off"].view(np.int32)).cuda()
    kb = np.zeros(len(cols["key_bytes"]) + 32, np.uint8)
    kb[:len(cols["key_bytes"])] = cols["key_bytes"]
    dev["key_bytes"] = torch.from_numpy(kb).cuda()
    torch.cuda.synchronize()
    b = N.KtaBatch()
    for k, t in dev.items():
        setattr(b, k, t.data_ptr())
    with kta.HipMetricHandler(P, now=NOW, hot_keys=True) as h:
        h.submit_device(b, len(cols["partition"]), 0, which=1)
        assert np.array_equal(h.hot_keys(), want)
        h.sync()


def _exemplar_of(table, key):
    """The bytes the table holds for `key` (None: no exemplar), looked up as the header says."""
    h = H.fnv1a(key)
    x = int(H.fmix32(np.array([h], np.uint64))[0])
    for at in (x & 1023, 1024 + ((x >> 10) & 1023)):
        e = table[at]
        if e["valid"] and int(e["hash"]) == h:
            return int(e["key_len"]), bytes(e["bytes"][:min(int(e["key_len"]), 32)])
    return None


def test_planted_keys_are_reported_with_bounds_and_exemplars():
    n, P = 1 << 20, 5
    rng = np.random.default_rng(12)
    planted = [b"a hot key of forty bytes: 0123456789abcdef"[:40], b"", b"third\\key\x01"]
    assert len(planted[0]) == 40
    background = [b"bg-%07d" % i for i in range(200_000)]
    which = rng.integers(0, len(background), size=n) + len(planted)
    r = rng.random(n)
    which[r < 0.10] = 0
    which[(r >= 0.10) & (r < 0.13)] = 1
    which[(r >= 0.13) & (r < 0.14)] = 2
    keys = planted + background
    kl_u, off_u, kb = _pack(keys)
    cols = {"partition": rng.integers(0, P, size=n).astype(np.int32), "key_len": kl_u[which], "key_off": off_u[which],
            "key_bytes": kb, "val_len": np.full(n, 10, np.int32), "ts_ms": np.full(n, 1_600_000_000_000, np.int64)}
    truth = {H.fnv1a(k): int((which == i).sum()) for i, k in enumerate(planted)}
    want = H.vector(cols, P)
    with kta.HipMetricHandler(P, now=NOW, hot_keys=True) as h:
        b, nb = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, nb, 0, which=1)
        got = h.hot_keys()
        table = h.hot_key_exemplars()
        info = h.hot_keys_info()
        h.sync()
        h.device_batch_free(b)
    assert np.array_equal(got, want) and info["keyed"] == n and info["launches"] == 5     # 2^16 .. 2^19, 2^16 left over
    found, keyed = kta.recover_hot_keys(got, 64)
    assert keyed == n and (found, keyed) == H.recover(want, 64)
    by_hash = {e[0]: e for e in found}
    for key in planted:
        hash_, upper, lower = by_hash[H.fnv1a(key)]
        assert lower <= truth[hash_] <= upper, (key, lower, truth[hash_], upper)
        assert _exemplar_of(table, key) == (len(key), key[:32]), key
    assert info["exemplars"] >= 3
    # every valid slot holds one record's key whose hash is the slot's
    data_hashes = {H.fnv1a(k) for k in planted} | set(int(v) for v in K.fnv_columns(kl_u, off_u, kb))
    valid = table[table["valid"] != 0]
    assert len(valid) >= 3
    for e in valid:
        assert int(e["hash"]) in data_hashes
        assert H.fnv1a(bytes(e["bytes"][:int(e["key_len"])])) == int(e["hash"]) or int(e["key_len"]) > 32
    text = kta.render_hot_keys(got, table, 3)
    assert text == H.section(want, 3, {H.fnv1a(k): k for k in planted})
    assert "a hot key of forty bytes: 012345..." in text and "third\\x5Ckey\\x01" in text


def _expected_flushes(n, period, cus):
    """Mid-stream flushes and workgroups of a batch of n records: launches of 2^16, 2^17, .. 2^26 records, at most one
    workgroup per CU, 4096 records per workgroup and round, a flush before every round that is a multiple of the period."""
    flushes = wgs = 0
    least = None
    slice_, at = 1 << 16, 0
    while at < n:
        take = min(slice_, n - at)
        steps = -(-take // 256)
        grid = min(-(-steps // 16), cus)
        rounds = -(-steps // (grid * 16))
        per_wg = (rounds - 1) // period
        flushes += grid * per_wg
        wgs += grid
        if take == 1 << 23:
            least = per_wg
        at += take
        slice_ = min(slice_ * 2, 1 << 26)
    return flushes, wgs, least


def test_contention_one_key_and_two_alternating_keys_with_flushes():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 1 << 26
    with kta.HipMetricHandler(3, now=NOW, hot_keys=True) as h:
        key = np.frombuffer(b"the one hot key!", np.uint8)
        cols = {"partition": np.full(n, 2, np.int32), "key_len": np.full(n, 16, np.int32),
                "val_len": np.full(n, 10, np.int32), "ts_ms": np.full(n, 1_600_000_000_000, np.int64),
                "key_off": np.zeros(n, np.uint32), "key_bytes": key}
        b, nb = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, nb, 0, which=1)
        want = H.vector_from_pairs([H.fnv1a(key.tobytes())], [n])
        assert np.array_equal(h.hot_keys(), want)
        info = h.hot_keys_info()
        assert info["keyed"] == n and info["groups"] < n // 32
        assert kta.recover_hot_keys(h.hot_keys(), 5) == ([(H.fnv1a(key.tobytes()), n, n)], n)
        assert _exemplar_of(h.hot_key_exemplars(), key.tobytes()) == (16, key.tobytes())
        h.sync()
        h.device_batch_free(b)
    # two keys alternating lane by lane, the LDS counters flushed every second round: every workgroup of the launch of
    # 2^23 records flushes at least twice before its end (sized from the packing: 4096 records per round, one workgroup
    # per CU)
    n, period = 1 << 24, 2
    two = [b"even lanes' key", b"odd lanes' key, longer than sixteen bytes"]
    kl_u, off_u, kb = _pack(two)
    lane = (np.arange(n) & 1).astype(np.int64)
    cols = {"partition": np.zeros(n, np.int32), "key_len": kl_u[lane], "key_off": off_u[lane], "key_bytes": kb,
            "val_len": np.full(n, 10, np.int32), "ts_ms": np.full(n, 1_600_000_000_000, np.int64)}
    with kta.HipMetricHandler(1, now=NOW, hot_keys=True) as h:
        h.set_hot_flush_rounds(period)
        b, nb = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, nb, 0, which=1)
        want = H.vector_from_pairs([H.fnv1a(k) for k in two], [n // 2, n // 2])
        assert np.array_equal(h.hot_keys(), want)
        info = h.hot_keys_info()
        flushes, wgs, least = _expected_flushes(n, period, cus)
        assert least is not None and least >= 2
        assert info["keyed"] == n and info["flushes"] == flushes and info["workgroups"] == wgs
        assert info["groups"] < n // 16                       # both keys' lanes add as one each
        with pytest.raises(kta.KtaError):
            h.set_hot_flush_rounds(512)
        h.sync()
        h.device_batch_free(b)


def test_refusal_reset_and_calls_without_the_flag():
    P = 4
    cols = _cols(3, n=5000, P=P)
    with kta.HipMetricHandler(P, now=NOW, hot_keys=True) as h:
        b, n = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, n, 0, which=1)
        v0, c0 = h.hot_keys(), h.finish(allow_bad_partition=True)[1]
        assert np.array_equal(v0, H.vector(cols, P))
        nokeys = N.KtaBatch()
        nokeys.partition, nokeys.key_len, nokeys.val_len, nokeys.ts_ms = b.partition, b.key_len, b.val_len, b.ts_ms
        for which in (1, 3):
            with pytest.raises(kta.KtaError, match="key columns missing"):
                h.submit_device(nokeys, n, 0, which=which)
        assert np.array_equal(h.hot_keys(), v0) and np.array_equal(h.finish(allow_bad_partition=True)[1], c0)
        h.reset()
        assert not h.hot_keys().any() and not h.hot_key_exemplars()["valid"].any()
        h.finish(allow_bad_partition=True)
        assert not h.exchange_hot_keys().any()
        assert h.hot_keys_info() == {"keyed": 0, "groups": 0, "flushes": 0, "launches": 0, "exemplars": 0, "workgroups": 0}
        with pytest.raises(kta.KtaError):
            h.replay_messages({k: v for k, v in cols.items() if k not in ("key_off", "key_bytes")})
        h.sync()
        h.device_batch_free(b)
    with kta.HipMetricHandler(P, now=NOW) as h:
        for fn in (h.hot_keys, h.exchange_hot_keys, h.hot_keys_result_vector, h.hot_keys_info, h.hot_key_exemplars,
                   lambda: h.set_hot_flush_rounds(3)):
            with pytest.raises(kta.KtaError, match="KTA_FLAG_HOT_KEYS"):
                fn()


def test_with_c_the_fused_pass_is_still_taken_and_all_opt_ins_compose():
    sp, _ = kta.synth_preset("c3")
    n, P = 1 << 22, 64
    cols = kta.synth_fill_host(sp, 0, n, with_keys=True)
    o = Oracle(NOW, count_alive_keys=True)
    o.run_soa(cols)
    want = H.vector(cols, P)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, hot_keys=True) as h:
        b, nb = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, nb, 0, which=3)
        res, c = h.finish()
        info = h.alive_pass_info()
        assert info["fused"] > 0 and info["scanned"] == 0
        assert np.array_equal(c, o.counters(P)) and res.alive_keys == o.alive_keys()
        assert np.array_equal(h.exchange_hot_keys(), want)
        h.sync()
        h.device_batch_free(b)
    # -c, analytics, a timeline, the key sketch and the hot keys at once: each result what it is alone
    tl = (int(sp.ts_base_ms), 1_000, 40)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, batch_capacity=1 << 21, key_bytes_capacity=1 << 26,
                              analytics=True, timeline=tl, key_sketch=True, hot_keys=True) as h, \
            kta.HipMetricHandler(P, now=NOW, batch_capacity=1 << 21, analytics=True) as alone:
        for x in (h, alone):
            x.submit_columns(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"], cols["key_off"],
                             cols["key_bytes"])
        res, c = h.finish()
        alone.finish()
        assert np.array_equal(c, o.counters(P)) and res.alive_keys == o.alive_keys()
        assert np.array_equal(h.exchange_hot_keys(), want)
        assert np.array_equal(h.exchange_key_sketch(), K.sketch(cols, P))
        assert np.array_equal(h.exchange_timeline(), T.timeline_vector(cols, P, *tl))
        a, a0 = h.exchange_analytics(), alone.exchange_analytics()
        assert a.keys() == a0.keys() and all(np.array_equal(a[k], a0[k]) for k in a)


def test_kafka_decode_zero_copy_keys():
    from kafka_cases import random_record_set
    lib = N.load()
    rng = np.random.default_rng(42)
    P = 4
    blobs, hashes = [], []
    for fetch in range(6):
        part = fetch % P
        blob, (pl, klen, vlen, ts, keys), _ = random_record_set(rng, 50, partition=part, key_space=300, with_noise=False)
        blobs.append((blob, part))
        hashes += [H.fnv1a(bytes(k)) for k in keys if k is not None]
    want = H.vector_from_hashes(np.array(hashes, np.uint64))
    assert want.any()
    with kta.HipMetricHandler(P, now=NOW, hot_keys=True) as h:
        for blob, part in blobs:
            st = N.KtaKafkaIndexStats()
            h._check(lib.kta_kafka_consume(h._ctx, blob, len(blob), part, C.byref(st)))
        assert np.array_equal(h.hot_keys(), want)


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
import hot_keys_py as H
from helpers import NOW, random_cols

P = 7
rng = np.random.default_rng(31)
cols = random_cols(rng, 80000, P, key_space=20000, tomb=0.3, max_key=64)
n = len(cols["partition"])
cols["seq"] = np.arange(n, dtype=np.uint64)
half = n // 2

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

vec = lambda idx: H.vector(subset(idx), P)
want = {"first": vec(np.arange(half)), "all": vec(np.arange(n))}

for nranks in (2, 3):
    for with_c in (False, True):
        uid = kta.HipMetricHandler.comm_unique_id()
        errors = []
        def run(rank):
            try:
                h = kta.HipMetricHandler(P, count_alive_keys=with_c, now=NOW, seq_column=with_c, hot_keys=True)
                h.comm_create(nranks, rank, uid)
                mine = cols["partition"] % nranks == rank
                for stage, idx in (("first", np.arange(half)[mine[:half]]), ("all", np.arange(half, n)[mine[half:]])):
                    sh = subset(idx)
                    if not with_c:
                        del sh["seq"]
                    b, nb = h.upload_batch(sh, with_keys=True)
                    h.submit_device(b, nb, 0)
                    h.exchange()
                    assert np.array_equal(h.exchange_hot_keys(), want[stage]), (nranks, with_c, rank, stage, "exchanged")
                    own = np.nonzero(mine[:half if stage == "first" else n])[0]
                    assert np.array_equal(h.hot_keys(), vec(own)), (nranks, with_c, rank, stage, "own")
                    h.exchange()
                    assert np.array_equal(h.exchange_hot_keys(), want[stage]), (nranks, with_c, rank, stage, "again")
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


def test_exchange_hot_keys_on_two_and_three_ranks_with_and_without_c(tmp_path, mock_rccl):
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
    at = stdout.index("Hot keys, at most")
    return stdout[:at], stdout[at:]


def _keys_by_hash(cols):
    """{hash: key bytes} of the keyed records of columns (the first key of a hash)."""
    kl, off, kb = cols["key_len"], cols["key_off"], cols["key_bytes"].tobytes()
    hashes = K.fnv_columns(kl, off, cols["key_bytes"])
    out = {}
    for i in np.nonzero(kl >= 0)[0]:
        out.setdefault(int(hashes[i]), kb[int(off[i]):int(off[i]) + int(kl[i])] if kl[i] > 0 else b"")
    return out


def test_cli_hot_keys_section_single_sharded_per_message(mock_rccl):
    src = "synthetic://c2?records=250000"
    sp, _ = kta.synth_preset("c2")
    cols = kta.synth_fill_host(sp, 0, 250000, with_keys=True)
    P = int(sp.n_partitions)
    vec = H.vector(cols, P)
    want = H.section(vec, 5, _keys_by_hash(cols))
    assert "| 1 |     | 811c9dc5 |" in want           # the empty key, about 1 % of c2's records, printed as it is
    plain = _cli("-t", "c2", "-b", src)
    assert plain.returncode == 0, plain.stderr
    one = _cli("-t", "c2", "-b", src, "--librdkafka", "kta.hot_keys=5")
    assert one.returncode == 0, one.stderr
    report, section = _split(one.stdout)
    assert section == want and _normalise(report) == _normalise(plain.stdout)
    both = _cli("-t", "c2", "-b", src, "--librdkafka", "kta.analytics=1,kta.timeline=1h,kta.distinct_keys=1,kta.hot_keys=5")
    assert both.returncode == 0, both.stderr
    rep2, sec2 = _split(both.stdout)
    assert sec2 == want and "Timeline, 1h" in rep2 and "Size histograms" in rep2 and "Distinct keys per partition" in rep2
    env = dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl)
    for c in ([], ["-c"]):
        many = _cli("-t", "c2", "-b", src, *c, "--librdkafka", "kta.hot_keys=5,kta.gpus=2,kta.batch=32768,kta.oversubscribe=1",
                    env=env)
        assert many.returncode == 0, (c, many.stderr[-2000:])
        assert many.stdout.count("Hot keys, at most") == 1 and _split(many.stdout)[1] == want, c
    pm = _cli("-t", "c2", "-b", src, "--librdkafka", "kta.hot_keys=5,kta.per_message=1,kta.batch=4096")
    assert pm.returncode == 0, pm.stderr
    assert _split(pm.stdout)[1] == want


def test_cli_hot_keys_section_on_raw_kafka_log_segments(tmp_path):
    import kafka_format as F

    def encode_record_set(rng, keys, partition):
        """A log segment of the records with these keys, 100 to a batch."""
        blob, offset = bytearray(), 1000 * partition
        for lo in range(0, len(keys), 100):
            recs = [(int(rng.integers(0, 5000)), k, None if rng.random() < 0.2 else b"v" * int(rng.integers(0, 50)), [])
                    for k in keys[lo:lo + 100]]
            base_ts = 1_600_000_000_000 + lo
            blob += F.encode_batch(offset, recs, base_ts, attributes=0, max_ts=max(base_ts + r[0] for r in recs), compression=None)
            offset += len(recs)
        return bytes(blob)

    rng = np.random.default_rng(8)
    hot = b"order-4711\\eu"
    files, hashes = [], []
    for p in range(3):
        keys = [hot if rng.random() < 0.2 else (None if rng.random() < 0.1 else b"k%05d" % rng.integers(0, 3000))
                for _ in range(4000)]
        blob = encode_record_set(rng, keys, partition=p)
        path = tmp_path / ("%020d.log" % p)
        path.write_bytes(blob)
        files.append(str(path))
        hashes += [H.fnv1a(k) for k in keys if k is not None]
    vec = H.vector_from_hashes(np.array(hashes, np.uint64))
    want = H.section(vec, 1, {H.fnv1a(hot): hot})
    assert "| 1 | order-4711\\x5Ceu |" in want
    r = _cli("-t", "seg", "-b", "segment://" + ",".join(files), "--librdkafka", "kta.hot_keys=1")
    assert r.returncode == 0, r.stderr
    report, section = _split(r.stdout)
    assert section == want
    plain = _cli("-t", "seg", "-b", "segment://" + ",".join(files))
    assert plain.returncode == 0 and _normalise(plain.stdout) == _normalise(report)
    # a topic without a keyed record: the title and one line
    empty = tmp_path / "empty"
    empty.mkdir()
    blob = encode_record_set(rng, [None] * 50, partition=0)
    (empty / "0.log").write_bytes(blob)
    r = _cli("-t", "seg", "-b", "segment://" + str(empty / "0.log"), "--librdkafka", "kta.hot_keys=3")
    assert r.returncode == 0, r.stderr
    assert _split(r.stdout)[1] == H.title(3) + "No key holds 1/512 of the 0 keyed records.\n"

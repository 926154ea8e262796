"""GPU tests of the key sketch (KTA_FLAG_KEY_SKETCH: a HyperLogLog sketch of the key hashes per partition; no reference
counterpart), the registers bit-exact against the independent numpy restatement in tests/key_sketch_py.py:

    random columns           null and empty keys, tombstones, bad partitions, key lengths 0..300: the staging ring,
                             kta_handle_message, kta_replay_messages, raw and tile-compact device batches, views; the
                             counters identical to a context without the flag
    behaviour                a batch without key columns refused, kta_reset, the calls of a context without the flag
    with -c                  which == 3: the fused pass still taken, the alive count the oracle's; with analytics and a
                             timeline as well
    the Kafka decode         raw log segments, zero-copy keys
    the c3 law at 2^30       tile-compact device batches, the topic-wide estimate within 3 % of the distinct hashes
    contention               one key 2^26 times; P = 1 with 2^26 distinct keys
    kta_exchange             the RCCL test double, 2 and 3 ranks, with and without -c
    kta-analyzer             kta.distinct_keys=1 on synthetic://, segment://, kta.per_message=1 and kta.gpus=2"""
import ctypes as C
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import key_sketch_py as K
import timeline_py as T
from helpers import NOW, random_cols
from oracle_c import Oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
THREADS = 16                          # the CPU allotment of a GPU machine, not os.cpu_count()
CHUNK = 1 << 22


def _cols(seed, n=60000, P=6):
    rng = np.random.default_rng(seed)
    cols = random_cols(rng, n, P, key_space=9000, null_key=0.15, empty_key=0.05, tomb=0.3, max_key=300)
    cols["partition"][rng.random(n) < 0.02] = -1            # a damaged batch's records
    cols["partition"][rng.random(n) < 0.02] = P + 3          # out of range
    return cols


def _keyed(cols, P):
    return np.array([((cols["partition"] == p) & (cols["key_len"] >= 0)).sum() for p in range(P)], np.uint64)


def test_random_columns_every_entry_path_bit_exact():
    P = 6
    cols = _cols(1)
    assert set(np.unique(cols["key_len"] % 16)) > {0, 1, 3} and cols["key_len"].max() > 250
    want = K.sketch(cols, P)
    assert want.any() and int(want.max()) >= 10
    # the staging ring (several batches), against a context without the flag fed the same records
    with kta.HipMetricHandler(P, now=NOW, batch_capacity=1 << 13, key_bytes_capacity=1 << 17, key_sketch=True) as h, \
            kta.HipMetricHandler(P, now=NOW, batch_capacity=1 << 13) as plain:
        for x in (h, plain):
            x.submit_columns(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"], cols["key_off"],
                             cols["key_bytes"])
        assert np.array_equal(h.key_sketch(), want)
        res, c = h.finish(allow_bad_partition=True)
        res0, c0 = plain.finish(allow_bad_partition=True)
        assert np.array_equal(c, c0) and bytes(res) == bytes(res0)
        assert np.array_equal(h.exchange_key_sketch(), want)
        info = h.key_sketch_info()
        assert info["keyed"] == int(_keyed(cols, P).sum()) and info["launches"] >= 8
        assert info["atomics"] <= info["reads"] <= info["keyed"]
    # kta_handle_message (one message at a time) and kta_replay_messages
    sub = {k: v[:3000] for k, v in cols.items() if k != "key_bytes"}
    sub["key_bytes"] = cols["key_bytes"]
    want_sub = K.sketch(sub, P)
    with kta.HipMetricHandler(P, now=NOW, batch_capacity=1 << 10, key_sketch=True) as h:
        kb = cols["key_bytes"].tobytes()
        for i in range(3000):
            kl = int(cols["key_len"][i])
            key = None if kl < 0 else kb[int(cols["key_off"][i]):int(cols["key_off"][i]) + kl]
            h.handle_message(kta.Message(int(cols["partition"][i]), int(cols["ts_ms"][i]), key, int(cols["val_len"][i])))
        assert np.array_equal(h.key_sketch(), want_sub)
        h.reset()
        assert not h.key_sketch().any()
        h.replay_messages(cols)
        assert np.array_equal(h.key_sketch(), want)
    # tile-compact device batches, views at record offsets (which = 1 for the metrics handler alone)
    with kta.HipMetricHandler(P, now=NOW, key_sketch=True) as h:
        b, n = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, n, 0, which=1)
        assert np.array_equal(h.key_sketch(), want)
        h.reset()
        cut = 1000 + 36                                     # (a view's columns stay 16-byte aligned)
        for lo, hi in ((0, cut), (cut, 2 * 1024 + 4), (2 * 1024 + 4, n)):
            v = N.KtaBatch()
            v.partition, v.key_len, v.val_len = b.partition + 4 * lo, b.key_len + 4 * lo, b.val_len + 4 * lo
            v.ts_ms, v.key_off, v.key_bytes = b.ts_ms + 8 * lo, b.key_off + 4 * lo, b.key_bytes
            h.submit_device(v, hi - lo, 0, which=1)
        assert np.array_equal(h.key_sketch(), want)
        h.reset()
        h.submit_device(b, n, 0, which=2)                   # the alive-key handler alone: not the sketch's records
        assert not h.key_sketch().any()
        h.sync()
        h.device_batch_free(b)


def test_raw_layout_device_batch():
    import torch
    P = 6
    cols = _cols(2, n=40000)
    want = K.sketch(cols, P)
    dev = {k: torch.from_numpy(np.ascontiguousarray(cols[k])).cuda() for k in ("partition", "key_len", "val_len", "ts_ms")}
    dev["key_off"] = torch.from_numpy(cols["key_off"].view(np.int32)).cuda()
    kb = np.zeros(len(cols["key_bytes"]) + 32, np.uint8)
    kb[:len(cols["key_bytes"])] = cols["key_bytes"]
    dev["key_bytes"] = torch.from_numpy(kb).cuda()
    torch.cuda.synchronize()
    b = N.KtaBatch()
    for k, t in dev.items():
        setattr(b, k, t.data_ptr())
    with kta.HipMetricHandler(P, now=NOW, key_sketch=True) as h:
        h.submit_device(b, len(cols["partition"]), 0, which=1)
        assert np.array_equal(h.key_sketch(), want)
        h.sync()


def test_refusal_reset_and_calls_without_the_flag():
    P = 4
    cols = _cols(3, n=5000, P=P)
    with kta.HipMetricHandler(P, now=NOW, key_sketch=True) as h:
        b, n = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, n, 0, which=1)
        sk0, c0 = h.key_sketch(), h.finish(allow_bad_partition=True)[1]
        nokeys = N.KtaBatch()
        nokeys.partition, nokeys.key_len, nokeys.val_len, nokeys.ts_ms = b.partition, b.key_len, b.val_len, b.ts_ms
        for which in (1, 3):
            with pytest.raises(kta.KtaError, match="key columns missing"):
                h.submit_device(nokeys, n, 0, which=which)
        assert np.array_equal(h.key_sketch(), sk0) and np.array_equal(h.finish(allow_bad_partition=True)[1], c0)
        h.reset()
        assert not h.key_sketch().any()
        h.finish(allow_bad_partition=True)
        assert not h.exchange_key_sketch().any()
        with pytest.raises(kta.KtaError):
            h.replay_messages({k: v for k, v in cols.items() if k not in ("key_off", "key_bytes")})
        h.sync()
        h.device_batch_free(b)
    with kta.HipMetricHandler(P, now=NOW) as h:
        for fn in (h.key_sketch, h.exchange_key_sketch, h.key_sketch_result_vector, h.key_sketch_info):
            with pytest.raises(kta.KtaError, match="KTA_FLAG_KEY_SKETCH"):
                fn()


def test_with_c_the_fused_pass_is_still_taken():
    sp, _ = kta.synth_preset("c3")
    n, P = 1 << 22, 64
    cols = kta.synth_fill_host(sp, 0, n, with_keys=True)
    o = Oracle(NOW, count_alive_keys=True)
    o.run_soa(cols)
    want = K.sketch(cols, P)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, key_sketch=True) as h:
        b, nb = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, nb, 0, which=3)
        res, c = h.finish()
        info = h.alive_pass_info()
        assert info["fused"] > 0 and info["scanned"] == 0
        assert np.array_equal(c, o.counters(P)) and res.alive_keys == o.alive_keys()
        assert np.array_equal(h.exchange_key_sketch(), want)
        h.sync()
        h.device_batch_free(b)
    # with analytics and a timeline (the batch then takes the scan, then the alive-key pass)
    tl = (int(sp.ts_base_ms), 1_000, 40)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, batch_capacity=1 << 21, key_bytes_capacity=1 << 26,
                              analytics=True, timeline=tl, key_sketch=True) as h:
        h.submit_columns(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"], cols["key_off"],
                         cols["key_bytes"])
        res, c = h.finish()
        assert np.array_equal(c, o.counters(P)) and res.alive_keys == o.alive_keys()
        assert np.array_equal(h.exchange_key_sketch(), want)
        assert np.array_equal(h.exchange_timeline(), T.timeline_vector(cols, P, *tl))


def test_kafka_decode_zero_copy_keys():
    from kafka_cases import random_record_set
    lib = N.load()
    rng = np.random.default_rng(42)
    P = 4
    blobs, parts, hashes = [], [], []
    for fetch in range(6):
        part = fetch % P
        blob, (pl, klen, vlen, ts, keys), _ = random_record_set(rng, 50, partition=part, key_space=300, with_noise=False)
        blobs.append((blob, part))
        for k in keys:
            if k is not None:
                parts.append(part)
                hashes.append(K.fnv1a(bytes(k)))
    want = K.sketch_from_hashes(np.array(parts), np.array(hashes, np.uint64), P)
    assert want.any()
    with kta.HipMetricHandler(P, now=NOW, key_sketch=True) as h:
        for blob, part in blobs:
            st = N.KtaKafkaIndexStats()
            h._check(lib.kta_kafka_consume(h._ctx, blob, len(blob), part, C.byref(st)))
        assert np.array_equal(h.key_sketch(), want)


def _c3_truth(sp, n):
    """(the set of key ids the c3 law draws among records [0, n), by 16 threads in chunks)."""
    seen = np.zeros(int(sp.n_distinct_keys), np.bool_)
    chunks = iter([(lo, min(CHUNK, n - lo)) for lo in range(0, n, CHUNK)])
    lock = threading.Lock()
    errors = []

    def work():
        try:
            while True:
                with lock:
                    ch = next(chunks, None)
                if ch is None:
                    return
                kid = K.synth_key_ids(sp, *ch)
                seen[kid[kid >= 0]] = True          # (idempotent stores: no lock needed)
        except BaseException as e:   # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=work) for _ in range(THREADS)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errors, errors
    return np.nonzero(seen)[0]


def test_c3_law_2e30_records_tile_compact():
    sp, _ = kta.synth_preset("c3")
    n, P = 1 << 30, int(sp.n_partitions)
    assert sp.part_mode == 1 and P == 64
    ids = _c3_truth(sp, n)
    h32 = K.synth_key_hashes(sp, ids)
    want = K.sketch_from_hashes(ids % P, h32, P)
    distinct_hashes = len(np.unique(h32))
    step = 1 << 27                                          # (key bytes of a batch: < 4 GiB)
    with kta.HipMetricHandler(P, now=NOW, key_sketch=True) as h:
        b = h.device_batch_alloc(step, 16 * step + 16)
        for lo in range(0, n, step):
            h.synth_fill_device(sp, lo, step, b)
            h.submit_device(b, step, lo, which=1)
        res, c = h.finish()
        info = h.key_sketch_info()
        h.device_batch_free(b)
        got = h.exchange_key_sketch()
    assert res.overall_count == n and np.array_equal(got, want)
    per, topic = kta.estimate_distinct_keys(got, P)
    assert abs(topic / distinct_hashes - 1) <= 0.03, (topic, distinct_hashes)
    assert info["keyed"] == int(c[:, N.KTA_C_KEY_NON_NULL].sum())
    print("c3 sketch work:", info, "distinct hashes", distinct_hashes, "estimate", topic)


def test_contention_one_key_and_one_partition():
    n = 1 << 26
    with kta.HipMetricHandler(3, now=NOW, key_sketch=True) as h:
        key = np.frombuffer(b"the one hot key!", np.uint8)
        cols = {"partition": np.full(n, 2, np.int32), "key_len": np.full(n, 16, np.int32),
                "val_len": np.full(n, 10, np.int32), "ts_ms": np.full(n, 1_600_000_000_000, np.int64),
                "key_off": np.zeros(n, np.uint32), "key_bytes": key}
        b, nb = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, nb, 0, which=1)
        want = K.sketch_from_hashes(np.array([2]), np.array([K.fnv1a(key.tobytes())], np.uint64), 3)
        assert np.array_equal(h.key_sketch(), want)
        info = h.key_sketch_info()
        assert info["keyed"] == n and info["atomics"] < n // 64
        h.sync()
        h.device_batch_free(b)
    sp, _ = kta.synth_preset("c3")
    sp.n_partitions, sp.n_distinct_keys, sp.key_null_permille, sp.key_empty_permille = 1, 0, 0, 0
    with kta.HipMetricHandler(1, now=NOW, key_sketch=True) as h:
        b = h.device_batch_alloc(n, 16 * n + 16)
        h.synth_fill_device(sp, 0, n, b)
        h.submit_device(b, n, 0, which=1)
        got = h.key_sketch()
        h.sync()
        h.device_batch_free(b)
    parts = [K.synth_key_hashes(sp, np.arange(lo, min(lo + CHUNK, n))) for lo in range(0, n, CHUNK)]
    h32 = np.concatenate(parts)
    assert np.array_equal(got, K.sketch_from_hashes(np.zeros(n, np.int64), h32, 1))
    (e,), _ = kta.estimate_distinct_keys(got, 1)
    assert abs(e / len(np.unique(h32)) - 1) <= 0.05


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
import key_sketch_py as K
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

sk = lambda idx: K.sketch(subset(idx), P)
want = {"first": sk(np.arange(half)), "all": sk(np.arange(n))}

for nranks in (2, 3):
    for with_c in (False, True):
        uid = kta.HipMetricHandler.comm_unique_id()
        errors = []
        def run(rank):
            try:
                h = kta.HipMetricHandler(P, count_alive_keys=with_c, now=NOW, seq_column=with_c, key_sketch=True)
                h.comm_create(nranks, rank, uid)
                mine = cols["partition"] % nranks == rank
                for stage, idx in (("first", np.arange(half)[mine[:half]]), ("all", np.arange(half, n)[mine[half:]])):
                    sh = subset(idx)
                    if not with_c:
                        del sh["seq"]
                    b, nb = h.upload_batch(sh, with_keys=True)
                    h.submit_device(b, nb, 0)
                    h.exchange()
                    assert np.array_equal(h.exchange_key_sketch(), want[stage]), (nranks, with_c, rank, stage, "exchanged")
                    own = np.nonzero(mine[:half if stage == "first" else n])[0]
                    assert np.array_equal(h.key_sketch(), sk(own)), (nranks, with_c, rank, stage, "own")
                    h.exchange()
                    assert np.array_equal(h.exchange_key_sketch(), want[stage]), (nranks, with_c, rank, stage, "again")
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


def test_exchange_key_sketch_on_two_and_three_ranks_with_and_without_c(tmp_path, mock_rccl):
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
    at = stdout.index("Distinct keys per partition")
    return stdout[:at], stdout[at:]


def test_cli_distinct_keys_section_single_sharded_per_message(mock_rccl):
    src = "synthetic://c2?records=250000"
    sp, _ = kta.synth_preset("c2")
    cols = kta.synth_fill_host(sp, 0, 250000, with_keys=True)
    P = int(sp.n_partitions)
    want = K.section(K.sketch(cols, P), _keyed(cols, P))
    plain = _cli("-t", "c2", "-b", src)
    assert plain.returncode == 0, plain.stderr
    one = _cli("-t", "c2", "-b", src, "--librdkafka", "kta.distinct_keys=1")
    assert one.returncode == 0, one.stderr
    report, section = _split(one.stdout)
    assert section == want and _normalise(report) == _normalise(plain.stdout)
    both = _cli("-t", "c2", "-b", src, "--librdkafka", "kta.analytics=1,kta.timeline=1h,kta.distinct_keys=1")
    assert both.returncode == 0, both.stderr
    rep2, sec2 = _split(both.stdout)
    assert sec2 == want and "Timeline, 1h" in rep2 and "Size histograms" in rep2
    assert rep2.index("Size histograms") < rep2.index("Timeline, 1h")
    env = dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl)
    for c in ([], ["-c"]):
        many = _cli("-t", "c2", "-b", src, *c, "--librdkafka",
                    "kta.distinct_keys=1,kta.gpus=2,kta.batch=32768,kta.oversubscribe=1", env=env)
        assert many.returncode == 0, (c, many.stderr[-2000:])
        assert many.stdout.count("Distinct keys per partition") == 1 and _split(many.stdout)[1] == want, c
    pm = _cli("-t", "c2", "-b", src, "--librdkafka", "kta.distinct_keys=1,kta.per_message=1,kta.batch=4096")
    assert pm.returncode == 0, pm.stderr
    assert _split(pm.stdout)[1] == want


def test_cli_distinct_keys_section_on_raw_kafka_log_segments(tmp_path):
    from kafka_cases import random_record_set
    rng = np.random.default_rng(8)
    files, parts, hashes, keyed = [], [], [], np.zeros(4, np.uint64)
    for p in range(4):
        blob, (part, klen, vlen, ts, keys), _ = random_record_set(rng, 20, partition=p, key_space=300, with_noise=False,
                                                                   snappy=(p == 1))
        path = tmp_path / ("%020d.log" % p)
        path.write_bytes(blob)
        files.append(str(path))
        for k in keys:
            if k is not None:
                parts.append(p)
                hashes.append(K.fnv1a(bytes(k)))
                keyed[p] += 1
    want = K.section(K.sketch_from_hashes(np.array(parts), np.array(hashes, np.uint64), 4), keyed)
    r = _cli("-t", "seg", "-b", "segment://" + ",".join(files), "--librdkafka", "kta.distinct_keys=1")
    assert r.returncode == 0, r.stderr
    report, section = _split(r.stdout)
    assert section == want
    plain = _cli("-t", "seg", "-b", "segment://" + ",".join(files))
    assert plain.returncode == 0 and _normalise(plain.stdout) == _normalise(report)

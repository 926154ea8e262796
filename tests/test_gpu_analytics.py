"""GPU tests of the exchanged and printed analytics (KTA_FLAG_ANALYTICS, ABI 7):

    config 4 at 2^30 records on one GPU    histograms + every partition's extrema bit-exact against the oracle's
                                           analytics (kto_analytics_*), the reference counters against its counters
    kta_exchange on the RCCL test double   2 and 3 ranks, with and without -c: the exchanged snapshot is the unsharded
                                           oracle's, the live accumulator stays the rank's own, a second exchange
                                           after more batches counts nothing twice
    kta-analyzer --librdkafka kta.analytics=1
                                           the report unchanged, the section after it equal to the Python restatement
                                           (tests/analytics_py.py) of the oracle's analytics, the same under kta.gpus=N,
                                           kta.per_message=1 and segment://"""
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import analytics_py as AP
from helpers import NOW
from oracle_c import Oracle, analytics as oracle_analytics

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
CHUNK = 1 << 22
ORACLE_THREADS = 16                   # the CPU allotment of a GPU machine, not os.cpu_count()


def _merge_decoded(a, b):
    """Two decoded analytics dicts of disjoint record sets -> the union's (sentinels are the identities)."""
    return {"key_size_hist": a["key_size_hist"] + b["key_size_hist"],
            "value_size_hist": a["value_size_hist"] + b["value_size_hist"],
            "part_min_ts_sec": np.minimum(a["part_min_ts_sec"], b["part_min_ts_sec"]),
            "part_max_ts_sec": np.maximum(a["part_max_ts_sec"], b["part_max_ts_sec"]),
            "part_smallest": np.minimum(a["part_smallest"], b["part_smallest"]),
            "part_largest": np.maximum(a["part_largest"], b["part_largest"])}


def _assert_same(got, want, what=""):
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k)


def _oracle_threaded(spec, n, P):
    """The oracle's counters[P,7] and analytics over records [0, n) of the synthetic topic: independent instances over
    consecutive chunks (sums and extrema merge exactly), ORACLE_THREADS threads (ctypes calls release the GIL)."""
    chunks = [(lo, min(CHUNK, n - lo)) for lo in range(0, n, CHUNK)]
    oracles = [Oracle(NOW) for _ in range(ORACLE_THREADS)]
    parts = [None] * ORACLE_THREADS
    nxt = iter(range(len(chunks)))
    lock = threading.Lock()
    errors = []

    def work(t):
        try:
            while True:
                with lock:
                    k = next(nxt, None)
                if k is None:
                    return
                cols = kta.synth_fill_host(spec, *chunks[k])
                oracles[t].run_soa(cols)
                a = oracle_analytics(cols, P)
                parts[t] = a if parts[t] is None else _merge_decoded(parts[t], a)
        except BaseException as e:   # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=work, args=(t,)) for t in range(ORACLE_THREADS)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errors, errors
    counters = sum(o.counters(P) for o in oracles)
    for o in oracles:
        o.close()
    got = [p for p in parts if p is not None]
    acc = got[0]
    for p in got[1:]:
        acc = _merge_decoded(acc, p)
    return counters, acc


# ------------------------------------------------------------------------------------------ 6. config 4, 2^30 records
def test_analytics_config_4_256_partitions_2e30_records_bit_exact():
    sp, _ = kta.synth_preset("c4")
    n, P = 1 << 30, 256
    assert sp.n_partitions == P
    want_c, want_a = _oracle_threaded(sp, n, P)
    with kta.HipMetricHandler(P, now=NOW, analytics=True) as h:
        b = h.device_batch_alloc(n)
        h.synth_fill_device(sp, 0, n, b)
        h.submit_device(b, n, 0, which=1)
        res, c = h.finish()
        h.device_batch_free(b)
        live, snap = h.analytics(), h.exchange_analytics()
    assert np.array_equal(c, want_c) and res.overall_count == n
    _assert_same(live, want_a, "live")
    _assert_same(snap, want_a, "snapshot")
    assert int(live["key_size_hist"].sum()) == int(live["value_size_hist"].sum()) == n
    assert (live["part_max_ts_sec"] != np.iinfo(np.int64).min).all()          # every partition of c4 has records


# ------------------------------------------------------------------------------------------ 7. kta_exchange, test double
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
from helpers import NOW, random_cols
from oracle_c import Oracle, analytics

P = 7
rng = np.random.default_rng(23)
cols = random_cols(rng, 160000, P, key_space=3000, tomb=0.3, big_sizes=True)
cols["val_len"][cols["partition"] == 5] = -1                        # a tombstone-only partition
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
            "ts_ms": cols["ts_ms"][idx], "key_off": off.astype(np.uint32), "key_bytes": kb[:int(kl.sum())],
            "seq": cols["seq"][idx]}

def oracle(idx, with_c):
    c = subset(idx)
    o = Oracle(NOW, with_c); o.run_soa(c)
    return o, analytics(c, P)

first, everything = np.arange(half), np.arange(n)
want = {k: oracle(idx, True) for k, idx in (("first", first), ("all", everything))}

def same(got, ref, what):
    for k in ref:
        assert np.array_equal(np.asarray(got[k]), np.asarray(ref[k])), (what, k)

for nranks in (2, 3):
    for with_c in (False, True):
        uid = kta.HipMetricHandler.comm_unique_id()
        errors = []
        def run(rank):
            try:
                h = kta.HipMetricHandler(P, count_alive_keys=with_c, now=NOW, analytics=True, seq_column=with_c)
                h.comm_create(nranks, rank, uid)
                mine = cols["partition"] % nranks == rank
                for stage, idx in (("first", first[mine[first]]), ("all", np.arange(half, n)[mine[half:]])):
                    sh = subset(idx)
                    if not with_c:
                        del sh["seq"]
                    b, nb = h.upload_batch(sh, with_keys=with_c)
                    h.submit_device(b, nb, 0)
                    h.exchange()
                    o, a = want[stage]
                    same(h.exchange_analytics(), a, (nranks, with_c, rank, stage, "exchanged"))
                    own = np.nonzero(mine[:half if stage == "first" else n])[0]
                    same(h.analytics(), oracle(own, False)[1], (nranks, with_c, rank, stage, "own"))
                    res, c = h.exchange_result()
                    assert np.array_equal(c, o.counters(P)), (nranks, with_c, rank, stage)
                    if with_c and stage == "first":
                        assert res.alive_keys == o.alive_keys(), (nranks, rank, stage, res.alive_keys, o.alive_keys())
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


def test_exchange_analytics_on_two_and_three_ranks_with_and_without_c(tmp_path, mock_rccl):
    script = tmp_path / "exchange_worker.py"
    script.write_text(_EXCHANGE_WORKER)
    env = dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(script), ROOT], capture_output=True, text=True,
                       timeout=330, env=env)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count(" OK") == 4


# ------------------------------------------------------------------------------------------ 8. the CLI
def _cli(*args, env=None, cwd=None):
    return subprocess.run(["timeout", "-k", "10", "240", CLI, *args], capture_output=True, text=True, timeout=270,
                          env=env, cwd=cwd)


def _normalise(text):
    text = re.sub(r"Scanning took: \d+ seconds", "Scanning took: 3 seconds", text)
    return re.sub(r"Estimated Msg/s: \d+", "Estimated Msg/s: 133", text)


def _section(stdout):
    at = stdout.index("Size histograms and per-partition extrema")
    return stdout[:at], stdout[at:]


def test_cli_analytics_section_single_sharded_per_message(mock_rccl):
    src = "synthetic://c2?records=250000"
    sp, _ = kta.synth_preset("c2")
    want = AP.section(oracle_analytics(kta.synth_fill_host(sp, 0, 250000), int(sp.n_partitions)))
    plain = _cli("-t", "c2", "-b", src)
    assert plain.returncode == 0, plain.stderr
    assert "Size histograms" not in plain.stdout
    env = dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl)
    for c in ([], ["-c"]):
        one = _cli("-t", "c2", "-b", src, *c, "--librdkafka", "kta.analytics=1")
        assert one.returncode == 0, one.stderr
        report, section = _section(one.stdout)
        assert section == want, c
        if not c:
            assert _normalise(report) == _normalise(plain.stdout)          # the reference report, unchanged
        else:
            assert "Alive keys: " in report
        for knobs in ("kta.gpus=2,kta.batch=32768,kta.oversubscribe=1", "kta.gpus=3,kta.oversubscribe=1"):
            many = _cli("-t", "c2", "-b", src, *c, "--librdkafka", "kta.analytics=1," + knobs, env=env)
            assert many.returncode == 0, (knobs, c, many.stderr[-2000:])
            assert _normalise(many.stdout) == _normalise(one.stdout), (knobs, c)
            assert many.stdout.count("Size histograms") == 1
    pm = _cli("-t", "c2", "-b", src, "--librdkafka", "kta.analytics=1,kta.per_message=1,kta.batch=4096")
    assert pm.returncode == 0, pm.stderr
    assert _section(pm.stdout)[1] == want


def test_cli_analytics_section_on_raw_kafka_log_segments(tmp_path):
    from kafka_cases import random_record_set
    rng = np.random.default_rng(8)
    files, cols = [], {"partition": [], "key_len": [], "val_len": [], "ts_ms": []}
    for p in range(4):
        blob, (part, klen, vlen, ts, keys), _ = random_record_set(rng, 20, partition=p, key_space=30, with_noise=False,
                                                                   snappy=(p == 1))
        path = tmp_path / ("%020d.log" % p)
        path.write_bytes(blob)
        files.append(str(path))
        cols["partition"] += [p] * len(part)
        cols["key_len"] += list(klen)
        cols["val_len"] += list(vlen)
        cols["ts_ms"] += list(ts)
    cols = {"partition": np.array(cols["partition"], np.int32), "key_len": np.array(cols["key_len"], np.int32),
            "val_len": np.array(cols["val_len"], np.int32), "ts_ms": np.array(cols["ts_ms"], np.int64)}
    want = AP.section(oracle_analytics(cols, 4))
    r = _cli("-t", "seg", "-b", "segment://" + ",".join(files), "--librdkafka", "kta.analytics=1")
    assert r.returncode == 0, r.stderr
    report, section = _section(r.stdout)
    assert section == want
    plain = _cli("-t", "seg", "-b", "segment://" + ",".join(files))
    assert plain.returncode == 0 and _normalise(plain.stdout) == _normalise(report)

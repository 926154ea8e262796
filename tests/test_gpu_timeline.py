"""GPU tests of the timeline (kta_set_timeline: records, tombstones and bytes per time bucket; no reference counterpart),
each against the independent numpy restatement in tests/timeline_py.py:

    boundary timestamps      raw host batches and tile-compact device batches, widths 1 ms, 7 ms, 1 h and 2^40 ms,
                             tombstones, null keys, bad partitions (left out)
    config 4 at 2^30 records tile-compact device batches, W = 10 s, 1024 buckets: bit-exact, and the counters identical
                             to a context without the timeline fed the same batches
    the c3 law with -c       analytics and timeline together: counters and alive keys against the oracle, the timeline
                             against numpy, the batches through the scan and not the fused pass
    other paths              the Kafka decode, the per-message path, kta_reset, the refusals
    kta_exchange             the RCCL test double, 2 and 3 ranks, with and without -c
    kta-analyzer             kta.timeline=1m with a pinned start: the report unchanged, the section the restatement's,
                             with kta.analytics=1, kta.gpus=2, segment:// and kta.per_message=1"""
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
import analytics_py as AP
import timeline_py as T
from helpers import NOW, random_cols
from oracle_c import Oracle, analytics as oracle_analytics, kafka_decode

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
I64_MAX = int(np.iinfo(np.int64).max)
CHUNK = 1 << 22
THREADS = 16                          # the CPU allotment of a GPU machine, not os.cpu_count()


def _boundary_cols(origin, W, n, rng):
    end = origin + n * W
    edges = [-1, -5, 0, origin - 1, origin, origin + W - 1, origin + W, end - 1, end, I64_MAX, I64_MAX - 1,
             I64_MAX - W, end + W, origin + (n // 2) * W, origin + (n // 2) * W - 1]
    edges = [t for t in edges if t >= -5]
    m = 6000
    ts = np.concatenate([np.repeat(np.array(edges, np.int64), 40),
                         rng.integers(max(origin - 3 * W, 0), min(end + 3 * W, I64_MAX), size=m, dtype=np.int64)])
    rng.shuffle(ts)
    cols = random_cols(rng, len(ts), 5, tomb=0.25, null_key=0.2, big_sizes=True)
    cols["ts_ms"] = ts
    cols["partition"][rng.random(len(ts)) < 0.02] = -1           # bad partitions: counted as such, not placed
    cols["partition"][rng.random(len(ts)) < 0.02] = 5
    return cols


@pytest.mark.parametrize("W", [1, 7, 3_600_000, 1 << 40])
def test_boundary_timestamps_host_and_device_batches(W):
    rng = np.random.default_rng(W % 1000 + 11)
    origin = 1000 if W == 1 << 40 else 1_600_000_000_000
    n = 5 if W == 1 << 40 else 37
    cols = _boundary_cols(origin, W, n, rng)
    want = T.timeline_vector(cols, 5, origin, W, n)
    assert want[0, 0] and want[1, 0] and want[n + 2, 0] and want[2, 0] and want[n + 1, 0]
    assert int(want[:, 0].sum()) == int(((cols["partition"] >= 0) & (cols["partition"] < 5)).sum())
    # host batches through the staging ring (several batches: the capacity is small)
    with kta.HipMetricHandler(5, now=NOW, batch_capacity=1 << 11, timeline=(origin, W, n)) as h:
        h.submit_columns(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"])
        assert np.array_equal(h.timeline(), want)
        h.finish_device()
        assert np.array_equal(h.exchange_timeline(), want)
    # tile-compact device batches (tiles that do not fit the compact form stay raw), with analytics as well
    for analytics in (False, True):
        with kta.HipMetricHandler(5, now=NOW, analytics=analytics, timeline=(origin, W, n)) as h:
            b, nb = h.upload_batch(cols)
            h.submit_device(b, nb, 0, which=1)
            assert np.array_equal(h.timeline(), want), analytics
            h.sync()
            h.device_batch_free(b)


def test_compact_tiles_place_records_like_raw_ones():
    """An ordered stream (every tile compact) over bucket boundaries, and the same records in a raw batch."""
    rng = np.random.default_rng(5)
    n_rec = 1 << 16
    origin, W, n = 1_600_000_000_000, 7, 1024
    ts = origin - 100 + np.sort(rng.integers(0, 7 * 1100, size=n_rec)).astype(np.int64)
    ts[rng.random(n_rec) < 0.01] = -1
    cols = random_cols(rng, n_rec, 3, tomb=0.3)
    cols["ts_ms"] = ts
    want = T.timeline_vector(cols, 3, origin, W, n)
    with kta.HipMetricHandler(3, now=NOW, timeline=(origin, W, n)) as h:
        b, nb = h.upload_batch(cols)
        h.submit_device(b, nb, 0, which=1)
        assert np.array_equal(h.timeline(), want)
        h.sync()
        h.device_batch_free(b)
        h.reset()
        assert not h.timeline().any()                      # kta_reset zeroes the timeline and keeps it
        h.submit_columns(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"])
        assert np.array_equal(h.timeline(), want)


def _numpy_threaded(spec, n, P, tl):
    chunks = [(lo, min(CHUNK, n - lo)) for lo in range(0, n, CHUNK)]
    parts = [np.zeros((tl[2] + 3, 3), np.uint64) for _ in range(THREADS)]
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
                parts[t] += T.timeline_vector(kta.synth_fill_host(spec, *chunks[k]), P, *tl)
        except BaseException as e:   # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=work, args=(t,)) for t in range(THREADS)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errors, errors
    return sum(parts)


def test_timeline_config_4_2e30_records_tile_compact_bit_exact():
    sp, _ = kta.synth_preset("c4")
    n, P = 1 << 30, 256
    tl = (int(sp.ts_base_ms) - 30 * 60 * 1000, 10_000, 1024)
    want = _numpy_threaded(sp, n, P, tl)
    assert want[1, 0] and want[1026, 0] and want[0, 0] and int(want[:, 0].sum()) == n
    with kta.HipMetricHandler(P, now=NOW, timeline=tl) as h, kta.HipMetricHandler(P, now=NOW) as plain:
        b = h.device_batch_alloc(n)
        h.synth_fill_device(sp, 0, n, b)
        h.sync()                                           # (the other context's stream does not wait for h's)
        h.submit_device(b, n, 0, which=1)
        plain.submit_device(b, n, 0, which=1)
        res, c = h.finish()
        res0, c0 = plain.finish()
        h.device_batch_free(b)
        assert np.array_equal(h.timeline(), want) and np.array_equal(h.exchange_timeline(), want)
    assert np.array_equal(c, c0) and bytes(res) == bytes(res0) and res.overall_count == n


def test_c3_law_with_c_analytics_and_timeline_take_the_scan():
    sp, _ = kta.synth_preset("c3")
    n, P = 1 << 22, 64
    cols = kta.synth_fill_host(sp, 0, n, with_keys=True)
    tl = (int(sp.ts_base_ms) + 5_000, 1_000, 40)
    o = Oracle(NOW, count_alive_keys=True)
    o.run_soa(cols)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, batch_capacity=1 << 21, key_bytes_capacity=1 << 26,
                              analytics=True, timeline=tl) as h:
        h.submit_columns(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"], cols["key_off"],
                         cols["key_bytes"])
        res, c = h.finish()
        info = h.alive_pass_info()
        assert np.array_equal(c, o.counters(P)) and res.alive_keys == o.alive_keys()
        assert np.array_equal(h.exchange_timeline(), T.timeline_vector(cols, P, *tl))
        want_a = oracle_analytics(cols, P)
        got_a = h.exchange_analytics()
        for k in want_a:
            assert np.array_equal(np.asarray(got_a[k]), np.asarray(want_a[k])), k
    assert info["fuse"] and info["slices"] > 0 and info["fused"] == 0


def test_kafka_decode_and_per_message_paths():
    from kafka_cases import random_record_set
    lib = N.load()
    rng = np.random.default_rng(42)
    P = 4
    blobs, decoded = [], []
    for fetch in range(6):
        part = fetch % P
        blob, _, _ = random_record_set(rng, 50, partition=part, key_space=80)
        cols, _ = kafka_decode(blob, part)
        blobs.append((blob, part))
        decoded.append({k: v for k, v in cols.items() if k != "offset"})
    allc = {k: np.concatenate([d[k] for d in decoded]) for k in ("partition", "key_len", "val_len", "ts_ms")}
    ts = allc["ts_ms"][allc["ts_ms"] >= 0]
    tl = (int(np.percentile(ts, 10)), max(int(ts.max() - ts.min()) // 50, 1), 60)
    want = T.timeline_vector(allc, P, *tl)
    with kta.HipMetricHandler(P, now=NOW, timeline=tl) as h:
        for blob, part in blobs:
            st = N.KtaKafkaIndexStats()
            h._check(lib.kta_kafka_consume(h._ctx, blob, len(blob), part, C.byref(st)))
        assert np.array_equal(h.timeline(), want)
    with kta.HipMetricHandler(P, now=NOW, batch_capacity=1 << 10, timeline=tl) as h:
        h.replay_messages(allc)
        assert np.array_equal(h.timeline(), want)             # (kta_get_timeline flushes the staged messages)
        h.reset()
        sub = {k: v[:100] for k, v in allc.items()}
        h.replay_messages(sub)
        assert np.array_equal(h.timeline(), T.timeline_vector(sub, P, *tl))


def test_refusals():
    with kta.HipMetricHandler(3, now=NOW) as h:
        for fn in (lambda: h.timeline(), lambda: h.exchange_timeline(), lambda: h.timeline_vector(),
                   lambda: h.timeline_result_vector()):
            with pytest.raises(kta.KtaError, match="no timeline"):
                fn()
        for bad in ((-1, 10, 5), (0, 0, 5), (0, 10, 0), (0, 10, 1025), (I64_MAX - 10, 10, 2), (0, I64_MAX // 3, 4)):
            with pytest.raises(kta.KtaError):
                h.set_timeline(*bad)
        h.set_timeline(0, 10, 4)
        h.set_timeline(100, 10, 8)                         # again, before any record
        h.submit_columns(np.array([0], np.int32), np.array([1], np.int32), np.array([1], np.int32),
                         np.array([105], np.int64))
        with pytest.raises(kta.KtaError, match="handed records"):
            h.set_timeline(0, 10, 4)
        assert h.timeline()[2, 0] == 1 and h.timeline().shape == (11, 3)
        h.reset()
        h.set_timeline(0, 10, 4)                           # after kta_reset: accepted
    big = kta.timeline_max_partitions(1024, analytics=True)
    with kta.HipMetricHandler(big + 1, now=NOW, analytics=True) as h:
        with pytest.raises(kta.KtaError, match="admits at most"):
            h.set_timeline(0, 10, 1024)
        h.set_timeline(0, 10, 1)


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
import timeline_py as T
from helpers import NOW, random_cols

P = 7
TL = (1_600_000_000_000 - 200_000_000, 5_000_000, 100)
rng = np.random.default_rng(29)
cols = random_cols(rng, 120000, P, key_space=3000, tomb=0.3, big_sizes=True)
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

tv = lambda idx: T.timeline_vector(subset(idx), P, *TL)
want = {"first": tv(np.arange(half)), "all": tv(np.arange(n))}

for nranks in (2, 3):
    for with_c in (False, True):
        uid = kta.HipMetricHandler.comm_unique_id()
        errors = []
        def run(rank):
            try:
                h = kta.HipMetricHandler(P, count_alive_keys=with_c, now=NOW, seq_column=with_c, timeline=TL)
                h.comm_create(nranks, rank, uid)
                mine = cols["partition"] % nranks == rank
                for stage, idx in (("first", np.arange(half)[mine[:half]]), ("all", np.arange(half, n)[mine[half:]])):
                    sh = subset(idx)
                    if not with_c:
                        del sh["seq"]
                    b, nb = h.upload_batch(sh, with_keys=with_c)
                    h.submit_device(b, nb, 0)
                    h.exchange()
                    assert np.array_equal(h.exchange_timeline(), want[stage]), (nranks, with_c, rank, stage, "exchanged")
                    own = np.nonzero(mine[:half if stage == "first" else n])[0]
                    assert np.array_equal(h.timeline(), tv(own)), (nranks, with_c, rank, stage, "own")
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


def test_exchange_timeline_on_two_and_three_ranks_with_and_without_c(tmp_path, mock_rccl):
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
    at = stdout.index("Timeline, ")
    return stdout[:at], stdout[at:]


START = 1_600_000_000 - 120          # kta.timeline.start (unix seconds): the c2 topic starts 2 minutes later


def test_cli_timeline_section_single_sharded_per_message_analytics(mock_rccl):
    src = "synthetic://c2?records=250000"
    sp, _ = kta.synth_preset("c2")
    cols = kta.synth_fill_host(sp, 0, 250000)
    P = int(sp.n_partitions)
    tl = (START * 1000, 60_000, 168)
    want = T.section(T.timeline_vector(cols, P, *tl), *tl)
    knob = "kta.timeline=1m,kta.timeline.start=%d" % START
    plain = _cli("-t", "c2", "-b", src)
    assert plain.returncode == 0, plain.stderr
    one = _cli("-t", "c2", "-b", src, "--librdkafka", knob)
    assert one.returncode == 0, one.stderr
    report, section = _split(one.stdout)
    assert section == want and _normalise(report) == _normalise(plain.stdout)
    both = _cli("-t", "c2", "-b", src, "--librdkafka", "kta.analytics=1," + knob)
    assert both.returncode == 0, both.stderr
    report2, section2 = _split(both.stdout)
    assert section2 == want
    at = report2.index("Size histograms and per-partition extrema")
    assert _normalise(report2[:at]) == _normalise(plain.stdout)
    assert report2[at:] == AP.section(oracle_analytics(cols, P))
    env = dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl)
    for c in ([], ["-c"]):
        many = _cli("-t", "c2", "-b", src, *c, "--librdkafka", knob + ",kta.gpus=2,kta.batch=32768,kta.oversubscribe=1",
                    env=env)
        assert many.returncode == 0, (c, many.stderr[-2000:])
        assert many.stdout.count("Timeline, ") == 1 and _split(many.stdout)[1] == want, c
    pm = _cli("-t", "c2", "-b", src, "--librdkafka", knob + ",kta.per_message=1,kta.batch=4096")
    assert pm.returncode == 0, pm.stderr
    assert _split(pm.stdout)[1] == want
    # without kta.timeline.start the last bucket holds the run's start: the whole c2 topic (2020) is "before"
    now = _cli("-t", "c2", "-b", src, "--librdkafka", "kta.timeline=1h")
    assert now.returncode == 0 and now.stdout.count("Timeline, 1h buckets from ") == 1
    assert re.search(r"^\| Before [^|]+\| 2[0-9]{5} ", now.stdout, flags=re.M)


def test_cli_timeline_section_on_raw_kafka_log_segments(tmp_path):
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
    ts = cols["ts_ms"][cols["ts_ms"] >= 0]
    start = int(np.percentile(ts, 20)) // 1000
    width_s = max((int(ts.max()) // 1000 - start) // 30, 1)
    tl = (start * 1000, width_s * 1000, 40)
    want = T.section(T.timeline_vector(cols, 4, *tl), *tl)
    r = _cli("-t", "seg", "-b", "segment://" + ",".join(files), "--librdkafka",
             "kta.timeline=%d,kta.timeline.buckets=40,kta.timeline.start=%d" % (width_s, start))
    assert r.returncode == 0, r.stderr
    report, section = _split(r.stdout)
    assert section == want
    plain = _cli("-t", "seg", "-b", "segment://" + ",".join(files))
    assert plain.returncode == 0 and _normalise(plain.stdout) == _normalise(report)

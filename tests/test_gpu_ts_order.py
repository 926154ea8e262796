"""GPU tests of the timestamp-order pass (KTA_FLAG_TS_ORDER): the device vector is held bit for bit against the numpy
restatement in tests/ts_order_py.py (written from the definition in include/kta_hip.h) — single instructions, chunks and
launches, the carry across batches, both layouts and every submission path, P up to the bound, the three laws, the
exchange on the RCCL test double and the CLI section."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import analytics_py as AP
import timeline_py as TL
import ts_order_py as T
from helpers import NOW
from oracle_c import Oracle, analytics as oracle_analytics

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
I63 = (1 << 63) - 1
BASE = 1_600_000_000_000
SIZES = (("partition", 4), ("key_len", 4), ("val_len", 4), ("ts_ms", 8))


def _cols(part, ts, rng=None):
    n = len(part)
    rng = rng or np.random.default_rng(n)
    return {"partition": np.ascontiguousarray(part, np.int32), "ts_ms": np.ascontiguousarray(ts, np.int64),
            "key_len": rng.integers(-1, 40, n).astype(np.int32), "val_len": rng.integers(-1, 500, n).astype(np.int32)}


def _submit(h, cols):
    h.submit_columns(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"])


def _device(h, cols, which=1):
    b, nb = h.upload_batch(cols)
    h.submit_device(b, nb, 0, which=which)
    h.sync()
    h.device_batch_free(b)


def _vec(h):
    return h.ts_order()["vector"]


def _ramp(rng, n, P, jitter=5000, none=0.02, bad=0.02, step=10):
    part = rng.integers(0, P, n).astype(np.int32)
    ts = BASE + np.arange(n, dtype=np.int64) * step + rng.integers(-jitter, jitter + 1, n)
    ts[rng.random(n) < none] = -1
    m = rng.random(n) < bad
    part[m] = np.where(rng.random(int(m.sum())) < 0.5, -1, P)
    return part, ts


# ------------------------------------------------------------------------------------------ one instruction
def _instruction_cases(P, n):
    rng = np.random.default_rng(100 * P + n)
    ramp = BASE + np.arange(n, dtype=np.int64) * 3
    out = {"descending": (np.full(n, P - 1), ramp[::-1].copy()), "ascending": (np.full(n, 0), ramp),
           "equal": (np.full(n, P // 2), np.full(n, 777, np.int64)),
           "distinct": (np.arange(n) % P, ramp + rng.integers(-500, 500, n)),
           "alternating": ((np.arange(n) & 1) % P, ramp + rng.integers(-2000, 2000, n)),
           "random": (rng.integers(0, P, n), ramp + rng.integers(-3000, 3000, n)),
           "extremes": (rng.integers(0, P, n), rng.choice(np.array([0, I63, 1, I63 - 1], np.int64), n))}
    part, ts = rng.integers(0, P, n), ramp + rng.integers(-3000, 3000, n)
    kind = rng.integers(0, 9, n)
    out["a third invalid"] = (np.where(kind == 1, -1, np.where(kind == 2, P, part)), np.where(kind == 0, -1, ts))
    return out


@pytest.mark.parametrize("n", [64, 65])
@pytest.mark.parametrize("P", [1, 3, 64])
def test_one_instruction_host_and_device_batches(P, n):
    with kta.HipMetricHandler(P, now=NOW, ts_order=True) as h:
        for name, (part, ts) in _instruction_cases(P, n).items():
            cols = _cols(part, ts)
            want = T.vector_of(P, cols["partition"], cols["ts_ms"])
            h.reset()
            _submit(h, cols)
            assert np.array_equal(_vec(h), want), (name, "host batch")
            h.reset()
            _device(h, cols)
            assert np.array_equal(_vec(h), want), (name, "device batch")
    assert T.vector_of(3, [0] * 64, list(range(64, 0, -1)))[0] == 63          # (the cases do hold late records)


# ------------------------------------------------------------------------------------------ chunks and launches
def test_chunks_and_launches():
    rng = np.random.default_rng(2)
    P, n = 5, 50_000
    part, ts = _ramp(rng, n, P)
    cols = _cols(part, ts)
    want = T.vector_of(P, part, ts)
    assert want[0] > 1000 and want[2 * P + 63] < n
    # partition 0: its only early maximum in the first chunk, its late records in the last, nothing between
    part2 = rng.integers(1, P, n).astype(np.int32)
    ts2 = BASE + np.arange(n, dtype=np.int64) + rng.integers(-50, 50, n)
    part2[:40], ts2[10] = 0, BASE + 10_000_000
    part2[-30:] = 0
    cols2 = _cols(part2, ts2)
    want2 = T.vector_of(P, part2, ts2)
    assert want2[0] >= 30 + 29 and int(want2[2 * P + 64]) > 9_000_000
    with kta.HipMetricHandler(P, now=NOW, ts_order=True) as h:
        for chunk in (64, 0, 128, 4096):
            for c, w in ((cols, want), (cols2, want2)):
                h.reset()
                h.set_ts_order_chunk(chunk)
                _device(h, c)
                assert np.array_equal(_vec(h), w), chunk
                info = h.ts_order_info()
                if chunk:
                    assert info["chunk_records"] == chunk and info["chunks"] == -(-n // chunk)
                h.reset()
                _submit(h, c)
                assert np.array_equal(_vec(h), w), (chunk, "host")
        for bad in (1, 63, 100):
            with pytest.raises(kta.KtaError, match="multiple of 64"):
                h.set_ts_order_chunk(bad)


# ------------------------------------------------------------------------------------------ carry across batches
def test_carry_across_batches_and_submission_paths():
    rng = np.random.default_rng(3)
    P, n = 4, 9000
    part, ts = _ramp(rng, n, P, jitter=20_000)
    cols = _cols(part, ts)
    want = T.vector_of(P, part, ts)
    with kta.HipMetricHandler(P, now=NOW, ts_order=True) as h:
        _submit(h, cols)
        assert np.array_equal(_vec(h), want)
        for cut in (1, 63, 64, 65, 1023, 1025, 4097):
            for path in (_submit, _device):
                h.reset()
                for lo, hi in ((0, cut), (cut, n)):
                    path(h, {k: v[lo:hi] for k, v in cols.items()})
                assert np.array_equal(_vec(h), want), (cut, path.__name__)
        h.reset()                                                           # many batches of 1025
        for lo in range(0, n, 1025):
            _device(h, {k: v[lo:lo + 1025] for k, v in cols.items()})
        assert np.array_equal(_vec(h), want)
    with kta.HipMetricHandler(P, now=NOW, ts_order=True, batch_capacity=2048) as h:   # the staging ring
        _submit(h, cols)
        assert np.array_equal(_vec(h), want)
        h.reset()
        h.replay_messages(cols)
        assert np.array_equal(_vec(h), want)
        h.reset()
        m = 2000
        for i in range(m):                                                  # handle_message one by one
            t = int(ts[i])
            h.handle_message(kta.Message(int(part[i]), None if t == -1 else t, b"k", 3))
        assert np.array_equal(_vec(h), T.vector_of(P, part[:m], ts[:m]))


# ------------------------------------------------------------------------------------------ layouts
def _tile_modes(h, b, tiles):
    raw = np.zeros(tiles * 4, np.uint32)
    h._check(h._lib.kta_copy_to_host(h._ctx, C.c_void_p(raw.ctypes.data), b.tile_hdr, raw.nbytes))
    return raw[2::4]


def test_layouts_compact_raw_mixed_and_a_view():
    rng = np.random.default_rng(4)
    P, n = 3, 1 << 15
    part = rng.integers(0, P, n).astype(np.int32)
    ts = BASE + np.sort(rng.integers(0, 50_000, n)).astype(np.int64)
    ts[rng.random(n) < 0.3] -= 700                                         # late records inside compact tiles
    ts[rng.random(n) < 0.01] = -1
    cols = _cols(part, ts)
    want = T.vector_of(P, part, ts)
    assert want[0] > 100
    with kta.HipMetricHandler(P, now=NOW, ts_order=True) as h:
        b, nb = h.upload_batch(cols)
        assert b.layout == N.KTA_LAYOUT_TILE_COMPACT and (_tile_modes(h, b, n // 1024) == N.KTA_TILE_COMPACT).all()
        h.submit_device(b, nb, 0, which=1)
        assert np.array_equal(_vec(h), want)
        # a view that starts inside a tile of the allocation: records [lo, n)
        for lo in (4, 1000, 1024 + 36):
            h.reset()
            v = kta.KtaBatch()
            for f, sz in SIZES:
                setattr(v, f, getattr(b, f) + lo * sz)
            h.submit_device(v, n - lo, 0, which=1)
            assert np.array_equal(_vec(h), T.vector_of(P, part[lo:], ts[lo:])), lo
        h.sync()
        h.device_batch_free(b)
        h.reset()
        _submit(h, cols)                                                   # the same records in a raw batch
        assert np.array_equal(_vec(h), want)
        # tiles that do not fit the compact form, timestamps next to INT64_MAX
        ts2 = ts.copy()
        wide = (np.arange(n) // 1024) % 2 == 1
        ts2[wide & (rng.random(n) < 0.1)] = I63 - rng.integers(0, 1000)
        ts2[wide & (rng.random(n) < 0.05)] = I63
        part2 = part.copy()
        part2[(np.arange(n) // 1024 == 4) & (rng.random(n) < 0.1)] = 70_000        # a partition id the u16 form cannot hold
        cols2 = _cols(part2, ts2)
        want2 = T.vector_of(P, part2, ts2)
        h.reset()
        b, nb = h.upload_batch(cols2)
        modes = _tile_modes(h, b, n // 1024)
        assert (modes == N.KTA_TILE_RAW).any() and (modes == N.KTA_TILE_COMPACT).any()
        h.submit_device(b, nb, 0, which=1)
        assert np.array_equal(_vec(h), want2) and int(want2[2 * P + 64:].max()) > (1 << 62)
        h.sync()
        h.device_batch_free(b)


# ------------------------------------------------------------------------------------------ P
@pytest.mark.parametrize("P", [1, 256, 1024, 4096])
def test_partition_counts(P):
    if P > kta.ts_order_max_partitions():
        with pytest.raises(kta.KtaError, match="KTA_FLAG_TS_ORDER admits at most %d" % kta.ts_order_max_partitions()):
            kta.HipMetricHandler(P, now=NOW, ts_order=True)
        return
    rng = np.random.default_rng(P)
    n = 1 << 16
    part, ts = _ramp(rng, n, P, jitter=200_000)
    cols = _cols(part, ts)
    want = T.vector_of(P, part, ts)
    assert want[:2 * P:2].sum() > n // 8
    with kta.HipMetricHandler(P, now=NOW, ts_order=True) as h:
        _device(h, cols)
        assert np.array_equal(_vec(h), want)
        h.reset()
        h.set_ts_order_chunk(256)
        _submit(h, cols)
        assert np.array_equal(_vec(h), want)


def test_refusal_above_the_bound_comes_before_any_launch():
    lib = N.load()
    bound = kta.ts_order_max_partitions()
    assert bound >= 1024
    cfg = N.KtaConfig(0, bound + 1, 0, 0, 0, 0, N.KTA_FLAG_TS_ORDER, 0)
    ctx = C.c_void_p()
    assert lib.kta_create(C.byref(cfg), C.byref(ctx)) == N.KTA_ERR_INVALID and not ctx.value   # no context, so no launch
    with kta.HipMetricHandler(3, now=NOW) as h:
        for fn in (h.ts_order, h.exchange_ts_order, h.ts_order_result_vector, h.ts_order_info, lambda: h.set_ts_order_chunk(64)):
            with pytest.raises(kta.KtaError, match="KTA_FLAG_TS_ORDER"):
                fn()


# ------------------------------------------------------------------------------------------ laws
LAW_N, LAW_PIECE = 1 << 24, 1 << 22


def _law(sp, P):
    """(device vector, info, restatement fed in pieces with carry) of the first 2^24 records, tile-compact on the device"""
    t = T.TsOrder(P)
    for lo in range(0, LAW_N, LAW_PIECE):
        c = kta.synth_fill_host(sp, lo, LAW_PIECE)
        t.feed(c["partition"], c["ts_ms"])
    with kta.HipMetricHandler(P, now=NOW, ts_order=True) as h:
        b = h.device_batch_alloc(LAW_N)
        h.synth_fill_device(sp, 0, LAW_N, b)
        h.submit_device(b, LAW_N, 0, which=1)
        got, info = h.ts_order(), h.ts_order_info()
        h.sync()
        h.device_batch_free(b)
    return got, info, t.vector()


def test_law_config_4_random_partitions_nearly_every_record_late():
    sp, _ = kta.synth_preset("c4")
    P = int(sp.n_partitions)
    got, info, want = _law(sp, P)
    assert np.array_equal(got["vector"], want)
    assert got["timed"] > 0 and int(got["late"].sum()) > got["timed"] // 2
    assert info["groups"] > 0 and info["instructions"] >= got["timed"] // 64


def test_law_config_4_partition_runs_without_jitter_nothing_late():
    sp, _ = kta.synth_preset("c4")
    sp.part_mode, sp.part_run_len, sp.ts_jitter_ms = N.KTA_PART_RUNS, 500, 0
    P = int(sp.n_partitions)
    got, info, want = _law(sp, P)
    assert np.array_equal(got["vector"], want)
    assert not got["late"].any() and not got["hist"].any() and got["timed"] > 0
    assert info["one_partition"] > info["instructions"] // 2           # runs of 500: most instructions hold one partition


def test_law_config_3_with_c_fused_pass_still_taken_and_right():
    sp, _ = kta.synth_preset("c3")
    P, n = int(sp.n_partitions), LAW_N
    cols = kta.synth_fill_host(sp, 0, n, with_keys=True)
    o = Oracle(NOW, count_alive_keys=True)
    o.run_soa(cols)
    t = T.TsOrder(P)
    for lo in range(0, n, LAW_PIECE):
        t.feed(cols["partition"][lo:lo + LAW_PIECE], cols["ts_ms"][lo:lo + LAW_PIECE])
    want = t.vector()
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, batch_capacity=1 << 21, key_bytes_capacity=1 << 26,
                              ts_order=True) as h:
        h.submit_columns(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"], cols["key_off"], cols["key_bytes"])
        res, c = h.finish()
        info = h.alive_pass_info()
        assert np.array_equal(c, o.counters(P)) and res.alive_keys == o.alive_keys()
        assert np.array_equal(_vec(h), want) and np.array_equal(h.exchange_ts_order()["vector"], want)
    assert info["fuse"] and info["slices"] > 0 and info["fused"] > 0


# ------------------------------------------------------------------------------------------ nothing else moves
def test_nothing_else_moves_reset_and_which_2():
    rng = np.random.default_rng(6)
    P, n = 6, 20_000
    part, ts = _ramp(rng, n, P)
    cols = _cols(part, ts)
    with kta.HipMetricHandler(P, now=NOW, ts_order=True) as h, kta.HipMetricHandler(P, now=NOW) as plain:
        for x in (h, plain):
            _submit(x, cols)
            _device(x, cols)
        res, c = h.finish(allow_bad_partition=True)
        res0, c0 = plain.finish(allow_bad_partition=True)
        assert np.array_equal(c, c0) and bytes(res) == bytes(res0)
        assert np.array_equal(h.exchange_ts_order()["vector"], T.TsOrder(P).feed(part, ts).feed(part, ts).vector())
        h.reset()
        assert not _vec(h).any()
        # hi is cleared too: a first record older than the maximum before the reset is not late
        one = _cols(np.array([0, 0]), np.array([5, 4]))
        _submit(h, one)
        v = h.ts_order()
        assert v["timed"] == 2 and list(v["late"][:1]) == [1] and int(v["late_ms_sum"][0]) == 1
        before = _vec(h).copy()
        _device(h, cols, which=2)                                        # the alive-key handler alone: nothing
        assert np.array_equal(_vec(h), before)


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
import ts_order_py as T
from helpers import NOW, random_cols

P = 7
rng = np.random.default_rng(31)
cols = random_cols(rng, 60000, P, key_space=3000, tomb=0.3)
n = len(cols["partition"])
cols["ts_ms"] = 1_600_000_000_000 + np.arange(n, dtype=np.int64) * 7 + rng.integers(-4000, 4000, n)
cols["ts_ms"][rng.random(n) < 0.02] = -1
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

want = {"first": T.vector_of(P, cols["partition"][:half], cols["ts_ms"][:half]), "all": T.vector_of(P, cols["partition"], cols["ts_ms"])}

for nranks in (2, 3):
    for with_c in (False, True):
        uid = kta.HipMetricHandler.comm_unique_id()
        errors = []
        def run(rank):
            try:
                h = kta.HipMetricHandler(P, count_alive_keys=with_c, now=NOW, seq_column=with_c, ts_order=True)
                h.comm_create(nranks, rank, uid)
                mine = cols["partition"] % nranks == rank
                for stage, idx in (("first", np.arange(half)[mine[:half]]), ("all", np.arange(half, n)[mine[half:]])):
                    sh = subset(idx)
                    if not with_c:
                        del sh["seq"]
                    b, nb = h.upload_batch(sh, with_keys=with_c)
                    h.submit_device(b, nb, 0)
                    for again in range(2):                     # a second exchange counts nothing twice
                        h.exchange()
                        assert np.array_equal(h.exchange_ts_order()["vector"], want[stage]), (nranks, with_c, rank, stage, again)
                    upto = half if stage == "first" else n
                    own = np.nonzero(mine[:upto])[0]
                    assert np.array_equal(h.ts_order()["vector"], T.vector_of(P, cols["partition"][own], cols["ts_ms"][own])), "own"
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


def test_exchange_on_two_and_three_ranks_with_and_without_c(tmp_path, mock_rccl):
    script = tmp_path / "exchange_worker.py"
    script.write_text(_EXCHANGE_WORKER)
    env = dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(script), ROOT], capture_output=True, text=True,
                       timeout=330, env=env)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count(" OK") == 4


# ------------------------------------------------------------------------------------------ the CLI
def _cli(*args, env=None):
    return subprocess.run(["timeout", "-k", "10", "240", CLI, *args], capture_output=True, text=True, timeout=270, env=env)


def _normalise(text):
    text = re.sub(r"Scanning took: \d+ seconds", "Scanning took: 3 seconds", text)
    return re.sub(r"Estimated Msg/s: \d+", "Estimated Msg/s: 133", text)


def _split(stdout):
    at = stdout.index("Timestamp order: ")
    return stdout[:at], stdout[at:]


def test_cli_section_single_sharded_per_message_and_with_the_other_sections(mock_rccl):
    src = "synthetic://c2?records=200000"
    sp, _ = kta.synth_preset("c2")
    cols = kta.synth_fill_host(sp, 0, 200000)
    P = int(sp.n_partitions)
    records = np.bincount(cols["partition"], minlength=P)
    want = T.section(T.vector_of(P, cols["partition"], cols["ts_ms"]), records)
    plain = _cli("-t", "c2", "-b", src)
    assert plain.returncode == 0, plain.stderr
    assert "Timestamp order" not in plain.stdout
    off = _cli("-t", "c2", "-b", src, "--librdkafka", "kta.ts_order=0")
    assert off.returncode == 0 and _normalise(off.stdout) == _normalise(plain.stdout)
    one = _cli("-t", "c2", "-b", src, "--librdkafka", "kta.ts_order=1")
    assert one.returncode == 0, one.stderr
    report, section = _split(one.stdout)
    assert section == want and _normalise(report) == _normalise(plain.stdout)
    env = dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl)
    for c in ([], ["-c"]):
        many = _cli("-t", "c2", "-b", src, *c, "--librdkafka", "kta.ts_order=1,kta.gpus=2,kta.batch=32768,kta.oversubscribe=1", env=env)
        assert many.returncode == 0, (c, many.stderr[-2000:])
        assert many.stdout.count("Timestamp order: ") == 1 and _split(many.stdout)[1] == want, c
    pm = _cli("-t", "c2", "-b", src, "--librdkafka", "kta.ts_order=1,kta.per_message=1,kta.batch=4096")
    assert pm.returncode == 0, pm.stderr
    assert _split(pm.stdout)[1] == want
    start = 1_600_000_000 - 120
    tl = (start * 1000, 60_000, 168)
    both = _cli("-t", "c2", "-b", src, "--librdkafka", "kta.analytics=1,kta.ts_order=1,kta.timeline=1m,kta.timeline.start=%d" % start)
    assert both.returncode == 0, both.stderr
    head, section2 = _split(both.stdout)
    assert section2 == want
    at = head.index("Size histograms and per-partition extrema")
    assert _normalise(head[:at]) == _normalise(plain.stdout)
    assert head[at:] == AP.section(oracle_analytics(cols, P)) + TL.section(TL.timeline_vector(cols, P, *tl), *tl)

"""GPU tests of the segment pass of the retention what-if (kta_set_segments): the device vector is held bit for bit against
the pure-Python restatement in tests/segments_py.py (a sequential loop written from the definition in include/kta_hip.h),
and in every test the identities with the context's own counter vector hold — single instructions, chunks and launches
with the skip of chunks that close nothing, the carry across batches and kta_reset, sizes that pass 2^32 in one chunk,
records larger than a segment, a clamped partition, both layouts and every tile form, a view, every submission path, P up
to the bound, and every opt-in pass at once."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import hot_keys_py as HK
import key_sketch_py as KS
import partitioner_py as R
import segments_py as SP
import timeline_py as TL
import ts_order_py as TS
from helpers import NOW, random_cols

pytestmark = pytest.mark.gpu

BASE = 1_600_000_000_000
SIZES = (("partition", 4), ("key_len", 4), ("val_len", 4), ("ts_ms", 8))


def _cols(seed, n, P, max_key=40, max_val=500, bad=0.02, none=0.02, jitter=5000):
    rng = np.random.default_rng(seed)
    part = rng.integers(0, P, n).astype(np.int32)
    m = rng.random(n) < bad
    part[m] = np.where(rng.random(int(m.sum())) < 0.5, -1, P)
    ts = BASE + np.arange(n, dtype=np.int64) * 10 + rng.integers(-jitter, jitter + 1, n)
    ts[rng.random(n) < none] = -1
    return {"partition": part, "key_len": rng.integers(-1, max_key, n).astype(np.int32),
            "val_len": rng.integers(-1, max_val, n).astype(np.int32), "ts_ms": ts}


def _cut(cols, lo, hi):
    return {k: v[lo:hi] for k, v in cols.items()}


def _want(cols, P, cfg, into=None):
    return SP.segments_vector(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"], P, *cfg, into=into)


def _submit(h, cols):
    h.submit_columns(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"])


def _device(h, cols, which=1):
    b, nb = h.upload_batch(cols)
    h.submit_device(b, nb, 0, which=which)
    h.sync()
    h.device_batch_free(b)


def _hold(h, want, P):
    """the live vector is `want`, and the identities hold against the context's own counter vector"""
    got = h.segments()
    assert np.array_equal(got["vector"], want)
    h.finish(allow_bad_partition=True)
    cv = h.result_vector_host()
    c, g = cv[:P * 7].reshape(P, 7), cv[P * 7:]
    t, gl = got["totals"], got["globals"]
    overhead = int(gl[5])
    assert np.array_equal(t[:, 0], c[:, N.KTA_C_TOTAL]) and np.array_equal(t[:, 2], c[:, N.KTA_C_TOMBSTONES])
    assert np.array_equal(t[:, 1] - np.uint64(overhead) * t[:, 0], c[:, N.KTA_C_KEY_SIZE_SUM] + c[:, N.KTA_C_VALUE_SIZE_SUM])
    # (KTA_G_RECORDS counts the records inside [0, P) only — overall_count —, so global 0 equals it as it is)
    assert int(gl[0]) == int(g[N.KTA_G_RECORDS]) and int(gl[1]) == int(g[N.KTA_G_BAD_PARTITION])
    return got


# ------------------------------------------------------------------------------------------ one instruction
@pytest.mark.parametrize("n", [64, 65])
@pytest.mark.parametrize("P", [1, 3, 64])
def test_one_instruction_host_and_device_batches(P, n):
    rng = np.random.default_rng(100 * P + n)
    cases = {"one partition": np.full(n, P - 1), "distinct": np.arange(n) % P, "alternating": (np.arange(n) & 1) % P,
             "random": rng.integers(0, P, n), "a third outside": np.where(rng.random(n) < 1 / 3, rng.choice([-1, P], n), rng.integers(0, P, n))}
    closed = 0
    for S in (1, 100, 1 << 40):
        cfg = (S, 8, 2)
        with kta.HipMetricHandler(P, now=NOW, segments=cfg) as h:
            for name, part in cases.items():
                cols = _cols(n + len(name), n, P, bad=0)
                cols["partition"] = part.astype(np.int32)
                want = _want(cols, P, cfg)
                closed += int(SP.split(want, P, 8)["globals"][2])
                h.reset()
                _submit(h, cols)
                _hold(h, want, P)
                h.reset()
                _device(h, cols)
                _hold(h, want, P)
        if S == 1 << 40:
            assert not SP.split(want, P, 8)["rows"].any()
    assert closed > 0                                                      # (the cases do close rows)


# ------------------------------------------------------------------------------------------ chunks and launches
def test_chunks_and_launches_and_the_skip():
    P, n = 5, 50_000
    cols = _cols(2, n, P)
    cfg = (50_000, 64, 7)
    want = _want(cols, P, cfg)
    assert 100 < int(SP.split(want, P, 64)["globals"][2]) < P * 63
    # exactly one partition crossing, in one known chunk: partition 0 has 12 records of 2^27 - 1 bytes, the 9th of which —
    # record 30 000, in chunk 30 000 // 4096 = 7 of 13 — takes it past S = 2^30; every other partition stays below S
    big = (1 << 30, 4, 0)
    one = _cols(3, n, P, max_key=20, max_val=100, bad=0)
    one["partition"] = np.random.default_rng(4).integers(1, P, n).astype(np.int32)
    at = np.array([10, 500, 5000, 9000, 15000, 20000, 25000, 29000, 30000, 35000, 40000, 49999])
    one["partition"][at] = 0
    one["val_len"][at] = (1 << 27) - 1
    one["key_len"][at] = -1
    want_one = _want(one, P, big)
    s = SP.split(want_one, P, 4)
    assert int(s["globals"][2]) == 1 and int(s["rows"][0][0][0]) == 9 and int(s["totals"][:, 1].max()) == 12 * ((1 << 27) - 1)
    with kta.HipMetricHandler(P, now=NOW, segments=cfg) as h:
        for chunk in (64, 0, 128, 4096):
            h.reset()
            h.set_segments_chunk(chunk)
            _device(h, cols)
            _hold(h, want, P)
            info = h.segments_info()
            if chunk:
                assert info["chunk_records"] == chunk and info["chunks"] == -(-n // chunk)
            assert info["chunks_applied"] + info["chunks_skipped"] == info["chunks"] and info["chunks_applied"] > 0
            h.reset()
            _submit(h, cols)
            _hold(h, want, P)
        for bad in (1, 63, 100):
            with pytest.raises(kta.KtaError, match="multiple of 64"):
                h.set_segments_chunk(bad)
    with kta.HipMetricHandler(P, now=NOW, segments=big) as h:
        h.set_segments_chunk(4096)
        _device(h, one)
        _hold(h, want_one, P)
        info = h.segments_info()
        assert info["chunks"] == 13 and info["chunks_applied"] == 1 and info["chunks_skipped"] == 12


# ------------------------------------------------------------------------------------------ carry across batches, reset
def test_carry_across_three_batches_and_reset():
    P, n = 4, 9000
    cols = _cols(5, n, P, jitter=20_000)
    cfg = (3000, 200, 1)
    want = _want(cols, P, cfg)
    with kta.HipMetricHandler(P, now=NOW, segments=cfg) as h:
        for cuts in ((1, 63), (64, 65), (1023, 4097), (3000, 6000)):
            for path in (_submit, _device):
                h.reset()
                for lo, hi in zip((0,) + cuts, cuts + (n,)):
                    path(h, _cut(cols, lo, hi))
                _hold(h, want, P)
        h.reset()                                                          # the state is cleared, the configuration kept
        got = h.segments()
        assert list(got["globals"]) == [0, 0, 0, 3000, 200, 1, 0, 0] and not got["vector"][:-8].any()
        _device(h, _cut(cols, 0, 100))
        _hold(h, _want(_cut(cols, 0, 100), P, cfg), P)
        with pytest.raises(kta.KtaError, match="handed records"):          # refused after the first record
            h.set_segments(5000, 10, 0)
        h.reset()
        h.set_segments(5000, 10, 0)                                        # another M: a vector of another length
        _device(h, cols)
        _hold(h, _want(cols, P, (5000, 10, 0)), P)


# ------------------------------------------------------------------------------------------ sizes
def test_lengths_of_int32_max_a_record_larger_than_s_and_a_clamped_partition():
    P, n = 3, 5000
    rng = np.random.default_rng(6)
    cols = _cols(6, n, P)
    huge = rng.random(n) < 0.5
    cols["key_len"][huge] = 2**31 - 1
    cols["val_len"][huge & (rng.random(n) < 0.7)] = 2**31 - 1
    cfg = (1 << 33, 1000, 0)                                               # B passes 2^32 within every chunk of 64
    want = _want(cols, P, cfg)
    assert int(SP.split(want, P, 1000)["totals"][:, 1].min()) > 1 << 40
    with kta.HipMetricHandler(P, now=NOW, segments=cfg) as h:
        _device(h, cols)
        _hold(h, want, P)
        h.reset()
        _submit(h, cols)
        _hold(h, want, P)
    # records of 3 S + 1 bytes skip rows: they stay zero between closed ones
    cols = _cols(7, 3000, P, max_val=90)
    cols["val_len"][::100] = 3 * 1000 + 1
    cfg = (1000, 400, 0)
    want = _want(cols, P, cfg)
    rows = SP.split(want, P, 400)["rows"]
    used = int(max(np.nonzero(rows[0][:, 0])[0]))
    assert (rows[0][:used, 0] == 0).sum() >= 6
    with kta.HipMetricHandler(P, now=NOW, segments=cfg) as h:
        _device(h, cols)
        _hold(h, want, P)
    # M = 2: row 0 closes once per partition, everything else lies in the last row
    cfg = (500, 2, 4)
    want = _want(cols, P, cfg)
    assert int(SP.split(want, P, 2)["globals"][2]) == P
    with kta.HipMetricHandler(P, now=NOW, segments=cfg) as h:
        _device(h, cols)
        _hold(h, want, P)
        out = kta.retention_whatif(h.segments()["vector"], P, 2, 10**13, retention_bytes=0)
        assert np.array_equal(out, np.array(SP.retention_brute(want, P, 2, 10**13, -1, 0), np.uint64)) and out[:P, 9].all()


# ------------------------------------------------------------------------------------------ layouts
def _headers(h, b, ntiles):
    """[(lens, mode)] of the batch's first tiles."""
    raw = np.empty(2 * ntiles, np.uint64)
    h._check(N.load().kta_copy_to_host(h._ctx, raw.ctypes.data, b.tile_hdr, raw.nbytes))
    return [(int(x) >> 32, int(x) & 0xFFFFFFFF) for x in raw[1::2]]


def _view(b, lo):
    v = N.KtaBatch()
    for f, sz in SIZES:
        setattr(v, f, getattr(b, f) + lo * sz)
    return v


def test_every_tile_form_both_layouts_and_a_view():
    P, n = 6, 5 * 1024 + 5
    cols = _cols(30, n, P, jitter=500)
    cols["val_len"][1024 + 77] = 65535                                     # tile 1: i32 lengths beside u16 tiles
    cols["ts_ms"][2 * 1024 + 5] = BASE + 2**32                             # tile 2: raw partitions and timestamps
    cols["key_len"][3 * 1024 + 9] = 70000                                  # tile 3: both
    cols["ts_ms"][3 * 1024 + 10] = BASE + 2**33
    cfg = (4096, 300, 5)
    want = _want(cols, P, cfg)
    with kta.HipMetricHandler(P, now=NOW, segments=cfg) as h:
        b, nb = h.upload_batch(cols)                                       # keyless: u16 lengths where they fit
        before = _headers(h, b, 6)
        assert before == [(1, 1), (0, 1), (1, 0), (0, 0), (1, 1), (1, 1)]  # (lens, mode) of the six tiles
        for chunk in (0, 64):
            h.reset()
            h.set_segments_chunk(chunk)
            h.submit_device(b, nb, 0, which=1)
            _hold(h, want, P)
        assert _headers(h, b, 6) == before                                 # nothing was widened
        for lo, hi in ((4, n - 37), (1024 + 512, 4 * 1024 + 512)):         # views over several forms
            h.reset()
            h.submit_device(_view(b, lo), hi - lo, 0, which=1)
            _hold(h, _want(_cut(cols, lo, hi), P, cfg), P)
        h.sync()
        h.device_batch_free(b)
        h.reset()                                                          # a keyed allocation: i32 lengths in every tile
        keyed = dict(cols, key_off=np.zeros(n, np.uint32), key_bytes=np.zeros(16, np.uint8))
        b, nb = h.upload_batch(keyed, with_keys=True)
        assert all(lens == 0 for lens, _ in _headers(h, b, 6))
        h.submit_device(b, nb, 0, which=1)
        _hold(h, want, P)
        h.sync()
        h.device_batch_free(b)
        h.reset()                                                          # the raw layout: a host batch
        _submit(h, cols)
        _hold(h, want, P)


# ------------------------------------------------------------------------------------------ submission paths
def test_staging_ring_handle_message_replay_and_which_2():
    P, n = 6, 20000
    rng = np.random.default_rng(40)
    cols = random_cols(rng, n, P, key_space=500, null_key=0.15, empty_key=0.05, tomb=0.3, max_key=70, max_val=70000)
    cols["partition"][rng.random(n) < 0.02] = -1
    cols["partition"][rng.random(n) < 0.02] = P
    cfg = (1 << 20, 700, 12)
    with kta.HipMetricHandler(P, now=NOW, batch_capacity=1 << 12, segments=cfg) as h:
        _submit(h, cols)                                                   # five host batches
        _hold(h, _want(cols, P, cfg), P)
        h.reset()
        h.replay_messages(cols)
        _hold(h, _want(cols, P, cfg), P)
        h.reset()
        kb = cols["key_bytes"].tobytes()
        for i in range(3000):
            kl, vl = int(cols["key_len"][i]), int(cols["val_len"][i])
            key = None if kl < 0 else kb[int(cols["key_off"][i]):int(cols["key_off"][i]) + kl]
            h.handle_message(kta.Message(int(cols["partition"][i]), int(cols["ts_ms"][i]), key, None if vl < 0 else vl))
        want = _want(_cut({k: cols[k] for k in ("partition", "key_len", "val_len", "ts_ms")}, 0, 3000), P, cfg)
        _hold(h, want, P)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, segments=cfg) as h:
        b, nb = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, nb, 0, which=2)                                 # the alive-key handler alone: nothing
        got = h.segments()
        assert list(got["globals"]) == [0, 0, 0, 1 << 20, 700, 12, 0, 0] and not got["vector"][:-8].any()
        h.submit_device(b, nb, 0, which=3)
        _hold(h, _want(cols, P, cfg), P)
        h.sync()
        h.device_batch_free(b)


def test_kafka_decode():
    from kafka_cases import random_record_set
    lib = N.load()
    rng = np.random.default_rng(42)
    P = 4
    blobs, part, klen, vlen, tss = [], [], [], [], []
    for fetch in range(6):
        p = fetch % P
        blob, (pl, kl, vl, ts, keys), _ = random_record_set(rng, 50, partition=p, key_space=300, with_noise=False)
        blobs.append((blob, p))
        part += [p] * len(kl)
        klen += [int(x) for x in kl]
        vlen += [int(x) for x in vl]
        tss += [int(x) for x in ts]
    cols = {"partition": np.array(part, np.int32), "key_len": np.array(klen, np.int32), "val_len": np.array(vlen, np.int32),
            "ts_ms": np.array(tss, np.int64)}
    cfg = (2000, 500, 70)
    want = _want(cols, P, cfg)
    assert int(SP.split(want, P, 500)["globals"][2]) > 3
    with kta.HipMetricHandler(P, now=NOW, segments=cfg) as h:
        for blob, p in blobs:
            st = N.KtaKafkaIndexStats()
            h._check(lib.kta_kafka_consume(h._ctx, blob, len(blob), p, C.byref(st)))
        _hold(h, want, P)


def test_filtered_context_sees_the_passing_records():
    P, n = 6, 20000
    cols = _cols(50, n, P, jitter=0)
    frm, to, parts = BASE + 50_000, BASE + 150_000, [0, 2, 3, 5]
    keep = np.isin(cols["partition"].astype(np.int64), parts) & (cols["ts_ms"] >= frm) & (cols["ts_ms"] < to)
    assert 1000 < int(keep.sum()) < n // 2
    taken = {k: np.ascontiguousarray(v[keep]) for k, v in cols.items()}
    cfg = (10_000, 100, 0)
    with kta.HipMetricHandler(P, now=NOW, segments=cfg) as h:
        h.set_filter(frm, to, parts)
        h.set_filter_slice(8192)
        _device(h, cols)
        _hold(h, _want(taken, P, cfg), P)


def test_compaction_replay_touches_nothing():
    P = 5
    cols = random_cols(np.random.default_rng(51), 8000, P, key_space=900, null_key=0.1, tomb=0.3, max_key=40)
    cfg = (50_000, 100, 0)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True, segments=cfg) as h:
        b, nb = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, nb, 0)
        want = _want(cols, P, cfg)
        _hold(h, want, P)
        with h.compaction_replay():
            h.submit_device(b, nb, 0)
            assert h.compaction()["replayed"] == nb
        _hold(h, want, P)
        h.sync()
        h.device_batch_free(b)


# ------------------------------------------------------------------------------------------ P
def test_partition_count_at_the_bound_and_refusals():
    bound = kta.segments_max_partitions()
    assert bound >= 1024
    for P in (600, bound):                                                 # two and one wave per workgroup
        M = (1 << 20) // P
        cols = _cols(P, 1 << 15, P, none=0.1)
        cfg = (700, min(M, 64), 3)
        with kta.HipMetricHandler(P, now=NOW, segments=cfg) as h:
            h.set_segments_chunk(1024)
            _device(h, cols)
            _hold(h, _want(cols, P, cfg), P)
    with pytest.raises(kta.KtaError, match="at most %d partitions" % bound):
        kta.HipMetricHandler(bound + 1, now=NOW, segments=(1000, 2, 0))
    for cfg, msg in (((0, 4, 0), "segment_bytes"), (((1 << 40) + 1, 4, 0), "segment_bytes"), ((100, 1, 0), "rows_per_partition"),
                     ((100, (1 << 20) // 3 + 1, 0), "rows_per_partition")):
        with pytest.raises(kta.KtaError, match=msg):
            kta.HipMetricHandler(3, now=NOW, segments=cfg)
    with kta.HipMetricHandler(3, now=NOW) as h:
        for fn in (h._lib.kta_segments_info, ):
            out = (C.c_uint64 * 6)()
            assert fn(h._ctx, C.byref(out)) == N.KTA_ERR_INVALID
        with pytest.raises(kta.KtaError, match="kta_set_segments"):
            h.set_segments_chunk(64)
        with pytest.raises(kta.KtaError, match="no segments"):
            h.segments()


# ------------------------------------------------------------------------------------------ with every other pass
def test_every_opt_in_at_once_the_other_vectors_are_those_of_a_context_without_segments():
    P, n = 6, 30000
    cols = random_cols(np.random.default_rng(52), n, P, key_space=4000, null_key=0.1, empty_key=0.05, tomb=0.3, max_key=64)
    tl = (BASE - 10**9, 50_000_000, 40)
    cfg = (100_000, 50, 9)
    got = []
    for seg in (cfg, None):
        with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, batch_capacity=1 << 13, key_bytes_capacity=1 << 19, analytics=True,
                                  timeline=tl, key_sketch=True, hot_keys=True, ts_order=True, partitioner=True, size_quantiles=True,
                                  segments=seg) as h:
            h.submit_columns(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"], cols["key_off"], cols["key_bytes"])
            res, c = h.finish()
            got.append([bytes(res), c, h.exchange_partitioner()["vector"], h.exchange_key_sketch(), h.exchange_timeline(),
                        h.exchange_ts_order()["vector"], h.exchange_hot_keys(), h.exchange_size_quantiles()["vector"],
                        str({k: np.asarray(v).tolist() for k, v in sorted(h.exchange_analytics().items())}).encode()])
            if seg:
                _hold(h, _want(cols, P, cfg), P)
    for a, b in zip(*got):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    assert np.array_equal(got[0][2], R.vector(cols, P, P)) and np.array_equal(got[0][3], KS.sketch(cols, P))
    assert np.array_equal(got[0][4], TL.timeline_vector(cols, P, *tl))
    assert np.array_equal(got[0][5], TS.vector_of(P, cols["partition"], cols["ts_ms"]))
    assert np.array_equal(got[0][6].reshape(-1), np.asarray(HK.vector(cols, P)).reshape(-1))


# ------------------------------------------------------------------------------------------ the CLI
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")


@pytest.fixture(scope="module")
def mock_rccl(tmp_path_factory):
    lib = tmp_path_factory.mktemp("mock") / "libmock_rccl.so"
    r = subprocess.run(["timeout", "-k", "10", "600", "/opt/rocm/bin/hipcc", "-O1", "-shared", "-fPIC", "-std=c++17",
                        os.path.join(ROOT, "tests", "mock_rccl.cpp"), "-o", str(lib), "-lrt", "-lpthread"],
                       capture_output=True, text=True, timeout=660)
    assert r.returncode == 0, r.stderr[-2000:]
    return str(lib)


def _cli(*args, env=None):
    return subprocess.run(["timeout", "-k", "10", "240", CLI, *args], capture_output=True, text=True, timeout=270, env=env)


def _normalise(text):
    text = re.sub(r"Scanning took: \d+ seconds", "Scanning took: 3 seconds", text)
    return re.sub(r"Estimated Msg/s: \d+", "Estimated Msg/s: 133", text)


def _split_cli(stdout):
    at = stdout.index("Retention what-if: ")
    return stdout[:at], stdout[at:]


def test_cli_section_on_synthetic_sharded_per_message_and_nothing_without_the_knob(mock_rccl):
    src = "synthetic://c4?records=200000"
    sp, _ = kta.synth_preset("c4")
    cols = kta.synth_fill_host(sp, 0, 200000)
    P = int(sp.n_partitions)
    M = min(1024, (1 << 20) // P)
    S, overhead, now_s = 64 << 10, 70, int(cols["ts_ms"].max()) // 1000 + 5
    vec = _want(cols, P, (S, M, overhead))
    assert int(SP.split(vec, P, M)["globals"][2]) > P
    span = int(cols["ts_ms"].max() - cols["ts_ms"][cols["ts_ms"] >= 0].min()) // 1000
    rms_s = max(span // 2, 1)
    knobs = "kta.segments=64k,kta.segments.overhead=70,kta.retention.now=%d" % now_s
    plain = _cli("-t", "c4", "-b", src)
    assert plain.returncode == 0 and "Retention what-if" not in plain.stdout, plain.stderr
    only = _cli("-t", "c4", "-b", src, "--librdkafka", knobs)                  # no policy: the segment columns only
    assert only.returncode == 0, only.stderr
    report, section = _split_cli(only.stdout)
    assert section == SP.section(vec, P, M, now_s * 1000) and _normalise(report) == _normalise(plain.stdout)
    policy = knobs + ",kta.retention.ms=%ds,kta.retention.bytes=128k" % rms_s
    want = SP.section(vec, P, M, now_s * 1000, rms_s * 1000, 128 << 10)
    assert " time " in want or " size " in want                                # (the policy does cut something)
    one = _cli("-t", "c4", "-b", src, "--librdkafka", policy)
    assert one.returncode == 0, one.stderr
    report, section = _split_cli(one.stdout)
    assert section == want and _normalise(report) == _normalise(plain.stdout)
    env = dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl)
    many = _cli("-t", "c4", "-b", src, "--librdkafka", policy + ",kta.gpus=2,kta.batch=32768,kta.oversubscribe=1", env=env)
    assert many.returncode == 0, many.stderr[-2000:]
    assert many.stdout.count("Retention what-if: ") == 1 and _split_cli(many.stdout)[1] == want
    pm = _cli("-t", "c4", "-b", src, "--librdkafka", policy + ",kta.per_message=1,kta.batch=4096")
    assert pm.returncode == 0, pm.stderr
    assert _split_cli(pm.stdout)[1] == want

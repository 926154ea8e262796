"""CPU tests of the exchanged and printed analytics (KTA_FLAG_ANALYTICS, ABI 7): the host-side decode, merge and
render of an analytics vector against the independent restatement in tests/analytics_py.py, the torch twin of the
exchange over gloo, the new exports against the header, and the CLI's opt-in knob where no GPU is needed."""
import ctypes as C
import os
import re
import socket
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import analytics_py as AP
from helpers import random_cols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
I64_MIN = np.iinfo(np.int64).min
NEW_EXPORTS = ("kta_exchange_analytics", "kta_analytics_result_vector", "kta_decode_analytics", "kta_merge_analytics",
               "kta_render_analytics", "kta_analytics_max_partitions")


def _vec(P, hist_k=None, hist_v=None, parts=()):
    """A hand-made analytics vector: parts = [(p, min_ms, max_ms, smallest or None, largest or None)]."""
    v = np.zeros(AP.HIST + 4 * P, np.int64)
    if hist_k:
        for b, c in hist_k.items():
            v[b] = c
    if hist_v:
        for b, c in hist_v.items():
            v[34 + b] = c
    x = v[AP.HIST:].reshape(P, 4)
    x[:] = I64_MIN
    for p, lo, hi, sm, lg in parts:
        x[p, 0], x[p, 1] = ~lo, hi
        if sm is not None:
            x[p, 2], x[p, 3] = ~sm, lg
    return v.view(np.uint64)


# ------------------------------------------------------------------------------------------ 1. render
CASES = {
    # empty buckets between used ones, a partition without records (1), a tombstone-only partition (2)
    "gaps": (3, {0: 5, 1: 2, 4: 7, 9: 1}, {0: 3, 2: 4, 12: 8}, [(0, 1_600_000_000_000, 1_600_000_999_999, 3, 4100),
                                                             (2, 1_500_000_000_123, 1_500_000_000_999, None, None)]),
    # a partition whose timestamps are negative (truncation toward zero: -1500 ms -> -1 s) and one at epoch 0 (the
    # reference's -1 -> 0 rule has already happened on the device)
    "negative": (2, {2: 10}, {3: 6, 1: 4}, [(0, -86_400_000 * 400 - 1500, -1500, 0, 0), (1, 0, 0, 1, 7)]),
    # bucket 33 (2^31 .. 2^32-1) and the widest label
    "bucket33": (1, {33: 1, 1: 1}, {33: 2}, [(0, 1, 2, 2147483648, 4294967295)]),
    # nothing at all: None and 0 rows still printed, every partition dashes
    "empty": (2, {}, {}, []),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_render_analytics_matches_the_python_restatement(case):
    P, hk, hv, parts = CASES[case]
    v = _vec(P, hk, hv, parts)
    got = kta.render_analytics(v, P)
    want = AP.section(AP.decode(v, P))
    assert got == want
    assert got.startswith("Size histograms and per-partition extrema") and "not part of the reference report" in got
    assert got.endswith("=" * 120 + "\n")
    lines = got.splitlines()
    assert any(l.startswith("| None ") for l in lines) and any(l.startswith("| 0 ") for l in lines)
    if case == "gaps":
        assert "| 2-3 " not in got and "| 8-15 " not in got                      # empty buckets are not printed
        for label in ("1", "4-7", "128-255", "1024-2047"):
            assert any(l.startswith("| %s " % label) for l in lines), label
        assert re.search(r"^\| 1 +\| - +\| - +\| - +\| - +\|$", got, flags=re.M)          # no records
        assert re.search(r"^\| 2 +\| 2017-07-14 02:40:00 UTC \| 2017-07-14 02:40:00 UTC \| - +\| - +\|$", got,
                         flags=re.M)                                                     # tombstones only
    if case == "negative":
        assert "1969-12-31 23:59:59 UTC" in got and "1970-01-01 00:00:00 UTC" in got
    if case == "bucket33":
        assert any(l.startswith("| 2147483648-4294967295 ") for l in lines) and "4294967295 |" in got
        assert "| 100.00 " in got                 # 2 values over 2 records
    if case == "empty":
        assert "| 0.00 " in got and got.count("| - ") == 4 * P


def test_render_analytics_percentages_and_buffer_contract():
    v = _vec(1, {1: 1, 2: 2}, {5: 3}, [(0, 0, 0, 1, 9)])
    got = kta.render_analytics(v, 1)
    assert "| 0     | 1    | 33.33  |" in got and "| 1     | 2    | 66.67  |" in got and "| 100.00 |" in got
    lib = N.load()
    n = C.c_size_t()
    small = C.create_string_buffer(11)
    assert lib.kta_render_analytics(v.ctypes.data, 1, small, len(small), C.byref(n)) == N.KTA_OK
    assert n.value == len(got) and small.value.decode() == got[:10]
    assert lib.kta_render_analytics(None, 1, small, len(small), C.byref(n)) == N.KTA_ERR_INVALID
    assert lib.kta_render_analytics(v.ctypes.data, 0, small, len(small), C.byref(n)) == N.KTA_ERR_INVALID


# ------------------------------------------------------------------------------------------ 2. decode / merge
def test_decode_analytics_against_numpy_on_random_records():
    rng = np.random.default_rng(3)
    for P in (1, 5, 64):
        cols = random_cols(rng, 4000, P, big_sizes=True)
        cols["val_len"][cols["partition"] == 0] = -1            # a tombstone-only partition
        keep = cols["partition"] != P - 1 if P > 2 else np.ones(len(cols["partition"]), bool)
        cols = {k: (v[keep] if k != "key_bytes" else v) for k, v in cols.items()}
        v = AP.analytics_vector(cols, P)
        got = kta.decode_analytics(v, P)
        want = AP.decode(v, P)
        for k in want:
            assert np.array_equal(got[k], want[k]), (P, k)
        assert int(got["key_size_hist"].sum()) == len(cols["partition"]) == int(got["value_size_hist"].sum())
        assert got["part_smallest"][0] == np.iinfo(np.uint64).max and got["part_largest"][0] == 0
        if P > 2:
            assert got["part_max_ts_sec"][P - 1] == I64_MIN and got["part_min_ts_sec"][P - 1] == np.iinfo(np.int64).max


@pytest.mark.parametrize("shards", [2, 3, 5])
def test_merge_analytics_of_disjoint_shards_is_the_union(shards):
    rng = np.random.default_rng(40 + shards)
    P = 12
    cols = random_cols(rng, 30000, P, big_sizes=True)
    cols["ts_ms"][:50] = -rng.integers(1, 10**12, size=50)       # negative timestamps take part as well
    whole = AP.analytics_vector(cols, P)
    # by partition (what a sharded run does) and by record (any disjoint split): both merge to the union
    for owner in (cols["partition"] % shards, rng.integers(0, shards, size=len(cols["partition"]))):
        vecs = [AP.analytics_vector({k: v[owner == r] for k, v in cols.items() if k != "key_bytes"}, P)
                for r in range(shards)]
        acc = vecs[0].copy()
        for v in vecs[1:]:
            kta.merge_analytics(acc, v, P)
        assert np.array_equal(acc, whole)
        ref = vecs[0]
        for v in vecs[1:]:
            ref = AP.merge(ref, v, P)
        assert np.array_equal(ref, whole)
    # random vectors: the C merge is the numpy one, in place on uint64 and on int64 views alike
    for _ in range(20):
        a = rng.integers(I64_MIN, np.iinfo(np.int64).max, size=AP.HIST + 4 * P, dtype=np.int64, endpoint=True)
        b = rng.integers(I64_MIN, np.iinfo(np.int64).max, size=AP.HIST + 4 * P, dtype=np.int64, endpoint=True)
        want = AP.merge(a.view(np.uint64), b.view(np.uint64), P)
        got = a.copy()
        kta.merge_analytics(got, b, P)
        assert np.array_equal(got.view(np.uint64), want)
        got = a.view(np.uint64).copy()
        assert kta.merge_analytics(got, b.view(np.uint64), P) is got and np.array_equal(got, want)
    with pytest.raises(ValueError):
        kta.merge_analytics(np.zeros(AP.HIST + 4 * P, np.uint64), np.zeros(AP.HIST + 4 * P - 1, np.uint64), P)


# ------------------------------------------------------------------------------------------ 3. ABI
def test_new_exports_are_declared_bound_and_abi_is_7():
    header = open(os.path.join(ROOT, "include", "kta_hip.h")).read()
    assert int(re.search(r"#define KTA_ABI_VERSION (\d+)", header).group(1)) == 7
    lib = N.load()
    assert lib.kta_abi_version() == N.KTA_ABI_VERSION == 7
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_EXPORTS:
        assert re.search(r"^int\s+%s\s*\(" % name, text, flags=re.M), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name


def test_analytics_partition_limit_is_the_scan_lds_plan():
    """7 u64 per partition slot + the 2 x 34 x 16 u32 histograms (+ the scan's static reduction words) within the
    160 KiB of LDS a gfx950 workgroup has."""
    limit = kta.analytics_max_partitions()
    hist, static = 2 * 34 * 16 * 4, (256 // 64) * 6 * 8
    assert limit * 56 + hist + static <= 160 * 1024 < (limit + 1) * 56 + hist + static
    assert 2000 < limit < 4096


# ------------------------------------------------------------------------------------------ 4. torch twin (gloo)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, P, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rng = np.random.default_rng(77)
        cols = random_cols(rng, 20000, P, big_sizes=True)       # the same topic on every rank
        cols["val_len"][cols["partition"] == 1] = -1
        mine = cols["partition"] % world == rank
        vecs = [AP.analytics_vector({k: v[cols["partition"] % world == r] for k, v in cols.items() if k != "key_bytes"}, P)
                for r in range(world)]
        t = torch.from_numpy(vecs[rank].view(np.int64).copy())
        from kafka_topic_analyzer_amd import distributed as D
        D.allreduce_analytics_vector(t, P)
        acc = vecs[0].copy()
        for v in vecs[1:]:
            kta.merge_analytics(acc, v, P)
        ok = np.array_equal(t.numpy().view(np.uint64), acc) and \
            np.array_equal(acc, AP.analytics_vector({k: v for k, v in cols.items() if k != "key_bytes"}, P)) and \
            bool(mine.any())
        q.put((rank, ok))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_allreduce_analytics_vector_over_gloo_equals_the_merge(world):
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, 9, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(r for r, _ in res) == list(range(world))
    assert all(ok for _, ok in res), res


# ------------------------------------------------------------------------------------------ 5. CLI without a GPU
def test_cli_help_is_unchanged_by_the_analytics_knob():
    plain = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    knob = subprocess.run([CLI, "--librdkafka", "kta.analytics=1", "--help"], capture_output=True, text=True, timeout=60)
    assert plain.returncode == knob.returncode == 0 and knob.stdout == plain.stdout and "analytics" not in plain.stdout


def test_cli_refuses_analytics_beyond_the_lds_plan_before_any_kernel(tmp_path):
    """More partitions than the analytics scan admits: a clear message and exit 2 before a context exists (so on a
    machine without a GPU as well); the same topic without the knob goes on to the reference's own checks."""
    n = kta.analytics_max_partitions() + 1
    d = tmp_path / "s"
    d.mkdir()
    for p in range(n):
        (d / ("%d" % p)).write_bytes(b"")
    src = "segment://" + ",".join("s/%d" % p for p in range(n))
    r = subprocess.run([CLI, "-t", "wide", "-b", src, "--librdkafka", "kta.analytics=1"], capture_output=True,
                       text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 2 and r.stdout == ""
    assert "kta.analytics=1" in r.stderr and ("at most %d" % (n - 1)) in r.stderr and str(n) in r.stderr
    r = subprocess.run([CLI, "-t", "wide", "-b", src], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 254 and "no content" in r.stderr               # main.rs:98-101, unchanged

"""CPU tests of the timeline (kta_set_timeline; no reference counterpart): the host-only render against the independent
restatement in tests/timeline_py.py, the partition limit of the scan's LDS plan, the new exports, the CLI's refusals
(before any context, so without a GPU), and the torch twin of the exchange over gloo."""
import ctypes as C
import os
import re
import socket
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import timeline_py as T
from helpers import random_cols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
NEW_EXPORTS = ("kta_set_timeline", "kta_timeline_max_partitions", "kta_get_timeline", "kta_timeline_vector",
               "kta_exchange_timeline", "kta_timeline_result_vector", "kta_render_timeline")


def _vec(n, rows):
    v = np.zeros((n + 3, 3), np.uint64)
    for r, x in rows.items():
        v[r] = x
    return v


# ------------------------------------------------------------------------------------------ 1. render
CASES = {
    "empty": (1_600_000_000_000, 3_600_000, 168, {}),
    "no_timestamp_only": (0, 1000, 10, {0: (7, 2, 900)}),
    "before_and_after": (1_700_000_000_000, 60_000, 24, {1: (3, 0, 30), 26: (5, 1, 50)}),
    "gaps": (1_600_000_000_000, 900_000, 96, {0: (1, 0, 3), 5: (10, 2, 1 << 40), 9: (4, 4, 0), 20: (1, 0, 7)}),
    "one_bucket": (86_400_000, 86_400_000, 1, {2: (9, 1, 99), 3: (1, 0, 1)}),
    "max_buckets": (1_600_000_000_007, 7, 1024, {2: (1, 0, 1), 1025: (2, 1, 2), 1026: (3, 0, 3)}),
    "odd_width_ms": (1_234, 1_500, 3, {3: (1, 0, 0)}),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_render_timeline_matches_the_python_restatement(case):
    origin, W, n, rows = CASES[case]
    v = _vec(n, rows)
    got = kta.render_timeline(v, origin, W, n)
    assert got == T.section(v, origin, W, n)
    assert got.startswith("Timeline, ") and "not part of the reference report" in got
    assert got.endswith("=" * 120 + "\n")
    lines = got.splitlines()
    for label in ("| No timestamp ", "| Before ", "| After "):
        assert sum(l.startswith(label) for l in lines) == 1, label
    bucket_rows = [l for l in lines if re.match(r"^\| [0-9+-]", l)]
    used = [k for k in range(n) if v[2 + k, 0]]
    assert len(bucket_rows) == (used[-1] - used[0] + 1 if used else 0)
    if case == "gaps":
        assert len(bucket_rows) == 16 and sum("| 0       | 0.00 " in l for l in bucket_rows) == 13
    if case == "empty":
        assert got.count("| 0.00 ") == 3
    if case == "max_buckets":
        assert len(bucket_rows) == 1024 and "Timeline, 7ms buckets from 2020-09-13 12:26:40.007 UTC" in got


def test_render_timeline_percentages_and_buffer_contract():
    v = _vec(2, {0: (1, 0, 0), 2: (1, 0, 0), 3: (1, 0, 0)})
    got = kta.render_timeline(v, 0, 1000, 2)
    assert got.count("| 33.33 ") == 3 and "| 0.00 " in got
    v = _vec(1, {1: (2, 0, 0), 2: (1, 0, 0)})
    got = kta.render_timeline(v, 0, 1000, 1)
    assert "| 66.67 " in got and "| 33.33 " in got
    lib = N.load()
    n = C.c_size_t()
    small = C.create_string_buffer(11)
    vv = np.ascontiguousarray(v.reshape(-1))
    assert lib.kta_render_timeline(vv.ctypes.data, 0, 1000, 1, small, len(small), C.byref(n)) == N.KTA_OK
    assert n.value == len(got) and small.value.decode() == got[:10]
    for bad in ((-1, 1000, 1), (0, 0, 1), (0, 1000, 0), (0, 1000, 1025), (2**62, 2**62, 2)):
        assert lib.kta_render_timeline(vv.ctypes.data, *bad, small, len(small), C.byref(n)) == N.KTA_ERR_INVALID, bad
    assert lib.kta_render_timeline(None, 0, 1000, 1, small, len(small), C.byref(n)) == N.KTA_ERR_INVALID
    with pytest.raises(ValueError):
        kta.render_timeline(np.zeros(10, np.uint64), 0, 1000, 1)


def test_restatement_places_every_counted_record_once():
    rng = np.random.default_rng(9)
    cols = random_cols(rng, 20000, 6, tomb=0.3)
    cols["partition"][:100] = -1
    v = T.timeline_vector(cols, 6, 1_600_000_000_000 - 10**8, 10**6, 150)
    ok = (cols["partition"] >= 0) & (cols["partition"] < 6)
    assert int(v[:, 0].sum()) == int(ok.sum()) and int(v[:, 1].sum()) == int((cols["val_len"][ok] == -1).sum())
    assert int(v[:, 2].sum()) == int((np.maximum(cols["key_len"][ok], 0).astype(np.int64) +
                                      np.maximum(cols["val_len"][ok], 0)).sum())


# ------------------------------------------------------------------------------------------ 2. ABI, LDS plan
def test_new_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "kta_hip.h")).read()
    assert re.search(r"#define KTA_TIMELINE_MAX_BUCKETS 1024\b", header)
    assert re.search(r"#define KTA_TIMELINE_COLS 3\b", header)
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = N.load()
    for name in NEW_EXPORTS:
        assert re.search(r"^int\s+%s\s*\(" % name, text, flags=re.M), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name


def test_timeline_partition_limit_is_monotone_and_below_the_analytics_limit():
    a_max = kta.analytics_max_partitions()
    prev_plain = prev_an = None
    for n in (1, 2, 24, 168, 500, 1000, 1023, 1024):
        plain, an = kta.timeline_max_partitions(n), kta.timeline_max_partitions(n, analytics=True)
        assert an <= a_max and an <= plain <= 4096
        if prev_plain is not None:
            assert plain <= prev_plain and an <= prev_an, n
        prev_plain, prev_an = plain, an
    # 7 u64 per partition + the histograms + 16 B per timeline row + the static reduction words, in 160 KiB
    an = kta.timeline_max_partitions(1024, analytics=True)
    fixed = 2 * 34 * 16 * 4 + 1027 * 16 + (256 // 64) * 6 * 8
    assert an * 56 + fixed <= 160 * 1024 < (an + 1) * 56 + fixed
    assert kta.timeline_max_partitions(1024) == 4096
    assert kta.timeline_max_partitions(0) == 0 and kta.timeline_max_partitions(1025) == 0


# ------------------------------------------------------------------------------------------ 3. CLI without a GPU
def _cli(args, cwd=None):
    return subprocess.run([CLI, "-t", "c2", *args], capture_output=True, text=True, timeout=120, cwd=cwd)


@pytest.mark.parametrize("knobs,needle", [
    ("kta.timeline=0", "kta.timeline=0: expected a bucket width"),
    ("kta.timeline=abc", "kta.timeline=abc: expected a bucket width"),
    ("kta.timeline=5x", "kta.timeline=5x: expected a bucket width"),
    ("kta.timeline=-3", "kta.timeline=-3: expected a bucket width"),
    ("kta.timeline=1h,kta.timeline.buckets=0", "kta.timeline.buckets=0: expected a bucket count in [1, 1024]"),
    ("kta.timeline=1h,kta.timeline.buckets=1025", "kta.timeline.buckets=1025: expected a bucket count in [1, 1024]"),
    ("kta.timeline=1h,kta.timeline.start=-5", "kta.timeline.start=-5: expected unix seconds >= 0"),
    ("kta.timeline=106751990d,kta.timeline.buckets=1024,kta.timeline.start=0", "overflow"),
])
def test_cli_refuses_a_bad_timeline_before_any_context(knobs, needle):
    r = _cli(["-b", "synthetic://c2?records=1000", "--librdkafka", knobs])
    assert r.returncode == 2 and r.stdout == "", (r.returncode, r.stdout, r.stderr)
    assert needle in r.stderr and "kta_create" not in r.stderr and "HIP device" not in r.stderr


def test_cli_refuses_a_timeline_beyond_the_lds_plan_before_any_context(tmp_path):
    n = kta.timeline_max_partitions(1024, analytics=True) + 1
    assert n <= kta.analytics_max_partitions()              # the analytics alone would be admitted
    d = tmp_path / "s"
    d.mkdir()
    for p in range(n):
        (d / ("%d" % p)).write_bytes(b"")
    src = "segment://" + ",".join("s/%d" % p for p in range(n))
    r = _cli(["-b", src, "--librdkafka", "kta.analytics=1,kta.timeline=1h,kta.timeline.buckets=1024"], cwd=str(tmp_path))
    assert r.returncode == 2 and r.stdout == ""
    assert "kta.timeline=1h" in r.stderr and ("at most %d" % (n - 1)) in r.stderr and str(n) in r.stderr
    r = _cli(["-b", src, "--librdkafka", "kta.analytics=1,kta.timeline=1h,kta.timeline.buckets=168"], cwd=str(tmp_path))
    assert r.returncode == 254 and "no content" in r.stderr               # admitted: on to main.rs:98-101


def test_cli_help_is_unchanged_by_the_timeline_knob():
    plain = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    knob = subprocess.run([CLI, "--librdkafka", "kta.timeline=1h", "--help"], capture_output=True, text=True, timeout=60)
    assert plain.returncode == knob.returncode == 0 and knob.stdout == plain.stdout


# ------------------------------------------------------------------------------------------ 4. torch twin (gloo)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        P, tl = 9, (1_600_000_000_000 - 5 * 10**8, 10**7, 100)
        cols = random_cols(np.random.default_rng(78), 20000, P, big_sizes=True)      # the same topic on every rank
        vecs = [T.timeline_vector({k: v[cols["partition"] % world == r] for k, v in cols.items() if k != "key_bytes"},
                                  P, *tl) for r in range(world)]
        t = torch.from_numpy(vecs[rank].reshape(-1).view(np.int64).copy())
        from kafka_topic_analyzer_amd import distributed as D
        D.allreduce_timeline_vector(t)
        whole = T.timeline_vector(cols, P, *tl)
        ok = np.array_equal(t.numpy().view(np.uint64).reshape(-1, 3), whole) and \
            np.array_equal(sum(vecs), whole) and bool(vecs[rank][:, 0].any())
        q.put((rank, ok))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_allreduce_timeline_vector_over_gloo_equals_the_sum(world):
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(r for r, _ in res) == list(range(world))
    assert all(ok for _, ok in res), res

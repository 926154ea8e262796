"""CPU tests of the timestamp-order pass (KTA_FLAG_TS_ORDER; no reference counterpart): the header's constants and the
unchanged ABI number, the host-only merge and section against the restatement in tests/ts_order_py.py, the partition
bound, and the CLI's refusal of a bad kta.ts_order value (before any context, so without a GPU)."""
import os
import re
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import ts_order_py as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
NEW_EXPORTS = ("kta_get_ts_order", "kta_exchange_ts_order", "kta_ts_order_result_vector", "kta_merge_ts_order",
               "kta_ts_order_max_partitions", "kta_ts_order_info", "kta_set_ts_order_chunk", "kta_render_ts_order")
I63 = (1 << 63) - 1


def _counter_vec(records):
    P = len(records)
    c = np.zeros(P * N.KTA_NCOUNTERS + N.KTA_NGLOBALS, np.uint64)
    c[0:P * N.KTA_NCOUNTERS:N.KTA_NCOUNTERS] = np.array(records, np.uint64)
    return c


def _stream(seed, P, n, jitter=5000, none=0.02, bad=0.02):
    rng = np.random.default_rng(seed)
    part = rng.integers(0, P, n).astype(np.int32)
    ts = np.arange(n, dtype=np.int64) * 10 + 1_600_000_000_000 + rng.integers(-jitter, jitter + 1, n)
    ts[rng.random(n) < none] = -1
    part[rng.random(n) < bad] = rng.choice(np.array([-1, P], np.int32))
    return part, ts


# ------------------------------------------------------------------------------------------ 1. the restatement itself
def test_the_vectorised_restatement_equals_the_loop():
    for seed, P in ((1, 1), (2, 3), (3, 17)):
        part, ts = _stream(seed, P, 4000)
        a, b = T.TsOrder(P), T.TsOrder(P)
        for lo in range(0, 4000, 700):                       # batches with carry
            a.feed(part[lo:lo + 700], ts[lo:lo + 700])
        b.feed_loop(part, ts)
        assert np.array_equal(a.vector(), b.vector()) and a.hi == b.hi
        v = kta.split_ts_order(a.vector(), P)
        assert int(v["late"].sum()) == int(v["hist"].sum()) > 0 and v["timed"] < 4000
        assert (v["max_late_ms"] <= v["late_ms_sum"]).all()


def test_definition_corner_cases():
    t = T.TsOrder(2).feed_loop([0, 0, 0, 1, 0, 5, -1, 0], [10, 10, 9, 3, -5, 1, 1, I63])
    v = kta.split_ts_order(t.vector(), 2)
    assert v["timed"] == 5 and list(v["late"]) == [1, 0] and list(v["late_ms_sum"]) == [1, 0]      # equal is in order; d = 1
    assert v["hist"][0] == 1 and v["hist"][1:].sum() == 0 and list(v["max_late_ms"]) == [1, 0]
    t.feed_loop([0], [0])                                                                          # d = 2^63 - 1
    v = kta.split_ts_order(t.vector(), 2)
    assert v["hist"][62] == 1 and int(v["max_late_ms"][0]) == I63 and int(v["late_ms_sum"][0]) == I63 + 1


# ------------------------------------------------------------------------------------------ 2. merge and section
def test_merge_is_sum_prefix_and_max_suffix():
    P = 6
    rng = np.random.default_rng(9)
    a = rng.integers(0, 1 << 62, T.words(P), dtype=np.uint64)
    b = rng.integers(0, 1 << 62, T.words(P), dtype=np.uint64)
    a[1], b[1] = (1 << 64) - 5, 9                           # a late_ms_sum that wraps
    want = T.merge(a, b, P)
    assert int(want[1]) == 4
    got = a.copy()
    assert kta.merge_ts_order(got, b, P) is got and np.array_equal(got, want)
    s = 2 * P + 64
    assert np.array_equal(got[:s], a[:s] + b[:s]) and np.array_equal(got[s:], np.maximum(a[s:], b[s:]))
    # partitions sharded p % 2 through two contexts merge to the unsharded vector
    part, ts = _stream(4, P, 6000)
    halves = [T.vector_of(P, np.where(part % 2 == r, part, -1), ts) for r in (0, 1)]
    assert np.array_equal(kta.merge_ts_order(halves[0], halves[1], P), T.vector_of(P, part, ts))
    lib = N.load()
    assert lib.kta_merge_ts_order(None, b.ctypes.data, P) == N.KTA_ERR_INVALID
    assert lib.kta_merge_ts_order(a.ctypes.data, b.ctypes.data, 0) == N.KTA_ERR_INVALID


def _render_cases():
    out = {}
    out["empty"] = (np.zeros(T.words(3), np.uint64), [0, 0, 0])
    out["none late"] = (T.vector_of(2, [0, 0, 1, 0], [5, 6, 7, 6]), [3, 1])
    out["one late, d = 1"] = (T.vector_of(2, [0, 0, 1, 0], [5, 6, 7, 5]), [3, 1])
    out["d = 2^63 - 1"] = (T.vector_of(1, [0, 0, 0], [I63, 0, -1]), [3])
    part, ts = _stream(12, 256, 30000)
    out["256 partitions"] = (T.vector_of(256, part, ts), np.bincount(part[(part >= 0) & (part < 256)], minlength=256))
    part, ts = _stream(13, 5, 20000, jitter=3_600_000)
    out["wide jitter"] = (T.vector_of(5, part, ts), np.bincount(part[(part >= 0) & (part < 5)], minlength=5))
    return out


@pytest.mark.parametrize("name", ["empty", "none late", "one late, d = 1", "d = 2^63 - 1", "256 partitions", "wide jitter"])
def test_render_equals_the_restatement(name):
    vec, records = _render_cases()[name]
    P = len(records)
    text = kta.render_ts_order(vec, _counter_vec(records), P)
    assert text == T.section(vec, records)
    assert text.startswith(T.TITLE) and text.endswith("=" * 120 + "\n")
    if name in ("empty", "none late"):
        assert "No record is late.\n" in text and "Late by" not in text
    if name == "one late, d = 1":
        assert re.search(r"\| 0 +\| 3 +\| 1 +\| 33\.33 +\| 1 +\| 1 +\|", text) and re.search(r"\| < 2 ms +\| 1 +\| 100\.00 +\|", text)
        assert re.search(r"\| 1 +\| 1 +\| 0 +\| 0\.00 +\| - +\| - +\|", text)
    if name == "d = 2^63 - 1":
        assert "< 9223372036854775808 ms" in text and str(I63) in text and "Records without a timestamp: 1\n" in text


def test_render_refuses_bad_arguments_and_reports_the_length():
    import ctypes as C
    lib = N.load()
    vec, records = _render_cases()["one late, d = 1"]
    cv = _counter_vec(records)
    n = C.c_size_t()
    assert lib.kta_render_ts_order(vec.ctypes.data, cv.ctypes.data, 2, None, 0, C.byref(n)) == N.KTA_OK
    assert n.value == len(T.section(vec, records))
    buf = C.create_string_buffer(20)
    assert lib.kta_render_ts_order(vec.ctypes.data, cv.ctypes.data, 2, buf, 20, C.byref(n)) == N.KTA_OK
    assert buf.value.decode() == T.section(vec, records)[:19]
    assert lib.kta_render_ts_order(None, cv.ctypes.data, 2, None, 0, C.byref(n)) == N.KTA_ERR_INVALID
    assert lib.kta_render_ts_order(vec.ctypes.data, None, 2, None, 0, C.byref(n)) == N.KTA_ERR_INVALID
    assert lib.kta_render_ts_order(vec.ctypes.data, cv.ctypes.data, 0, None, 0, C.byref(n)) == N.KTA_ERR_INVALID
    with pytest.raises(ValueError):
        kta.render_ts_order(vec[:-1], cv, 2)


# ------------------------------------------------------------------------------------------ 3. ABI, bound, CLI
def test_new_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "kta_hip.h")).read()
    assert re.search(r"#define KTA_FLAG_TS_ORDER 32u\b", header) and re.search(r"#define KTA_TS_ORDER_HIST 63\b", header)
    assert re.search(r"#define KTA_ABI_VERSION 7\b", header)
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = N.load()
    for name in NEW_EXPORTS:
        assert re.search(r"^int\s+%s\s*\(" % name, text, flags=re.M), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    assert lib.kta_abi_version() == 7
    assert N.KTA_FLAG_TS_ORDER == 32 and N.KTA_TS_ORDER_HIST == T.HIST == 63
    flags = [int(v) for v in re.findall(r"#define KTA_FLAG_\w+ (\d+)u", header)]
    assert sorted(flags) == [1, 2, 4, 8, 16, 32]              # the next free bit, no bit twice


def test_the_pass_admits_at_least_1024_partitions():
    assert kta.ts_order_max_partitions() >= 1024


@pytest.mark.parametrize("value", ["2", "yes", "", "-1", "01"])
def test_cli_refuses_a_bad_ts_order_value_before_any_context(value):
    r = subprocess.run([CLI, "-t", "c2", "-b", "synthetic://c2?records=1000", "--librdkafka", "kta.ts_order=" + value],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and r.stdout == "" and "kta.ts_order=" in r.stderr and "expected 0 or 1" in r.stderr


def test_cli_help_is_unchanged_by_the_ts_order_knob():
    plain = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    knob = subprocess.run([CLI, "--librdkafka", "kta.ts_order=1", "--help"], capture_output=True, text=True, timeout=60)
    assert plain.returncode == knob.returncode == 0 and knob.stdout == plain.stdout

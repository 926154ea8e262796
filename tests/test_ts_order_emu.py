"""The wave step of the timestamp-order pass — the apply kernel's own source (csrc/kta_ts_order_wave.h) — run on the CPU:
tests/native/wave_emu.h makes the 64 lanes fibers that meet at ballots, shuffles and readlanes, and runs them between two
meetings in ascending, descending and shuffled order, so a step that relied on the order in which lanes reach LDS fails
under one of them.  A sequence of 200 instructions shares one `run` table; every lane's `prev` and the final table are
compared with the definition's sequential loop.  The GPU tests stay the parity gate (tests/test_gpu_ts_order.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
ORDERS = [(0, 0), (1, 0), (2, 7)]
INSTR = 200
I63 = (1 << 63) - 1


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu") / "libkta_ts_order_emu.so")
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.environ.get("KTA_EMU_ASAN") else []
    r = subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", *sanitize,
                        "-I", CSRC, "-I", NATIVE, os.path.join(NATIVE, "ts_order_emu.cpp"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.kta_emu_ts_order.restype = C.c_int
    lib.kta_emu_ts_order.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_uint32, C.c_char_p, C.c_uint64]
    return lib


def sequential(part, ts, P, seed):
    """the definition's loop: prev of every record (-1: not timestamped, or none before it) and the final table"""
    run = [int(x) for x in seed]
    prev = np.full(len(part), -1, np.int64)
    for i, (p, t) in enumerate(zip(part.tolist(), ts.tolist())):
        if 0 <= p < P and t >= 0:
            prev[i] = run[p]
            run[p] = max(run[p], t)
    return prev, np.array(run, np.int64)


def run_step(lib, part, ts, P, seed, order):
    part = np.ascontiguousarray(part, np.int32)
    ts = np.ascontiguousarray(ts, np.int64)
    n_instr = len(part) // 64
    run = np.ascontiguousarray(seed, np.int64).copy()
    prev = np.full(len(part), -7, np.int64)
    counters = np.zeros(2, np.uint32)
    err = C.create_string_buffer(320)
    rc = lib.kta_emu_ts_order(part.ctypes.data, ts.ctypes.data, n_instr, P, run.ctypes.data, prev.ctypes.data, counters.ctypes.data,
                              order[0], order[1], err, 320)
    assert rc == 0, err.value
    return prev, run, counters


def _cases():
    rng = np.random.default_rng(5)
    n = INSTR * 64
    ramp = np.arange(n, dtype=np.int64) * 3 + 10000
    out = {}
    out["one partition, descending"] = (4, np.full(n, 2, np.int32), ramp[::-1].copy())
    out["one partition, ascending"] = (4, np.full(n, 2, np.int32), ramp)
    out["one partition, equal"] = (4, np.full(n, 1, np.int32), np.full(n, 777, np.int64))
    out["64 distinct partitions"] = (64, np.tile(rng.permutation(64).astype(np.int32), INSTR), ramp + rng.integers(-500, 500, n))
    out["two partitions alternating"] = (2, (np.arange(n) & 1).astype(np.int32), ramp + rng.integers(-2000, 2000, n))
    for P in (3, 7, 256):
        out["random, P = %d" % P] = (P, rng.integers(0, P, n).astype(np.int32), ramp + rng.integers(-3000, 3000, n))
    P = 7
    part = rng.integers(0, P, n).astype(np.int32)
    ts = ramp + rng.integers(-3000, 3000, n)
    bad = rng.random(n) < 1 / 3
    kind = rng.integers(0, 3, n)
    ts = np.where(bad & (kind == 0), rng.choice(np.array([-1, -2, -(1 << 62)], np.int64), n), ts)
    part = np.where(bad & (kind == 1), -1, np.where(bad & (kind == 2), P, part)).astype(np.int32)
    out["a third of the lanes invalid"] = (P, part, ts)
    out["timestamps 0 and 2^63 - 1"] = (5, rng.integers(0, 5, n).astype(np.int32),
                                        rng.choice(np.array([0, I63, 1, I63 - 1], np.int64), n))
    # runs of 128 records of one partition with 1 % strays: both paths within one table (an instruction lies in one run
    # and holds no stray with probability 0.99^64 = 0.53: about 105 of the 200 take the one-partition path)
    part = np.repeat(rng.integers(0, 6, n // 128), 128).astype(np.int32)
    stray = rng.random(n) < 0.01
    part = np.where(stray, rng.integers(0, 6, n), part).astype(np.int32)
    out["runs with strays"] = (6, part, ramp + rng.integers(-100, 100, n))
    return out


CASES = _cases()


@pytest.mark.parametrize("order", ORDERS, ids=["ascending", "descending", "shuffled"])
@pytest.mark.parametrize("name", list(CASES))
def test_wave_step_equals_the_sequential_loop(emu, name, order):
    P, part, ts = CASES[name]
    rng = np.random.default_rng(len(name))
    seed = np.where(rng.random(P) < 0.5, -1, rng.integers(0, 5000, P)).astype(np.int64)
    want_prev, want_run = sequential(part, ts, P, seed)
    prev, run, counters = run_step(emu, part, ts, P, seed, order)
    assert np.array_equal(prev, want_prev)
    assert np.array_equal(run, want_run)
    if name.startswith("one partition"):
        assert counters[0] == INSTR and counters[1] == 0
    if name.startswith("64 distinct"):
        assert counters[0] == 0 and counters[1] == 0
    if name.startswith("two partitions"):
        assert counters[0] == 0 and counters[1] == 2 * INSTR
    if name.startswith("runs with strays"):
        assert counters[0] > INSTR // 4 and counters[1] > 0


def test_an_instruction_without_a_timestamped_lane_touches_nothing(emu):
    part = np.full(64 * 3, -1, np.int32)
    ts = np.full(64 * 3, 5, np.int64)
    seed = np.array([9, -1, 3], np.int64)
    prev, run, counters = run_step(emu, part, ts, 3, seed, ORDERS[2])
    assert (prev == -1).all() and np.array_equal(run, seed) and not counters.any()

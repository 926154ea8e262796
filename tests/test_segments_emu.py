"""The wave step of the segment pass — the apply kernel's own source (csrc/kta_segments_wave.h) — run on the CPU:
tests/native/wave_emu.h makes the 64 lanes fibers that meet at ballots, shuffles and readlanes, and runs them between two
meetings in ascending, descending and shuffled order.  A sequence of 200 instructions shares one `run` table; every lane's
state, every row a lane closes and the final tables are compared with the definition's sequential loop
(tests/segments_py.py).  The GPU tests stay the parity gate (tests/test_gpu_segments.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import segments_py as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
ORDERS = [(0, 0), (1, 0), (2, 7)]
INSTR = 200
NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu") / "libkta_segments_emu.so")
    r = subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas",
                        "-I", CSRC, "-I", NATIVE, os.path.join(NATIVE, "segments_emu.cpp"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.kta_emu_segments.restype = C.c_int
    lib.kta_emu_segments.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4 + \
        [C.c_int, C.c_uint32, C.c_char_p, C.c_uint64]
    return lib


def sequential(part, klen, vlen, ts, P, S, M, overhead, seed):
    """the definition's loop from the seeded running state: every record's trace, the rows and the final state"""
    v = SP.empty_vector(P, S, M, overhead)
    tot = P * M * SP.ROW
    v[tot:tot + P * SP.ROW] = [int(x) for x in seed.reshape(-1)]
    trace = []
    SP.apply_records(v, P, part.tolist(), klen.tolist(), vlen.tolist(), ts.tolist(), trace)
    at = np.full((len(part), 6), NONE, np.uint64)
    for i, t in enumerate(trace):
        if t is not None:
            at[i] = np.array(t, dtype=np.uint64)
    return at, np.array(v[tot:tot + P * SP.ROW], dtype=np.uint64).reshape(P, SP.ROW)


def run_step(lib, part, klen, vlen, ts, P, S, M, overhead, seed, order):
    part, klen, vlen = (np.ascontiguousarray(a, np.int32) for a in (part, klen, vlen))
    ts = np.ascontiguousarray(ts, np.int64)
    run = np.ascontiguousarray(seed, np.uint64).copy()
    nxt = np.zeros(P, np.uint64)
    at = np.zeros((len(part), 6), np.uint64)
    counters = np.zeros(2, np.uint32)
    err = C.create_string_buffer(320)
    rc = lib.kta_emu_segments(part.ctypes.data, klen.ctypes.data, vlen.ctypes.data, ts.ctypes.data, len(part) // 64, P, S, M, overhead,
                              run.ctypes.data, nxt.ctypes.data, at.ctypes.data, counters.ctypes.data, order[0], order[1], err, 320)
    assert rc == 0, err.value
    return at, run, nxt, counters


def _cases():
    rng = np.random.default_rng(11)
    n = INSTR * 64
    ramp = np.arange(n, dtype=np.int64) * 3 + 10000

    def lens():
        k = rng.integers(-1, 40, n).astype(np.int32)
        v = np.where(rng.random(n) < 0.1, -1, rng.integers(0, 300, n)).astype(np.int32)
        return k, v

    out = {}
    out["one partition"] = (4, np.full(n, 2, np.int32), *lens(), ramp + rng.integers(-500, 500, n))
    out["64 distinct partitions"] = (64, np.tile(rng.permutation(64).astype(np.int32), INSTR), *lens(), ramp)
    out["two partitions alternating"] = (2, (np.arange(n) & 1).astype(np.int32), *lens(), ramp + rng.integers(-2000, 2000, n))
    for P in (1, 3, 64):
        out["random, P = %d" % P] = (P, rng.integers(0, P, n).astype(np.int32), *lens(), ramp + rng.integers(-3000, 3000, n))
    P = 7
    part = rng.integers(0, P, n).astype(np.int32)
    bad = rng.random(n) < 1 / 3
    part = np.where(bad, rng.choice(np.array([-1, P, P + 9, -(1 << 31)], np.int64), n), part).astype(np.int32)
    ts = np.where(rng.random(n) < 0.3, rng.choice(np.array([-1, -2, -(1 << 62)], np.int64), n), ramp)
    out["a third of the lanes not taking part"] = (P, part, *lens(), ts)
    part = np.repeat(rng.integers(0, 6, n // 128), 128).astype(np.int32)
    part = np.where(rng.random(n) < 0.01, rng.integers(0, 6, n), part).astype(np.int32)
    out["runs with strays"] = (6, part, *lens(), ramp)
    out["lengths of 2^31 - 1"] = (3, rng.integers(0, 3, n).astype(np.int32), np.full(n, 2**31 - 1, np.int32),
                                  np.where(rng.random(n) < 0.5, 2**31 - 1, -1).astype(np.int32), ramp)
    return out


CASES = _cases()


# every case at S = 7 in all three lane orders; S = 1 (every record closes a row) and S = 2^40 (none does) in the shuffled
# order, without the two cases whose many groups per instruction make the emulator slow
ORDER_IDS = ["ascending", "descending", "shuffled"]
SLOW = ("random, P = 64", "a third of the lanes not taking part")
PARAMS = [pytest.param(name, 7, o, id="%s-7-%s" % (name, i)) for name in CASES for o, i in zip(ORDERS, ORDER_IDS)] + \
         [pytest.param(name, S, ORDERS[2], id="%s-%d-shuffled" % (name, S)) for name in CASES if name not in SLOW for S in (1, 1 << 40)]


@pytest.mark.parametrize("name,S,order", PARAMS)
def test_wave_step_equals_the_sequential_loop(emu, name, S, order):
    P, part, klen, vlen, ts = CASES[name]
    M, overhead = 9, 3
    rng = np.random.default_rng(len(name) + S % 1000)
    seed = np.zeros((P, SP.ROW), np.uint64)
    seed[:, 0] = rng.integers(0, 5000, P)
    seed[:, 1] = rng.integers(0, 3 * S if S < 1 << 30 else 1 << 41, P)
    seed[:, 2] = rng.integers(0, 50, P)
    seed[:, 3] = np.where(rng.random(P) < 0.5, 0, rng.integers(1, 5000, P))
    want_at, want_run = sequential(part, klen, vlen, ts, P, S, M, overhead, seed)
    at, run, nxt, counters = run_step(emu, part, klen, vlen, ts, P, S, M, overhead, seed, order)
    assert np.array_equal(at, want_at)
    assert np.array_equal(run, want_run)
    for p in range(P):   # the boundary beside run[p] is the one of where the partition stands
        b = int(run[p, 1])
        assert int(nxt[p]) == ((b // S + 1) * S if b // S < M - 1 else (1 << 64) - 1)
    if name == "one partition":
        assert counters[0] == INSTR and counters[1] == 0
    if name.startswith("64 distinct"):
        assert counters[0] == 0 and counters[1] == 0
    if name.startswith("two partitions"):
        assert counters[0] == 0 and counters[1] == 2 * INSTR
    if S == 1 and name.startswith("random"):
        assert want_at[:, 4].astype(np.int64).clip(0, 1).sum() > 0   # rows were closed in this case


def test_an_instruction_without_a_record_that_takes_part_touches_nothing(emu):
    part = np.full(64 * 3, -1, np.int32)
    z = np.full(64 * 3, 5, np.int32)
    seed = np.arange(12, dtype=np.uint64).reshape(3, 4)
    at, run, nxt, counters = run_step(emu, part, z, z, z.astype(np.int64), 3, 100, 4, 0, seed, ORDERS[2])
    assert (at == NONE).all() and np.array_equal(run, seed) and not counters.any()

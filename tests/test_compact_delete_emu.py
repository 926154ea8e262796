"""The KEPT instantiation of the segment pass's wave step — the kept-apply kernel's own source, seg_wave_step<true> of
csrc/kta_segments_wave.h — run on the CPU: tests/native/wave_emu.h makes the 64 lanes fibers that meet at ballots,
shuffles and readlanes, and runs them between two meetings in ascending, descending and shuffled order.  A sequence of 200
instructions shares one `run` table {L, B, T, K}; every lane's state, every row a lane closes and the final tables are
compared with the definition's sequential loop (tests/compact_delete_py.py).  The class of every record is random over
{0, 1, 2}.  The GPU tests stay the parity gate (tests/test_gpu_compact_delete.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import compact_delete_py as CD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
ORDERS = [(0, 0), (1, 0), (2, 7)]
INSTR = 200
NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu") / "libkta_compact_delete_emu.so")
    r = subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas",
                        "-I", CSRC, "-I", NATIVE, os.path.join(NATIVE, "compact_delete_emu.cpp"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.kta_emu_kept.restype = C.c_int
    lib.kta_emu_kept.argtypes = [C.c_void_p] * 4 + [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4 + \
        [C.c_int, C.c_uint32, C.c_char_p, C.c_uint64]
    return lib


def sequential(part, klen, vlen, cls, P, S, M, overhead, seed):
    """the definition's loop from the seeded running state: every record's trace, and the final state"""
    v = CD.empty_vector(P, S, M, overhead)
    tot = P * M * CD.ROW
    v[tot:tot + P * CD.ROW] = [int(x) for x in seed.reshape(-1)]
    trace = []
    CD.apply_records(v, P, M, part.tolist(), klen.tolist(), vlen.tolist(), cls.tolist(), trace)
    at = np.full((len(part), 6), NONE, np.uint64)
    for i, t in enumerate(trace):
        if t is not None:
            at[i] = np.array(t, dtype=np.uint64)
    return at, np.array(v[tot:tot + P * CD.ROW], dtype=np.uint64).reshape(P, CD.ROW)


def run_step(lib, part, klen, vlen, cls, P, S, M, overhead, seed, order):
    part, klen, vlen = (np.ascontiguousarray(a, np.int32) for a in (part, klen, vlen))
    cls = np.ascontiguousarray(cls, np.uint8)
    run = np.ascontiguousarray(seed, np.uint64).copy()
    nxt = np.zeros(P, np.uint64)
    at = np.zeros((len(part), 6), np.uint64)
    counters = np.zeros(2, np.uint32)
    err = C.create_string_buffer(320)
    rc = lib.kta_emu_kept(part.ctypes.data, klen.ctypes.data, vlen.ctypes.data, cls.ctypes.data, len(part) // 64, P, S, M, overhead,
                          run.ctypes.data, nxt.ctypes.data, at.ctypes.data, counters.ctypes.data, order[0], order[1], err, 320)
    assert rc == 0, err.value
    return at, run, nxt, counters


def _cases():
    rng = np.random.default_rng(23)
    n = INSTR * 64

    def rest():
        k = rng.integers(-1, 40, n).astype(np.int32)
        v = np.where(rng.random(n) < 0.1, -1, rng.integers(0, 300, n)).astype(np.int32)
        return k, v, rng.integers(0, 3, n).astype(np.uint8)

    out = {}
    out["one partition"] = (4, np.full(n, 2, np.int32), *rest())
    out["64 distinct partitions"] = (64, np.tile(rng.permutation(64).astype(np.int32), INSTR), *rest())
    out["two partitions alternating"] = (2, (np.arange(n) & 1).astype(np.int32), *rest())
    for P in (1, 3, 64):
        out["random, P = %d" % P] = (P, rng.integers(0, P, n).astype(np.int32), *rest())
    P = 7
    part = rng.integers(0, P, n).astype(np.int32)
    bad = rng.random(n) < 1 / 3
    part = np.where(bad, rng.choice(np.array([-1, P, P + 9, -(1 << 31)], np.int64), n), part).astype(np.int32)
    out["a third of the lanes not taking part"] = (P, part, *rest())
    return out


CASES = _cases()

# every case at S = 7 in all three lane orders; S = 1 (every record closes a row) and S = 2^40 (none does) in the shuffled
# order, without the two cases whose many groups per instruction make the emulator slow
ORDER_IDS = ["ascending", "descending", "shuffled"]
SLOW = ("random, P = 64", "a third of the lanes not taking part")
PARAMS = [pytest.param(name, 7, o, id="%s-7-%s" % (name, i)) for name in CASES for o, i in zip(ORDERS, ORDER_IDS)] + \
         [pytest.param(name, S, ORDERS[2], id="%s-%d-shuffled" % (name, S)) for name in CASES if name not in SLOW for S in (1, 1 << 40)]


@pytest.mark.parametrize("name,S,order", PARAMS)
def test_kept_wave_step_equals_the_sequential_loop(emu, name, S, order):
    P, part, klen, vlen, cls = CASES[name]
    M, overhead = 9, 3
    rng = np.random.default_rng(len(name) + S % 1000)
    seed = np.zeros((P, CD.ROW), np.uint64)
    seed[:, 0] = rng.integers(0, 5000, P)
    seed[:, 1] = rng.integers(0, 3 * S if S < 1 << 30 else 1 << 41, P)
    seed[:, 2] = rng.integers(0, 50, P)
    seed[:, 3] = rng.integers(0, 1 << 40, P)
    want_at, want_run = sequential(part, klen, vlen, cls, P, S, M, overhead, seed)
    at, run, nxt, counters = run_step(emu, part, klen, vlen, cls, P, S, M, overhead, seed, order)
    assert np.array_equal(at, want_at)
    assert np.array_equal(run, want_run)
    for p in range(P):   # the boundary beside run[p] is the one of where the partition stands
        b = int(run[p, 1])
        assert int(nxt[p]) == ((b // S + 1) * S if b // S < M - 1 else (1 << 64) - 1)
    # the fourth word is a sum and the first a count of flags: both differ from the segment step's maximum and constant 1
    taking = (part >= 0) & (part < P)
    assert int(run[:, 0].sum() - seed[:, 0].sum()) == int(((cls == 1) & taking).sum()) < int(taking.sum())
    assert int(run[:, 2].sum() - seed[:, 2].sum()) == int(((cls == 2) & taking).sum())
    z = overhead + np.maximum(klen, 0).astype(np.int64) + np.maximum(vlen, 0)
    assert int(run[:, 3].sum() - seed[:, 3].sum()) == int(z[taking & (cls != 0)].sum())
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
    at, run, nxt, counters = run_step(emu, part, z, z, np.ones(64 * 3, np.uint8), 3, 100, 4, 0, seed, ORDERS[2])
    assert (at == NONE).all() and np.array_equal(run, seed) and not counters.any()

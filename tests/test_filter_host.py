"""The record filter's rules on the CPU (csrc/kta_filter.h through the library's host entry points kta_filter_host and
kta_filter_tile_host, and as the stand-alone sanitizer build tests/native/filter_check.cpp) against the restatement in
tests/filter_py.py.  No GPU: tests/test_gpu_filter.py holds the kernels and the contract."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import filter_py as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc")
TILE = 1024
I64_MIN, I64_MAX = -2**63, 2**63 - 1
W0, W1 = 1_600_000_000_000, 1_600_000_500_000


class Hdr(C.Structure):                       # kta_tile_hdr
    _fields_ = [("ts_base", C.c_int64), ("mode", C.c_uint32), ("lens", C.c_uint32)]


def _columns(seed, n=20000, P=37):
    rng = np.random.default_rng(seed)
    p = rng.integers(0, P, n).astype(np.int32)
    p[rng.random(n) < 0.03] = -1
    p[rng.random(n) < 0.03] = P
    p[rng.random(n) < 0.02] = P + 40
    p[rng.random(n) < 0.01] = -(2**31)
    t = (W0 + rng.integers(-300_000, 800_000, n)).astype(np.int64)
    t[rng.random(n) < 0.05] = -1
    for edge in (W0 - 1, W0, W0 + 1, W1 - 1, W1, W1 + 1, I64_MIN, I64_MIN + 1, I64_MAX - 1, I64_MAX, 0, -2):
        t[rng.integers(0, n, 40)] = edge
    return p, t, P


WINDOWS = [(None, None), (W0, W1), (W0, None), (None, W1), (I64_MIN + 1, I64_MAX - 1), (I64_MAX - 1, None), (None, I64_MIN + 1),
           (-2, 1), (W1 - 1, W1)]
SETS = [None, [0], [3, 31, 32, 36], list(range(37)), []]


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("parts", SETS)
def test_kta_filter_host_is_the_restated_predicate(window, parts):
    p, t, P = _columns(3)
    if window == (None, None) and parts is None:
        pass                                                # no filter: every record, bad partitions included
    want = np.nonzero(F.passes(p, t, P, window[0], window[1], parts))[0]
    got = kta.filter_host(p, t, P, window[0], window[1], parts)
    assert np.array_equal(got, want.astype(np.uint64))
    # the vectorised restatement against the record-by-record one, Python integers
    sample = np.random.default_rng(5).integers(0, len(p), 300)
    mask = F.passes(p, t, P, window[0], window[1], parts)
    for i in sample:
        assert bool(mask[i]) == F.record_passes(int(p[i]), int(t[i]), P, window[0], window[1], parts)


def test_edges_said_as_literals():
    P = 4
    p = np.array([1, 1, 1, 1, 1, 7, -1, 2, 2], np.int32)
    t = np.array([999, 1000, 4999, 5000, -1, 2000, 2000, 2000, -1], np.int64)
    assert kta.filter_host(p, t, P, 1000, 5000).tolist() == [1, 2, 5, 6, 7]          # [from, to); -1 fails; bad partitions pass
    assert kta.filter_host(p, t, P, None, None, [2]).tolist() == [7, 8]              # a set alone: -1 passes
    assert kta.filter_host(p, t, P, 1000, 5000, [1, 2]).tolist() == [1, 2, 7]        # with a set a bad partition fails
    assert kta.filter_host(p, t, P).tolist() == list(range(9))
    assert kta.filter_host(p, t, P, None, 1000).tolist() == [0]
    assert kta.filter_host(p, t, P, 5000, None).tolist() == [3]
    lib = N.load()
    m = C.c_uint64(0)
    assert lib.kta_filter_host(p.ctypes.data, t.ctypes.data, 9, P, 5, 5, None, 0, None, C.byref(m)) == N.KTA_ERR_INVALID
    assert lib.kta_filter_host(p.ctypes.data, t.ctypes.data, 9, P, 1000, 5000, None, 0, None, C.byref(m)) == N.KTA_OK and m.value == 5


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    """tile_pack_host behind a C interface (tests/native/tile_summary.cpp)."""
    so = str(tmp_path_factory.mktemp("filter") / "libkta_tile_summary.so")
    r = subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        "-I", CSRC, os.path.join(ROOT, "tests", "native", "tile_summary.cpp"), "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.kta_tile_summary_pack.restype = None
    lib.kta_tile_summary_pack.argtypes = [C.c_void_p] * 4 + [C.c_uint64, C.c_int] + [C.c_void_p] * 4 + [C.POINTER(Hdr), C.POINTER(N.KtaTileSum)]
    return lib


def _pack(packer, p, t):
    p, t = np.ascontiguousarray(p, np.int32), np.ascontiguousarray(t, np.int64)
    k = np.full(len(p), 5, np.int32)
    img = [np.zeros(TILE * 4, np.uint8), np.zeros(TILE * 8, np.uint8), np.zeros(TILE * 4, np.uint8), np.zeros(TILE * 4, np.uint8)]
    hdr, s = Hdr(), N.KtaTileSum()
    packer.kta_tile_summary_pack(p.ctypes.data, t.ctypes.data, k.ctypes.data, k.ctypes.data, len(p), 1, *[g.ctypes.data for g in img],
                                 C.byref(hdr), C.byref(s))
    assert (hdr.mode, hdr.ts_base, s.ts_span, s.part_max, s.flags) == F.tile_header_and_summary(p, t)
    return hdr, s


def _tile(rng, lo, hi, P, m=TILE):
    t = rng.integers(lo, hi + 1, m).astype(np.int64)
    t[0], t[-1] = lo, hi
    return rng.integers(0, P, m).astype(np.int32), t


def _tiles(P):
    rng = np.random.default_rng(11)
    out = {"just inside": _tile(rng, W0, W1 - 1, P), "one ms early": _tile(rng, W0 - 1, W1 - 1, P), "one ms late": _tile(rng, W0, W1, P),
           "just before": _tile(rng, W0 - 9000, W0 - 1, P), "touches from": _tile(rng, W0 - 9000, W0, P),
           "just after": _tile(rng, W1, W1 + 9000, P), "touches to": _tile(rng, W1 - 1, W1 + 9000, P),
           "straddles both": _tile(rng, W0 - 5, W1 + 5, P), "partial last tile": _tile(rng, W0, W1 - 1, P, 517)}
    p, t = _tile(rng, W0, W1 - 1, P)
    t[100] = -1
    out["untimed inside"] = (p, t)
    p, t = _tile(rng, W1, W1 + 10, P)
    t[100] = -1
    out["untimed outside"] = (p, t)
    out["no timestamp at all"] = (p.copy(), np.full(TILE, -1, np.int64))
    p, t = _tile(rng, W0, W1 - 1, P)
    p[17] = -1
    out["part_max == 0xFFFF"] = (p, t)
    p, t = _tile(rng, W0, W1 - 1, P)
    p[17] = P
    out["part_max == P"] = (p, t)
    p, t = _tile(rng, W0, W1 - 1, P)
    p[17] = 70000
    out["raw: a partition beyond u16"] = (p, t)
    p, t = _tile(rng, W0, W1 - 1, P)
    t[5] = W0 + 2**31 + 5
    out["raw: a span beyond i32"] = (p, t)
    return out


EXPECTED = {  # for the window [W0, W1) without a set
    "just inside": F.ALL, "one ms early": F.READ, "one ms late": F.READ, "just before": F.NONE, "touches from": F.READ, "just after": F.NONE,
    "touches to": F.READ, "straddles both": F.READ, "partial last tile": F.READ, "untimed inside": F.READ, "untimed outside": F.NONE,
    "no timestamp at all": F.NONE, "part_max == 0xFFFF": F.READ, "part_max == P": F.READ, "raw: a partition beyond u16": F.READ,
    "raw: a span beyond i32": F.READ}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_tile_decision_against_brute_force_over_the_tiles_records(packer, name):
    P = 9
    lib = N.load()
    p, t = _tiles(P)[name]
    hdr, s = _pack(packer, p, t)
    whole = len(p) == TILE
    for window in WINDOWS[1:] + [(W0 + 100, W1 - 100), (W0 - 100, W1 + 100)]:
        for parts in (None, [0, 5]):
            frm, to = window
            got = lib.kta_filter_tile_host(P, I64_MIN if frm is None else frm, I64_MAX if to is None else to, int(parts is not None),
                                           C.byref(hdr), C.byref(s), int(whole))
            assert got == F.tile_decision(P, frm, to, parts is not None, hdr.mode, hdr.ts_base, s.ts_span, s.part_max, s.flags, whole)
            passing = int(F.passes(p, t, P, frm, to, parts).sum())
            if got == F.NONE:
                assert passing == 0
            if got == F.ALL:
                assert passing == TILE == len(p) and parts is None
            if window == (W0, W1) and parts is None:
                assert got == EXPECTED[name]
            if parts is not None:
                assert got != F.ALL
            # cut by the slice: always read
            assert lib.kta_filter_tile_host(P, I64_MIN if frm is None else frm, I64_MAX if to is None else to, int(parts is not None),
                                            C.byref(hdr), C.byref(s), 0) == F.READ
    # a set alone decides nothing
    assert lib.kta_filter_tile_host(P, I64_MIN, I64_MAX, 1, C.byref(hdr), C.byref(s), int(whole)) == F.READ


def test_predict_tiles_counts_every_tile_once():
    P = 5
    rng = np.random.default_rng(2)
    n = 3 * TILE + 517
    cols = {"partition": rng.integers(0, P, n).astype(np.int32), "ts_ms": (W0 + np.arange(n) * 100).astype(np.int64)}
    none, all_, read, slices = F.predict_tiles(cols, P, W0 + 100 * TILE, W0 + 100 * (2 * TILE + 512))
    assert (none, all_, read, slices) == (1, 1, 2, 1)
    assert F.predict_tiles(cols, P, W0 + 100 * TILE, W0 + 100 * (2 * TILE + 512), slice_records=2048) == (1, 1, 2, 2)
    assert F.predict_tiles(cols, P, None, None, [1]) == (0, 0, 4, 1)


def test_native_check_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/filter_check.cpp: a program of its own that calls kta_filter.h, built with the sanitizers and run directly."""
    exe = str(tmp_path / "filter_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "native", "filter_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK "), (r.stdout[-500:], r.stderr[-3000:])


def test_partition_bitmap():
    assert kta.partition_bitmap([0, 3, 32], 40).tolist() == [0b1001, 1]
    assert kta.partition_bitmap([], 5).tolist() == [0]
    with pytest.raises(ValueError):
        kta.partition_bitmap([-1], 5)


def test_render_filter_is_the_restated_section():
    cases = [(5, 1234, 99, 1_600_000_010_000, 1_600_000_020_000, [0, 3, 4]), (40, 0, 0, None, 1500, []), (8, 10, 10, None, None, [7]),
             (8, 3, 1, 0, None, None), (70, 1000, 7, 1000, 2000, [0, 1, 2, 31, 32, 33, 64, 69]), (3, 2**40, 2**39, 86_400_000, None, [0, 1, 2])]
    for P, seen, passed, frm, to, parts in cases:
        assert kta.render_filter(P, seen, passed, frm, to, parts) == F.section(P, seen, passed, frm, to, parts)
    assert "| Partitions          | 0-2,31-33,64,69 " in kta.render_filter(*cases[4][:3], *cases[4][3:])
    lib = N.load()
    n = C.c_size_t()
    assert lib.kta_render_filter(5, 5, None, 4, 0, 0, None, 0, C.byref(n)) == N.KTA_ERR_INVALID
    assert lib.kta_render_filter(1, 5, None, 0, 0, 0, None, 0, C.byref(n)) == N.KTA_ERR_INVALID


CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")


@pytest.mark.parametrize("knobs, says", [
    ("kta.from=abc", "kta.from=abc: expected unix seconds >= 0"), ("kta.to=-5", "kta.to=-5: expected unix seconds >= 0"),
    ("kta.from=", "kta.from=: expected unix seconds"), ("kta.from=20,kta.to=20", "expected kta.from below kta.to"),
    ("kta.from=21,kta.to=20", "expected kta.from below kta.to"), ("kta.partitions=8", "kta.partitions=8: expected partitions and ranges of the topic's 8"),
    ("kta.partitions=0,3-9", "kta.partitions=0,3-9: expected"), ("kta.partitions=3-1", "kta.partitions=3-1: expected"),
    ("kta.partitions=", "kta.partitions=: expected"), ("kta.partitions=1-", "kta.partitions=1-: expected"),
    ("kta.partitions=-1", "kta.partitions=-1: expected"), ("kta.partitions=0,1-2-3", "kta.partitions=0,1-2-3: expected")])
def test_cli_refuses_malformed_filter_keys_before_any_device_work(knobs, says):
    """usage errors in the style of the other kta.* keys: a line on stderr, exit status 2, nothing on stdout (c2 has 8 partitions)"""
    r = subprocess.run([CLI, "-t", "x", "-b", "synthetic://c2?records=100", "--librdkafka", knobs], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and says in r.stderr and r.stdout == "", (r.returncode, r.stderr)


def test_cli_a_piece_without_equals_still_panics_unless_it_continues_kta_partitions():
    r = subprocess.run([CLI, "-t", "x", "-b", "synthetic://c2?records=100", "--librdkafka", "kta.partitions=0,zz"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 101 and "src/main.rs:89" in r.stderr
    r = subprocess.run([CLI, "-t", "x", "-b", "synthetic://c2?records=100", "--librdkafka", "kta.from=5,7"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 101 and "src/main.rs:89" in r.stderr

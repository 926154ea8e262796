"""csrc/kta_tile.h on the CPU: the per-tile summary (kta_tile_sum, include/kta_hip.h) that tile_pack_host writes
beside the header (tests/native/tile_summary.cpp, plain g++), against a numpy restatement of its definition — over random
tiles and the definition's own edges.  The 16-byte header and the four images must be what the entry without a summary
gives.  No GPU: tests/test_gpu_tile_summary.py holds the device producer and the scan that reads summaries against this."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 1024                                   # KTA_TILE_RECORDS
RAW, COMPACT = 0, 1
VALID, TIMED, UNTIMED = 1, 2, 4               # KTA_TILE_SUM_*
PART_NONE = 0xFFFF                            # KTA_COMPACT_PART_NONE
I64_MIN, I64_MAX = -2**63, 2**63 - 1
POISON = 0x5A


class Hdr(C.Structure):                       # kta_tile_hdr
    _fields_ = [("ts_base", C.c_int64), ("mode", C.c_uint32), ("lens", C.c_uint32)]


class Sum(C.Structure):                       # kta_tile_sum
    _fields_ = [("ts_span", C.c_uint32), ("part_max", C.c_uint16), ("flags", C.c_uint16)]


assert C.sizeof(Hdr) == 16 and C.sizeof(Sum) == 8


@pytest.fixture(scope="module")
def codec(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tilesum") / "libkta_tile_summary.so")
    r = subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "tile_summary.cpp"), "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    common = [C.c_void_p] * 4 + [C.c_uint64, C.c_int] + [C.c_void_p] * 4 + [C.POINTER(Hdr)]
    lib.kta_tile_summary_pack.restype = None
    lib.kta_tile_summary_pack.argtypes = common + [C.POINTER(Sum)]
    lib.kta_tile_summary_pack_plain.restype = None
    lib.kta_tile_summary_pack_plain.argtypes = common
    return lib


def images():
    return [np.full(TILE * 4, POISON, np.uint8), np.full(TILE * 8, POISON, np.uint8),
            np.full(TILE * 4, POISON, np.uint8), np.full(TILE * 4, POISON, np.uint8)]


def restated(p, t):
    """kta_tile_sum as include/kta_hip.h words it -> (mode, ts_base, (ts_span, part_max, flags)); Python integers."""
    stamps = [int(x) for x in t if x != -1]
    lo, hi = (min(stamps), max(stamps)) if stamps else (0, 0)
    compact = all(-1 <= int(x) < 65535 for x in p) and hi - lo < 2**31
    if not compact:
        return RAW, 0, (0, 0, 0)
    if len(p) != TILE:
        return COMPACT, lo, (0, 0, 0)                           # the call did not write the whole tile: no summary
    part_max = max(PART_NONE if int(x) == -1 else int(x) for x in p)
    flags = VALID | (TIMED if stamps else 0) | (UNTIMED if len(stamps) < len(t) else 0)
    return COMPACT, lo, (hi - lo, part_max, flags)


def pack(codec, p, t, k, v, lens16=True):
    """Both entries on the same tile: header and images equal, and the summary is the restatement's.  -> (Hdr, (span, max, flags))"""
    cols = [np.ascontiguousarray(p, np.int32), np.ascontiguousarray(t, np.int64), np.ascontiguousarray(k, np.int32),
            np.ascontiguousarray(v, np.int32)]
    m = len(p)
    got, hdr, s = images(), Hdr(), Sum(0xDEADBEEF, 0xBEEF, 0xDEAD)   # (poisoned: the pack writes every field, zero included)
    codec.kta_tile_summary_pack(*[c.ctypes.data for c in cols], m, int(lens16), *[g.ctypes.data for g in got], C.byref(hdr), C.byref(s))
    plain, phdr = images(), Hdr()
    codec.kta_tile_summary_pack_plain(*[c.ctypes.data for c in cols], m, int(lens16), *[g.ctypes.data for g in plain], C.byref(phdr))
    assert bytes(hdr) == bytes(phdr), "the 16-byte header must be what the entry without a summary returns"
    for g, w in zip(got, plain):
        assert np.array_equal(g, w)
    mode, base, want = restated(cols[0], cols[1])
    assert (hdr.mode, hdr.ts_base) == (mode, base)
    assert (s.ts_span, s.part_max, s.flags) == want
    if s.flags & TIMED:   # the latest timestamp is ts_base + ts_span in modular u64 arithmetic
        latest = (hdr.ts_base + s.ts_span + 2**63) % 2**64 - 2**63
        assert latest == max(int(x) for x in cols[1] if x != -1)
    return hdr, (s.ts_span, s.part_max, s.flags)


def fitting(m, seed=0):
    rng = np.random.default_rng(seed + m)
    p = rng.integers(0, 100, m).astype(np.int32)
    t = (1_700_000_000_000 + rng.integers(0, 3_600_000, m)).astype(np.int64)
    k = rng.integers(-1, 40, m).astype(np.int32)
    v = rng.integers(-1, 2000, m).astype(np.int32)
    return p, t, k, v


@pytest.mark.parametrize("seed", range(8))
def test_random_tiles(codec, seed):
    rng = np.random.default_rng(100 + seed)
    p, t, k, v = fitting(TILE, seed)
    p[:] = rng.integers(-1 if seed % 2 else 0, [3, 100, 65535, 40000][seed % 4], TILE)
    t[rng.random(TILE) < [0.0, 0.01, 0.5, 0.999][seed % 4]] = -1
    t[t != -1] += int(rng.integers(-2**40, 2**40))
    _, (_, _, flags) = pack(codec, p, t, k, v, lens16=bool(seed & 1))
    assert flags & VALID


def test_a_whole_tile_has_a_summary_and_1023_records_have_none(codec):
    p, t, k, v = fitting(TILE)
    hdr, s = pack(codec, p, t, k, v)
    assert hdr.mode == COMPACT and s == (int(t.max() - t.min()), int(p.max()), VALID | TIMED)
    hdr, s = pack(codec, p[:1023], t[:1023], k[:1023], v[:1023])
    assert hdr.mode == COMPACT and s == (0, 0, 0)


def test_every_timestamp_missing(codec):
    p, t, k, v = fitting(TILE)
    t[:] = -1
    hdr, s = pack(codec, p, t, k, v)
    assert (hdr.mode, hdr.ts_base) == (COMPACT, 0) and s == (0, int(p.max()), VALID | UNTIMED)


def test_missing_and_timed_records_mixed(codec):
    p, t, k, v = fitting(TILE)
    t[::3] = -1
    t[1], t[1000] = 1_700_000_000_000 - 7, 1_700_000_000_000 + 2**30
    hdr, s = pack(codec, p, t, k, v)
    assert hdr.ts_base == 1_700_000_000_000 - 7 and s == (2**30 + 7, int(p.max()), VALID | TIMED | UNTIMED)


@pytest.mark.parametrize("base", [I64_MIN + 1, I64_MAX - (2**31 - 1)])
def test_the_full_span_at_the_ends_of_int64(codec, base):
    p, t, k, v = fitting(TILE)
    t[:] = base + 5
    t[17], t[900] = base, base + 2**31 - 1
    hdr, s = pack(codec, p, t, k, v)
    assert hdr.ts_base == base and s == (2**31 - 1, int(p.max()), VALID | TIMED)


def test_negative_timestamps_other_than_minus_1(codec):
    p, t, k, v = fitting(TILE)
    t[:] = -2
    t[5], t[6], t[7] = -77_000, -3, -1
    hdr, s = pack(codec, p, t, k, v)
    assert hdr.ts_base == -77_000 and s == (77_000 - 2, int(p.max()), VALID | TIMED | UNTIMED)


def test_a_record_of_partition_minus_1_is_the_largest_stored_partition(codec):
    p, t, k, v = fitting(TILE)
    p[333] = -1
    hdr, s = pack(codec, p, t, k, v)
    assert hdr.mode == COMPACT and s[1] == PART_NONE and s[2] & VALID


@pytest.mark.parametrize("why", ["partition 65535", "span 2^31"])
def test_a_raw_tile_has_a_zero_summary(codec, why):
    p, t, k, v = fitting(TILE)
    if why == "partition 65535":
        p[12] = 65535
    else:
        t[:] = 1_700_000_000_000
        t[1023] += 2**31
    hdr, s = pack(codec, p, t, k, v)
    assert hdr.mode == RAW and s == (0, 0, 0)
    p, t, k, v = fitting(TILE)                  # (65534 is the largest id the compact form holds)
    p[12] = 65534
    hdr, s = pack(codec, p, t, k, v)
    assert hdr.mode == COMPACT and s[1] == 65534

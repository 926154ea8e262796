"""csrc/kta_tile.h on the CPU: its whole-tile host pack and unpack (tests/native/tile_codec.cpp, plain g++) against a numpy
restatement of the format as include/kta_hip.h words it — header fields, the exact bytes of the four column images, the
round trip — for single tiles of 1, 4, 1023 and 1024 records and the format's own edges.  No GPU: the device readers of
the same header are held against the host by tests/test_tile_compact.py and tests/test_tile_lens.py.

    KTA_EMU_ASAN=1 ASAN_OPTIONS=detect_leaks=0 LD_PRELOAD="$(g++ -print-file-name=libasan.so) $(g++ -print-file-name=libubsan.so)" \
        python -m pytest tests/test_tile_codec_host.py
builds the shim with AddressSanitizer + UBSan (the inputs are heap blocks of exactly m records, the images of one tile)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 1024                                   # KTA_TILE_RECORDS
RAW, COMPACT, LENS_I32, LENS_U16 = 0, 1, 0, 1
I32_MIN, I32_MAX, I64_MIN, I64_MAX = -2**31, 2**31 - 1, -2**63, 2**63 - 1
SIZES = [1, 4, 1023, 1024]
EDGES = [-2, -1, 0, 65534, 65535, 65536, I32_MIN, I32_MAX]
POISON = 0x5A                                 # what the images hold before the pack: what it does not write stays


class Hdr(C.Structure):                       # kta_tile_hdr
    _fields_ = [("ts_base", C.c_int64), ("mode", C.c_uint32), ("lens", C.c_uint32)]


@pytest.fixture(scope="module")
def codec(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tile") / "libkta_tile_codec.so")
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if os.environ.get("KTA_EMU_ASAN") else []
    r = subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", *sanitize,
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "tile_codec.cpp"), "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.kta_tile_codec_pack.restype = None
    lib.kta_tile_codec_pack.argtypes = [C.c_void_p] * 4 + [C.c_uint64, C.c_int] + [C.c_void_p] * 4 + [C.POINTER(Hdr)]
    lib.kta_tile_codec_unpack.restype = None
    lib.kta_tile_codec_unpack.argtypes = [C.POINTER(Hdr)] + [C.c_void_p] * 4 + [C.c_uint64, C.c_uint64] + [C.c_void_p] * 4
    return lib


def images():
    return [np.full(TILE * 4, POISON, np.uint8), np.full(TILE * 8, POISON, np.uint8),
            np.full(TILE * 4, POISON, np.uint8), np.full(TILE * 4, POISON, np.uint8)]   # partition, ts_ms, key_len, val_len


def reference(p, t, k, v, lens16):
    """include/kta_hip.h, restated: (mode, lens, ts_base) and the bytes of the four images."""
    m = len(p)
    part, ts, klen, vlen = images()
    stamps = t[t != -1]
    lo, hi = (int(stamps.min()), int(stamps.max())) if len(stamps) else (0, 0)        # (Python integers: no overflow)
    compact = bool(np.all((p >= -1) & (p < 65535))) and hi - lo < 2**31
    base = lo if compact else 0
    if compact:     # u16 / i32 offsets in the first half of the tile's bytes; 0xFFFF / INT32_MIN: -1
        part.view(np.uint16)[:m] = np.where(p == -1, 0xFFFF, p).astype(np.uint16)
        ts.view(np.int32)[:m] = np.where(t == -1, I32_MIN, (t.astype(np.uint64) - np.uint64(base % 2**64)).astype(np.int64))
    else:
        part.view(np.int32)[:m] = p
        ts.view(np.int64)[:m] = t
    u16 = lens16 and bool(np.all((k >= -1) & (k < 65535) & (v >= -1) & (v < 65535)))
    if u16:         # 256 groups of 16 B in the key_len bytes: four key lengths, then their four value lengths; val_len unused
        g, j = klen.view(np.uint16), np.arange(m)
        g[(j // 4) * 8 + j % 4] = np.where(k == -1, 0xFFFF, k).astype(np.uint16)
        g[(j // 4) * 8 + 4 + j % 4] = np.where(v == -1, 0xFFFF, v).astype(np.uint16)
    else:
        klen.view(np.int32)[:m] = k
        vlen.view(np.int32)[:m] = v
    return (COMPACT if compact else RAW, LENS_U16 if u16 else LENS_I32, base), [part, ts, klen, vlen]


def fitting(m, seed=0):
    """A tile every value of which fits the compact forms (a few None keys, tombstones and timestamps among them)."""
    rng = np.random.default_rng(seed + m)
    p = rng.integers(0, 100, m).astype(np.int32)
    t = (1_700_000_000_000 + rng.integers(0, 3_600_000, m)).astype(np.int64)
    k = rng.integers(-1, 40, m).astype(np.int32)
    v = rng.integers(-1, 2000, m).astype(np.int32)
    return p, t, k, v


def check(codec, p, t, k, v, lens16, want_mode, want_lens, want_base=None):
    """Pack, hold header and images against the restatement and against what the case expects, unpack all and a part."""
    m = len(p)
    cols = [np.ascontiguousarray(p, np.int32), np.ascontiguousarray(t, np.int64), np.ascontiguousarray(k, np.int32),
            np.ascontiguousarray(v, np.int32)]
    (mode, lens, base), want = reference(*cols, lens16)
    assert (mode, lens) == (want_mode, want_lens), "the restatement itself disagrees with the case"
    if want_base is not None:
        assert base == want_base
    got, hdr = images(), Hdr()
    codec.kta_tile_codec_pack(*[c.ctypes.data for c in cols], m, int(lens16), *[g.ctypes.data for g in got], C.byref(hdr))
    assert (hdr.mode, hdr.lens, hdr.ts_base) == (mode, lens, base)
    for name, g, w in zip(("partition", "ts_ms", "key_len", "val_len"), got, want):
        assert np.array_equal(g, w), name
    for j0, j1 in {(0, m), (m // 3, m - m // 4)}:
        out = [np.full(j1 - j0, -7, np.int32), np.full(j1 - j0, -7, np.int64), np.full(j1 - j0, -7, np.int32), np.full(j1 - j0, -7, np.int32)]
        codec.kta_tile_codec_unpack(C.byref(hdr), *[g.ctypes.data for g in got], j0, j1, *[o.ctypes.data for o in out])
        for name, o, c in zip(("partition", "ts_ms", "key_len", "val_len"), out, cols):
            assert np.array_equal(o, c[j0:j1]), (name, j0, j1)
    return hdr


@pytest.mark.parametrize("m", SIZES)
def test_a_fitting_tile_is_compact_in_both_halves_and_round_trips(codec, m):
    p, t, k, v = fitting(m)
    hdr = check(codec, p, t, k, v, True, COMPACT, LENS_U16)
    assert hdr.ts_base == int(t.min())


@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("x", EDGES)
def test_one_partition_id_flips_mode_and_nothing_else(codec, m, x):
    p, t, k, v = fitting(m)
    p[m // 2] = x
    check(codec, p, t, k, v, True, COMPACT if -1 <= x < 65535 else RAW, LENS_U16)


@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("column", ["key_len", "val_len"])
@pytest.mark.parametrize("x", EDGES)
def test_one_length_flips_lens_and_nothing_else(codec, m, column, x):
    p, t, k, v = fitting(m)
    (k if column == "key_len" else v)[m - 1] = x
    check(codec, p, t, k, v, True, COMPACT, LENS_U16 if -1 <= x < 65535 else LENS_I32)


@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("x", EDGES)
def test_a_keyed_allocation_never_takes_u16_lengths(codec, m, x):
    p, t, k, v = fitting(m)
    check(codec, p, t, k, v, False, COMPACT, LENS_I32)           # lengths that would fit
    k[0] = v[m - 1] = x
    check(codec, p, t, k, v, False, COMPACT, LENS_I32)


@pytest.mark.parametrize("m", SIZES)
def test_without_length_images_the_lengths_are_left_alone(codec, m):
    p, t, k, v = fitting(m)
    got, hdr = images(), Hdr()
    codec.kta_tile_codec_pack(p.ctypes.data, t.ctypes.data, None, None, m, 1, got[0].ctypes.data, got[1].ctypes.data, None, None, C.byref(hdr))
    (mode, _, base), want = reference(p, t, k, v, True)
    assert (hdr.mode, hdr.lens, hdr.ts_base) == (mode, LENS_I32, base)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.all(got[2] == POISON) and np.all(got[3] == POISON)
    out_p, out_t = np.zeros(m, np.int32), np.zeros(m, np.int64)
    codec.kta_tile_codec_unpack(C.byref(hdr), got[0].ctypes.data, got[1].ctypes.data, None, None, 0, m, out_p.ctypes.data, out_t.ctypes.data, None, None)
    assert np.array_equal(out_p, p) and np.array_equal(out_t, t)


# a timestamp span needs two records
@pytest.mark.parametrize("m", [s for s in SIZES if s >= 2])
@pytest.mark.parametrize("lo", [0, 1_700_000_000_000, -5, I64_MIN + 1, I64_MAX - (2**31 - 1) - 1])
def test_a_span_of_2_31_minus_1_is_compact_and_2_31_is_raw(codec, m, lo):
    p, t, k, v = fitting(m)
    t[:] = lo if lo != -1 else 0
    t[m - 1] = lo + 2**31 - 1
    hdr = check(codec, p, t, k, v, True, COMPACT, LENS_U16, want_base=lo)
    assert hdr.ts_base == lo
    t[m - 1] = lo + 2**31
    check(codec, p, t, k, v, True, RAW, LENS_U16, want_base=0)


@pytest.mark.parametrize("m", [s for s in SIZES if s >= 2])
def test_the_widest_pair_of_timestamps_is_raw_and_exact(codec, m):
    p, t, k, v = fitting(m)
    t[0], t[m - 1] = I64_MIN + 1, I64_MAX
    check(codec, p, t, k, v, True, RAW, LENS_U16, want_base=0)
    t[0], t[m - 1] = I64_MAX, I64_MIN
    check(codec, p, t, k, v, True, RAW, LENS_U16, want_base=0)


@pytest.mark.parametrize("m", SIZES)
def test_a_tile_of_no_timestamps_is_compact_with_base_0(codec, m):
    p, t, k, v = fitting(m)
    t[:] = -1
    hdr = check(codec, p, t, k, v, True, COMPACT, LENS_U16, want_base=0)
    assert hdr.ts_base == 0


@pytest.mark.parametrize("m", [s for s in SIZES if s >= 2])
@pytest.mark.parametrize("base", [2**62, I64_MAX - 5, 1, 0, I64_MIN, -2])
def test_no_timestamp_next_to_a_large_base(codec, m, base):
    p, t, k, v = fitting(m)
    t[:] = base
    t[m - 1] = base + 5
    t[0] = -1
    if m == 2:
        t[1] = base
    check(codec, p, t, k, v, True, COMPACT, LENS_U16, want_base=base)

"""The generator and the model of tests/device_batch_model.py, without a GPU: over the seed list the GPU test
(tests/test_gpu_device_batch_sequences.py) runs, the sequences must reach every writer, every pair of writers on a common
tile, the cuts through tiles that should carry a summary (the stale-summary case, at the tile's front and at its back),
reader views that start or end inside such a tile, every value class and an extreme timestamp that lives only in a tile a
later writer partly overwrites — so that the GPU test cannot quietly test nothing.  These are conditions, not
measurements: where the seed list misses one, the list or the generator's weights change, not the numbers here.
And summary_definition(), the GPU test's yardstick for a tile's summary, against the host packer (csrc/kta_tile.h through
tests/native/tile_summary.cpp) on whole tiles of every value class."""
import ctypes as C
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import device_batch_model as M
from device_batch_model import CAPACITY, T, TILES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def coverage():
    """One pass over every seed's sequence with the model and the tracker beside it."""
    cov = {"writers": Counter(), "pairs": Counter(), "cuts": Counter(), "views": 0, "classes": Counter(), "extreme_cut": 0,
           "range_kinds": Counter(), "sequences": {}}
    for seed in M.SEEDS:
        P = M.P_of(seed)
        ops = M.gen_sequence(seed, CAPACITY, P)
        cov["sequences"][seed] = ops
        model, tracker = M.Model(), M.Tracker()
        for op in ops:
            name = type(op).__name__
            cov["writers"][name] += 1
            if name == "Upload":
                cov["classes"].update(op.classes)
            extreme = M.extreme_tiles(model, P)
            model.apply(op)
            cuts = tracker.note(op, model)
            for t, side in cuts:
                cov["cuts"][side] += 1
            cov["cuts"]["any"] += bool(cuts)
            cov["extreme_cut"] += len({t for t, _ in cuts} & extreme)
            lo, m = op.view
            inside = [x // T for x in (lo, lo + m) if x % T and x // T < TILES]
            cov["views"] += any(tracker.summed[t] for t in inside)
            end = op.lo + op.m
            cov["range_kinds"]["whole" if (op.lo, op.m) == (0, CAPACITY) else
                               "tiles" if op.lo % T == 0 and end % T == 0 else
                               "last_partial" if end == CAPACITY else
                               "inside_one" if op.lo // T == (end - 1) // T else
                               "starts_inside" if op.lo % T else "ends_inside"] += 1
        for names in tracker.touched:
            for i, a in enumerate(names):
                for b in names[i + 1:]:
                    cov["pairs"][(a, b)] += 1
    return cov


def test_sequences_are_deterministic_and_well_formed(coverage):
    for seed, ops in coverage["sequences"].items():
        assert ops == M.gen_sequence(seed, CAPACITY, M.P_of(seed))
        assert len(ops) == M.N_OPS and (ops[0].lo, ops[0].m) == (0, CAPACITY) and not isinstance(ops[0], M.Widen)
        assert sum(op.extra for op in ops) == 1
        assert eval(M.format_ops(ops), {k: getattr(M, k) for k in M.WRITERS}) == ops       # the printed form pastes back
        for op in ops:
            assert op.m >= 1 and op.lo >= 0 and op.lo + op.m <= CAPACITY and op.lo % 4 == 0    # 16-byte aligned columns
            assert not isinstance(op, M.Upload) or op.lo % T == 0                              # kta_batch_from_raw's rule
            assert not isinstance(op, M.Decode) or op.m in M.RECORD_SET_SIZES
            lo, m = op.view
            assert m >= 1 and lo >= 0 and lo + m <= CAPACITY and lo % 4 == 0
            assert not isinstance(op, M.Widen) or (seed // 2) % 2 == 1
            a, e = M.clobbered(op)
            assert op.lo + op.m == a <= e <= CAPACITY and (e == a or e % T == 0 or e == CAPACITY)


def test_every_writer_occurs(coverage):
    for w in M.WRITERS:
        assert coverage["writers"][w] >= 10, (w, coverage["writers"])


def test_every_ordered_pair_of_writers_meets_on_a_tile(coverage):
    for a in M.WRITERS:
        for b in M.WRITERS:
            assert coverage["pairs"][(a, b)] >= 1, (a, b)


def test_every_range_class_occurs(coverage):
    for kind in M.RANGE_KINDS:
        assert coverage["range_kinds"][kind] >= 5, (kind, coverage["range_kinds"])


def test_summarised_tiles_are_cut_at_the_front_and_at_the_back(coverage):
    assert coverage["cuts"]["any"] >= 10 and coverage["cuts"]["front"] >= 5 and coverage["cuts"]["back"] >= 5, coverage["cuts"]


def test_reader_views_start_or_end_inside_a_summarised_tile(coverage):
    assert coverage["views"] >= 10, coverage["views"]


def test_every_value_class_occurs(coverage):
    for cls in M.VALUE_CLASSES:
        assert coverage["classes"][cls] >= 5, (cls, coverage["classes"])


def test_an_extreme_timestamp_lives_only_in_a_tile_that_is_later_cut(coverage):
    assert coverage["extreme_cut"] >= 3, coverage["extreme_cut"]


def test_the_model_takes_a_writer_where_it_writes():
    m = M.Model()
    m.apply(M.Upload(0, CAPACITY, 5, 1, ("fit",) * 7))
    before = {k: m.cols[k].copy() for k in M.NAMES}
    op = M.Decode(1500, 701, 3)
    m.apply(op)
    want = M.decode_cols(op)
    for k in M.NAMES:
        assert np.array_equal(m.cols[k][1500:2201], want[k]) and np.array_equal(m.cols[k][:1500], before[k][:1500])
        assert np.array_equal(m.cols[k][2201:], before[k][2201:])
    assert (want["partition"] == 3).all() and (want["key_len"] == -1).any() and (want["val_len"] == -1).any()
    m.apply(M.Widen(0, CAPACITY))
    assert all(np.array_equal(m.cols[k][1500:2201], want[k]) for k in M.NAMES)
    assert M.clobbered(M.Upload(1024, 1500, 5, 1, ("fit",) * 2)) == (2524, 3072)
    assert M.clobbered(M.SynthFill(1024, 1500, "c2", 0, 5)) == (2524, 3072) and M.clobbered(M.SynthFill(1028, 1500, "c2", 0, 5)) == (2528, 2528)
    assert M.clobbered(M.Upload(6144, 37, 5, 1, ("fit",))) == (CAPACITY, CAPACITY) and M.clobbered(M.Decode(1024, 40, 0)) == (1064, 1064)
    assert M.clobbered(M.Upload(6144, 30, 5, 1, ("fit",))) == (6174, CAPACITY)


# ---- summary_definition against the host packer ---------------------------------------------------------------------------
class Hdr(C.Structure):                       # kta_tile_hdr
    _fields_ = [("ts_base", C.c_int64), ("mode", C.c_uint32), ("lens", C.c_uint32)]


class Sum(C.Structure):                       # kta_tile_sum
    _fields_ = [("ts_span", C.c_uint32), ("part_max", C.c_uint16), ("flags", C.c_uint16)]


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("model") / "libkta_tile_summary.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "tile_summary.cpp"), "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.kta_tile_summary_pack.restype = None
    lib.kta_tile_summary_pack.argtypes = [C.c_void_p] * 4 + [C.c_uint64, C.c_int] + [C.c_void_p] * 4 + [C.POINTER(Hdr), C.POINTER(Sum)]
    return lib


@pytest.mark.parametrize("P", [5, 300])
@pytest.mark.parametrize("cls", M.VALUE_CLASSES)
def test_summary_definition_is_the_host_packers(packer, cls, P):
    for seed in range(4):
        op = M.Upload(T, T, P, seed, (cls,))
        model = M.Model()
        model.apply(op)
        c = {k: np.ascontiguousarray(v) for k, v in M.upload_cols(op).items()}
        img = [np.zeros(T * 8, np.uint8) for _ in range(4)]
        hdr, s = Hdr(), Sum(0xDEADBEEF, 0xBEEF, 0xDEAD)
        packer.kta_tile_summary_pack(c["partition"].ctypes.data, c["ts_ms"].ctypes.data, c["key_len"].ctypes.data, c["val_len"].ctypes.data,
                                     T, 1, *[x.ctypes.data for x in img], C.byref(hdr), C.byref(s))
        want = M.summary_definition(model, 1)
        tile = model.tile(1)
        assert (hdr.mode == M.COMPACT) == M.compactable(tile["partition"], tile["ts_ms"]) == (want is not None)
        assert (hdr.lens == M.LENS_U16) == M.lens_fit(tile["key_len"], tile["val_len"])
        if want is None:
            assert cls in ("raw_part", "raw_span") and (s.ts_span, s.part_max, s.flags) == (0, 0, 0)
        else:
            assert (hdr.ts_base, s.ts_span, s.part_max, s.flags) == want
        # the classes are what their names say
        assert (hdr.mode == M.RAW) == (cls in ("raw_part", "raw_span")) and (hdr.lens == M.LENS_I32) == (cls == "wide_len")
        if want is not None:
            flags = want[3]
            assert bool(flags & M.UNTIMED) == (cls in ("untimed", "some_untimed")) and bool(flags & M.TIMED) == (cls != "untimed")
            assert (want[2] == M.PART_NONE) == (cls == "part_none") and (P <= want[2] < M.PART_NONE) == (cls == "bad_compact")
            assert (want[0] == M.EARLY and want[0] + want[1] == M.LATE) == (cls == "extreme")
    assert M.summary_definition(model, TILES) is None           # the partial last tile: no summary can be VALID


def test_check_layout_refuses_what_it_must():
    """The soundness check itself: a stale VALID summary, a COMPACT header over content that does not fit, u16 lengths over
    a wide length, a VALID summary on the partial last tile."""
    model = M.Model()
    model.apply(M.Upload(0, CAPACITY, 5, 3, ("extreme", "fit", "raw_part", "wide_len", "fit", "fit", "fit")))
    sums = np.zeros(TILES + 1, np.dtype([("ts_span", np.uint32), ("part_max", np.uint16), ("flags", np.uint16)]))
    hdrs = []
    for t in range(TILES + 1):
        c = model.tile(t)
        d = M.summary_definition(model, t)
        fits = M.compactable(c["partition"], c["ts_ms"])
        stamps = c["ts_ms"][c["ts_ms"] != -1]
        hdrs.append((int(stamps.min()) if fits else 0, M.COMPACT if fits else M.RAW,
                     M.LENS_U16 if M.lens_fit(c["key_len"], c["val_len"]) else M.LENS_I32))
        if d is not None:
            sums[t] = d[1:]
    assert [h[1:] for h in hdrs] == [(1, 1), (1, 1), (0, 1), (1, 0), (1, 1), (1, 1), (1, 1)]
    M.check_layout(model, hdrs, sums)
    M.check_layout(model, hdrs, np.zeros_like(sums))             # no summary at all is sound

    def refused(h=hdrs, s=sums):
        with pytest.raises(AssertionError):
            M.check_layout(model, h, s)
    was = int(model.cols["ts_ms"][7])
    model.cols["ts_ms"][7] = M.EARLY - 5                         # content changed behind a VALID summary
    refused()
    model.cols["ts_ms"][7] = was
    was = int(model.cols["partition"][T + 9])
    model.cols["partition"][T + 9] = -1                          # part_max is stale
    refused()
    model.cols["partition"][T + 9] = was
    M.check_layout(model, hdrs, sums)
    refused(h=hdrs[:2] + [(M.BASE_TS, M.COMPACT, M.LENS_U16)] + hdrs[3:])
    refused(h=hdrs[:3] + [(hdrs[3][0], M.COMPACT, M.LENS_U16)] + hdrs[4:])
    bad = sums.copy()
    bad[TILES] = (5, 4, M.VALID | M.TIMED)
    refused(s=bad)
    bad = sums.copy()
    bad["flags"][1] |= M.UNTIMED
    refused(s=bad)

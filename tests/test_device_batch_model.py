"""The generator and the model of tests/device_batch_model.py, without a GPU: over the seed list the GPU test
(tests/test_gpu_device_batch_sequences.py) runs, the sequences must reach every writer, every pair of writers on a common
tile, the cuts through tiles that should carry a summary (the stale-summary case, at the tile's front and at its back),
reader views that start or end inside such a tile, every value class and an extreme timestamp that lives only in a tile a
later writer partly overwrites — so that the GPU test cannot quietly test nothing.  These are conditions, not
measurements: where the seed list misses one, the list or the generator's weights change, not the numbers here.
Seeds 0..19 are held to the ops they always ran by a digest (tests/golden/device_batch_sequences.sha256) and to the
conditions they always met; seeds 20..31, the plane profile, to conditions of their own on marked tiles: cut, written by
both producers, widened, viewed, read under three partition counts, with ids beyond the handler's, with an extreme size
that a cut removes, without a valued record.  The filters of the filtered readers: every kind, and bounds on summaries
written after a cut.
And summary_definition() and plane_definition(), the GPU test's yardsticks for a tile's summary and for its mark, plane
and size words, against the host packer (csrc/kta_tile.h through tests/native/tile_summary.cpp) on whole tiles of every
value class; and check_layout() itself on what it must refuse."""
import ctypes as C
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import device_batch_model as M
from device_batch_model import CAPACITY, T, TILES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cover(seeds):
    """One pass over the sequences of `seeds` with the model and the tracker beside them."""
    cov = {"writers": Counter(), "pairs": Counter(), "cuts": Counter(), "views": 0, "classes": Counter(), "extreme_cut": 0,
           "range_kinds": Counter(), "sequences": {}, "marked_cuts": Counter(), "marked_written": Counter(), "widen_marked": 0,
           "marked_views": 0, "marked_at_read": Counter(), "marked_beyond_P": 0, "size_extreme_cut": 0, "no_values_marked": 0,
           "windows": Counter(), "windows_recut": 0}
    for seed in seeds:
        P = M.P_of(seed)
        ops = M.gen_sequence(seed, CAPACITY, P)
        cov["sequences"][seed] = ops
        model, tracker = M.Model(), M.Tracker()
        for op in ops:
            name = type(op).__name__
            cov["writers"][name] += 1
            if name == "Upload":
                cov["classes"].update(op.classes)
            extreme, size_extreme = M.extreme_tiles(model, P), M.size_extreme_tiles(model, P)
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
            # the tiles that should carry a mark: cut (they were marked before this writer), written, widened, viewed, read
            for t, side in tracker.marked_cuts:
                cov["marked_cuts"][side] += 1
            cov["size_extreme_cut"] += len({t for t, _ in tracker.marked_cuts} & size_extreme)
            cov["marked_written"][name] += sum(tracker.marked[t] is not None for t in M.wrote_whole(op))
            cov["widen_marked"] += bool(tracker.widened)
            cov["marked_views"] += any(tracker.marked[t] for t in inside)
            marked = [t for t in range(TILES) if tracker.marked[t]]
            cov["marked_at_read"][P] += len(marked)
            cov["marked_beyond_P"] += sum(int(model.tile(t)["partition"].max()) >= P for t in marked)
            cov["no_values_marked"] += sum(bool((model.tile(t)["val_len"] == -1).all()) for t in marked)
            for kind, aim, _, _, _ in op.windows:
                cov["windows"][kind] += 1
                cov["windows_recut"] += aim is not None and tracker.summed[aim] and tracker.was_cut[aim]
        for names in tracker.touched:
            for i, a in enumerate(names):
                for b in names[i + 1:]:
                    cov["pairs"][(a, b)] += 1
    return cov


@pytest.fixture(scope="module")
def coverage():
    """The seeds the suite has always run: what they reach is asserted as it always was."""
    return _cover(M.OLD_SEEDS)


@pytest.fixture(scope="module")
def plane_coverage():
    """The seeds of the plane profile."""
    return _cover(M.PLANE_SEEDS)


def test_the_old_seeds_run_the_ops_they_always_ran(coverage):
    """New fields and classes must not move what seeds 0..19 draw: the digest of their ops, on the fields an op had when the
    digests were taken (format_ops_pinned), is the recorded one."""
    import hashlib
    with open(os.path.join(ROOT, "tests", "golden", "device_batch_sequences.sha256")) as f:
        want = {int(line.split()[2]): line.split()[0] for line in f if line.strip()}
    assert sorted(want) == list(M.OLD_SEEDS)
    for seed in M.OLD_SEEDS:
        got = hashlib.sha256(M.format_ops_pinned(coverage["sequences"][seed]).encode()).hexdigest()
        assert got == want[seed], f"seed {seed} no longer generates the ops it did"
        assert all(not isinstance(op, M.Upload) or (op.ids == 0 and not set(op.classes) & set(M.PLANE_CLASSES))
                   for op in coverage["sequences"][seed])


def test_sequences_are_deterministic_and_well_formed(coverage, plane_coverage):
    assert tuple(coverage["sequences"]) + tuple(plane_coverage["sequences"]) == M.SEEDS
    for seed, ops in list(coverage["sequences"].items()) + list(plane_coverage["sequences"].items()):
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
            assert 1 <= len(op.windows) <= 2 and len({w[0] for w in op.windows}) == len(op.windows)
            for kind, aim, frm, to, parts in op.windows:             # what kta_set_filter takes, and a filter at all
                assert kind in M.WINDOW_KINDS and (aim is None or 0 <= aim < TILES)
                assert (frm is None or to is None or frm < to) and (parts is None or (parts and all(0 <= q < M.P_of(seed) for q in parts)))
                assert (parts is not None) == (kind in ("set", "both")) and (frm is not None or to is not None) == (kind != "set")


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


# ---- what the plane profile's seeds reach ----------------------------------------------------------------------------------
def test_the_plane_seeds_run_on_three_partition_counts_and_both_handlers():
    assert {M.P_of(s) for s in M.PLANE_SEEDS} == {5, 256, 300} and all(M.profile_of(s) == "plane" for s in M.PLANE_SEEDS)
    assert {M.P_of(s) for s in M.PLANE_SEEDS if (s // 2) % 2 == 1} == {5, 256, 300}      # the Widen seeds, on the -c handler
    assert all(M.profile_of(s) == "mixed" for s in M.OLD_SEEDS)


def test_every_plane_class_occurs(plane_coverage):
    for cls in M.PLANE_CLASSES:
        assert plane_coverage["classes"][cls] >= 5, (cls, plane_coverage["classes"])


def test_marked_tiles_are_cut_at_the_front_and_at_the_back(plane_coverage):
    assert plane_coverage["marked_cuts"]["front"] >= 5 and plane_coverage["marked_cuts"]["back"] >= 5, plane_coverage["marked_cuts"]


def test_both_whole_tile_producers_write_marked_tiles(plane_coverage):
    for w in ("Upload", "SynthFill"):
        assert plane_coverage["marked_written"][w] >= 10, plane_coverage["marked_written"]


def test_a_widen_meets_marked_tiles(plane_coverage):
    assert plane_coverage["widen_marked"] >= 5, plane_coverage["widen_marked"]


def test_reader_views_start_or_end_inside_a_marked_tile(plane_coverage):
    assert plane_coverage["marked_views"] >= 10, plane_coverage["marked_views"]


def test_marked_tiles_are_read_under_each_partition_count(plane_coverage):
    for P in (5, 256, 300):
        assert plane_coverage["marked_at_read"][P] >= 20, plane_coverage["marked_at_read"]


def test_marked_tiles_hold_ids_beyond_the_handlers_partitions(plane_coverage):
    """Marked, but not for the lean kernel to take: part_max >= P."""
    assert plane_coverage["marked_beyond_P"] >= 5, plane_coverage["marked_beyond_P"]


def test_an_extreme_size_lives_only_in_a_marked_tile_that_is_later_cut(plane_coverage):
    """The size words of that tile then know a size the batch no longer has."""
    assert plane_coverage["size_extreme_cut"] >= 3, plane_coverage["size_extreme_cut"]


def test_a_tile_without_a_value_is_marked_at_a_read(plane_coverage):
    assert plane_coverage["no_values_marked"] >= 3, plane_coverage["no_values_marked"]


def test_every_window_kind_occurs_and_windows_sit_on_summaries_written_after_a_cut(coverage, plane_coverage):
    for kind in M.WINDOW_KINDS:
        assert coverage["windows"][kind] + plane_coverage["windows"][kind] >= 5, kind
    assert coverage["windows_recut"] + plane_coverage["windows_recut"] >= 10


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
    lib.kta_tile_summary_plane.restype = C.c_uint32
    lib.kta_tile_summary_plane.argtypes = [C.POINTER(Hdr)] + [C.c_void_p] * 3 + [C.c_uint64] + [C.c_void_p] * 2
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


POISON = 0xA5A5A5A5


@pytest.mark.parametrize("P", [5, 256, 300])
@pytest.mark.parametrize("cls", M.VALUE_CLASSES + M.PLANE_CLASSES)
def test_plane_definition_is_the_host_packers(packer, cls, P):
    """plane_definition(), the GPU test's yardstick for a mark, a plane and the size words, against kta::tile_plane_host
    behind kta::tile_pack_host on whole tiles of every value class; at P = 300 with the ids as drawn and drawn below 256."""
    for seed, ids in [(s, 0) for s in range(4)] + ([(s, M.PLANE_PARTS) for s in range(4, 6)] if P > M.PLANE_PARTS else []):
        op = M.Upload(T, T, P, seed, (cls,), ids=ids)
        model = M.Model()
        model.apply(op)
        c = {k: np.ascontiguousarray(v) for k, v in M.upload_cols(op).items()}
        img = [np.zeros(T * 8, np.uint8) for _ in range(4)]
        hdr, s, sizes = Hdr(), Sum(), np.full(2, POISON, np.uint32)
        packer.kta_tile_summary_pack(c["partition"].ctypes.data, c["ts_ms"].ctypes.data, c["key_len"].ctypes.data, c["val_len"].ctypes.data,
                                     T, 1, *[x.ctypes.data for x in img], C.byref(hdr), C.byref(s))
        before = img[1].copy()
        mark = packer.kta_tile_summary_plane(C.byref(hdr), c["partition"].ctypes.data, c["key_len"].ctypes.data, c["val_len"].ctypes.data,
                                             T, img[1].ctypes.data, sizes.ctypes.data)
        want = M.plane_definition(model, 1)
        tile = model.tile(1)
        assert mark == (want is not None) and np.array_equal(img[1][:T * 4], before[:T * 4])
        assert (want is not None) == (hdr.mode == M.COMPACT and M.plane_fits(tile["partition"], tile["key_len"], tile["val_len"]))
        if want is None:
            assert np.array_equal(img[1], before) and sizes.tolist() == [POISON, POISON]      # nothing written without a mark
        else:
            assert np.array_equal(img[1][T * 4:].view(np.uint32), want[0]) and tuple(int(x) for x in sizes) == want[1]
            assert M.summary_definition(model, 1) is not None
        # the classes are what their names say
        ids_fit = P <= M.PLANE_PARTS or ids == M.PLANE_PARTS
        never = ("raw_part", "raw_span", "wide_len", "part_none", "bad_compact", "key_255", "part_256")
        assert cls not in never or want is None
        if cls in M.PLANE_CLASSES and cls not in never:
            assert want is not None                                     # (their ids stay below 256 under any P)
        elif cls not in never:
            assert (want is not None) == ids_fit
        p, k, v = tile["partition"], tile["key_len"], tile["val_len"]
        if cls == "plane_edge":
            assert int(p.max()) == min(P, M.PLANE_PARTS) - 1 and ((k == M.KEY_MAX) & (v == M.VAL_MAX)).any()
            assert ((k == -1) & (v == -1)).any() and ((k == 0) & (v == 0)).any() and want[1][1] == M.KEY_MAX + M.VAL_MAX
            quads = [q for q in range(0, T, 4) if len({(int(p[j]), int(k[j]), int(v[j])) for j in range(q, q + 4)}) == 1]
            assert quads and (want[0] >> 16 == M.LEN_NONE).any() and ((want[0] >> 8) & 0xFF == M.PLANE_KEY_NONE).any()
        elif cls == "key_255":
            assert (k == M.KEY_MAX + 1).sum() == 1 and M.lens_fit(k, v) and hdr.mode == M.COMPACT      # a lean tile without a plane
        elif cls == "part_256":
            assert (p == M.PLANE_PARTS).sum() == 1 and hdr.mode == M.COMPACT and int(((p < 0) | (p >= P)).sum()) == (P <= 256)
        elif cls == "no_values":
            assert (v == -1).all() and want[1] == M.SIZE_NONE
        elif cls == "size_extreme":
            assert want[1] == (0, M.KEY_MAX + M.VAL_MAX)
            sz = np.sort(np.maximum(k, 0) + v)
            assert sz[1] >= 110 and sz[-2] < 1040                       # the band: only those two records are outside
    assert M.plane_definition(model, TILES) is None                    # the partial last tile: no mark can be 1


def test_check_layout_refuses_what_it_must():
    """The soundness check itself: a stale VALID summary, a COMPACT header over content that does not fit, u16 lengths over
    a wide length, a VALID summary on the partial last tile; behind a mark of 1 a stale plane word, a stale size word, a
    record that fits no plane, the partial last tile; and of a tile written whole in this step a missing summary or a
    wrong mark."""
    model = M.Model()
    model.apply(M.Upload(0, CAPACITY, 5, 3, ("extreme", "fit", "raw_part", "wide_len", "fit", "fit", "fit")))
    sums = np.zeros(TILES + 1, np.dtype([("ts_span", np.uint32), ("part_max", np.uint16), ("flags", np.uint16)]))
    hdrs, marks, sizes, planes = [], np.zeros(TILES + 1, np.uint32), np.full((TILES + 1, 2), POISON, np.uint32), np.full((TILES, T), POISON, np.uint32)
    for t in range(TILES + 1):
        c = model.tile(t)
        d = M.summary_definition(model, t)
        fits = M.compactable(c["partition"], c["ts_ms"])
        stamps = c["ts_ms"][c["ts_ms"] != -1]
        hdrs.append((int(stamps.min()) if fits else 0, M.COMPACT if fits else M.RAW,
                     M.LENS_U16 if M.lens_fit(c["key_len"], c["val_len"]) else M.LENS_I32))
        if d is not None:
            sums[t] = d[1:]
        plane = M.plane_definition(model, t)
        if plane is not None:
            marks[t], planes[t], sizes[t] = 1, plane[0], plane[1]
    assert [h[1:] for h in hdrs] == [(1, 1), (1, 1), (0, 1), (1, 0), (1, 1), (1, 1), (1, 1)]
    assert marks.tolist() == [1, 1, 0, 0, 1, 1, 0]
    side = (marks, sizes, planes)
    whole = list(range(TILES))
    M.check_layout(model, hdrs, sums, *side, wrote=whole)
    M.check_layout(model, hdrs, np.zeros_like(sums), *side)      # no summary at all is sound, and the marks then say nothing
    M.check_layout(model, hdrs, np.zeros_like(sums), np.ones_like(marks), np.zeros_like(sizes), np.zeros_like(planes))
    M.check_layout(model, hdrs, sums, np.zeros_like(marks), sizes, planes)     # nor is an earlier writer's tile owed a mark
    raw = [(0, M.RAW, M.LENS_I32)] * (TILES + 1)                  # a raw producer over marked tiles: marks and words stay, unjudged
    M.check_layout(model, raw, sums, np.ones_like(marks), np.zeros_like(sizes), np.zeros_like(planes))

    def refused(h=hdrs, s=sums, marks=marks, sizes=sizes, planes=planes, wrote=(), match=None):
        with pytest.raises(AssertionError, match=match):
            M.check_layout(model, h, s, marks, sizes, planes, wrote=wrote)
    bad = planes.copy()
    bad[4][1023] ^= 1 << 8                                       # a stale plane word behind a mark of 1
    refused(planes=bad, match="tile 4: the plane's words")
    for col, what in ((0, "size_min"), (1, "size_max")):
        bad = sizes.copy()
        bad[1][col] += 1                                         # a stale size word
        refused(sizes=bad, match="tile 1: size words")
    for name, value in (("key_len", 255), ("partition", 256)):   # a mark of 1 over a record that fits no plane
        was = int(model.cols[name][T + 5])
        model.cols[name][T + 5] = value
        now = sums.copy()
        now[1] = M.summary_definition(model, 1)[1:]
        refused(s=now, match="tile 1: a mark of 1")
        unmarked = marks.copy()
        unmarked[1] = 0
        M.check_layout(model, hdrs, now, unmarked, sizes, planes, wrote=whole)
        model.cols[name][T + 5] = was
    bad, last = sums.copy(), marks.copy()
    bad[TILES], last[TILES] = (5, 4, M.VALID | M.TIMED), 1       # a mark of 1 on the partial last tile beside a VALID summary
    refused(s=bad, marks=last, match=f"tile {TILES}: a mark of 1")
    unmarked = marks.copy()
    unmarked[0] = 0                                              # written whole in this step, every record fits: the mark is owed
    refused(marks=unmarked, wrote=whole, match="tile 0: written whole in this step: mark 0")
    bad = sums.copy()
    bad[3] = (0, 0, 0)                                           # written whole in this step, compactable: the summary is owed
    refused(s=bad, wrote=whole, match="tile 3: written whole in this step, compactable")
    M.check_layout(model, hdrs, bad, *side, wrote=[0, 1, 2, 4, 5])
    was = int(model.cols["ts_ms"][7])
    model.cols["ts_ms"][7] = M.EARLY - 5                         # content changed behind a VALID summary
    refused(match="tile 0: summary")
    model.cols["ts_ms"][7] = was
    was = int(model.cols["partition"][T + 9])
    model.cols["partition"][T + 9] = -1                          # part_max is stale
    refused(marks=np.zeros_like(marks), match="tile 1: summary")
    model.cols["partition"][T + 9] = was
    M.check_layout(model, hdrs, sums, *side)
    refused(h=hdrs[:2] + [(M.BASE_TS, M.COMPACT, M.LENS_U16)] + hdrs[3:])
    refused(h=hdrs[:3] + [(hdrs[3][0], M.COMPACT, M.LENS_U16)] + hdrs[4:])
    bad = sums.copy()
    bad[TILES] = (5, 4, M.VALID | M.TIMED)
    refused(s=bad, match=f"tile {TILES}: a VALID summary")
    bad = sums.copy()
    bad["flags"][1] |= M.UNTIMED
    refused(s=bad, match="tile 1: summary")

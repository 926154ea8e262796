"""The scan plane (include/kta_hip.h): a compact tile of 1024 records that all fit one dword —
partition | key << 8 | val << 16 — carries them a second time in the unused half of its ts_ms bytes, its mark says so, and
the lean kernel of the packed scan reads such a tile from the plane alone (lean_run<NT, true>), 4 B per record.

Every case compares finish() — the result and counters[P, 7] — bit for bit with the C oracle on the same columns (as
test_gpu_scan_lean._checked does), under scan variants 0, 16 (non-temporal loads), 48 (no summaries), 64 and 80 (the marks
are ignored: every summarised tile is read in its u16 form), and the five must agree.  The marks are read back through
kta_batch_tile_planes.  Shapes are 1 to 70 tiles, with 1, 3 or 8 workgroups."""
import ctypes as C

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
from helpers import NOW
from test_gpu_scan_lean import FT, LEAN, NT_EXC, PATTERNS, _checked
from test_gpu_scan_packed import BASE_TS, COLS, T, _tile_hdrs, _topic

pytestmark = pytest.mark.gpu

VARIANTS = (0, 16, 48, 64, 80)
VALID = N.KTA_TILE_SUM_VALID
I32 = (N.KTA_TILE_COMPACT, N.KTA_TILE_LENS_I32)
RAW = (N.KTA_TILE_RAW, N.KTA_TILE_LENS_U16)


def _view(b, lo):
    v = kta.KtaBatch()
    for f, sz in COLS:
        setattr(v, f, getattr(b, f) + lo * sz)
    return v


def _scan_all(h, b, P, cols, workgroups=(1,), views=()):
    """The batch (or every (lo, m) of `views`) under the five variants and every grid of `workgroups`."""
    n = len(cols["partition"])
    for wgs in workgroups:
        for lo, m in (views or ((0, n),)):
            got = []
            for variant in VARIANTS:
                h.reset()
                h.set_tuning(scan_workgroups=wgs, scan_variant=variant)
                h.submit_device(b if lo == 0 else _view(b, lo), m, 0, which=1)
                got.append(_checked(h, P, {k: cols[k][lo:lo + m] for k, _ in COLS}))
            assert all(g == got[0] for g in got), "the scan variants disagree"


def _five(P, cols, workgroups=(1,), views=(), marks=None, expect_hdrs=None):
    """Upload, check the marks (and the headers), scan."""
    n = len(cols["partition"])
    with kta.HipMetricHandler(P, now=NOW) as h:
        b, _ = h.upload_batch(cols)
        if expect_hdrs is not None:
            assert _tile_hdrs(h, b, len(expect_hdrs)) == expect_hdrs
        if marks is not None:
            assert h.batch_tile_planes(b, n).tolist() == marks
        _scan_all(h, b, P, cols, workgroups, views)
        h.device_batch_free(b)


def _upload_into(h, b, cols):
    metric = {k: np.ascontiguousarray(cols[k]) for k, _ in COLS}
    h._check(h._lib.kta_batch_from_raw(h._ctx, C.byref(kta._host_batch(metric)), len(metric["partition"]), C.byref(b)))


# ---- the ring fills and drains ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [256, 5, 1])
def test_ring_fill_and_drain(P):
    for ntiles in (1, 2, 3, 4, 5):                      # one workgroup
        cols = _topic(ntiles * T, P, seed=21)
        if P == 256:
            cols["partition"][ntiles * T - 3] = 255     # no marker: id 255 is a partition like any other
        _five(P, cols, workgroups=(1,), marks=[1] * ntiles, expect_hdrs=[LEAN] * ntiles)
    for ntiles in (3 * 2 - 1, 3 * 2, 3 * 2 + 1):        # W k - 1, W k, W k + 1 tiles, W = 3 workgroups
        cols = _topic(ntiles * T, P, seed=22)
        if P == 256:
            cols["partition"][5] = 255
        _five(P, cols, workgroups=(3,), marks=[1] * ntiles)
    _five(P, _topic(3 * T, P, seed=23), workgroups=(8,), marks=[1] * 3)   # more workgroups than tiles
    _five(P, _topic(2 * T + 37, P, seed=24), workgroups=(1, 3), marks=[1, 1, 0])   # a partial last tile has no plane


# ---- edges inside a marked tile ---------------------------------------------------------------------------------------
def test_edges_inside_a_marked_tile():
    P, ntiles = 256, 3
    cols = _topic(ntiles * T, P, seed=25)
    k, v, p = cols["key_len"], cols["val_len"], cols["partition"]
    k[T + 1], k[T + 2], k[T + 3] = 254, -1, 0           # the longest key that fits, no key, an empty key
    v[T + 5], v[T + 6], v[T + 7] = 65534, -1, 0         # the longest value that fits, a tombstone, an empty value
    k[T + 8], v[T + 8], p[T + 8] = 254, 65534, 255      # all three at once: the largest message of the batch
    k[T + 9], v[T + 9], p[T + 9] = -1, -1, 0
    k[2 * T:2 * T + 4], v[2 * T:2 * T + 4], p[2 * T:2 * T + 4] = 254, 65534, 255   # a lane's four records alike: one add
    _five(P, cols, workgroups=(1, 3), marks=[1] * ntiles, expect_hdrs=[LEAN] * ntiles)


# ---- tiles that must not be marked, at every position of the ring and of the front interval -------------------------
def _make_unmarked(kind, cols, tile):
    """Turn one tile into the kind; -> its expected header."""
    p, t, k, v = cols["partition"], cols["ts_ms"], cols["key_len"], cols["val_len"]
    s = tile * T
    if kind == "key_255":
        k[s + 9] = 255
        return LEAN
    if kind == "part_none":
        p[s + 7] = -1
        return LEAN
    if kind == "part_256":
        p[s + 7] = 256
        return LEAN
    if kind == "val_70000":
        v[s + 9] = 70000
        return I32
    assert kind == "raw"                                # a timestamp span of 2^31
    t[s + 1], t[s + 5] = BASE_TS, BASE_TS + (1 << 31)
    return RAW


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("kind", ["key_255", "part_none", "part_256", "val_70000", "raw"])
def test_tiles_that_must_not_be_marked(kind, pattern):
    """(key_255 and part_256 stay lean tiles of the 6-byte form next to plane tiles: the two forms of the loop alternate.)"""
    P = 300 if kind == "part_256" else 8
    cols = _topic(NT_EXC * T, 8, seed=31)
    hdrs, marks = [LEAN] * NT_EXC, [1] * NT_EXC
    for tile in PATTERNS[pattern]:
        hdrs[tile] = _make_unmarked(kind, cols, tile)
        marks[tile] = 0
    _five(P, cols, workgroups=(1,), marks=marks, expect_hdrs=hdrs)


def test_forms_alternate_with_three_workgroups():
    """Plane tiles and 6-byte lean tiles (one key of 255) alternate; three workgroups deal them so that one sees one form
    only and the others both."""
    ntiles = 20
    cols = _topic(ntiles * T, 8, seed=33)
    for tile in range(0, ntiles, 2):
        cols["key_len"][tile * T + tile] = 255
    _five(8, cols, workgroups=(1, 3, 8), marks=[t % 2 for t in range(ntiles)], expect_hdrs=[LEAN] * ntiles)


# ---- marked but not taken ----------------------------------------------------------------------------------------------
def test_marked_but_not_taken():
    """A handler of 200 partitions over marked tiles whose part_max is 255: every record of 200..255 is bad."""
    ntiles = 12
    cols = _topic(ntiles * T, 256, seed=51)
    cols["partition"][np.arange(ntiles) * T + 11] = 255
    _five(200, cols, workgroups=(1, 3), marks=[1] * ntiles)


# ---- views -------------------------------------------------------------------------------------------------------------
def test_views_cut_the_first_and_the_last_tile():
    P = 8
    n = NT_EXC * T
    _five(P, _topic(n, P, seed=32), workgroups=(1, 3), marks=[1] * NT_EXC,
          views=((4, n - 4), (0, n - T + 37), (T + 4, n - 2 * T - 4 + 37), (2 * T, 3 * T)))


# ---- state changes -----------------------------------------------------------------------------------------------------
def test_a_raw_producer_writes_into_a_marked_tile():
    P, ntiles = 8, 5
    n = ntiles * T
    cols = _topic(n, P, seed=41)
    sp, _ = kta.synth_preset("c2")
    sp.n_partitions, sp.seed = P, 77
    lo, m = T + 4, T // 2                               # inside tile 1 only
    patch = kta.synth_fill_host(sp, 0, m)
    with kta.HipMetricHandler(P, now=NOW) as h:
        b, _ = h.upload_batch(cols)
        assert h.batch_tile_planes(b, n).tolist() == [1] * ntiles
        v = _view(b, lo)
        v.capacity = m
        h.synth_fill_device(sp, 0, m, v)                # not from a tile boundary: the raw fill, its tile made raw first
        for k, _ in COLS:
            cols[k][lo:lo + m] = patch[k]
        assert _tile_hdrs(h, b, ntiles) == [LEAN, (N.KTA_TILE_RAW, N.KTA_TILE_LENS_I32)] + [LEAN] * 3   # (the lengths are widened with it)
        _scan_all(h, b, P, cols, workgroups=(1, 3))     # (the mark of tile 1 may still be 1: next to a RAW header it says nothing)
        h.device_batch_free(b)


def test_lengths_widened_keep_the_plane():
    """A -c handler is handed a view of a keyless batch with key columns of its own: the lengths of its tiles are widened
    (i32); the marks stay, the plane is still right, and such a tile is taken through the plane (not as a lean tile)."""
    P, n = 8, 4 * T + 37
    sp, _ = kta.synth_preset("c2")
    sp.n_partitions, sp.part_mode = P, N.KTA_PART_RANDOM
    cols = {k: np.array(v) for k, v in kta.synth_fill_host(sp, 0, n, with_keys=True).items()}
    metric = {k: cols[k] for k, _ in COLS}
    with kta.HipMetricHandler(P, now=NOW, count_alive_keys=True) as h:
        b, _ = h.upload_batch(metric)
        keyed, _ = h.upload_batch(cols, with_keys=True)
        assert h.batch_tile_planes(b, n).tolist() == [1] * 4 + [0]
        assert h.batch_tile_planes(keyed, n).tolist() == [1] * 4 + [0]   # keyed allocations have planes too
        v = _view(b, 0)
        v.key_off, v.key_bytes = keyed.key_off, keyed.key_bytes
        h.submit_device(v, n, 0, which=2)               # the alive-key pass: widens the lengths first
        assert _tile_hdrs(h, b, 5) == [I32] * 5
        assert h.batch_tile_planes(b, n).tolist() == [1] * 4 + [0]
        _scan_all(h, b, P, metric, workgroups=(1, 3))
        _scan_all(h, keyed, P, metric, workgroups=(1,))
        h.device_batch_free(keyed)
        h.device_batch_free(b)


@pytest.mark.parametrize("producer", ["from_raw", "synth"])
def test_refill_clears_and_sets_the_mark(producer):
    P, ntiles = 8, 4
    n = ntiles * T
    sp, _ = kta.synth_preset("c2")
    sp.n_partitions = P
    long_keys, _ = kta.synth_preset("c2")
    long_keys.n_partitions, long_keys.seed = P, 9
    for i in range(long_keys.n_key_lens):
        long_keys.key_lens[i] = 300                     # no record with a key fits
    with kta.HipMetricHandler(P, now=NOW) as h:
        b = h.device_batch_alloc(n)
        assert h.batch_tile_planes(b, n).tolist() == [0] * ntiles   # a fresh allocation has none
        for spec, want in ((sp, 1), (long_keys, 0), (sp, 1)):
            cols = {k: v for k, v in kta.synth_fill_host(spec, 0, n).items() if k in dict(COLS)}
            if producer == "synth":
                h.synth_fill_device(spec, 0, n, b)
            else:
                _upload_into(h, b, cols)
            assert _tile_hdrs(h, b, ntiles) == [LEAN] * ntiles
            assert all(int(x) & VALID for x in h.batch_tile_summaries(b, n)["flags"])
            assert h.batch_tile_planes(b, n).tolist() == [want] * ntiles
            _scan_all(h, b, P, cols, workgroups=(1, 3))
        h.device_batch_free(b)


def test_device_and_host_producer_write_the_same_marks_and_planes():
    sp, _ = kta.synth_preset("c4")
    n = 4 * T + 37
    with kta.HipMetricHandler(sp.n_partitions, now=NOW) as h:
        d = h.device_batch_alloc(n)
        h.synth_fill_device(sp, 0, n, d)
        host_cols = kta.synth_fill_host(sp, 0, n)
        u, _ = h.upload_batch({k: host_cols[k] for k, _ in COLS})
        assert h.batch_tile_planes(d, n).tolist() == h.batch_tile_planes(u, n).tolist() == [1] * 4 + [0]
        img = [np.empty(4 * T, np.uint64) for _ in range(2)]         # the ts_ms bytes of the four whole tiles
        for a, b in zip(img, (d, u)):
            h._check(h._lib.kta_copy_to_host(h._ctx, a.ctypes.data, b.ts_ms, a.nbytes))
        assert img[0].tobytes() == img[1].tobytes()
        w = img[0].view(np.uint32).reshape(4, 2 * T)[:, T:].reshape(-1)   # the planes: the second half of each tile's bytes
        p, k, v = (host_cols[c][:4 * T].astype(np.int64) for c in ("partition", "key_len", "val_len"))
        assert np.array_equal(w, (p | ((k & 0xFF) << 8) | ((v & 0xFFFF) << 16)).astype(np.uint32))
        assert h.batch_tile_planes(_view(d, 2 * T), 2 * T).tolist() == [1, 1]
        with pytest.raises(kta.KtaError) as e:
            h.batch_tile_planes(_view(d, 2 * T + 4), T)
        assert e.value.code == N.KTA_ERR_INVALID
        h.device_batch_free(u)
        h.device_batch_free(d)


# ---- config 4 ----------------------------------------------------------------------------------------------------------
def test_config_4_is_marked_throughout():
    """The headline's batch: were a tile of config 4 not marked, bench.py would silently stay on the 6-byte path."""
    sp, _ = kta.synth_preset("c4")
    n = 1 << 20
    with kta.HipMetricHandler(sp.n_partitions, now=NOW) as h:
        b = h.device_batch_alloc(n)
        h.synth_fill_device(sp, 0, n, b)
        assert int(h.batch_tile_planes(b, n).sum()) == n // T
        h.device_batch_free(b)


# ---- runs and odd P ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["random", "runs"])
@pytest.mark.parametrize("P", [1, 5, 256, 300])
def test_runs_and_odd_p(P, order):
    ntiles = 2 * FT + 6                                 # the plan's grid; every workgroup meets a front flush or none
    cols = _topic(ntiles * T, P, seed=61, runs=(order == "runs"))
    _five(P, cols, workgroups=(0, 1))

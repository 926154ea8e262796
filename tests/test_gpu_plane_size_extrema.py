"""The plane tiles' size extrema and raw sums (csrc/kta_tile.h): the producers of a marked tile write
the least and the largest key + value size of its valued records into two words behind the marks, the plane loop of the
lean kernel no longer looks at sizes per record and folds those words behind the loop, and it adds the lengths as stored
— 0xFF for a key of -1, 0xFFFF for a value of -1 — which the front flush takes out again by the interval's counts of null
keys and tombstones.

Every scan compares finish() — counters[P, 7] and the four extrema — bit for bit with the C oracle on the same columns
(test_gpu_scan_lean._checked) under scan variants 0, 16, 48, 64 and 80, and the five must agree.  Batches are 1 to 33
tiles, built from numpy columns with kta_batch_from_raw."""
import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
from helpers import NOW
from test_gpu_scan_lean import FT, LEAN, _checked
from test_gpu_scan_packed import BASE_TS, COLS, T, _tile_hdrs
from test_gpu_scan_plane import VARIANTS, _five, _upload_into, _view

pytestmark = pytest.mark.gpu

KEY_MAX, VAL_MAX = 254, 65534                           # the largest lengths that fit a plane
SIDE_BEFORE_SIZES = 16 + 8 + 4                          # kta_tile.h's address rule: headers, summaries, marks, then the sizes
NONE = (0xFFFFFFFF, 0)                                  # the two words of a tile without a valued record
KEY_SUM, VAL_SUM = N.KTA_C_KEY_SIZE_SUM, N.KTA_C_VALUE_SIZE_SUM


def _cols(p, k, v):
    n = len(p)
    return {"partition": np.ascontiguousarray(p, np.int32), "key_len": np.ascontiguousarray(k, np.int32),
            "val_len": np.ascontiguousarray(v, np.int32), "ts_ms": (BASE_TS + np.arange(n)).astype(np.int64)}


def _plain(n, P, seed):
    """Keys of 10..49 and values of 100..999 bytes, a twentieth of the records without a key, a twentieth without a
    value: every sized record has between 100 and 1048 bytes."""
    rng = np.random.default_rng(seed)
    k, v = rng.integers(10, 50, n), rng.integers(100, 1000, n)
    k[rng.random(n) < 0.05] = -1
    v[rng.random(n) < 0.05] = -1
    return _cols(rng.integers(0, P, n), k, v)


def _sizes(cols):
    """(smallest, largest) key + value size over the records with a value, NONE without one: the oracle's rule."""
    k, v = cols["key_len"].astype(np.int64), cols["val_len"].astype(np.int64)
    sz = (np.maximum(k, 0) + v)[v != -1]
    return (int(sz.min()), int(sz.max())) if len(sz) else NONE


def _scan(h, b, P, cols, workgroups=(1,), lo=0, m=None):
    """Records [lo, lo + m) of the batch under the five variants and every grid; -> (counters[P, 7], smallest, largest)."""
    m = len(cols["partition"]) - lo if m is None else m
    got = []
    for wgs in workgroups:
        for variant in VARIANTS:
            h.reset()
            h.set_tuning(scan_workgroups=wgs, scan_variant=variant)
            h.submit_device(b if lo == 0 else _view(b, lo), m, 0, which=1)
            got.append(_checked(h, P, {c: cols[c][lo:lo + m] for c, _ in COLS}))
    assert all(g == got[0] for g in got), "the scan variants disagree"
    return np.frombuffer(got[0][0], np.uint64).reshape(P, 7), got[0][3], got[0][4]


def _size_words(h, b, ntiles):
    """The two size words of the first ntiles tiles of an allocation, by kta_tile.h's address rule."""
    alloc_tiles = max(1, (b.capacity + T - 1) // T)
    out = np.empty(2 * ntiles, np.uint32)
    h._check(h._lib.kta_copy_to_host(h._ctx, out.ctypes.data, b.tile_hdr + alloc_tiles * SIDE_BEFORE_SIZES, out.nbytes))
    return [tuple(int(x) for x in w) for w in out.reshape(ntiles, 2)]


# ---- all nulls and tombstones ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_full", [False, True])
def test_all_null_keys_and_tombstones(one_full):
    """Every record adds 0xFF and 0xFFFF to the raw sums; the flush must bring both sums to exactly 0 (or to the one
    full record's 254 and 65534), and the tiles' size words say "none" (or that one record's size)."""
    P, n = 8, 2 * T
    rng = np.random.default_rng(5)
    cols = _cols(rng.integers(0, P, n), np.full(n, -1), np.full(n, -1))
    if one_full:
        cols["partition"][T + 77], cols["key_len"][T + 77], cols["val_len"][T + 77] = 3, KEY_MAX, VAL_MAX
    with kta.HipMetricHandler(P, now=NOW) as h:
        b, _ = h.upload_batch(cols)
        assert h.batch_tile_planes(b, n).tolist() == [1, 1]
        full = (KEY_MAX + VAL_MAX, KEY_MAX + VAL_MAX)
        assert _size_words(h, b, 2) == [NONE, full if one_full else NONE]
        c, smallest, largest = _scan(h, b, P, cols, workgroups=(1, 3))
        want_k, want_v = np.zeros(P, np.uint64), np.zeros(P, np.uint64)
        if one_full:
            want_k[3], want_v[3] = KEY_MAX, VAL_MAX
            assert (smallest, largest) == full
        assert np.array_equal(c[:, KEY_SUM], want_k) and np.array_equal(c[:, VAL_SUM], want_v)
        assert int(c[:, N.KTA_C_TOMBSTONES].sum()) == int(c[:, N.KTA_C_KEY_NULL].sum()) == n - one_full
        h.device_batch_free(b)


# ---- a front interval at its bounds -----------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 256])
@pytest.mark.parametrize("fill", ["longest", "null_key_tombstone"])
def test_a_front_interval_at_its_bounds(P, fill):
    """One workgroup, FT + 1 whole marked tiles: the first FT fill one front interval to the bound of its fields (every
    record the longest key and value, or every record both markers), the last crosses the flush.  P = 1: one slot group
    takes everything, through the uniform-quad path; P = 256 with partition = record % 256: the per-record path."""
    assert FT == 32
    n = (FT + 1) * T
    k, v = (KEY_MAX, VAL_MAX) if fill == "longest" else (-1, -1)
    cols = _cols(np.arange(n) % P, np.full(n, k), np.full(n, v))
    with kta.HipMetricHandler(P, now=NOW) as h:
        b, _ = h.upload_batch(cols)
        assert h.batch_tile_planes(b, n).tolist() == [1] * (FT + 1)
        c, smallest, largest = _scan(h, b, P, cols, workgroups=(1,))
        per = n // P
        assert c[:, KEY_SUM].tolist() == [per * max(k, 0)] * P and c[:, VAL_SUM].tolist() == [per * max(v, 0)] * P
        if fill == "longest":
            assert (smallest, largest) == (KEY_MAX + VAL_MAX, KEY_MAX + VAL_MAX)
        h.device_batch_free(b)


# ---- the two forms inside one front interval --------------------------------------------------------------------------
@pytest.mark.parametrize("every", [2, 3])
def test_forms_alternate_inside_one_front_interval(every):
    """Marked tiles (raw sums, corrected at the flush) and unmarked u16 tiles (a 300-byte key; exact sums) in turn, with
    null keys and tombstones in both kinds, all inside one front interval of a workgroup: one correction rule must not be
    applied to the other form's records.  With three workgroups and every third tile unmarked, one workgroup sees the
    6-byte form only and two the plane form only; with every second, all three see both."""
    P, ntiles = 8, 14
    assert ntiles < FT
    cols = _plain(ntiles * T, P, seed=71)
    marks = [1] * ntiles
    for tile in range(0, ntiles, every):
        cols["key_len"][tile * T + tile] = 300
        marks[tile] = 0
    for tile in range(ntiles):                          # both markers in every tile, whatever the draw
        cols["key_len"][tile * T + 500], cols["val_len"][tile * T + 501] = -1, -1
        cols["key_len"][tile * T + 502], cols["val_len"][tile * T + 502] = -1, -1
    _five(P, cols, workgroups=(1, 3), marks=marks, expect_hdrs=[LEAN] * ntiles)


# ---- the extrema come from the right tiles ----------------------------------------------------------------------------
def test_smallest_size_in_a_marked_tile_that_a_view_cuts():
    """The view's smallest record lies in tile 0, which the view cuts (it starts at record 4): that tile goes to the rest
    kernel, record by record.  A smaller record lies in front of the view: tile 0's size words know it, the view's result
    must not."""
    P, n = 8, 4 * T
    cols = _plain(n, P, seed=72)
    cols["key_len"][1], cols["val_len"][1] = 0, 0       # not in the view
    cols["key_len"][100], cols["val_len"][100] = 0, 1   # the view's smallest
    assert _sizes(cols)[0] == 0 and _sizes({c: cols[c][4:] for c, _ in COLS})[0] == 1
    with kta.HipMetricHandler(P, now=NOW) as h:
        b, _ = h.upload_batch(cols)
        assert h.batch_tile_planes(b, n).tolist() == [1] * 4
        assert _size_words(h, b, 1)[0][0] == 0
        assert _scan(h, b, P, cols, workgroups=(1, 3), lo=4)[1] == 1
        assert _scan(h, b, P, cols, workgroups=(1, 3))[1] == 0
        h.device_batch_free(b)


@pytest.mark.parametrize("producer", ["from_raw", "synth"])
def test_largest_size_in_a_tile_whose_mark_a_refill_cleared(producer):
    """Tile 1 is marked and holds the largest record a plane can; a refill gives it 300-byte keys: its mark is cleared,
    and its two words are vouched for by nothing (the device producer leaves them as they were: larger than anything the
    refill holds).  The refill's largest record lies in that tile (from_raw) or in tiles like it (synth: none is marked)."""
    P, n = 8, 4 * T
    first = _plain(n, P, seed=73)
    first["key_len"][T + 9], first["val_len"][T + 9] = KEY_MAX, VAL_MAX
    long_keys, _ = kta.synth_preset("c2")
    long_keys.n_partitions, long_keys.seed, long_keys.val_mode, long_keys.val_mean = P, 9, N.KTA_VAL_FIXED, 1000
    for i in range(long_keys.n_key_lens):
        long_keys.key_lens[i] = 300
    if producer == "synth":
        second = {c: a for c, a in kta.synth_fill_host(long_keys, 0, n).items() if c in dict(COLS)}
        marks = [0] * 4
    else:
        second = _plain(n, P, seed=74)
        second["key_len"][T + 9], second["val_len"][T + 9] = 300, 1000
        marks = [1, 0, 1, 1]
    assert _sizes(second)[1] == 1300 < KEY_MAX + VAL_MAX
    with kta.HipMetricHandler(P, now=NOW) as h:
        b = h.device_batch_alloc(n)
        _upload_into(h, b, first)
        assert h.batch_tile_planes(b, n).tolist() == [1] * 4
        assert _scan(h, b, P, first, workgroups=(1, 3))[2] == KEY_MAX + VAL_MAX
        if producer == "synth":
            h.synth_fill_device(long_keys, 0, n, b)
            assert _size_words(h, b, 2)[1][1] == KEY_MAX + VAL_MAX      # stale
        else:
            _upload_into(h, b, second)
        assert h.batch_tile_planes(b, n).tolist() == marks
        assert _scan(h, b, P, second, workgroups=(1, 3))[2] == 1300
        h.device_batch_free(b)


def test_stale_size_words_behind_a_tile_that_a_raw_producer_overwrote():
    """Tile 1's size words hold the job's smallest and largest size; a raw producer then overwrites those records (the
    tile turns RAW, mark and words stay as they are)."""
    P, ntiles = 8, 4
    n = ntiles * T
    cols = _plain(n, P, seed=75)
    cols["key_len"][T + 10], cols["val_len"][T + 10] = 0, 0
    cols["key_len"][T + 11], cols["val_len"][T + 11] = KEY_MAX, VAL_MAX
    sp, _ = kta.synth_preset("c2")
    sp.n_partitions, sp.seed, sp.val_mode, sp.val_mean, sp.val_empty_permille = P, 78, N.KTA_VAL_FIXED, 200, 0
    lo, m = T + 4, T // 2                               # inside tile 1 only, over both records
    patch = kta.synth_fill_host(sp, 0, m)
    with kta.HipMetricHandler(P, now=NOW) as h:
        b, _ = h.upload_batch(cols)
        assert _size_words(h, b, 2)[1] == (0, KEY_MAX + VAL_MAX)
        v = _view(b, lo)
        v.capacity = m
        h.synth_fill_device(sp, 0, m, v)
        for c, _ in COLS:
            cols[c][lo:lo + m] = patch[c]
        assert _tile_hdrs(h, b, ntiles) == [LEAN, (N.KTA_TILE_RAW, N.KTA_TILE_LENS_I32)] + [LEAN] * 2
        assert _size_words(h, b, 2)[1] == (0, KEY_MAX + VAL_MAX)
        want = _sizes(cols)
        assert 0 < want[0] and want[1] < KEY_MAX + VAL_MAX
        assert _scan(h, b, P, cols, workgroups=(1, 3))[1:] == want
        h.device_batch_free(b)


# ---- host and device producers ----------------------------------------------------------------------------------------
def test_device_and_host_producer_write_the_same_size_words():
    """synth_fill_tiles and tile_plane_host, the same records: two tiles of config 4, then two of which no record has a
    value, then a partial tile (not marked: its words are nobody's)."""
    sp, _ = kta.synth_preset("c4")
    tombs, _ = kta.synth_preset("c4")
    tombs.tombstone_permille, tombs.val_empty_permille = 1000, 0
    n = 4 * T + 37
    with kta.HipMetricHandler(sp.n_partitions, now=NOW) as h:
        d = h.device_batch_alloc(n)
        h.synth_fill_device(sp, 0, 2 * T, d)
        rest = _view(d, 2 * T)
        rest.capacity = n - 2 * T
        h.synth_fill_device(tombs, 2 * T, n - 2 * T, rest)
        a, z = kta.synth_fill_host(sp, 0, 2 * T), kta.synth_fill_host(tombs, 2 * T, n - 2 * T)
        cols = {c: np.concatenate([a[c], z[c]]) for c, _ in COLS}
        u, _ = h.upload_batch(cols)
        assert h.batch_tile_planes(d, n).tolist() == h.batch_tile_planes(u, n).tolist() == [1] * 4 + [0]
        want = [_sizes({c: cols[c][t * T:(t + 1) * T] for c, _ in COLS}) for t in range(4)]
        assert want[2] == want[3] == NONE and want[0] != NONE
        assert _size_words(h, d, 4) == _size_words(h, u, 4) == want
        _scan(h, d, sp.n_partitions, cols, workgroups=(1, 3))
        _scan(h, u, sp.n_partitions, cols, workgroups=(1, 3))
        h.device_batch_free(u)
        h.device_batch_free(d)

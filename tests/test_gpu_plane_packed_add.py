"""The plane loop's packed add (csrc/kta_plane_pack.h): a plane record adds ONE 64-bit word — count (14 bits),
raw key sum (21) and raw value sum (29) — to its front slot, and its two flags go with a 32-bit add of their own, executed
only by the lanes that have one.  The fields hold what ONE slot takes in one plane interval — min(FT, 8 R) tiles for R
replicas, 8192 records at most — and the flush unpacks every replica before it sums.

A lane's four records are records 4 tid .. 4 tid + 3 of the tile and its replica is tid & (R - 1), so slot (p, r) takes
records from 256 / R lanes only.  Every scan compares finish() — counters[P, 7] and the four extrema — bit for bit with
the C oracle on the same columns (test_gpu_scan_lean._checked) under scan variants 0, 16, 48, 64 and 80, the five must
agree, and batch_tile_planes must say that every tile is marked.  Batches are 3 to 67 tiles."""
import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
from helpers import NOW
from test_gpu_plane_size_extrema import KEY_MAX, KEY_SUM, VAL_MAX, VAL_SUM, _cols, _plain, _scan
from test_gpu_scan_lean import FT
from test_gpu_scan_packed import T

pytestmark = pytest.mark.gpu

TOMBS, KNULL = N.KTA_C_TOMBSTONES, N.KTA_C_KEY_NULL


def _marked_scan(P, cols, workgroups=(1,)):
    """Upload, check that every tile is marked, scan under the five variants and every grid; -> counters[P, 7]."""
    n = len(cols["partition"])
    assert n % T == 0
    with kta.HipMetricHandler(P, now=NOW) as h:
        b, _ = h.upload_batch(cols)
        assert h.batch_tile_planes(b, n).tolist() == [1] * (n // T)
        c, _, _ = _scan(h, b, P, cols, workgroups=workgroups)
        h.device_batch_free(b)
    return c


def _one_partition(lengths):
    """FT + 1 = 33 whole tiles, every record in partition 7 with the same two lengths."""
    assert FT == 32
    n = (FT + 1) * T
    return _cols(np.full(n, 7), np.full(n, lengths[0]), np.full(n, lengths[1]))


LENGTHS = [(KEY_MAX, VAL_MAX), (-1, -1)]


# ---- one slot at the bound --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", LENGTHS)
def test_one_slot_at_the_bound(lengths):
    """A handler of 256 partitions has R = 4 replicas; every record lies in partition 7, so every lane adds a uniform quad
    and each of partition 7's four slots takes 64 lanes x 4 records x 32 tiles = 8192 records before the flush: the count
    field at 8192 of 2^14, and with (-1, -1) the raw sums at 8192 x 0xFF and 8192 x 0xFFFF, the bounds of their fields.
    The 33rd tile crosses the flush."""
    k, v = lengths
    cols = _one_partition(lengths)
    c = _marked_scan(256, cols)
    n = len(cols["partition"])
    assert int(c[7, KEY_SUM]) == n * max(k, 0) and int(c[7, VAL_SUM]) == n * max(v, 0)
    assert int(c[7, TOMBS]) == int(c[7, KNULL]) == (n if k < 0 else 0)
    assert not c[np.arange(256) != 7].any()


# ---- the per-record path at its most ----------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", LENGTHS)
def test_the_per_record_path_at_its_most(lengths):
    """The same, with every lane's fourth record in partition 8: no quad is uniform, every record is an add of its own (and
    with (-1, -1) a flag add of its own), and partition 7's slots take 64 x 3 x 32 = 6144 records per interval."""
    k, v = lengths
    cols = _one_partition(lengths)
    cols["partition"][3::4] = 8
    c = _marked_scan(256, cols)
    n = len(cols["partition"])
    assert int(c[7, KEY_SUM]) == 3 * n // 4 * max(k, 0) and int(c[8, VAL_SUM]) == n // 4 * max(v, 0)


# ---- short intervals --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", LENGTHS)
@pytest.mark.parametrize("P,R", [(400, 2), (600, 1)])
def test_short_intervals(P, R, lengths):
    """Handlers of 400 and 600 partitions over the one-partition data.  plan_scan gives the packed scan the largest power of
    two R <= 64 with 16 P R + 40 P <= 32 KiB (two replicated front words and five back words per partition): 16 x 400 x 2 +
    16 000 = 28 800 fits and 41 600 does not, so R = 2; 16 x 600 + 24 000 = 33 600 does not fit at all, so R = 1.  A slot
    then takes 512 or 1024 records per tile, and a plane interval must be 16 or 8 tiles: with 32 the count field of 14
    bits would carry into the key sum at 16 384 or 32 768 records."""
    assert R == max(r for r in (1, 2, 4, 8, 16, 32, 64) if r == 1 or 16 * P * r + 40 * P <= 32 * 1024)
    k, v = lengths
    cols = _one_partition(lengths)
    c = _marked_scan(P, cols)
    n = len(cols["partition"])
    assert int(c[7, KEY_SUM]) == n * max(k, 0) and int(c[7, VAL_SUM]) == n * max(v, 0)
    assert not c[np.arange(P) != 7].any()


# ---- flags ------------------------------------------------------------------------------------------------------------
def test_flags():
    """Three tiles, 8 partitions, no markers but these: every tile has exactly one null key, one tombstone and one record
    with both.  In tiles 0 and 2 they lie in three lanes, among records of other partitions (three lanes of a wave execute
    the flag add, or one); in tile 1 they are three of lane 50's four records, which all lie in partition 3: the uniform
    quad with a flag word of 2 | 2 << 16."""
    P, ntiles = 8, 3
    n = ntiles * T
    rng = np.random.default_rng(81)
    cols = _cols(rng.integers(0, P, n), rng.integers(10, 50, n), rng.integers(100, 1000, n))
    p, k, v = cols["partition"], cols["key_len"], cols["val_len"]
    for tile, (a, b, both) in ((0, (5, 261, 1023)), (2, (64 * 4, 64 * 4 + 7, 64 * 4 + 9))):
        s = tile * T
        k[s + a], v[s + b] = -1, -1
        k[s + both], v[s + both] = -1, -1
    q = T + 4 * 50
    p[q:q + 4] = 3
    k[q], v[q + 1] = -1, -1
    k[q + 2], v[q + 2] = -1, -1
    assert int((k == -1).sum()) == int((v == -1).sum()) == 2 * ntiles
    c = _marked_scan(P, cols, workgroups=(1, 3))
    assert int(c[:, KNULL].sum()) == int(c[:, TOMBS].sum()) == 2 * ntiles
    assert int(c[3, KNULL]) >= 2 and int(c[3, TOMBS]) >= 2


# ---- several intervals, two grids -------------------------------------------------------------------------------------
def test_several_intervals_two_grids():
    """2 FT + 3 tiles of mixed records over 256 partitions: one workgroup flushes twice inside the loop and once behind it,
    each of three workgroups meets no flush but the last."""
    _marked_scan(256, _plain((2 * FT + 3) * T, 256, seed=82), workgroups=(1, 3))

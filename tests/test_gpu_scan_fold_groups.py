"""The fold of the scan's partial rows in groups (kta_fold_partials, csrc/kta_fold.h, csrc/kta_fold_groups.h): a
workgroup of the fold takes the rows of one group, kFoldGroupRows of them and fewer in the last, and reads them
kFoldLoads at a time.

Every case compares finish() — the result and counters[P, 7] — bit for bit with the C oracle on the same records (one
oracle run per batch, shared by the variants), under scan variants 0 and 16 (non-temporal loads), and the two must agree.
Grids — the fold's rows — around the group's and the load block's edges, rows that the scan's second kernel merged
into and rows it left alone, submits without a reset between them at changing grids (a row beyond the grid is stale and
must not be read), and rows of 13 and of 10 008 words."""
import os
import re

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
from helpers import NOW
from oracle_c import Oracle
from test_gpu_scan_lean import NT_EXC, PATTERNS, _make_exceptional
from test_gpu_scan_packed import COLS, T, _topic

pytestmark = pytest.mark.gpu

VARIANTS = (0, 16)


def _define(header, name):
    src = open(os.path.join(os.path.dirname(N.__file__), "csrc", header)).read()
    return int(re.search(r"#define %s (\d+)" % name, src).group(1))


G = _define("kta_fold_groups.h", "KTA_FOLD_GROUP_ROWS")     # rows of a group
L = _define("kta_fold.h", "KTA_FOLD_LOADS")                 # rows a thread loads together


def _expected(P, batches):
    """What finish() must give after the handler of P partitions took every batch of `batches` (columns), one after
    another: the oracle is given the records the product counts, the others are the bad ones."""
    o = Oracle(NOW)
    bad = 0
    for cols in batches:
        p = cols["partition"]
        good = (p >= 0) & (p < P)
        bad += int((~good).sum())
        o.run_soa({k: np.ascontiguousarray(cols[k][good]) for k, _ in COLS})
    want = (o.counters(P).tobytes(), o.earliest(), o.latest(), o.get("smallest_message"), o.get("largest_message"),
            o.get("overall_count"), o.get("overall_size"), bad)
    o.close()
    return want


def _finished(h, P):
    res, c = h.finish(allow_bad_partition=True)
    assert c.shape == (P, 7)
    mm = kta.MessageMetrics(res, c, h.now)
    return (c.tobytes(), mm.earliest_message(), mm.latest_message(), mm.smallest_message(), mm.largest_message(),
            res.overall_count, res.overall_size, res.bad_partition_records)


def _view(b, lo):
    v = kta.KtaBatch()
    for f, sz in COLS:
        setattr(v, f, getattr(b, f) + lo * sz)
    return v


def _host(cols, lo=0, m=None):
    return {k: cols[k][lo:(len(cols[k]) if m is None else lo + m)] for k, _ in COLS}


def _four(h, P, submits, want):
    """submits: (batch, records, workgroups) in order, no reset between them; under each variant, against `want`."""
    for variant in VARIANTS:
        h.reset()
        for b, m, wgs in submits:
            h.set_tuning(scan_workgroups=wgs, scan_variant=variant)
            h.submit_device(b, m, 0, which=1)
        assert _finished(h, P) == want, "scan variant %d differs from the oracle" % variant


def _c4(P, seed=None):
    sp, _ = kta.synth_preset("c4")
    sp.n_partitions = P
    if seed is not None:
        sp.seed = seed
    return sp


def _planes(h, sp, n):
    """A device batch of n records that the device producer filled (plane tiles), and the same records on the host."""
    b = h.device_batch_alloc(n)
    h.synth_fill_device(sp, 0, n, b)
    return b, _host(kta.synth_fill_host(sp, 0, n))


# ---- the group's edges ------------------------------------------------------------------------------------------------
GRIDS = tuple(sorted({1, L - 1, L, L + 1, G - 1, G, G + 1, 2 * G + 1, 63}))


@pytest.mark.parametrize("tiles", ["six_byte", "plane"])
@pytest.mark.parametrize("P", [256, 5])
def test_group_edges(P, tiles):
    nmax = (3 * max(GRIDS) + 1) * T
    with kta.HipMetricHandler(P, now=NOW) as h:
        if tiles == "plane":
            b, cols = _planes(h, _c4(P), nmax)
            assert int(h.batch_tile_planes(b, nmax).sum()) == nmax // T
        else:
            cols = _topic(nmax, P, seed=71)
            b, _ = h.upload_batch(cols)
            assert b.layout == N.KTA_LAYOUT_TILE_COMPACT
        for grid in GRIDS:
            n = (3 * grid + 1) * T
            _four(h, P, [(b, n, grid)], _expected(P, [_host(cols, 0, n)]))
        h.device_batch_free(b)


# ---- the flagship's own grid ------------------------------------------------------------------------------------------
def test_the_plans_grid_over_config_4():
    n = (1 << 21) + 123
    sp = _c4(256)
    with kta.HipMetricHandler(256, now=NOW) as h:
        b, cols = _planes(h, sp, n)
        _four(h, 256, [(b, n, 0)], _expected(256, [cols]))
        h.device_batch_free(b)


# ---- groups of which some workgroups merged into their rows -----------------------------------------------------------
def test_cut_view_two_rows_merged():
    """Records 4 .. n - 37 at 17 workgroups: the cut first and last tile are the second kernel's, every other is lean."""
    P, grid = 256, 17
    n = (3 * grid + 1) * T
    with kta.HipMetricHandler(P, now=NOW) as h:
        b, cols = _planes(h, _c4(P), n)
        m = n - 4 - 37
        _four(h, P, [(_view(b, 4), m, grid)], _expected(P, [_host(cols, 4, m)]))
        h.device_batch_free(b)


@pytest.mark.parametrize("grid", [1, 3, G + 1])
def test_one_raw_tile_mid_batch(grid):
    P = 8
    cols = _topic(NT_EXC * T, P, seed=72)
    _make_exceptional("raw", cols, NT_EXC // 2, P)
    with kta.HipMetricHandler(P, now=NOW) as h:
        b, _ = h.upload_batch(cols)
        _four(h, P, [(b, NT_EXC * T, grid)], _expected(P, [cols]))
        h.device_batch_free(b)


@pytest.mark.parametrize("grid", [1, 3])
def test_alternating_tiles_are_handed_over(grid):
    P = 8
    cols = _topic(NT_EXC * T, P, seed=73)
    for tile in PATTERNS["alternating"]:
        _make_exceptional("i32", cols, tile, P)
    with kta.HipMetricHandler(P, now=NOW) as h:
        b, _ = h.upload_batch(cols)
        _four(h, P, [(b, NT_EXC * T, grid)], _expected(P, [cols]))
        h.device_batch_free(b)


# ---- submits without a reset --------------------------------------------------------------------------------------------
def test_every_row_merged_five_submits_without_reset():
    """A handler of 200 partitions over config 4's 256 at 64 workgroups: no tile's summary applies, every workgroup of the
    second kernel merges into its row.  Five submits of different records without a reset: the totals are the five
    oracles' sum."""
    P, grid = 200, 64
    n = (3 * grid + 1) * T
    with kta.HipMetricHandler(P, now=NOW) as h:
        made = [_planes(h, _c4(256, seed=81 + i), n) for i in range(5)]
        _four(h, P, [(b, n, grid) for b, _ in made], _expected(P, [cols for _, cols in made]))
        for b, _ in made:
            h.device_batch_free(b)


def test_any_sequence_of_grids_without_reset():
    P = 256
    n = (3 * 64 + 1) * T
    with kta.HipMetricHandler(P, now=NOW) as h:
        b, cols = _planes(h, _c4(P), n)
        _four(h, P, [(b, n, grid) for grid in (17, 9, 0, 7, 64)], _expected(P, [cols] * 5))
        _four(h, P, [(b, n, 0)], _expected(P, [cols]))          # (each variant behind a reset)
        h.device_batch_free(b)


# ---- the row's length -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2000])
def test_row_length(P):
    """P = 1: 13 words per row, most threads of the one column block have no column; P = 2000: 10 008 words, 40 blocks."""
    n = (3 * (G + 1) + 1) * T
    with kta.HipMetricHandler(P, now=NOW) as h:
        b, cols = _planes(h, _c4(P), n)
        for grid in (3, G + 1):
            _four(h, P, [(b, n, grid)], _expected(P, [cols]))
        h.device_batch_free(b)

"""The lean kernel of the summary-reading packed scan and the kernel behind it (kta_metrics_scan_packed<NT, true>,
kta_metrics_scan_packed_rest): summarised compact / u16 tiles go through a ring of 6-register slots with
the headers and summaries a step ahead in scalar registers; any other tile is listed in the workgroup's row (four at
most) or handed over with everything behind it, and accumulated by the second kernel's loop over whole Quads.

Every case compares finish() — the result and counters[P, 7] — bit for bit with the C oracle on the same columns, under
scan variants 0, 16 (non-temporal loads) and 48 (no summaries: the kernel of before), and the three must agree with one
another.  One to three workgroups walk many tiles, so the ring fills, drains, meets the front flush and the list's end."""
import os
import re

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
from helpers import NOW
from oracle_c import Oracle
from test_gpu_scan_packed import BASE_TS, COLS, F, T, _tile_hdrs, _topic

pytestmark = pytest.mark.gpu

VARIANTS = (0, 16, 48)
VALID, TIMED, UNTIMED = N.KTA_TILE_SUM_VALID, N.KTA_TILE_SUM_TIMED, N.KTA_TILE_SUM_UNTIMED
LEAN = (N.KTA_TILE_COMPACT, N.KTA_TILE_LENS_U16)
FT = F // T                       # tiles between two front flushes
LISTED = 4                        # kLeanListed: the tiles a workgroup's row can list


def test_the_list_length_is_the_kernels():
    src = open(os.path.join(os.path.dirname(N.__file__), "csrc", "kta_kernels.hip")).read()
    assert int(re.search(r"constexpr uint32_t kLeanListed = (\d+);", src).group(1)) == LISTED
    assert len(PATTERNS["alternating"]) > LISTED       # that pattern is handed over, the others are listed


def _checked(h, P, cols):
    """finish() against the oracle (given the records the product counts); -> what the variants must agree on."""
    p = cols["partition"]
    good = (p >= 0) & (p < P)
    o = Oracle(NOW)
    o.run_soa({k: np.ascontiguousarray(cols[k][good]) for k, _ in COLS})
    res, c = h.finish(allow_bad_partition=True)
    assert c.shape == (P, 7) and np.array_equal(c, o.counters(P)), "per-partition counters differ"
    mm = kta.MessageMetrics(res, c, h.now)
    assert mm.earliest_message() == o.earliest() and mm.latest_message() == o.latest()
    assert mm.smallest_message() == o.get("smallest_message") and mm.largest_message() == o.get("largest_message")
    assert res.overall_count == o.get("overall_count") and res.overall_size == o.get("overall_size")
    assert res.bad_partition_records == int((~good).sum())
    o.close()
    return (c.tobytes(), mm.earliest_message(), mm.latest_message(), mm.smallest_message(), mm.largest_message(),
            res.overall_count, res.overall_size, res.bad_partition_records)


def _three(P, cols, workgroups=(1,), views=(), expect_hdrs=None, lean_tiles=None):
    """The batch (or every (lo, m) of `views`: records [lo, lo + m), lo a multiple of 4) under the three variants and every
    grid of `workgroups`.  expect_hdrs: the tiles' (mode, lens); lean_tiles: per tile True — its summary is VALID and its
    largest partition counts: the lean loop takes it —, "part_max" — VALID, but the largest partition does not count —, or
    False: the header (raw, i32 lengths) or a view's cut says why it does not qualify."""
    n = len(cols["partition"])
    with kta.HipMetricHandler(P, now=NOW) as h:
        b, _ = h.upload_batch(cols)
        assert b.layout == N.KTA_LAYOUT_TILE_COMPACT
        if expect_hdrs is not None:
            assert _tile_hdrs(h, b, len(expect_hdrs)) == expect_hdrs
        if lean_tiles is not None:
            s = h.batch_tile_summaries(b, n)
            for t, lean in enumerate(lean_tiles):
                if lean is True:
                    assert int(s["flags"][t]) & VALID and int(s["part_max"][t]) < min(P, 0xFFFF), t
                elif lean == "part_max":                # a summarised compact tile kept out by its largest partition
                    assert int(s["flags"][t]) & VALID and int(s["part_max"][t]) >= min(P, 0xFFFF), t
        for wgs in workgroups:
            for lo, m in (views or ((0, n),)):
                got = []
                for variant in VARIANTS:
                    h.reset()
                    h.set_tuning(scan_workgroups=wgs, scan_variant=variant)
                    v = kta.KtaBatch()
                    for f, sz in COLS:
                        setattr(v, f, getattr(b, f) + lo * sz)
                    h.submit_device(b if lo == 0 else v, m, 0, which=1)
                    got.append(_checked(h, P, {k: cols[k][lo:lo + m] for k, _ in COLS}))
                assert got[0] == got[1] == got[2], "the scan variants disagree"
        h.device_batch_free(b)


# ---- the ring fills and drains ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [256, 5])
def test_ring_fill_and_drain(P):
    for ntiles in (1, 2, 3, 4, 5):                      # one workgroup
        _three(P, _topic(ntiles * T, P, seed=21), workgroups=(1,), expect_hdrs=[LEAN] * ntiles, lean_tiles=[True] * ntiles)
    for ntiles in (3 * 2 - 1, 3 * 2, 3 * 2 + 1):        # W k - 1, W k, W k + 1 tiles, W = 3 workgroups
        _three(P, _topic(ntiles * T, P, seed=22), workgroups=(3,), expect_hdrs=[LEAN] * ntiles, lean_tiles=[True] * ntiles)
    _three(P, _topic(3 * T, P, seed=23), workgroups=(8,), lean_tiles=[True] * 3)   # more workgroups than tiles


# ---- exceptional tiles at every position of the ring and of the front interval ---------------------------------------
NT_EXC = 2 * FT + 3
PATTERNS = {
    "at_0": [0], "at_1": [1], "at_2": [2], "before_flush": [FT - 1], "at_flush": [FT], "after_flush": [FT + 1],
    "last_but_one": [NT_EXC - 2], "last": [NT_EXC - 1], "adjacent": [5, 6],
    "alternating": list(range(1, NT_EXC, 2)),           # more than the row lists: the rest is handed over
}


def _make_exceptional(kind, cols, tile, P):
    """Turn one tile into the kind; -> its expected header."""
    p, t, k = cols["partition"], cols["ts_ms"], cols["key_len"]
    s = tile * T
    if kind == "raw":                                   # a timestamp span of 2^31
        t[s + 1], t[s + 5] = BASE_TS, BASE_TS + (1 << 31)
        return (N.KTA_TILE_RAW, N.KTA_TILE_LENS_U16)
    if kind == "i32":                                   # a length that does not fit u16
        k[s + 9] = 70000
        return (N.KTA_TILE_COMPACT, N.KTA_TILE_LENS_I32)
    if kind == "part_none":                             # a partition of -1: part_max is the marker
        p[s + 7] = -1
        return LEAN
    assert kind == "part_P"                             # a partition of P: counted in bad_partition_records
    p[s + 7] = P
    return LEAN


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("kind", ["raw", "i32", "part_none", "part_P"])
def test_exceptional_tiles(kind, pattern):
    P = 8
    cols = _topic(NT_EXC * T, P, seed=31)
    hdrs, lean = [LEAN] * NT_EXC, [True] * NT_EXC
    for tile in PATTERNS[pattern]:
        hdrs[tile] = _make_exceptional(kind, cols, tile, P)
        lean[tile] = "part_max" if kind in ("part_none", "part_P") else False
    _three(P, cols, workgroups=(1,), expect_hdrs=hdrs, lean_tiles=lean)


def test_views_cut_the_first_and_the_last_tile():
    P = 8
    cols = _topic(NT_EXC * T, P, seed=32)
    n = NT_EXC * T
    # a view that starts 4 records into a tile, one that ends 37 records into a tile, both
    _three(P, cols, workgroups=(1, 2), views=((4, n - 4), (0, n - T + 37), (T + 4, n - 2 * T - 4 + 37)),
           expect_hdrs=[LEAN] * NT_EXC, lean_tiles=[True] * NT_EXC)


def test_partial_last_tile_of_an_upload():
    P = 8
    ntiles = 2 * FT + 1
    n = ntiles * T + 37
    hdrs = [LEAN] * (ntiles + 1)
    with kta.HipMetricHandler(P, now=NOW) as h:         # (the partial tile has no summary)
        b, _ = h.upload_batch(_topic(n, P, seed=33))
        assert int(h.batch_tile_summaries(b, n)["flags"][ntiles]) == 0
        h.device_batch_free(b)
    _three(P, _topic(n, P, seed=33), workgroups=(1, 3), expect_hdrs=hdrs, lean_tiles=[True] * ntiles + [False])


# ---- summaries that stay lean but change the extrema ------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("what", ["untimed", "one_missing"])
def test_lean_summaries_that_change_the_extrema(what, where):
    P, ntiles = 8, 6
    cols = _topic(ntiles * T, P, seed=41)
    tile = 0 if where == "first" else ntiles - 1
    s = slice(tile * T, (tile + 1) * T)
    if what == "untimed":
        cols["ts_ms"][s] = -1                            # UNTIMED, not TIMED
        want = VALID | UNTIMED
    else:
        cols["ts_ms"][s] = BASE_TS + np.arange(T)
        cols["ts_ms"][tile * T + 500] = -1               # one -1 among timed records
        want = VALID | TIMED | UNTIMED
    with kta.HipMetricHandler(P, now=NOW) as h:
        b, _ = h.upload_batch(cols)
        assert int(h.batch_tile_summaries(b, ntiles * T)["flags"][tile]) == want
        h.device_batch_free(b)
    _three(P, cols, workgroups=(1, 3), expect_hdrs=[LEAN] * ntiles, lean_tiles=[True] * ntiles)


# ---- no tile qualifies ------------------------------------------------------------------------------------------------
def test_no_tile_qualifies():
    """A handler of 200 partitions over data with 256: every tile's part_max >= P, every record of 200..255 is bad."""
    ntiles = 40
    cols = _topic(ntiles * T, 256, seed=51)
    assert all(cols["partition"][t * T:(t + 1) * T].max() >= 200 for t in range(ntiles))
    _three(200, cols, workgroups=(3,), expect_hdrs=[LEAN] * ntiles, lean_tiles=["part_max"] * ntiles)


@pytest.mark.parametrize("P", [3, 256])
def test_every_tile_handed_over_across_a_front_flush(P):
    """One workgroup, one tile more than a front interval, two partitions more in the data than the handler has: the
    second kernel's ring starts at the first tile and meets its own front flush (variant 48: the kernel without
    summaries does); then the same through a view that cuts the first and the last tile."""
    ntiles = FT + 1
    n = ntiles * T
    cols = _topic(n, P + 2, seed=52)
    assert all(cols["partition"][t * T:(t + 1) * T].max() >= P for t in range(ntiles))
    _three(P, cols, workgroups=(1,), expect_hdrs=[LEAN] * ntiles, lean_tiles=["part_max"] * ntiles)
    _three(P, cols, workgroups=(1,), views=((4, n - 4 - T + 37),))


# ---- fields at their limits, one slot ---------------------------------------------------------------------------------
# plan_scan replicates a partition's front slots 2^r times while 16 P 2^r + 40 P bytes fit 32 KiB: a single replica
# (r = 0) from the least P with 16 * 2 P + 40 P > 32768 on.
P_ONE_REPLICA = 32768 // (16 * 2 + 40) + 1
assert 16 * 2 * P_ONE_REPLICA + 40 * P_ONE_REPLICA > 32 * 1024 >= 16 * 2 * (P_ONE_REPLICA - 1) + 40 * (P_ONE_REPLICA - 1)


@pytest.mark.parametrize("fill", ["longest", "tombstone_null_key", "alternating"])
def test_field_limits_in_one_slot(fill):
    n = 2 * F + T + 37
    # (alternating by quad: a lane's four records are alike, and with one partition every quad is uniform)
    full = (np.arange(n) // 4) % 2 == 0 if fill == "alternating" else np.full(n, fill == "longest")
    cols = {"partition": np.full(n, 77, np.int32),
            "key_len": np.where(full, 65534, -1).astype(np.int32),
            "val_len": np.where(full, 65534, -1).astype(np.int32),
            "ts_ms": (BASE_TS + np.arange(n)).astype(np.int64)}
    ntiles = (n + T - 1) // T
    _three(P_ONE_REPLICA, cols, workgroups=(1,), expect_hdrs=[LEAN] * ntiles, lean_tiles=[True] * (ntiles - 1) + [False])


# ---- runs and odd P ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["random", "runs"])
@pytest.mark.parametrize("P", [1, 5, 256, 300])
def test_runs_and_odd_p(P, order):
    ntiles = 70
    _three(P, _topic(ntiles * T, P, seed=61, runs=(order == "runs")), workgroups=(0,), lean_tiles=[True] * ntiles)

"""The packed metrics scan of tile-compact batches (kta_metrics_scan_packed): two 64-bit LDS atomics per
record into packed front words, a full-width back level in LDS, one row write at the end.  Every case compares
finish() — the result and counters[P, 7] — bit for bit with the C oracle on the same columns, with temporal and
non-temporal loads (scan variants 0 and 16).  Batches are uploaded keyless, so their tiles are u16 where the values allow."""
import os
import re

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
from helpers import NOW
from oracle_c import Oracle

pytestmark = pytest.mark.gpu

T = 1024                 # KTA_TILE_RECORDS
BASE_TS = 1_600_000_000_000
COLS = (("partition", 4), ("key_len", 4), ("val_len", 4), ("ts_ms", 8))


def _front_records():
    """F: the records a workgroup accumulates between two front flushes, from the kernel's own constant."""
    src = open(os.path.join(os.path.dirname(N.__file__), "csrc", "kta_kernels.hip")).read()
    return int(re.search(r"constexpr uint32_t kFrontFlushTiles = (\d+);", src).group(1)) * T


F = _front_records()


def _topic(n, P, seed=3, runs=False):
    sp, _ = kta.synth_preset("c2")
    sp.seed, sp.n_partitions = seed, P
    if runs:
        sp.part_mode, sp.part_run_len = N.KTA_PART_RUNS, 500
    else:
        sp.part_mode = N.KTA_PART_RANDOM
    c = kta.synth_fill_host(sp, 0, n)
    return {k: c[k] for k, _ in COLS}


def _tile_hdrs(h, b, ntiles):
    """(mode, lens) of the batch's first ntiles tiles."""
    raw = np.empty(2 * ntiles, np.uint64)
    h._check(N.load().kta_copy_to_host(h._ctx, raw.ctypes.data, b.tile_hdr, raw.nbytes))
    return [(int(x) & 0xFFFFFFFF, int(x) >> 32) for x in raw[1::2]]


def _assert_matches_oracle(h, P, cols):
    """(The oracle keeps a map of whatever partition ids it meets; the product counts a record whose id is outside
    [0, P) in bad_partition_records and in nothing else: the oracle is given the records the product counts.)"""
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


def _scan(P, cols, scan_variant, scan_workgroups=0, views=(), expect_hdrs=None):
    """The whole batch, then every (lo, m) of `views` (records [lo, lo + m), lo a multiple of 4), against the oracle."""
    n = len(cols["partition"])
    with kta.HipMetricHandler(P, now=NOW) as h:
        h.set_tuning(scan_workgroups=scan_workgroups, scan_variant=scan_variant)
        b, _ = h.upload_batch(cols)
        assert b.layout == N.KTA_LAYOUT_TILE_COMPACT
        if expect_hdrs is not None:
            assert _tile_hdrs(h, b, len(expect_hdrs)) == expect_hdrs
        h.submit_device(b, n, 0, which=1)
        _assert_matches_oracle(h, P, cols)
        for lo, m in views:
            h.reset()
            v = kta.KtaBatch()
            for f, sz in COLS:
                setattr(v, f, getattr(b, f) + lo * sz)
            h.submit_device(v, m, 0, which=1)
            _assert_matches_oracle(h, P, {k: cols[k][lo:lo + m] for k, _ in COLS})
        h.device_batch_free(b)


# ---- fields at their limits, one slot ---------------------------------------------------------------------------------
# The plan replicates a partition's front slots 2^r times while 16 P 2^r + 40 P bytes fit 32 KiB: r = 0 from
# 16 * 2 P + 40 P > 32768, P >= 456.  One workgroup and one partition: every record of a front interval lands in ONE slot.
P_ONE_REPLICA = 512
assert 16 * 2 * P_ONE_REPLICA + 40 * P_ONE_REPLICA > 32 * 1024


@pytest.mark.parametrize("scan_variant", [0, 16])
@pytest.mark.parametrize("fill", ["longest", "tombstone_null_key", "alternating"])
def test_fields_at_their_limits_one_slot(fill, scan_variant):
    n = 2 * F + T + 37
    full = np.arange(n) % 2 == 0 if fill == "alternating" else np.full(n, fill == "longest")
    cols = {"partition": np.full(n, 77, np.int32),
            "key_len": np.where(full, 65534, -1).astype(np.int32),
            "val_len": np.where(full, 65534, -1).astype(np.int32),
            "ts_ms": (BASE_TS + np.arange(n)).astype(np.int64)}
    hdrs = [(N.KTA_TILE_COMPACT, N.KTA_TILE_LENS_U16)] * ((n + T - 1) // T)
    _scan(P_ONE_REPLICA, cols, scan_variant, scan_workgroups=1, expect_hdrs=hdrs)


# ---- the flush boundary with mixed tiles ------------------------------------------------------------------------------
def _mixed_tiles(n, P):
    """Tile kinds shuffled by tile; the i32 kinds on both sides of the first front flush.  -> columns, expected headers."""
    cols = _topic(n, P, seed=11)
    p, t, k, v = cols["partition"], cols["ts_ms"], cols["key_len"], cols["val_len"]
    u16, i32 = N.KTA_TILE_LENS_U16, N.KTA_TILE_LENS_I32
    cmp_, raw = N.KTA_TILE_COMPACT, N.KTA_TILE_RAW
    kinds = [
        (lambda s: None, (cmp_, u16)),
        (lambda s: k.__setitem__(s.start + 9, 70000), (cmp_, i32)),
        (lambda s: v.__setitem__(s.start + 2, -2), (cmp_, i32)),
        (lambda s: (t.__setitem__(s.start + 1, BASE_TS), t.__setitem__(s.start + 5, BASE_TS + (1 << 31))), (raw, u16)),
        (lambda s: p.__setitem__(s.start + 7, 65535), (raw, u16)),
        (lambda s: (p.__setitem__(slice(s.start, s.start + 40, 3), P + 3), p.__setitem__(slice(s.start + 1, s.start + 40, 3), -1)),
         (cmp_, u16)),
    ]
    ntiles = (n + T - 1) // T
    flush_tile = F // T
    order = np.random.default_rng(5).permutation(np.arange(ntiles) % len(kinds))
    order[flush_tile - 2:flush_tile + 2] = [1, 2, 2, 1]          # i32 tiles right before and right after the flush
    order[flush_tile + 2] = 3
    hdrs = []
    for tile in range(ntiles):
        s = slice(tile * T, min(n, (tile + 1) * T))
        c = int(order[tile]) if s.stop - s.start >= 64 else 0
        kinds[c][0](s)
        hdrs.append(kinds[c][1])
    assert {1, 2} <= set(order[:flush_tile]) and {1, 2} <= set(order[flush_tile:])
    return cols, hdrs


@pytest.mark.parametrize("scan_variant", [0, 16])
@pytest.mark.parametrize("P", [8, 300])
def test_flush_boundary_with_mixed_tiles(P, scan_variant):
    n = F + 3 * T + 5
    cols, hdrs = _mixed_tiles(n, P)
    _scan(P, cols, scan_variant, scan_workgroups=1, expect_hdrs=hdrs)


# ---- both accumulate paths --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan_variant", [0, 16])
@pytest.mark.parametrize("order", ["interleaved", "runs"])
@pytest.mark.parametrize("P", [1, 8, 256])
def test_interleaved_and_runs(P, order, scan_variant):
    n = 5 * T + 3
    cols = _topic(n, P, seed=7, runs=(order == "runs"))
    for wgs in (1, 2, 0):
        # (the last view starts and ends inside a tile)
        _scan(P, cols, scan_variant, scan_workgroups=wgs, views=((T + 500, 2 * T + 301),) if wgs == 2 else ())


# ---- a P whose plan needs more than 48 KiB of LDS (the opt-in) --------------------------------------------------------
@pytest.mark.parametrize("scan_variant", [0, 16])
def test_more_than_48_kib_of_lds(scan_variant):
    P = 1000
    assert 16 * P + 40 * P > 48 * 1024
    _scan(P, _topic(4 * T, P, seed=9), scan_variant)


# ---- timestamps: the tile-local extrema -------------------------------------------------------------------------------
def _ts_tiles():
    """Four tiles: compact, all timestamps missing but one; compact, the whole span ts_base .. ts_base + 2^31 - 1; raw with a
    negative timestamp; raw with a timestamp above 2^40."""
    base = _topic(T, 8, seed=13)
    tiles = []
    t = np.full(T, -1, np.int64)
    t[613] = BASE_TS + 12345
    tiles.append((t, N.KTA_TILE_COMPACT))
    t = np.full(T, BASE_TS + 1000, np.int64)
    t[17], t[900] = BASE_TS, BASE_TS + (1 << 31) - 1
    tiles.append((t, N.KTA_TILE_COMPACT))
    t = (BASE_TS + np.arange(T)).astype(np.int64)
    t[5] = -77_000
    tiles.append((t, N.KTA_TILE_RAW))
    t = np.full(T, 1 << 41, np.int64)
    t[3] = (1 << 41) + (1 << 33)
    tiles.append((t, N.KTA_TILE_RAW))
    return base, tiles


@pytest.mark.parametrize("scan_variant", [0, 16])
def test_timestamp_extrema_per_tile_kind(scan_variant):
    base, tiles = _ts_tiles()
    for t, mode in tiles:                         # each tile alone: its extrema are the result's
        cols = dict(base, ts_ms=t)
        _scan(8, cols, scan_variant, expect_hdrs=[(mode, N.KTA_TILE_LENS_U16)])
    cols = {k: np.concatenate([base[k]] * len(tiles)) for k in ("partition", "key_len", "val_len")}
    cols["ts_ms"] = np.concatenate([t for t, _ in tiles])
    _scan(8, cols, scan_variant, expect_hdrs=[(m, N.KTA_TILE_LENS_U16) for _, m in tiles])

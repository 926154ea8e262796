"""Tile summaries (kta_tile_sum, include/kta_hip.h): the packed metrics scan takes the earliest and the
latest timestamp of a summarised tile from the summary its producer wrote and does not load the tile's timestamps.  Every
case compares finish() — the result and counters[P, 7] — bit for bit with the C oracle on the same records, with scan
variants 0, 16, 32 and 48 (temporal / non-temporal loads, with and without summaries), and the four results must be equal.
Batches are uploaded keyless, so their tiles are u16 where the values allow."""
import ctypes as C
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
EARLY, LATE = BASE_TS - 1_000_000, BASE_TS + 1_000_000_000     # beyond every other timestamp of a topic here
COLS = (("partition", 4), ("key_len", 4), ("val_len", 4), ("ts_ms", 8))
VARIANTS = (0, 16, 32, 48)
VALID, TIMED, UNTIMED = N.KTA_TILE_SUM_VALID, N.KTA_TILE_SUM_TIMED, N.KTA_TILE_SUM_UNTIMED
N_ODD = 4 * T + 37       # four whole tiles and an odd tail


def _front_records():
    """F: the records a workgroup accumulates between two front flushes, from the kernel's own constant."""
    src = open(os.path.join(os.path.dirname(N.__file__), "csrc", "kta_kernels.hip")).read()
    return int(re.search(r"constexpr uint32_t kFrontFlushTiles = (\d+);", src).group(1)) * T


F = _front_records()


def _topic(n, P, seed=3):
    """Random partitions in [0, P), mixed lengths, timestamps BASE_TS + 10000 + i: ordinary ones strictly inside (EARLY, LATE)."""
    sp, _ = kta.synth_preset("c2")
    sp.seed, sp.n_partitions, sp.part_mode = seed, P, N.KTA_PART_RANDOM
    c = kta.synth_fill_host(sp, 0, n)
    cols = {k: c[k].copy() for k, _ in COLS}
    cols["ts_ms"] = (BASE_TS + 10_000 + np.arange(n)).astype(np.int64)
    return cols


def _cut(cols, lo, m):
    return {k: cols[k][lo:lo + m] for k, _ in COLS}


def _view(b, lo):
    v = kta.KtaBatch()
    for f, sz in COLS:
        setattr(v, f, getattr(b, f) + lo * sz)
    return v


def _checked(h, P, cols):
    """finish() against the oracle on the records the product counts (partition in [0, P)); -> the result, to compare runs."""
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
    return tuple(getattr(res, f) for f, _ in N.KtaResult._fields_), c.tobytes()


def _four(P, scenario, scan_workgroups=0, **handler):
    """scenario(h) -> anything comparable, under each of the four scan variants; the four must agree."""
    got = []
    for sv in VARIANTS:
        with kta.HipMetricHandler(P, now=NOW, **handler) as h:
            h.set_tuning(scan_workgroups=scan_workgroups, scan_variant=sv)
            got.append(scenario(h))
    assert all(g == got[0] for g in got[1:]), "the scan variants disagree"


def _upload_into(h, b, cols):
    """kta_batch_from_raw into an existing device batch (upload_batch allocates a new one)."""
    metric = {k: np.ascontiguousarray(cols[k]) for k, _ in COLS}
    h._check(h._lib.kta_batch_from_raw(h._ctx, C.byref(kta._host_batch(metric)), len(metric["partition"]), C.byref(b)))


def _flags(h, b, n):
    return [int(x) for x in h.batch_tile_summaries(b, n)["flags"]]


def _whole_and_views(P, cols, views=(), scan_workgroups=0, want_flags=None):
    """The whole batch, then every (lo, m) of `views`, against the oracle."""
    n = len(cols["partition"])

    def scenario(h):
        b, _ = h.upload_batch(cols)
        if want_flags is not None:
            assert _flags(h, b, n) == want_flags
        h.submit_device(b, n, 0, which=1)
        out = [_checked(h, P, cols)]
        for lo, m in views:
            h.reset()
            h.submit_device(_view(b, lo), m, 0, which=1)
            out.append(_checked(h, P, _cut(cols, lo, m)))
        h.device_batch_free(b)
        return out
    _four(P, scenario, scan_workgroups=scan_workgroups)


# ---- 1. extrema that live only in summarised tiles ---------------------------------------------------------------------
@pytest.mark.parametrize("scan_workgroups", [1, 0])
def test_extrema_in_different_full_tiles(scan_workgroups):
    cols = _topic(N_ODD, 8)
    cols["ts_ms"][T + 5], cols["ts_ms"][3 * T + 77] = EARLY, LATE
    _whole_and_views(8, cols, scan_workgroups=scan_workgroups, want_flags=[VALID | TIMED] * 4 + [0])


def test_summarised_tiles_across_a_front_flush():
    n = F + 2 * T + 37
    cols = _topic(n, 8, seed=5)
    cols["ts_ms"][F - T + 9], cols["ts_ms"][F + T + 1000] = EARLY, LATE      # the tile before the flush, the second after it
    _whole_and_views(8, cols, scan_workgroups=1, want_flags=[VALID | TIMED] * (n // T) + [0])


# ---- 2. extremes on records that must not count ------------------------------------------------------------------------
def test_extremes_on_records_that_do_not_count():
    P = 8
    cols = _topic(N_ODD, P, seed=7)
    cols["partition"][T + 10], cols["ts_ms"][T + 10] = P + 3, EARLY
    cols["partition"][T + 20], cols["ts_ms"][T + 20] = -1, LATE
    n = N_ODD

    def bad_tile(h):     # the tile's largest stored partition is the -1 marker: read the old way, the extremes ignored
        b, _ = h.upload_batch(cols)
        s = h.batch_tile_summaries(b, n)
        assert int(s["part_max"][1]) == N.KTA_COMPACT_PART_NONE and int(s["flags"][1]) == VALID | TIMED
        h.submit_device(b, n, 0, which=1)
        return _checked(h, P, cols)
    _four(P, bad_tile)

    cols["partition"][T + 20] = P + 3

    def out_of_range(h):   # part_max = P + 3 >= P: still the old way
        b, _ = h.upload_batch(cols)
        assert int(h.batch_tile_summaries(b, n)["part_max"][1]) == P + 3
        h.submit_device(b, n, 0, which=1)
        return _checked(h, P, cols)
    _four(P, out_of_range)
    _four(P + 4, lambda h: (h.submit_device(h.upload_batch(cols)[0], n, 0, which=1), _checked(h, P + 4, cols))[1])   # the summary applies


# ---- 3. timestamps of -1 -----------------------------------------------------------------------------------------------
def test_missing_timestamps_in_summarised_tiles():
    cols = _topic(N_ODD, 8, seed=9)
    cols["ts_ms"][T + 3:2 * T:7] = -1
    cols["ts_ms"][2 * T:3 * T] = -1
    _whole_and_views(8, cols, want_flags=[VALID | TIMED, VALID | TIMED | UNTIMED, VALID | UNTIMED, VALID | TIMED, 0])
    # only tile 2 is untimed and alone in the view: earliest and latest are both 0
    _whole_and_views(8, cols, views=((2 * T, T),))


def test_the_only_timed_tile_is_cut_by_the_view():
    cols = _topic(N_ODD, 8, seed=11)
    t = cols["ts_ms"].copy()
    cols["ts_ms"][:] = -1
    cols["ts_ms"][2 * T:3 * T] = t[2 * T:3 * T]
    cols["ts_ms"][2 * T + 50], cols["ts_ms"][2 * T + 60] = EARLY, LATE       # in the part the view cuts off
    _whole_and_views(8, cols, views=((2 * T + 100, T),), want_flags=[VALID | UNTIMED] * 2 + [VALID | TIMED, VALID | UNTIMED, 0])


# ---- 4. views ----------------------------------------------------------------------------------------------------------
def test_views():
    n = 6 * T + 37
    cols = _topic(n, 8, seed=13)
    ts = cols["ts_ms"]
    ts[T + 100], ts[4 * T + 900] = EARLY, LATE                               # cut off by the first view
    ts[T + 600], ts[4 * T + 100] = EARLY + 5, LATE - 5                       # inside its cut first and last tile
    ts[2 * T + 1], ts[3 * T + 1] = EARLY + 9, LATE - 9                       # in its whole tiles
    _whole_and_views(8, cols, views=((T + 500, 3 * T + 300),     # starts and ends inside a tile
                                     (2 * T, 3 * T),             # whole tiles from a tile boundary: rec0 != 0 with summaries in use
                                     (2 * T, 2 * T),             # (the extremes of the tiles behind it must not count)
                                     (3 * T, T)),                # exactly one full tile
                     want_flags=[VALID | TIMED] * 6 + [0])
    _whole_and_views(8, cols, views=((T + 500, 3 * T + 300), (2 * T, 3 * T)), scan_workgroups=1)


# ---- 5. rewrites -------------------------------------------------------------------------------------------------------
def test_upload_over_an_upload():
    P = 8
    a = _topic(4 * T, P, seed=15)                     # A's last tile is full and holds A's extremes
    a["ts_ms"][3 * T + 40], a["ts_ms"][3 * T + 50] = EARLY, LATE
    b_cols = _topic(3 * T + 37, P, seed=17)           # B's last tile is partial, over A's full one
    b_cols["ts_ms"][5], b_cols["ts_ms"][3 * T + 2] = EARLY + 77, LATE - 77

    def scenario(h):
        b, _ = h.upload_batch(a)
        assert _flags(h, b, 4 * T) == [VALID | TIMED] * 4
        h.submit_device(b, 4 * T, 0, which=1)
        out = [_checked(h, P, a)]
        _upload_into(h, b, b_cols)
        assert _flags(h, b, 3 * T + 37) == [VALID | TIMED] * 3 + [0]
        h.reset()
        h.submit_device(b, 3 * T + 37, 0, which=1)
        out.append(_checked(h, P, b_cols))
        return out
    _four(P, scenario)


def test_synth_fill_over_an_upload_and_back():
    P = 8
    a = _topic(N_ODD, P, seed=19)
    a["ts_ms"][2 * T + 40], a["ts_ms"][3 * T + 50] = EARLY, LATE
    sp, _ = kta.synth_preset("c2")
    sp.n_partitions = P
    n2, n3 = 3 * T + 5, 2 * T + 9
    synth = {k: v for k, v in kta.synth_fill_host(sp, 0, n2).items() if k in dict(COLS)}
    c = _topic(n3, P, seed=21)
    c["ts_ms"][7], c["ts_ms"][2 * T + 3] = EARLY + 1, LATE - 1

    def scenario(h):
        b, _ = h.upload_batch(a)
        h.submit_device(b, N_ODD, 0, which=1)
        out = [_checked(h, P, a)]
        h.synth_fill_device(sp, 0, n2, b)             # the device producer over the uploaded batch
        f = _flags(h, b, n2)
        assert all(x & VALID for x in f[:3]) and f[3] == 0
        h.reset()
        h.submit_device(b, n2, 0, which=1)
        out.append(_checked(h, P, synth))
        _upload_into(h, b, c)                         # and the host producer over the device producer's
        assert _flags(h, b, n3) == [VALID | TIMED] * 2 + [0]
        h.reset()
        h.submit_device(b, n3, 0, which=1)
        out.append(_checked(h, P, c))
        return out
    _four(P, scenario)


def test_lengths_widened_for_a_key_reading_pass_keep_the_summary():
    """A -c handler is handed a view of a keyless batch with key columns of its own: the lengths of the view's tiles are
    widened (i32), partitions and timestamps stay compact and the summaries valid; then the metrics handler scans."""
    P, n = 8, N_ODD
    sp, _ = kta.synth_preset("c2")
    sp.n_partitions, sp.part_mode = P, N.KTA_PART_RANDOM
    cols = kta.synth_fill_host(sp, 0, n, with_keys=True)
    cols = {k: np.array(v) for k, v in cols.items()}
    cols["ts_ms"] = (BASE_TS + 10_000 + np.arange(n)).astype(np.int64)
    cols["ts_ms"][T + 5], cols["ts_ms"][2 * T + 77] = EARLY, LATE
    metric = {k: cols[k] for k, _ in COLS}

    def scenario(h):
        b, _ = h.upload_batch(metric)
        before = h.batch_tile_summaries(b, n).tobytes()
        keyed, _ = h.upload_batch(cols, with_keys=True)
        v = _view(b, 0)
        v.key_off, v.key_bytes = keyed.key_off, keyed.key_bytes
        h.submit_device(v, n, 0, which=2)             # the alive-key pass: widens the lengths first
        raw = np.empty(2 * 5, np.uint64)
        h._check(h._lib.kta_copy_to_host(h._ctx, raw.ctypes.data, b.tile_hdr, raw.nbytes))
        assert [(int(x) & 0xFFFFFFFF, int(x) >> 32) for x in raw[1::2]] == [(N.KTA_TILE_COMPACT, N.KTA_TILE_LENS_I32)] * 5
        assert h.batch_tile_summaries(b, n).tobytes() == before
        h.submit_device(b, n, 0, which=1)
        return _checked(h, P, metric)
    _four(P, scenario, count_alive_keys=True)


# ---- 6. producers agree ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", ["c2", "c4"])
def test_device_and_host_producer_write_the_same_summaries(preset):
    sp, _ = kta.synth_preset(preset)
    n = N_ODD
    with kta.HipMetricHandler(sp.n_partitions, now=NOW) as h:
        d = h.device_batch_alloc(n)
        h.synth_fill_device(sp, 0, n, d)
        dev = h.batch_tile_summaries(d, n)
        host_cols = kta.synth_fill_host(sp, 0, n)
        u, _ = h.upload_batch({k: host_cols[k] for k, _ in COLS})
        up = h.batch_tile_summaries(u, n)
        assert dev.tobytes() == up.tobytes()
        assert all(int(x) & VALID for x in dev["flags"][:4]) and dev[4].tobytes() == bytes(8)
        # (the restatement: a whole tile's span and largest partition)
        t, p = host_cols["ts_ms"][:T], host_cols["partition"][:T]
        assert int(dev["ts_span"][0]) == int(t[t != -1].max() - t[t != -1].min()) and int(dev["part_max"][0]) == int(p.max())
        # a view reads its own tiles' summaries, and only from a tile boundary
        assert h.batch_tile_summaries(_view(d, 2 * T), 2 * T).tobytes() == dev[2:4].tobytes()
        with pytest.raises(kta.KtaError) as e:
            h.batch_tile_summaries(_view(d, 2 * T + 4), T)
        assert e.value.code == N.KTA_ERR_INVALID


# ---- 7. no summaries ---------------------------------------------------------------------------------------------------
def test_a_hand_built_batch_with_its_own_headers_has_no_summaries():
    """The columns and headers of another context's allocation, handed over as a tile-compact kta_batch: the scanning
    context knows no summaries for it (kta_batch_tile_summaries refuses it) and reads every timestamp."""
    P = 8
    cols = _topic(N_ODD, P, seed=23)
    cols["ts_ms"][T + 5], cols["ts_ms"][3 * T + 77] = EARLY, LATE
    with kta.HipMetricHandler(P, now=NOW) as owner:
        b, _ = owner.upload_batch(cols)
        owner.sync()

        def scenario(h):
            own = kta.KtaBatch()
            for f, _ in COLS:
                setattr(own, f, getattr(b, f))
            own.capacity, own.tile_hdr, own.layout = b.capacity, b.tile_hdr, N.KTA_LAYOUT_TILE_COMPACT
            with pytest.raises(kta.KtaError) as e:
                h.batch_tile_summaries(own, N_ODD)
            assert e.value.code == N.KTA_ERR_INVALID
            h.submit_device(own, N_ODD, 0, which=1)
            return _checked(h, P, cols)
        _four(P, scenario)


def test_more_partitions_than_the_packed_scan_takes():
    P = 3000                                         # above 2925: kta_metrics_scan, which reads every timestamp
    cols = _topic(N_ODD, P, seed=25)
    cols["ts_ms"][T + 5], cols["ts_ms"][3 * T + 77] = EARLY, LATE
    _whole_and_views(P, cols, views=((2 * T, 2 * T),), want_flags=[VALID | TIMED] * 4 + [0])

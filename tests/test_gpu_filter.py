"""GPU tests of the record filter (kta_set_filter: a time window and a set of partitions in front of every pass).  The
contract: a filtered context is left in exactly the state of an UNFILTERED context that was handed only the passing records,
as ONE batch, in the same order and with the same sequence numbers.  Which records pass comes from the numpy restatement
(tests/filter_py.py), never from the code under test.

    base shape      3 * 1024 + 517 records, P = 5: tile 0 wholly before the window, tile 1 wholly inside, tile 2 straddling
                    its end, the partial tile mixed with timestamps of -1; ~40 distinct keys with tombstones; bad partitions
    paths           the staging ring, a tile-compact device batch, a view at record 300 of a larger allocation,
                    kta_handle_message; window only, set only, both; bit set state with every opt-in at once, the fused
                    pass, the table state with and without a caller's seq column
    slices          kta_set_filter_slice(1024) and (2048): identical results, the expected slice counts
    summaries       kta_filter_info's tiles decided by summary are the restatement's; none on the staging path
    edges           nothing passes, everything passes, chrono range in and out of the window, bad partitions under a set,
                    kta_set_filter after a record, kta_reset keeps the filter, refused arguments
    the Kafka decode, two ranks on the RCCL test double, kta-analyzer"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import filter_py as F
from helpers import NOW, random_cols

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
TILE = 1024
P = 5
N_REC = 3 * TILE + 517
T0 = 1_600_000_000_000
FROM, TO = T0 + 10_000, T0 + 20_000
KINDS = {"time": (FROM, TO, None), "set": (None, None, [1, 3]), "both": (FROM, TO, [0, 1, 3])}
TIMELINE = (T0, 1_000, 30)
EVERYTHING = dict(count_alive_keys=True, analytics=True, timeline=TIMELINE, key_sketch=True, hot_keys=True, ts_order=True,
                  partitioner=True, repartition=7)


def _base_cols():
    rng = np.random.default_rng(17)
    cols = random_cols(rng, N_REC, P, key_space=40, null_key=0.1, tomb=0.3, max_key=24, ts_missing=0.0)
    ts = np.empty(N_REC, np.int64)
    ts[:TILE] = T0 + rng.integers(0, 10_000, TILE)                      # wholly before
    ts[0] = FROM - 1
    ts[TILE:2 * TILE] = FROM + rng.integers(0, 5_000, TILE)             # wholly inside
    ts[TILE] = FROM
    ts[2 * TILE:3 * TILE] = TO - 600 + rng.integers(0, 1_200, TILE)     # straddles the end
    ts[2 * TILE + 1], ts[2 * TILE + 2] = TO - 1, TO
    ts[3 * TILE:] = FROM - 3_000 + rng.integers(0, 16_000, N_REC - 3 * TILE)
    ts[3 * TILE:][rng.random(N_REC - 3 * TILE) < 0.15] = -1
    cols["ts_ms"] = ts
    part = cols["partition"]
    for lo, hi in ((0, TILE), (2 * TILE, N_REC)):                        # tile 1 keeps real partitions only
        sel = np.arange(lo, hi)
        part[sel[rng.random(hi - lo) < 0.02]] = -1
        part[sel[rng.random(hi - lo) < 0.02]] = P + 3
    return cols


@pytest.fixture(scope="module")
def base():
    cols = _base_cols()
    want = {k: np.nonzero(F.passes(cols["partition"], cols["ts_ms"], P, *v))[0] for k, v in KINDS.items()}
    return {"cols": cols, "idx": want}


def test_the_base_shape_is_what_the_tests_say(base):
    cols, idx = base["cols"], base["idx"]
    t = cols["ts_ms"]
    inwin = F.passes(cols["partition"], t, P, FROM, TO)
    assert not inwin[:TILE].any() and inwin[TILE:2 * TILE].all()
    assert inwin[2 * TILE:3 * TILE].any() and not inwin[2 * TILE:3 * TILE].all()
    assert inwin[3 * TILE:].any() and not inwin[3 * TILE:].all() and (t[3 * TILE:] == -1).any()
    assert F.predict_tiles(cols, P, FROM, TO) == (1, 1, 2, 1)
    assert (cols["partition"] == -1).any() and (cols["partition"] == P + 3).any() and (cols["val_len"] < 0).any()
    assert 0 < len(idx["both"]) < len(idx["time"]) < N_REC and 0 < len(idx["set"]) < N_REC
    assert (t[idx["set"]] == -1).any()                                  # a set alone lets "not available" through


# ---------------------------------------------------------------------------------------------- state of a context
_VECTORS = ("result_vector", "analytics_result_vector", "timeline_result_vector", "key_sketch_result_vector",
            "hot_keys_result_vector", "ts_order_result_vector", "partitioner_result_vector")


def snapshot(h, flags, table=False, bitmap=False):
    """Everything the contract names: kta_finish's status, result and counters, every section's snapshot vector, and the
    alive set (the exported bitmap, or the table's entries)."""
    lib = N.load()
    res = N.KtaResult()
    counters = np.zeros((h.n_partitions, N.KTA_NCOUNTERS), np.uint64)
    out = {"rc": lib.kta_finish(h._ctx, C.byref(res), counters.ctypes.data), "res": bytes(res), "counters": counters}
    for name in _VECTORS:
        if name != "result_vector" and not flags.get({"analytics_result_vector": "analytics", "timeline_result_vector": "timeline",
                                                      "key_sketch_result_vector": "key_sketch", "hot_keys_result_vector": "hot_keys",
                                                      "ts_order_result_vector": "ts_order", "partitioner_result_vector": "partitioner"}[name]):
            continue
        p, n = getattr(h, name)()
        a = np.empty(n, np.uint64)
        h._check(lib.kta_copy_to_host(h._ctx, a.ctypes.data, C.c_void_p(p), a.nbytes))
        out[name] = a
    if flags.get("count_alive_keys"):
        out["alive_keys"] = int(res.alive_keys)
        if table:
            slots, vals = h.alive_export_entries_host()
            order = np.argsort(slots, kind="stable")
            out["table_slots"], out["table_vals"] = slots[order], vals[order]
        if bitmap:
            out["bitmap"] = h.export_alive_bitmap()
    return out


def assert_same(got, want, what=""):
    assert set(got) == set(want), what
    for k in want:
        if isinstance(want[k], np.ndarray):
            assert np.array_equal(got[k], want[k]), (what, k)
        else:
            assert got[k] == want[k], (what, k, got[k], want[k])


def reference(flags, cols, idx, table=False, bitmap=False, seq=None):
    """An unfiltered context handed the records idx of cols as one batch (seq: their sequence numbers, table state)."""
    sub = F.take(cols, idx)
    if seq is not None:
        sub["seq"] = np.asarray(seq, np.uint64)[idx]
    with kta.HipMetricHandler(P, now=NOW, **flags) as h:
        b = None
        if len(idx):
            b, n = h.upload_batch(sub, with_keys=True)
            h.submit_device(b, n, 0)
        snap = snapshot(h, flags, table, bitmap)
        h.sync()
        if b is not None:
            h.device_batch_free(b)
    return snap


@pytest.fixture(scope="module")
def ref_everything(base):
    return {k: reference(EVERYTHING, base["cols"], base["idx"][k], bitmap=True) for k in KINDS}


def _view(b, lo):
    v = N.KtaBatch()
    v.partition, v.key_len, v.val_len = b.partition + 4 * lo, b.key_len + 4 * lo, b.val_len + 4 * lo
    v.ts_ms, v.key_off, v.key_bytes = b.ts_ms + 8 * lo, b.key_off + 4 * lo, b.key_bytes
    if b.seq:
        v.seq = b.seq + 8 * lo
    return v


def _with_front(cols, k):
    """cols behind k records of another kind: what a view at record k of the allocation skips"""
    rng = np.random.default_rng(99)
    front = random_cols(rng, k, P, key_space=7, max_key=9)
    front["ts_ms"][:] = FROM + 5                                         # would pass, were they part of the batch
    out = {name: np.concatenate([front[name], cols[name]]) for name in ("partition", "key_len", "val_len", "ts_ms")}
    out["key_off"] = np.concatenate([front["key_off"], cols["key_off"] + np.uint32(len(front["key_bytes"]))]).astype(np.uint32)
    out["key_bytes"] = np.concatenate([front["key_bytes"], cols["key_bytes"]])
    return out


def feed(h, cols, path, base_seq=0):
    """-> the device batches to free after the context's last read"""
    if path == "staging":
        h.submit_columns(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"], cols["key_off"], cols["key_bytes"], base_seq=base_seq)
        return []
    if path == "compact":
        b, n = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, n, base_seq)
        return [b]
    if path == "view":
        big = _with_front(cols, 300)
        if "seq" in cols:
            big["seq"] = np.concatenate([np.zeros(300, np.uint64), cols["seq"]])
        b, n = h.upload_batch(big, with_keys=True)
        h.submit_device(_view(b, 300), n - 300, base_seq)
        return [b]
    assert path == "messages"
    kb = cols["key_bytes"].tobytes()
    for i in range(len(cols["partition"])):
        kl = int(cols["key_len"][i])
        key = None if kl < 0 else kb[int(cols["key_off"][i]):int(cols["key_off"][i]) + kl]
        vl = int(cols["val_len"][i])
        h.handle_message(kta.Message(int(cols["partition"][i]), int(cols["ts_ms"][i]), key, None if vl < 0 else vl))
    return []


def filtered(flags, cols, kind, path, table=False, bitmap=False, slice_records=None, base_seq=0, **ctx):
    frm, to, parts = KINDS[kind] if isinstance(kind, str) else kind
    with kta.HipMetricHandler(P, now=NOW, **flags, **ctx) as h:
        h.set_filter(frm, to, parts)
        if slice_records:
            h.set_filter_slice(slice_records)
        held = feed(h, cols, path, base_seq)
        snap = snapshot(h, flags, table, bitmap)
        info = h.filter_info()
        h.sync()
        for b in held:
            h.device_batch_free(b)
    return snap, info


# ---------------------------------------------------------------------------------------------- the paths
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("path", ["staging", "compact", "view", "messages"])
def test_every_path_every_opt_in_bit_set_state(base, ref_everything, path, kind):
    ctx = {"batch_capacity": 1 << 10} if path == "messages" else {}
    got, info = filtered(EVERYTHING, base["cols"], kind, path, bitmap=True, **ctx)
    assert_same(got, ref_everything[kind], (path, kind))
    assert (info["seen"], info["passed"]) == (N_REC, len(base["idx"][kind]))
    frm, to, parts = KINDS[kind]
    if path == "compact":
        assert (info["tiles_summary_none"], info["tiles_summary_all"], info["tiles_read"], info["slices"]) == \
            F.predict_tiles(base["cols"], P, frm, to, parts)
    elif path == "view":
        assert (info["tiles_summary_none"], info["tiles_summary_all"], info["tiles_read"], info["slices"]) == \
            F.predict_tiles(_with_front(base["cols"], 300), P, frm, to, parts, first=300)
    else:                                                                # raw staging: no summaries to decide by
        batches = 4 if path == "messages" else 1
        assert (info["tiles_summary_none"], info["tiles_summary_all"]) == (0, 0)
        assert info["tiles_read"] == 4 and info["slices"] == batches


def test_summaries_decide_tiles_on_the_compact_path_only(base):
    _, compact = filtered({}, base["cols"], "time", "compact")
    assert (compact["tiles_summary_none"], compact["tiles_summary_all"], compact["tiles_read"]) == (1, 1, 2)
    _, view = filtered({}, base["cols"], "time", "view")                # the view shifts the records against the allocation's tiles
    assert (view["tiles_summary_none"], view["tiles_summary_all"], view["tiles_read"], view["slices"]) == \
        F.predict_tiles(_with_front(base["cols"], 300), P, FROM, TO, first=300)
    _, staged = filtered({}, base["cols"], "time", "staging")
    assert (staged["tiles_summary_none"], staged["tiles_summary_all"], staged["tiles_read"]) == (0, 0, 4)
    _, by_set = filtered({}, base["cols"], "set", "compact")
    assert (by_set["tiles_summary_none"], by_set["tiles_summary_all"], by_set["tiles_read"]) == (0, 0, 4)


@pytest.mark.parametrize("path", ["staging", "compact"])
def test_the_fused_pass_behind_the_filter(base, path):
    """-c alone: both handlers in one pass over the scratch batch (bit set state, which == 3)."""
    flags = dict(count_alive_keys=True)
    want = reference(flags, base["cols"], base["idx"]["both"], bitmap=True)
    got, _ = filtered(flags, base["cols"], "both", path, bitmap=True)
    assert_same(got, want, path)
    plain = reference({}, base["cols"], base["idx"]["both"])
    got, _ = filtered({}, base["cols"], "both", path)
    assert_same(got, plain, path)


@pytest.mark.parametrize("path", ["staging", "compact", "view"])
def test_table_state_without_a_seq_column(base, path):
    """records keep base_seq + their index in the batch they came in"""
    flags = dict(count_alive_keys=True, alive_table=True, ts_order=True)
    want = reference(flags, base["cols"], base["idx"]["both"], table=True, seq=77 + np.arange(N_REC))
    got, _ = filtered(flags, base["cols"], "both", path, table=True, base_seq=77)
    assert_same(got, want, path)
    assert len(want["table_slots"]) > 10


@pytest.mark.parametrize("path", ["compact", "view"])
def test_table_state_with_a_callers_seq_column(base, path):
    flags = dict(count_alive_keys=True, alive_table=True)
    seq = (1000 + 3 * np.arange(N_REC)).astype(np.uint64)
    cols = dict(base["cols"], seq=seq)
    want = reference(flags, base["cols"], base["idx"]["time"], table=True, seq=seq)
    got, _ = filtered(flags, cols, "time", path, table=True)
    assert_same(got, want, path)
    # a descending seq column: the earliest record of a key is its last writer; the single-kernel update takes the batch
    seq = (10**6 - 3 * np.arange(N_REC)).astype(np.uint64)
    want = reference(flags, base["cols"], base["idx"]["time"], table=True, seq=seq)
    got, _ = filtered(flags, dict(base["cols"], seq=seq), "time", path, table=True)
    assert_same(got, want, path + ", descending")


def test_staged_seq_column_and_handle_message_in_the_table_state(base):
    """KTA_FLAG_SEQ_COLUMN: the ring's seq column; kta_handle_message numbers the records it is handed, passing or not"""
    flags = dict(count_alive_keys=True, seq_column=True)
    want = reference(dict(count_alive_keys=True, alive_table=True), base["cols"], base["idx"]["both"], table=True, seq=np.arange(N_REC))
    got, info = filtered(flags, base["cols"], "both", "messages", table=True, batch_capacity=1 << 10)
    assert_same(got, want)
    assert info["slices"] == 4 and info["seen"] == N_REC


@pytest.mark.parametrize("first", [5, 8])
def test_whole_tiles_behind_a_cut_one(base, first):
    """`first` records of tile 0 pass, tiles 1 and 2 pass whole: behind an offset that is a multiple of four they are copied
    with 16-byte stores, behind any other record by record — compact, raw (staging) and u16-length tiles, with key_off and seq"""
    cols = {k: v.copy() for k, v in base["cols"].items()}
    cols["partition"][:3 * TILE] = np.where((cols["partition"][:3 * TILE] < 0) | (cols["partition"][:3 * TILE] >= P), 1, cols["partition"][:3 * TILE])
    rng = np.random.default_rng(first)
    cols["ts_ms"][:TILE] = T0 + rng.integers(0, 9_000, TILE)
    cols["ts_ms"][rng.choice(TILE, first, replace=False)] = FROM + 7
    cols["ts_ms"][TILE:3 * TILE] = FROM + rng.integers(0, 9_000, 2 * TILE)
    idx = np.nonzero(F.passes(cols["partition"], cols["ts_ms"], P, FROM, TO))[0]
    assert (idx < TILE).sum() == first and ((idx >= TILE) & (idx < 3 * TILE)).sum() == 2 * TILE
    flags = dict(count_alive_keys=True, alive_table=True, key_sketch=True, ts_order=True)
    want = reference(flags, cols, idx, table=True, seq=3 + np.arange(N_REC))
    for path in ("compact", "staging", "view"):
        got, info = filtered(flags, cols, (FROM, TO, None), path, table=True, base_seq=3)
        assert_same(got, want, path)
        if path == "compact":
            assert (info["tiles_summary_none"], info["tiles_summary_all"], info["tiles_read"]) == (0, 2, 2)
    seq = (50 + 2 * np.arange(N_REC)).astype(np.uint64)
    want = reference(flags, cols, idx, table=True, seq=seq)
    got, _ = filtered(flags, dict(cols, seq=seq), (FROM, TO, None), "compact", table=True)
    assert_same(got, want, "seq column")
    plain = reference({}, cols, idx)                                    # a keyless allocation: u16 lengths in the tiles
    with kta.HipMetricHandler(P, now=NOW) as h:
        h.set_filter(FROM, TO)
        b, n = h.upload_batch(cols, with_keys=False)
        h.submit_device(b, n, 0, which=1)
        assert_same(snapshot(h, {}), plain, "keyless")
        h.sync()
        h.device_batch_free(b)


# ---------------------------------------------------------------------------------------------- slices
@pytest.mark.parametrize("path", ["compact", "staging", "view"])
def test_slices_of_1024_and_2048_give_identical_results(base, ref_everything, path):
    one, info1 = filtered(EVERYTHING, base["cols"], "time", path, bitmap=False, slice_records=1024)
    two, info2 = filtered(EVERYTHING, base["cols"], "time", path, bitmap=False, slice_records=2048)
    want = {k: v for k, v in ref_everything["time"].items() if k != "bitmap"}
    assert_same(one, want, path)
    assert_same(two, want, path)
    assert (info1["slices"], info2["slices"]) == (4, 2)
    assert info1["passed"] == info2["passed"] == len(base["idx"]["time"])
    if path == "compact":
        for info, step in ((info1, 1024), (info2, 2048)):
            assert (info["tiles_summary_none"], info["tiles_summary_all"], info["tiles_read"], info["slices"]) == \
                F.predict_tiles(base["cols"], P, FROM, TO, slice_records=step)


def test_slices_in_the_table_state(base):
    flags = dict(count_alive_keys=True, alive_table=True)
    want = reference(flags, base["cols"], base["idx"]["both"], table=True, seq=5 + np.arange(N_REC))
    for step in (1024, 2048):
        got, info = filtered(flags, base["cols"], "both", "compact", table=True, slice_records=step, base_seq=5)
        assert_same(got, want, step)


# ---------------------------------------------------------------------------------------------- edges
def test_nothing_passes_leaves_a_fresh_context(base):
    with kta.HipMetricHandler(P, now=NOW, **EVERYTHING) as h:
        fresh = snapshot(h, EVERYTHING, bitmap=True)
    for path in ("staging", "compact"):
        got, info = filtered(EVERYTHING, base["cols"], (1, 2, None), path, bitmap=True)
        assert_same(got, fresh, path)
        assert got["result_vector"][P * 7 + N.KTA_G_RECORDS] == 0 and got["rc"] == N.KTA_OK
        assert (info["seen"], info["passed"]) == (N_REC, 0)
        if path == "compact":                                           # three whole tiles rejected from 24 bytes each
            assert (info["tiles_summary_none"], info["tiles_read"]) == (3, 1)


def test_everything_passes_equals_no_filter(base):
    cols = {k: v.copy() for k, v in base["cols"].items()}
    cols["partition"] = np.where((cols["partition"] < 0) | (cols["partition"] >= P), 2, cols["partition"]).astype(np.int32)
    want = reference(EVERYTHING, cols, np.arange(N_REC), bitmap=True)
    for path in ("staging", "compact", "view"):
        got, info = filtered(EVERYTHING, cols, (None, None, list(range(P))), path, bitmap=True)
        assert_same(got, want, path)
        assert info["passed"] == info["seen"] == N_REC
    # a window over every timestamp: whole tiles pass by their summaries, and the batch is handed on as it is
    cols["ts_ms"] = np.where(cols["ts_ms"] == -1, FROM, cols["ts_ms"])
    want = reference(EVERYTHING, cols, np.arange(N_REC), bitmap=True)
    for path in ("compact", "view", "staging"):
        got, info = filtered(EVERYTHING, cols, (T0 - 1, T0 + 10**9, None), path, bitmap=True, slice_records=2048)
        assert_same(got, want, path)
        assert info["passed"] == N_REC
        if path == "compact":
            assert (info["tiles_summary_all"], info["tiles_read"]) == (3, 1)
    want = reference(dict(count_alive_keys=True, alive_table=True), cols, np.arange(N_REC), table=True, seq=9 + np.arange(N_REC))
    got, _ = filtered(dict(count_alive_keys=True, alive_table=True), cols, (T0 - 1, T0 + 10**9, None), "compact", table=True,
                      slice_records=1024, base_seq=9)
    assert_same(got, want, "table state, handed on in slices")


def test_chrono_range_and_bad_partitions(base):
    cols = {k: v.copy() for k, v in base["cols"].items()}
    cols["ts_ms"][5] = (N.KTA_CHRONO_MAX_SEC + 5) * 1000                 # where the reference panics
    cols["partition"][5] = 1
    for path in ("staging", "compact"):
        got, _ = filtered({}, cols, (FROM, TO, None), path)
        assert got["rc"] == N.KTA_ERR_BAD_PARTITION                     # outside the window: no chrono panic; bad partitions pass
        inside, _ = filtered({}, cols, (FROM, None, None), path)
        assert inside["rc"] == N.KTA_ERR_TIMESTAMP_RANGE
        idx = np.nonzero(F.passes(cols["partition"], cols["ts_ms"], P, FROM, None))[0]
        assert 5 in idx
        assert_same(inside, reference({}, cols, idx), path)
        under_set, _ = filtered({}, cols, (None, None, [0, 1, 2, 3, 4]), path)
        assert under_set["rc"] == N.KTA_ERR_TIMESTAMP_RANGE             # record 5 passes the set
        quiet, _ = filtered({}, cols, (FROM, TO, [0, 1, 2, 3, 4]), path)
        assert quiet["rc"] == N.KTA_OK and quiet["result_vector"][P * 7 + N.KTA_G_BAD_PARTITION] == 0
    no_set = reference({}, cols, base["idx"]["time"])
    assert no_set["result_vector"][P * 7 + N.KTA_G_BAD_PARTITION] > 0   # counted and reported as without a filter


def test_set_filter_rules_and_reset(base):
    cols = base["cols"]
    with kta.HipMetricHandler(P, now=NOW, count_alive_keys=True, ts_order=True) as h:
        flags = dict(count_alive_keys=True, ts_order=True)
        with pytest.raises(kta.KtaError, match="below to_ms"):
            h.set_filter(5, 5)
        with pytest.raises(kta.KtaError, match="below to_ms"):
            h.set_filter(6, 5)
        with pytest.raises(kta.KtaError, match="at or beyond P"):
            h.set_filter(partitions=[P])
        with pytest.raises(kta.KtaError, match="at or beyond P"):
            h.set_filter(partitions=[1, 64])
        with pytest.raises(kta.KtaError, match="multiple of 1024"):
            h.set_filter_slice(1000)
        with pytest.raises(kta.KtaError):
            h.set_filter_slice((1 << 26) + 1024)
        assert h.filter_info() == dict(seen=0, passed=0, tiles_summary_none=0, tiles_summary_all=0, tiles_read=0, slices=0)
        h.set_filter(1, 2)
        h.set_filter(*KINDS["both"])                                    # may be changed while no record was handed over
        held = feed(h, cols, "compact")
        first = snapshot(h, flags, bitmap=True)
        with pytest.raises(kta.KtaError, match="handed records"):
            h.set_filter(FROM, TO)
        assert h.filter_info()["passed"] == len(base["idx"]["both"])
        h.reset()
        assert h.filter_info()["seen"] == 0
        feed(h, cols, "staging")                                        # the filter is kept
        again = snapshot(h, flags, bitmap=True)
        assert_same(again, first)
        assert_same(first, reference(flags, cols, base["idx"]["both"], bitmap=True))
        h.reset()
        h.set_filter()                                                  # no bound, no set: no filter again
        feed(h, cols, "staging")
        assert_same(snapshot(h, flags), reference(flags, cols, np.arange(N_REC)))
        assert h.filter_info()["seen"] == 0
        h.sync()
        for b in held:
            h.device_batch_free(b)
    with kta.HipMetricHandler(P, now=NOW) as h:                          # a staged message counts as a record handed over
        h.handle_message(kta.Message(1, FROM, b"k", 3))
        with pytest.raises(kta.KtaError, match="handed records"):
            h.set_filter(FROM, TO)


def test_which_selects_the_handlers_behind_the_filter(base):
    cols, idx = base["cols"], base["idx"]["both"]
    flags = dict(count_alive_keys=True)
    want = reference(flags, cols, idx, bitmap=True)
    with kta.HipMetricHandler(P, now=NOW, **flags) as h:
        h.set_filter(*KINDS["both"])
        b, n = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, n, 0, which=2)
        only_alive = snapshot(h, flags, bitmap=True)
        assert only_alive["alive_keys"] == want["alive_keys"] and np.array_equal(only_alive["bitmap"], want["bitmap"])
        assert not only_alive["counters"].any()
        h.submit_device(b, n, 0, which=1)
        assert_same(snapshot(h, flags, bitmap=True), want)
        h.sync()
        h.device_batch_free(b)


def test_lengths_of_a_keyless_allocation_are_widened_on_the_way(base):
    """u16 lengths in the tiles of a keyless allocation: the scatter widens them; a view with the caller's own key columns"""
    cols = base["cols"]
    for flags, which in ((dict(), 1), (dict(key_sketch=True, partitioner=True), 1)):
        want = reference(flags, cols, base["idx"]["time"])
        with kta.HipMetricHandler(P, now=NOW, **flags) as h:
            h.set_filter(FROM, TO)
            keyless, n = h.upload_batch(cols, with_keys=False)
            v = keyless
            keyed = None
            if flags:
                keyed, _ = h.upload_batch(cols, with_keys=True)
                v = N.KtaBatch()
                v.partition, v.key_len, v.val_len, v.ts_ms = keyless.partition, keyless.key_len, keyless.val_len, keyless.ts_ms
                v.key_off, v.key_bytes = keyed.key_off, keyed.key_bytes
            h.submit_device(v, n, 0, which=which)
            assert_same(snapshot(h, flags), want, str(flags))
            h.sync()
            h.device_batch_free(keyless)
            if keyed is not None:
                h.device_batch_free(keyed)


# ---------------------------------------------------------------------------------------------- the Kafka decode
def test_kafka_consume_behind_the_filter():
    lib = N.load()
    spec, _ = kta.synth_preset("c2")
    n, rpb, part = 3000, 500, 2
    cols = kta.synth_fill_host(spec, 0, n, with_keys=True)
    cols["partition"] = np.full(n, part, np.int32)
    ln = C.c_uint64()
    lib.kta_kafka_encode_synth_host(C.byref(spec), 0, n, rpb, None, 0, C.byref(ln))
    buf = np.zeros(ln.value + 128, np.uint8)
    assert lib.kta_kafka_encode_synth_host(C.byref(spec), 0, n, rpb, buf.ctypes.data, ln.value, C.byref(ln)) == N.KTA_OK
    blob = buf[:ln.value].tobytes()
    timed = np.sort(cols["ts_ms"][cols["ts_ms"] != -1])
    frm, to = int(timed[len(timed) // 4]), int(timed[3 * len(timed) // 4])
    P_ = int(spec.n_partitions)
    flags = dict(count_alive_keys=True, ts_order=True, partitioner=True)
    for parts, expect_some in (([part], True), ([part + 1], False), (None, True)):
        idx = np.nonzero(F.passes(cols["partition"], cols["ts_ms"], P_, frm, to, parts))[0]
        assert (len(idx) > 100) == expect_some and len(idx) < n
        with kta.HipMetricHandler(P_, now=NOW, **flags) as ref:
            b = None
            if len(idx):
                b, m = ref.upload_batch(F.take(cols, idx), with_keys=True)
                ref.submit_device(b, m, 0)
            want = snapshot(ref, flags, bitmap=True)
            ref.sync()
            if b is not None:
                ref.device_batch_free(b)
        with kta.HipMetricHandler(P_, now=NOW, **flags) as h:
            h.set_filter(frm, to, parts)
            st = N.KtaKafkaIndexStats()
            h._check(lib.kta_kafka_consume(h._ctx, blob, len(blob), part, C.byref(st)))
            assert st.n_records == n
            assert_same(snapshot(h, flags, bitmap=True), want, str(parts))
            info = h.filter_info()
            assert (info["seen"], info["passed"]) == (n, len(idx))


# ---------------------------------------------------------------------------------------------- two ranks, test double
@pytest.fixture(scope="module")
def mock_rccl(tmp_path_factory):
    lib = tmp_path_factory.mktemp("mock") / "libmock_rccl.so"
    r = subprocess.run(["timeout", "-k", "10", "600", "/opt/rocm/bin/hipcc", "-O1", "-shared", "-fPIC", "-std=c++17",
                        os.path.join(ROOT, "tests", "mock_rccl.cpp"), "-o", str(lib), "-lrt", "-lpthread"],
                       capture_output=True, text=True, timeout=660)
    assert r.returncode == 0, r.stderr[-2000:]
    return str(lib)


_EXCHANGE_WORKER = r'''
import os, sys, threading
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import ctypes as C
import numpy as np
import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import filter_py as F
from helpers import NOW, random_cols

P, nranks = 6, 2
rng = np.random.default_rng(23)
cols = random_cols(rng, 30000, P, key_space=2000, tomb=0.3, max_key=32)
n = len(cols["partition"])
cols["seq"] = np.arange(n, dtype=np.uint64)
timed = np.sort(cols["ts_ms"][cols["ts_ms"] != -1])
FROM, TO, PARTS = int(timed[n // 5]), int(timed[4 * n // 5]), [0, 1, 2, 4]
idx = np.nonzero(F.passes(cols["partition"], cols["ts_ms"], P, FROM, TO, PARTS))[0]
assert 1000 < len(idx) < n
VECTORS = ("result_vector", "ts_order_result_vector", "partitioner_result_vector", "key_sketch_result_vector")

def vectors(h):
    out = {}
    for name in VECTORS:
        p, m = getattr(h, name)()
        a = np.empty(m, np.uint64)
        h._check(h._lib.kta_copy_to_host(h._ctx, a.ctypes.data, C.c_void_p(p), a.nbytes))
        out[name] = a
    return out

for with_c in (False, True):
    flags = dict(count_alive_keys=with_c, seq_column=with_c, ts_order=True, partitioner=True, key_sketch=True)
    # the unsharded, unfiltered context handed the host-filtered records as one batch
    ref = kta.HipMetricHandler(P, now=NOW, **flags)
    sub = F.take(cols, idx, with_seq=with_c)
    b, m = ref.upload_batch(sub, with_keys=True)
    ref.submit_device(b, m, 0)
    want_res, want_c = ref.finish()
    want = vectors(ref)
    ref.sync(); ref.device_batch_free(b); ref.close()
    uid = kta.HipMetricHandler.comm_unique_id()
    errors = []
    def run(rank):
        try:
            h = kta.HipMetricHandler(P, now=NOW, **flags)
            h.set_filter(FROM, TO, PARTS)
            h.set_filter_slice(4096)
            h.comm_create(nranks, rank, uid)
            mine = np.nonzero(cols["partition"] % nranks == rank)[0]
            b, m = h.upload_batch(F.take(cols, mine, with_seq=with_c), with_keys=True)
            h.submit_device(b, m, 0)
            h.exchange()
            res, c = h.exchange_result()
            assert np.array_equal(c, want_c), (with_c, rank, "counters")
            assert (res.overall_count, res.alive_keys) == (want_res.overall_count, want_res.alive_keys), (with_c, rank, res.alive_keys, want_res.alive_keys)
            got = vectors(h)
            for name in VECTORS:
                if name == "result_vector":
                    continue    # (its alive word is the owner's share until decoded: compared through exchange_result above)
                assert np.array_equal(got[name], want[name]), (with_c, rank, name)
            info = h.filter_info()
            assert info["seen"] == len(mine) and info["passed"] == int(np.isin(mine, idx).sum()), (rank, info)
            h.sync(); h.device_batch_free(b)
            h.comm_destroy(); h.close()
        except BaseException as e:
            errors.append((rank, repr(e)))
            print("rank %d: %r" % (rank, e), file=sys.stderr, flush=True)
            os._exit(2)        # the other rank would wait in its collectives for ever
    ts = [threading.Thread(target=run, args=(r,)) for r in range(nranks)]
    [t.start() for t in ts]; [t.join() for t in ts]
    assert not errors, errors
    print("ranks", nranks, "-c" if with_c else "", "OK", flush=True)
print("OK")
'''


def test_two_filtered_ranks_equal_the_unsharded_host_filtered_result(tmp_path, mock_rccl):
    script = tmp_path / "filter_exchange_worker.py"
    script.write_text(_EXCHANGE_WORKER)
    env = dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(script), ROOT], capture_output=True, text=True,
                       timeout=330, env=env)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count(" OK") == 2


# ---------------------------------------------------------------------------------------------- kta-analyzer
def _cli(*args, env=None):
    return subprocess.run(["timeout", "-k", "10", "240", CLI, *args], capture_output=True, text=True, timeout=270, env=env)


def _normalise(text):
    text = re.sub(r"Scanning took: \d+ seconds", "Scanning took: 3 seconds", text)
    return re.sub(r"Estimated Msg/s: \d+", "Estimated Msg/s: 133", text)


HEAD = "Subscribing to %s\nStarting message consumption...\n"


def _mirror_report(topic, cols, idx, n_partitions, with_c, start, end):
    """The report of the Python mirror (kta_render_report over the oracle's counter vector) for the records idx of cols."""
    from oracle_c import Oracle
    from test_dist import oracle_vector
    from test_report_cli import render
    sub = F.take(cols, idx)
    vec, _ = oracle_vector(sub, n_partitions, NOW)
    if with_c:
        o = Oracle(NOW, count_alive_keys=True)
        o.run_soa(sub)
        vec[n_partitions * 7 + N.KTA_G_ALIVE_KEYS] = o.alive_keys()
    rc, text = render(topic, 3, vec, n_partitions, 1 if with_c else 0, NOW, start, end)
    assert rc == N.KTA_OK
    return _normalise(text)


def test_cli_synthetic_topic_with_a_window_and_a_set(mock_rccl):
    n = 60000
    src = "synthetic://c2?records=%d" % n
    sp, _ = kta.synth_preset("c2")
    cols = kta.synth_fill_host(sp, 0, n, with_keys=True)
    P_ = int(sp.n_partitions)
    timed = np.sort(cols["ts_ms"][cols["ts_ms"] != -1])
    frm, to = int(timed[n // 4]) // 1000, int(timed[3 * n // 4]) // 1000
    assert frm < to
    parts = [0, 3, 4, 5]
    idx = np.nonzero(F.passes(cols["partition"], cols["ts_ms"], P_, frm * 1000, to * 1000, parts))[0]
    assert 1000 < len(idx) < n // 2
    totals = np.bincount(cols["partition"][idx], minlength=P_).astype(np.int64)
    section = F.section(P_, n, len(idx), frm * 1000, to * 1000, parts)
    knobs = "kta.from=%d,kta.to=%d,kta.partitions=0,3-5" % (frm, to)
    for with_c in (False, True):
        want = _mirror_report("c2", cols, idx, P_, with_c, np.zeros(P_, np.int64), totals) + section
        r = _cli("-t", "c2", "-b", src, *(["-c"] if with_c else []), "--librdkafka", knobs + ",kta.batch=8192")
        assert r.returncode == 0, r.stderr
        assert r.stdout.startswith(HEAD % "c2") and _normalise(r.stdout[len(HEAD % "c2"):]) == want, with_c
    want = _mirror_report("c2", cols, idx, P_, True, np.zeros(P_, np.int64), totals) + section
    pm = _cli("-t", "c2", "-b", src, "-c", "--librdkafka", "kta.partitions=0,3-5,kta.per_message=1,kta.batch=4096,kta.from=%d,kta.to=%d" % (frm, to))
    assert pm.returncode == 0 and _normalise(pm.stdout[len(HEAD % "c2"):]) == want, pm.stderr
    env = dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl)
    for c in ([], ["-c"]):
        many = _cli("-t", "c2", "-b", src, *c, "--librdkafka", knobs + ",kta.gpus=2,kta.batch=8192,kta.oversubscribe=1", env=env)
        assert many.returncode == 0, (c, many.stderr[-2000:])
        want = _mirror_report("c2", cols, idx, P_, bool(c), np.zeros(P_, np.int64), totals) + section
        assert _normalise(many.stdout[len(HEAD % "c2"):]) == want, c
    # with the other sections: each describes the passing records, the filter's comes after all of them; one bound alone
    others = "kta.ts_order=1,kta.partitioner=murmur2"
    r = _cli("-t", "c2", "-b", src, "--librdkafka", others + ",kta.from=%d" % frm)
    assert r.returncode == 0, r.stderr
    idx_from = np.nonzero(F.passes(cols["partition"], cols["ts_ms"], P_, frm * 1000))[0]
    assert r.stdout.endswith(F.section(P_, n, len(idx_from), frm * 1000))
    assert r.stdout.index("Timestamp order") < r.stdout.index("Partitioner check:") < r.stdout.index("Record filter:")
    import partitioner_py as R
    sub = F.take(cols, idx_from)
    assert R.section(R.vector(sub, P_, P_), R.counters(sub, P_), P_, P_) in r.stdout


def test_cli_without_the_keys_prints_the_existing_golden_and_a_dump_source_filters_too(tmp_path):
    from helpers import GOLDEN, load_golden, records_to_cols, scenario_records
    from test_report_cli import write_dump
    g = load_golden("scenarios.json")
    P_ = g["n_partitions"]
    cols = records_to_cols(scenario_records(g["scenarios"]["mixed_400"]))
    path = str(tmp_path / "mixed_400.ktadump")
    write_dump(path, cols, P_)
    topic = "synthetic.mixed_400"
    for with_c in (False, True):
        r = _cli("-t", topic, "-b", "dump://" + path, *(["-c"] if with_c else []), "--librdkafka", "kta.batch=128")
        assert r.returncode == 0, r.stderr
        want = open(os.path.join(GOLDEN, "report_mixed_400_%s.txt" % ("with_c" if with_c else "without_c"))).read()
        assert _normalise(r.stdout[len(HEAD % topic):]) == want and "Record filter" not in r.stdout
    timed = np.sort(cols["ts_ms"][cols["ts_ms"] >= 0])
    to = int(timed[len(timed) // 2]) // 1000 + 1
    parts = list(range(1, P_))
    idx = np.nonzero(F.passes(cols["partition"], cols["ts_ms"], P_, None, to * 1000, parts))[0]
    assert 10 < len(idx) < len(cols["partition"])
    totals = np.bincount(cols["partition"][(cols["partition"] >= 0) & (cols["partition"] < P_)], minlength=P_).astype(np.int64)
    r = _cli("-t", topic, "-b", "dump://" + path, "-c", "--librdkafka", "kta.batch=128,kta.to=%d,kta.partitions=1-%d" % (to, P_ - 1))
    assert r.returncode == 0, r.stderr
    want = _mirror_report(topic, cols, idx, P_, True, np.zeros(P_, np.int64), totals) + F.section(P_, len(cols["partition"]), len(idx), None, to * 1000, parts)
    assert _normalise(r.stdout[len(HEAD % topic):]) == want

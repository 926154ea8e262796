"""GPU tests of the host layer's section table (csrc/kta_api.hip, sections_of): one context with every snapshot section
on, and for every section, by one list, what the table promises of all of them alike — the read-back, the snapshot and
the merge agree on the length; the snapshot kta_finish_device takes is the live vector; a buffer of another length is
refused; kta_reset empties the live vector and leaves the snapshot; a context without the section refuses each of its
entry points with the section's own message.  What any one section computes is its own test file's business."""
import ctypes as C

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N

pytestmark = pytest.mark.gpu

P, Q, M = 3, 5, 4
TIMELINE = (0, 10, 4)
SEGMENTS = (1000, M, 0)
CONFIG = dict(analytics=True, key_sketch=True, hot_keys=True, ts_order=True, partitioner=True, repartition=Q, size_quantiles=True,
              timeline=TIMELINE, segments=SEGMENTS, batch_capacity=256, key_bytes_capacity=1 << 14)

# name: (the arguments of kta_merge_<name> behind the two vectors, a substring of the section's "off" message)
SECTIONS = {
    "analytics": ((P,), "KTA_FLAG_ANALYTICS"),
    "timeline": (None, "no timeline"),                     # (no merge: every word a sum)
    "key_sketch": ((P,), "KTA_FLAG_KEY_SKETCH"),
    "hot_keys": ((), "KTA_FLAG_HOT_KEYS"),
    "ts_order": ((P,), "KTA_FLAG_TS_ORDER"),
    "partitioner": ((P, Q), "KTA_FLAG_PARTITIONER"),
    "size_quantiles": ((P,), "KTA_FLAG_SIZE_QUANTILES"),
    "segments": ((P, M), "no segments"),
}
U64_SECTIONS = [s for s in SECTIONS if s != "analytics"]   # (the analytics read-back is struct-shaped: no buffer length)


def _records():
    """About 300 keyed records over the three partitions: a few tombstones, a few with partition id 3, in two batches."""
    rng = np.random.default_rng(7)
    n = 300
    part = rng.integers(0, P, n).astype(np.int32)
    part[::37] = P                                          # outside [0, P)
    key_len = np.full(n, 8, np.int32)
    val_len = rng.integers(0, 400, n).astype(np.int32)
    val_len[::23] = -1                                      # tombstones
    ts = (np.arange(n, dtype=np.int64) // 5 + rng.integers(-3, 4, n)).clip(0)   # buckets, "after", and late records
    keys = rng.integers(0, 20, n).astype("<u8")             # 20 distinct 8-byte keys: some are heavy
    cols = {"partition": part, "key_len": key_len, "val_len": val_len, "ts_ms": ts, "key_off": (np.arange(n) * 8).astype(np.uint32),
            "key_bytes": keys.view(np.uint8)}
    return cols, n


def _feed(h):
    cols, n = _records()
    for lo, hi in ((0, n // 2), (n // 2, n)):
        h.submit_columns(cols["partition"][lo:hi], cols["key_len"][lo:hi], cols["val_len"][lo:hi], cols["ts_ms"][lo:hi],
                         cols["key_off"][lo:hi] - 8 * lo, cols["key_bytes"][8 * lo:8 * hi])


def _flat(x):
    """A read-back as the handler answers it -> the section's u64 vector (the analytics dict: its parts, in one order)."""
    if isinstance(x, dict) and "vector" in x:
        return np.asarray(x["vector"]).reshape(-1)
    if isinstance(x, dict):
        return np.concatenate([np.asarray(x[k]).reshape(-1).view(np.uint64) for k in sorted(x)])
    return np.asarray(x).reshape(-1)


def _live(h, name):
    return _flat(getattr(h, name)())


def _snapshot(h, name):
    return _flat(getattr(h, "exchange_" + name)())


def _merge_words(entry, args):
    """The words the merge `entry` works on: those it changes when every word of acc is 0 and every word of other is 1 (a
    sum and either maximum make 1 of them), counted in buffers with room to spare behind them."""
    room = 2 * 1024 * 23 + 4096 * P + 64
    acc, other = np.zeros(room, np.uint64), np.ones(room, np.uint64)
    assert getattr(N.load(), entry)(acc.ctypes.data, other.ctypes.data, *args) == N.KTA_OK
    words = int(acc.sum())
    assert acc[:words].all() and not acc[words:].any() and words < room
    return words


@pytest.fixture(scope="module")
def state():
    """The fed context after kta_finish_device and kta_reset, with what it answered at each stage (read once, shared)."""
    with kta.HipMetricHandler(P, **CONFIG) as h, kta.HipMetricHandler(P, **CONFIG) as fresh:
        _feed(h)
        live = {s: _live(h, s) for s in SECTIONS}
        lengths = {s: getattr(h, s + "_result_vector")()[1] for s in SECTIONS}
        h.finish_device()
        snap = {s: _snapshot(h, s) for s in SECTIONS}
        counters = h.result_vector_host()
        h.reset()
        yield {"h": h, "live": live, "counters": counters, "counters_after_reset": h.result_vector_host(), "lengths": lengths,
               "snap": snap, "after_reset": {s: _live(h, s) for s in SECTIONS},
               "snap_after_reset": {s: _snapshot(h, s) for s in SECTIONS}, "fresh": {s: _live(fresh, s) for s in SECTIONS}}


@pytest.mark.parametrize("name", list(SECTIONS))
def test_read_back_snapshot_and_merge_agree_on_the_length(state, name):
    words = state["lengths"][name]
    print(name, "result vector:", words, "read-back:", state["live"][name].size)
    if name != "analytics":      # (the analytics dict holds the vector decoded: the histograms and four arrays of P)
        assert state["live"][name].size == words
    else:
        assert state["live"][name].size == N.KTA_ANALYTICS_HIST + 4 * P == words
    if name == "timeline":
        assert words == (TIMELINE[2] + 3) * N.KTA_TIMELINE_COLS
    elif name == "segments":     # (kta_merge_segments has its own rule and refuses what is no segment vector)
        assert words == N.load().kta_segments_words(P, M)
    else:
        assert words == _merge_words("kta_merge_" + name, SECTIONS[name][0])


@pytest.mark.parametrize("name", list(SECTIONS))
def test_snapshot_is_the_live_vector(state, name):
    """One rank: what kta_finish_device snapshots is the live vector, word for word (the key sketch's: its widened
    registers).  A kind that the snapshot loop misses leaves its snapshot at the zeros it was created with."""
    assert state["live"][name].any(), "the records reach every section"
    assert np.array_equal(state["snap"][name], state["live"][name])


def test_counters_row(state):
    """The one section that is always on, and the only one without a u64 read-back of its live vector: its snapshot has the
    length kta_merge_vectors works on, holds what the records say, and stays through kta_reset."""
    cols, n = _records()
    v = state["counters"]
    assert v.size == P * N.KTA_NCOUNTERS + N.KTA_NGLOBALS == _merge_words("kta_merge_vectors", (P,))
    inside = cols["partition"] < P
    assert np.array_equal(v[:P * N.KTA_NCOUNTERS].reshape(P, N.KTA_NCOUNTERS)[:, N.KTA_C_TOTAL], np.bincount(cols["partition"][inside], minlength=P))
    assert v[P * N.KTA_NCOUNTERS + N.KTA_G_BAD_PARTITION] == n - inside.sum() > 0
    assert np.array_equal(state["counters_after_reset"], v)


@pytest.mark.parametrize("name", U64_SECTIONS)
@pytest.mark.parametrize("entry", ["kta_get_", "kta_exchange_"])
@pytest.mark.parametrize("off_by", [-1, 1])
def test_buffer_of_another_length_is_refused(state, name, entry, off_by):
    h, lib = state["h"], N.load()
    words = state["lengths"][name] + off_by
    buf = np.zeros(words, np.uint64)
    rc = getattr(lib, entry + name)(h._ctx, buf.ctypes.data, words)
    msg = lib.kta_last_error(h._ctx).decode()
    print(entry + name, words, "->", rc, msg)
    assert rc == N.KTA_ERR_INVALID and "u64 words, not" in msg and not buf.any()


@pytest.mark.parametrize("name", list(SECTIONS))
def test_reset_empties_the_live_vector_and_keeps_the_snapshot(state, name):
    assert np.array_equal(state["after_reset"][name], state["fresh"][name])
    assert np.array_equal(state["snap_after_reset"][name], state["snap"][name])


@pytest.fixture(scope="module")
def bare():
    with kta.HipMetricHandler(P) as h:
        yield h


@pytest.mark.parametrize("name", list(SECTIONS))
def test_context_without_the_section_refuses_its_entry_points(bare, name):
    lib, ctx, want = N.load(), bare._ctx, SECTIONS[name][1]
    buf, ptr, n = np.zeros(8, np.uint64), C.c_void_p(), C.c_size_t()

    def refused(rc):
        msg = lib.kta_last_error(ctx).decode()
        print(name, "->", rc, msg)
        return rc == N.KTA_ERR_INVALID and want in msg

    assert refused(getattr(lib, "kta_%s_result_vector" % name)(ctx, C.byref(ptr), C.byref(n)))
    if name == "analytics":
        a, parts = N.KtaAnalytics(), [np.zeros(P, np.uint64) for _ in range(4)]
        for fn in (lib.kta_get_analytics, lib.kta_exchange_analytics):
            assert refused(fn(ctx, C.byref(a), *[p.ctypes.data for p in parts]))
    else:
        for entry in ("kta_get_", "kta_exchange_"):
            assert refused(getattr(lib, entry + name)(ctx, buf.ctypes.data, buf.size))
    if name in ("analytics", "timeline"):                   # (the two with a live-vector hand-out)
        assert refused(getattr(lib, "kta_%s_vector" % name)(ctx, C.byref(ptr), C.byref(n)))

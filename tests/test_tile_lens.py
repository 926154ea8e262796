"""u16 lengths in the tiles of keyless tile-compact device batches (include/kta_hip.h): kta_tile_hdr.lens,
packed by kta_batch_from_raw / kta_synth_fill_device, unpacked by kta_batch_to_raw, widened in place before a raw-layout
producer or a key-reading pass touches them, read by the tiled scan.  Every result must be what the raw layout gives,
bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
from helpers import NOW
from oracle_c import Oracle

T = 1024                 # KTA_TILE_RECORDS
METRIC = ("partition", "key_len", "val_len", "ts_ms")
SIZES = (("partition", 4), ("key_len", 4), ("val_len", 4), ("ts_ms", 8))


def test_layout_constants():
    src = open(N.__file__.replace("_native.py", "../include/kta_hip.h")).read()
    assert "#define KTA_TILE_LENS_I32 0u" in src and N.KTA_TILE_LENS_I32 == 0
    assert "#define KTA_TILE_LENS_U16 1u" in src and N.KTA_TILE_LENS_U16 == 1
    assert "#define KTA_COMPACT_LEN_NONE 0xFFFFu" in src
    assert "#define KTA_ABI_VERSION 7 " in src


@pytest.mark.parametrize("preset", ["c4", "c2"])
def test_presets_are_all_u16(preset):
    """The condition under which every tile of the bench's batch is stored with u16 lengths."""
    sp, _ = kta.synth_preset(preset)
    cols = kta.synth_fill_host(sp, 0, 1 << 20)
    for k in ("key_len", "val_len"):
        assert cols[k].min() >= -1 and cols[k].max() < 65535, k


# ---- the edge cases of the u16 form, one per tile ------------------------------------------------------------------
def _case_list(cols):
    p, kl, vl = cols["partition"], cols["key_len"], cols["val_len"]

    def at(s, j):
        return s.start + j % (s.stop - s.start)

    def all_none(s):
        kl[s] = -1
        vl[s] = -1

    # (apply, lens, mode or None: whatever the generated partitions and timestamps give — compact)
    return [
        (lambda s: None, 1, 1),                                        # lengths as generated
        (lambda s: kl.__setitem__(at(s, 3), 65534), 1, 1),             # the largest u16 length
        (lambda s: kl.__setitem__(at(s, 3), 65535), 0, 1),             # the sentinel's value: i32
        (lambda s: vl.__setitem__(at(s, 5), 65535), 0, 1),
        (lambda s: vl.__setitem__(at(s, 5), 1 << 20), 0, 1),
        (lambda s: kl.__setitem__(at(s, 7), -2), 0, 1),                # below -1: i32
        (all_none, 1, 1),                                              # every length None
        (lambda s: p.__setitem__(at(s, 9), 1 << 20), 1, 0),            # u16 lengths, raw partitions
        (lambda s: vl.__setitem__(at(s, 11), 70000), 0, 1),            # i32 lengths, compact partitions
    ]


def _edge_tiles(cols, first_case=0):
    """Overwrite whole tiles of a topic's columns with the cases, tile k taking case (first_case + k) % 9; returns the
    expected (lens, mode) of every tile."""
    n = len(cols["partition"])
    cases = _case_list(cols)
    want = []
    for k in range((n + T - 1) // T):
        s = slice(k * T, min(n, (k + 1) * T))
        apply, lens, mode = cases[(first_case + k) % len(cases)]
        apply(s)
        want.append((lens, mode))
    return want


def _topic(n, P, with_keys=False, seed=2):
    sp, _ = kta.synth_preset("c2")
    sp.seed, sp.n_partitions = seed, P
    return kta.synth_fill_host(sp, 0, n, with_keys=with_keys)


def _headers(h, b, ntiles):
    """[(lens, mode)] of the batch's first tiles."""
    raw = np.empty(2 * ntiles, np.uint64)
    h._check(N.load().kta_copy_to_host(h._ctx, raw.ctypes.data, b.tile_hdr, raw.nbytes))
    return [(int(x) >> 32, int(x) & 0xFFFFFFFF) for x in raw[1::2]]


def _view(b, lo, extra=()):
    v = kta.KtaBatch()
    for f, sz in SIZES + tuple(extra):
        setattr(v, f, getattr(b, f) + lo * sz)
    return v


def _round_trip(h, cols, want):
    n = len(cols["partition"])
    b, _ = h.upload_batch(cols)
    assert b.layout == N.KTA_LAYOUT_TILE_COMPACT
    assert _headers(h, b, len(want)) == want
    back = h.download_batch(b, n)
    for k in METRIC:
        assert np.array_equal(back[k], cols[k]), k
    if n > 1500:      # a view that starts inside a u16 tile and one that ends inside one
        part = h.download_batch(_view(b, 1500), n - 1500)
        for k in METRIC:
            assert np.array_equal(part[k], cols[k][1500:]), k
        part = h.download_batch(_view(b, 2 * T), 3 * T + 100)
        for k in METRIC:
            assert np.array_equal(part[k], cols[k][2 * T:5 * T + 100]), k
    h.device_batch_free(b)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1000, T, 10 * T + 37])
def test_keyless_round_trip(n):
    with kta.HipMetricHandler(8, now=NOW) as h:
        # a batch of one tile takes every case in turn, a larger one has them side by side
        for first_case in (range(9) if n <= T else (0, 4)):
            cols = _topic(n, 8)
            want = _edge_tiles(cols, first_case)
            _round_trip(h, cols, want)


@pytest.mark.gpu
def test_keyed_upload_has_no_u16_tiles():
    n = 10 * T + 37
    cols = _topic(n, 8, with_keys=True)
    want = _edge_tiles(cols)
    with kta.HipMetricHandler(8, now=NOW) as h:
        b, _ = h.upload_batch(cols, with_keys=True)
        assert _headers(h, b, len(want)) == [(0, mode) for _, mode in want]
        back = h.download_batch(b, n)
        for k in METRIC:
            assert np.array_equal(back[k], cols[k]), k
        h.device_batch_free(b)


# ---- the scan ------------------------------------------------------------------------------------------------------
N_MIXED = 31 * T + 1023


@functools.lru_cache(maxsize=None)
def _mixed(P):
    """The mixed batch of the scan tests (never modified by them), its expected headers, and the records' oracle."""
    cols = _topic(N_MIXED, max(P - 20, 4))
    want = _edge_tiles(cols)
    for v in cols.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return cols, want


def _oracle(cols, with_keys=False):
    o = Oracle(NOW, with_keys)
    o.run_soa(cols)
    return o


def _raw_device_batch(cols):
    """The same records as a hand-built raw-layout device batch (plain device arrays, a zero-initialised kta_batch)."""
    import torch
    dev = {k: torch.from_numpy(np.array(cols[k])).cuda() for k in METRIC}
    torch.cuda.synchronize()
    b = N.KtaBatch()
    for k, t in dev.items():
        setattr(b, k, t.data_ptr())
    return b, dev


def _check_against_oracle(h, o, P):
    res, c = h.finish(allow_bad_partition=True)
    assert np.array_equal(c[:P], o.counters(P)), "per-partition counters differ"
    mm = kta.MessageMetrics(res, c, h.now)
    assert mm.earliest_message() == o.earliest() and mm.latest_message() == o.latest()
    assert mm.smallest_message() == o.get("smallest_message") and mm.largest_message() == o.get("largest_message")
    h.finish_device()
    return h.result_vector_host()


@pytest.mark.gpu
@pytest.mark.parametrize("scan_variant", [0, 16])
@pytest.mark.parametrize("P", [8, 300])
def test_scan_mixed_tiles_matches_oracle(P, scan_variant):
    cols, want = _mixed(P)
    n = N_MIXED
    with kta.HipMetricHandler(P, now=NOW) as h, kta.HipMetricHandler(P, now=NOW) as r:
        h.set_tuning(scan_variant=scan_variant)
        r.set_tuning(scan_variant=scan_variant)
        b, _ = h.upload_batch(cols)
        assert _headers(h, b, len(want)) == want
        rb, keep = _raw_device_batch(cols)
        # the whole batch, then a view at record 1500 that ends inside a tile
        for lo, m in ((0, n), (1500, 20 * T + 77)):
            h.reset()
            r.reset()
            h.submit_device(_view(b, lo), m, 0, which=1)
            r.submit_device(_view(rb, lo), m, 0, which=1)
            sub = {k: cols[k][lo:lo + m] for k in METRIC}
            vec = _check_against_oracle(h, _oracle(sub), P)
            assert np.array_equal(vec, _check_against_oracle(r, _oracle(sub), P))
        r.sync()
        del keep
        assert _headers(h, b, len(want)) == want      # a scan leaves the tiles as they are
        h.device_batch_free(b)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["analytics", "timeline"])
def test_analytics_and_timeline_match_raw_path(kind):
    P = 64
    cols, want = _mixed(P)
    n = N_MIXED
    kw = {"analytics": True} if kind == "analytics" else {}
    with kta.HipMetricHandler(P, now=NOW, **kw) as h, kta.HipMetricHandler(P, now=NOW, **kw) as r:
        if kind == "timeline":
            for x in (h, r):
                x.set_timeline(1_600_000_000_000 - 1_000_000, 60_000, 100)
        b, _ = h.upload_batch(cols)
        rb, keep = _raw_device_batch(cols)
        for lo, m in ((0, n), (1500, 20 * T + 77)):
            h.reset()
            r.reset()
            h.submit_device(_view(b, lo), m, 0, which=1)
            r.submit_device(_view(rb, lo), m, 0, which=1)
            if kind == "analytics":
                a, ra = h.analytics(), r.analytics()
                for k in ra:
                    assert np.array_equal(np.asarray(a[k]), np.asarray(ra[k])), k
            else:
                tl = h.timeline()
                assert tl[:, 0].sum() > 0 and np.array_equal(tl, r.timeline())
            sub = {k: cols[k][lo:lo + m] for k in METRIC}
            vec = _check_against_oracle(h, _oracle(sub), P)
            assert np.array_equal(vec, _check_against_oracle(r, _oracle(sub), P))
        r.sync()
        del keep
        h.device_batch_free(b)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5 * T + 3, 2 * T])
@pytest.mark.parametrize("wgs", [1, 2])
def test_one_workgroup_walks_several_tiles(wgs, n):
    """The prefetch ring's start and drain: tiles fewer than, equal to and slightly more than its depth per workgroup."""
    P = 8
    cols = _topic(n, P)
    _edge_tiles(cols)
    o = _oracle(cols)
    with kta.HipMetricHandler(P, now=NOW) as h:
        b, _ = h.upload_batch(cols)
        for variant in (0, 16):
            h.reset()
            h.set_tuning(scan_workgroups=wgs, scan_variant=variant)
            h.submit_device(b, n, 0, which=1)
            _check_against_oracle(h, o, P)
        h.device_batch_free(b)


# ---- producers -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_synth_fill_device_u16_matches_host():
    sp, _ = kta.synth_preset("c4")
    n = 1 << 20
    ref = kta.synth_fill_host(sp, 0, n)
    with kta.HipMetricHandler(256, now=NOW) as h:
        b = h.device_batch_alloc(n)
        h.synth_fill_device(sp, 0, n, b)
        assert set(_headers(h, b, n // T)) == {(1, 1)}
        back = h.download_batch(b, n)
        for k in METRIC:
            assert np.array_equal(back[k], ref[k]), k
        h.submit_device(b, n, 0, which=1)
        _check_against_oracle(h, _oracle(ref), 256)
        h.device_batch_free(b)
        # the same fill into a batch with key columns: plain i32 lengths
        kb = h.device_batch_alloc(n, key_bytes_capacity=80 * n)
        h.synth_fill_device(sp, 0, n, kb)
        assert set(_headers(h, kb, n // T)) == {(0, 1)}
        back = h.download_batch(kb, n)
        for k in METRIC:
            assert np.array_equal(back[k], ref[k]), k
        h.device_batch_free(kb)


def _kafka_blob():
    import kafka_format as K
    rng = np.random.default_rng(11)
    blob = bytearray()
    for i in range(25):
        recs = [(int(rng.integers(0, 1000)), bytes(rng.integers(0, 256, size=int(rng.integers(0, 30)), dtype=np.uint8)),
                 bytes(rng.integers(0, 256, size=int(rng.integers(0, 300)), dtype=np.uint8))) for _ in range(88)]
        blob += K.encode_batch(len(blob), recs, 1_600_000_000_000 + 1000 * i)
    return bytes(blob)


@pytest.mark.gpu
def test_writes_into_part_of_a_u16_batch():
    """The decode and the raw synth fill store the raw layout: into records [700, 2900) of a batch whose tiles held u16
    lengths they leave the records around them as they were."""
    from test_kafka_decode import index_host
    blob = _kafka_blob()
    lib = N.load()
    rc, descs, st = index_host(blob, 2)
    assert rc == N.KTA_OK
    n = st.n_records
    assert n == 2200
    total = 4 * T + 50
    sp, _ = kta.synth_preset("c4")
    ref = kta.synth_fill_host(sp, 0, total)
    with kta.HipMetricHandler(256, now=NOW) as h:
        buf_bytes = ((len(blob) + 127) & ~63) + st.inflate_bytes + 128
        blob_dev = h.device_batch_alloc(buf_bytes // 4 + 1)
        arr = np.frombuffer(blob + b"\0" * ((-len(blob)) % 4), dtype=np.uint8).copy()
        h._check(lib.kta_copy_to_device(h._ctx, blob_dev.partition, arr.ctypes.data, arr.nbytes))

        def decode(out):
            bad = C.c_uint64()
            h._check(lib.kta_kafka_decode_device(h._ctx, blob_dev.partition, len(blob), descs, st.n_batches, n,
                                                 C.byref(out), None, C.byref(bad)))
            return bad.value

        fresh = h.device_batch_alloc(n)
        assert decode(fresh) == 0
        want = h.download_batch(fresh, n)

        big = h.device_batch_alloc(total)
        h.synth_fill_device(sp, 0, total, big)
        assert set(_headers(h, big, 5)) == {(1, 1)}
        v = _view(big, 700)
        v.capacity = total - 700
        assert decode(v) == 0
        # tiles 0 and 2 are cut by the range, tile 1 lies inside it: all three are raw now; tiles 3 and 4 are untouched
        assert _headers(h, big, 5) == [(0, 0), (0, 0), (0, 0), (1, 1), (1, 1)]
        expect = {k: np.concatenate([ref[k][:700], want[k], ref[k][700 + n:]]) for k in METRIC}
        whole = h.download_batch(big, total)
        for k in METRIC:
            assert np.array_equal(whole[k], expect[k]), k
        h.submit_device(big, total, 0, which=1)
        _check_against_oracle(h, _oracle(expect), 256)

        # the raw synth fill at an offset that is no tile boundary: records [3 T + 10, 3 T + 10 + 500) of the same batch
        lo, m = 3 * T + 10, 500
        v = _view(big, lo)
        v.capacity = total - lo
        h.synth_fill_device(sp, 7777, m, v)
        new = kta.synth_fill_host(sp, 7777, m)
        assert _headers(h, big, 5) == [(0, 0), (0, 0), (0, 0), (0, 0), (1, 1)]
        for k in METRIC:
            expect[k][lo:lo + m] = new[k]
        whole = h.download_batch(big, total)
        for k in METRIC:
            assert np.array_equal(whole[k], expect[k]), k
        h.reset()
        h.submit_device(big, total, 0, which=1)
        _check_against_oracle(h, _oracle(expect), 256)
        for b in (fresh, big, blob_dev):
            h.device_batch_free(b)


@pytest.mark.gpu
@pytest.mark.parametrize("which", [3, 2])
def test_foreign_key_columns_on_a_keyless_view(which):
    """A -c context is handed a view whose metric columns lie in a keyless u16 batch and whose key columns are its own:
    the lengths of the view's tiles are widened before the alive-key pass reads them."""
    P, n = 16, 6 * T + 300
    cols = _topic(n, P, with_keys=True)
    lo, m = 1500, 3 * T + 11      # starts and ends inside tiles
    sub = {k: cols[k][lo:lo + m] for k in METRIC}
    sub["key_off"] = cols["key_off"][lo:lo + m] - cols["key_off"][lo]
    k0 = int(cols["key_off"][lo])
    sub["key_bytes"] = cols["key_bytes"][k0:]
    o = _oracle(sub, True)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW) as h:
        b, _ = h.upload_batch({k: cols[k] for k in METRIC})
        assert set(_headers(h, b, 7)) == {(1, 1)}
        keyed, _ = h.upload_batch(sub, with_keys=True)
        v = _view(b, lo)
        v.key_off, v.key_bytes = keyed.key_off, keyed.key_bytes
        h.submit_device(v, m, 0, which=which)
        if which == 2:
            h.submit_device(v, m, 0, which=1)
        res, c = h.finish(allow_bad_partition=True)
        assert res.alive_keys == o.alive_keys()
        assert np.array_equal(c[:P], o.counters(P))
        # the tiles of the view hold i32 lengths now, the others are as they were, and every record is still its own
        assert _headers(h, b, 7) == [(1, 1), (0, 1), (0, 1), (0, 1), (0, 1), (1, 1), (1, 1)]
        back = h.download_batch(b, n)
        for k in METRIC:
            assert np.array_equal(back[k], cols[k]), k
        for x in (b, keyed):
            h.device_batch_free(x)

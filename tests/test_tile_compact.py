"""The tile-compact device batch layout (include/kta_hip.h): what kta_device_batch_alloc returns, packed
by kta_batch_from_raw / kta_synth_fill_device, unpacked by kta_batch_to_raw, read by the scan and the fused pass.
Every result must be what the raw layout gives, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
from helpers import NOW
from oracle_c import Oracle

T = 1024                 # KTA_TILE_RECORDS
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
BASE_TS = 1_600_000_000_000


def test_abi_layout_constants():
    src = open(N.__file__.replace("_native.py", "../include/kta_hip.h")).read()
    assert "#define KTA_TILE_RECORDS 1024u" in src and N.KTA_TILE_RECORDS == T
    # the ctypes mirror ends with the layout fields: a zero-initialised batch is the raw layout
    names = [f[0] for f in N.KtaBatch._fields_]
    assert names[-3:] == ["tile_hdr", "layout", "reserved"]
    assert kta.KtaBatch().layout == 0 and C.sizeof(N.KtaBatch) == 7 * 8 + 2 * 8 + 8 + 8


def _edge_tiles(cols):
    """Overwrite whole tiles of a topic's columns with the edge cases of the compact form; returns the expected mode of
    every tile (1 compact, 0 raw)."""
    p, t = cols["partition"], cols["ts_ms"]
    n = len(p)
    modes = []
    cases = [
        lambda s: None,                                                           # the topic as generated
        lambda s: (t.__setitem__(s, BASE_TS), t.__setitem__(s.start + 5, BASE_TS + (1 << 31) - 1)),   # span 2^31 - 1
        lambda s: (t.__setitem__(s, BASE_TS), t.__setitem__(s.start + 5, BASE_TS + (1 << 31))),       # span 2^31: raw
        lambda s: p.__setitem__(s.start + 3, 65534),                              # largest compact id (bad for P)
        lambda s: p.__setitem__(s.start + 3, 65535),                              # the sentinel's value: raw
        lambda s: p.__setitem__(slice(s.start, s.start + 40), -1),                # a damaged batch's marker
        lambda s: p.__setitem__(s.start + 7, 1 << 20),                            # large id: raw
        lambda s: t.__setitem__(s, -1),                                           # no timestamp at all
        lambda s: t.__setitem__(slice(s.start, s.stop, 3), -1),                   # some missing
        lambda s: (t.__setitem__(s, BASE_TS - 5), t.__setitem__(s.start + 1, -1)),
    ]
    want = [1, 1, 0, 1, 0, 1, 0, 1, 1, 1]
    for k in range((n + T - 1) // T):
        s = slice(k * T, min(n, (k + 1) * T))
        c = k % len(cases)
        if s.stop - s.start < 8 and c:
            c = 0
        cases[c](s)
        modes.append(want[c])
    return modes


def _topic(n, P, with_keys=False, seed=2):
    sp, _ = kta.synth_preset("c2")
    sp.seed, sp.n_partitions = seed, P
    return kta.synth_fill_host(sp, 0, n, with_keys=with_keys)


def _tile_modes(h, b, ntiles):
    raw = np.empty(2 * ntiles, np.uint64)
    h._check(N.load().kta_copy_to_host(h._ctx, raw.ctypes.data, b.tile_hdr, raw.nbytes))
    return [int(x) & 0xFFFFFFFF for x in raw[1::2]]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1000, T, 10 * T + 37, 31 * T + 1023])
def test_upload_download_round_trip(n):
    cols = _topic(n, 8)
    modes = _edge_tiles(cols)
    with kta.HipMetricHandler(8, now=NOW) as h:
        b, _ = h.upload_batch(cols)
        assert b.layout == N.KTA_LAYOUT_TILE_COMPACT
        assert _tile_modes(h, b, len(modes)) == modes
        back = h.download_batch(b, n)
        for k in ("partition", "key_len", "val_len", "ts_ms"):
            assert np.array_equal(back[k], cols[k]), k
        # a view at a record offset (pointer arithmetic on the columns, raw layout field) reads the same records
        if n > 1500:
            v = kta.KtaBatch()
            for f, sz in (("partition", 4), ("key_len", 4), ("val_len", 4), ("ts_ms", 8)):
                setattr(v, f, getattr(b, f) + 1500 * sz)
            part = h.download_batch(v, n - 1500)
            for k in ("partition", "ts_ms"):
                assert np.array_equal(part[k], cols[k][1500:]), k
        h.device_batch_free(b)


@pytest.mark.gpu
def test_round_trip_extreme_values():
    """Arbitrary i32 / i64 columns come back exactly: raw tiles where the compact form cannot hold them."""
    rng = np.random.default_rng(5)
    n = 8 * T + 100
    cols = {"partition": rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64).astype(np.int32),
            "key_len": rng.integers(-1, 1 << 20, n).astype(np.int32),
            "val_len": rng.integers(-1, 1 << 30, n).astype(np.int32),
            "ts_ms": rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)}
    cols["ts_ms"][:4] = [I64_MIN, I64_MAX, -1, 0]
    # tiles 2..3: compact-able except for one extreme value each; tile 5: spans of exactly 2^31 - 1 around INT64_MIN
    cols["partition"][2 * T:6 * T] = rng.integers(0, 65535, 4 * T)
    cols["ts_ms"][2 * T:6 * T] = BASE_TS
    cols["ts_ms"][2 * T + 9] = I64_MAX
    cols["ts_ms"][3 * T + 9] = I64_MIN
    cols["ts_ms"][4 * T:5 * T] = -1
    cols["ts_ms"][5 * T:6 * T] = I64_MIN
    cols["ts_ms"][5 * T + 1] = I64_MIN + (1 << 31) - 1
    with kta.HipMetricHandler(4, now=NOW) as h:
        b, _ = h.upload_batch(cols)
        assert _tile_modes(h, b, 9)[2:6] == [0, 0, 1, 1]
        back = h.download_batch(b, n)
        for k in cols:
            assert np.array_equal(back[k], cols[k]), k
        h.device_batch_free(b)


def _oracle(cols, with_keys=False):
    o = Oracle(NOW, with_keys)
    o.run_soa(cols)
    return o


def _raw_vector(P, cols, **kw):
    """The counter vector of the same records through the staging ring (the raw layout)."""
    with kta.HipMetricHandler(P, now=NOW, **kw) as r:
        keys = (cols["key_off"], cols["key_bytes"]) if kw.get("count_alive_keys") else ()
        r.submit_columns(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"], *keys)
        r.finish_device()
        return r.result_vector_host()


def _check(h, o, P, cols, **kw):
    """Counters and extrema against the oracle, the whole counter vector against the raw layout's."""
    res, c = h.finish(allow_bad_partition=True)
    assert np.array_equal(c[:P], o.counters(P)), "per-partition counters differ"
    mm = kta.MessageMetrics(res, c, h.now)
    assert mm.earliest_message() == o.earliest() and mm.latest_message() == o.latest()
    assert mm.smallest_message() == o.get("smallest_message") and mm.largest_message() == o.get("largest_message")
    h.finish_device()
    assert np.array_equal(h.result_vector_host(), _raw_vector(P, cols, **kw))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("scan_variant", [0, 16])
def test_scan_mixed_tiles_matches_oracle(scan_variant):
    P, n = 300, 60 * T + 333
    cols = _topic(n, P - 20)
    _edge_tiles(cols)
    o = _oracle(cols)
    with kta.HipMetricHandler(P, now=NOW) as h:
        h.set_tuning(scan_variant=scan_variant)
        b, _ = h.upload_batch(cols)
        h.submit_device(b, n, 0, which=1)
        res = _check(h, o, P, cols)
        assert res.bad_partition_records == int(((cols["partition"] < 0) | (cols["partition"] >= P)).sum()) > 0
        # views that start and end inside tiles, and more workgroups than tiles
        # (the metric columns of a submitted view stay 16-byte aligned: a record offset that is a multiple of 4)
        for lo, m, wgs in ((4, n - 4, 0), (T + 4, 5 * T + 7, 0), (776, 3, 0), (2 * T - 4, n - 2 * T + 4, 4096)):
            h.reset()
            h.set_tuning(scan_workgroups=wgs, scan_variant=scan_variant)
            v = kta.KtaBatch()
            for f, sz in (("partition", 4), ("key_len", 4), ("val_len", 4), ("ts_ms", 8)):
                setattr(v, f, getattr(b, f) + lo * sz)
            h.submit_device(v, m, 0, which=1)
            sub = {k: cols[k][lo:lo + m] for k in ("partition", "key_len", "val_len", "ts_ms")}
            _check(h, _oracle(sub), P, sub)
        h.device_batch_free(b)


@pytest.mark.gpu
def test_analytics_mixed_tiles_match_raw_path():
    P, n = 64, 40 * T + 9
    cols = _topic(n, P)
    _edge_tiles(cols)
    with kta.HipMetricHandler(P, now=NOW, analytics=True) as h, kta.HipMetricHandler(P, now=NOW, analytics=True) as r:
        b, _ = h.upload_batch(cols)
        h.submit_device(b, n, 0, which=1)
        r.submit_columns(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"])   # the staging ring: raw
        a, ra = h.analytics(), r.analytics()
        for k in ra:
            assert np.array_equal(np.asarray(a[k]), np.asarray(ra[k])), k
        _check(h, _oracle(cols), P, cols, analytics=True)
        h.device_batch_free(b)


@pytest.mark.gpu
@pytest.mark.parametrize("state", ["bitset", "table"])
def test_both_handlers_fused_mixed_tiles(state):
    P, n = 128, (1 << 21) + 3 * T + 5
    cols = _topic(n, P, with_keys=True)
    _edge_tiles(cols)
    o = _oracle(cols, True)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, alive_table=(state == "table")) as h:
        if state == "table":
            h.set_tuning(alive_variant=13)
        b, _ = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, n, 0, which=3)
        info = (C.c_uint64 * 6)()
        h._check(N.load().kta_alive_pass_info(h._ctx, info))
        if state == "bitset":
            assert info[2] >= 1, "the batch did not take the fused pass"
        res = _check(h, o, P, cols, count_alive_keys=True, alive_table=(state == "table"))
        assert res.alive_keys == o.alive_keys()
        h.device_batch_free(b)


@pytest.mark.gpu
def test_synth_fill_device_compact_matches_host():
    sp, _ = kta.synth_preset("c4")
    n = 100 * T + 17
    with kta.HipMetricHandler(256, now=NOW) as h:
        b = h.device_batch_alloc(n)
        h.synth_fill_device(sp, 5, n, b)
        ref = kta.synth_fill_host(sp, 5, n)
        assert set(_tile_modes(h, b, (n + T - 1) // T)) == {1}      # config 4's timestamps and ids: every tile compact
        back = h.download_batch(b, n)
        for k in ("partition", "key_len", "val_len", "ts_ms"):
            assert np.array_equal(back[k], ref[k]), k
        h.submit_device(b, n, 0, which=1)
        _check(h, _oracle(ref), 256, ref)
        h.device_batch_free(b)


@pytest.mark.gpu
def test_decode_into_compact_batch():
    """The decode stores raw tiles: into a batch whose tiles were compact it gives what it gives into a fresh one, damaged
    (CRC-failed) batches' partition -1 included, and a view that starts inside a compact tile keeps the records before it."""
    import kafka_format as K
    from test_kafka_decode import _batches_of, index_host
    rng = np.random.default_rng(11)
    blob = bytearray()
    for i in range(40):
        recs = [(int(rng.integers(0, 1000)), bytes(rng.integers(0, 256, size=int(rng.integers(0, 30)), dtype=np.uint8)),
                 bytes(rng.integers(0, 256, size=int(rng.integers(0, 300)), dtype=np.uint8))) for _ in range(90)]
        blob += K.encode_batch(len(blob), recs, BASE_TS + 1000 * i)
    batches = _batches_of(bytes(blob))
    for bi in (3, 17):                       # corrupt two batches behind their CRC
        p, t = batches[bi]
        blob[p + 61 + (t - 61) // 2] ^= 0x40
    blob = bytes(blob)
    lib = N.load()
    rc, descs, st = index_host(blob, 2)
    assert rc == N.KTA_OK
    n = st.n_records
    sp, _ = kta.synth_preset("c4")
    with kta.HipMetricHandler(4, now=NOW) as h:
        h._check(lib.kta_kafka_set_check_crcs(h._ctx, 1))
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
        assert decode(fresh) == 2
        want = h.download_batch(fresh, n)
        assert (want["partition"] == -1).sum() == 180 and set(np.unique(want["partition"])) == {-1, 2}
        reused = h.device_batch_alloc(n + 3 * T)
        h.synth_fill_device(sp, 0, n + 3 * T, reused)
        assert decode(reused) == 2
        got = h.download_batch(reused, n)
        for k in ("partition", "key_len", "val_len", "ts_ms"):
            assert np.array_equal(got[k], want[k]), k
        # a view at record 700 of a compact batch: records 0..699 and those behind the decoded ones survive
        big = h.device_batch_alloc(n + 3 * T)
        h.synth_fill_device(sp, 0, n + 3 * T, big)
        ref = kta.synth_fill_host(sp, 0, n + 3 * T)
        v = kta.KtaBatch()
        for f, sz in (("partition", 4), ("key_len", 4), ("val_len", 4), ("ts_ms", 8)):
            setattr(v, f, getattr(big, f) + 700 * sz)
        v.capacity = n + 3 * T - 700
        assert decode(v) == 2
        whole = h.download_batch(big, n + 3 * T)
        for k in ("partition", "key_len", "val_len", "ts_ms"):
            assert np.array_equal(whole[k][:700], ref[k][:700]), k
            assert np.array_equal(whole[k][700:700 + n], want[k]), k
            assert np.array_equal(whole[k][700 + n:], ref[k][700 + n:]), k
        for b in (fresh, reused, big, blob_dev):
            h.device_batch_free(b)

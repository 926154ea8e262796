"""GPU tests of the size percentiles (KTA_FLAG_SIZE_QUANTILES: per partition a 464-bin histogram of the key, value and message
sizes; no reference counterpart), the vector bit-exact against the independent restatement in tests/size_quantiles_py.py and
the identities with the counter vector held in every test:

    sizes and partitions     sizes from both sides of every place where the bin rule changes, and -1; partitions -1 and P
    record counts, views     n = 1, 1023, 1024, 1025, 3 * 1024 + 5; a view from record 4 to n - 37
    slices                   P = 1; P = 7 with a forced slice of 3 (the last one partial); P = S and S + 1 for the plan's S
    tile forms in one batch  u16 lengths, i32 lengths (a 65535 beside u16 tiles), a raw tile, a keyed allocation, a
                             hand-built raw-layout batch whose last group of four is partial; the tile headers unchanged
    submission paths         kta_handle_message, host batches through the staging ring, the Kafka decode
    contention               4096 records of one partition and one size: one LDS add per instruction and word
    with the rest            kta_set_filter, a compaction replay, every opt-in pass at once, kta_reset, the refusals
    kta_exchange             the RCCL test double, 2 and 3 ranks (tests/test_size_quantiles_dist.py)
    kta-analyzer             kta.percentiles=1 on synthetic:// and dump://; nothing changes without the knob"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import hot_keys_py as HK
import key_sketch_py as KS
import partitioner_py as R
import size_quantiles_py as SQ
import timeline_py as T
import ts_order_py as TS
from helpers import NOW, random_cols

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
TS0 = 1_600_000_000_000
BOUNDARY = np.array([-1, 0, 1, 31, 32, 63, 64, 65534, 65535, 65536, 2**31 - 1], np.int64)   # (the i32 columns end at 2^31 - 1)
SMALL = np.array([-1, 0, 1, 31, 32, 63, 64, 300, 5000, 65534], np.int64)                    # what a u16 tile holds


def _cols(seed, n, P, pool=BOUNDARY):
    """sizes drawn from the pool, partitions from -1 .. P (both ends are bad), timestamps within a few minutes"""
    rng = np.random.default_rng(seed)
    return {"partition": rng.integers(-1, P + 1, size=n).astype(np.int32), "key_len": rng.choice(pool, size=n).astype(np.int32),
            "val_len": rng.choice(pool, size=n).astype(np.int32), "ts_ms": (TS0 + rng.integers(0, 300_000, size=n)).astype(np.int64)}


def _cut(cols, lo, hi):
    return {k: v[lo:hi] for k, v in cols.items() if k != "key_bytes"}


def _hold(h, want, P):
    """the live vector is `want`, and the identities hold against the context's own counter vector"""
    got = h.size_quantiles()
    assert np.array_equal(got["vector"], want)
    h.finish(allow_bad_partition=True)
    cv = h.result_vector_host()
    assert SQ.identities_hold(got["vector"], cv, P)
    assert np.array_equal(h.exchange_size_quantiles()["vector"], want)
    assert kta.render_size_percentiles(got["vector"], cv, P) == SQ.section(want, P)
    return got


def _headers(h, b, ntiles):
    """[(lens, mode)] of the batch's first tiles."""
    raw = np.empty(2 * ntiles, np.uint64)
    h._check(N.load().kta_copy_to_host(h._ctx, raw.ctypes.data, b.tile_hdr, raw.nbytes))
    return [(int(x) >> 32, int(x) & 0xFFFFFFFF) for x in raw[1::2]]


def _view(b, lo):
    v = N.KtaBatch()
    v.partition, v.key_len, v.val_len, v.ts_ms = b.partition + 4 * lo, b.key_len + 4 * lo, b.val_len + 4 * lo, b.ts_ms + 8 * lo
    return v


def test_the_input_exercises_every_bin_boundary_and_both_bad_partitions():
    P = 5
    cols = _cols(1, 3 * 1024 + 5, P)
    v = kta.split_size_quantiles(SQ.vector(cols, P), P)
    assert v["bad_partition"] > 0 and (cols["partition"] == -1).any() and (cols["partition"] == P).any()
    for size in SQ.BOUNDARY_SIZES[:-2]:
        assert v["key"][:, SQ.bin_of(size)].any() and v["value"][:, SQ.bin_of(size)].any()
    assert v["message"][:, SQ.bin_of(2**32 - 2)].any()                                 # 2 (2^31 - 1): the largest message
    assert v["keyed"] < v["records"] and v["alive"] < v["records"]


# ------------------------------------------------------------------------------------------ record counts, views
@pytest.mark.parametrize("pool", ["boundary", "small"])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 3 * 1024 + 5])
def test_record_counts_around_the_tile_and_a_view(n, pool):
    P = 5
    cols = _cols(10 + n, n, P, BOUNDARY if pool == "boundary" else SMALL)
    with kta.HipMetricHandler(P, now=NOW, size_quantiles=True) as h:
        b, nb = h.upload_batch(cols)
        h.submit_device(b, nb, 0, which=1)
        _hold(h, SQ.vector(cols, P), P)
        if n > 41:
            h.reset()
            h.submit_device(_view(b, 4), n - 37 - 4, 0, which=1)
            _hold(h, SQ.vector(_cut(cols, 4, n - 37), P), P)
        h.reset()
        h.submit_device(b, nb, 0, which=2)                                             # the alive-key handler alone: nothing
        assert not h.size_quantiles()["vector"].any()
        h.sync()
        h.device_batch_free(b)


# ------------------------------------------------------------------------------------------ slices
def _plan_slice():
    with kta.HipMetricHandler(64, now=NOW, size_quantiles=True) as h:
        return h.size_quantiles_info()["slice"]


@pytest.mark.parametrize("case", ["P1", "P7_forced3", "P_is_S", "P_is_S_plus_1", "P_is_64"])
def test_slices(case):
    S = _plan_slice()
    assert 12 <= S <= 28                                                               # a dozen partitions: one slice
    P, forced = {"P1": (1, 0), "P7_forced3": (7, 3), "P_is_S": (S, 0), "P_is_S_plus_1": (S + 1, 0), "P_is_64": (64, 0)}[case]
    cols = _cols(20 + P, 6000, P)
    with kta.HipMetricHandler(P, now=NOW, size_quantiles=True) as h:
        if forced:
            h.set_size_quantiles_slice(forced)
        b, nb = h.upload_batch(cols)
        h.submit_device(b, nb, 0, which=1)
        _hold(h, SQ.vector(cols, P), P)
        info = h.size_quantiles_info()
        want_s = min(forced or S, P)
        assert info["slice"] == want_s and info["slices"] == -(-P // want_s) and info["lds_bytes"] == want_s * 3 * 464 * 4
        assert info["threads"] in (256, 1024) and info["workgroups"] >= info["slices"] and info["lds_adds"] > 0
        if case == "P7_forced3":
            assert info["slices"] == 3
        if case == "P_is_S":
            assert info["slices"] == 1
        if case == "P_is_S_plus_1":
            assert info["slices"] == 2
        with pytest.raises(kta.KtaError, match="at most 28"):
            h.set_size_quantiles_slice(29)
        h.sync()
        h.device_batch_free(b)


# ------------------------------------------------------------------------------------------ tile forms
def test_every_tile_form_in_one_batch_and_the_headers_stay():
    P, n = 6, 5 * 1024 + 5
    cols = _cols(30, n, P, SMALL)
    cols["val_len"][1024 + 77] = 65535                                                  # tile 1: i32 lengths beside u16 tiles
    cols["ts_ms"][2 * 1024 + 5] = TS0 + 2**32                                           # tile 2: raw partitions and timestamps
    cols["partition"][2 * 1024:2 * 1024 + 40] = -1
    cols["key_len"][3 * 1024 + 9] = 70000                                               # tile 3: both
    cols["ts_ms"][3 * 1024 + 10] = TS0 + 2**33
    want = SQ.vector(cols, P)
    with kta.HipMetricHandler(P, now=NOW, size_quantiles=True) as h:
        b, nb = h.upload_batch(cols)                                                    # keyless: u16 lengths where they fit
        before = _headers(h, b, 6)
        assert before == [(1, 1), (0, 1), (1, 0), (0, 0), (1, 1), (1, 1)]               # (lens, mode) of the six tiles
        h.submit_device(b, nb, 0, which=1)
        _hold(h, want, P)
        assert _headers(h, b, 6) == before                                              # nothing was widened
        back = h.download_batch(b, nb)
        assert all(np.array_equal(back[k], cols[k]) for k in ("partition", "key_len", "val_len", "ts_ms"))
        h.reset()
        h.submit_device(_view(b, 1024 + 512), 3 * 1024, 0, which=1)                     # a view over four forms
        _hold(h, SQ.vector(_cut(cols, 1024 + 512, 4 * 1024 + 512), P), P)
        h.sync()
        h.device_batch_free(b)
        # a keyed allocation: i32 lengths in every tile (the pass reads no key)
        h.reset()
        keyed = dict(cols, key_off=np.zeros(n, np.uint32), key_bytes=np.zeros(16, np.uint8))
        b, nb = h.upload_batch(keyed, with_keys=True)
        assert all(lens == 0 for lens, _ in _headers(h, b, 6))
        h.submit_device(b, nb, 0, which=1)
        _hold(h, want, P)
        h.sync()
        h.device_batch_free(b)


def test_hand_built_raw_layout_batch_with_a_partial_last_group():
    import torch
    P, n = 4, 4 * 1024 + 3
    cols = _cols(31, n, P)
    dev = {k: torch.from_numpy(np.ascontiguousarray(cols[k])).cuda() for k in ("partition", "key_len", "val_len", "ts_ms")}
    torch.cuda.synchronize()
    b = N.KtaBatch()
    for k, t in dev.items():
        setattr(b, k, t.data_ptr())
    with kta.HipMetricHandler(P, now=NOW, size_quantiles=True) as h:
        h.submit_device(b, n, 0, which=1)
        _hold(h, SQ.vector(cols, P), P)
        h.sync()


# ------------------------------------------------------------------------------------------ submission paths
def test_handle_message_and_host_batches_through_the_staging_ring():
    P = 6
    rng = np.random.default_rng(40)
    cols = random_cols(rng, 20000, P, key_space=500, null_key=0.15, empty_key=0.05, tomb=0.3, max_key=70, max_val=70000)
    cols["partition"][rng.random(20000) < 0.02] = -1
    cols["partition"][rng.random(20000) < 0.02] = P
    with kta.HipMetricHandler(P, now=NOW, batch_capacity=1 << 12, size_quantiles=True) as h:
        h.submit_columns(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"])      # five host batches
        _hold(h, SQ.vector(cols, P), P)
        h.reset()
        kb = cols["key_bytes"].tobytes()
        for i in range(3000):
            kl = int(cols["key_len"][i])
            key = None if kl < 0 else kb[int(cols["key_off"][i]):int(cols["key_off"][i]) + kl]
            vl = int(cols["val_len"][i])
            h.handle_message(kta.Message(int(cols["partition"][i]), int(cols["ts_ms"][i]), key, None if vl < 0 else vl))
        _hold(h, SQ.vector(_cut(cols, 0, 3000), P), P)
        h.reset()
        h.replay_messages(cols)
        _hold(h, SQ.vector(cols, P), P)


def test_kafka_decode():
    from kafka_cases import random_record_set
    lib = N.load()
    rng = np.random.default_rng(42)
    P = 4
    blobs, part, klen, vlen = [], [], [], []
    for fetch in range(6):
        p = fetch % P
        blob, (pl, kl, vl, ts, keys), _ = random_record_set(rng, 50, partition=p, key_space=300, with_noise=False)
        blobs.append((blob, p))
        part += [p] * len(kl)
        klen += [int(x) for x in kl]
        vlen += [int(x) for x in vl]
    cols = {"partition": np.array(part, np.int32), "key_len": np.array(klen, np.int32), "val_len": np.array(vlen, np.int32)}
    with kta.HipMetricHandler(P, now=NOW, size_quantiles=True) as h:
        for blob, p in blobs:
            st = N.KtaKafkaIndexStats()
            h._check(lib.kta_kafka_consume(h._ctx, blob, len(blob), p, C.byref(st)))
        got = _hold(h, SQ.vector(cols, P), P)
        assert got["records"] == len(part) and got["keyed"] > 0 and got["alive"] > 0


# ------------------------------------------------------------------------------------------ contention
@pytest.mark.parametrize("P,p", [(1, 0), (40, 33)])
def test_contention_one_partition_one_size(P, p):
    """Lanes of one instruction that share a word add once: a full instruction of 64 equal records is one LDS add to its K
    word, one to its V word and one to its M word — 3 * records / 64 for 4096 records that fill whole instructions."""
    n = 4096
    cols = {"partition": np.full(n, p, np.int32), "key_len": np.full(n, 100, np.int32), "val_len": np.full(n, 1000, np.int32),
            "ts_ms": np.full(n, TS0, np.int64)}
    with kta.HipMetricHandler(P, now=NOW, size_quantiles=True) as h:
        b, nb = h.upload_batch(cols)
        h.submit_device(b, nb, 0, which=1)
        got = _hold(h, SQ.vector(cols, P), P)
        assert int(got["key"][p, SQ.bin_of(100)]) == int(got["value"][p, SQ.bin_of(1000)]) == int(got["message"][p, SQ.bin_of(1100)]) == n
        adds = h.size_quantiles_info()["lds_adds"]
        assert 0 < adds <= 3 * n // 64, adds
        h.sync()
        h.device_batch_free(b)


# ------------------------------------------------------------------------------------------ with the rest of the library
def test_filtered_context_bins_the_passing_records():
    P, n = 6, 20000
    cols = _cols(50, n, P)
    frm, to, parts = TS0 + 50_000, TS0 + 200_000, [0, 2, 3, 5]
    p, t = cols["partition"].astype(np.int64), cols["ts_ms"]
    keep = np.isin(p, parts) & (t >= frm) & (t < to)
    assert 1000 < int(keep.sum()) < n // 2
    taken = {k: np.ascontiguousarray(v[keep]) for k, v in cols.items()}
    with kta.HipMetricHandler(P, now=NOW, size_quantiles=True) as h, kta.HipMetricHandler(P, now=NOW, size_quantiles=True) as plain:
        h.set_filter(frm, to, parts)
        h.set_filter_slice(8192)
        b, nb = h.upload_batch(cols)
        h.submit_device(b, nb, 0, which=1)
        pb, pn = plain.upload_batch(taken)
        plain.submit_device(pb, pn, 0, which=1)
        want = SQ.vector(taken, P)
        assert np.array_equal(_hold(h, want, P)["vector"], _hold(plain, want, P)["vector"])
        for x, bb in ((h, b), (plain, pb)):
            x.sync()
            x.device_batch_free(bb)


def test_compaction_replay_bins_nothing():
    P = 5
    cols = random_cols(np.random.default_rng(51), 8000, P, key_space=900, null_key=0.1, tomb=0.3, max_key=40)
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True, size_quantiles=True) as h:
        b, nb = h.upload_batch(cols, with_keys=True)
        h.submit_device(b, nb, 0)
        want = SQ.vector(cols, P)
        _hold(h, want, P)
        with h.compaction_replay():
            h.submit_device(b, nb, 0)
            assert h.compaction()["replayed"] == nb
        _hold(h, want, P)
        h.sync()
        h.device_batch_free(b)


def test_every_opt_in_at_once_the_other_vectors_are_those_of_a_context_without_the_flag():
    P, n = 6, 30000
    cols = random_cols(np.random.default_rng(52), n, P, key_space=4000, null_key=0.1, empty_key=0.05, tomb=0.3, max_key=64)
    tl = (TS0 - 10**9, 50_000_000, 40)
    got = []
    for flag in (True, False):
        with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, batch_capacity=1 << 13, key_bytes_capacity=1 << 19, analytics=True,
                                  timeline=tl, key_sketch=True, hot_keys=True, ts_order=True, partitioner=True, size_quantiles=flag) as h:
            h.submit_columns(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"], cols["key_off"], cols["key_bytes"])
            res, c = h.finish()
            got.append([bytes(res), c, h.exchange_partitioner()["vector"], h.exchange_key_sketch(), h.exchange_timeline(),
                        h.exchange_ts_order()["vector"], h.exchange_hot_keys(),
                        str({k: np.asarray(v).tolist() for k, v in sorted(h.exchange_analytics().items())}).encode()])
            if flag:
                _hold(h, SQ.vector(cols, P), P)
    for a, b in zip(*got):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    assert np.array_equal(got[0][2], R.vector(cols, P, P)) and np.array_equal(got[0][3], KS.sketch(cols, P))
    assert np.array_equal(got[0][4], T.timeline_vector(cols, P, *tl))
    assert np.array_equal(got[0][5], TS.vector_of(P, cols["partition"], cols["ts_ms"]))
    assert np.array_equal(got[0][6].reshape(-1), np.asarray(HK.vector(cols, P)).reshape(-1))


def test_reset_the_calls_without_the_flag_and_the_limit():
    P = 4
    cols = _cols(53, 5000, P)
    with kta.HipMetricHandler(P, now=NOW, size_quantiles=True) as h:
        b, nb = h.upload_batch(cols)
        h.submit_device(b, nb, 0, which=1)
        _hold(h, SQ.vector(cols, P), P)
        h.reset()
        assert not h.size_quantiles()["vector"].any() and h.size_quantiles_info()["lds_adds"] == 0
        h.finish()
        assert not h.exchange_size_quantiles()["vector"].any()
        h.submit_device(b, nb, 0, which=1)
        _hold(h, SQ.vector(cols, P), P)
        h.sync()
        h.device_batch_free(b)
    with kta.HipMetricHandler(P, now=NOW) as h:
        for fn in (h.size_quantiles, h.exchange_size_quantiles, h.size_quantiles_result_vector, h.size_quantiles_info,
                   lambda: h.set_size_quantiles_slice(3)):
            with pytest.raises(kta.KtaError, match="KTA_FLAG_SIZE_QUANTILES") as e:
                fn()
            assert e.value.code == N.KTA_ERR_INVALID
    limit = kta.size_quantiles_max_partitions()
    with pytest.raises(kta.KtaError, match="KTA_FLAG_SIZE_QUANTILES admits at most %d" % limit):
        kta.HipMetricHandler(limit + 1, now=NOW, size_quantiles=True)


# ------------------------------------------------------------------------------------------ the CLI
def _cli(*args):
    return subprocess.run(["timeout", "-k", "10", "240", CLI, *args], capture_output=True, text=True, timeout=270)


def _normalise(text):
    text = re.sub(r"Scanning took: \d+ seconds", "Scanning took: 3 seconds", text)
    return re.sub(r"Estimated Msg/s: \d+", "Estimated Msg/s: 133", text)


def test_cli_section_on_synthetic_and_dump_and_nothing_without_the_knob(tmp_path):
    src, records = "synthetic://c2?records=60000", 60000
    sp, _ = kta.synth_preset("c2")
    from test_report_cli import write_dump
    cols = kta.synth_fill_host(sp, 0, records, with_keys=True)
    P = int(sp.n_partitions)
    want = SQ.section(SQ.vector(cols, P), P)
    dump = str(tmp_path / "c2.dump")
    write_dump(dump, cols, P)
    plain = _cli("-t", "c2", "-b", src)
    assert plain.returncode == 0 and "percentiles" not in plain.stdout, plain.stderr
    for source in (src, "dump://" + dump):
        base = plain if source == src else _cli("-t", "c2", "-b", source)
        one = _cli("-t", "c2", "-b", source, "--librdkafka", "kta.percentiles=1")
        assert base.returncode == 0 and one.returncode == 0, one.stderr
        at = one.stdout.index("Size percentiles per partition")
        assert one.stdout[at:] == want and _normalise(one.stdout[:at]) == _normalise(base.stdout)      # after the closing rule
        assert one.stdout[:at].endswith("=" * 120 + "\n")
        off = _cli("-t", "c2", "-b", source, "--librdkafka", "kta.percentiles=0")
        assert off.returncode == 0 and _normalise(off.stdout) == _normalise(base.stdout)
    # behind the analytics section, before the others; kta.per_message=1 feeds the same records
    others = "kta.analytics=1,kta.timeline=1h,kta.ts_order=1"
    without = _cli("-t", "c2", "-b", src, "--librdkafka", others)
    both = _cli("-t", "c2", "-b", src, "--librdkafka", others + ",kta.percentiles=1")
    assert without.returncode == 0 and both.returncode == 0, both.stderr
    at = both.stdout.index("Size percentiles per partition")
    assert both.stdout[at:at + len(want)] == want
    assert _normalise(both.stdout[:at] + both.stdout[at + len(want):]) == _normalise(without.stdout)
    assert "histogram" in both.stdout[:at].lower() and "Timeline" in both.stdout[at + len(want):]
    pm = _cli("-t", "c2", "-b", src, "--librdkafka", "kta.percentiles=1,kta.per_message=1,kta.batch=4096")
    assert pm.returncode == 0 and pm.stdout[pm.stdout.index("Size percentiles per partition"):] == want, pm.stderr

"""GPU tests of the compression what-if (KTA_FLAG_COMPRESS_WHATIF; no reference counterpart): the live vector that
kta_lz4_model accumulates from the batches of every decode call is np.array_equal to the host rule's
(kta_compress_whatif_host, itself held against tests/lz4_model_py.py by tests/test_lz4_model_host.py) and its identities hold.
The kernel's geometry: a wave (= workgroup) per batch, a lane per position of a stride of 64, blocks of 65536 bytes.

    section lengths   12, 13, 16, 64, 65, 75, 76, 77, 140; 4096; 65535 / 65536 / 65537; 65536 + 12 / + 13; 3 * 65536 + 5 — the
                      records of a batch take exactly that many bytes (a record takes at least 8: a section of 1 byte is no
                      batch the device decodes; the emulator and the host tests run it) —, one batch a blob and all in one blob
    laws              zeros; period 1, 2, 3 (offsets below 4); 24; 63, 64, 65 (the stride's seam); text; random
    crafted blocks    compress_whatif_inputs.crafted() as values of one record each: the blocks then lie inside a section
    codecs, failures  every codec on disk alone and all in one blob; a forged count, streams that do not inflate, a failed CRC
    partitions        alternating batch by batch in one call (a flush at every change); outside [0, P); a blob of one partition
    filter            a partition set; a window that cuts between batches (whole batches that overlap it)
    composition       kta_kafka_consume in chunks, kta_reset, the snapshot; a compaction replay; the flag off; two ranks over
                      tests/mock_rccl.cpp
    kta-analyzer      kta.compress_whatif=lz4 alone, behind the other sections and with kta.gpus=2,kta.oversubscribe=1"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import compress_whatif_inputs as I
import lz4_model_py as M
import payload_blobs as B
import record_batches_blobs as RB
from helpers import NOW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
GOLDEN = os.path.join(ROOT, "tests", "golden", "compress_whatif_cli_section.txt")
P = 4
T0 = B.T0
CODECS = [c for c in B.CODECS if c != "zstd" or RB.have_zstd()]
DEVICE_LENGTHS = [n for n in I.LENGTHS if n >= 12]


def _n_batches(blob):
    n, pos = 0, 0
    while pos + 61 <= len(blob):
        pos += 12 + int.from_bytes(blob[pos + 8:pos + 12], "big")
        n += 1
    return n


def _decode(h, blob, partition=0, partitions=None):
    """One kta_kafka_decode_device call over the whole blob.  partitions: one per descriptor, instead of `partition`."""
    lib, st = N.load(), N.KtaKafkaIndexStats()
    cap = max(_n_batches(blob), 1)
    descs = (N.KtaKafkaBatchDesc * cap)()
    assert lib.kta_kafka_index_host(blob, len(blob), partition, 0, 0, (len(blob) + 127) & ~63, descs, cap, C.byref(st)) == N.KTA_OK
    if partitions is not None:
        assert len(partitions) == st.n_batches
        for i, p in enumerate(partitions):
            descs[i].partition = p
    out = h.device_batch_alloc(max(st.n_records, 1), 0)
    buf_bytes = ((len(blob) + 127) & ~63) + st.inflate_bytes + 128
    dev = h.device_batch_alloc(buf_bytes // 4 + 1)                 # a column serves as the raw byte buffer
    arr = np.frombuffer(blob + b"\0" * ((-len(blob)) % 4), dtype=np.uint8).copy()
    h._check(lib.kta_copy_to_device(h._ctx, dev.partition, arr.ctypes.data, arr.nbytes))
    h._check(lib.kta_kafka_decode_device(h._ctx, dev.partition, len(blob), descs, st.n_batches, st.n_records, C.byref(out), None, None))
    vec = h.compress_whatif()["vector"].copy()                     # (waits for the compute stream before the buffers go)
    h.device_batch_free(out)
    h.device_batch_free(dev)
    return vec, st


def _consume(h, blob, partition):
    st = N.KtaKafkaIndexStats()
    h._check(N.load().kta_kafka_consume(h._ctx, blob, len(blob), partition, C.byref(st)))
    return st


def _holds(v, P_=P):
    bad = [n for n, ok in M.identities(v, P_) if not ok]
    assert not bad, bad
    assert kta.compress_whatif_identities(v, P_)


def _same(h, blob, partition=1):
    """the blob through one decode call of a context that is reset first: the vector equals the host rule's, bit for bit"""
    h.reset()
    got, st = _decode(h, blob, partition)
    want = kta.compress_whatif_host(blob, partition, P)
    assert np.array_equal(got, want), (np.flatnonzero(got != want)[:20], got[got != want][:8], want[got != want][:8])
    _holds(got)
    return got, st


@pytest.fixture(scope="module")
def ctx():
    with kta.HipMetricHandler(P, now=NOW, compress_whatif=True) as h:
        yield h


# ------------------------------------------------------------------------------------------ lengths, laws, crafted blocks
@pytest.mark.parametrize("name", I.LAWS)
def test_every_section_length_of_a_law_single_batch_and_multi_batch(ctx, name):
    batches = []
    for k, n in enumerate(DEVICE_LENGTHS):
        b, raw = I.batch(n, name, seed=n, base_offset=2 * k)
        assert len(raw) == n                                                         # the payload length, computed and asserted
        got, st = _same(ctx, b)
        assert st.n_batches == 1 and got[M.PW + M.RAW] == n and got[M.PW + M.BLOCKS] == (n + 65535) // 65536
        batches.append((b, raw))
    blob, _ = B.join(batches)
    got, st = _same(ctx, blob, partition=3)
    assert st.n_batches == len(DEVICE_LENGTHS) == got[3 * M.PW + M.BATCHES] and got[3 * M.PW + M.RAW] == sum(DEVICE_LENGTHS)
    if name in ("zeros", "period3", "period24"):
        assert got[3 * M.PW + M.MODEL] < got[3 * M.PW + M.RAW] // 20                  # long matches all the way
    if name == "random":
        assert got[3 * M.PW + M.STORED] == got[3 * M.PW + M.BLOCKS]


def test_crafted_blocks_inside_a_records_section(ctx):
    blocks = I.crafted()
    batches = []
    for k, (name, (block, _)) in enumerate(blocks.items()):
        recs = [B.record(0, block[:65000], key=None)]
        batches.append(B.batch(k, recs))
        _same(ctx, batches[-1][0])
    info0 = ctx.compress_whatif_info()
    got, st = _same(ctx, B.join(batches)[0], partition=0)
    info = ctx.compress_whatif_info()
    assert info["launches"] == info0["launches"] + 1 and info["batches"] == info0["batches"] + len(blocks) and info["workgroups"] == len(blocks)
    assert np.array_equal(got, M.restate([(0, None, len(b), raw) for b, raw in batches], P)) and got[M.SEQUENCES] > 0   # the twin as well


# ------------------------------------------------------------------------------------------ codecs, failures
def _batches(compression, seed=0, n=6, base_ts=T0, step_ms=0):
    out, off = [], 0
    for b in range(n):
        recs = [B.record(i, I.text(40 + 30 * ((b + i) % 5), seed + 10 * b + i), key=b"k%d" % i) for i in range(8 + b)]
        comp = compression[b % len(compression)] if isinstance(compression, (list, tuple)) else compression
        out.append(B.batch(off, recs, compression=comp, base_ts=base_ts + step_ms * b))
        off += len(recs)
    return out


@pytest.mark.parametrize("comp", CODECS + ["all"])
def test_each_codec_on_disk(ctx, comp):
    bs = _batches(CODECS if comp == "all" else comp, seed=3, n=10 if comp == "all" else 6)
    got, _ = _same(ctx, B.join(bs)[0], partition=2)
    s = kta.split_compress_whatif(got, P)
    plain = kta.split_compress_whatif(kta.compress_whatif_host(B.join(_batches(None, seed=3, n=len(bs)))[0], 2, P), P)
    same = [k for k in range(M.PW) if k != M.NOW]
    assert np.array_equal(s["partitions"][2][same], plain["partitions"][2][same])     # the same records: the same model, whatever lies on disk
    if comp != "all":
        assert s["codecs"][M.CODEC_OF[comp], 0] == 6 and s["codecs"][:, 0].sum() == 6
    else:
        assert (s["codecs"][[M.CODEC_OF[c] for c in CODECS], 0] == 2).all()


def test_forged_counts_and_corrupt_streams_add_nothing(ctx):
    good = _batches(None, n=2) + _batches("snappy", seed=4, n=1)
    out = [good[0], (RB.patch(_batches(None, seed=7, n=1)[0][0], count=1000), b"")]    # a forged count: bad framing
    for comp in [c for c in CODECS if c]:                                              # a stream that does not inflate
        b, raw = _batches(comp, seed=8, n=1)[0]
        out.append((RB.corrupt_stream(b, comp), raw))
    out += good[1:]
    got, st = _same(ctx, B.join(out)[0])
    assert st.n_batches == len(out) and got[M.PW + M.BATCHES] == 3
    assert np.array_equal(got, M.restate([(1, c, len(b), raw) for c, (b, raw) in zip((None, None, "snappy"), good)], P))


def test_a_failed_batch_under_check_crcs_adds_nothing():
    (g0, r0), (b, _), (g1, r1) = _batches(None, n=3)
    bad = b[:70] + bytes([b[70] ^ 1]) + b[71:]                                      # one bit inside the CRC's range
    with kta.HipMetricHandler(P, now=NOW, compress_whatif=True) as h:
        h._check(N.load().kta_kafka_set_check_crcs(h._ctx, 1))
        got, st = _decode(h, g0 + bad + g1, 0)
    assert st.n_batches == 3 and got[M.BATCHES] == 2
    assert np.array_equal(got, M.restate([(0, None, len(g0), r0), (0, None, len(g1), r1)], P))
    assert np.array_equal(got, kta.compress_whatif_host(g0 + g1, 0, P))


# ------------------------------------------------------------------------------------------ partitions, the filter
def test_partitions_alternating_batch_by_batch_and_outside_the_range(ctx):
    bs = _batches(CODECS, seed=11, n=24)
    blob, _ = B.join(bs)
    parts = [(i % 2) * 3 if i < 12 else (i * 5 + i // 6) % (P + 2) - 1 for i in range(24)]   # 0 3 0 3 ..., then all of -1 .. P
    want = np.zeros(M.words(P), np.uint64)
    for (b, _), p in zip(bs, parts):
        kta.compress_whatif_host(b, p, P, want)
    ctx.reset()
    got, _ = _decode(ctx, blob, partitions=parts)
    assert np.array_equal(got, want) and want[M.BATCHES:M.PW * P:M.PW].all()
    assert int(got[M.BATCHES:M.PW * P:M.PW].sum()) == sum(1 for p in parts if 0 <= p < P) < 24
    _holds(got)


def test_a_blob_of_one_partition_through_few_workgroups(ctx):
    blob, _ = B.join(_batches(None, seed=13, n=40))
    got, _ = _same(ctx, blob, partition=2)
    assert got[2 * M.PW + M.BATCHES] == 40 and not got[:2 * M.PW].any()


@pytest.mark.parametrize("flt", [(None, None, (0, 2)), (None, None, (3,)), (T0 + 2000, None, None), (None, T0 + 2000, None), (T0 + 1500, T0 + 3500, (1, 2))])
def test_a_partition_set_and_a_window_that_cuts_between_batches(flt):
    sets = [(p, _batches(CODECS[:3], seed=20 + p, n=6, step_ms=1000)) for p in range(P)]    # batch b of a partition: all records at T0 + 1000 b
    lo, hi, parts = flt
    want, whole = np.zeros(M.words(P), np.uint64), np.zeros(M.words(P), np.uint64)
    for p, bs in sets:
        for k, (b, _) in enumerate(bs):
            ts = T0 + 1000 * k
            kta.compress_whatif_host(b, p, P, whole)
            if (parts is None or p in parts) and (hi is None or ts < hi) and (lo is None or ts >= lo):
                kta.compress_whatif_host(b, p, P, want)
    with kta.HipMetricHandler(P, now=NOW, compress_whatif=True) as h:
        h.set_filter(*flt)
        for p, bs in sets:
            _consume(h, B.join(bs)[0], p)
        got = h.compress_whatif()["vector"]
    assert np.array_equal(got, want) and 0 < want[M.BATCHES:M.PW * P:M.PW].sum() < whole[M.BATCHES:M.PW * P:M.PW].sum()
    _holds(got)


# ------------------------------------------------------------------------------------------ submission paths
def test_consume_in_chunks_accumulates_resets_and_snapshots():
    blob, _ = B.join(_batches(CODECS[:3], seed=31, n=120))
    other, _ = B.join(_batches(None, seed=32, n=10))
    want = kta.compress_whatif_host(blob, 2, P)
    with kta.HipMetricHandler(P, now=NOW, compress_whatif=True) as h:
        h._check(N.load().kta_kafka_configure(h._ctx, 16384, 3))                    # a few batches per staging blob
        h.set_timing(True)
        st = _consume(h, blob, 2)
        info = h.compress_whatif_info()
        assert st.n_batches == 120 == info["batches"] and info["launches"] > 5 and info["timed"] == info["launches"] and info["kernel_ms"] > 0
        assert np.array_equal(h.compress_whatif()["vector"], want)
        h.finish()
        assert np.array_equal(h.exchange_compress_whatif()["vector"], want)
        _consume(h, other, 0)                                                       # a second call accumulates
        both = kta.compress_whatif_host(other, 0, P, want.copy())
        assert np.array_equal(h.compress_whatif()["vector"], both)
        assert np.array_equal(h.exchange_compress_whatif()["vector"], want)         # the snapshot is finish()'s
        h.reset()
        assert not h.compress_whatif()["vector"].any()
        _consume(h, other, 0)
        assert np.array_equal(h.compress_whatif()["vector"], kta.compress_whatif_host(other, 0, P))


def test_a_compaction_replay_counts_nothing_twice():
    blob, _ = B.join(_batches(None, seed=41, n=30))
    with kta.HipMetricHandler(P, count_alive_keys=True, now=NOW, compaction=True, compress_whatif=True) as h:
        _consume(h, blob, 1)
        h.finish()
        launches = h.compress_whatif_info()["launches"]
        with h.compaction_replay():
            _consume(h, blob, 1)
        assert h.compress_whatif_info()["launches"] == launches                     # the pass is skipped
        assert np.array_equal(h.compress_whatif()["vector"], kta.compress_whatif_host(blob, 1, P))


OTHERS = dict(record_batches=True, payload=True, header_names=True, value_bytes=True)
OTHER_SECTIONS = ("get_record_batches", "get_payload", "header_names", "value_bytes")
OTHER_INFOS = ("payload_info", "header_names_info", "value_bytes_info")


def _flat(x):
    if isinstance(x, dict) and "vector" in x:
        return np.asarray(x["vector"]).reshape(-1)
    if isinstance(x, dict):
        return np.concatenate([np.asarray(x[k]).reshape(-1).view(np.uint64) for k in sorted(x)])
    return np.asarray(x).reshape(-1)


def test_flag_off_nothing_is_launched_and_the_other_sections_are_untouched():
    sets = [(B.join(_batches(CODECS[:3], seed=50 + p, n=12))[0], p) for p in range(P)]
    state = {}
    for on in (False, True):
        with kta.HipMetricHandler(P, now=NOW, compress_whatif=on, **OTHERS) as h:
            for blob, p in sets:
                _consume(h, blob, p)
            h.finish()
            state[on] = {s: _flat(getattr(h, s)()).copy() for s in OTHER_SECTIONS}
            state[on]["counters"] = h.result_vector_host()
            state[on].update({i: np.array([getattr(h, i)()[k] for k in ("launches", "batches", "workgroups")]) for i in OTHER_INFOS})
            if on:
                want = np.zeros(M.words(P), np.uint64)
                for blob, p in sets:
                    kta.compress_whatif_host(blob, p, P, want)
                assert np.array_equal(h.compress_whatif()["vector"], want)
                assert h.compress_whatif_info()["launches"] == state[on]["value_bytes_info"][0] > 0
            else:
                for call in (h.compress_whatif, h.exchange_compress_whatif, h.compress_whatif_info, h.compress_whatif_vector, h.compress_whatif_result_vector):
                    with pytest.raises(kta.KtaError, match="KTA_FLAG_COMPRESS_WHATIF"):
                        call()
    for name in state[True]:
        assert np.array_equal(state[True][name], state[False][name]), name


# ------------------------------------------------------------------------------------------ two ranks
@pytest.fixture(scope="module")
def mock_rccl(tmp_path_factory):
    lib = tmp_path_factory.mktemp("mock") / "libmock_rccl.so"
    r = subprocess.run(["timeout", "-k", "10", "600", "/opt/rocm/bin/hipcc", "-O1", "-shared", "-fPIC", "-std=c++17",
                        os.path.join(ROOT, "tests", "mock_rccl.cpp"), "-o", str(lib), "-lrt", "-lpthread"],
                       capture_output=True, text=True, timeout=660)
    assert r.returncode == 0, r.stderr[-2000:]
    return str(lib)


_EXCHANGE_WORKER = r'''
import ctypes as C, os, sys, threading
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import compress_whatif_inputs as I
import lz4_model_py as M
import payload_blobs as B
from helpers import NOW

P, nranks = 5, 2
sets = []
for p in range(P):
    bs = [B.batch(3 * b, [B.record(i, I.text(60 + 25 * i + 7 * p, 9 * p + b), key=b"k") for i in range(3)], compression=(None, "snappy", "lz4")[b % 3]) for b in range(4 + p)]
    sets.append((B.join(bs)[0], p))
def host(which):
    v = np.zeros(M.words(P), np.uint64)
    for blob, p in which:
        kta.compress_whatif_host(blob, p, P, v)
    return v
want = host(sets)
assert want[M.MODEL:M.PW * P:M.PW].all() and all(ok for _, ok in M.identities(want, P))
uid = kta.HipMetricHandler.comm_unique_id()
def run(rank):
    try:
        h = kta.HipMetricHandler(P, now=NOW, compress_whatif=True)
        h.comm_create(nranks, rank, uid)
        mine = [s for s in sets if s[1] % nranks == rank]
        for blob, p in mine:
            st = N.KtaKafkaIndexStats()
            h._check(N.load().kta_kafka_consume(h._ctx, blob, len(blob), p, C.byref(st)))
        h.exchange()
        assert np.array_equal(h.exchange_compress_whatif()["vector"], want), (rank, "exchanged")
        own = host(mine)
        assert np.array_equal(h.compress_whatif()["vector"], own), (rank, "own")
        other = host([s for s in sets if s[1] % nranks != rank])
        assert np.array_equal(kta.merge_compress_whatif(own.copy(), other, P), want), (rank, "merged")
        h.exchange()
        assert np.array_equal(h.exchange_compress_whatif()["vector"], want), (rank, "again")
        h.sync()
        h.comm_destroy(); h.close()
    except BaseException as e:
        print("rank %d: %r" % (rank, e), file=sys.stderr, flush=True)
        os._exit(2)        # the other rank would wait in its collective for ever
ts = [threading.Thread(target=run, args=(r,)) for r in range(nranks)]
[t.start() for t in ts]; [t.join() for t in ts]
print("OK")
'''


def test_exchange_on_two_ranks_ends_with_the_unsharded_vector(tmp_path, mock_rccl):
    script = tmp_path / "exchange_worker.py"
    script.write_text(_EXCHANGE_WORKER)
    env = dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=330, env=env)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.stdout[-2000:], r.stderr[-3000:])


# ------------------------------------------------------------------------------------------ the CLI
def _cli(*args, env=None):
    return subprocess.run(["timeout", "-k", "10", "240", CLI, *args], capture_output=True, text=True, timeout=270, env=env)


def _normalise(text):
    text = re.sub(r"Scanning took: \d+ seconds", "Scanning took: 3 seconds", text)
    return re.sub(r"Estimated Msg/s: \d+", "Estimated Msg/s: 133", text)


def cli_topic():
    """[(blob, partition)] of the topic the CLI's golden section was rendered from"""
    return [(B.join(_batches([None, "snappy", "lz4", "gzip"], seed=60 + p, n=10 + 4 * p))[0], p) for p in range(2)]


def test_cli_prints_the_section_alone_and_on_two_ranks(tmp_path, mock_rccl):
    files, v = [], np.zeros(M.words(2), np.uint64)
    for blob, p in cli_topic():
        path = tmp_path / ("%d.log" % p)
        path.write_bytes(blob)
        files.append(str(path))
        kta.compress_whatif_host(blob, p, 2, v)
    src = "segment://" + ",".join(files)
    want = open(GOLDEN).read()
    assert want == kta.render_compress_whatif(v, 2)
    plain = _cli("-t", "seg", "-b", src)
    one = _cli("-t", "seg", "-b", src, "--librdkafka", "kta.compress_whatif=lz4")
    assert plain.returncode == 0 and one.returncode == 0, one.stderr
    assert "Compression what-if:" not in plain.stdout
    at = one.stdout.index("Compression what-if: what compression.type=lz4")
    assert one.stdout[at:] == want and _normalise(one.stdout[:at]) == _normalise(plain.stdout)   # the default output stays as it is
    both = _cli("-t", "seg", "-b", src, "--librdkafka", "kta.compress_whatif=lz4,kta.value_bytes=1,kta.payload=1")
    assert both.returncode == 0, both.stderr
    assert both.stdout.endswith(want) and both.stdout.index("Payload: value formats") < both.stdout.index("Value bytes:") < both.stdout.index("Compression what-if:")
    # two ranks, both on the one reachable GPU, RCCL replaced by tests/mock_rccl.cpp (real RCCL refuses two ranks on one device)
    ranks = _cli("-t", "seg", "-b", src, "--librdkafka", "kta.compress_whatif=lz4,kta.gpus=2,kta.oversubscribe=1", env=dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl))
    assert ranks.returncode == 0, ranks.stderr
    assert ranks.stdout.endswith(want)
    flt = _cli("-t", "seg", "-b", src, "-c", "--librdkafka", "kta.compress_whatif=lz4,kta.partitions=1")
    assert flt.returncode == 0, flt.stderr
    only1 = np.zeros(M.words(2), np.uint64)
    kta.compress_whatif_host(cli_topic()[1][0], 1, 2, only1)
    assert kta.render_compress_whatif(only1, 2) in flt.stdout

"""The value-byte section (KTA_FLAG_VALUE_BYTES) without a GPU: the host rule (kta_value_bytes_host) against the restatement
(tests/value_bytes_py.py: np.bincount of every value, the value against itself shifted by one) on blobs of every codec and on
the boundary blobs of tests/value_bytes_blobs.py; the identities, each broken by one word, with and without a payload and a
counter vector; the summary against the restatement, H0 to 1e-12 relative (256 double terms: each term and the sum carry a few
ulps of 2^-53, far inside it); the rendered section against a golden text whose decimals lie away from a rounding tie; the
merge; the exports; the CLI's refusals that need no device; the torch twin of the exchange over gloo; and the rule's own source
(csrc/kta_value_bytes.h) run natively under AddressSanitizer + UBSan (tests/native/value_bytes_check.cpp, a program of its
own)."""
import os
import re
import socket
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
from kafka_topic_analyzer_amd import distributed
import payload_blobs as B
import payload_py as R
import value_bytes_blobs as VB
import value_bytes_py as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
CSRC = os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "value_bytes_section.txt")
NEW_EXPORTS = ("kta_get_value_bytes", "kta_exchange_value_bytes", "kta_value_bytes_result_vector", "kta_value_bytes_vector", "kta_merge_value_bytes",
               "kta_value_bytes_identities", "kta_value_bytes_summary", "kta_value_bytes_host", "kta_render_value_bytes")
P = 4


def _holds(v, payload=None, counters=None, P_=P):
    bad = [n for n, ok in V.identities(v, P_, payload, counters) if not ok]
    assert not bad, bad
    assert kta.value_bytes_identities(v, P_, payload, counters)


def _same_summary(words):
    got, want = kta.value_bytes_summary(words), V.summary(words)
    assert {k: v for k, v in got.items() if k != "entropy_bits"} == {k: v for k, v in want.items() if k != "entropy_bits"}
    assert abs(got["entropy_bits"] - want["entropy_bits"]) <= 1e-12 * want["entropy_bits"]
    return got


def _lcg_bytes(n, seed=1):
    """n pseudo-random bytes of a generator of its own (the same on every machine)"""
    out, x = bytearray(n), seed
    for i in range(n):
        x = (x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        out[i] = x >> 56
    return bytes(out)


# ------------------------------------------------------------------------------------------ 1. the rule
def test_host_rule_equals_the_restatement_on_blobs_of_every_codec():
    acc, pl, sets = None, np.zeros(R.words(P), np.uint64), []
    for part, comp in enumerate((None, "gzip", "snappy", "lz4", "zstd", B.CODECS)):
        blob, raw = B.mixed(7, 40, seed=part, compression=comp)
        acc = kta.value_bytes_host(blob, part % P, P, vec=acc)
        kta.payload_host(blob, part % P, P, vec=pl)
        sets.append((blob, part % P, raw, set()))
    want = V.restate(sets, P)
    assert np.array_equal(acc, want) and want[V.REPEATS::V.PW].all() and want[V.RECORDS::V.PW].sum() > want[V.VALUES::V.PW].sum()
    _holds(acc)
    _holds(acc, pl)                                                                  # the identities with the payload vector of the same run
    assert not kta.value_bytes_host(sets[0][0], -1, P).any() and not kta.value_bytes_host(sets[0][0], P, P).any()   # outside [0, P)
    split = kta.split_value_bytes(acc, P)
    assert split["partitions"].shape == (P, 264) and len(split["summaries"]) == P and split["topic"]["bytes"] == int(want[V.BYTES::V.PW].sum())


def test_host_rule_on_the_boundary_blobs():
    for blob, raw in (VB.lengths(), VB.astride()[:2], VB.alignments()[:2], VB.every_byte_at_every_position()[:2], VB.one_byte_in_every_lane(0xFF),
                      VB.seams()[:2], VB.neighbours_outside_the_value()):
        got = kta.value_bytes_host(blob, 2, P)
        assert np.array_equal(got, V.restate([(blob, 2, raw, set())], P))
        _holds(got)
    blob, raw, at = VB.seams()
    assert V.restate([(blob, 0, raw, set())], 1)[V.REPEATS] == len(at)
    blob, raw = VB.neighbours_outside_the_value()
    assert V.restate([(blob, 0, raw, set())], 1)[V.REPEATS] == 1                      # the one pair inside a value
    (const, const_raw), (alt, alt_raw) = VB.constant_and_alternating()
    w = kta.value_bytes_host(const, 0, 1)
    assert w[V.REPEATS] == w[V.BYTES] - w[V.VALUES] and w[V.VALUES] == 3
    w = kta.value_bytes_host(alt, 0, 1)
    assert w[V.REPEATS] == 0 and w[V.BYTES] == 2 * (500 + 501)


# ------------------------------------------------------------------------------------------ 2. the summary
def _golden():
    """four partitions: JSON-like text, 80 035 pseudo-random bytes, zero-padded binary records, nothing"""
    v = np.zeros(V.words(P), np.uint64)
    for i in range(300):
        V.add_value(v[:V.PW], b'{"id":%d,"name":"user-%d","tags":["a","b"],"ok":true}\n' % (i * 37, i % 11))
    V.add_value(v[:V.PW], None)
    for i in range(5):
        V.add_value(v[V.PW:2 * V.PW], _lcg_bytes(16001 + 3 * i, seed=i + 1))
    for i in range(40):
        V.add_value(v[2 * V.PW:3 * V.PW], bytes([i, 0xC3, 0x80 + i]) + b"\x00" * 29 + b"name%02d" % i)
    V.add_value(v[3 * V.PW:], b"")
    return v


def test_summary_equals_the_restatement():
    v = _golden()
    s = [_same_summary(v[V.PW * p:V.PW * (p + 1)]) for p in range(P)] + [_same_summary(V.topic(v, P))]
    assert [x["class"] for x in s] == ["text", "dense", "binary", "none", "dense"]
    assert s[1]["entropy_bits"] > 7.99 and s[1]["distinct"] == 256 and s[1]["floor_bytes"] < 80035
    assert s[2]["top_byte"] == 0 and s[2]["zero"] >= 40 * 29 and s[2]["repeats"] >= 40 * 28 and s[0]["high"] == 0
    assert s[3] == dict(s[3], bytes=0, records=1, values=0, entropy_bits=0.0, floor_bytes=0, distinct=0, top_count=0)
    for blob, raw in (B.mixed(9, 20, seed=3), VB.lengths((1, 2, 3, 17, 3073))):
        got = kta.value_bytes_host(blob, 1, P)
        _same_summary(got[V.PW:2 * V.PW])
    one = np.zeros(V.PW, np.uint64)                                                  # a single bin: H0 = 0, not -0 or a NaN
    one[0x41], one[V.BYTES], one[V.VALUES], one[V.RECORDS] = 7, 7, 1, 1
    assert _same_summary(one)["entropy_bits"] == 0.0
    tie = np.zeros(V.PW, np.uint64)                                                  # a tie goes to the lowest byte
    tie[9], tie[200], tie[V.BYTES] = 5, 5, 10
    assert _same_summary(tie)["top_byte"] == 9
    edge = np.zeros(V.PW, np.uint64)                                                 # 95 % printable exactly is text; below it is not
    edge[0x20], edge[0x7F], edge[V.BYTES] = 95, 5, 100
    assert _same_summary(edge)["class"] == "text"
    edge[0x20], edge[0x7F] = 94, 6
    assert _same_summary(edge)["class"] == "binary"
    with pytest.raises(ValueError):
        kta.value_bytes_summary(v[:V.PW - 1])


def test_dense_needs_65536_bytes_and_seven_and_a_half_bits():
    w = np.zeros(V.PW, np.uint64)
    w[:256], w[V.BYTES] = 255, 255 * 256
    assert _same_summary(w)["class"] == "binary" and kta.value_bytes_summary(w)["entropy_bits"] == 8.0
    w[:256], w[V.BYTES] = 256, 65536
    assert _same_summary(w)["class"] == "dense" and kta.value_bytes_summary(w)["floor_bytes"] == 65536
    w[:256], w[V.BYTES] = 0, 181 * 400
    w[70:251] = 400                                                                  # 181 bytes alike: log2(181) = 7.4998 bits
    assert 7.49 < _same_summary(w)["entropy_bits"] < 7.5 and kta.value_bytes_summary(w)["class"] == "binary"


# ------------------------------------------------------------------------------------------ 3. golden, identities, merge
def test_rendered_section_matches_the_golden_text():
    v = _golden()
    _holds(v)
    assert V.decimals_clear_of_a_tie(v, P)                                           # no printed figure within 1e-6 of x.xx5
    text = kta.render_value_bytes(v, P)
    assert text == open(GOLDEN).read() == V.section(v, P)
    lines = text.splitlines()
    assert "kta.value_bytes=1; not part of the reference report" in lines[0] and text.endswith("=" * 120 + "\n")
    assert "heuristic" in lines[-3] and "LZ matching" in lines[-2] and "entropy coder alone" in lines[-2]
    assert [re.split(r"\s*\|\s*", l)[-2] for l in lines if l.startswith("| ")] == ["Class", "text", "dense", "binary", "none", "dense"]
    assert text.count("n/a") == 7                                                    # the partition without bytes


def test_identities_each_broken_by_one_word():
    blob, raw = B.mixed(9, 20, seed=3)
    v, pl = kta.value_bytes_host(blob, 2, P), kta.payload_host(blob, 2, P)
    counters = np.zeros(7 * P + 8, np.uint64)
    R.restate([(blob, 2, raw, set())], P, sizes=counters)
    _holds(v)
    _holds(v, pl)
    _holds(v, pl, counters)
    at = 2 * V.PW
    used = at + int(np.flatnonzero(v[at:at + 256])[0])
    for word, by in ((used, 1), (at + V.BYTES, 1), (at + V.REPEATS, int(v[at + V.BYTES])), (at + V.VALUES, int(v[at + V.RECORDS])), (at + 260, 1), (at + 263, 1),
                     (V.PW + 261, 1)):
        w = v.copy()
        w[word] += np.uint64(by)
        assert not kta.value_bytes_identities(w, P) and not all(ok for _, ok in V.identities(w, P)), word
    for col in (R.RECORDS, R.CLASS_BYTES + R.OTHER, R.CLASS + R.JSON):                # these only the payload vector pins down
        q = pl.copy()
        q[2 * R.PW + col] += 1
        assert kta.value_bytes_identities(v, P) and not kta.value_bytes_identities(v, P, q) and not all(ok for _, ok in V.identities(v, P, q)), col
    c = counters.copy()
    c[7 * 2] += 1
    assert not kta.value_bytes_identities(v, P, None, c) and not all(ok for _, ok in V.identities(v, P, None, c))
    with pytest.raises(ValueError):
        kta.value_bytes_identities(v, P, pl[:-1])
    with pytest.raises(ValueError):
        kta.value_bytes_identities(v[:-1], P)


def test_merge_adds_every_word():
    a = kta.value_bytes_host(B.mixed(5, 9, seed=1)[0], 0, P)
    b = kta.value_bytes_host(B.mixed(6, 7, seed=2)[0], 1, P)
    acc = a.copy()
    assert kta.merge_value_bytes(acc, b, P) is acc and np.array_equal(acc, a + b)
    _holds(acc)
    i64 = a.view(np.int64).copy()
    kta.merge_value_bytes(i64, b, P)
    assert np.array_equal(i64.view(np.uint64), a + b)
    with pytest.raises(ValueError):
        kta.merge_value_bytes(acc, b[:-1], P)


# ------------------------------------------------------------------------------------------ 4. exports, CLI
def test_new_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "kta_hip.h")).read()
    m = re.search(r"#define KTA_FLAG_VALUE_BYTES (\w+?)[uU]\s", header)
    assert m and int(m.group(1), 0) == 0x1000 == N.KTA_FLAG_VALUE_BYTES
    others = [int(v, 0) for v in re.findall(r"#define KTA_FLAG_(?!VALUE_BYTES)\w+ +\(?(\w+?)[uU]\b", header)]
    assert 0x1000 not in others and all(f & 0x1000 == 0 for f in others)            # bit 12 was free
    assert re.search(r"#define KTA_ABI_VERSION 7\b", header) and N.load().kta_abi_version() == 7
    assert (N.KTA_VALUE_BYTES_PARTITION_WORDS, N.KTA_VALUE_BYTES_BINS) == (V.PW, V.BINS) and re.search(r"#define KTA_VALUE_BYTES_PARTITION_WORDS 264\b", header)
    assert kta.VALUE_BYTES_CLASSES == V.CLASSES and N.C.sizeof(N.KtaValueBytesSummary) == 96
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    kafka_text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kta_kafka.h")).read(), flags=re.S)
    lib = N.load()
    for name in NEW_EXPORTS:
        assert re.search(r"^int\s+%s\s*\(" % name, text, flags=re.M), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    assert re.search(r"^int\s+kta_value_bytes_info\s*\(", kafka_text, flags=re.M) and hasattr(lib, "kta_value_bytes_info")
    for name in ("split_value_bytes", "merge_value_bytes", "value_bytes_identities", "value_bytes_summary", "value_bytes_host", "render_value_bytes"):
        assert name in kta.__all__ and callable(getattr(kta, name))
    for name in ("value_bytes", "exchange_value_bytes", "value_bytes_result_vector", "value_bytes_vector", "value_bytes_info"):
        assert callable(getattr(kta.HipMetricHandler, name))
    assert callable(distributed.allreduce_value_bytes_vector)


def _cli(*knobs, src="synthetic://c2?records=100", flags=()):
    return subprocess.run([CLI, "-t", "x", "-b", src, *flags, "--librdkafka", ",".join(knobs)], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value", ["2", "", "yes"])
def test_cli_refuses_a_value_other_than_0_or_1(value):
    r = _cli("kta.value_bytes=" + value)
    assert r.returncode == 2 and "kta.value_bytes=%s: expected 0 or 1" % value in r.stderr and r.stdout == "", (r.returncode, r.stderr)
    assert len(r.stderr.strip().splitlines()) == 1


@pytest.mark.parametrize("src,knobs", [("synthetic://c2?records=100", ()), ("dump:///nonexistent.dump", ()), ("localhost:1", ()),
                                       ("segment:///nonexistent.log", ("kta.per_message=1",)), ("synthetic://c2?records=100", ("kta.gpus=2",))])
def test_cli_refuses_sources_that_do_not_hold_the_log_bytes(src, knobs):
    """one line that says why, before a broker, a file or a device is asked for anything"""
    r = _cli("kta.value_bytes=1", *knobs, src=src)
    assert r.returncode == 2 and r.stdout == "", (r.returncode, r.stdout, r.stderr)
    lines = r.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("kta.value_bytes=1: needs a segment:// source") and "not the bytes of the log" in lines[0]


def test_cli_help_is_unchanged_by_the_knob():
    plain = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    knob = subprocess.run([CLI, "--librdkafka", "kta.value_bytes=1", "--help"], capture_output=True, text=True, timeout=60)
    assert plain.returncode == knob.returncode == 0 and knob.stdout == plain.stdout


# ------------------------------------------------------------------------------------------ 5. torch twin (gloo)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sets = []
        for p in range(5):                                                        # the same topic on every rank
            blob, raw = B.mixed(2, 9, seed=p)
            sets.append((blob, p, raw, set()))
        vecs = [V.restate([s for s in sets if s[1] % world == r], 5) for r in range(world)]
        t = torch.from_numpy(vecs[rank].view(np.int64).copy())
        from kafka_topic_analyzer_amd import distributed as D
        D.allreduce_value_bytes_vector(t, 5)
        whole = V.restate(sets, 5)
        q.put((rank, bool(np.array_equal(t.numpy().view(np.uint64), whole) and vecs[rank].any() and not np.array_equal(vecs[rank], whole))))
    finally:
        dist.destroy_process_group()


def test_allreduce_value_bytes_vector_over_gloo_equals_the_unsharded_vector():
    pytest.importorskip("torch")
    import multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(r for r, _ in res) == list(range(world))
    assert all(ok for _, ok in res), res


def test_allreduce_helper_checks_the_length():
    torch = pytest.importorskip("torch")
    with pytest.raises(AssertionError):
        distributed.allreduce_value_bytes_vector(torch.zeros(5, dtype=torch.int64), 4)


# ------------------------------------------------------------------------------------------ 6. the rule's own source
def test_native_check_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/value_bytes_check.cpp: a program of its own that calls kta_value_bytes.h, built with the sanitizers and run directly."""
    exe = str(tmp_path / "value_bytes_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "native", "value_bytes_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.returncode, r.stdout[-500:], r.stderr[-2000:])

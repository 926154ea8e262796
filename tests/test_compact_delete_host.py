"""CPU tests of the compact,delete what-if (kta_set_compact_delete; no reference counterpart): the restatement in
tests/compact_delete_py.py holds the identities; the host-only entry points — kta_compact_delete_whatif,
kta_render_compact_delete — against the restatement's formula, and both against its brute force, which builds every
partition's list of cleaned segments and runs the broker's two loops literally, on hand cases and random ones; the
mismatch verdicts; the header and the unchanged ABI number; the CLI's refusals that need no device; and the rule's own
source (csrc/kta_compact_delete.h) run natively under AddressSanitizer + UBSan (tests/native/compact_delete_check.cpp, a
program of its own)."""
import os
import re
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import compact_delete_py as CD
import compaction_py as CP
import segments_py as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc")
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
BASE = 1_600_000_000_000


def make(records, ts=None):
    """records: (partition, key or None, val_len) -> columns; ts: per record, or BASE + 1000 i"""
    blob = b""
    c = {"partition": [], "key_len": [], "val_len": [], "ts_ms": [], "key_off": []}
    for i, (p, key, vl) in enumerate(records):
        c["partition"].append(p), c["key_len"].append(-1 if key is None else len(key)), c["val_len"].append(vl)
        c["ts_ms"].append(BASE + 1000 * i if ts is None else ts[i]), c["key_off"].append(len(blob))
        blob += key or b""
    out = {k: np.array(v, np.int64 if k == "ts_ms" else np.uint32 if k == "key_off" else np.int32) for k, v in c.items()}
    out["key_bytes"] = np.frombuffer(blob, np.uint8).copy()
    return out


def random_topic(seed, n, P):
    """keys of 1 to 24 bytes from a pool of n / 8, 10 % tombstones, 5 % null keys, a few records outside [0, P)"""
    rng = np.random.default_rng(seed)
    pool = [bytes(rng.integers(0, 256, int(rng.integers(1, 25)), dtype=np.uint8)) for _ in range(max(n // 8, 1))]
    recs = []
    for _ in range(n):
        key = None if rng.random() < 0.05 else pool[int(rng.integers(0, len(pool)))]
        p = int(rng.integers(0, P)) if rng.random() > 0.03 else int(rng.choice([-1, P]))
        recs.append((p, key, -1 if rng.random() < 0.1 else int(rng.integers(0, 400))))
    ts = BASE + np.arange(n, dtype=np.int64) * 1000 + rng.integers(-5000, 5001, n)
    ts[rng.random(n) < 0.03] = -1
    return make(recs, ts.tolist())


def vectors(cols, P, S, M, overhead=0):
    seg = SP.segments_vector(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"], P, S, M, overhead)
    return seg, CD.kept_vector(cols, P, S, M, overhead), CP.brute_force(cols, P)


def whatif(cols, P, S, M, overhead, now, rms=-1, rb=-1, v=None):
    """the library's what-if == the restated formula == the brute force over explicit segment lists"""
    seg, kept, comp = v or vectors(cols, P, S, M, overhead)
    assert CD.identities_hold(seg, kept, comp, P, M)
    got = kta.compact_delete_whatif(seg, kept, comp, P, M, now, rms, rb)
    formula = np.array(CD.whatif_formula(seg, kept, P, M, now, rms, rb), np.uint64)
    brute = np.array(CD.whatif_brute(cols, P, S, M, overhead, now, rms, rb), np.uint64)
    assert np.array_equal(got, formula), (now, rms, rb, got.tolist(), formula.tolist())
    assert np.array_equal(got, brute), (now, rms, rb, got.tolist(), brute.tolist())
    return got


# ------------------------------------------------------------------------------------------ 1. the restatement
def test_the_restated_vectors_hold_the_identities():
    P, n, S, M, overhead = 5, 4000, 3000, 60, 11
    cols = random_topic(1, n, P)
    seg, kept, comp = vectors(cols, P, S, M, overhead)
    assert CD.identities_hold(seg, kept, comp, P, M)
    s, k, c = SP.split(seg, P, M), CD.split(kept, P, M), CP.split(comp, P)
    assert list(k["globals"]) == list(s["globals"]) and int(k["globals"][2]) > 20
    assert np.array_equal(k["totals"][:, 1], s["totals"][:, 1])
    assert np.array_equal(k["totals"][:, 0], c["live_records"]) and np.array_equal(k["totals"][:, 2], c["tombstone_records"])
    assert np.array_equal(k["totals"][:, 3], np.uint64(overhead) * (k["totals"][:, 0] + k["totals"][:, 2]) + c["live_key_bytes"] +
                          c["live_value_bytes"] + c["tombstone_key_bytes"])
    closed = s["rows"][:, :, 0] != 0
    assert np.array_equal(closed, k["rows"][:, :, 1] != 0) and np.array_equal(k["rows"][:, :, 1][closed], s["rows"][:, :, 1][closed])
    for p in range(P):
        rows = k["rows"][p][closed[p]]
        assert (np.diff(rows[:, [0, 2, 3]].astype(np.int64), axis=0) >= 0).all()
    # the input exercises the feature: survivors in closed rows, superseded records, and fewer kept than there are
    cls = np.array(CD.classes(cols))
    assert int(k["rows"][:, :, 0].max()) > 0 and int(k["rows"][:, :, 2].max()) > 0
    assert ((cls == 0) & (cols["key_len"] >= 0)).sum() > n // 2 and (cls == 1).any() and (cls == 2).any() and not (cls == -1).any()
    assert int(k["totals"][:, 0].sum() + k["totals"][:, 2].sum()) < int(s["totals"][:, 0].sum())
    # kta.compact_delete_whatif takes the restated vectors
    kta.compact_delete_whatif(seg, kept, comp, P, M, BASE)


# ------------------------------------------------------------------------------------------ 2. the what-if, hand cases
def test_no_closed_row_the_whole_log_is_active_and_nothing_is_cleaned():
    cols = make([(0, b"a", 10), (0, b"a", 10), (0, b"b", -1), (0, None, 5)])
    out = whatif(cols, 1, 1000, 4, 0, BASE + 10**9, rms=0, rb=0)
    assert list(out[0]) == [4, 28, 4, 28, 4, 28, 1, 0, 0, 0]                       # even the superseded "a" stays: the active segment
    assert list(out[1]) == list(out[0])


def test_every_row_deleted_but_the_active_one():
    # segments of 20 bytes: [a a] [b a] [c(tombstone) d] | active: a, unkeyed
    recs = [(0, b"a", 9), (0, b"a", 9), (0, b"b", 9), (0, b"a", 9), (0, b"c", -1), (0, b"d", 18), (0, b"a", 3), (0, None, 2)]
    cols = make(recs)
    out = whatif(cols, 1, 20, 10, 0, BASE + 10**9, rms=-1, rb=-1)
    # compaction alone: b, c (tombstone), d survive in closed rows; the active segment is whole
    assert list(out[0]) == [8, 66, 5, 10 + 1 + 19 + 6, 5, 36, 1, 0, 0, 0]
    out = whatif(cols, 1, 20, 10, 0, BASE + 10**9, rms=0)                          # everything closed is older than now
    assert list(out[0]) == [8, 66, 5, 36, 2, 6, 0, 3, 1, 0]
    out = whatif(cols, 1, 20, 10, 0, BASE, rms=-1, rb=0)                           # and the size rule alone takes them all as well
    assert list(out[0]) == [8, 66, 5, 36, 2, 6, 0, 3, 2, 0]


def test_only_one_of_the_two_rules_on():
    recs = [(0, bytes([65 + i]), 9) for i in range(10)] + [(0, b"z", 1)]           # ten segments of 10 bytes, all survive; active: 2 bytes
    cols = make(recs)
    now = BASE + 20_000
    out = whatif(cols, 1, 10, 30, 0, now, rms=15_000)                              # time: ts <= BASE + 4000: 5 segments
    assert out[0][7] == 5 and out[0][8] == 1 and out[0][4] == 6 and out[0][5] == 52
    out = whatif(cols, 1, 10, 30, 0, now, rb=72)                                   # size: 102 - 10 k >= 72: 3 segments
    assert out[0][7] == 3 and out[0][8] == 2 and out[0][5] == 72
    out = whatif(cols, 1, 10, 30, 0, now, rms=15_000, rb=72)                       # both: the longer
    assert out[0][7] == 5 and out[0][8] == 1
    out = whatif(cols, 1, 10, 30, 0, now, rms=18_500, rb=32)                       # time 2, size 7
    assert out[0][7] == 7 and out[0][8] == 2


def test_the_size_rule_looks_at_compacted_sizes():
    # three segments of 100 raw bytes of one key: compacted they hold 0, 0 and 0 bytes but for the last writer in the active one
    recs = [(0, b"k", 99)] * 3 + [(0, b"k", 4)]
    cols = make(recs)
    out = whatif(cols, 1, 100, 10, 0, BASE, rb=5)                                  # the compacted log is 5 bytes: every row's rest is >= 5
    assert list(out[0]) == [4, 305, 1, 5, 1, 5, 0, 3, 2, 0]
    out = whatif(cols, 1, 100, 10, 0, BASE, rb=6)                                  # 5 < 6: nothing goes, though the raw log is 305 bytes
    assert list(out[0]) == [4, 305, 1, 5, 1, 5, 0, 0, 0, 0]
    assert kta.retention_whatif(vectors(cols, 1, 100, 10)[0], 1, 10, BASE, -1, 6)[0][7] == 2   # (delete alone would take two)


def test_a_clamped_partition():
    recs = [(0, bytes([65 + i]), 99) for i in range(10)]
    cols = make(recs)
    out = whatif(cols, 1, 100, 3, 0, BASE, rb=0)                                   # rows 0 and 1 close, row 2 holds the other 8 and is active
    assert list(out[0]) == [10, 1000, 10, 1000, 8, 800, 0, 2, 2, 1]
    assert out[1][9] == 1
    seg, kept, comp = vectors(cols, 1, 100, 3)
    assert "0+ " in kta.render_compact_delete(seg, kept, comp, 1, 3, BASE, -1, 0)


def test_a_last_writer_in_a_deleted_segment_while_older_copies_sit_in_another_partition():
    # key "k": partition 1 holds two old copies, partition 0 the last writer, in a segment retention deletes.  Keys are
    # counted topic-wide: the copies in partition 1 are superseded, so the policy leaves no record of "k" at all.
    recs = [(1, b"k", 4), (1, b"k", 4), (0, b"k", 9), (0, b"x", 9), (1, b"y", 0), (0, b"w", 3)]
    cols = make(recs)
    out = whatif(cols, 2, 10, 8, 0, BASE + 10**9, rms=0)
    # partition 0: segments [k] [x] deleted by time, active [w]; partition 1: segment [k k] (5 + 5 bytes reach S) is empty after
    # cleaning and then deleted, active [y]
    assert list(out[0]) == [3, 24, 3, 24, 1, 4, 0, 2, 1, 0]
    assert list(out[1]) == [3, 11, 1, 1, 1, 1, 0, 1, 1, 0]
    # with an active segment that still holds an old copy, that copy stays: the active segment is not cleaned
    out = whatif(make(recs[:2] + [(1, b"k", 4)] + recs[2:]), 2, 10, 8, 0, BASE + 10**9, rms=0)
    assert list(out[1]) == [4, 16, 2, 6, 2, 6, 0, 1, 1, 0]
    cls = CD.classes(cols)
    assert cls[:3] == [0, 0, 1]


# ------------------------------------------------------------------------------------------ 3. random cases
@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("S", [1, 3000, 1 << 40])
def test_random_topics_and_policies(P, S):
    n, M, overhead = 4000, 1 << 13 if S == 1 else 40, 0 if S == 1 else 7
    if S == 1:
        overhead = 1                                                                # every record has at least a byte: each closes a row
    cols = random_topic(100 + P, n, P)
    v = vectors(cols, P, S, M, overhead)
    s = SP.split(v[0], P, M)
    if S == 1:                                                                      # every record closes a row until the rows run out
        assert int(s["globals"][2]) > 0 and (s["rows"][:, :M - 1, 0] != 0).sum(axis=1).max() <= M - 1 and (s["totals"][:, 1] >= M - 1).all()
        inside = (cols["partition"] >= 0) & (cols["partition"] < P)
        z = overhead + np.maximum(cols["key_len"], 0) + np.maximum(cols["val_len"], 0)
        want = 0
        for p in range(P):
            before = np.cumsum(z[inside & (cols["partition"] == p)]) - z[inside & (cols["partition"] == p)]
            want += int((before < M - 1).sum())
        assert int(s["globals"][2]) == want
    if S == 1 << 40:
        assert int(s["globals"][2]) == 0
    last = int(cols["ts_ms"].max())
    total = int(CD.split(v[1], P, M)["totals"][:, 3].max())
    for now in (last, last + 10**6, BASE):
        for rms in (-1, 0, 10**5, 2 * 10**6):
            for rb in (-1, 0, total // 3, total, total * 2):
                whatif(cols, P, S, M, overhead, now, rms, rb, v=v)
    text = kta.render_compact_delete(*v, P, M, last, 10**5, total // 3)
    assert text == CD.section(*v, P, M, last, 10**5, total // 3) and text.endswith("=" * 120 + "\n")
    assert kta.render_compact_delete(*v, P, M, last) == CD.section(*v, P, M, last)
    assert "retention.ms=-, retention.bytes=-, now=- ms" in CD.section(*v, P, M, last)


# ------------------------------------------------------------------------------------------ 4. the mismatch verdicts
def test_mismatch_verdicts_and_refusals():
    P, S, M = 3, 500, 50
    cols = random_topic(7, 1500, P)
    seg, kept, comp = vectors(cols, P, S, M, 2)
    kta.compact_delete_whatif(seg, kept, comp, P, M, BASE)
    tot = (P * M) * 4
    cases = {}
    bad = kept.copy(); bad[tot + 1] += np.uint64(1); cases["a perturbed B"] = (seg, bad, comp)
    row = int(np.flatnonzero(seg[:tot:4])[0]) * 4
    bad = kept.copy(); bad[row + 1] += np.uint64(1); cases["a perturbed row B"] = (seg, bad, comp)
    bad = kept.copy(); bad[row:row + 4] = 0; cases["a closed row missing"] = (seg, bad, comp)
    badc = comp.copy(); badc[5 * P + 2] = 1; cases["unknown != 0"] = (seg, kept, badc)
    other = CD.kept_vector(cols, P, S + 1, M, 2); cases["differing S"] = (seg, other, comp)
    half = {k: (v if k == "key_bytes" else v[:700]) for k, v in cols.items()}
    cases["another feed"] = (seg, CD.kept_vector(half, P, S, M, 2), CP.brute_force(half, P))
    for name, (a, b, c) in cases.items():
        assert not CD.identities_hold(a, b, c, P, M), name
        with pytest.raises(kta.KtaError):
            kta.compact_delete_whatif(a, b, c, P, M, BASE)
        with pytest.raises(kta.KtaError) as e:
            kta.render_compact_delete(a, b, c, P, M, BASE, 1000, 5)
        assert e.value.text == CD.section(a, b, c, P, M, BASE, 1000, 5), name
        assert "did not match the first pass" in e.value.text and "| P " not in e.value.text
    for badargs in ((-2, -1), (-1, -2)):
        with pytest.raises(kta.KtaError) as e:
            kta.compact_delete_whatif(seg, kept, comp, P, M, 0, *badargs)
        with pytest.raises(kta.KtaError) as e:
            kta.render_compact_delete(seg, kept, comp, P, M, 0, *badargs)
        assert e.value.text == ""
    lib = N.load()
    out = np.zeros((P + 1) * 10, np.uint64)
    args = (seg.ctypes.data, kept.ctypes.data, comp.ctypes.data, P, M, 0, -1, -1)
    assert lib.kta_compact_delete_whatif(*args, out.ctypes.data, out.size) == N.KTA_OK
    assert lib.kta_compact_delete_whatif(*args, out.ctypes.data, out.size - 1) == N.KTA_ERR_INVALID
    for k in range(3):
        a = list(args); a[k] = None
        assert lib.kta_compact_delete_whatif(*a, out.ctypes.data, out.size) == N.KTA_ERR_INVALID
    assert kta.compact_delete_max_partitions() == 2048 == min(kta.segments_max_partitions(), kta.compaction_max_partitions())


# ------------------------------------------------------------------------------------------ 5. header, ABI, CLI
def test_header_states_the_definition_and_the_abi_number_stays():
    text = open(os.path.join(ROOT, "include", "kta_hip.h")).read()
    for needle in ("int kta_set_compact_delete(", "int kta_get_compact_delete(", "int kta_compact_delete_info(", "int kta_compact_delete_whatif(",
                   "int kta_render_compact_delete(", "int kta_compact_delete_max_partitions(", "#define KTA_COMPACT_DELETE_WORDS 10",
                   "(klast.K + A.B) - kept[k].K >= retention_bytes"):
        assert needle in text, needle
    assert re.search(r"#define KTA_ABI_VERSION 7\b", text) and N.KTA_ABI_VERSION == 7
    for name in ("kta_set_compact_delete", "kta_get_compact_delete", "kta_compact_delete_info", "kta_compact_delete_whatif",
                 "kta_render_compact_delete", "kta_compact_delete_max_partitions"):
        assert hasattr(N.load(), name)


def _cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("flags,knobs,message", [
    (("-c",), "kta.segments=1g,kta.compact_delete=1", "kta.compact_delete=1: needs kta.compaction=1"),
    (("-c",), "kta.compaction=0,kta.segments=1g,kta.compact_delete=1", "kta.compact_delete=1: needs kta.compaction=1"),
    (("-c",), "kta.compaction=1,kta.compact_delete=1", "kta.compact_delete=1: needs kta.segments=<size>"),
    (("-c",), "kta.compaction=1,kta.segments=1g,kta.compact_delete=2", "kta.compact_delete=2: expected 0 or 1"),
    (("-c",), "kta.compaction=1,kta.segments=1g,kta.compact_delete=yes", "kta.compact_delete=yes: expected 0 or 1"),
    ((), "kta.compaction=1,kta.segments=1g,kta.compact_delete=1", "kta.compaction=1: needs -c"),
    (("-c",), "kta.compaction=1,kta.segments=1g,kta.compact_delete=1,kta.gpus=2", "kta.compaction=1: not with kta.gpus=2"),
    (("-c",), "kta.compaction=1,kta.segments=1g,kta.compact_delete=1,kta.per_message=1", "kta.compaction=1: not with kta.per_message=1"),
])
def test_cli_refusals_need_no_device(flags, knobs, message):
    r = _cli("-t", "c4", "-b", "synthetic://c4?records=1000", *flags, "--librdkafka", knobs)
    assert r.returncode == 2 and r.stderr.startswith(message) and r.stdout == "", (r.returncode, r.stderr, r.stdout)


def test_cli_refuses_a_broker_list():
    r = _cli("-t", "c4", "-b", "localhost:1", "-c", "--librdkafka", "kta.compaction=1,kta.segments=1g,kta.compact_delete=1")
    assert r.returncode == 2 and r.stderr.startswith("kta.compaction=1: needs a synthetic://") and r.stdout == ""


# ------------------------------------------------------------------------------------------ 6. the rule's own source
def test_native_check_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/compact_delete_check.cpp: a program of its own that calls kta_compact_delete.h, built with the sanitizers and run directly."""
    exe = str(tmp_path / "compact_delete_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "native", "compact_delete_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK "), (r.stdout[-500:], r.stderr[-3000:])

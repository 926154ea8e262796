"""CPU tests of the retention what-if (kta_set_segments; no reference counterpart): the restatement in tests/segments_py.py
holds the identities; the host-only entry points — kta_merge_segments, kta_retention_whatif, kta_render_retention — against
the restatement, the what-if against a brute-force simulation that builds the list of segments and runs the broker's two
loops literally, on hand cases and random ones; the header's definition and the unchanged ABI number; the CLI's refusals
that need no device; and the rule's own source (csrc/kta_segments.h) run natively under AddressSanitizer + UBSan
(tests/native/segments_check.cpp, a program of its own)."""
import os
import re
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import segments_py as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc")
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
BASE = 1_600_000_000_000


def _cols(seed, n, P, max_val=500):
    rng = np.random.default_rng(seed)
    part = rng.integers(-1, P + 1, n).astype(np.int32)
    ts = BASE + np.arange(n, dtype=np.int64) * 1000 + rng.integers(-5000, 5001, n)
    ts[rng.random(n) < 0.05] = -1
    return {"partition": part, "key_len": rng.integers(-1, 40, n).astype(np.int32),
            "val_len": rng.integers(-1, max_val, n).astype(np.int32), "ts_ms": ts}


def _vec(cols, P, S, M, overhead=0):
    return SP.segments_vector(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"], P, S, M, overhead)


def _whatif(vec, P, M, now, rms=-1, rb=-1):
    got = kta.retention_whatif(vec, P, M, now, rms, rb)
    want = np.array(SP.retention_brute(vec, P, M, now, rms, rb), np.uint64)
    assert np.array_equal(got, want), (now, rms, rb, got.tolist(), want.tolist())
    return got


# ------------------------------------------------------------------------------------------ 1. the restatement
def test_the_restated_vector_holds_the_identities():
    P, n, overhead = 5, 4000, 11
    cols = _cols(1, n, P)
    s = SP.split(_vec(cols, P, 3000, 50, overhead), P, 50)
    p, k, v = cols["partition"], cols["key_len"], cols["val_len"]
    for q in range(P):
        m = p == q
        c, b, t, h1 = (int(x) for x in s["totals"][q])
        assert c == int(m.sum()) and t == int((v[m] < 0).sum())
        assert b - overhead * c == int(np.maximum(k[m], 0).sum() + np.maximum(v[m], 0).sum())
        assert h1 == int(cols["ts_ms"][m].max()) + 1
    inside = (p >= 0) & (p < P)
    assert list(s["globals"]) == [int(inside.sum()), int((~inside).sum()), int((s["rows"][:, :, 0] != 0).sum()), 3000, 50, overhead, 0, 0]
    assert int(s["globals"][2]) > 20 and not s["rows"][:, 49].any()                 # rows were closed; the last row never closes
    assert kta.segments_words(P, 50) == SP.words(P, 50) == len(s["rows"].reshape(-1)) + P * 4 + 8


def test_merge_is_the_sum_and_refuses_another_configuration():
    P, M = 4, 30
    cols = _cols(2, 3000, P)
    whole = _vec(cols, P, 2000, M, 3)
    parts = []
    for r in range(2):
        m = cols["partition"] % 2 == r
        parts.append(_vec({k: v[m] for k, v in cols.items()}, P, 2000, M, 3))
    acc = parts[0].copy()
    assert kta.merge_segments(acc, parts[1], P, M) is acc and np.array_equal(acc, whole)
    assert np.array_equal(SP.merge(parts[0], parts[1], P, M), whole)
    for other in ((2001, M, 3), (2000, M, 4)):
        acc = parts[0].copy()
        with pytest.raises(kta.KtaError):
            kta.merge_segments(acc, _vec(cols, P, *other), P, M)
        assert np.array_equal(acc, parts[0])
    with pytest.raises(kta.KtaError):                                               # another M is another length
        kta.merge_segments(parts[0].copy(), _vec(cols, P, 2000, M + 1, 3), P, M)
    with pytest.raises(ValueError):
        SP.merge(parts[0], _vec(cols, P, 2001, M, 3), P, M)


# ------------------------------------------------------------------------------------------ 2. the what-if, hand cases
def _one(records, S, M, overhead=0):
    """one partition; records: (value bytes, ts_ms)"""
    n = len(records)
    return SP.segments_vector(np.zeros(n, np.int32), np.full(n, -1, np.int32), np.array([r[0] for r in records], np.int32),
                              np.array([r[1] for r in records], np.int64), 1, S, M, overhead)


def test_a_young_out_of_order_record_protects_what_is_behind_it_and_itself():
    # four segments of 100 bytes; the second holds one record with a young timestamp: the time rule takes segment 0 only
    recs = [(100, 1000), (50, 2000), (50, 900_000), (100, 3000), (100, 4000), (10, 5000)]
    v = _one(recs, 100, 10)
    out = _whatif(v, 1, 10, now=1_000_000, rms=500_000)
    assert list(out[0]) == [5, 6, 410, 0, 5, 310, 0, 1, 1, 0]
    out = _whatif(v, 1, 10, now=2_000_000, rms=500_000)                             # later, everything closed is old
    assert out[0][7] == 4 and out[0][4] == 1 and out[0][5] == 10


def test_a_prefix_without_timestamps_is_not_deleted_by_time():
    recs = [(100, -1), (100, -1), (100, 1000), (100, 2000), (5, 3000)]
    v = _one(recs, 100, 10)
    out = _whatif(v, 1, 10, now=10**9, rms=1)
    assert out[0][7] == 0 and out[0][8] == 0 and out[0][4] == 5
    out = _whatif(v, 1, 10, now=10**9, rms=1, rb=205)                               # the size rule takes it: 405 - 200 >= 205
    assert out[0][7] == 2 and out[0][8] == 2 and out[0][5] == 205


def test_a_record_of_3_s_plus_1_bytes_skips_rows():
    recs = [(60, 1000), (301, 2000), (50, 3000), (60, 4000)]
    v = _one(recs, 100, 10)
    rows = SP.split(v, 1, 10)["rows"][0]
    assert [int(r[0]) for r in rows[:6]] == [2, 0, 0, 3, 0, 0]                      # rows 1 and 2 stay zero; the tail lies in row 4
    out = _whatif(v, 1, 10, now=10**7, rms=-1, rb=100)                              # 471 - 361 >= 100, 471 - 411 < 100
    assert list(out[0][:3]) == [3, 4, 471] and out[0][7] == 1 and out[0][5] == 110


def test_the_last_record_closes_its_segment_exactly_an_empty_tail():
    recs = [(100, 1000), (100, 2000)]
    v = _one(recs, 100, 10)
    out = _whatif(v, 1, 10, now=10**7, rms=0)
    assert list(out[0]) == [2, 2, 200, 0, 0, 0, 0, 2, 1, 0]                         # nothing is active: everything may go


def test_a_clamped_partition_and_retention_bytes_0():
    recs = [(100, 1000 * i) for i in range(10)]
    v = _one(recs, 100, 3)                                                          # rows 0 and 1 close, row 2 holds the other 8
    out = _whatif(v, 1, 3, now=10**7, rms=-1, rb=0)
    assert list(out[0]) == [3, 10, 1000, 0, 8, 800, 0, 2, 2, 1]
    out = _whatif(_one(recs, 100, 30), 1, 30, now=10**7, rms=-1, rb=0)              # unclamped: all ten are closed and go
    assert list(out[0]) == [10, 10, 1000, 0, 0, 0, 0, 10, 2, 0]


def test_both_rules_on_each_the_longer():
    recs = [(100, 1000 * i) for i in range(10)] + [(5, 20_000)]
    v = _one(recs, 100, 30)
    out = _whatif(v, 1, 30, now=20_000, rms=15_000, rb=905)                         # time: ts <= 4000, 5 segments; size: 1
    assert out[0][7] == 5 and out[0][8] == 1
    out = _whatif(v, 1, 30, now=20_000, rms=18_500, rb=305)                         # time: 2 segments; size: 7
    assert out[0][7] == 7 and out[0][8] == 2
    out = _whatif(v, 1, 30, now=20_000, rms=15_000, rb=505)                         # both 5: the tie is the time rule's
    assert out[0][7] == 5 and out[0][8] == 1


def test_random_topics_and_policies_and_the_refusals():
    for seed, (P, S, M) in enumerate([(1, 700, 40), (4, 5000, 12), (7, 300, 200)]):
        cols = _cols(10 + seed, 3000, P)
        v = _vec(cols, P, S, M, seed)
        last = int(cols["ts_ms"].max())
        total = int(SP.split(v, P, M)["totals"][:, 1].max())
        for now in (last, last + 10**6, BASE, 0):
            for rms in (-1, 0, 10**5, 10**6):
                for rb in (-1, 0, total // 3, total, total * 2):
                    _whatif(v, P, M, now, rms, rb)
    for bad in ((-2, -1), (-1, -2)):
        with pytest.raises(kta.KtaError):
            kta.retention_whatif(v, P, M, 0, *bad)
    with pytest.raises(kta.KtaError):
        kta.retention_whatif(np.zeros(SP.words(P, M), np.uint64), P, M, 0)          # no configuration in it: not a vector


# ------------------------------------------------------------------------------------------ 3. the section
def test_rendered_section_against_the_restated_text():
    P, M = 4, 12
    cols = _cols(20, 3000, P)
    v = _vec(cols, P, 5000, M, 9)
    last = int(cols["ts_ms"].max())
    for rms, rb in ((-1, -1), (10**6, -1), (-1, 20_000), (2 * 10**6, 30_000)):
        text = kta.render_retention(v, P, M, last, rms, rb)
        assert text == SP.section(v, P, M, last, rms, rb)
        assert ("Records kept" in text) == (rms >= 0 or rb >= 0) and text.endswith("=" * 120 + "\n")
    assert "outgrew the 12 rows" in text and "+ " in text                            # this topic is clamped at M = 12
    assert "outgrew" not in kta.render_retention(_vec(cols, P, 5000, 200, 9), P, 200, last, 10**6)


# ------------------------------------------------------------------------------------------ 4. header, ABI, CLI
def test_header_states_the_definition_and_the_abi_number_stays():
    text = open(os.path.join(ROOT, "include", "kta_hip.h")).read()
    for needle in ("s_next = min(floor(B[p] / S), M - 1)", "the record CLOSES segment s", "u64[(P*M + P) * 4 + 8]", "segment.ms rolling is not modelled",
                   "int kta_set_segments(", "int kta_retention_whatif(", "int kta_render_retention(", "int kta_exchange_segments("):
        assert needle in text, needle
    assert re.search(r"#define KTA_ABI_VERSION 7\b", text) and N.KTA_ABI_VERSION == 7


def _cli(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("knobs,message", [
    ("kta.retention.ms=7d", "kta.retention.ms=7d: needs kta.segments=<size>"),
    ("kta.retention.bytes=1g", "kta.retention.bytes=1g: needs kta.segments=<size>"),
    ("kta.retention.now=5", "kta.retention.now=5: needs kta.segments=<size>"),
    ("kta.segments=0", "kta.segments=0: expected a segment size"),
    ("kta.segments=2048g", "kta.segments=2048g: expected a segment size"),
    ("kta.segments=1g,kta.segments.rows=1", "kta.segments.rows=1: expected the rows kept per partition"),
    ("kta.segments=1g,kta.retention.ms=soon", "kta.retention.ms=soon: expected a duration"),
    ("kta.segments=1g,kta.retention.bytes=-5", "kta.retention.bytes=-5: expected a size"),
])
def test_cli_refusals_need_no_device(knobs, message):
    r = _cli("-t", "c4", "-b", "synthetic://c4?records=1000", "--librdkafka", knobs)
    assert r.returncode == 2 and r.stderr.startswith(message) and r.stdout == "", (r.returncode, r.stderr, r.stdout)


# ------------------------------------------------------------------------------------------ 5. the rule's own source
def test_native_check_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/segments_check.cpp: a program of its own that calls kta_segments.h, built with the sanitizers and run directly."""
    exe = str(tmp_path / "segments_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "native", "segments_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK "), (r.stdout[-500:], r.stderr[-3000:])

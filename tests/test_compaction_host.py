"""CPU tests of the compaction what-if (KTA_FLAG_COMPACTION; no reference counterpart): the restatement in
tests/compaction_py.py against a brute-force dict loop, the host-only section (kta_render_compaction) against the
restated text — a mixed topic, an empty partition, a replay that does not match —, the header's definition and the
unchanged ABI number, the CLI's refusals that need no device, and the rule's own source (csrc/kta_compaction.h) run
natively under AddressSanitizer + UBSan (tests/native/compaction_check.cpp, a program of its own)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import compaction_py as CP
from helpers import random_cols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
CSRC = os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc")
NEW_EXPORTS = ("kta_compaction_replay", "kta_get_compaction", "kta_compaction_max_partitions", "kta_compaction_info",
               "kta_render_compaction")


def _cols(seed, n, P, key_space):
    rng = np.random.default_rng(seed)
    cols = random_cols(rng, n, P, key_space=key_space, null_key=0.1, empty_key=0.05, tomb=0.3, max_key=40)
    cols["partition"][rng.random(n) < 0.02] = -1
    cols["partition"][rng.random(n) < 0.02] = P + 3
    return cols


# ------------------------------------------------------------------------------------------ 1. the restatement
def test_restatement_equals_a_brute_force_dict_loop():
    P = 5
    cols = _cols(1, 5000, P, 700)
    v = CP.vector(cols, P)
    assert np.array_equal(v, CP.brute_force(cols, P))
    d = CP.split(v, P)
    assert d["unknown"] == 0 and d["replayed"] == 5000 and d["unkeyed"] > 0 and d["live_outside"] + d["tombstones_outside"] > 0
    assert (d["live_records"] > 0).all() and (d["tombstone_records"] > 0).all()
    # sequence numbers that neither ascend nor are consecutive
    seq = np.random.default_rng(2).permutation(5000).astype(np.uint64) * np.uint64(3) + np.uint64(10)
    assert np.array_equal(CP.vector(cols, P, seq), CP.brute_force(cols, P, seq))
    assert not np.array_equal(CP.vector(cols, P, seq), v)


def test_restatement_of_a_replay_that_does_not_match():
    P = 5
    cols = _cols(3, 2000, P, 300)
    table = CP.last_writers(cols, np.arange(2000, dtype=np.uint64))
    shifted = CP.split(CP.vector(cols, P, np.arange(2000, dtype=np.uint64) + np.uint64(7), table), P)
    assert shifted["unknown"] > 0
    # with sequence numbers shifted DOWN nothing is unknown and nothing survives but by accident of the alive bit
    half = {k: (v if k == "key_bytes" else v[:1000]) for k, v in cols.items()}
    d = CP.split(CP.vector(half, P, None, table), P)
    assert d["replayed"] == 1000 and d["unknown"] == 0


# ------------------------------------------------------------------------------------------ 2. the section
def test_render_compaction_is_the_restated_section():
    P = 5
    cols = _cols(4, 5000, P, 700)
    vec, cv = CP.vector(cols, P), CP.counters(cols, P)
    text = kta.render_compaction(vec, cv, P)
    assert text == CP.section(vec, cv, P)
    assert text.startswith(CP.TITLE) and "Kept outside the partition range:" in text and text.endswith(CP.NOTE + "=" * 120 + "\n")
    d = CP.split(vec, P)
    assert "Records without a key: %d (not kept: compaction goes by key)\n" % d["unkeyed"] in text
    total = "| Topic | %d " % int(cv[0:7 * P:7].sum())
    assert total in text and " n/a " not in text


def test_render_compaction_an_empty_partition_prints_n_a():
    P = 4
    cols = _cols(5, 3000, P, 400)
    cols["partition"][cols["partition"] == 2] = 1                  # partition 2 holds nothing
    cols["partition"][cols["partition"] < 0] = 0
    cols["partition"][cols["partition"] >= P] = 3
    vec, cv = CP.vector(cols, P), CP.counters(cols, P)
    text = kta.render_compaction(vec, cv, P)
    assert text == CP.section(vec, cv, P)
    row = [ln for ln in text.splitlines() if ln.startswith("| 2 ")][0]
    assert row.count(" n/a ") == 2 and "Kept outside" not in text
    # nothing at all: every share n/a, no division
    empty = np.zeros(CP.words(P), np.uint64)
    text = kta.render_compaction(empty, np.zeros(P * 7 + 8, np.uint64), P)
    assert text == CP.section(empty, np.zeros(P * 7 + 8, np.uint64), P) and text.count(" n/a ") == 2 * (P + 1)


def test_render_compaction_refuses_a_replay_that_does_not_match():
    P = 5
    cols = _cols(6, 2000, P, 300)
    vec, cv = CP.vector(cols, P), CP.counters(cols, P)
    lib = N.load()
    n = C.c_size_t()
    for word, what in ((CP.WORDS * P + CP.UNKNOWN, "unknown != 0"), (CP.WORDS * P + CP.REPLAYED, "replayed short")):
        bad = vec.copy()
        bad[word] = bad[word] + np.uint64(1) if what == "unknown != 0" else bad[word] - np.uint64(10)
        with pytest.raises(kta.KtaError) as e:
            kta.render_compaction(bad, cv, P)
        assert e.value.code == N.KTA_ERR_INVALID, what
        assert e.value.text == CP.section(bad, cv, P) and "The replay did not match the first pass" in e.value.text, what
        assert "| Topic" not in e.value.text
        assert lib.kta_render_compaction(bad.ctypes.data, cv.ctypes.data, P, None, 0, C.byref(n)) == N.KTA_ERR_INVALID
        assert n.value == len(e.value.text)
    # replayed counts the records outside the partition range too: records + bad-partition records
    assert int(vec[CP.WORDS * P + CP.REPLAYED]) == int(cv[7 * P + N.KTA_G_RECORDS] + cv[7 * P + N.KTA_G_BAD_PARTITION]) == 2000
    assert cv[7 * P + N.KTA_G_BAD_PARTITION] > 0
    # the buffer conventions, and the arguments
    assert lib.kta_render_compaction(vec.ctypes.data, cv.ctypes.data, P, None, 0, C.byref(n)) == N.KTA_OK
    buf = C.create_string_buffer(20)
    assert lib.kta_render_compaction(vec.ctypes.data, cv.ctypes.data, P, buf, 20, C.byref(n)) == N.KTA_OK
    assert buf.value.decode() == CP.TITLE[:19] and n.value == len(CP.section(vec, cv, P))
    assert lib.kta_render_compaction(None, cv.ctypes.data, P, None, 0, C.byref(n)) == N.KTA_ERR_INVALID
    assert lib.kta_render_compaction(vec.ctypes.data, None, P, None, 0, C.byref(n)) == N.KTA_ERR_INVALID
    assert lib.kta_render_compaction(vec.ctypes.data, cv.ctypes.data, 0, None, 0, C.byref(n)) == N.KTA_ERR_INVALID
    assert lib.kta_render_compaction(vec.ctypes.data, cv.ctypes.data, kta.compaction_max_partitions() + 1, None, 0, C.byref(n)) == N.KTA_ERR_INVALID
    with pytest.raises(ValueError):
        kta.render_compaction(vec[:-1], cv, P)


def test_split_compaction():
    P = 3
    v = np.arange(CP.words(P), dtype=np.uint64) + np.uint64(100)
    d = kta.split_compaction(v, P)
    assert d["live_records"].tolist() == [100, 105, 110] and d["tombstone_key_bytes"].tolist() == [104, 109, 114]
    assert (d["replayed"], d["unkeyed"], d["unknown"], d["live_outside"], d["tombstones_outside"]) == (115, 116, 117, 118, 119)
    assert np.array_equal(d["vector"], v)
    with pytest.raises(ValueError):
        kta.split_compaction(v[:-1], P)


# ------------------------------------------------------------------------------------------ 3. ABI, limit, CLI
def test_new_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "kta_hip.h")).read()
    m = re.search(r"#define KTA_FLAG_COMPACTION \(?(\w+)u\)?\s", header)
    assert m and int(m.group(1), 0) == 0x80 == N.KTA_FLAG_COMPACTION
    assert re.search(r"#define KTA_ABI_VERSION 7\b", header)
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = N.load()
    for name in NEW_EXPORTS:
        assert re.search(r"^int\s+%s\s*\(" % name, text, flags=re.M), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    assert lib.kta_abi_version() == 7
    flags = [int(v, 0) for v in re.findall(r"#define KTA_FLAG_\w+ +\(?(\w+)u\b", header)]
    assert sorted(flags) == [1, 2, 4, 8, 16, 32, 64, 128]        # the next free bit, no bit twice
    assert N.KTA_COMPACTION_WORDS == CP.WORDS == 5 and N.KTA_COMPACTION_GLOBALS == CP.GLOBALS == 6
    assert re.search(r"#define KTA_COMPACTION_WORDS 5\b", header) and re.search(r"#define KTA_COMPACTION_GLOBALS 6\b", header)


def test_the_pass_admits_at_least_4096_partitions():
    assert kta.compaction_max_partitions() >= 4096


def _cli(*knobs, src="synthetic://c2?records=100", flags=("-c",)):
    return subprocess.run([CLI, "-t", "x", "-b", src, *flags, "--librdkafka", ",".join(knobs)], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("knobs, flags, src, says", [
    (("kta.compaction=1",), (), None, "kta.compaction=1: needs -c"),
    (("kta.compaction=2",), ("-c",), None, "kta.compaction=2: expected 0 or 1"),
    (("kta.compaction=",), ("-c",), None, "kta.compaction=: expected 0 or 1"),
    (("kta.compaction=yes",), ("-c",), None, "kta.compaction=yes: expected 0 or 1"),
    (("kta.compaction=1", "kta.gpus=2"), ("-c",), None, "kta.compaction=1: not with kta.gpus=2"),
    (("kta.compaction=1", "kta.per_message=1"), ("-c",), None, "kta.compaction=1: not with kta.per_message=1"),
    (("kta.compaction=1",), ("-c",), "127.0.0.1:9,127.0.0.1:10", "kta.compaction=1: needs a synthetic://, segment:// or dump:// source"),
])
def test_cli_refusals_that_need_no_device(knobs, flags, src, says):
    """usage errors in the style of the other kta.* keys: a line on stderr, exit status 2, nothing on stdout"""
    r = _cli(*knobs, flags=flags) if src is None else _cli(*knobs, src=src, flags=flags)
    assert r.returncode == 2 and says in r.stderr and r.stdout == "", (r.returncode, r.stderr)
    assert len(r.stderr.strip().splitlines()) == 1


def test_cli_refuses_more_partitions_than_the_pass_admits(tmp_path):
    """a topic dump of limit + 1 partitions: refused after its header was read, before any context is created"""
    P = kta.compaction_max_partitions() + 1
    path = tmp_path / "wide.dump"
    import struct
    with open(path, "wb") as f:
        f.write(b"KTADUMP1" + struct.pack("<IIQQ", 1, P, 0, 0) + struct.pack("<%dq" % P, *([0] * P)) + struct.pack("<%dq" % P, *([1] * P)))
    r = _cli("kta.compaction=1", src="dump://" + str(path))
    assert r.returncode == 2 and r.stdout == "", (r.returncode, r.stderr)
    assert "kta.compaction=1: the topic has %d partitions, the compaction pass admits at most %d" % (P, P - 1) in r.stderr


def test_cli_help_is_unchanged_by_the_compaction_knob():
    plain = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    knob = subprocess.run([CLI, "-c", "--librdkafka", "kta.compaction=1", "--help"], capture_output=True, text=True, timeout=60)
    assert plain.returncode == knob.returncode == 0 and knob.stdout == plain.stdout


# ------------------------------------------------------------------------------------------ 4. the rule's own source
def test_native_check_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/compaction_check.cpp: a program of its own that calls kta_compaction.h, built with the sanitizers and run directly."""
    exe = str(tmp_path / "compaction_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "native", "compaction_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK "), (r.stdout[-500:], r.stderr[-3000:])

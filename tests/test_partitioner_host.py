"""CPU tests of the partitioner pass (KTA_FLAG_PARTITIONER; no reference counterpart): the host helper kta_murmur2 against
Kafka's known answers and the restatement in tests/partitioner_py.py, the host-only merge and section, the header's
constants and the unchanged ABI number, the CLI's refusals that need no device, and the hash's own source
(csrc/kta_murmur2.h) run natively under AddressSanitizer + UBSan (tests/native/murmur2_check.cpp, a child process)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import partitioner_py as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
CSRC = os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
NEW_EXPORTS = ("kta_set_repartition", "kta_get_partitioner", "kta_exchange_partitioner", "kta_partitioner_result_vector",
               "kta_merge_partitioner", "kta_partitioner_max_partitions", "kta_partitioner_info", "kta_render_partitioner")


# ------------------------------------------------------------------------------------------ 1. the hash
def test_murmur2_known_answers():
    for key, want in R.KNOWN.items():
        assert R.murmur2(key) == want & 0xFFFFFFFF, key
        assert kta.murmur2(key) == want & 0xFFFFFFFF, key
    assert kta.murmur2(b"") == 0x106E08D9
    assert R.to_positive(R.murmur2(b"21")) == (-973932308) & 0x7FFFFFFF        # toPositive, not abs


def test_murmur2_equals_the_restatement_on_random_keys():
    rng = np.random.default_rng(5)
    keys = [rng.integers(0, 256, int(rng.integers(0, 301)), dtype=np.uint8).tobytes() for _ in range(2000)]
    keys += [bytes([255]) * L for L in range(0, 40)]
    assert {len(k) % 4 for k in keys} == {0, 1, 2, 3} and max(map(len, keys)) > 290
    top = 0
    for k in keys:
        h = R.murmur2(k)
        assert kta.murmur2(k) == h, k
        top += h >> 31
    assert 0 < top < len(keys)
    # the column form of the restatement is the scalar form
    blob = np.frombuffer(b"".join(keys), np.uint8)
    kl = np.array([len(k) for k in keys], np.int32)
    off = np.concatenate([[0], np.cumsum(kl)[:-1]]).astype(np.uint32)
    got = R.hashes({"key_len": kl, "key_off": off, "key_bytes": blob})
    assert np.array_equal(got, np.array([R.murmur2(k) for k in keys], np.uint32))


@pytest.fixture(scope="module")
def murmur2_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("murmur2_check") / "murmur2_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-Wno-unknown-pragmas", "-I", CSRC, "-I", NATIVE, os.path.join(NATIVE, "murmur2_check.cpp"),
                        "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("no AddressSanitizer toolchain: " + r.stderr[-300:])
    return exe


def test_the_kernels_hash_source_is_memory_safe_and_exact_natively(murmur2_check):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:detect_stack_use_after_return=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([murmur2_check], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("OK "), (r.stdout + r.stderr)[-4000:]
    assert int(r.stdout.split()[1]) > 81 * 4 * 4


# ------------------------------------------------------------------------------------------ 2. merge and section
def _cols(records):
    """[(partition, key | None, val_len)] -> columns"""
    blob, off = b"", []
    for _, k, _ in records:
        off.append(len(blob))
        blob += k or b""
    return {"partition": np.array([r[0] for r in records], np.int32),
            "key_len": np.array([-1 if r[1] is None else len(r[1]) for r in records], np.int32),
            "val_len": np.array([r[2] for r in records], np.int32), "key_off": np.array(off, np.uint32),
            "key_bytes": np.frombuffer(blob + b"\0", np.uint8)}


def _key_for(p, P, tag):
    """A key that murmur2 places on partition p of P."""
    i = 0
    while True:
        k = b"%s-%d" % (tag, i)
        if R.to_positive(R.murmur2(k)) % P == p:
            return k
        i += 1


def test_vector_of_a_hand_built_topic():
    P, Q = 3, 7
    k0, k2 = _key_for(0, P, b"a"), _key_for(2, P, b"b")
    recs = [(0, k0, 10), (2, k0, -1), (2, k2, 5), (1, None, 9), (5, k0, 1), (-1, k2, 1), (2, b"", 0)]
    v = kta.split_partitioner(R.vector(_cols(recs), P, Q), P, Q)
    e = R.to_positive(R.murmur2(b"")) % P
    assert list(v["checked"]) == [1, 0, 3] and list(v["placed"]) == [1, 0, 1 + (e == 2)]
    assert int(v["target_records"].sum()) == 4
    assert int(v["target_bytes"].sum()) == len(k0) + 10 + len(k0) + len(k2) + 5                 # a tombstone adds its key only
    q0 = R.to_positive(R.murmur2(k0)) % Q
    assert int(v["target_records"][q0]) >= 2


def test_merge_adds_every_word():
    P, Q = 5, 9
    rng = np.random.default_rng(3)
    a = rng.integers(0, 1 << 62, R.words(P, Q), dtype=np.uint64)
    b = rng.integers(0, 1 << 62, R.words(P, Q), dtype=np.uint64)
    a[3], b[3] = (1 << 64) - 5, 9
    want = R.merge(a, b)
    assert int(want[3]) == 4
    got = a.copy()
    assert kta.merge_partitioner(got, b, P, Q) is got and np.array_equal(got, want)
    lib = N.load()
    assert lib.kta_merge_partitioner(None, b.ctypes.data, P, Q) == N.KTA_ERR_INVALID
    assert lib.kta_merge_partitioner(a.ctypes.data, b.ctypes.data, 0, Q) == N.KTA_ERR_INVALID
    assert lib.kta_merge_partitioner(a.ctypes.data, b.ctypes.data, P, 0) == N.KTA_ERR_INVALID
    assert lib.kta_merge_partitioner(a.ctypes.data, b.ctypes.data, P, kta.partitioner_max_partitions() + 1) == N.KTA_ERR_INVALID
    with pytest.raises(ValueError):
        kta.merge_partitioner(got, b[:-1], P, Q)


def _render_cases():
    out = {}
    P = 4
    recs = [(p, _key_for(p, P, b"k%d" % j), 10 * j) for j in range(30) for p in range(P)] + [(1, None, 7)] * 3
    out["all placed"] = (_cols(recs), P, P)
    P = 3
    recs = [(0, _key_for(0, P, b"x"), 100)] * 5 + [(2, _key_for(0, P, b"y"), 50)] * 2 + [(2, _key_for(2, P, b"z"), -1)] * 4 + \
           [(1, None, 5)] * 6
    out["P = 3, Q = 7, a partition without keyed records"] = (_cols(recs), P, 7)
    out["nothing keyed"] = (_cols([(0, None, 5), (1, None, -1), (1, None, 0)]), 2, 5)
    P = 8
    recs = [(p, b"key-%d" % j, j) for j in range(400) for p in [(j * 5 + 3) % P]]
    out["placed by another rule"] = (_cols(recs), P, 12)
    return out


@pytest.mark.parametrize("name", ["all placed", "P = 3, Q = 7, a partition without keyed records", "nothing keyed",
                                  "placed by another rule"])
def test_render_equals_the_restatement(name):
    cols, P, Q = _render_cases()[name]
    vec, cv = R.vector(cols, P, Q), R.counters(cols, P)
    text = kta.render_partitioner(vec, cv, P, Q)
    assert text == R.section(vec, cv, P, Q)
    assert text.startswith(R.TITLE) and text.endswith("=" * 120 + "\n") and text.count("\n" + "=" * 120) == 1
    assert "Repartition what-if: the keyed records over Q = %d partitions by murmur2\n" % Q in text
    if name == "all placed":
        assert "All keyed records lie on murmur2's partition" in text and "Records without a key: 3 " in text
        assert re.search(r"\| Topic +\| 120 +\| 120 +\| 100\.00 +\|", text)
    if name.startswith("P = 3"):
        assert re.search(r"\| 1 +\| 0 +\| - +\| - +\|", text) and re.search(r"\| 2 +\| 6 +\| 4 +\| 66\.67 +\|", text)
        assert "81.82 % of the keyed records lie on murmur2's partition" in text and "Records without a key: 6 " in text
        assert len(re.findall(r"^\| \d+ +\|", text, flags=re.M)) == 3 + 7
    if name == "nothing keyed":
        assert "No record has a key: nothing to check.\n" in text and re.search(r"\| Topic +\| 0 +\| - +\| - +\|", text)
        assert "records -, bytes -; the topic as it is (P = 2): records -, bytes " in text
    if name == "placed by another rule":
        assert "No more keyed records lie on murmur2's partition than chance puts there" in text and "1/P = 12.50 %" in text


def test_render_refuses_bad_arguments_and_reports_the_length():
    lib = N.load()
    cols, P, Q = _render_cases()["all placed"]
    vec, cv = R.vector(cols, P, Q), R.counters(cols, P)
    n = C.c_size_t()
    assert lib.kta_render_partitioner(vec.ctypes.data, cv.ctypes.data, P, Q, None, 0, C.byref(n)) == N.KTA_OK
    assert n.value == len(R.section(vec, cv, P, Q))
    buf = C.create_string_buffer(20)
    assert lib.kta_render_partitioner(vec.ctypes.data, cv.ctypes.data, P, Q, buf, 20, C.byref(n)) == N.KTA_OK
    assert buf.value.decode() == R.section(vec, cv, P, Q)[:19]
    assert lib.kta_render_partitioner(None, cv.ctypes.data, P, Q, None, 0, C.byref(n)) == N.KTA_ERR_INVALID
    assert lib.kta_render_partitioner(vec.ctypes.data, None, P, Q, None, 0, C.byref(n)) == N.KTA_ERR_INVALID
    assert lib.kta_render_partitioner(vec.ctypes.data, cv.ctypes.data, 0, Q, None, 0, C.byref(n)) == N.KTA_ERR_INVALID
    assert lib.kta_render_partitioner(vec.ctypes.data, cv.ctypes.data, P, 0, None, 0, C.byref(n)) == N.KTA_ERR_INVALID
    with pytest.raises(ValueError):
        kta.render_partitioner(vec[:-1], cv, P, Q)


# ------------------------------------------------------------------------------------------ 3. ABI, limit, CLI
def test_new_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "kta_hip.h")).read()
    m = re.search(r"#define KTA_FLAG_PARTITIONER (\w+)u\b", header)
    assert m and int(m.group(1), 0) == 64 == N.KTA_FLAG_PARTITIONER
    assert re.search(r"#define KTA_ABI_VERSION 7\b", header)
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = N.load()
    for name in NEW_EXPORTS:
        assert re.search(r"^int\s+%s\s*\(" % name, text, flags=re.M), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    assert re.search(r"^uint32_t\s+kta_murmur2\s*\(", text, flags=re.M) and "kta_murmur2" in N.SIGNATURES
    assert lib.kta_abi_version() == 7
    flags = [int(v, 0) for v in re.findall(r"#define KTA_FLAG_\w+ +(\w+)u\b", header)]
    assert sorted(flags) == [1, 2, 4, 8, 16, 32, 64]             # the next free bit, no bit twice


def test_the_pass_admits_at_least_4096_partitions_and_targets():
    assert kta.partitioner_max_partitions() >= 4096


def _cli(*kv):
    return subprocess.run([CLI, "-t", "c2", "-b", "synthetic://c2?records=1000", "--librdkafka", ",".join(kv)],
                          capture_output=True, text=True, timeout=60)


def test_cli_refusals_that_need_no_device():
    r = _cli("kta.partitioner=crc32")
    assert r.returncode == 2 and r.stdout == "" and "kta.partitioner=crc32" in r.stderr and "murmur2" in r.stderr
    r = _cli("kta.partitioner=murmur2", "kta.repartition=0")
    assert r.returncode == 2 and r.stdout == "" and "kta.repartition=0" in r.stderr
    r = _cli("kta.repartition=5")
    assert r.returncode == 2 and r.stdout == "" and "kta.repartition=5" in r.stderr and "kta.partitioner" in r.stderr
    for bad in ("", "x", "-3", "1e3", str(kta.partitioner_max_partitions() + 1)):
        r = _cli("kta.partitioner=murmur2", "kta.repartition=" + bad)
        assert r.returncode == 2 and r.stdout == "" and "kta.repartition=" in r.stderr, bad
    r = _cli("kta.partitioner=1")
    assert r.returncode == 2 and "murmur2" in r.stderr


def test_cli_help_is_unchanged_by_the_partitioner_knob():
    plain = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    knob = subprocess.run([CLI, "--librdkafka", "kta.partitioner=murmur2", "--help"], capture_output=True, text=True, timeout=60)
    assert plain.returncode == knob.returncode == 0 and knob.stdout == plain.stdout

"""CPU tests of the key sketch (KTA_FLAG_KEY_SKETCH; no reference counterpart): the host-only estimator, merge and section
against the independent restatement in tests/key_sketch_py.py, the estimator's accuracy on known sets of hashes, the new
exports, the CLI's refusal (before any context, so without a GPU), and the torch twin of the exchange over gloo."""
import json
import os
import re
import socket
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import key_sketch_py as K
from helpers import random_cols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
NEW_EXPORTS = ("kta_get_key_sketch", "kta_exchange_key_sketch", "kta_key_sketch_result_vector", "kta_merge_key_sketch",
               "kta_key_sketch_estimate", "kta_key_sketch_info", "kta_render_distinct_keys")


def _distinct_hashes(n, seed):
    rng = np.random.default_rng(seed)
    h = np.unique(rng.integers(0, 1 << 32, size=n + n // 8 + 64, dtype=np.uint64))
    rng.shuffle(h)
    assert len(h) >= n
    return h[:n]


def _rel(a, b):
    if a == b:
        return 0.0
    return abs(a - b) / max(abs(a), abs(b))


# ------------------------------------------------------------------------------------------ 1. the restatement
def test_restatement_fnv_matches_the_golden_kats():
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "fnv32_kats.json")))
    assert len(kats) >= 8
    keys = [bytes.fromhex(k["key_hex"]) for k in kats]
    for k, key in zip(kats, keys):
        assert K.fnv1a(key) == k["hash"], k["key_hex"]
    off = np.cumsum([0] + [len(k) for k in keys[:-1]]).astype(np.uint32)
    kb = np.frombuffer(b"".join(keys), np.uint8)
    got = K.fnv_columns(np.array([len(k) for k in keys]), off, kb)
    assert [int(x) for x in got] == [k["hash"] for k in kats]


def test_restatement_rho_and_register_of_edge_hashes():
    # fmix32 is a bijection: find hashes whose mixed value has all-zero low bits, or a single low bit
    x = K.fmix32(np.arange(1 << 22, dtype=np.uint64))
    assert len(np.unique(x)) == 1 << 22
    j, rho = K.register_and_rho(np.arange(1 << 22, dtype=np.uint64))
    w = (x << np.uint64(12)) & K.U32
    assert np.array_equal(j, (x >> np.uint64(20)).astype(np.int64))
    assert rho.min() >= 1 and rho.max() <= 21
    for k in range(1, 21):   # rho == k exactly when the top k-1 bits of w are 0 and bit k-1 is 1
        sel = rho == k
        assert np.all((w[sel] >> np.uint64(32 - k)) == 1), k
    assert np.all(w[rho == 21] == 0)


# ------------------------------------------------------------------------------------------ 2. estimator, merge
def _sketches(P, rng):
    empty = np.zeros((P, K.M), np.uint64)
    single = empty.copy()
    single[P - 1, 17] = 5
    rnd = rng.integers(0, 22, size=(P, K.M)).astype(np.uint64)
    sparse = np.where(rng.random((P, K.M)) < 0.01, rng.integers(1, 8, size=(P, K.M)), 0).astype(np.uint64)
    sat = np.full((P, K.M), 21, np.uint64)
    return {"empty": empty, "single": single, "random": rnd, "sparse": sparse, "saturated": sat}


@pytest.mark.parametrize("P", [1, 2, 7, 64, 300])
def test_estimate_equals_the_python_estimator(P):
    rng = np.random.default_rng(P)
    for name, sk in _sketches(P, rng).items():
        per, topic = kta.estimate_distinct_keys(sk, P)
        want_per, want_topic = K.estimate(sk)
        assert len(per) == P
        for a, b in zip(per, want_per):
            assert (a == b) if not np.isfinite(b) else _rel(a, b) <= 1e-12, (name, a, b)
        assert (topic == want_topic) if not np.isfinite(want_topic) else _rel(topic, want_topic) <= 1e-12, name
    per, topic = kta.estimate_distinct_keys(np.zeros((P, K.M), np.uint64), P)
    assert topic == 0.0 and np.all(per == 0.0)
    per, topic = kta.estimate_distinct_keys(np.full((P, K.M), 21, np.uint64), P)
    assert topic == np.inf and np.all(per == np.inf)


def test_estimate_refuses_a_register_above_21():
    sk = np.zeros((2, K.M), np.uint64)
    sk[1, 3] = 22
    with pytest.raises(kta.KtaError):
        kta.estimate_distinct_keys(sk, 2)
    with pytest.raises(ValueError):
        kta.estimate_distinct_keys(np.zeros(K.M, np.uint64), 2)


@pytest.mark.parametrize("n", [1, 2, 3, 10, 50, 100, 300, 1000, 3000, 10_000, 100_000, 1_000_000, 10_000_000])
def test_estimate_of_n_distinct_hashes(n):
    h = _distinct_hashes(n, seed=n)
    sk = K.sketch_from_hashes(np.zeros(n, np.int64), h, 1)
    (e,), topic = kta.estimate_distinct_keys(sk, 1)
    assert e == topic
    if n <= 1000:
        assert abs(e - n) <= 0.02 * n + 1, (n, e)
    else:
        assert abs(e / n - 1) <= 0.05, (n, e)


def test_topic_estimate_counts_a_hash_of_two_partitions_once():
    h = _distinct_hashes(200_000, seed=5)
    part = np.arange(len(h)) % 4
    sk = K.sketch_from_hashes(part, h, 4)
    dup = K.sketch_from_hashes(np.concatenate([part, (part + 1) % 4]), np.concatenate([h, h]), 4)
    per, topic = kta.estimate_distinct_keys(sk, 4)
    per2, topic2 = kta.estimate_distinct_keys(dup, 4)
    assert abs(topic / 200_000 - 1) <= 0.05 and abs(topic2 / topic - 1) < 1e-12
    assert all(abs(e / 50_000 - 1) <= 0.05 for e in per) and all(abs(e / 100_000 - 1) <= 0.05 for e in per2)


def test_merge_is_the_element_wise_max():
    rng = np.random.default_rng(3)
    P = 5
    a = rng.integers(0, 22, size=(P, K.M)).astype(np.uint64)
    b = rng.integers(0, 22, size=(P, K.M)).astype(np.uint64)
    acc = a.copy()
    assert kta.merge_key_sketch(acc, b, P) is acc
    assert np.array_equal(acc, np.maximum(a, b)) and np.array_equal(acc, K.merge(a, b))
    i64 = a.view(np.int64).copy()
    kta.merge_key_sketch(i64, b, P)
    assert np.array_equal(i64.view(np.uint64), np.maximum(a, b))
    with pytest.raises(ValueError):
        kta.merge_key_sketch(a.copy(), b[:2], P)


# ------------------------------------------------------------------------------------------ 3. the section
def _counter_vec(keyed):
    P = len(keyed)
    v = np.zeros(P * N.KTA_NCOUNTERS + N.KTA_NGLOBALS, np.uint64)
    v[N.KTA_C_KEY_NON_NULL:P * N.KTA_NCOUNTERS:N.KTA_NCOUNTERS] = keyed
    v[N.KTA_C_TOTAL:P * N.KTA_NCOUNTERS:N.KTA_NCOUNTERS] = np.asarray(keyed) * 2 + 1
    return v


@pytest.mark.parametrize("case", ["columns", "empty_partition", "no_keys", "saturated", "one_partition"])
def test_render_distinct_keys_matches_the_python_restatement(case):
    rng = np.random.default_rng(17)
    if case == "columns":
        P = 6
        cols = random_cols(rng, 30000, P, key_space=4000)
        sk = K.sketch(cols, P)
        keyed = np.array([((cols["partition"] == p) & (cols["key_len"] >= 0)).sum() for p in range(P)], np.uint64)
    elif case == "empty_partition":
        P = 4
        h = _distinct_hashes(5000, 9)
        part = np.arange(5000) % 3                 # partition 3 never keyed
        sk = K.sketch_from_hashes(part, h, P)
        keyed = np.array([np.sum(part == p) * 3 for p in range(P)], np.uint64)
    elif case == "no_keys":
        P = 3
        sk = np.zeros((P, K.M), np.uint64)
        keyed = np.zeros(P, np.uint64)
    elif case == "saturated":
        P = 2
        sk = np.full((P, K.M), 21, np.uint64)
        keyed = np.array([5, 7], np.uint64)
    else:
        P = 1
        sk = K.sketch_from_hashes(np.zeros(1, np.int64), np.array([12345], np.uint64), 1)
        keyed = np.array([1_000_000], np.uint64)
    text = kta.render_distinct_keys(sk, _counter_vec(keyed), P)
    assert text == K.section(sk, keyed)
    assert text.startswith(K.TITLE) and text.endswith("=" * 120 + "\n")
    assert "not part of the reference report" in text.splitlines()[0]
    assert re.search(r"^\| Topic ", text, flags=re.M)


def test_render_distinct_keys_buffer_contract():
    P = 2
    sk = np.zeros((P, K.M), np.uint64)
    sk[0, :10] = 1
    cv = _counter_vec([10, 0])
    lib = N.load()
    import ctypes as C
    n = C.c_size_t()
    v = np.ascontiguousarray(sk.reshape(-1))
    assert lib.kta_render_distinct_keys(C.c_void_p(v.ctypes.data), C.c_void_p(cv.ctypes.data), P, None, 0,
                                        C.byref(n)) == N.KTA_OK
    full = kta.render_distinct_keys(sk, cv, P)
    assert n.value == len(full)
    buf = C.create_string_buffer(20)
    assert lib.kta_render_distinct_keys(C.c_void_p(v.ctypes.data), C.c_void_p(cv.ctypes.data), P, buf, 20,
                                        C.byref(n)) == N.KTA_OK
    assert buf.value.decode() == full[:19] and n.value == len(full)
    assert lib.kta_render_distinct_keys(None, C.c_void_p(cv.ctypes.data), P, None, 0, C.byref(n)) == N.KTA_ERR_INVALID


# ------------------------------------------------------------------------------------------ 4. ABI, CLI
def test_new_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "kta_hip.h")).read()
    assert re.search(r"#define KTA_FLAG_KEY_SKETCH 8u\b", header)
    assert re.search(r"#define KTA_SKETCH_LOG2 12\b", header)
    assert re.search(r"#define KTA_SKETCH_MAX_PARTITIONS 16384\b", header)
    assert re.search(r"#define KTA_ABI_VERSION 7\b", header)
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = N.load()
    for name in NEW_EXPORTS:
        assert re.search(r"^int\s+%s\s*\(" % name, text, flags=re.M), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    assert lib.kta_abi_version() == 7


def test_cli_refuses_distinct_keys_beyond_16384_partitions_before_any_context(tmp_path):
    """More partitions than the sketch admits: a clear message and exit 2 before a context exists (so on a machine
    without a GPU as well); the same topic without the knob goes on to the reference's own checks."""
    n = N.KTA_SKETCH_MAX_PARTITIONS + 1
    d = tmp_path / "s"
    d.mkdir()
    for p in range(n):
        (d / ("%d" % p)).write_bytes(b"")
    src = "segment://" + ",".join("s/%d" % p for p in range(n))
    r = subprocess.run([CLI, "-t", "wide", "-b", src, "--librdkafka", "kta.distinct_keys=1"], capture_output=True,
                       text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 2 and r.stdout == ""
    assert "kta.distinct_keys=1" in r.stderr and "at most 16384" in r.stderr and str(n) in r.stderr
    r = subprocess.run([CLI, "-t", "wide", "-b", src], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 254 and "no content" in r.stderr               # main.rs:98-101, unchanged


def test_cli_help_is_unchanged_by_the_distinct_keys_knob():
    plain = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    knob = subprocess.run([CLI, "--librdkafka", "kta.distinct_keys=1", "--help"], capture_output=True, text=True, timeout=60)
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
        P = 5
        cols = random_cols(np.random.default_rng(41), 20000, P, key_space=5000)      # the same topic on every rank
        mine = [cols["partition"] % world == r for r in range(world)]
        sks = [K.sketch({k: (v[m] if k != "key_bytes" else v) for k, v in cols.items()}, P) for m in mine]
        t = torch.from_numpy(sks[rank].reshape(-1).view(np.int64).copy())
        from kafka_topic_analyzer_amd import distributed as D
        D.allreduce_key_sketch_vector(t)
        whole = K.sketch(cols, P)
        merged = sks[0].copy()
        for s in sks[1:]:
            kta.merge_key_sketch(merged, s, P)
        ok = np.array_equal(t.numpy().view(np.uint64).reshape(P, -1), whole) and np.array_equal(merged, whole) and \
            bool(sks[rank].any())
        q.put((rank, ok))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_allreduce_key_sketch_vector_over_gloo_equals_the_merge(world):
    import multiprocessing as mp
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

"""CPU tests of the hot-key sketch (KTA_FLAG_HOT_KEYS; no reference counterpart): the host-only readout, merge and section
against the independent restatement in tests/hot_keys_py.py, the guaranteed bounds on planted mixes, the inverse of
fmix32, the new exports, the CLI's refusal of a bad K (before any context, so without a GPU), and the torch twin of the
exchange over gloo."""
import os
import re
import socket
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import hot_keys_py as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
NEW_EXPORTS = ("kta_get_hot_keys", "kta_exchange_hot_keys", "kta_hot_keys_result_vector", "kta_merge_hot_keys",
               "kta_hot_keys_recover", "kta_get_hot_key_exemplars", "kta_hot_keys_info", "kta_set_hot_flush_rounds",
               "kta_render_hot_keys")


def _planted(seed, n=1 << 20, background=200_000, shares=(0.10, 0.03, 0.01), zipf=None):
    """(hashes, counts, {planted hash: its records}): planted keys over a background of distinct hashes, uniform or Zipf."""
    rng = np.random.default_rng(seed)
    h = np.unique(rng.integers(0, 1 << 32, size=background + len(shares) + 64, dtype=np.uint64))
    rng.shuffle(h)
    planted, back = h[:len(shares)], h[len(shares):len(shares) + background]
    pc = np.array([int(n * s) for s in shares], np.uint64)
    left = n - int(pc.sum())
    if zipf is None:
        draw = rng.integers(0, len(back), size=left)
    else:
        w = 1.0 / np.arange(1, len(back) + 1) ** zipf
        draw = rng.choice(len(back), size=left, p=w / w.sum())
    bc = np.bincount(draw, minlength=len(back)).astype(np.uint64)
    hashes = np.concatenate([planted, back[bc > 0]])
    counts = np.concatenate([pc, bc[bc > 0]])
    return hashes, counts, {int(k): int(c) for k, c in zip(planted, pc)}


def _random_vector(rng):
    """Sums no record set of this size could be counted into: a few dozen hashes with up to 2^40 records each, and on top
    of them sparse cells of arbitrary totals and bit counts (no larger than the totals: what the readout admits)."""
    vec = H.vector_from_pairs(rng.integers(0, 1 << 32, size=40, dtype=np.uint64), rng.integers(1, 1 << 40, size=40, dtype=np.uint64))
    T = np.where(rng.random((H.ROWS, H.CELLS)) < 0.97, 0, rng.integers(0, 1 << 36, size=(H.ROWS, H.CELLS))).astype(np.uint64)
    frac = rng.random((H.ROWS, H.CELLS, H.BITS))
    vec[:, :, 0] += T
    vec[:, :, 1:] += np.minimum((T[:, :, None].astype(np.float64) * frac).astype(np.uint64), T[:, :, None])
    return vec


def _cases():
    rng = np.random.default_rng(7)
    one = H.vector_from_pairs([H.fnv1a(b"the one key")], [12345])
    out = {"empty": np.zeros((H.ROWS, H.CELLS, H.WORDS), np.uint64), "one key": one}
    for name, kw in (("planted", {}), ("planted zipf 0.8", {"zipf": 0.8}), ("planted zipf 1.1", {"zipf": 1.1}),
                     ("small", {"n": 60000, "background": 9000})):
        h, c, _ = _planted(11, **kw)
        out[name] = H.vector_from_pairs(h, c)
    for k in range(3):
        out["random %d" % k] = _random_vector(rng)
    return out


CASES = _cases()


# ------------------------------------------------------------------------------------------ 1. the restatement itself
def test_fmix32_inverse_round_trips():
    rng = np.random.default_rng(3)
    hs = [0, 1, 0xFFFFFFFF, 0x811C9DC5] + [int(v) for v in rng.integers(0, 1 << 32, size=2000)]
    x = H.fmix32(np.array(hs, np.uint64))
    assert [H.fmix32_inverse(int(v)) for v in x] == hs
    # the library's inverse: a vector of one hash reports exactly that hash
    for h in hs[:200]:
        found, keyed = kta.recover_hot_keys(H.vector_from_pairs([h], [7]), 4)
        assert found == [(h, 7, 7)] and keyed == 7


def test_rows_put_x_together_again():
    x = np.random.default_rng(4).integers(0, 1 << 32, size=5000, dtype=np.uint64)
    for row in range(H.ROWS):
        cell, y = H.cell_and_rest(x, row)
        assert int(y.max()) < 1 << 22 and int(cell.max()) < 1024
        assert np.array_equal(H.x_of(row, cell, y), x)


def test_vector_from_hashes_and_from_pairs_agree():
    rng = np.random.default_rng(5)
    h = rng.integers(0, 1 << 32, size=300, dtype=np.uint64)
    recs = h[rng.integers(0, 300, size=20000)]
    u, c = np.unique(recs, return_counts=True)
    a, b = H.vector_from_hashes(recs), H.vector_from_pairs(u, c)
    assert np.array_equal(a, b) and int(a[0, :, 0].sum()) == int(a[1, :, 0].sum()) == 20000


# ------------------------------------------------------------------------------------------ 2. readout, merge, section
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("K", [1, 10, 64])
def test_recover_equals_the_restatement(name, K):
    vec = CASES[name]
    got, keyed = kta.recover_hot_keys(vec, K)
    want, want_keyed = H.recover(vec, K)
    assert keyed == want_keyed and got == want
    assert len(got) <= K
    if name in ("empty",):
        assert got == [] and keyed == 0


@pytest.mark.parametrize("kw", [{}, {"zipf": 0.8}, {"zipf": 1.1}, {"n": 60000, "background": 9000}])
@pytest.mark.parametrize("seed", [1, 2])
def test_planted_keys_are_reported_within_their_bounds(kw, seed):
    h, c, planted = _planted(seed, **kw)
    truth = {int(k): int(v) for k, v in zip(h, c)}
    found, keyed = kta.recover_hot_keys(H.vector_from_pairs(h, c), 64)
    assert keyed == int(c.sum())
    by_hash = {e[0]: e for e in found}
    for k, n in planted.items():
        assert k in by_hash, (hex(k), n)
    for hash_, upper, lower in found:
        # the guarantee holds for every hash, reported or not: one absent from the data has true count 0
        assert lower <= truth.get(hash_, 0) <= upper, (hex(hash_), lower, truth.get(hash_, 0), upper)
        assert upper * 512 >= keyed
    assert [e[1] for e in found] == sorted((e[1] for e in found), reverse=True)


def test_recover_refuses_a_vector_no_record_set_leaves():
    vec = CASES["one key"].copy()
    cell = int(np.nonzero(vec[0, :, 0])[0][0])
    vec[0, cell, 5] = vec[0, cell, 0] + np.uint64(1)
    with pytest.raises(kta.KtaError):
        kta.recover_hot_keys(vec, 4)
    with pytest.raises(kta.KtaError):
        kta.render_hot_keys(vec, None, 4)
    with pytest.raises(ValueError):
        kta.recover_hot_keys(np.zeros(17, np.uint64), 4)


def test_merge_is_the_word_wise_sum():
    a, b = CASES["planted"].copy(), CASES["random 0"]
    want = H.merge(a, b)
    assert kta.merge_hot_keys(a, b) is a and np.array_equal(a, want)
    h, c, _ = _planted(21, n=50000, background=3000)
    half = len(h) // 2
    parts = H.vector_from_pairs(h[:half], c[:half])
    kta.merge_hot_keys(parts, H.vector_from_pairs(h[half:], c[half:]))
    assert np.array_equal(parts, H.vector_from_pairs(h, c))


def _exemplar_table(keys):
    t = np.zeros(H.ROWS * H.CELLS, kta.HOT_EXEMPLAR_DTYPE)
    for i, key in enumerate(keys):
        h = H.fnv1a(key)
        x = int(H.fmix32(np.array([h], np.uint64))[0])
        at = (x & 1023) if i % 2 == 0 else 1024 + ((x >> 10) & 1023)     # either of the key's two slots
        t[at]["hash"], t[at]["key_len"], t[at]["valid"] = h, len(key), 1
        t[at]["bytes"][:min(len(key), 32)] = np.frombuffer(key[:32], np.uint8)
    return t


def test_render_equals_the_restatement():
    for name, vec in CASES.items():
        for K in (1, 10, 64):
            assert kta.render_hot_keys(vec, None, K) == H.section(vec, K), (name, K)
    assert kta.render_hot_keys(CASES["empty"], None, 5) == H.title(5) + "No key holds 1/512 of the 0 keyed records.\n"
    keys = [b"plain-key", b"", b"back\\slash and \x00\xff bytes", b"x" * 32, b"y" * 40, b"no exemplar for this one"]
    counts = [5000, 4000, 3000, 2000, 1000, 900]
    vec = H.vector_from_pairs([H.fnv1a(k) for k in keys], counts)
    table = _exemplar_table(keys[:-1])
    by_hash = {H.fnv1a(k): k for k in keys[:-1]}
    text = kta.render_hot_keys(vec, table, 10)
    assert text == H.section(vec, 10, by_hash)
    assert text == H.section(vec, 10, H.exemplar_keys(table))
    lines = text.splitlines()
    assert "| plain-key " in lines[4] and "| 5000 " in lines[4] and "| 31.45 " in lines[4]
    assert "back\\x5Cslash and \\x00\\xFF bytes" in text and ("y" * 32 + "...") in text and ("x" * 32 + " ") in text
    assert re.search(r"\| 6 \| - +\| %08x \| 900 +\| 900 " % H.fnv1a(keys[-1]), text)
    assert text.endswith("=" * 120 + "\n")
    # a slot that holds another hash is no exemplar
    table["hash"] ^= 1
    assert kta.render_hot_keys(vec, table, 10) == H.section(vec, 10)
    for bad in (0, 65):
        with pytest.raises(kta.KtaError):
            kta.render_hot_keys(vec, None, bad)


# ------------------------------------------------------------------------------------------ 3. ABI, CLI
def test_new_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "kta_hip.h")).read()
    assert re.search(r"#define KTA_FLAG_HOT_KEYS 16u\b", header)
    assert re.search(r"#define KTA_HOT_ROWS 2\b", header) and re.search(r"#define KTA_HOT_CELLS 1024\b", header)
    assert re.search(r"#define KTA_HOT_WORDS 23\b", header)
    assert re.search(r"#define KTA_ABI_VERSION 7\b", header)
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = N.load()
    for name in NEW_EXPORTS:
        assert re.search(r"^int\s+%s\s*\(" % name, text, flags=re.M), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    assert lib.kta_abi_version() == 7
    assert N.KTA_HOT_VECTOR_WORDS == 47104 and kta.HOT_EXEMPLAR_DTYPE.itemsize == 48


@pytest.mark.parametrize("value", ["0", "65", "ten", ""])
def test_cli_refuses_a_bad_hot_keys_count_before_any_context(value):
    r = subprocess.run([CLI, "-t", "c2", "-b", "synthetic://c2?records=1000", "--librdkafka", "kta.hot_keys=" + value],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and r.stdout == "" and "kta.hot_keys=" in r.stderr and "1 to 64" in r.stderr


def test_cli_help_is_unchanged_by_the_hot_keys_knob():
    plain = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    knob = subprocess.run([CLI, "--librdkafka", "kta.hot_keys=5", "--help"], capture_output=True, text=True, timeout=60)
    assert plain.returncode == knob.returncode == 0 and knob.stdout == plain.stdout


# ------------------------------------------------------------------------------------------ 4. torch twin (gloo)
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
        h, c, _ = _planted(41, n=40000, background=5000)          # the same topic on every rank
        mine = np.arange(len(h)) % world == rank
        own = H.vector_from_pairs(h[mine], c[mine])
        t = torch.from_numpy(own.reshape(-1).view(np.int64).copy())
        from kafka_topic_analyzer_amd import distributed as D
        D.allreduce_hot_keys_vector(t)
        whole = H.vector_from_pairs(h, c)
        q.put((rank, bool(np.array_equal(t.numpy().view(np.uint64).reshape(whole.shape), whole)) and bool(own.any())))
    finally:
        dist.destroy_process_group()


def test_allreduce_hot_keys_vector_over_gloo_world_2():
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

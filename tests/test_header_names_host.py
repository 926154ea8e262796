"""CPU tests of the header-name section (KTA_FLAG_HEADER_NAMES; no reference counterpart): kta_header_names_host — the
section's rule over the records of a raw record set, compressed batches inflated on the host — against the restatement in
tests/header_names_py.py on blobs of every codec and on every kind of bad header section; the read-off and the rendered section
against the restatement's on boundary tables (empty, one name, 1024 names, a pair that collides in both rows, an inconsistent
L); the rendered section against a golden text; the identities with and without a payload vector, each broken by one flipped
word; the merge; the exports; the CLI's refusals that need no device; the torch twin of the exchange over gloo; and the rule's
own source (csrc/kta_header_names.h) run natively under AddressSanitizer + UBSan (tests/native/header_names_check.cpp, a
program of its own)."""
import os
import re
import socket
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
from kafka_topic_analyzer_amd import distributed
import header_names_blobs as HB
import header_names_py as H
import payload_blobs as B
import payload_py as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
CSRC = os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "header_names_section.txt")
NEW_EXPORTS = ("kta_get_header_names", "kta_exchange_header_names", "kta_header_names_result_vector", "kta_header_names_vector",
               "kta_merge_header_names", "kta_get_header_name_table", "kta_header_names_identities", "kta_header_names_list",
               "kta_header_names_host", "kta_render_header_names")
P = 4


def _holds(v, payload=None, P_=P):
    bad = [n for n, ok in H.identities(v, payload, P_) if not ok]
    assert not bad, bad
    assert kta.header_names_identities(v, payload, P_ if payload is not None else 0)


def _same_list(v, table=None):
    """kta_header_names_list and kta_render_header_names against the restatement's list and section"""
    found, uo, uv = H.list_names(v)
    got = kta.header_names_list(v, table)
    assert [n[:5] for n in got["names"]] == found and (got["unresolved_occurrences"], got["unresolved_value_bytes"]) == (uo, uv)
    names = {} if table is None else H.table_names(table)
    assert all(n[5] == names.get(n[0]) for n in got["names"])
    for cap in (256, 3):
        assert kta.render_header_names(v, table, cap) == H.section(v, names, cap)
    return got


def _table_of(names_values):
    """(vector, name table) of [(name, value | None), ...] by the restatement and a first-writer-wins table of its own"""
    v, table = np.zeros(H.WORDS, np.uint64), np.zeros(2048, kta.HEADER_NAME_DTYPE)
    for name, value in names_values:
        H.add_occurrence(v, name, value)
        h = H.fnv1a(name)
        for r in range(2):
            e = table[r * 1024 + H.cell(r, h)]
            if e["state"] == 0:
                e["hash"], e["name_len"], e["state"] = h, len(name), 2
                e["bytes"][:min(len(name), 48)] = np.frombuffer(name[:48], np.uint8)
    return v, table


# ------------------------------------------------------------------------------------------ 1. the rule
def test_host_rule_equals_the_restatement_on_blobs_of_every_codec():
    acc, table, pl, sets, seen = None, None, np.zeros(R.words(P), np.uint64), [], {}
    for part, comp in enumerate((None, "gzip", "snappy", "lz4", "zstd", B.CODECS)):
        blob, raw = B.mixed(7, 40, seed=part, compression=comp)
        acc, table = kta.header_names_host(blob, part % P, P, vec=acc, table=table)
        kta.payload_host(blob, part % P, P, vec=pl)
        sets.append((blob, part % P, raw, set()))
    want = H.restate(sets, P, seen=seen)
    assert np.array_equal(acc, want) and want[H.OCC] and want[H.NULLS]
    _holds(acc)
    _holds(acc, pl)                                                                  # the identities with the payload vector of the same run
    H.check_table(table, seen)
    got = _same_list(acc, table)
    assert [n[5] for n in got["names"]] == [b"h0", b"h1", b"h2"] and got["unresolved_occurrences"] == 0
    d = kta.split_header_names(acc, table)
    assert d["occurrences"] == want[H.OCC] and d["looked"] == want[H.LOOKED] and d["table"].shape == (2, 1024, 36) and d["names"] == got
    assert not kta.header_names_host(blob, P, P)[0].any() and not kta.header_names_host(blob, -1, P)[0].any()       # outside [0, P)


@pytest.mark.parametrize("kind", sorted(B.BAD_HEADERS))
def test_every_bad_header_kind_adds_nothing(kind):
    good = [B.record(i, B.framed(9), headers=[(b"a", b"bc"), (b"", None)]) for i in range(5)]
    for place in (0, 2, 4):
        recs = list(good)
        recs[place] = B.record(place, b'{"v":1}', raw_headers=B.BAD_HEADERS[kind])
        blob, raw = B.join([B.batch(0, recs, compression="lz4" if place else None)])
        got, _ = kta.header_names_host(blob, 1, P)
        assert np.array_equal(got, H.restate([(blob, 1, raw, set())], P)), (kind, place)
        assert [int(x) for x in got[:8]] == [8, 4, 8, 4, 4, 4, 0, 0]                  # the four good records alone
        _holds(got, kta.payload_host(blob, 1, P))


def test_large_records_and_window_edge_blobs_on_the_host():
    recs = B.large_records()
    for blob, raw in (B.join([B.batch(0, recs), B.batch(40, recs, compression="snappy")]), HB.astride("name")[:2], HB.astride("value")[:2],
                      HB.hot_wave(), HB.distinct_names(200)[:2]):
        seen = {}
        got, table = kta.header_names_host(blob, 0, P)
        assert np.array_equal(got, H.restate([(blob, 0, raw, set())], P, seen=seen))
        H.check_table(table, seen)
        _same_list(got, table)


# ------------------------------------------------------------------------------------------ 2. the read-off on boundary tables
def test_list_and_render_of_an_empty_vector_and_of_one_name():
    v = np.zeros(H.WORDS, np.uint64)
    got = _same_list(v)
    assert got["names"] == [] and "0 names listed" in kta.render_header_names(v) and "Unresolved" not in kta.render_header_names(v)
    v, table = _table_of([(b"", None)])
    got = _same_list(v, table)
    assert got["names"] == [(0x811C9DC5, 1, 0, 0, 1, b"")]
    text = kta.render_header_names(v, table)
    assert text.count("n/a") == 3 and "| 811c9dc5 " in text                         # no record with headers, no value that is not null, no header byte
    assert "#811c9dc5" in kta.render_header_names(v)                                # without a table: the hash stands for the name
    with pytest.raises(ValueError):
        kta.render_header_names(v[:-1])
    with pytest.raises(ValueError):
        kta.header_names_list(v, table[:-1])


def test_list_and_render_of_1024_names():
    v, table = _table_of([(b"name-%d" % i, None if i % 5 == 0 else b"v" * (i % 7)) for i in range(1024) for _ in range(i % 3 + 1)])
    got = _same_list(v, table)
    assert len(got["names"]) > 512                                                 # 1024 names in 1024 cells: whatever the peel leaves is a remainder
    assert sum(n[1] for n in got["names"]) + got["unresolved_occurrences"] == v[H.OCC]
    assert sum(n[3] for n in got["names"]) + got["unresolved_value_bytes"] == v[H.VALB]
    text = kta.render_header_names(v, table)
    assert "... and %d more\n" % (len(got["names"]) - 256) in text and ("Unresolved: " in text) == (got["unresolved_occurrences"] > 0)


def test_names_that_share_cells_and_an_inconsistent_l():
    one, both = HB.colliding_names()
    v, table = _table_of([(one[i % 2], b"x" * (i % 3)) for i in range(20)])
    got = _same_list(v, table)
    assert sorted(n[5] for n in got["names"]) == sorted(one) and got["unresolved_occurrences"] == 0
    v, table = _table_of([(both[i % 2], b"x" * (i % 3)) for i in range(20)] + [(b"other", b"")])
    got = _same_list(v, table)
    assert [n[5] for n in got["names"]] == [b"other"] and (got["unresolved_occurrences"], got["unresolved_value_bytes"]) == (20, 19)
    v, table = _table_of([(b"abc", b"12")] * 2)
    assert len(_same_list(v, table)["names"]) == 1
    for r in range(2):
        v[H.cell_at(r, H.cell(r, H.fnv1a(b"abc"))) + H.L] += 1                       # 7 name bytes in 2 occurrences: no name has that
    got = _same_list(v, table)
    assert got["names"] == [] and (got["unresolved_occurrences"], got["unresolved_value_bytes"]) == (2, 4)


# ------------------------------------------------------------------------------------------ 3. golden, identities, merge
def _golden():
    one, both = HB.colliding_names()
    occ = [(b"traceparent", b"00-0af7651916cd43dd8448eb211c80319c-b7ad6b7169203331-01")] * 40 + [(b"correlation-id", b"c" * 36)] * 40
    occ += [(b"__replicated-from", None)] * 7 + [(b"__replicated-from", b"east")] * 3 + [(b"", b"")] * 2
    occ += [(b"x" * 49, b"long")] * 4 + [(b"y" * 48, None)] + [(b"bin\x00\\\xff", b"\x01\x02")] * 5
    occ += [(both[i % 2], b"zz") for i in range(6)]
    v, table = _table_of(occ)
    v[H.WITH], v[H.LOOKED] = 45, 60
    table[H.cell(0, H.fnv1a(b"correlation-id"))]["state"] = 0                         # this name lost both of its slots
    table[1024 + H.cell(1, H.fnv1a(b"correlation-id"))]["state"] = 0
    return v, table


def test_rendered_section_matches_the_golden_text():
    v, table = _golden()
    _holds(v)
    text = kta.render_header_names(v, table)
    assert text == open(GOLDEN).read() == H.section(v, H.table_names(table))
    assert "kta.headers=1; not part of the reference report" in text.splitlines()[0]
    assert "| " + "x" * 48 + "... " in text and "| " + "y" * 48 + " " in text and "bin\\x00\\x5C\\xFF" in text and "| #" in text
    assert "Unresolved: 6 occurrences, 12 value bytes in table cells that hold several names" in text and text.endswith("=" * 120 + "\n")
    assert text.count("n/a") == 1                                                   # the name whose only value is null has no mean value


def test_identities_broken_by_one_word_with_and_without_a_payload_vector():
    blob, raw = B.mixed(9, 20, seed=3)
    v, _ = kta.header_names_host(blob, 2, P)
    pl = kta.payload_host(blob, 2, P)
    _holds(v)
    _holds(v, pl)
    used = np.flatnonzero(v[H.GLOBALS:])[0] + H.GLOBALS
    for word in (H.OCC, H.NAMEB, H.VALB, H.NULLS, 6, 7, used):
        w = v.copy()
        w[word] += 1
        assert not kta.header_names_identities(w) and not all(ok for _, ok in H.identities(w)), word
    for word in (H.WITH, H.LOOKED):                                                  # these two only the payload vector pins down
        w = v.copy()
        w[word] += 1
        assert not kta.header_names_identities(w, pl, P) and not all(ok for _, ok in H.identities(w, pl, P)), word
    for col in (R.HEADERS, R.HKEY, R.HVAL, R.HNULL, R.WITH, R.BAD):
        q = pl.copy()
        q[2 * R.PW + col] += 1
        assert not kta.header_names_identities(v, q, P) and not all(ok for _, ok in H.identities(v, q, P)), col
    with pytest.raises(ValueError):
        kta.header_names_identities(v, pl[:-1], P)


def test_merge_adds_every_word():
    a, _ = kta.header_names_host(B.mixed(5, 9, seed=1)[0], 0, P)
    b, _ = kta.header_names_host(B.mixed(6, 7, seed=2)[0], 1, P)
    acc = a.copy()
    assert kta.merge_header_names(acc, b) is acc and np.array_equal(acc, a + b)
    _holds(acc)
    i64 = a.view(np.int64).copy()
    kta.merge_header_names(i64, b)
    assert np.array_equal(i64.view(np.uint64), a + b)
    with pytest.raises(ValueError):
        kta.merge_header_names(acc, b[:-1])


# ------------------------------------------------------------------------------------------ 4. exports, CLI
def test_new_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "kta_hip.h")).read()
    m = re.search(r"#define KTA_FLAG_HEADER_NAMES (\w+?)[uU]\s", header)
    assert m and int(m.group(1), 0) == 0x800 == N.KTA_FLAG_HEADER_NAMES
    others = [int(v, 0) for v in re.findall(r"#define KTA_FLAG_(?!HEADER_NAMES)\w+ +\(?(\w+?)[uU]\b", header)]
    assert 0x800 not in others and all(f & 0x800 == 0 for f in others)              # bit 11 was free
    assert re.search(r"#define KTA_ABI_VERSION 7\b", header) and N.load().kta_abi_version() == 7
    assert (N.KTA_HEADER_NAMES_WORDS, N.KTA_HEADER_NAMES_GLOBALS, N.KTA_HEADER_NAMES_ROWS, N.KTA_HEADER_NAMES_CELLS, N.KTA_HEADER_NAMES_CELL_WORDS,
            N.KTA_HEADER_NAME_BYTES) == (H.WORDS, H.GLOBALS, H.ROWS, H.CELLS, H.CW, H.KEPT)
    assert kta.HEADER_NAME_DTYPE.itemsize == 64 == N.C.sizeof(N.KtaHeaderName) and N.C.sizeof(N.KtaHeaderNameRow) == 88
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    kafka_text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kta_kafka.h")).read(), flags=re.S)
    lib = N.load()
    for name in NEW_EXPORTS:
        assert re.search(r"^int\s+%s\s*\(" % name, text, flags=re.M), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    assert re.search(r"^int\s+kta_header_names_info\s*\(", kafka_text, flags=re.M) and hasattr(lib, "kta_header_names_info")
    for name in ("split_header_names", "merge_header_names", "header_names_identities", "header_names_list", "header_names_host", "render_header_names"):
        assert name in kta.__all__ and callable(getattr(kta, name))
    for name in ("header_names", "exchange_header_names", "header_name_table", "header_names_result_vector", "header_names_vector", "header_names_info"):
        assert callable(getattr(kta.HipMetricHandler, name))
    assert callable(distributed.allreduce_header_names_vector)


def _cli(*knobs, src="synthetic://c2?records=100", flags=()):
    return subprocess.run([CLI, "-t", "x", "-b", src, *flags, "--librdkafka", ",".join(knobs)], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value", ["2", "", "yes"])
def test_cli_refuses_a_value_other_than_0_or_1(value):
    r = _cli("kta.headers=" + value)
    assert r.returncode == 2 and "kta.headers=%s: expected 0 or 1" % value in r.stderr and r.stdout == "", (r.returncode, r.stderr)
    assert len(r.stderr.strip().splitlines()) == 1


@pytest.mark.parametrize("src,knobs", [("synthetic://c2?records=100", ()), ("dump:///nonexistent.dump", ()), ("localhost:1", ()),
                                       ("segment:///nonexistent.log", ("kta.per_message=1",))])
def test_cli_refuses_sources_that_do_not_hold_the_log_bytes(src, knobs):
    """one line that says why, before a broker, a file or a device is asked for anything"""
    r = _cli("kta.headers=1", *knobs, src=src)
    assert r.returncode == 2 and r.stdout == "", (r.returncode, r.stdout, r.stderr)
    lines = r.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("kta.headers=1: needs a segment:// source") and "not the bytes of the log" in lines[0]


def test_cli_help_is_unchanged_by_the_knob():
    plain = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    knob = subprocess.run([CLI, "--librdkafka", "kta.headers=1", "--help"], capture_output=True, text=True, timeout=60)
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
        vecs = [H.restate([s for s in sets if s[1] % world == r], 5) for r in range(world)]
        t = torch.from_numpy(vecs[rank].view(np.int64).copy())
        from kafka_topic_analyzer_amd import distributed as D
        D.allreduce_header_names_vector(t)
        whole = H.restate(sets, 5)
        q.put((rank, bool(np.array_equal(t.numpy().view(np.uint64), whole) and vecs[rank].any() and not np.array_equal(vecs[rank], whole))))
    finally:
        dist.destroy_process_group()


def test_allreduce_header_names_vector_over_gloo_equals_the_unsharded_vector():
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
        distributed.allreduce_header_names_vector(torch.zeros(5, dtype=torch.int64))


# ------------------------------------------------------------------------------------------ 6. the rule's own source
def test_native_check_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/header_names_check.cpp: a program of its own that calls kta_header_names.h, built with the sanitizers and run directly."""
    exe = str(tmp_path / "header_names_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "native", "header_names_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.returncode, r.stdout[-500:], r.stderr[-2000:])

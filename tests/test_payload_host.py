"""CPU tests of the payload section (KTA_FLAG_PAYLOAD; no reference counterpart): kta_payload_host — the section's rule over the
records of a raw record set, compressed batches inflated on the host — against the restatement in tests/payload_py.py on blobs
of every codec and on every kind of bad header section; the schema-id read-off (consecutive ids, shared cells, a peel chain, a
pair that collides in both rows, a cell that spells another cell's id); the merge and the identities, each broken by one
flipped word; the rendered section against a golden text; the CLI's refusals that need no device; the exports; the torch twin
of the exchange over gloo; and the rule's own source (csrc/kta_payload.h) run natively under AddressSanitizer + UBSan
(tests/native/payload_check.cpp, a program of its own)."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
CSRC = os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "payload_section.txt")
NEW_EXPORTS = ("kta_get_payload", "kta_exchange_payload", "kta_payload_result_vector", "kta_payload_vector", "kta_merge_payload",
               "kta_payload_identities", "kta_payload_schema_ids", "kta_payload_host", "kta_render_payload")
P = 4


def _holds(v, P_=P, counters=None):
    bad = [n for n, ok in R.identities(v, P_, counters) if not ok]
    assert not bad, bad
    assert kta.payload_identities(v, P_, counters)


# ------------------------------------------------------------------------------------------ 1. the rule
def test_host_rule_equals_the_restatement_on_blobs_of_every_codec():
    acc, sets = np.zeros(R.words(P), np.uint64), []
    for part, comp in enumerate((None, "gzip", "snappy", "lz4", "zstd", B.CODECS)):
        blob, raw = B.mixed(7, 40, seed=part, compression=comp)
        kta.payload_host(blob, part % P, P, vec=acc)
        sets.append((blob, part % P, raw, set()))
    want = R.restate(sets, P)
    assert np.array_equal(acc, want)
    _holds(acc)
    d = kta.split_payload(acc, P)
    assert d["partitions"][:, R.RECORDS].all() and d["partitions"][:, R.CLASS:R.CLASS + 5].all() and d["partitions"][:, R.BAD].sum() == 0
    assert d["partitions"][:, R.HNULL].sum() > 0 and d["headers_hist"][:4].all() and d["headers_hist"][4:].sum() == 0
    assert {i for i, _, _ in d["schema_ids"]["ids"]} == set(range(100, 107)) | set(range(5000, 5003)) and d["schema_ids"]["unresolved_records"] == 0
    assert kta.payload_host(blob, P, P).sum() == 0 and kta.payload_host(blob, -1, P).sum() == 0       # outside [0, P)


@pytest.mark.parametrize("kind", sorted(B.BAD_HEADERS))
@pytest.mark.parametrize("compression", [None, "lz4"])
def test_every_bad_header_kind_counts_one_bad_record_and_leaves_the_other_words(kind, compression):
    good = [B.record(i, B.framed(9), headers=[(b"a", b"bc"), (b"", None)]) for i in range(5)]
    for place in (0, 2, 4):
        recs = list(good)
        recs[place] = B.record(place, b'{"v":1}', headers=None, raw_headers=B.BAD_HEADERS[kind])
        blob, raw = B.join([B.batch(0, recs, compression=compression)])
        got = kta.payload_host(blob, 1, P)
        assert np.array_equal(got, R.restate([(blob, 1, raw, set())], P)), (kind, place)
        w = got[R.PW:2 * R.PW]
        assert (w[R.RECORDS], w[R.BAD], w[R.CLASS + R.JSON], w[R.CLASS + R.FRAMED]) == (5, 1, 1, 4)
        assert (w[R.WITH], w[R.HEADERS], w[R.HKEY], w[R.HVAL], w[R.HNULL], w[R.WIRE]) == (4, 8, 4, 8, 4, 4 * 8)    # the four good records alone
        assert got[R.PW * P + 2] == 4 and got[R.PW * P:R.PW * P + R.HIST].sum() == 4
        _holds(got)


def test_a_record_with_bad_framing_ends_its_batch_and_the_next_batch_counts():
    recs = [B.record(i, b"v%d" % i) for i in range(6)]
    broken = bytearray(recs[3])
    broken[0] += 100                                                               # a length that overruns the batch
    first = B.batch(0, recs[:3] + [bytes(broken)] + recs[4:])
    blob, raw = B.join([first, B.batch(6, recs[:2])])
    got = kta.payload_host(blob, 0, P)
    assert np.array_equal(got, R.restate([(blob, 0, raw, set())], P)) and got[R.RECORDS] == 3 + 2


# ------------------------------------------------------------------------------------------ 2. the read-off
def _table_of(ids_records_bytes, P_=1):
    """A vector whose framed records are (id, records, bytes per record) — through the restatement's own add."""
    v = np.zeros(R.words(P_), np.uint64)
    for x, n, size in ids_records_bytes:
        value = B.framed(x, b"z" * (size - 5))
        rec = B.record(0, value)
        for _ in range(n):
            R.add_record(v, P_, 0, value, rec, len(rec) - 1, len(rec))
    return v


def _read_off(v, P_=1):
    got, want = kta.payload_schema_ids(v, P_), R.schema_ids(v, P_)
    assert (got["ids"], got["unresolved_records"], got["unresolved_bytes"]) == want
    return got


def _same_cell(row, a, avoid=()):
    """the next id after `a` that shares a's cell in `row` and no cell with it in the other row"""
    x = a + 1
    while R.cell(row, x) != R.cell(row, a) or R.cell(1 - row, x) == R.cell(1 - row, a) or x in avoid:
        x += 1
    return x


def test_three_hundred_consecutive_ids_are_exact():
    v = _table_of([(70000 + i, 1 + i % 3, 5 + i % 11) for i in range(300)])
    got = _read_off(v)
    assert sorted(got["ids"]) == sorted((70000 + i, 1 + i % 3, (1 + i % 3) * (5 + i % 11)) for i in range(300))
    assert got["unresolved_records"] == 0 and got["unresolved_bytes"] == 0
    assert [r for _, r, _ in got["ids"]] == sorted((r for _, r, _ in got["ids"]), reverse=True)


def test_two_ids_that_share_a_row_0_cell_are_both_recovered():
    v = _table_of([(12, 3, 9), (12 + 1024, 5, 6)])
    assert R.cell(1, 12) != R.cell(1, 12 + 1024)
    assert _read_off(v)["ids"] == [(12 + 1024, 5, 30), (12, 3, 27)]


def test_a_peel_chain_recovers_all_three():
    a = 4242
    b = _same_cell(0, a)                       # a, b share a row-0 cell
    c = _same_cell(1, b, avoid=(a,))           # b, c share a row-1 cell; a is alone in row 1
    assert R.cell(1, a) not in (R.cell(1, b),) and R.cell(0, c) != R.cell(0, a)
    got = _read_off(_table_of([(a, 1, 5), (b, 2, 6), (c, 3, 7)]))
    assert got["ids"] == [(c, 3, 21), (b, 2, 12), (a, 1, 5)] and got["unresolved_records"] == 0


def double_collision(a=31337):
    """a and a + 1024 k with equal fmix32 & 1023: they share their cell in both rows"""
    k = 1
    while R.cell(1, a + 1024 * k) != R.cell(1, a):
        k += 1
    return a, a + 1024 * k


def test_two_ids_that_collide_in_both_rows_are_not_listed_and_the_remainder_is_exact():
    a, b = double_collision()
    got = _read_off(_table_of([(a, 4, 10), (b, 7, 13), (99, 2, 8)]))
    assert got["ids"] == [(99, 2, 16)]
    assert got["unresolved_records"] == 11 and got["unresolved_bytes"] == 4 * 10 + 7 * 13


def test_a_cell_whose_bit_counts_spell_an_id_of_another_cell_is_not_pure():
    v = np.zeros(R.words(1), np.uint64)
    at = R.cell_at(1, 0, 9)
    v[at], v[at + 1], v[at + 2 + 1] = 4, 40, 4                                      # cell 9 of row 0 spells id 2: cell 2's
    got = _read_off(v)
    assert got["ids"] == [] and got["unresolved_records"] == 4 and got["unresolved_bytes"] == 40


# ------------------------------------------------------------------------------------------ 3. merge, identities, rendering
def _golden_vector():
    recs = []
    for i in range(70):                                                              # 70 ids: more than the section lists
        recs += [B.record(len(recs), B.framed(1000 + i, b"r" * (i % 9)), headers=[(b"trace", b"0123456789abcdef")] * (i % 3))] * (1 + i % 4)
    a, b = double_collision()
    recs += [B.record(0, B.framed(a)), B.record(0, B.framed(b, b"long-body"))] * 2
    p0, raw0 = B.join([B.batch(0, recs)])
    p2, raw2 = B.join([B.batch(0, [B.record(0, None, headers=[(b"h", None)] * 16), B.record(1, b""), B.record(2, b'{"k":1}'),
                                   B.record(3, b"text", raw_headers=B.BAD_HEADERS["absent"]), B.record(4, b"[]", headers=[(b"a", b"b")] * 14)])])
    return R.restate([(p0, 0, raw0, set()), (p2, 2, raw2, set())], 3)


def _golden_counters():
    c = np.zeros(7 * 3 + 8, np.uint64)
    c[0 * 7 + 5], c[0 * 7 + 6], c[2 * 7 + 5], c[2 * 7 + 6] = 181, 2000, 5, 13
    return c


def test_merge_adds_every_word_and_checks_its_arguments():
    blob, raw = B.mixed(3, 20)
    a, b = kta.payload_host(blob, 0, P), kta.payload_host(blob, 3, P)
    acc = a.copy()
    kta.merge_payload(acc, b, P)
    assert np.array_equal(acc, a + b) and np.array_equal(acc, R.restate([(blob, 0, raw, set()), (blob, 3, raw, set())], P))
    _holds(acc)
    assert N.load().kta_merge_payload(acc.ctypes.data, b.ctypes.data, 0) == N.KTA_ERR_INVALID
    assert N.load().kta_merge_payload(acc.ctypes.data, b.ctypes.data, 4097) == N.KTA_ERR_INVALID
    with pytest.raises(ValueError):
        kta.merge_payload(acc, b[:-1], P)


@pytest.mark.parametrize("word", [R.RECORDS, R.CLASS + R.JSON, R.CLASS_BYTES + R.NULL, R.CLASS_BYTES + R.EMPTY, R.WITH, R.BAD, 20,
                                  "hist0", "hist3", "row0T", "row1T", "row0B", "row1B", "bit"])
def test_each_identity_is_broken_by_one_flipped_word(word):
    blob, _ = B.mixed(3, 20)
    v = kta.payload_host(blob, 0, P)
    _holds(v)
    x = int(np.flatnonzero(v[R.cell_at(P, 0, 0):R.cell_at(P, 1, 0):R.CW])[0])          # a row-0 cell that holds an id
    at = {"hist0": R.PW * P, "hist3": R.PW * P + 3, "row0T": R.cell_at(P, 0, x), "row1T": R.cell_at(P, 1, 0), "row0B": R.cell_at(P, 0, x) + 1,
          "row1B": R.cell_at(P, 1, 5) + 1, "bit": R.cell_at(P, 0, x) + 2 + 31}.get(word, word)
    v[at] += 1000
    assert not kta.payload_identities(v, P) and not all(ok for _, ok in R.identities(v, P))


def test_counter_identities_take_the_counter_vector():
    blob, _ = B.mixed(3, 20)
    v = kta.payload_host(blob, 1, P)
    c = np.zeros(7 * P + 8, np.uint64)
    c[7], c[8] = v[R.PW + R.RECORDS], v[R.PW + R.CLASS + R.NULL]
    _holds(v, counters=c)
    c[8] += 1
    assert not kta.payload_identities(v, P, c)
    with pytest.raises(ValueError):
        kta.payload_identities(v, P, c[:-1])


def test_rendered_section_matches_the_golden_text():
    v = _golden_vector()
    _holds(v, 3)
    text = kta.render_payload(v, 3, _golden_counters())
    assert text == open(GOLDEN).read()
    assert "... and 6 more" in text and "Unresolved: 4 records, 48 bytes in table cells that hold several ids" in text
    assert text.count("n/a") == 7 and text.endswith("=" * 120 + "\n")              # the empty partition
    assert "| >=15 " in text and "heuristic" in text and "not a subject's" in text and "header names" in text and "failed batches" in text
    assert kta.render_payload(v, 3).count("n/a") == 7 + 3                            # without counters: no share of the bytes anywhere


def test_render_of_an_empty_vector():
    text = kta.render_payload(np.zeros(R.words(2), np.uint64), 2)
    assert "Schema ids: none" in text and text.count("n/a") == 3 * 7
    with pytest.raises(ValueError):
        kta.render_payload(np.zeros(5, np.uint64), 2)


# ------------------------------------------------------------------------------------------ 4. exports, CLI
def test_new_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "kta_hip.h")).read()
    m = re.search(r"#define KTA_FLAG_PAYLOAD (\w+?)[uU]\s", header)
    assert m and int(m.group(1), 0) == 0x400 == N.KTA_FLAG_PAYLOAD
    others = [int(v, 0) for v in re.findall(r"#define KTA_FLAG_(?!PAYLOAD)\w+ +\(?(\w+?)[uU]\b", header)]
    assert 0x400 not in others and all(f & 0x400 == 0 for f in others)              # bit 10 was free
    assert re.search(r"#define KTA_ABI_VERSION 7\b", header) and N.load().kta_abi_version() == 7
    assert (N.KTA_PAYLOAD_PARTITION_WORDS, N.KTA_PAYLOAD_CLASSES, N.KTA_PAYLOAD_HIST_BINS, N.KTA_PAYLOAD_ROWS, N.KTA_PAYLOAD_CELLS,
            N.KTA_PAYLOAD_CELL_WORDS) == (R.PW, 5, R.HIST, R.ROWS, R.CELLS, R.CW)
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    kafka_text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kta_kafka.h")).read(), flags=re.S)
    lib = N.load()
    for name in NEW_EXPORTS:
        assert re.search(r"^int\s+%s\s*\(" % name, text, flags=re.M), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    assert re.search(r"^int\s+kta_payload_info\s*\(", kafka_text, flags=re.M) and hasattr(lib, "kta_payload_info")
    for name in ("split_payload", "merge_payload", "payload_identities", "payload_schema_ids", "payload_host", "render_payload"):
        assert name in kta.__all__ and callable(getattr(kta, name))
    for name in ("get_payload", "exchange_payload", "payload_result_vector", "payload_vector", "payload_info"):
        assert callable(getattr(kta.HipMetricHandler, name))
    assert callable(distributed.allreduce_payload_vector)


def _cli(*knobs, src="synthetic://c2?records=100", flags=()):
    return subprocess.run([CLI, "-t", "x", "-b", src, *flags, "--librdkafka", ",".join(knobs)], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value", ["2", "", "yes"])
def test_cli_refuses_a_value_other_than_0_or_1(value):
    r = _cli("kta.payload=" + value)
    assert r.returncode == 2 and "kta.payload=%s: expected 0 or 1" % value in r.stderr and r.stdout == "", (r.returncode, r.stderr)
    assert len(r.stderr.strip().splitlines()) == 1


@pytest.mark.parametrize("src,knobs", [("synthetic://c2?records=100", ()), ("dump:///nonexistent.dump", ()), ("localhost:1", ()),
                                       ("segment:///nonexistent.log", ("kta.per_message=1",))])
def test_cli_refuses_sources_that_do_not_hold_the_log_bytes(src, knobs):
    """one line that says why, before a broker, a file or a device is asked for anything"""
    r = _cli("kta.payload=1", *knobs, src=src)
    assert r.returncode == 2 and r.stdout == "", (r.returncode, r.stdout, r.stderr)
    lines = r.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("kta.payload=1: needs a segment:// source") and "not the bytes of the log" in lines[0]


def test_cli_help_is_unchanged_by_the_knob():
    plain = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    knob = subprocess.run([CLI, "--librdkafka", "kta.payload=1", "--help"], capture_output=True, text=True, timeout=60)
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
        vecs = [R.restate([s for s in sets if s[1] % world == r], 5) for r in range(world)]
        t = torch.from_numpy(vecs[rank].view(np.int64).copy())
        from kafka_topic_analyzer_amd import distributed as D
        D.allreduce_payload_vector(t, 5)
        whole = R.restate(sets, 5)
        q.put((rank, bool(np.array_equal(t.numpy().view(np.uint64), whole) and vecs[rank].any() and not np.array_equal(vecs[rank], whole))))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_allreduce_payload_vector_over_gloo_equals_the_unsharded_vector(world):
    pytest.importorskip("torch")
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


def test_allreduce_helper_checks_the_length():
    torch = pytest.importorskip("torch")
    with pytest.raises(AssertionError):
        distributed.allreduce_payload_vector(torch.zeros(5, dtype=torch.int64), 2)


# ------------------------------------------------------------------------------------------ 6. the rule's own source
def test_native_check_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/payload_check.cpp: a program of its own that calls kta_payload.h, built with the sanitizers and run directly."""
    exe = str(tmp_path / "payload_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "native", "payload_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK "), (r.stdout[-500:], r.stderr[-3000:])

"""The compression what-if (KTA_FLAG_COMPRESS_WHATIF) without a GPU.  The model compressor's frames (kta_lz4_model_host)
against an independent restatement (tests/lz4_model_py.py), byte for byte, on every length and law of
tests/compress_whatif_inputs.py and on its crafted blocks; the frames inflate to their input with the analyzer's own LZ4
decoder and with liblz4 (pyarrow, when present); the host rule (kta_compress_whatif_host) on batches of every codec; the
identities, each broken by one word; the merge; the rendered section against a golden text; the exports; the CLI's refusals
that need no device; the torch twin of the exchange over gloo; the model's own source (csrc/kta_lz4_model.h) run natively
under AddressSanitizer + UBSan (tests/native/lz4_model_check.cpp, a program of its own).

THE FLOOR.  The section's note says that liblz4 does better than the model.  Measured here, blocks against liblz4 1.9.3
(LZ4_compress_default through pyarrow's lz4_raw), the model's bytes over liblz4's:
    the generator's text law (words, numbers, punctuation), 6000 records: 1.008 (8 records a batch, 2 KiB), 1.017 (60, 16 KiB),
        1.023 (240, 63 KiB)
    the generator's patterned law (the bench's 24-byte period with keys and varints between): 1.131, 1.129, 1.125
    zeros: equal.  Random bytes: both store (the model's stored block is the smaller by liblz4's own overhead).
The tests assert the 16 KiB figures + 0.05, room for other seeds: 1.067 and 1.179."""
import ctypes as C
import os
import re
import socket
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
from kafka_topic_analyzer_amd import distributed
import compress_whatif_inputs as I
import lz4_model_py as M
import payload_blobs as B
import record_batches_blobs as RB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
CSRC = os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "compress_whatif_section.txt")
NEW_EXPORTS = ("kta_get_compress_whatif", "kta_exchange_compress_whatif", "kta_compress_whatif_result_vector", "kta_compress_whatif_vector",
               "kta_merge_compress_whatif", "kta_compress_whatif_identities", "kta_render_compress_whatif")
P = 4
CODECS = [c for c in B.CODECS if c != "zstd" or RB.have_zstd()]
TEXT_BOUND, PATTERNED_BOUND = 1.017 + 0.05, 1.129 + 0.05


def _holds(v, P_=P):
    bad = [n for n, ok in M.identities(v, P_) if not ok]
    assert not bad, bad
    assert kta.compress_whatif_identities(v, P_)


def _inflate(frame, n):
    out = C.create_string_buffer(n + 1)
    got = N.load().kta_lz4_inflate_host(frame, len(frame), out, n)
    return got, out.raw[:max(got, 0)]


def _frame_checks(data):
    want, (blocks, stored, _, _) = M.frame(data)
    got = kta.lz4_model(data)
    assert got == want, (len(data), len(got), len(want))
    assert kta.lz4_model_size(data) == len(got)                                    # dst == NULL
    assert got[:7] == b"\x04\x22\x4d\x18\x60\x40" + bytes([(M.xxh32(b"\x60\x40") >> 8) & 0xFF]) and got[-4:] == bytes(4)
    assert blocks == (len(data) + 65535) // 65536 and len(got) <= len(data) + 11 + 4 * blocks
    n, back = _inflate(got, len(data))
    assert n == len(data) and back == data
    return got


# ------------------------------------------------------------------------------------------ 1. frames
@pytest.mark.parametrize("name", I.LAWS)
def test_frames_equal_the_twins_and_inflate_to_their_input(name):
    for n in I.LENGTHS:
        _frame_checks(I.law(name, n, n))


def test_frames_of_the_crafted_blocks():
    for name, (block, check) in I.crafted().items():
        assert check(M.sequences(block)), name
        _frame_checks(block)


def test_the_empty_section_a_short_destination_and_a_null_source():
    assert kta.lz4_model(b"") == b"\x04\x22\x4d\x18\x60\x40\x82" + bytes(4) and M.frame(b"")[0] == kta.lz4_model(b"")
    data = I.text(3000, 1)
    whole = kta.lz4_model(data)
    small = (C.c_uint8 * 100)()
    assert N.load().kta_lz4_model_host(data, len(data), small, 100) == len(whole) and bytes(small) == whole[:100]
    assert N.load().kta_lz4_model_host(None, 5, None, 0) == -1


def test_liblz4_reads_the_frames():
    pa = pytest.importorskip("pyarrow")
    codec = pa.Codec("lz4")
    for name in I.LAWS:
        for n in I.LENGTHS:
            data = I.law(name, n, n)
            assert codec.decompress(kta.lz4_model(data), decompressed_size=len(data), asbytes=True) == data, (name, n)
    for block, _ in I.crafted().values():
        assert codec.decompress(kta.lz4_model(block), decompressed_size=len(block), asbytes=True) == block


def test_the_stride_looks_the_table_up_as_it_stood_before_the_stride():
    """period 3 from position 0: every position of the first stride finds the empty table — candidate 0, a hit only where the
    phase is 0 —, so the first match begins at position 3 with offset 3 and runs to n - 5"""
    data = I.law("period3", 300)
    seqs = M.sequences(data)
    assert seqs[0] == (0, 3, 3, 300 - 5 - 3) and len(seqs) == 2
    assert len(kta.lz4_model(data)) == 11 + 4 + M.block_cost(seqs)


# ------------------------------------------------------------------------------------------ 2. the rule on batches
def _batches(compression, seed=0, n=6):
    out, off = [], 0
    for b in range(n):
        recs = [B.record(i, I.text(40 + 30 * ((b + i) % 5), seed + 10 * b + i), key=b"k%d" % i) for i in range(8 + b)]
        out.append(B.batch(off, recs, compression=compression[b % len(compression)] if isinstance(compression, (list, tuple)) else compression))
        off += len(recs)
    return out


def test_host_rule_equals_the_restatement_and_the_codec_on_disk_changes_only_now_bytes():
    vecs = {}
    for comp in CODECS:
        bs = _batches(comp)
        blob, _ = B.join(bs)
        v = kta.compress_whatif_host(blob, 2, P)
        assert np.array_equal(v, M.restate([(2, comp, len(b), raw) for b, raw in bs], P)), comp
        _holds(v)
        vecs[comp] = kta.split_compress_whatif(v, P)
        s = vecs[comp]
        assert s["codecs"][M.CODEC_OF[comp], 0] == 6 == s["partitions"][2, M.BATCHES] and s["codecs"].sum() == s["codecs"][M.CODEC_OF[comp]].sum()
    plain = vecs[None]["partitions"][2]
    assert plain[M.NOW] == plain[M.RAW] and plain[M.MODEL] < plain[M.RAW] and plain[M.SEQUENCES] > 0
    for comp in CODECS[1:]:
        w = vecs[comp]["partitions"][2]
        same = [k for k in range(M.PW) if k != M.NOW]
        assert np.array_equal(w[same], plain[same]) and w[M.NOW] < plain[M.NOW], comp            # the same records: the same model


def test_mixed_codecs_other_partitions_and_batches_that_do_not_inflate():
    bs = _batches(CODECS, seed=5, n=10)
    blob, _ = B.join(bs)
    v = kta.compress_whatif_host(blob, 1, P)
    assert np.array_equal(v, M.restate([(1, CODECS[i % len(CODECS)], len(b), raw) for i, (b, raw) in enumerate(bs)], P))
    _holds(v)
    assert not kta.compress_whatif_host(blob, P, P).any() and not kta.compress_whatif_host(blob, -1, P).any()
    acc = kta.compress_whatif_host(blob, 0, P, v.copy())                                       # adds to a vector
    assert np.array_equal(acc[:M.PW], v[M.PW:2 * M.PW]) and np.array_equal(acc[M.PW * P:], 2 * v[M.PW * P:])
    good = _batches(None, n=2)
    broken = [(RB.corrupt_stream(b, c), raw) for c in CODECS[1:] for b, raw in _batches(c, n=1)]
    blob, _ = B.join(good[:1] + broken + good[1:])
    assert np.array_equal(kta.compress_whatif_host(blob, 0, P), M.restate([(0, None, len(b), raw) for b, raw in good], P))


def test_identities_each_broken_by_one_word():
    blob, _ = B.join(_batches(CODECS, seed=9, n=10))
    v = kta.compress_whatif_host(blob, 2, P)
    _holds(v)
    at, codec0 = 2 * M.PW, M.PW * P
    for word, by in ((at + M.STORED, int(v[at + M.BLOCKS]) + 1), (at + M.MATCH_BYTES, int(v[at + M.RAW])), (at + M.SEQUENCES, int(v[at + M.MATCH_BYTES])),
                     (at + M.BATCHES, 1), (at + M.RAW, 1), (at + M.NOW, 1), (codec0 + 3, 1), (codec0 + M.CW * 4, 1)):
        w = v.copy()
        w[word] += np.uint64(by)
        assert not kta.compress_whatif_identities(w, P) and not all(ok for _, ok in M.identities(w, P)), word
    w = v.copy()
    w[at + M.MODEL] += np.uint64(int(v[at + M.RAW]) + 11 * int(v[at + M.BATCHES]) + 4 * int(v[at + M.BLOCKS]))
    w[codec0 + 3] += w[at + M.MODEL] - v[at + M.MODEL]
    assert not kta.compress_whatif_identities(w, P) and not all(ok for _, ok in M.identities(w, P))   # larger than every block stored
    with pytest.raises(ValueError):
        kta.compress_whatif_identities(v[:-1], P)


def test_merge_adds_every_word():
    a = kta.compress_whatif_host(B.join(_batches(None, seed=1))[0], 0, P)
    b = kta.compress_whatif_host(B.join(_batches("snappy", seed=2))[0], 1, P)
    acc = a.copy()
    assert kta.merge_compress_whatif(acc, b, P) is acc and np.array_equal(acc, a + b)
    _holds(acc)
    with pytest.raises(ValueError):
        kta.merge_compress_whatif(acc, b[:-1], P)


# ------------------------------------------------------------------------------------------ 3. the rendered section
def _golden():
    v = np.zeros(M.words(P), np.uint64)
    for p, comp in ((0, None), (1, "snappy"), (3, "lz4")):
        kta.compress_whatif_host(B.join(_batches(comp, seed=p, n=4 + p))[0], p, P, v)
    kta.compress_whatif_host(B.join([I.batch(70000, "random", 3), I.batch(300, "zeros")])[0], 3, P, v)
    return v


def test_rendered_section_matches_the_golden_text():
    v = _golden()
    _holds(v)
    text = kta.render_compress_whatif(v, P)
    assert text == open(GOLDEN).read()
    lines = text.splitlines()
    assert "kta.compress_whatif=lz4; not part of the reference report" in lines[0] and text.endswith("=" * 120 + "\n")
    assert "64 positions at a time" in lines[-5] and "floor" in lines[-4] and "liblz4" in lines[-4] and "61 header bytes" in lines[-3] and "batching" in lines[-2]
    rows = [re.split(r"\s*\|\s*", l)[1:-1] for l in lines if l.startswith("| ")]
    assert rows[0][:3] == ["P", "Batches", "Record bytes/batch"] and [r[0] for r in rows[1:6]] == ["0", "1", "2", "3", "Topic"]
    assert [r[0] for r in rows[6:]] == ["Codec", "none", "gzip", "snappy", "lz4", "zstd"]
    assert rows[3][1] == "0" and rows[3].count("n/a") == 6                            # the partition without batches
    s = kta.split_compress_whatif(v, P)
    topic = rows[5]
    assert [int(topic[k]) for k in (1, 3, 4, 6)] == [int(s["topic"][k]) for k in (M.BATCHES, M.RAW, M.NOW, M.MODEL)]
    assert topic[7] == "%.2f" % (int(s["topic"][M.RAW]) / int(s["topic"][M.MODEL]))


# ------------------------------------------------------------------------------------------ 4. exports, CLI
def test_new_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "kta_hip.h")).read()
    m = re.search(r"#define KTA_FLAG_COMPRESS_WHATIF (\w+?)[uU]\s", header)
    assert m and int(m.group(1), 0) == 0x2000 == N.KTA_FLAG_COMPRESS_WHATIF
    others = [int(v, 0) for v in re.findall(r"#define KTA_FLAG_(?!COMPRESS_WHATIF)\w+ +\(?(\w+?)[uU]\b", header)]
    assert 0x2000 not in others and all(f & 0x2000 == 0 for f in others)            # bit 13 was free
    assert re.search(r"#define KTA_ABI_VERSION 7\b", header) and N.load().kta_abi_version() == 7
    assert (N.KTA_COMPRESS_WHATIF_PARTITION_WORDS, N.KTA_COMPRESS_WHATIF_CODECS, N.KTA_COMPRESS_WHATIF_CODEC_WORDS) == (M.PW, M.CODECS, M.CW)
    assert re.search(r"#define KTA_COMPRESS_WHATIF_WORDS\(P\) \(8u \* \(size_t\)\(P\) \+ 20u\)", header)
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    kafka_text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kta_kafka.h")).read(), flags=re.S)
    lib = N.load()
    for name in NEW_EXPORTS:
        assert re.search(r"^int\s+%s\s*\(" % name, text, flags=re.M), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    for name, ret in (("kta_compress_whatif_info", "int"), ("kta_compress_whatif_host", "int"), ("kta_lz4_model_host", "int64_t")):
        assert re.search(r"^%s\s+%s\s*\(" % (ret, name), kafka_text, flags=re.M) and hasattr(lib, name) and name in N.SIGNATURES, name
    for name in ("split_compress_whatif", "merge_compress_whatif", "compress_whatif_identities", "compress_whatif_host", "render_compress_whatif",
                 "lz4_model", "lz4_model_size"):
        assert name in kta.__all__ and callable(getattr(kta, name))
    for name in ("compress_whatif", "exchange_compress_whatif", "compress_whatif_result_vector", "compress_whatif_vector", "compress_whatif_info"):
        assert callable(getattr(kta.HipMetricHandler, name))
    assert callable(distributed.allreduce_compress_whatif_vector)
    assert kta.COMPRESS_WHATIF_CODECS == tuple("none" if c is None else c for c in B.CODECS)


def _cli(*knobs, src="synthetic://c2?records=100", flags=()):
    return subprocess.run([CLI, "-t", "x", "-b", src, *flags, "--librdkafka", ",".join(knobs)], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value", ["1", "0", "", "zstd", "LZ4"])
def test_cli_refuses_a_value_other_than_lz4(value):
    r = _cli("kta.compress_whatif=" + value)
    assert r.returncode == 2 and "kta.compress_whatif=%s: expected lz4" % value in r.stderr and r.stdout == "", (r.returncode, r.stderr)
    assert len(r.stderr.strip().splitlines()) == 1


@pytest.mark.parametrize("src,knobs", [("synthetic://c2?records=100", ()), ("dump:///nonexistent.dump", ()), ("localhost:1", ()),
                                       ("segment:///nonexistent.log", ("kta.per_message=1",)), ("synthetic://c2?records=100", ("kta.gpus=2",))])
def test_cli_refuses_sources_that_do_not_hold_the_log_bytes(src, knobs):
    """one line that says why, before a broker, a file or a device is asked for anything"""
    r = _cli("kta.compress_whatif=lz4", *knobs, src=src)
    assert r.returncode == 2 and r.stdout == "", (r.returncode, r.stdout, r.stderr)
    lines = r.stderr.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("kta.compress_whatif=lz4: needs a segment:// source") and "not the bytes of the log" in lines[0]


def test_cli_help_is_unchanged_by_the_knob():
    plain = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    knob = subprocess.run([CLI, "--librdkafka", "kta.compress_whatif=lz4", "--help"], capture_output=True, text=True, timeout=60)
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
        sets = [(p, c, len(b), raw) for p in range(5) for c in (None, "snappy") for b, raw in _batches(c, seed=p, n=2)]
        vecs = [M.restate([s for s in sets if s[0] % world == r], 5) for r in range(world)]
        t = torch.from_numpy(vecs[rank].view(np.int64).copy())
        from kafka_topic_analyzer_amd import distributed as D
        D.allreduce_compress_whatif_vector(t, 5)
        whole = M.restate(sets, 5)
        q.put((rank, bool(np.array_equal(t.numpy().view(np.uint64), whole) and vecs[rank].any() and not np.array_equal(vecs[rank], whole))))
    finally:
        dist.destroy_process_group()


def test_allreduce_compress_whatif_vector_over_gloo_equals_the_unsharded_vector():
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
        distributed.allreduce_compress_whatif_vector(torch.zeros(8 * 4 + 19, dtype=torch.int64), 4)


# ------------------------------------------------------------------------------------------ 6. the model's own source
def test_native_check_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/lz4_model_check.cpp: a program of its own that calls kta_lz4_model.h, built with the sanitizers and run directly."""
    exe = str(tmp_path / "lz4_model_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "native", "lz4_model_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.returncode, r.stdout[-500:], r.stderr[-2000:])


# ------------------------------------------------------------------------------------------ 7. the floor, measured
def _generator_sections(flag, records=3000, per_batch=60):
    """the records sections of the synthetic encoder's batches (bench.py's source): flag 0 its patterned values, 0x200 its text"""
    lib = N.load()
    spec, _ = kta.synth_preset("c4")
    ln = C.c_uint64()
    lib.kta_kafka_encode_synth_host_ex(C.byref(spec), 0, records, per_batch, 0x100 | flag, None, 0, C.byref(ln))
    buf = np.zeros(ln.value + 128, np.uint8)
    assert lib.kta_kafka_encode_synth_host_ex(C.byref(spec), 0, records, per_batch, 0x100 | flag, buf.ctypes.data, ln.value, C.byref(ln)) == N.KTA_OK
    plain, out, pos = buf[:ln.value].tobytes(), [], 0
    while pos + 61 <= len(plain):
        total = 12 + int.from_bytes(plain[pos + 8:pos + 12], "big")
        out.append(plain[pos + 61:pos + total])
        pos += total
    return out


def _blocks_over_liblz4(sections, codec):
    model = lib = 0
    for s in sections:
        for pos in range(0, len(s), 65536):
            block = s[pos:pos + 65536]
            model += kta.lz4_model_size(block) - 15                                 # the frame of one block without its 15 bytes of framing
            lib += len(codec.compress(block, asbytes=True))
    return model, lib


@pytest.mark.parametrize("flag,bound", [(0x200, TEXT_BOUND), (0, PATTERNED_BOUND)], ids=["text", "patterned"])
def test_the_model_is_a_floor_liblz4_is_within_the_measured_ratio(flag, bound):
    pa = pytest.importorskip("pyarrow")
    sections = _generator_sections(flag)
    assert len(sections) == 50 and 12000 < len(sections[0]) < 20000
    model, lib = _blocks_over_liblz4(sections, pa.Codec("lz4_raw"))
    print("model %d bytes, liblz4 %d bytes, ratio %.4f (bound %.3f)" % (model, lib, model / lib, bound))
    assert lib <= model <= bound * lib                                              # a floor: liblz4 does no worse, and not by more than measured


def test_on_zeros_the_model_equals_liblz4():
    pa = pytest.importorskip("pyarrow")
    for n in (200, 4096, 65536):
        model, lib = _blocks_over_liblz4([bytes(n)], pa.Codec("lz4_raw"))
        assert model == lib, n

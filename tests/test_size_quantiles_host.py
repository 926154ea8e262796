"""CPU tests of the size percentiles (KTA_FLAG_SIZE_QUANTILES; no reference counterpart): the host-only entry points
(kta_size_bin, kta_size_bin_bounds, kta_size_quantile, kta_merge_size_quantiles, kta_render_size_percentiles) against the
restatement in tests/size_quantiles_py.py, the header's definition and the unchanged ABI number, the CLI's refusals that need
no device, and the rule's own source (csrc/kta_size_bins.h) run natively under AddressSanitizer + UBSan
(tests/native/size_bins_check.cpp, a program of its own)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
from kafka_topic_analyzer_amd import distributed
import size_quantiles_py as SQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
CSRC = os.path.join(ROOT, "kafka_topic_analyzer_amd", "csrc")
NEW_EXPORTS = ("kta_get_size_quantiles", "kta_exchange_size_quantiles", "kta_size_quantiles_result_vector", "kta_merge_size_quantiles",
               "kta_size_quantiles_max_partitions", "kta_size_quantiles_info", "kta_set_size_quantiles_slice", "kta_size_bin",
               "kta_size_bin_bounds", "kta_size_quantile", "kta_render_size_percentiles")


def _cols(seed, n, P):
    """sizes from the boundary list, -1 and small ones; partitions -1 and P among them"""
    rng = np.random.default_rng(seed)
    pool = np.array([-1, 0, 1, 7, 200, 5000, 31, 32, 63, 64, 65534, 65535, 65536, 2**31 - 1], np.int64)
    return {"partition": rng.integers(-1, P + 1, size=n).astype(np.int32), "key_len": rng.choice(pool, size=n).astype(np.int32),
            "val_len": rng.choice(pool, size=n).astype(np.int32), "ts_ms": np.full(n, 1_600_000_000_000, np.int64)}


# ------------------------------------------------------------------------------------------ 1. the rule
def test_size_bin_on_every_bound_and_both_sides_of_every_change():
    sizes = [SQ.lo(b) for b in range(SQ.BINS)] + [SQ.hi(b) for b in range(SQ.BINS)] + list(SQ.BOUNDARY_SIZES) + [0, 1, 33, 2**32 - 2]
    for v in sizes:
        assert kta.size_bin(v) == SQ.bin_of(v), v
    assert [kta.size_bin(v) for v in (31, 32, 63, 64, 2**32 - 1)] == [31, 32, 47, 48, 463]
    assert np.array_equal(SQ.bins_of(sizes), [SQ.bin_of(v) for v in sizes])          # the restatement's two forms agree


def test_bin_bounds_tile_the_sizes_and_are_a_sixteenth_wide():
    for b in range(SQ.BINS):
        lo, hi = kta.size_bin_bounds(b)
        assert (lo, hi) == (SQ.lo(b), SQ.hi(b))
        assert hi + 1 == SQ.lo(b + 1)
        if b + 1 < SQ.BINS:
            assert hi + 1 == kta.size_bin_bounds(b + 1)[0]
        if b >= 32:
            assert hi * 16 <= lo * 17                                                 # hi / lo <= 17 / 16
        else:
            assert lo == hi == b
    assert kta.size_bin_bounds(0)[0] == 0 and kta.size_bin_bounds(463)[1] == 2**32 - 1
    with pytest.raises(kta.KtaError):
        kta.size_bin_bounds(SQ.BINS)


# ------------------------------------------------------------------------------------------ 2. the read-off
@pytest.mark.parametrize("n", [1, 2, 1000, 1001])
def test_size_quantile_is_the_nearest_rank_of_the_sorted_sizes(n):
    rng = np.random.default_rng(n)
    sizes = (rng.integers(0, 2**32, size=n, dtype=np.uint64) >> rng.integers(0, 32, size=n).astype(np.uint64)).astype(np.uint64)
    hist = np.bincount(SQ.bins_of(sizes), minlength=SQ.BINS).astype(np.uint64)
    for num, den in SQ.PERCENTILES + ((0, 100), (100, 100)):
        got = kta.size_quantile(hist, num, den)
        assert got == SQ.quantile(hist, num, den)
        want = SQ.sorted_nearest_rank(sizes, num, den)
        assert got[0] <= want <= got[1]
        assert got[1] == want if want < 32 else got[1] * 16 <= want * 17              # the printed value: exact, or at most 6.25 % high


def test_size_quantile_of_the_empty_histogram_and_of_bad_arguments():
    empty = np.zeros(SQ.BINS, np.uint64)
    assert kta.size_quantile(empty, 50, 100) is None and SQ.quantile(empty, 50, 100) is None
    one = empty.copy()
    one[40] = 1
    assert kta.size_quantile(one, 999, 1000) == (SQ.lo(40), SQ.hi(40))
    with pytest.raises(kta.KtaError):
        kta.size_quantile(one, 1, 0)
    with pytest.raises(kta.KtaError):
        kta.size_quantile(one, 101, 100)
    big = empty.copy()
    big[3], big[400] = 2**63, 2**63 - 1                                              # the product takes 128 bits
    assert kta.size_quantile(big, 50, 100) == (3, 3) and kta.size_quantile(big, 999, 1000) == (SQ.lo(400), SQ.hi(400))


# ------------------------------------------------------------------------------------------ 3. vector, merge, render
def test_restated_vector_holds_the_identities_and_merge_is_the_sum():
    P = 5
    a, b = _cols(1, 4000, P), _cols(2, 3000, P)
    va, vb = SQ.vector(a, P), SQ.vector(b, P)
    assert SQ.identities_hold(va, SQ.counters(a, P), P) and not SQ.identities_hold(va, SQ.counters(b, P), P)
    both = {k: np.concatenate([a[k], b[k]]) for k in a}
    acc = va.copy()
    assert kta.merge_size_quantiles(acc, vb, P) is acc
    assert np.array_equal(acc, SQ.merge(va, vb)) and np.array_equal(acc, SQ.vector(both, P))
    d = kta.split_size_quantiles(acc, P)
    assert d["records"] + d["bad_partition"] == 7000 and d["bad_partition"] > 0
    assert int(d["key"].sum()) == d["keyed"] and int(d["value"].sum()) == int(d["message"].sum()) == d["alive"]
    assert d["key"].shape == d["value"].shape == d["message"].shape == (P, SQ.BINS)
    with pytest.raises(ValueError):
        kta.split_size_quantiles(acc[:-1], P)
    assert N.load().kta_merge_size_quantiles(acc.ctypes.data, vb.ctypes.data, 0) == N.KTA_ERR_INVALID
    assert N.load().kta_merge_size_quantiles(acc.ctypes.data, vb.ctypes.data, kta.size_quantiles_max_partitions() + 1) == N.KTA_ERR_INVALID


def test_render_equals_the_restated_section():
    P = 4
    cols = _cols(3, 6000, P)
    cols["partition"][cols["partition"] == 2] = 1                                    # partition 2 is empty: a row of dashes
    v, c = SQ.vector(cols, P), SQ.counters(cols, P)
    text = kta.render_size_percentiles(v, c, P)
    assert text == SQ.section(v, P)
    lines = text.splitlines()
    assert lines[0] == SQ.TITLE.rstrip("\n") and "not part of the reference report" in lines[0]
    assert lines[-1] == "=" * 120 and lines[-2] == SQ.BOUND.rstrip("\n") and "6.25 %" in lines[-2]
    empty_rows = [ln for ln in lines if re.match(r"^\| 2 +\| 0 +\| - +\| - +\| - +\| - +\| - +\|$", ln)]
    assert len(empty_rows) == 3
    assert sum(1 for ln in lines if ln.startswith("| All ")) == 3 and sum(1 for ln in lines if ln.startswith("| P ")) == 3


def test_render_of_exact_small_sizes_prints_them():
    P = 1
    cols = {"partition": np.zeros(100, np.int32), "key_len": np.arange(100, dtype=np.int32) % 20, "val_len": np.full(100, 31, np.int32)}
    v = SQ.vector(cols, P)
    text = kta.render_size_percentiles(v, SQ.counters(cols, P), P)
    assert re.search(r"^\| 0 +\| 100 +\| 9 +\| 17 +\| 19 +\| 19 +\| 19 +\|$", text, flags=re.M)          # keys 0 .. 19, five of each
    assert re.search(r"^\| All +\| 100 +\| 31 +\| 31 +\| 31 +\| 31 +\| 31 +\|$", text, flags=re.M)      # values of 31 B


def test_render_refuses_a_vector_that_breaks_an_identity():
    P = 3
    cols = _cols(4, 2000, P)
    v, c = SQ.vector(cols, P), SQ.counters(cols, P)
    kta.render_size_percentiles(v, c, P)
    for word in (0 * 3 * SQ.BINS + 5, (1 * 3 + 1) * SQ.BINS + 40, (2 * 3 + 2) * SQ.BINS + 463, P * 3 * SQ.BINS + 0, P * 3 * SQ.BINS + 1):
        bad = v.copy()
        bad[word] += np.uint64(1)
        with pytest.raises(kta.KtaError) as e:
            kta.render_size_percentiles(bad, c, P)
        assert e.value.code == N.KTA_ERR_INVALID
    with pytest.raises(ValueError):
        kta.render_size_percentiles(v, c[:-1], P)


def test_allreduce_helper_checks_the_length():
    torch = pytest.importorskip("torch")
    with pytest.raises(AssertionError):
        distributed.allreduce_size_quantiles_vector(torch.zeros(5, dtype=torch.int64), 2)


# ------------------------------------------------------------------------------------------ 4. ABI, limit, CLI
def test_new_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "kta_hip.h")).read()
    m = re.search(r"#define KTA_FLAG_SIZE_QUANTILES (\w+?)[uU]\s", header)
    assert m and int(m.group(1), 0) == 0x100 == N.KTA_FLAG_SIZE_QUANTILES
    others = [int(v, 0) for v in re.findall(r"#define KTA_FLAG_(?!SIZE_QUANTILES)\w+ +\(?(\w+?)[uU]\b", header)]
    assert 0x100 not in others and all(f & 0x100 == 0 for f in others)               # bit 8 was free
    assert re.search(r"#define KTA_ABI_VERSION 7\b", header)
    assert re.search(r"#define KTA_SIZE_BINS 464\b", header) and N.KTA_SIZE_BINS == SQ.BINS == 464
    assert (N.KTA_SIZE_QUANTITIES, N.KTA_SIZE_GLOBALS) == (SQ.QUANTITIES, SQ.GLOBALS) == (3, 8)
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = N.load()
    for name in NEW_EXPORTS:
        assert re.search(r"^(?:int|uint32_t)\s+%s\s*\(" % name, text, flags=re.M), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    assert lib.kta_abi_version() == 7
    for name in ("split_size_quantiles", "merge_size_quantiles", "render_size_percentiles", "size_bin", "size_bin_bounds", "size_quantile",
                 "size_quantiles_max_partitions"):
        assert name in kta.__all__ and callable(getattr(kta, name))
    for name in ("size_quantiles", "exchange_size_quantiles", "size_quantiles_info", "size_quantiles_result_vector", "set_size_quantiles_slice"):
        assert callable(getattr(kta.HipMetricHandler, name))
    assert callable(distributed.allreduce_size_quantiles_vector)


def test_the_limit_admits_the_flagship_topic_and_a_dozen_partitions():
    assert 256 <= kta.size_quantiles_max_partitions() <= 4096


def _cli(*knobs, src="synthetic://c2?records=100", flags=()):
    return subprocess.run([CLI, "-t", "x", "-b", src, *flags, "--librdkafka", ",".join(knobs)], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value", ["2", "", "yes", "01"])
def test_cli_refuses_a_value_other_than_0_or_1(value):
    """a usage error in the style of the other kta.* keys: a line on stderr, exit status 2, nothing on stdout"""
    r = _cli("kta.percentiles=" + value)
    assert r.returncode == 2 and "kta.percentiles=%s: expected 0 or 1" % value in r.stderr and r.stdout == "", (r.returncode, r.stderr)
    assert len(r.stderr.strip().splitlines()) == 1


def test_cli_refuses_more_partitions_than_the_pass_admits(tmp_path):
    """a topic dump of limit + 1 partitions: refused after its header was read, before any context is created"""
    P = kta.size_quantiles_max_partitions() + 1
    path = tmp_path / "wide.dump"
    with open(path, "wb") as f:
        f.write(b"KTADUMP1" + struct.pack("<IIQQ", 1, P, 0, 0) + struct.pack("<%dq" % P, *([0] * P)) + struct.pack("<%dq" % P, *([1] * P)))
    r = _cli("kta.percentiles=1", src="dump://" + str(path))
    assert r.returncode == 2 and r.stdout == "", (r.returncode, r.stderr)
    assert "kta.percentiles=1: the topic has %d partitions, the size-percentile pass admits at most %d" % (P, P - 1) in r.stderr


def test_cli_help_is_unchanged_by_the_knob():
    plain = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    knob = subprocess.run([CLI, "--librdkafka", "kta.percentiles=1", "--help"], capture_output=True, text=True, timeout=60)
    assert plain.returncode == knob.returncode == 0 and knob.stdout == plain.stdout


# ------------------------------------------------------------------------------------------ 5. the rule's own source
def test_native_check_under_address_and_undefined_sanitizers(tmp_path):
    """tests/native/size_bins_check.cpp: a program of its own that calls kta_size_bins.h, built with the sanitizers and run directly."""
    exe = str(tmp_path / "size_bins_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "native", "size_bins_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK "), (r.stdout[-500:], r.stderr[-3000:])

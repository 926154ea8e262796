"""bench.py's options: a plain run leaves the sub-benchmarks to --full, and --dump-outputs writes the
result a caller of the timed path receives, field for field, as float64."""
import importlib.util
import os

import numpy as np
import pytest

from kafka_topic_analyzer_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_cli_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_plain_run_times_the_headline_only():
    b = _bench()
    args = b.build_parser().parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (7, 2, False, None)
    assert not b.runs_full(args, 1)


def test_full_runs_the_sub_benchmarks_of_a_single_gpu_c4_run():
    b = _bench()
    p = b.build_parser()
    assert b.runs_full(p.parse_args(["--full"]), 1)
    assert b.runs_full(p.parse_args(["--full", "--no-alive", "--no-decode"]), 1)   # the --no-* options act inside it
    assert not b.runs_full(p.parse_args(["--full"]), 2)                             # N > 1: headline line only
    assert not b.runs_full(p.parse_args(["--full", "--config", "c5"]), 1)


def test_dump_outputs_writes_the_result_and_counters_as_float64(tmp_path):
    b = _bench()
    res = N.KtaResult(n_partitions=3, any_records=1, any_live=1, count_alive_keys=1, min_ts_sec=-62135596800,
                      max_ts_sec=1600014336, smallest_message=7, largest_message=3998, overall_count=1 << 30,
                      overall_size=274998334871, alive_keys=123456, bad_partition_records=0)
    counters = np.arange(3 * N.KTA_NCOUNTERS, dtype=np.uint64).reshape(3, N.KTA_NCOUNTERS) * np.uint64(1 << 33)
    out = tmp_path / "dump"
    b.dump_outputs(str(out), res, counters)
    assert sorted(os.listdir(out)) == ["counters.npy", "result.npy"]
    c = np.load(out / "counters.npy")
    r = np.load(out / "result.npy")
    assert c.dtype == np.float64 and c.shape == (3, N.KTA_NCOUNTERS)
    assert np.array_equal(c.astype(np.uint64), counters)
    assert r.dtype == np.float64 and r.shape == (len(N.KtaResult._fields_),)
    assert [int(x) for x in r] == [int(getattr(res, f)) for f, _ in N.KtaResult._fields_]


@pytest.mark.gpu
def test_plain_run_dumps_what_the_oracle_computes(tmp_path):
    """A plain bench.py run on a small c4 shard: the line carries no sub-benchmark block, and the dumped result of the last
    timed step is the C oracle's for the same synthetic records."""
    import json
    import subprocess
    import sys
    import kafka_topic_analyzer_amd as kta
    from oracle_c import Oracle
    n = 1 << 22
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--preroll", "2", "--records-per-gpu", str(n), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["unit"] == "records/s"
    for block in ("cpu_baseline", "alive_pass", "kafka_decode", "host_fed", "raw_log_e2e", "boundary_per_message"):
        assert block not in line, block
    spec, _ = kta.synth_preset("c4")
    o = Oracle()
    o.run_soa(kta.synth_fill_host(spec, 0, n))
    counters = np.load(out / "counters.npy")
    assert np.array_equal(counters, o.counters(256).astype(np.float64))
    res = dict(zip([f for f, _ in N.KtaResult._fields_], np.load(out / "result.npy")))
    assert res["overall_count"] == n and res["overall_size"] == o.get("overall_size")
    assert res["largest_message"] == o.get("largest_message")
    o.close()

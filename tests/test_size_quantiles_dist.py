"""The size-percentile vector's exchange.  On the CPU (gloo): allreduce_size_quantiles_vector over the vectors of
partition-sharded ranks (p on rank p % N) — and of ranks that share records any other way — ends with the unsharded vector
on every rank, as kta_merge_size_quantiles states it on the host.  On the GPU (the RCCL test double, tests/mock_rccl.cpp):
kta_exchange on two and three ranks ends with the unsharded vector on every rank, and a second exchange after more batches
counts nothing twice."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import distributed as D
import size_quantiles_py as SQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, SEED, RECORDS = 7, 17, 20000


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _topic():
    rng = np.random.default_rng(SEED)
    pool = np.array([-1, 0, 1, 31, 32, 63, 64, 65534, 65535, 65536, 2**31 - 1], np.int64)
    return {"partition": rng.integers(-1, P + 1, size=RECORDS).astype(np.int32), "key_len": rng.choice(pool, size=RECORDS).astype(np.int32),
            "val_len": rng.choice(pool, size=RECORDS).astype(np.int32), "ts_ms": np.full(RECORDS, 1_600_000_000_000, np.int64)}


def _worker(rank, world, port, by_partition, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cols = _topic()
        n = len(cols["partition"])
        keep = cols["partition"] % world == rank if by_partition else np.arange(n) % world == rank
        vec = SQ.vector({k: v[keep] for k, v in cols.items()}, P)
        t = torch.from_numpy(vec.view(np.int64).copy())
        D.allreduce_size_quantiles_vector(t, P)
        q.put((rank, t.numpy().view(np.uint64).copy(), vec))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,by_partition", [(2, True), (3, False)])
def test_allreduce_size_quantiles_vector_equals_unsharded(world, by_partition):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, by_partition, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = sorted([q.get(timeout=120) for _ in procs], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    cols = _topic()
    whole = SQ.vector(cols, P)
    assert SQ.identities_hold(whole, SQ.counters(cols, P), P) and kta.split_size_quantiles(whole, P)["bad_partition"] > 0
    acc = np.zeros(SQ.words(P), np.uint64)
    for _, reduced, own in outs:
        assert np.array_equal(reduced, whole)
        kta.merge_size_quantiles(acc, own, P)
    assert np.array_equal(acc, whole)


# ------------------------------------------------------------------------------------------ kta_exchange, test double
@pytest.fixture(scope="module")
def mock_rccl(tmp_path_factory):
    lib = tmp_path_factory.mktemp("mock") / "libmock_rccl.so"
    r = subprocess.run(["timeout", "-k", "10", "600", "/opt/rocm/bin/hipcc", "-O1", "-shared", "-fPIC", "-std=c++17",
                        os.path.join(ROOT, "tests", "mock_rccl.cpp"), "-o", str(lib), "-lrt", "-lpthread"],
                       capture_output=True, text=True, timeout=660)
    assert r.returncode == 0, r.stderr[-2000:]
    return str(lib)


_EXCHANGE_WORKER = r'''
import os, sys, threading
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import kafka_topic_analyzer_amd as kta
import size_quantiles_py as SQ
from helpers import NOW

P = 7
rng = np.random.default_rng(31)
n = 40000
pool = np.array([-1, 0, 1, 31, 32, 63, 64, 65534, 65535, 65536, 2**31 - 1], np.int64)
cols = {"partition": rng.integers(-1, P + 1, size=n).astype(np.int32), "key_len": rng.choice(pool, size=n).astype(np.int32),
        "val_len": rng.choice(pool, size=n).astype(np.int32), "ts_ms": np.full(n, 1_600_000_000_000, np.int64)}
half = n // 2
vec = lambda idx: SQ.vector({k: v[idx] for k, v in cols.items()}, P)
want = {"first": vec(np.arange(half)), "all": vec(np.arange(n))}

for nranks in (2, 3):
    uid = kta.HipMetricHandler.comm_unique_id()
    errors = []
    def run(rank):
        try:
            h = kta.HipMetricHandler(P, now=NOW, size_quantiles=True)
            h.comm_create(nranks, rank, uid)
            mine = cols["partition"] % nranks == rank        # (-1 % nranks is nranks - 1: every record is on one rank)
            for stage, idx in (("first", np.arange(half)[mine[:half]]), ("all", np.arange(half, n)[mine[half:]])):
                b, nb = h.upload_batch({k: v[idx] for k, v in cols.items()})
                h.submit_device(b, nb, 0, which=1)
                h.exchange()
                assert np.array_equal(h.exchange_size_quantiles()["vector"], want[stage]), (nranks, rank, stage, "exchanged")
                own = np.nonzero(mine[:half if stage == "first" else n])[0]
                assert np.array_equal(h.size_quantiles()["vector"], vec(own)), (nranks, rank, stage, "own")
                h.exchange()
                assert np.array_equal(h.exchange_size_quantiles()["vector"], want[stage]), (nranks, rank, stage, "again")
                cv = h.result_vector_host()
                assert SQ.identities_hold(want[stage], cv, P), (nranks, rank, stage, "identities")
                h.sync()
                h.device_batch_free(b)
            h.comm_destroy(); h.close()
        except BaseException as e:
            errors.append((rank, repr(e)))
            print("rank %d: %r" % (rank, e), file=sys.stderr, flush=True)
            os._exit(2)        # the other ranks would wait in their collectives for ever
    ts = [threading.Thread(target=run, args=(r,)) for r in range(nranks)]
    [t.start() for t in ts]; [t.join() for t in ts]
    assert not errors, errors
    print("ranks", nranks, "OK", flush=True)
print("OK")
'''


@pytest.mark.gpu
def test_exchange_size_quantiles_on_two_and_three_ranks(tmp_path, mock_rccl):
    script = tmp_path / "exchange_worker.py"
    script.write_text(_EXCHANGE_WORKER)
    env = dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(script), ROOT], capture_output=True, text=True,
                       timeout=330, env=env)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count(" OK") == 2


@pytest.mark.gpu
def test_cli_sharded_run_prints_the_exchanged_snapshot_once(mock_rccl):
    src, records = "synthetic://c2?records=60000", 60000
    sp, _ = kta.synth_preset("c2")
    cols = kta.synth_fill_host(sp, 0, records)
    Pc = int(sp.n_partitions)
    want = SQ.section(SQ.vector(cols, Pc), Pc)
    cli = os.path.join(ROOT, "kafka_topic_analyzer_amd", "kta-analyzer")
    env = dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl)
    r = subprocess.run(["timeout", "-k", "10", "240", cli, "-t", "c2", "-b", src, "--librdkafka",
                        "kta.percentiles=1,kta.gpus=2,kta.batch=32768,kta.oversubscribe=1"], capture_output=True, text=True, timeout=270, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("Size percentiles per partition") == 1
    assert r.stdout[r.stdout.index("Size percentiles per partition"):] == want

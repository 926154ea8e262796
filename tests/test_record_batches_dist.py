"""The record-batch vector's exchange.  On the CPU (gloo): allreduce_record_batches_vector over the vectors of
partition-sharded ranks (p on rank p % N) ends with the unsharded vector on every rank — sums over the first 16 P + 500
words, maxima behind them —, as kta_merge_record_batches states it on the host.  On the GPU (the RCCL test double,
tests/mock_rccl.cpp): kta_exchange on two and three ranks ends with the unsharded vector on every rank, and a second
exchange after more blobs counts nothing twice."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import distributed as D
import record_batches_blobs as B
import record_batches_py as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sets():
    """a blob per partition, with the tests' own compressors only: every process builds the same bytes"""
    out = []
    for p in range(P):
        blob, raw = B.mixed(70 + p, 60 + 25 * p, codecs=[None, "snappy", "lz4"])
        out.append((blob, p, raw, set()))
    return out


def _worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        vec = R.restate([s for s in _sets() if s[1] % world == rank], P)
        t = torch.from_numpy(vec.view(np.int64).copy())
        D.allreduce_record_batches_vector(t, P)
        q.put((rank, t.numpy().view(np.uint64).copy(), vec))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_allreduce_record_batches_vector_equals_unsharded(world):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = sorted([q.get(timeout=120) for _ in procs], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    whole = R.restate(_sets(), P)
    assert all(ok for _, ok in R.identities(whole, P)) and whole[R.sketch_at(P):].any() and whole[R.max_at(P, 0):R.sketch_at(P)].all()
    acc = np.zeros(R.words(P), np.uint64)
    for _, reduced, own in outs:
        assert np.array_equal(reduced, whole)
        kta.merge_record_batches(acc, own, P)
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
import ctypes as C, os, sys, threading
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import kafka_topic_analyzer_amd as kta
from kafka_topic_analyzer_amd import _native as N
import record_batches_blobs as B
import record_batches_py as R
from helpers import NOW

P = 5
def sets(seed):
    out = []
    for p in range(P):
        blob, raw = B.mixed(seed + p, 60 + 25 * p, codecs=[None, "snappy", "lz4"])
        out.append((blob, p, raw, set()))
    return out
first, second = sets(80), sets(90)
want = {"first": R.restate(first, P), "all": R.restate(first + second, P)}

for nranks in (2, 3):
    uid = kta.HipMetricHandler.comm_unique_id()
    errors = []
    def run(rank):
        try:
            h = kta.HipMetricHandler(P, now=NOW, record_batches=True)
            h.comm_create(nranks, rank, uid)
            mine = []
            for stage, batch_sets in (("first", first), ("all", second)):
                for blob, p, raw, failed in batch_sets:
                    if p % nranks != rank:
                        continue
                    st = N.KtaKafkaIndexStats()
                    h._check(N.load().kta_kafka_consume(h._ctx, blob, len(blob), p, C.byref(st)))
                    mine.append((blob, p, raw, failed))
                h.exchange()
                assert np.array_equal(h.exchange_record_batches()["vector"], want[stage]), (nranks, rank, stage, "exchanged")
                assert np.array_equal(h.get_record_batches()["vector"], R.restate(mine, P)), (nranks, rank, stage, "own")
                h.exchange()
                assert np.array_equal(h.exchange_record_batches()["vector"], want[stage]), (nranks, rank, stage, "again")
                h.sync()
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
def test_exchange_record_batches_on_two_and_three_ranks(tmp_path, mock_rccl):
    script = tmp_path / "exchange_worker.py"
    script.write_text(_EXCHANGE_WORKER)
    env = dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(script), ROOT], capture_output=True, text=True,
                       timeout=330, env=env)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count(" OK") == 2

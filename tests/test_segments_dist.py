"""The exchange of the segment vector (kta_set_segments): on the CPU over gloo, two ranks that shard the topic by partition
reduce their restated vectors with the product's allreduce_segments_vector and end with the unsharded one (sharding by
record index is no valid case here: a partition's records must go through one rank in order, the timestamp-order pass's
precondition); on the GPU over the RCCL test double, kta_exchange on two and three ranks ends with the unsharded vector on
every rank, and a second exchange after more batches counts nothing twice."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import segments_py as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, M, S, OVERHEAD = 7, 40, 9000, 6


def _topic():
    rng = np.random.default_rng(77)
    n = 20000
    part = rng.integers(0, P, n).astype(np.int32)
    part[rng.random(n) < 0.02] = -1
    ts = 1_600_000_000_000 + np.arange(n, dtype=np.int64) * 7 + rng.integers(-4000, 4000, n)
    ts[rng.random(n) < 0.02] = -1
    return {"partition": part, "key_len": rng.integers(-1, 30, n).astype(np.int32), "val_len": rng.integers(-1, 400, n).astype(np.int32),
            "ts_ms": ts}


def _vec(cols):
    return SP.segments_vector(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"], P, S, M, OVERHEAD)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    from kafka_topic_analyzer_amd import distributed as D
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cols = _topic()
        mine = cols["partition"] % world == rank           # (-1 % world is world - 1: the records outside [0, P) have an owner too)
        t = torch.from_numpy(_vec({k: v[mine] for k, v in cols.items()}).view(np.int64).copy())
        D.allreduce_segments_vector(t, P, M)
        q.put((rank, t.numpy().view(np.uint64).copy()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_gloo_two_ranks_by_partition_end_with_the_unsharded_vector():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    whole = _vec(_topic())
    assert int(SP.split(whole, P, M)["globals"][2]) > 50
    for _, vec in outs:
        assert np.array_equal(vec, whole)


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
import test_segments_dist as TD
from helpers import NOW

P, M, CFG = TD.P, TD.M, (TD.S, TD.M, TD.OVERHEAD)
cols = TD._topic()
n = len(cols["partition"])
half = n // 2
cut = lambda idx: {k: v[idx] for k, v in cols.items()}
want = {"first": TD._vec(cut(np.arange(half))), "all": TD._vec(cols)}

for nranks in (2, 3):
    uid = kta.HipMetricHandler.comm_unique_id()
    errors = []
    def run(rank):
        try:
            h = kta.HipMetricHandler(P, now=NOW, segments=CFG)
            h.comm_create(nranks, rank, uid)
            mine = cols["partition"] % nranks == rank
            for stage, idx in (("first", np.arange(half)[mine[:half]]), ("all", np.arange(half, n)[mine[half:]])):
                b, nb = h.upload_batch(cut(idx))
                h.submit_device(b, nb, 0, which=1)
                for again in range(2):                     # a second exchange counts nothing twice
                    h.exchange()
                    assert np.array_equal(h.exchange_segments()["vector"], want[stage]), (nranks, rank, stage, again)
                upto = half if stage == "first" else n
                own = np.nonzero(mine[:upto])[0]
                assert np.array_equal(h.segments()["vector"], TD._vec(cut(own))), "own"
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
def test_exchange_on_two_and_three_ranks(tmp_path, mock_rccl):
    script = tmp_path / "exchange_worker.py"
    script.write_text(_EXCHANGE_WORKER)
    env = dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(script), ROOT], capture_output=True, text=True,
                       timeout=330, env=env)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count(" OK") == 2

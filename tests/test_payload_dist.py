"""The payload vector's exchange on the GPU (the RCCL test double, tests/mock_rccl.cpp): kta_exchange on two and three ranks
that shard the topic by partition (p on rank p % N) ends with the unsharded vector on every rank, and a second exchange after
more blobs counts nothing twice.  (The torch twin over gloo is in tests/test_payload_host.py.)"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
import payload_blobs as B
import payload_py as R
from helpers import NOW

P = 5
def sets(seed):
    out = []
    for p in range(P):
        blob, raw = B.mixed(20 + 7 * p, 6, seed=seed + p, compression=[None, "snappy", "lz4"])
        out.append((blob, p, raw, set()))
    return out
first, second = sets(80), sets(90)
want = {"first": R.restate(first, P), "all": R.restate(first + second, P)}
assert want["first"][:R.PW * P:R.PW].all() and all(ok for _, ok in R.identities(want["all"], P))

for nranks in (2, 3):
    uid = kta.HipMetricHandler.comm_unique_id()
    errors = []
    def run(rank):
        try:
            h = kta.HipMetricHandler(P, now=NOW, payload=True)
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
                assert np.array_equal(h.exchange_payload()["vector"], want[stage]), (nranks, rank, stage, "exchanged")
                assert np.array_equal(h.get_payload()["vector"], R.restate(mine, P)), (nranks, rank, stage, "own")
                h.exchange()
                assert np.array_equal(h.exchange_payload()["vector"], want[stage]), (nranks, rank, stage, "again")
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
def test_exchange_payload_on_two_and_three_ranks(tmp_path, mock_rccl):
    script = tmp_path / "exchange_worker.py"
    script.write_text(_EXCHANGE_WORKER)
    env = dict(os.environ, KTA_RCCL_LIBRARY=mock_rccl)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(script), ROOT], capture_output=True, text=True,
                       timeout=330, env=env)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count(" OK") == 2

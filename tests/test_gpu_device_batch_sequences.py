"""Random sequences of writers over one device batch, every reader after every writer against a plain model
(tests/device_batch_model.py): kta_batch_from_raw, kta_synth_fill_device, kta_kafka_decode_device and the widening of the
lengths for a key-reading pass, over whole tiles, cut tiles and the partial last tile; kta_batch_to_raw, the headers,
summaries, marks, scan planes and size words, the six scan variants over the allocation and over a view, the same scans
behind two record filters, and once per sequence the analytics, the timeline, the timestamp order, the size percentiles
and the segment pass.  Everything is integer and bit exact.  tests/test_device_batch_model.py asserts, without a GPU,
what the seeds reach: seeds 0..19 are the sequences they always were (plus the filters), seeds 20..31 aim at marked tiles.

A failure prints the seed, the ops up to the failing writer and the first differing field.  Paste the ops into a named
test of the file that owns the writer (test_gpu_tile_summary.py, test_tile_lens.py, test_tile_compact.py,
test_gpu_scan_plane.py):
    from device_batch_model import *
    with kta.HipMetricHandler(P, now=NOW) as h:
        replay(Device(h), ops)"""
import pytest

import kafka_topic_analyzer_amd as kta
import device_batch_model as M
from helpers import NOW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def devices():
    """The handlers, made when first asked for and kept for the module: ('plain' | 'keyed' | 'extra', P) -> Device.
    keyed: -c in the bit set state, for sequences with a Widen; extra: analytics, a timeline, the timestamp order, the size
    percentiles and the segment pass."""
    made = {}

    def get(kind, P):
        if (kind, P) not in made:
            kw = {"plain": {}, "keyed": {"count_alive_keys": True},
                  "extra": {"analytics": True, "timeline": M.TIMELINE, "ts_order": True, "size_quantiles": True,
                            "segments": M.SEGMENTS}}[kind]
            made[(kind, P)] = M.Device(kta.HipMetricHandler(P, now=NOW, **kw), keyed=(kind == "keyed"))
        return made[(kind, P)]
    yield get
    for d in made.values():
        d.free()
        d.h.close()


@pytest.mark.parametrize("seed", M.SEEDS)
def test_sequence(devices, seed):
    P = M.P_of(seed)
    ops = M.gen_sequence(seed, M.CAPACITY, P)
    assert len(ops) == M.N_OPS
    keyed = any(isinstance(op, M.Widen) for op in ops)
    M.replay(devices("keyed" if keyed else "plain", P), ops, seed=seed, extra_dev=devices("extra", P))

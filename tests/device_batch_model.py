"""A stateful model of one device batch (include/kta_hip.h, "Device batch layouts"; csrc/kta_tile.h): random sequences of
writers over ONE tile-compact allocation, a plain numpy model of what record i logically is, and after every writer every
reader against the model, bit for bit.

The model (Model) knows nothing of headers, compact forms or summaries.  What the device keeps beside the records — a
header per tile, a summary per tile — is checked for SOUNDNESS against the model (check_layout): a COMPACT header only
over content the compact form holds, u16 lengths only over lengths that fit, and a VALID summary beside a COMPACT header
equal to summary_definition() of the model's tile.  A zero summary is always acceptable.

Writers (ops): Upload (kta_batch_from_raw), SynthFill (kta_synth_fill_device), Decode (kta_kafka_decode_device of a small
record set, record_set()), Widen (a -c context reads a view with key columns of its own: the lengths of the view's tiles
are widened, the content stays).  One thing the interface leaves open: a writer that stores whole tiles — kta_batch_from_raw
always ("may overwrite the rest of the last tile it touches"), kta_synth_fill_device from a tile boundary — and ends inside
a tile.  The records behind its end, up to the tile's end, are then whatever it left: the model takes them from the
first download after the writer (clobbered()), and from then on every reader has to agree with them like with any record.
On a machine without a GPU (gen_sequence, tests/test_device_batch_model.py) those records keep their old model values:
nothing the generator decides depends on them.

No GPU is needed to import this module, to generate sequences or to run the model; replay() and what it calls need one.
tests/test_gpu_device_batch_sequences.py is the GPU test; the coverage the fixed seed list gives is asserted on the CPU by
tests/test_device_batch_model.py."""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

T = 1024                                  # KTA_TILE_RECORDS
TILES = 6
CAPACITY = TILES * T + 37                 # six whole tiles and an odd tail
N_OPS = 12
SEEDS = tuple(range(20))
BASE_TS = 1_600_000_000_000
EARLY, LATE = BASE_TS - 500_000_000, BASE_TS + 1_500_000_000    # beyond every ordinary timestamp; LATE - EARLY < 2^31
FAR = BASE_TS - (1 << 31)                 # with an ordinary timestamp in the tile: a span of 2^31 and more
VARIANTS = (0, 16, 32, 48)                # temporal / non-temporal loads, with and without summaries
METRIC = (("partition", np.int32, 4), ("key_len", np.int32, 4), ("val_len", np.int32, 4), ("ts_ms", np.int64, 8))
NAMES = tuple(k for k, _, _ in METRIC)
RAW, COMPACT, LENS_I32, LENS_U16 = 0, 1, 0, 1
VALID, TIMED, UNTIMED = 1, 2, 4           # KTA_TILE_SUM_*
PART_NONE = LEN_NONE = 0xFFFF             # KTA_COMPACT_PART_NONE / KTA_COMPACT_LEN_NONE
TIMELINE = (BASE_TS - (1 << 20), 1 << 18, 16)
KEY_BYTES = 1 << 17                       # the Widen op's own key bytes: every key_len of the model has to stay below
VALUE_CLASSES = ("fit", "raw_part", "raw_span", "wide_len", "untimed", "some_untimed", "part_none", "bad_compact", "extreme")
WRITERS = ("Upload", "SynthFill", "Decode", "Widen")
RECORD_SET_SIZES = (37, 40, 701, 1024, 1061, 2048, 2600, CAPACITY)


def P_of(seed):
    return 5 if seed % 2 == 0 else 300    # 300: the packed scan's LDS replication takes another value


def tiles_of(lo, m):
    return range(lo // T, (lo + m + T - 1) // T)


# ---- the ops ------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Upload:
    """kta_batch_from_raw of m records into the view at record lo (a tile boundary).  The columns are upload_cols(op)."""
    lo: int
    m: int
    P: int
    seed: int
    classes: tuple                        # one value class per tile of the range
    view: tuple = (0, CAPACITY)           # the readers' view after this writer: (lo, m)
    extra: bool = False                   # also the analytics / timeline / timestamp-order readers after this writer


@dataclass(frozen=True)
class SynthFill:
    """kta_synth_fill_device of records [first, first + m) of `preset` with `parts` partitions into the view at record lo."""
    lo: int
    m: int
    preset: str
    first: int
    parts: int
    view: tuple = (0, CAPACITY)
    extra: bool = False


@dataclass(frozen=True)
class Decode:
    """kta_kafka_decode_device of the record set of m records (record_set(m)), indexed for `partition`, into the view at record lo."""
    lo: int
    m: int
    partition: int
    view: tuple = (0, CAPACITY)
    extra: bool = False


@dataclass(frozen=True)
class Widen:
    """Both handlers of a -c context over the view [lo, lo + m) with key columns of the caller's own: the lengths of the
    view's tiles are widened; the metrics handler's result is checked like a scan's."""
    lo: int
    m: int
    view: tuple = (0, CAPACITY)
    extra: bool = False


# ---- what the writers write ---------------------------------------------------------------------------------------------
def _tile_values(cls, rng, m, P):
    """One tile's m records of value class cls."""
    p = rng.integers(0, P, m).astype(np.int32)
    k = rng.integers(-1, 40, m).astype(np.int32)
    v = rng.integers(-1, 2000, m).astype(np.int32)
    t = (BASE_TS + 10_000 + rng.integers(0, 1_000_000, m)).astype(np.int64)
    a, b = (int(x) for x in rng.choice(m, 2, replace=False)) if m > 1 else (0, 0)
    if cls == "raw_part":
        p[a] = 65535 if rng.random() < 0.5 else 70000
    elif cls == "raw_span":
        t[a], t[b] = FAR, BASE_TS + 10_000
    elif cls == "wide_len":
        if rng.random() < 0.5:
            v[a] = 65535
        else:
            k[a] = 70000
    elif cls == "untimed":
        t[:] = -1
    elif cls == "some_untimed":
        t[int(rng.integers(0, 7))::7] = -1
    elif cls == "part_none":
        p[a], p[b] = -1, -1
    elif cls == "bad_compact":
        p[a], p[b] = P + 3, 65534
    elif cls == "extreme":
        t[a], t[b] = EARLY, LATE
    else:
        assert cls == "fit", cls
    return p, k, v, t


def upload_cols(op):
    rng = np.random.default_rng([op.seed, op.lo, op.m])
    parts = [_tile_values(cls, rng, min(T, op.m - i * T), op.P) for i, cls in enumerate(op.classes)]
    assert len(op.classes) == (op.m + T - 1) // T
    p, k, v, t = (np.concatenate(x) for x in zip(*parts))
    return {"partition": p, "key_len": k, "val_len": v, "ts_ms": t}


def synth_spec(op):
    import kafka_topic_analyzer_amd as kta
    sp, _ = kta.synth_preset(op.preset)
    sp.n_partitions = op.parts
    return sp


def synth_cols(op):
    import kafka_topic_analyzer_amd as kta
    c = kta.synth_fill_host(synth_spec(op), op.first, op.m)
    return {k: np.array(c[k]) for k in NAMES}


_RECORD_SETS = {}


def record_set(n):
    """-> (blob, batches as kafka_format.expected_columns takes them): n records in uncompressed v2 batches of at most
    150 records; null and empty keys, tombstones and empty values among them.  Built once per process."""
    if n not in _RECORD_SETS:
        import kafka_format as K
        rng = np.random.default_rng(1000 + n)
        blob, batches, left, i = bytearray(), [], n, 0
        while left:
            cnt = min(left, int(rng.integers(60, 151)))
            recs = []
            for _ in range(cnt):
                kl, vl = int(rng.integers(-1, 24)), int(rng.integers(-1, 48))
                recs.append((int(rng.integers(0, 1000)), None if kl < 0 else bytes(kl), None if vl < 0 else bytes(vl)))
            base_ts = BASE_TS + 20_000 + 1000 * i
            blob += K.encode_batch(len(blob), recs, base_ts)
            batches.append((base_ts, 0, max(base_ts + r[0] for r in recs), recs))
            left -= cnt
            i += 1
        _RECORD_SETS[n] = (bytes(blob), batches)
    return _RECORD_SETS[n]


def decode_cols(op):
    import kafka_format as K
    part, klen, vlen, ts, _ = K.expected_columns(op.partition, record_set(op.m)[1])
    return {"partition": np.array(part, np.int32), "key_len": np.array(klen, np.int32), "val_len": np.array(vlen, np.int32),
            "ts_ms": np.array(ts, np.int64)}


def op_cols(op):
    return {"Upload": upload_cols, "SynthFill": synth_cols, "Decode": decode_cols}[type(op).__name__](op)


def stores_whole_tiles(op):
    return isinstance(op, Upload) or (isinstance(op, SynthFill) and op.lo % T == 0)


def clobbered(op):
    """The records behind the writer's end that it may have overwritten: [a, b), empty for most."""
    end = op.lo + op.m
    if not stores_whole_tiles(op) or end % T == 0:
        return end, end
    return end, min((end // T + 1) * T, CAPACITY)


# ---- the model ----------------------------------------------------------------------------------------------------------
class Model:
    """The logical content of an allocation of `capacity` records: four columns, nothing else."""

    def __init__(self, capacity=CAPACITY):
        self.capacity = capacity
        self.cols = {k: np.zeros(capacity, dt) for k, dt, _ in METRIC}

    def apply(self, op):
        if isinstance(op, Widen):
            return
        assert 0 <= op.lo and op.m >= 1 and op.lo + op.m <= self.capacity
        c = op_cols(op)
        for k in NAMES:
            assert len(c[k]) == op.m
            self.cols[k][op.lo:op.lo + op.m] = c[k]

    def cut(self, lo, m):
        return {k: self.cols[k][lo:lo + m] for k in NAMES}

    def tile(self, t):
        return self.cut(t * T, min(T, self.capacity - t * T))


def compactable(p, t):
    """The fit rule of KTA_TILE_COMPACT: every partition in [-1, 65535), the timestamps other than -1 span less than 2^31."""
    stamps = t[t != -1]
    span = int(stamps.max()) - int(stamps.min()) if len(stamps) else 0
    return bool(((p >= -1) & (p < 65535)).all()) and span < (1 << 31)


def lens_fit(k, v):
    return bool(((k >= -1) & (k < 65535) & (v >= -1) & (v < 65535)).all())


def summary_definition(model, tile):
    """What the summary of `tile` may say if it says anything, from the model alone: (ts_base, ts_span, part_max, flags),
    or None where no VALID summary can exist — the model does not hold all 1024 records of the tile, or the compact form
    does not hold them.  ts_base is the header's: the least timestamp other than -1 (0 without one)."""
    c = model.tile(tile)
    p, t = c["partition"], c["ts_ms"]
    if len(p) != T or not compactable(p, t):
        return None
    stamps = t[t != -1]
    lo, hi = (int(stamps.min()), int(stamps.max())) if len(stamps) else (0, 0)
    part_max = int(np.where(p == -1, PART_NONE, p).max())
    flags = VALID | (TIMED if len(stamps) else 0) | (UNTIMED if len(stamps) < T else 0)
    return lo, hi - lo, part_max, flags


# ---- what the generator and the coverage test keep beside the model ---------------------------------------------------------
@dataclass
class Tracker:
    """Per tile: the writer that touched it last, whether that writer wrote it whole in the form that carries a summary
    (a whole tile from a writer that stores whole tiles, content compactable: `summed`), and the writers that ever touched
    it.  All from the ops and the model; nothing from a device."""
    summed: list = field(default_factory=lambda: [False] * (TILES + 1))
    touched: list = field(default_factory=lambda: [[] for _ in range(TILES + 1)])

    def note(self, op, model):
        """After model.apply(op).  -> the tiles this writer cut that were `summed`, as (tile, 'front' | 'back')."""
        cuts = []
        if isinstance(op, Widen):
            for t in tiles_of(op.lo, op.m):
                self.touched[t].append("Widen")
            return cuts
        end = op.lo + op.m
        for t in tiles_of(op.lo, op.m):
            whole = op.lo <= t * T and (t + 1) * T <= end
            if not whole and self.summed[t]:
                if op.lo > t * T:
                    cuts.append((t, "front"))
                if end < (t + 1) * T:
                    cuts.append((t, "back"))
            c = model.tile(t)
            self.summed[t] = whole and stores_whole_tiles(op) and compactable(c["partition"], c["ts_ms"])
            self.touched[t].append(type(op).__name__)
        return cuts


def extreme_tiles(model, P):
    """The tiles that alone hold the earliest / the latest timestamp among the records the scan counts: a set of tiles."""
    p, t = model.cols["partition"], np.where(model.cols["ts_ms"] == -1, 0, model.cols["ts_ms"])
    good = (p >= 0) & (p < P)
    out = set()
    if good.any():
        for x in (t[good].min(), t[good].max()):
            at = np.unique(np.nonzero(good & (t == x))[0] // T)
            if len(at) == 1:
                out.add(int(at[0]))
    return out


# ---- the generator ------------------------------------------------------------------------------------------------------
def _draw_range(rng, kind, granular, sizes=None):
    """(lo, m) of range class `kind`; granular: lo is a tile boundary.  sizes: m must be one of them.  None: not possible."""
    q = lambda x: int(x) // 4 * 4         # a view's columns stay 16-byte aligned
    if kind == "whole":
        lo, m = 0, CAPACITY
    elif kind == "tiles":
        a = int(rng.integers(0, TILES))
        lo, m = a * T, int(rng.integers(1, TILES - a + 1)) * T
    elif kind == "starts_inside":
        if granular:
            return None
        a = int(rng.integers(0, TILES))
        lo = a * T + max(4, q(rng.integers(4, T)))
        lo = min(lo, a * T + T - 4)
        end = int(rng.integers(a + 1, TILES + 1)) * T
        m = end - lo
    elif kind == "ends_inside":
        a = int(rng.integers(0, TILES))
        lo = a * T
        m = int(rng.integers(0, TILES - a)) * T + int(rng.integers(1, T))
    elif kind == "inside_one":
        a = int(rng.integers(0, TILES))
        lo = a * T if granular else a * T + q(rng.integers(0, T - 8))
        m = int(rng.integers(1, (a + 1) * T - lo))
    else:
        assert kind == "last_partial", kind
        lo = int(rng.integers(0, TILES + 1)) * T if granular else q(rng.integers(0, CAPACITY - 1))
        m = CAPACITY - lo
    if sizes is not None:                 # a record set: the size nearest below, the start kept (or moved, for the tail)
        fit = [s for s in sizes if s <= m]
        if not fit:
            return None
        s = max(fit)
        if kind == "last_partial":
            lo = CAPACITY - s
            if lo % 4:
                return None
        elif kind == "starts_inside" and (lo + m - s) % 4 == 0 and (lo + m - s) % T:
            lo = lo + m - s               # (the end stays on its tile boundary)
        m = s
        if kind == "whole" and m != CAPACITY:
            return None
    return lo, m


RANGE_KINDS = ("whole", "tiles", "starts_inside", "ends_inside", "inside_one", "last_partial")


def _draw_view(rng, tracker):
    """The readers' view: half the time one that starts or ends inside a tile that should carry a summary and reaches over
    the tile's other end (the clauses first >= rec0 and first + 1024 <= rec0 + n of the summarised path)."""
    summed = [t for t in range(TILES) if tracker.summed[t]]
    if summed and rng.random() < 0.5:
        t = summed[int(rng.integers(0, len(summed)))]
        if rng.random() < 0.5 and t + 1 <= TILES:          # starts inside t, ends behind it
            lo = t * T + int(rng.integers(1, T // 4)) * 4
            end = int(rng.integers((t + 1) * T, CAPACITY + 1))
            return lo, end - lo
        if t > 0:                                          # starts before t, ends inside it
            lo = int(rng.integers(0, t * T // 4 + 1)) * 4
            end = t * T + int(rng.integers(1, T))
            return lo, end - lo
    lo, m = _draw_range(rng, RANGE_KINDS[int(rng.integers(1, len(RANGE_KINDS)))], False)
    return lo, m


def gen_sequence(seed, capacity=CAPACITY, P=None, n_ops=N_OPS):
    """The ops of sequence `seed`: n_ops writers, the first over the whole capacity, each with its readers' view; one of
    them, chosen by the seed, with extra=True.  Widen ops only in the seeds with seed // 2 odd (their sequence runs on the -c
    handler).  Deterministic; needs no GPU."""
    assert capacity == CAPACITY
    P = P_of(seed) if P is None else P
    rng = np.random.default_rng(77_000 + seed)
    with_widen = (seed // 2) % 2 == 1
    model, tracker, ops = Model(), Tracker(), []
    extra_at = int(rng.integers(1, n_ops))
    while len(ops) < n_ops:
        first_op = not ops
        writers = ["Upload", "SynthFill", "Decode"] + (["Widen"] if with_widen and not first_op else [])
        weights = np.array([4, 3, 3, 2][:len(writers)], float)
        w = writers[int(rng.choice(len(writers), p=weights / weights.sum()))]
        kind = "whole" if first_op else RANGE_KINDS[int(rng.choice(len(RANGE_KINDS), p=[0.06, 0.2, 0.2, 0.22, 0.2, 0.12]))]
        summed = [t for t in range(TILES) if tracker.summed[t]]
        r = None
        if not first_op and summed and w in ("SynthFill", "Decode") and rng.random() < 0.45:
            # aim at a tile that should carry a summary: cut it at its front or at its back
            t = summed[int(rng.integers(0, len(summed)))]
            if w == "Decode":
                s = int(rng.choice([x for x in RECORD_SET_SIZES if x < 2 * T]))
                lo = (t * T + T - 40 if s <= 40 else t * T + T // 2) if rng.random() < 0.5 else max(0, t * T + 200 - s) // 4 * 4
                r = (lo, s) if lo + s <= CAPACITY else None
            elif rng.random() < 0.5:
                lo = t * T + int(rng.integers(1, T // 4)) * 4
                r = (lo, int(rng.integers(1, CAPACITY - lo + 1)))
            else:
                lo = int(rng.integers(0, t + 1)) * T
                r = (lo, t * T + int(rng.integers(1, T)) - lo)
        if r is None:
            r = _draw_range(rng, kind, w == "Upload", RECORD_SET_SIZES if w == "Decode" else None)
        if r is None:
            continue
        lo, m = r
        if w == "Upload":
            n_t = (m + T - 1) // T
            classes = tuple(VALUE_CLASSES[int(rng.choice(len(VALUE_CLASSES), p=[0.3, 0.07, 0.07, 0.08, 0.07, 0.09, 0.08, 0.09, 0.15]))]
                            for _ in range(n_t))
            op = Upload(lo, m, P, int(rng.integers(0, 1 << 30)), classes)
        elif w == "SynthFill":
            preset = "c2" if rng.random() < 0.5 else "c4"
            parts = P if rng.random() < 0.7 else (8 if preset == "c2" else 256)
            op = SynthFill(lo, m, preset, int(rng.integers(0, 1_000_000)), parts)
        elif w == "Decode":
            op = Decode(lo, m, int(rng.choice([0, P - 1, P + 2, 70000, -1], p=[0.35, 0.35, 0.1, 0.1, 0.1])))
        else:
            op = Widen(lo, m)
        model.apply(op)
        tracker.note(op, model)
        op = type(op)(**{**op.__dict__, "view": _draw_view(rng, tracker), "extra": len(ops) == extra_at})
        ops.append(op)
    return ops


# ---- the device side ----------------------------------------------------------------------------------------------------
def first_difference(got, want):
    """'' when equal, else 'index i: got x, want y' of the first differing element."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shape {got.shape}, want {want.shape}"
    d = np.nonzero(got.ravel() != want.ravel())[0]
    return "" if not len(d) else f"index {int(d[0])}: got {got.ravel()[d[0]]}, want {want.ravel()[d[0]]} ({len(d)} differ)"


def same(got, want, what):
    d = first_difference(got, want)
    assert not d, f"{what}: {d}"


class Device:
    """One handler and what the ops need beside the allocation under test: the record sets' blobs on the device and, on a
    -c handler, key columns of its own for Widen (every key is the same zero bytes: key_off is 0 everywhere)."""

    def __init__(self, h, keyed=False):
        self.h, self.P, self.keyed = h, h.n_partitions, keyed
        self.blobs, self.keys = {}, None

    def view(self, b, lo):
        import kafka_topic_analyzer_amd as kta
        v = kta.KtaBatch()
        for k, _, sz in METRIC:
            setattr(v, k, getattr(b, k) + lo * sz)
        v.capacity = CAPACITY - lo
        return v

    def blob(self, n):
        """-> (device pointer, length, descriptors, batches) of record set n for partition id 0 (the caller sets the id)."""
        from kafka_topic_analyzer_amd import _native as N
        if n not in self.blobs:
            h, blob = self.h, record_set(n)[0]
            dev = h.device_batch_alloc((((len(blob) + 127) & ~63) + 128) // 4 + 1)
            arr = np.frombuffer(blob + b"\0" * ((-len(blob)) % 16), dtype=np.uint8).copy()
            h._check(h._lib.kta_copy_to_device(h._ctx, dev.partition, arr.ctypes.data, arr.nbytes))
            self.blobs[n] = (dev, blob)
        return self.blobs[n]

    def key_columns(self):
        if self.keys is None:
            h = self.h
            self.keys = h.device_batch_alloc(CAPACITY, KEY_BYTES)
            for ptr, nbytes in ((self.keys.key_off, (TILES + 1) * T * 4), (self.keys.key_bytes, KEY_BYTES)):
                z = np.zeros(nbytes, np.uint8)
                h._check(h._lib.kta_copy_to_device(h._ctx, ptr, z.ctypes.data, z.nbytes))
        return self.keys

    def free(self):
        for dev, _ in self.blobs.values():
            self.h.device_batch_free(dev)
        if self.keys is not None:
            self.h.device_batch_free(self.keys)
        self.blobs, self.keys = {}, None


def apply_device(dev, b, op, model):
    """The writer on the device, then on the model (the records it may have clobbered: from the device)."""
    import kafka_topic_analyzer_amd as kta
    from kafka_topic_analyzer_amd import _native as N
    h = dev.h
    v = dev.view(b, op.lo)
    if isinstance(op, Upload):
        c = {k: np.ascontiguousarray(x) for k, x in upload_cols(op).items()}
        h._check(h._lib.kta_batch_from_raw(h._ctx, C.byref(kta._host_batch(c)), op.m, C.byref(v)))
    elif isinstance(op, SynthFill):
        h.synth_fill_device(synth_spec(op), op.first, op.m, v)
    elif isinstance(op, Decode):
        blob_dev, blob = dev.blob(op.m)
        st = N.KtaKafkaIndexStats()
        descs = (N.KtaKafkaBatchDesc * 256)()
        rc = h._lib.kta_kafka_index_host(blob, len(blob), op.partition, 0, 0, (len(blob) + 127) & ~63, descs, 256, C.byref(st))
        assert rc == N.KTA_OK and st.n_records == op.m, (rc, st.n_records)
        bad = C.c_uint64()
        h._check(h._lib.kta_kafka_decode_device(h._ctx, blob_dev.partition, len(blob), descs, st.n_batches, op.m, C.byref(v), None,
                                                C.byref(bad)))
        assert bad.value == 0
    elif dev.keyed:
        assert int(model.cols["key_len"].max()) <= KEY_BYTES - 16, "a key of the model is longer than Widen's key bytes"
        keys = dev.key_columns()
        v.key_off, v.key_bytes = keys.key_off, keys.key_bytes
        # both handlers: the lengths are widened, then the alive-key pass reads the view (at most 256 partitions: the
        # fused pass, which does the metrics handler's work as well — a reader of partitions and timestamps of its own)
        h.reset()
        h.submit_device(v, op.m, 0, which=3)
        check_finish(dev, _oracle_result(dev.P, model.cut(op.lo, op.m)), f"both handlers over the view ({op.lo}, {op.m})")
    # (a Widen on a handler without -c is left out: the content is the same, the tiles keep their u16 lengths)
    model.apply(op)
    a, e = clobbered(op)
    if e > a:
        got = h.download_batch(dev.view(b, a), e - a)
        for k in NAMES:
            model.cols[k][a:e] = got[k]


def read_layout(dev, b):
    """-> [(ts_base, mode, lens)] and the summaries of the allocation's tiles."""
    h = dev.h
    raw = np.empty(2 * (TILES + 1), np.uint64)
    h._check(h._lib.kta_copy_to_host(h._ctx, raw.ctypes.data, b.tile_hdr, raw.nbytes))
    hdrs = [(int(raw[2 * t].view(np.int64)), int(raw[2 * t + 1]) & 0xFFFFFFFF, int(raw[2 * t + 1]) >> 32) for t in range(TILES + 1)]
    return hdrs, h.batch_tile_summaries(b, CAPACITY)


def check_layout(model, hdrs, sums):
    """Headers and summaries are sound for the model's content."""
    for t, (base, mode, lens) in enumerate(hdrs):
        c = model.tile(t)
        assert mode in (RAW, COMPACT) and lens in (LENS_I32, LENS_U16), f"tile {t}: header mode {mode}, lens {lens}"
        if mode == COMPACT:
            assert compactable(c["partition"], c["ts_ms"]), f"tile {t}: a COMPACT header over content the compact form does not hold"
        if lens == LENS_U16:
            assert lens_fit(c["key_len"], c["val_len"]), f"tile {t}: u16 lengths over a length that does not fit"
        span, part_max, flags = int(sums["ts_span"][t]), int(sums["part_max"][t]), int(sums["flags"][t])
        if mode == COMPACT and flags & VALID:
            want = summary_definition(model, t)
            assert want is not None, f"tile {t}: a VALID summary of a tile that is not 1024 compactable records"
            got = (base if flags & TIMED else want[0], span, part_max, flags)
            if not flags & TIMED:
                assert base == 0, f"tile {t}: ts_base {base} without a timed record"
            assert got == want, f"tile {t}: summary (ts_base, ts_span, part_max, flags) {got}, the definition gives {want}"


def _oracle_result(P, cols):
    from helpers import NOW
    from oracle_c import Oracle
    p = cols["partition"]
    good = (p >= 0) & (p < P)
    o = Oracle(NOW)
    o.run_soa({k: np.ascontiguousarray(cols[k][good]) for k in NAMES})
    want = {"counters": o.counters(P), "earliest": o.earliest(), "latest": o.latest(), "smallest": o.get("smallest_message"),
            "largest": o.get("largest_message"), "overall_count": o.get("overall_count"), "overall_size": o.get("overall_size"),
            "bad_partition_records": int((~good).sum())}
    o.close()
    return want


def check_finish(dev, want, what):
    """finish() of dev's handler against an _oracle_result."""
    import kafka_topic_analyzer_amd as kta
    h = dev.h
    res, c = h.finish(allow_bad_partition=True)
    mm = kta.MessageMetrics(res, c, h.now)
    same(c, want["counters"], f"{what}: counters[P, 7]")
    got = {"earliest": mm.earliest_message(), "latest": mm.latest_message(), "smallest": mm.smallest_message(),
           "largest": mm.largest_message(), "overall_count": int(res.overall_count), "overall_size": int(res.overall_size),
           "bad_partition_records": int(res.bad_partition_records)}
    for k, g in got.items():
        assert g == want[k], f"{what}: {k} {g}, the oracle gives {want[k]}"


def check_scan(dev, batch, n, cols, what):
    """submit_device(which=1) of `batch` under the four scan variants against the C oracle on `cols`."""
    h = dev.h
    want = _oracle_result(dev.P, cols)
    for sv in VARIANTS:
        h.set_tuning(scan_variant=sv)
        h.reset()
        h.submit_device(batch, n, 0, which=1)
        check_finish(dev, want, f"{what}, scan variant {sv}")
    h.set_tuning()


def check_download(dev, b, model, lo, m, what):
    got = dev.h.download_batch(dev.view(b, lo) if lo else b, m)
    for k in NAMES:
        same(got[k], model.cols[k][lo:lo + m], f"{what}: {k}")


def run_readers(dev, b, op, model):
    lo, m = op.view
    check_download(dev, b, model, 0, CAPACITY, "download of the allocation")
    check_download(dev, b, model, lo, m, f"download of the view {op.view}")
    check_layout(model, *read_layout(dev, b))
    check_scan(dev, b, CAPACITY, model.cols, "scan of the allocation")
    check_scan(dev, dev.view(b, lo), m, model.cut(lo, m), f"scan of the view {op.view}")
    check_download(dev, b, model, 0, CAPACITY, "download after the readers")
    check_layout(model, *read_layout(dev, b))


def run_extra_readers(dev, b, op, model):
    """On a handler with analytics, a timeline and the timestamp order: the allocation and the view against the Python
    restatements."""
    import analytics_py as AP
    import timeline_py as TL
    import ts_order_py as TS
    h, P = dev.h, dev.P
    for (lo, m), batch in (((0, CAPACITY), b), (op.view, dev.view(b, op.view[0]))):
        cols = model.cut(lo, m)
        good = (cols["partition"] >= 0) & (cols["partition"] < P)
        counted = {k: cols[k][good] for k in NAMES}
        h.reset()
        h.submit_device(batch, m, 0, which=1)
        what = f"records [{lo}, {lo + m})"
        got, want = h.analytics(), AP.decode(AP.analytics_vector(counted, P), P)
        for k in want:
            same(got[k], want[k], f"analytics of {what}: {k}")
        same(h.timeline(), TL.timeline_vector(cols, P, *TIMELINE), f"timeline of {what}")
        same(h.ts_order()["vector"], TS.vector_of(P, cols["partition"], cols["ts_ms"]), f"timestamp order of {what}")
        res, _ = h.finish(allow_bad_partition=True)
        assert int(res.bad_partition_records) == int((~good).sum()), f"bad_partition_records of {what}"


def format_ops(ops):
    return "[\n" + "".join(f"    {op!r},\n" for op in ops) + "]"


def replay(dev, ops, upto=None, readers=True, seed=None, extra_dev=None):
    """Run ops[:upto] on a fresh allocation of dev's handler, the readers after every writer (readers=False: only the
    writers).  extra_dev: the handler with analytics, a timeline and the timestamp order, for the op with extra=True — it
    replays the writers up to that op on an allocation of its own and must arrive at the same model.  A failure names the
    seed, the ops up to the failing one — paste them into a regression test: replay(Device(h), ops) — and the first
    differing field.  -> the model."""
    ops = list(ops[:upto])
    model = Model()
    b = dev.h.device_batch_alloc(CAPACITY)
    try:
        for k, op in enumerate(ops):
            try:
                apply_device(dev, b, op, model)
                if readers:
                    run_readers(dev, b, op, model)
                if readers and op.extra and extra_dev is not None:
                    bx = extra_dev.h.device_batch_alloc(CAPACITY)
                    try:
                        mx = Model()
                        for o in ops[:k + 1]:
                            apply_device(extra_dev, bx, o, mx)
                        for name in NAMES:
                            same(mx.cols[name], model.cols[name], f"the same writers on a second handler: {name}")
                        run_extra_readers(extra_dev, bx, op, model)
                    finally:
                        extra_dev.h.device_batch_free(bx)
            except AssertionError as e:
                raise AssertionError(f"seed {seed}, P {dev.P}, after op {k} of\nops = {format_ops(ops[:k + 1])}\n{e}") from None
    finally:
        dev.h.set_tuning()
        dev.h.device_batch_free(b)
    return model

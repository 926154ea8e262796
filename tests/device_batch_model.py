"""A stateful model of one device batch (include/kta_hip.h, "Device batch layouts"; csrc/kta_tile.h): random sequences of
writers over ONE tile-compact allocation, a plain numpy model of what record i logically is, and after every writer every
reader against the model, bit for bit.

The model (Model) knows nothing of headers, compact forms, summaries or planes.  What the device keeps beside the records
— a header, a summary, a plane mark and two size words per tile, and a marked tile's scan plane in the second half of its
ts_ms bytes — is checked for SOUNDNESS against the model (check_layout): a COMPACT header only over content the compact
form holds, u16 lengths only over lengths that fit, a VALID summary beside a COMPACT header equal to
summary_definition() of the model's tile, and beside both a mark of 1 only over plane_definition()'s words and sizes.  A
zero summary is always acceptable, and so is a mark of 0 — except on a tile that the last writer wrote whole: there
header, summary and mark are what the content asks for (the rule "written in the same step" of csrc/kta_tile.h).

Readers: kta_batch_to_raw, the scan under VARIANTS, the same scan behind the record filter (two windows per writer, drawn
onto the bounds of a summary: filter_py says which records pass and at most how many tiles header and summary may
decide), and on a second handler the opt-in passes with tile-form loaders of their own.

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
OLD_SEEDS = tuple(range(20))              # their ops are pinned by tests/golden/device_batch_sequences.sha256
PLANE_SEEDS = tuple(range(20, 32))        # profile "plane": the value classes and the aims that reach scan planes and size words
SEEDS = OLD_SEEDS + PLANE_SEEDS
BASE_TS = 1_600_000_000_000
EARLY, LATE = BASE_TS - 500_000_000, BASE_TS + 1_500_000_000    # beyond every ordinary timestamp; LATE - EARLY < 2^31
FAR = BASE_TS - (1 << 31)                 # with an ordinary timestamp in the tile: a span of 2^31 and more
VARIANTS = (0, 16, 32, 48, 64, 80)        # temporal / non-temporal loads; with summaries, without, with summaries but no planes
METRIC = (("partition", np.int32, 4), ("key_len", np.int32, 4), ("val_len", np.int32, 4), ("ts_ms", np.int64, 8))
NAMES = tuple(k for k, _, _ in METRIC)
RAW, COMPACT, LENS_I32, LENS_U16 = 0, 1, 0, 1
VALID, TIMED, UNTIMED = 1, 2, 4           # KTA_TILE_SUM_*
PART_NONE = LEN_NONE = 0xFFFF             # KTA_COMPACT_PART_NONE / KTA_COMPACT_LEN_NONE
TIMELINE = (BASE_TS - (1 << 20), 1 << 18, 16)
KEY_BYTES = 1 << 17                       # the Widen op's own key bytes: every key_len of the model has to stay below
VALUE_CLASSES = ("fit", "raw_part", "raw_span", "wide_len", "untimed", "some_untimed", "part_none", "bad_compact", "extreme")
PLANE_CLASSES = ("plane_edge", "key_255", "part_256", "no_values", "size_extreme")     # drawn by the plane profile only
WRITERS = ("Upload", "SynthFill", "Decode", "Widen")
PLANE_PARTS, PLANE_KEY_NONE = 256, 0xFF   # KTA_PLANE_PARTS / KTA_PLANE_KEY_NONE
KEY_MAX, VAL_MAX = 254, 65534             # the largest lengths that fit a plane
SIZE_NONE = (0xFFFFFFFF, 0)               # kTileSizeMinNone / kTileSizeMaxNone: the size words of a tile without a valued record
SIDE_BEFORE_SIZES = 16 + 8 + 4            # kta_tile.h's address rule: headers, summaries, marks, then the size words
SEGMENTS = (4096, 8, 7)                   # the extra handler's segment pass: (segment_bytes, rows_per_partition, record_overhead)
WINDOW_KINDS = ("exact", "drop_latest", "drop_earliest", "behind", "before", "set", "both")
RECORD_SET_SIZES = (37, 40, 701, 1024, 1061, 2048, 2600, CAPACITY)


def P_of(seed):
    if seed in PLANE_SEEDS:               # 256: every id of a plane is a partition; 300: marked tiles under more partitions
        return (5, 256, 300)[(seed - PLANE_SEEDS[0]) % 3]
    return 5 if seed % 2 == 0 else 300    # 300: the packed scan's LDS replication takes another value


def profile_of(seed):
    return "plane" if seed in PLANE_SEEDS else "mixed"


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
    windows: tuple = ()                   # the filtered readers after this writer: (kind, aimed tile | None, from_ms, to_ms, partitions)
    ids: int = 0                          # the partition ids are drawn from [0, ids); 0: from [0, P)


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
    windows: tuple = ()


@dataclass(frozen=True)
class Decode:
    """kta_kafka_decode_device of the record set of m records (record_set(m)), indexed for `partition`, into the view at record lo."""
    lo: int
    m: int
    partition: int
    view: tuple = (0, CAPACITY)
    extra: bool = False
    windows: tuple = ()


@dataclass(frozen=True)
class Widen:
    """Both handlers of a -c context over the view [lo, lo + m) with key columns of the caller's own: the lengths of the
    view's tiles are widened; the metrics handler's result is checked like a scan's."""
    lo: int
    m: int
    view: tuple = (0, CAPACITY)
    extra: bool = False
    windows: tuple = ()


# ---- what the writers write ---------------------------------------------------------------------------------------------
def _tile_values(cls, rng, m, P, ids=0):
    """One tile's m records of value class cls.  The ids of the plane classes stay below 256 whatever P is."""
    cap = min(ids or P, PLANE_PARTS) if cls in PLANE_CLASSES else (ids or P)
    p = rng.integers(0, cap, m).astype(np.int32)
    k = rng.integers(-1, 40, m).astype(np.int32)
    v = rng.integers(-1, 2000, m).astype(np.int32)
    t = (BASE_TS + 10_000 + rng.integers(0, 1_000_000, m)).astype(np.int64)
    a, b = (int(x) for x in rng.choice(m, 2, replace=False)) if m > 1 else (0, 0)
    if cls == "plane_edge":               # the largest id, key and value a plane holds, both sentinels, zeros, a uniform quad
        q = int(rng.integers(0, max(m // 4, 1))) * 4
        p[q:q + 4], k[q:q + 4], v[q:q + 4] = p[q], k[q], v[q]
        at = [int(x) for x in rng.permutation(m) if not q <= x < q + 4][:4]
        for i, (pp, kk, vv) in zip(at, ((cap - 1, None, None), (None, KEY_MAX, VAL_MAX), (None, -1, -1), (None, 0, 0))):
            p[i] = p[i] if pp is None else pp
            k[i], v[i] = (k[i], v[i]) if kk is None else (kk, vv)
    elif cls == "key_255":
        k[a] = KEY_MAX + 1
    elif cls == "part_256":
        p[a] = PLANE_PARTS
    elif cls == "no_values":
        v[:] = -1
    elif cls == "size_extreme":           # every size in a middle band, but one of 0 and one of the largest a plane holds
        k[:], v[:] = rng.integers(10, 40, m), rng.integers(100, 1000, m)
        k[a], v[a] = -1, 0
        if b != a:
            k[b], v[b] = KEY_MAX, VAL_MAX
    elif cls == "raw_part":
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
    parts = [_tile_values(cls, rng, min(T, op.m - i * T), op.P, op.ids) for i, cls in enumerate(op.classes)]
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


def plane_fits(p, k, v):
    """The fit rule of a scan plane (kta_tile.h, tile_plane_fits): an id in [0, 256), a key length in [-1, 255), a value
    length in [-1, 65535)."""
    return bool(((p >= 0) & (p < PLANE_PARTS) & (k >= -1) & (k < PLANE_KEY_NONE) & (v >= -1) & (v < LEN_NONE)).all())


def plane_definition(model, tile):
    """What a mark of 1 on `tile` vouches for, from the model alone: (the plane's 1024 words p | (k & 0xFF) << 8 |
    (v & 0xFFFF) << 16, (size_min, size_max) — the least and the largest key_len + val_len over the records with a value, a
    key of -1 counting as 0; SIZE_NONE without one), or None where no tile of this content can be marked: it is not 1024
    compactable records that all fit."""
    c = model.tile(tile)
    p, k, v = (c[name].astype(np.int64) for name in ("partition", "key_len", "val_len"))
    if len(p) != T or not compactable(c["partition"], c["ts_ms"]) or not plane_fits(p, k, v):
        return None
    words = (p | ((k & 0xFF) << 8) | ((v & 0xFFFF) << 16)).astype(np.uint32)
    sz = (np.maximum(k, 0) + v)[v != -1]
    return words, ((int(sz.min()), int(sz.max())) if len(sz) else SIZE_NONE)


# ---- what the generator and the coverage test keep beside the model ---------------------------------------------------------
@dataclass
class Tracker:
    """Per tile: the writer that touched it last, whether that writer wrote it whole in the form that carries a summary
    (a whole tile from a writer that stores whole tiles, content compactable: `summed`), and the writers that ever touched
    it.  `marked`: a summed tile of which every record fits a scan plane (plane_definition), so that its writer had to
    mark it — the name of that writer, or None; `was_cut`: the tile was once cut while it was summed.  marked_cuts: what
    the last note() cut of marked tiles, widened: the marked tiles the last Widen reached.  All from the ops and the
    model; nothing from a device."""
    summed: list = field(default_factory=lambda: [False] * (TILES + 1))
    touched: list = field(default_factory=lambda: [[] for _ in range(TILES + 1)])
    marked: list = field(default_factory=lambda: [None] * (TILES + 1))
    was_cut: list = field(default_factory=lambda: [False] * (TILES + 1))
    marked_cuts: list = field(default_factory=list)
    widened: list = field(default_factory=list)

    def note(self, op, model):
        """After model.apply(op).  -> the tiles this writer cut that were `summed`, as (tile, 'front' | 'back')."""
        cuts, self.marked_cuts, self.widened = [], [], []
        if isinstance(op, Widen):
            for t in tiles_of(op.lo, op.m):
                self.touched[t].append("Widen")
                if self.marked[t]:
                    self.widened.append(t)
            return cuts
        end = op.lo + op.m
        for t in tiles_of(op.lo, op.m):
            whole = op.lo <= t * T and (t + 1) * T <= end
            if not whole and self.summed[t]:
                sides = (["front"] if op.lo > t * T else []) + (["back"] if end < (t + 1) * T else [])
                cuts += [(t, side) for side in sides]
                self.marked_cuts += [(t, side) for side in sides if self.marked[t]]
                self.was_cut[t] = True
            c = model.tile(t)
            self.summed[t] = whole and stores_whole_tiles(op) and compactable(c["partition"], c["ts_ms"])
            self.marked[t] = type(op).__name__ if self.summed[t] and plane_definition(model, t) is not None else None
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


def size_extreme_tiles(model, P):
    """extreme_tiles for sizes: the tiles that alone hold the smallest / the largest key + value size among the records the
    scan counts and that have a value."""
    p, k, v = model.cols["partition"], model.cols["key_len"].astype(np.int64), model.cols["val_len"].astype(np.int64)
    sized = (p >= 0) & (p < P) & (v != -1)
    sz = np.maximum(k, 0) + v
    out = set()
    if sized.any():
        for x in (sz[sized].min(), sz[sized].max()):
            at = np.unique(np.nonzero(sized & (sz == x))[0] // T)
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


def _aim_tiles(tracker, plane):
    """The tiles the generator aims cuts and views at: those that should carry a summary; in the plane profile those that
    should carry a mark, where there is one."""
    summed = [t for t in range(TILES) if tracker.summed[t]]
    marked = [t for t in summed if tracker.marked[t]]
    return marked if plane and marked else summed


def _draw_view(rng, tracker, plane=False):
    """The readers' view: half the time one that starts or ends inside a tile that should carry a summary and reaches over
    the tile's other end (the clauses first >= rec0 and first + 1024 <= rec0 + n of the summarised path)."""
    summed = _aim_tiles(tracker, plane)
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


def _draw_windows(rng, model, tracker, view, P):
    """The filters of the filtered readers after one writer: two of WINDOW_KINDS, each aimed at a tile that should carry a
    summary (one that was cut earlier and written whole again, where there is one), so that the window's bounds sit on
    that summary's own: -> ((kind, aimed tile | None, from_ms, to_ms, partitions | None), ...).  Without such a tile the
    bounds come from the view's timestamps."""
    out = []
    summed = [t for t in range(TILES) if tracker.summed[t]]
    recut = [t for t in summed if tracker.was_cut[t]]
    for kind in (WINDOW_KINDS[int(i)] for i in rng.choice(len(WINDOW_KINDS), 2, replace=False)):
        pool = recut if recut and rng.random() < 0.7 else summed
        aim = pool[int(rng.integers(0, len(pool)))] if pool else None
        c = model.tile(aim) if aim is not None else model.cut(*view)
        stamps = c["ts_ms"][c["ts_ms"] != -1]
        lo, hi = (int(stamps.min()), int(stamps.max())) if len(stamps) else (BASE_TS, BASE_TS)
        bounds = {"exact": (lo, hi + 1), "drop_latest": (lo, hi) if lo < hi else (None, hi), "drop_earliest": (lo + 1, None),
                  "behind": (hi + 1, None), "before": (None, lo), "set": (None, None)}
        frm, to = bounds[("exact", "drop_latest", "drop_earliest")[int(rng.integers(0, 3))] if kind == "both" else kind]
        parts = None
        if kind in ("set", "both"):                        # a few partitions, of those the aimed records have where they have any
            ids = np.unique(c["partition"][(c["partition"] >= 0) & (c["partition"] < P)])
            ids = ids if len(ids) and rng.random() < 0.8 else np.arange(P)
            parts = tuple(sorted(int(x) for x in rng.choice(ids, min(len(ids), int(rng.integers(1, 5))), replace=False)))
        out.append((kind, aim, frm, to, parts))
    return tuple(out)


PLANE_CLASS_WEIGHTS = dict(fit=0.2, raw_part=0.03, raw_span=0.03, wide_len=0.04, untimed=0.05, some_untimed=0.05, part_none=0.04,
                           bad_compact=0.04, extreme=0.08, plane_edge=0.12, key_255=0.07, part_256=0.07, no_values=0.09,
                           size_extreme=0.09)


def gen_sequence(seed, capacity=CAPACITY, P=None, n_ops=N_OPS, profile=None):
    """The ops of sequence `seed`: n_ops writers, the first over the whole capacity, each with its readers' view and its
    filtered readers' windows; one of them, chosen by the seed, with extra=True.  Widen ops only in the seeds with
    seed // 2 odd (their sequence runs on the -c handler).  profile "plane" (the seeds of PLANE_SEEDS): the upload classes
    of PLANE_CLASSES as well, ids below 256 under a handler of more partitions, and cuts, views and Widen ops aimed at
    marked tiles.  The windows come from a random stream of their own, so that the ops of OLD_SEEDS are, but for them,
    what they were (tests/golden/device_batch_sequences.sha256).  Deterministic; needs no GPU."""
    assert capacity == CAPACITY
    P = P_of(seed) if P is None else P
    plane = (profile_of(seed) if profile is None else profile) == "plane"
    rng = np.random.default_rng(77_000 + seed)
    with_widen = (seed // 2) % 2 == 1
    model, tracker, ops = Model(), Tracker(), []
    extra_at = int(rng.integers(1, n_ops))
    classes_of = PLANE_CLASS_WEIGHTS if plane else dict(zip(VALUE_CLASSES, [0.3, 0.07, 0.07, 0.08, 0.07, 0.09, 0.08, 0.09, 0.15]))
    class_names, class_p = list(classes_of), list(classes_of.values())
    while len(ops) < n_ops:
        first_op = not ops
        writers = ["Upload", "SynthFill", "Decode"] + (["Widen"] if with_widen and not first_op else [])
        weights = np.array([4, 3, 3, 2][:len(writers)], float)
        w = writers[int(rng.choice(len(writers), p=weights / weights.sum()))]
        kind = "whole" if first_op else RANGE_KINDS[int(rng.choice(len(RANGE_KINDS), p=[0.06, 0.2, 0.2, 0.22, 0.2, 0.12]))]
        aims = _aim_tiles(tracker, plane)
        r = None
        if not first_op and aims and w in ("SynthFill", "Decode") + (("Upload", "Widen") if plane else ()) and \
                rng.random() < (0.6 if plane else 0.45):
            # aim at a tile that should carry a summary (a mark): cut it at its front or at its back
            t = aims[int(rng.integers(0, len(aims)))]
            if w == "Decode":
                s = int(rng.choice([x for x in RECORD_SET_SIZES if x < 2 * T]))
                lo = (t * T + T - 40 if s <= 40 else t * T + T // 2) if rng.random() < 0.5 else max(0, t * T + 200 - s) // 4 * 4
                r = (lo, s) if lo + s <= CAPACITY else None
            elif w != "Upload" and rng.random() < 0.5:     # (an upload starts at a tile boundary: it cuts at the back)
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
            classes = tuple(class_names[int(rng.choice(len(class_names), p=class_p))] for _ in range(n_t))
            ids = PLANE_PARTS if plane and P > PLANE_PARTS else 0      # marked tiles under a handler of more partitions
            op = Upload(lo, m, P, int(rng.integers(0, 1 << 30)), classes, ids=ids)
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
        view = _draw_view(rng, tracker, plane)
        windows = _draw_windows(np.random.default_rng([77_001, seed, len(ops)]), model, tracker, view, P)
        op = type(op)(**{**op.__dict__, "view": view, "extra": len(ops) == extra_at, "windows": windows})
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
    """-> [(ts_base, mode, lens)], the summaries, the marks and the size words [tile, 2] of the allocation's tiles, and the
    second half of the ts_ms bytes of its TILES whole tiles as words [tile, 1024] (where a marked tile keeps its plane)."""
    h = dev.h
    raw = np.empty(2 * (TILES + 1), np.uint64)
    h._check(h._lib.kta_copy_to_host(h._ctx, raw.ctypes.data, b.tile_hdr, raw.nbytes))
    hdrs = [(int(raw[2 * t].view(np.int64)), int(raw[2 * t + 1]) & 0xFFFFFFFF, int(raw[2 * t + 1]) >> 32) for t in range(TILES + 1)]
    assert (b.capacity + T - 1) // T == TILES + 1
    sizes = np.empty((TILES + 1, 2), np.uint32)
    h._check(h._lib.kta_copy_to_host(h._ctx, sizes.ctypes.data, b.tile_hdr + (TILES + 1) * SIDE_BEFORE_SIZES, sizes.nbytes))
    ts = np.empty((TILES, 2 * T), np.uint32)
    h._check(h._lib.kta_copy_to_host(h._ctx, ts.ctypes.data, b.ts_ms, ts.nbytes))
    return hdrs, h.batch_tile_summaries(b, CAPACITY), h.batch_tile_planes(b, CAPACITY), sizes, ts[:, T:]


def wrote_whole(op):
    """The whole tiles (of the TILES) that `op` wrote whole as a writer that stores whole tiles: where it had to write header,
    summary and mark in the same step."""
    if not stores_whole_tiles(op):
        return []
    return [t for t in tiles_of(op.lo, op.m) if t < TILES and op.lo <= t * T and (t + 1) * T <= op.lo + op.m]


def check_layout(model, hdrs, sums, marks, sizes, planes, wrote=()):
    """Headers, summaries, marks, planes and size words are sound for the model's content; wrote: the tiles the last writer
    wrote whole (wrote_whole) — of those, every compactable one has a COMPACT header, a VALID summary and the mark that
    plane_definition asks for.  A mark next to a RAW header or a summary that is not VALID says nothing and is not judged."""
    for t, (base, mode, lens) in enumerate(hdrs):
        c = model.tile(t)
        assert mode in (RAW, COMPACT) and lens in (LENS_I32, LENS_U16), f"tile {t}: header mode {mode}, lens {lens}"
        if mode == COMPACT:
            assert compactable(c["partition"], c["ts_ms"]), f"tile {t}: a COMPACT header over content the compact form does not hold"
        if lens == LENS_U16:
            assert lens_fit(c["key_len"], c["val_len"]), f"tile {t}: u16 lengths over a length that does not fit"
        span, part_max, flags, mark = int(sums["ts_span"][t]), int(sums["part_max"][t]), int(sums["flags"][t]), int(marks[t])
        assert mark in (0, 1), f"tile {t}: mark {mark}"
        plane = plane_definition(model, t)
        trusted = mode == COMPACT and bool(flags & VALID)
        if trusted and mark == 1:
            assert plane is not None, f"tile {t}: a mark of 1 on a tile that is not 1024 compactable records that all fit a plane"
        if trusted:
            want = summary_definition(model, t)
            assert want is not None, f"tile {t}: a VALID summary of a tile that is not 1024 compactable records"
            got = (base if flags & TIMED else want[0], span, part_max, flags)
            if not flags & TIMED:
                assert base == 0, f"tile {t}: ts_base {base} without a timed record"
            assert got == want, f"tile {t}: summary (ts_base, ts_span, part_max, flags) {got}, the definition gives {want}"
        if trusted and mark == 1:
            same(planes[t], plane[0], f"tile {t}: the plane's words behind a mark of 1")
            got = (int(sizes[t][0]), int(sizes[t][1]))
            assert got == plane[1], f"tile {t}: size words (size_min, size_max) {got} behind a mark of 1, the definition gives {plane[1]}"
        if t in wrote and compactable(c["partition"], c["ts_ms"]):
            assert trusted, f"tile {t}: written whole in this step, compactable: header mode {mode}, summary flags {flags}"
            assert mark == (plane is not None), f"tile {t}: written whole in this step: mark {mark}, every record fits a plane: {plane is not None}"


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


def decided_tiles(model, P, lo, m, frm, to, has_set):
    """(none, all): how many tiles that lie whole inside records [lo, lo + m) the filter may decide NONE / ALL from header and
    summary alone — those whose summary_definition says so by filter_py.tile_decision.  An upper bound: a zero summary,
    which decides nothing, is always acceptable."""
    import filter_py as F
    none = whole = 0
    for t in range(TILES):
        d = summary_definition(model, t)
        if d is None or t * T < lo or (t + 1) * T > lo + m:
            continue
        decision = F.tile_decision(P, frm, to, has_set, COMPACT, *d, whole=True)
        none, whole = none + (decision == F.NONE), whole + (decision == F.ALL)
    return none, whole


def check_filtered(dev, batch, lo, m, model, window, what):
    """submit_device(which=1) of records [lo, lo + m) behind the filter `window` against the C oracle on the records that
    filter_py.passes lets through; the filter is removed again."""
    import filter_py as F
    h = dev.h
    kind, _, frm, to, parts = window
    cols = model.cut(lo, m)
    ok = F.passes(cols["partition"], cols["ts_ms"], dev.P, frm, to, parts)
    want = _oracle_result(dev.P, {k: cols[k][ok] for k in NAMES})
    what = f"{what} behind the filter {window}"
    h.reset()
    h.set_filter(frm, to, parts)
    try:
        h.submit_device(batch, m, 0, which=1)
        check_finish(dev, want, what)
        info = h.filter_info()
        assert (info["seen"], info["passed"]) == (m, int(ok.sum())), f"{what}: {info}, {int(ok.sum())} of {m} records pass"
        none, whole = decided_tiles(model, dev.P, lo, m, frm, to, parts is not None)
        assert info["tiles_summary_none"] <= none and info["tiles_summary_all"] <= whole, \
            f"{what}: {info}, the summaries' definitions decide at most {none} tiles NONE and {whole} ALL"
    finally:
        h.reset()
        h.set_filter()


def run_readers(dev, b, op, model):
    lo, m = op.view
    check_download(dev, b, model, 0, CAPACITY, "download of the allocation")
    check_download(dev, b, model, lo, m, f"download of the view {op.view}")
    check_layout(model, *read_layout(dev, b), wrote=wrote_whole(op))
    check_scan(dev, b, CAPACITY, model.cols, "scan of the allocation")
    check_scan(dev, dev.view(b, lo), m, model.cut(lo, m), f"scan of the view {op.view}")
    for window in op.windows:
        check_filtered(dev, b, 0, CAPACITY, model, window, "scan of the allocation")
        check_filtered(dev, dev.view(b, lo), lo, m, model, window, f"scan of the view {op.view}")
    check_download(dev, b, model, 0, CAPACITY, "download after the readers")
    check_layout(model, *read_layout(dev, b))


def run_extra_readers(dev, b, op, model):
    """On a handler with analytics, a timeline, the timestamp order, the size percentiles and the segment pass (SEGMENTS): the
    allocation and the view against the Python restatements."""
    import analytics_py as AP
    import segments_py as SG
    import size_quantiles_py as SQ
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
        same(h.size_quantiles()["vector"], SQ.vector(cols, P), f"size percentiles of {what}")
        same(h.segments()["vector"], SG.segments_vector(cols["partition"], cols["key_len"], cols["val_len"], cols["ts_ms"], P, *SEGMENTS),
             f"segments of {what}")
        res, _ = h.finish(allow_bad_partition=True)
        assert int(res.bad_partition_records) == int((~good).sum()), f"bad_partition_records of {what}"


def format_ops(ops):
    return "[\n" + "".join(f"    {op!r},\n" for op in ops) + "]"


def format_ops_pinned(ops):
    """format_ops as it was before the ops had `windows` and `ids`: the form whose digests tests/golden/device_batch_sequences.sha256
    keeps for OLD_SEEDS."""
    import dataclasses
    fields = lambda op: ", ".join(f"{f.name}={getattr(op, f.name)!r}" for f in dataclasses.fields(op) if f.name not in ("windows", "ids"))
    return "[\n" + "".join(f"    {type(op).__name__}({fields(op)}),\n" for op in ops) + "]"


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
        dev.h.reset()
        dev.h.set_filter()
        dev.h.device_batch_free(b)
    return model

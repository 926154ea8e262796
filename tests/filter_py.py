"""The record filter (kta_set_filter, include/kta_hip.h) restated in numpy and plain Python, independently of csrc/kta_filter.h:
which record passes, what a tile's header and summary decide without a record being read, and the columns a filtered
context must behave as if it had been handed.  Test infrastructure only."""
import numpy as np

TILE = 1024
RAW, COMPACT = 0, 1
VALID, TIMED, UNTIMED = 1, 2, 4
PART_NONE = 0xFFFF
I64_MIN, I64_MAX = -2**63, 2**63 - 1
READ, NONE, ALL = 0, 1, 2


def passes(partition, ts_ms, P, from_ms=None, to_ms=None, partitions=None) -> np.ndarray:
    """The mask of the passing records.  from_ms / to_ms None: no bound; partitions None: no set."""
    p = np.asarray(partition, np.int64)
    t = np.asarray(ts_ms, np.int64)
    ok = np.ones(len(p), bool)
    if partitions is not None:
        ok &= np.isin(p, [q for q in partitions if 0 <= q < P])
    if from_ms is not None or to_ms is not None:
        ok &= t != -1
        if from_ms is not None:
            ok &= t >= from_ms
        if to_ms is not None:
            ok &= t < to_ms
    return ok


def record_passes(p, t, P, from_ms=None, to_ms=None, partitions=None) -> bool:
    """One record, Python integers (no numpy overflow anywhere)."""
    if partitions is not None and not (0 <= p < P and p in set(partitions)):
        return False
    if from_ms is None and to_ms is None:
        return True
    if t == -1:
        return False
    return (from_ms is None or t >= from_ms) and (to_ms is None or t < to_ms)


def tile_header_and_summary(p, t):
    """What a producer of whole tiles stores for the records p / t of one tile (include/kta_hip.h, kta_tile_sum):
    -> (mode, ts_base, ts_span, part_max, flags); a tile of fewer than 1024 records has no summary."""
    stamps = [int(x) for x in t if x != -1]
    lo, hi = (min(stamps), max(stamps)) if stamps else (0, 0)
    if not (all(-1 <= int(x) < 65535 for x in p) and hi - lo < 2**31):
        return RAW, 0, 0, 0, 0
    if len(p) != TILE:
        return COMPACT, lo, 0, 0, 0
    part_max = max(PART_NONE if int(x) == -1 else int(x) for x in p)
    flags = VALID | (TIMED if stamps else 0) | (UNTIMED if len(stamps) < len(t) else 0)
    return COMPACT, lo, hi - lo, part_max, flags


def tile_decision(P, from_ms, to_ms, has_set, mode, ts_base, ts_span, part_max, flags, whole) -> int:
    """READ / NONE / ALL from a tile's header and summary alone, as the header words it."""
    if not whole or mode != COMPACT or not flags & VALID or (from_ms is None and to_ms is None):
        return READ
    if not flags & TIMED:
        return NONE                                  # every record is "not available", and a bound is set
    lo, hi = ts_base, ts_base + ts_span
    if (from_ms is not None and hi < from_ms) or (to_ms is not None and lo >= to_ms):
        return NONE
    inside = (from_ms is None or lo >= from_ms) and (to_ms is None or hi < to_ms)
    if inside and not flags & UNTIMED and not has_set and part_max < min(P, PART_NONE):
        return ALL
    return READ


def predict_tiles(cols, P, from_ms=None, to_ms=None, partitions=None, slice_records=None, first=0, n=None):
    """(tiles decided NONE, decided ALL, read, slices) for the batch of records [first, first + n) of a tile-compact
    allocation that cols was written to from its record 0 as whole tiles (kta_batch_from_raw), taken in slices of
    slice_records.  The tiles are the allocation's: a batch or a slice that starts or ends inside one cuts it."""
    total = len(cols["partition"])
    n = total - first if n is None else n
    step = slice_records or max(n, 1)
    out = [0, 0, 0, 0]
    for at in range(first, first + n, step):
        end = min(at + step, first + n)
        out[3] += 1
        for T in range(at // TILE, (end - 1) // TILE + 1):
            lo, hi = max(T * TILE, at), min(T * TILE + TILE, end)
            hdr = tile_header_and_summary(cols["partition"][T * TILE:min(T * TILE + TILE, total)], cols["ts_ms"][T * TILE:min(T * TILE + TILE, total)])
            d = tile_decision(P, from_ms, to_ms, partitions is not None, *hdr, whole=hi - lo == TILE)
            out[{NONE: 0, ALL: 1, READ: 2}[d]] += 1
    return tuple(out)


def take(cols, idx, with_seq=False):
    """The records idx of cols as columns of their own: keys repacked, and `seq` = the original indices (or the original
    seq column's values) when asked for — what an unfiltered context is handed for the comparison."""
    idx = np.asarray(idx, np.int64)
    out = {k: np.ascontiguousarray(cols[k][idx]) for k in ("partition", "key_len", "val_len", "ts_ms")}
    if "key_off" in cols:
        kl = np.maximum(out["key_len"], 0).astype(np.int64)
        off = np.zeros(len(idx), np.int64)
        if len(idx):
            off[1:] = np.cumsum(kl)[:-1]
        blob = np.zeros(max(int(kl.sum()), 1), np.uint8)
        src = cols["key_off"][idx].astype(np.int64)
        for j in np.nonzero(kl)[0]:
            blob[off[j]:off[j] + kl[j]] = cols["key_bytes"][src[j]:src[j] + kl[j]]
        out["key_off"], out["key_bytes"] = off.astype(np.uint32), blob
    if with_seq:
        out["seq"] = (cols["seq"][idx] if "seq" in cols else idx).astype(np.uint64)
    return out


TITLE = ("Record filter: everything above describes the records that passed, and no others "
         "(kta.from, kta.to, kta.partitions; not part of the reference report)\n")


def _table(rows):
    w = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    sep = "+" + "+".join("-" * (x + 2) for x in w) + "+\n"
    out = sep
    for r in rows:
        out += "|" + "|".join(" " + c.ljust(x) + " " for c, x in zip(r, w)) + "|\n" + sep
    return out


def _ranges(partitions, P):
    ps = sorted({p for p in partitions if 0 <= p < P})
    out, i = [], 0
    while i < len(ps):
        j = i
        while j + 1 < len(ps) and ps[j + 1] == ps[j] + 1:
            j += 1
        out.append(str(ps[i]) if i == j else "%d-%d" % (ps[i], ps[j]))
        i = j + 1
    return ",".join(out) or "none"


def section(P, seen, passed, from_ms=None, to_ms=None, partitions=None) -> str:
    """The section kta-analyzer prints after everything else for a filtered run, as include/kta_hip.h words it."""
    def bound(ms):
        if ms is None:
            return "-"
        whole, part = int(ms / 1000) if ms < 0 else ms // 1000, abs(ms) % 1000
        return "%d%s s (%d ms)" % (whole, ".%03d" % part if part else "", ms)

    rows = [["Filter", "Value"], ["From (timestamp >=)", bound(from_ms)], ["To (timestamp <)", bound(to_ms)],
            ["Partitions", "all" if partitions is None else _ranges(partitions, P)], ["Records seen", str(seen)],
            ["Records passed", str(passed)], ["Passed %", "%.2f" % (float(passed) * 100.0 / float(seen)) if seen else "-"]]
    return TITLE + _table(rows) + "=" * 120 + "\n"

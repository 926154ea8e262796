"""The compact,delete what-if (kta_set_compact_delete, include/kta_hip.h) restated in pure Python from the header's wording,
as the sequential loop the definition is — not from the kernels and not from csrc/kta_compact_delete.h: the last writer per
FNV hash slot, then ONE loop over the records that builds kept rows, totals and globals (kept_vector); the what-if both as
the header's formula (whatif_formula) and as a brute force that builds every partition's explicit list of segments with
their survivors, leaves the active segment whole and runs the broker's two deletion loops literally on compacted sizes
(whatif_brute); the identities; and the printed section."""
import numpy as np

import key_sketch_py as KS

ROW = 4            # L, B, T, K  (the segment vector's C, B, T, H + 1)
GLOBALS = 8        # counted, outside [0, P), rows closed, S, M, overhead, 0, 0
WORDS = 10         # records, bytes, compacted records, compacted bytes, kept records, kept bytes, kept tombstones, deleted, rule, clamped
U64 = (1 << 64) - 1


def words(P, M):
    return (P * M + P) * ROW + GLOBALS


def _keys(cols):
    kb = np.asarray(cols["key_bytes"], np.uint8).tobytes()
    kl, ko = np.asarray(cols["key_len"]).tolist(), np.asarray(cols["key_off"]).tolist()
    return [None if l < 0 else KS.fnv1a(kb[o:o + l]) for l, o in zip(kl, ko)]


def classes(cols, seq=None, table_cols=None, table_seq=None):
    """Per record 0 not kept, 1 live, 2 tombstone kept — by hash slot, topic-wide, whatever the partition — and -1 for a
    record the table never saw.  The table is what a first pass over table_cols (None: the very same records) leaves."""
    n = len(cols["partition"])
    seq = list(range(n)) if seq is None else [int(x) for x in seq]
    tc = cols if table_cols is None else table_cols
    ts = seq if table_cols is None else ([int(x) for x in table_seq] if table_seq is not None else list(range(len(tc["partition"]))))
    table = {}
    for key, s, vl in zip(_keys(tc), ts, np.asarray(tc["val_len"]).tolist()):
        if key is not None:
            table[key] = max(table.get(key, 0), ((s + 1) << 1) | (1 if vl >= 0 else 0))
    out = []
    for key, s, vl in zip(_keys(cols), seq, np.asarray(cols["val_len"]).tolist()):
        if key is None:
            out.append(0)
            continue
        val = ((s + 1) << 1) | (1 if vl >= 0 else 0)
        entry = table.get(key, 0)
        out.append(0 if entry > val else -1 if entry < val else 1 if vl >= 0 else 2)
    return out


def empty_vector(P, S, M, overhead):
    v = [0] * words(P, M)
    g = (P * M + P) * ROW
    v[g + 3], v[g + 4], v[g + 5] = S, M, overhead
    return v


def apply_records(v, P, M, part, klen, vlen, cls, trace=None):
    """The one loop: feeds records, in order, into the kept vector v (a list of Python ints, changed in place)."""
    g = (P * M + P) * ROW
    S, overhead = v[g + 3], v[g + 5]
    tot = P * M * ROW
    for p, k, l, c in zip(part, klen, vlen, cls):
        if not 0 <= p < P:
            v[g + 1] += 1
            if trace is not None:
                trace.append(None)
            continue
        v[g + 0] += 1
        z = overhead + max(k, 0) + max(l, 0)
        o = tot + p * ROW
        s = min(v[o + 1] // S, M - 1)
        v[o + 1] = (v[o + 1] + z) & U64
        if c == 1:
            v[o + 0] += 1
            v[o + 3] += z
        elif c == 2:
            v[o + 2] += 1
            v[o + 3] += z
        s_next = min(v[o + 1] // S, M - 1)
        if s_next > s:
            r = (p * M + s) * ROW
            v[r:r + ROW] = v[o:o + ROW]
            v[g + 2] += 1
        if trace is not None:
            trace.append((v[o], v[o + 1], v[o + 2], v[o + 3], int(s_next > s), s if s_next > s else 0))
    return v


def kept_vector(cols, P, S, M, overhead=0, cls=None, into=None):
    """The kept vector u64[(P M + P) 4 + 8] of a replay of cols (numpy uint64).  cls: the records' classes (None: against
    the table a first pass over the same records leaves); into: a vector to continue from."""
    cls = classes(cols) if cls is None else cls
    v = empty_vector(P, S, M, overhead) if into is None else [int(x) for x in into]
    apply_records(v, P, M, np.asarray(cols["partition"]).tolist(), np.asarray(cols["key_len"]).tolist(), np.asarray(cols["val_len"]).tolist(), cls)
    return np.array(v, dtype=np.uint64)


def split(vec, P, M):
    v = np.asarray(vec, dtype=np.uint64)
    assert len(v) == words(P, M)
    return {"rows": v[:P * M * ROW].reshape(P, M, ROW), "totals": v[P * M * ROW:(P * M + P) * ROW].reshape(P, ROW),
            "globals": v[(P * M + P) * ROW:]}


# ---- the identities ----------------------------------------------------------------------------------------------------
def identities_hold(seg, kept, comp, P, M) -> bool:
    """seg: the first pass's segment vector, kept: the replay's kept vector, comp: the replay's compaction vector u64[5 P + 6]"""
    s, k = split(seg, P, M), split(kept, P, M)
    c = [int(x) for x in np.asarray(comp, np.uint64)]
    if c[5 * P + 2] != 0:                                                   # unknown
        return False
    if [int(x) for x in s["globals"][:6]] != [int(x) for x in k["globals"][:6]]:
        return False
    overhead = int(s["globals"][5])
    for p in range(P):
        L, B, T, K = (int(x) for x in k["totals"][p])
        if B != int(s["totals"][p][1]) or L != c[5 * p] or T != c[5 * p + 3]:
            return False
        if K != overhead * (L + T) + c[5 * p + 1] + c[5 * p + 2] + c[5 * p + 4]:
            return False
        prev = (0, 0, 0)
        for r in range(M):
            closed = int(s["rows"][p][r][0]) != 0
            if closed != (int(k["rows"][p][r][1]) != 0) or int(k["rows"][p][r][1]) != int(s["rows"][p][r][1]):
                return False
            if closed:
                cur = (int(k["rows"][p][r][0]), int(k["rows"][p][r][2]), int(k["rows"][p][r][3]))
                if any(a < b for a, b in zip(cur, prev)):
                    return False
                prev = cur
        if any(a < b for a, b in zip((L, T, K), prev)):
            return False
    return True


# ---- the what-if -------------------------------------------------------------------------------------------------------
def whatif_formula(seg, kept, P, M, now_ms, retention_ms, retention_bytes):
    """The header's words, row by row.  Python lists [P + 1][WORDS]."""
    s, k = split(seg, P, M), split(kept, P, M)
    S = int(s["globals"][3])
    out = []
    for p in range(P):
        tot = [int(x) for x in s["totals"][p]]
        closed = [r for r in range(M - 1) if int(s["rows"][p][r][0]) != 0]
        last = [int(x) for x in s["rows"][p][closed[-1]]] if closed else [0] * 4
        klast = [int(x) for x in k["rows"][p][closed[-1]]] if closed else [0] * 4
        a_c, a_b, a_t = tot[0] - last[0], tot[1] - last[1], tot[2] - last[2]
        compacted = klast[3] + a_b
        timing = sizing = walking = True
        deleted = by_time = by_size = 0
        kcut = [0] * 4
        for r in closed:
            row, krow = [int(x) for x in s["rows"][p][r]], [int(x) for x in k["rows"][p][r]]
            timing = timing and retention_ms >= 0 and row[3] != 0 and now_ms >= row[3] - 1 and now_ms - (row[3] - 1) > retention_ms
            sizing = sizing and retention_bytes >= 0 and compacted - krow[3] >= retention_bytes
            by_time += timing
            by_size += sizing
            walking = walking and (timing or sizing)
            if walking:
                deleted += 1
                kcut = krow
        rec2 = klast[0] + klast[2] + a_c
        out.append([tot[0], tot[1], rec2, compacted, rec2 - (kcut[0] + kcut[2]), compacted - kcut[3], klast[2] - kcut[2] + a_t, deleted,
                    0 if deleted == 0 else 1 if by_time >= by_size else 2, 1 if tot[1] // S >= M - 1 else 0])
    return _with_topic_row(out)


def _with_topic_row(out):
    all_row = [sum(r[k] for r in out) for k in range(WORDS)]
    all_row[8] = 0
    for r in out:
        all_row[8] |= r[8]
    return out + [all_row]


def segment_lists(cols, P, S, M, overhead, cls=None):
    """Per partition the explicit log: a list of closed segments oldest first — each with all its records' count, bytes and
    tombstones, its survivors' (live, tombstones kept, bytes) and the largest timestamp the log had seen when it closed —
    and the active segment (whole: it is never cleaned)."""
    cls = classes(cols) if cls is None else cls
    logs = [{"segs": [], "cur": _new_seg(), "bytes": 0, "h": None} for _ in range(P)]
    for p, k, l, t, c in zip(np.asarray(cols["partition"]).tolist(), np.asarray(cols["key_len"]).tolist(), np.asarray(cols["val_len"]).tolist(),
                             np.asarray(cols["ts_ms"]).tolist(), cls):
        if not 0 <= p < P:
            continue
        lg = logs[p]
        z = overhead + max(k, 0) + max(l, 0)
        s = min(lg["bytes"] // S, M - 1)
        lg["bytes"] += z
        cur = lg["cur"]
        cur["records"] += 1
        cur["bytes"] += z
        cur["tombstones"] += 1 if l < 0 else 0
        if c in (1, 2):
            cur["live" if c == 1 else "tombs_kept"] += 1
            cur["kept_bytes"] += z
        if t >= 0:
            lg["h"] = t if lg["h"] is None else max(lg["h"], t)
        if min(lg["bytes"] // S, M - 1) > s:
            cur["largest_ts"] = lg["h"]
            lg["segs"].append(cur)
            lg["cur"] = _new_seg()
    return logs


def _new_seg():
    return {"records": 0, "bytes": 0, "tombstones": 0, "live": 0, "tombs_kept": 0, "kept_bytes": 0, "largest_ts": None}


def whatif_brute(cols, P, S, M, overhead, now_ms, retention_ms, retention_bytes, cls=None):
    """Clean every closed segment (its survivors are what is left of it), leave the active segment whole, then Kafka's
    deleteOldSegments on the compacted sizes: the time loop from the oldest while the segment's largest timestamp is older
    than the cut, then the size loop over what is left — diff = size - retention.bytes, delete the oldest while
    diff - segment.size >= 0.  The active segment is never deleted."""
    out = []
    for lg in segment_lists(cols, P, S, M, overhead, cls):
        segs, active = lg["segs"], lg["cur"]
        cleaned = [{"records": x["live"] + x["tombs_kept"], "bytes": x["kept_bytes"], "tombstones": x["tombs_kept"], "largest_ts": x["largest_ts"]}
                   for x in segs]
        log = list(cleaned)
        n_time = 0
        if retention_ms >= 0:
            while log and log[0]["largest_ts"] is not None and now_ms - log[0]["largest_ts"] > retention_ms:
                log.pop(0)
                n_time += 1
        n_size_after = 0
        if retention_bytes >= 0:
            diff = sum(x["bytes"] for x in log) + active["bytes"] - retention_bytes
            while log and diff - log[0]["bytes"] >= 0:
                diff -= log[0]["bytes"]
                log.pop(0)
                n_size_after += 1
        n_size = 0                                                        # how far the size rule reaches on its own
        if retention_bytes >= 0:
            diff = sum(x["bytes"] for x in cleaned) + active["bytes"] - retention_bytes
            for x in cleaned:
                if diff - x["bytes"] < 0:
                    break
                diff -= x["bytes"]
                n_size += 1
        deleted = n_time + n_size_after
        now_records = sum(x["records"] for x in segs) + active["records"]
        now_bytes = sum(x["bytes"] for x in segs) + active["bytes"]
        comp = lambda key: sum(x[key] for x in cleaned) + active[key]
        kept = lambda key: sum(x[key] for x in log) + active[key]
        out.append([now_records, now_bytes, comp("records"), comp("bytes"), kept("records"), kept("bytes"), kept("tombstones"), deleted,
                    0 if deleted == 0 else (1 if n_time >= n_size else 2), 1 if now_bytes // S >= M - 1 else 0])
    return _with_topic_row(out)


# ---- the printed section -----------------------------------------------------------------------------------------------
def _table(rows):
    w = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    sep = "+" + "+".join("-" * (x + 2) for x in w) + "+\n"
    out = sep
    for r in rows:
        out += "|" + "|".join(" " + c.ljust(x) + " " for c, x in zip(r, w)) + "|\n" + sep
    return out


def title(S, now_ms, retention_ms, retention_bytes):
    off = lambda v: "-" if v < 0 else str(v)
    return ("Compact,delete what-if: cleanup.policy=compact,delete over model log segments of %d bytes per partition (kta.compact_delete), "
            "retention.ms=%s, retention.bytes=%s, now=%s ms; the active segment is not cleaned (not part of the reference report)\n"
            % (S, off(retention_ms), off(retention_bytes), "-" if retention_ms < 0 else str(now_ms)))


MISMATCH = "The replay did not match the first pass. Nothing is reported.\n"


def section(seg, kept, comp, P, M, now_ms, retention_ms=-1, retention_bytes=-1) -> str:
    """The kta.compact_delete section as include/kta_hip.h describes it above kta_render_compact_delete."""
    g = split(seg, P, M)["globals"]
    out = title(int(g[3]), now_ms, retention_ms, retention_bytes)
    if not identities_hold(seg, kept, comp, P, M):
        return out + MISMATCH + "=" * 120 + "\n"
    w = whatif_formula(seg, kept, P, M, now_ms, retention_ms, retention_bytes)
    rows = [["P", "Records", "Bytes", "Compacted records", "Compacted bytes", "Kept records", "Kept bytes", "Tombstones kept", "Reclaimed %", "Rule"]]
    for p in range(P + 1):
        r = w[p]
        rows.append(["All" if p == P else str(p) + ("+" if r[9] else ""), str(r[0]), str(r[1]), str(r[2]), str(r[3]), str(r[4]), str(r[5]), str(r[6]),
                     "%.2f" % ((float(r[1]) - float(r[5])) * 100.0 / float(r[1])) if r[1] else "-", ("-", "time", "size", "time+size")[r[8] & 3]])
    out += _table(rows)
    if w[P][9]:
        out += ("%d partition(s) outgrew the %d rows kept per partition (P ends in +): the last row holds the rest and counts as the active "
                "segment (kta.segments.rows).\n" % (w[P][9], M))
    out += ("Model: a segment ends with the record whose bytes reach its size, so a boundary can differ from the broker's by one record per "
            "segment; segment.ms is not modelled; a record's size is key + value + %d bytes, not bytes on disk (no batch headers, no "
            "compression); the active segment is never cleaned and never deleted, and a prefix without any timestamp is not deleted by time. "
            "Keys are counted by 32-bit hash slot, topic-wide, as \"Alive keys\" is: a key written to several partitions is kept once. The time "
            "rule uses the largest timestamp of all records up to a segment's end, cleaned away or not, so it keeps at least what the broker "
            "keeps. delete.retention.ms, min.compaction.lag.ms and min.cleanable.dirty.ratio are not modelled: every tombstone that survives "
            "is kept, and every closed segment counts as cleaned.\n" % int(g[5]))
    return out + "=" * 120 + "\n"

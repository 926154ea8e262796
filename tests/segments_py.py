"""The retention what-if restated in pure Python from the wording of include/kta_hip.h (above kta_set_segments), as the
sequential loop the definition is — not from the kernels, which reach the same words with prefix sums, and not from
csrc/kta_segments.h.  Every parity test of the segment vector is bit for bit against segments_vector(); the what-if is
held against retention_brute(), which builds the list of segments and runs the broker's two loops literally."""
import numpy as np

ROW = 4            # C, B, T, H + 1
GLOBALS = 8        # counted, outside [0, P), rows closed, S, M, overhead, 0, 0
U64 = (1 << 64) - 1


def words(P, M):
    return (P * M + P) * ROW + GLOBALS


def empty_vector(P, S, M, overhead):
    v = [0] * words(P, M)
    g = (P * M + P) * ROW
    v[g + 3], v[g + 4], v[g + 5] = S, M, overhead
    return v


def apply_records(v, P, part, klen, vlen, ts, trace=None):
    """Feeds records, in order, into the vector v (a list of Python ints, changed in place).  trace: a list that gets, per
    record, None (it does not take part) or (C, B, T, H + 1, closes, row)."""
    g = (P * M_of(v, P) + P) * ROW
    S, M, overhead = v[g + 3], v[g + 4], v[g + 5]
    tot = P * M * ROW
    for p, k, l, t in zip(part, klen, vlen, ts):
        if not 0 <= p < P:
            v[g + 1] += 1
            if trace is not None:
                trace.append(None)
            continue
        v[g + 0] += 1
        z = overhead + max(k, 0) + max(l, 0)
        o = tot + p * ROW
        s = min(v[o + 1] // S, M - 1)
        v[o + 0] += 1
        v[o + 1] = (v[o + 1] + z) & U64
        v[o + 2] += 1 if l < 0 else 0
        if t >= 0:
            v[o + 3] = max(v[o + 3], t + 1)
        s_next = min(v[o + 1] // S, M - 1)
        if s_next > s:
            r = (p * M + s) * ROW
            v[r:r + ROW] = v[o:o + ROW]
            v[g + 2] += 1
        if trace is not None:
            trace.append((v[o], v[o + 1], v[o + 2], v[o + 3], int(s_next > s), s if s_next > s else 0))
    return v


def M_of(v, P):
    """M from the vector's length: len = (P M + P) 4 + 8"""
    return ((len(v) - GLOBALS) // ROW - P) // P


def segments_vector(part, klen, vlen, ts, P, S, M, overhead=0, into=None):
    """The vector u64[(P M + P) 4 + 8] of the records, as numpy uint64.  into: a vector (numpy) to continue from."""
    v = empty_vector(P, S, M, overhead) if into is None else [int(x) for x in into]
    apply_records(v, P, np.asarray(part).tolist(), np.asarray(klen).tolist(), np.asarray(vlen).tolist(), np.asarray(ts).tolist())
    return np.array(v, dtype=np.uint64)


def split(vec, P, M):
    v = np.asarray(vec, dtype=np.uint64)
    assert len(v) == words(P, M)
    return {"rows": v[:P * M * ROW].reshape(P, M, ROW), "totals": v[P * M * ROW:(P * M + P) * ROW].reshape(P, ROW),
            "globals": v[(P * M + P) * ROW:]}


def merge(acc, other, P, M):
    """every word a sum but S, M, overhead, which must agree"""
    a, b = [int(x) for x in acc], [int(x) for x in other]
    g = (P * M + P) * ROW
    if a[g + 3:g + 6] != b[g + 3:g + 6]:
        raise ValueError("segment vectors of different configurations")
    out = [(x + y) & U64 for x, y in zip(a, b)]
    out[g + 3:g + 6] = a[g + 3:g + 6]
    return np.array(out, dtype=np.uint64)


# ---- the what-if ------------------------------------------------------------------------------------------------------
RET_WORDS = 10   # segments, records, bytes, tombstones, records kept, bytes kept, tombstones kept, segments deleted, rule, clamped


def segment_list(vec, P, M, p):
    """The partition's closed, non-empty segments oldest first as dicts of their OWN records, bytes, tombstones and the
    largest timestamp the log had seen when the segment closed (None: none yet), then the active segment."""
    s = split(vec, P, M)
    segs, prev = [], (0, 0, 0)
    for k in range(M - 1):
        c, b, t, h1 = (int(x) for x in s["rows"][p][k])
        if c == 0:
            continue
        segs.append({"records": c - prev[0], "bytes": b - prev[1], "tombstones": t - prev[2], "largest_ts": h1 - 1 if h1 else None})
        prev = (c, b, t)
    c, b, t, _ = (int(x) for x in s["totals"][p])
    active = {"records": c - prev[0], "bytes": b - prev[1], "tombstones": t - prev[2]}
    return segs, active


def retention_brute(vec, P, M, now_ms, retention_ms, retention_bytes):
    """Kafka's deleteOldSegments over the model's segments: first the time loop — delete from the oldest while the segment's
    largest timestamp is older than the cut, stop at the first that is not —, then the size loop over what is left —
    diff = size - retention.bytes; delete the oldest while diff - segment.size >= 0.  The active segment is never deleted.
    Returns int64-free Python lists [P + 1][RET_WORDS]."""
    S = int(split(vec, P, M)["globals"][3])
    out = []
    for p in range(P):
        segs, active = segment_list(vec, P, M, p)
        log = list(segs)
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
        # how far the size rule reaches on its own, for the "which rule" word
        n_size = 0
        if retention_bytes >= 0:
            diff = sum(x["bytes"] for x in segs) + active["bytes"] - retention_bytes
            for x in segs:
                if diff - x["bytes"] < 0:
                    break
                diff -= x["bytes"]
                n_size += 1
        deleted = n_time + n_size_after
        tot = lambda key: sum(x[key] for x in segs) + active[key]
        kept = lambda key: sum(x[key] for x in log) + active[key]
        total_bytes = tot("bytes")
        out.append([len(segs) + (1 if active["records"] else 0), tot("records"), total_bytes, tot("tombstones"),
                    kept("records"), kept("bytes"), kept("tombstones"), deleted,
                    0 if deleted == 0 else (1 if n_time >= n_size else 2), 1 if total_bytes // S >= M - 1 else 0])
    all_row = [sum(r[k] for r in out) for k in range(RET_WORDS)]
    all_row[8] = 0
    for r in out:
        all_row[8] |= r[8]
    out.append(all_row)
    return out


# ---- the printed section ----------------------------------------------------------------------------------------------
def _table(rows):
    w = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    sep = "+" + "+".join("-" * (x + 2) for x in w) + "+\n"
    out = sep
    for r in rows:
        out += "|" + "|".join(" " + c.ljust(x) + " " for c, x in zip(r, w)) + "|\n" + sep
    return out


def section(vec, P, M, now_ms, retention_ms=-1, retention_bytes=-1) -> str:
    """The kta.segments section as include/kta_hip.h describes it above kta_render_retention."""
    g = split(vec, P, M)["globals"]
    w = retention_brute(vec, P, M, now_ms, retention_ms, retention_bytes)
    policy = retention_ms >= 0 or retention_bytes >= 0
    off = lambda v: "-" if v < 0 else str(v)
    out = "Retention what-if: model log segments of %d bytes per partition (kta.segments), " % int(g[3])
    out += ("retention.ms=%s, retention.bytes=%s, now=%d ms" % (off(retention_ms), off(retention_bytes), now_ms)) if policy \
        else "no retention policy given"
    out += " (not part of the reference report)\n"
    rows = [["P", "Segments", "Records", "Bytes"] + (["Records kept", "Bytes kept", "Reclaimed %", "Rule"] if policy else [])]
    for p in range(P + 1):
        r = w[p]
        row = ["All" if p == P else str(p), str(r[0]) + ("+" if p < P and r[9] else ""), str(r[1]), str(r[2])]
        if policy:
            row += [str(r[4]), str(r[5]), "%.2f" % (float(r[2] - r[5]) * 100.0 / float(r[2])) if r[2] else "-",
                    ("-", "time", "size", "time+size")[r[8] & 3]]
        rows.append(row)
    out += _table(rows)
    if w[P][9]:
        out += ("%d partition(s) outgrew the %d rows kept per partition (Segments ends in +): the last row holds the rest and counts as "
                "the active segment (kta.segments.rows).\n" % (w[P][9], M))
    out += ("Model: a segment ends with the record whose bytes reach its size, so a boundary can differ from the broker's by one record "
            "per segment; segment.ms is not modelled; a record's size is key + value + %d bytes, not bytes on disk (no batch headers, no "
            "compression); the active segment is never deleted, and a prefix without any timestamp is not deleted by time.\n" % int(g[5]))
    return out + "=" * 120 + "\n"

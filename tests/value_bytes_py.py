"""The value-byte section (KTA_FLAG_VALUE_BYTES) restated in Python (test infrastructure), from the section's definition and
the Kafka message format v2 — not from csrc/kta_value_bytes.h: the vector u64[264 P], what one record adds to it (np.bincount
of its value, and the value compared with itself shifted by one), the identities between its words, the read-off (entropy,
shares, class) and the section kta-analyzer prints.  It walks the encoder's own record bytes as payload_py.py does; a case is a
list of (blob, partition, raw, failed) as there."""
import math

import numpy as np

import payload_py as R

PW, BINS = 264, 256
RECORDS, VALUES, BYTES, REPEATS = 256, 257, 258, 259
CLASSES = ("none", "text", "dense", "binary")
PRINTABLE = [b for b in range(256) if 0x20 <= b <= 0x7E or b in (9, 10, 13)]


def words(P):
    return PW * P


def add_value(w, value):
    """what one counted record adds to its partition's 264 words; value: bytes, or None for a null value"""
    w[RECORDS] += 1
    if not value:
        return
    a = np.frombuffer(value, np.uint8)
    w[VALUES] += 1
    w[BYTES] += a.size
    w[:BINS] += np.bincount(a, minlength=BINS).astype(np.uint64)
    w[REPEATS] += int(np.count_nonzero(a[1:] == a[:-1]))


def restate(items, P, flt=None, vec=None):
    """The vector of a case.  flt: None or (from_ms | None, to_ms | None, set of partitions | None)."""
    vec = np.zeros(words(P), np.uint64) if vec is None else vec
    for blob, partition, raw, failed in items:
        if not 0 <= partition < P:
            continue
        w = vec[PW * partition:PW * partition + PW]
        for b in R.batches_of(blob):
            if b["magic"] != 2 or b["control"] or b["codec"] > 4 or b["count"] <= 0 or b["pos"] in failed:
                continue
            recs = raw[b["pos"]] if b["codec"] else b["recs"]
            for ts_delta, value, _hpos, _rec_end, _key_len in R.records_of(recs, b["count"]):
                ts = b["max_ts"] if b["attributes"] & 8 else b["base_ts"] + ts_delta
                if R.passes(flt, partition, ts):
                    add_value(w, value)
    return vec


def identities(v, P, payload=None, counters=None):
    """[(name, holds)].  payload: the payload vector of the same run; counters: the counter vector u64[7 P + 8] of the same
    unfiltered run without failed batches."""
    w = np.asarray(v, np.uint64).reshape(P, PW).astype(object)
    out = [("bins sum to bytes", all(sum(w[p, :BINS]) == w[p, BYTES] for p in range(P))),
           ("repeats <= bytes - values", all(w[p, REPEATS] <= w[p, BYTES] - w[p, VALUES] for p in range(P))),
           ("values <= records", all(w[p, VALUES] <= w[p, RECORDS] for p in range(P))),
           ("spare words are zero", not w[:, 260:].any())]
    if payload is not None:
        l = np.asarray(payload, np.uint64)[:R.PW * P].reshape(P, R.PW).astype(object)
        out.append(("records == the payload's", all(w[p, RECORDS] == l[p, R.RECORDS] for p in range(P))))
        out.append(("bytes == the payload's class bytes", all(w[p, BYTES] == sum(l[p, R.CLASS_BYTES:R.CLASS_BYTES + 5]) for p in range(P))))
        out.append(("values == framed + json + other", all(w[p, VALUES] == sum(l[p, R.CLASS + R.FRAMED:R.CLASS + R.OTHER + 1]) for p in range(P))))
    if counters is not None:
        c = np.asarray(counters, np.uint64)[:7 * P].reshape(P, 7).astype(object)
        out.append(("records == total_messages", all(w[p, RECORDS] == c[p, 0] for p in range(P))))
    return out


def summary(w):
    """The read-off of 264 words (one partition's, or the topic's sum), in exact arithmetic but for H0: math.fsum over the
    non-zero bins, each term in double."""
    w = [int(x) for x in np.asarray(w, np.uint64)]
    bins = w[:BINS]
    B = sum(bins)
    h = -math.fsum((c / B) * math.log2(c / B) for c in bins if c) if B else 0.0
    h = max(h, 0.0)
    top = max(range(BINS), key=lambda b: (bins[b], -b)) if B else 0
    printable = sum(bins[b] for b in PRINTABLE)
    cls = "none" if B == 0 else "text" if 20 * printable >= 19 * B else "dense" if B >= 65536 and h >= 7.5 else "binary"
    return {"records": w[RECORDS], "values": w[VALUES], "bytes": w[BYTES], "repeats": w[REPEATS], "distinct": sum(1 for c in bins if c),
            "entropy_bits": h, "floor_bytes": math.ceil(B * h / 8.0), "printable": printable, "zero": bins[0], "high": sum(bins[128:]),
            "top_byte": top, "top_count": bins[top] if B else 0, "class": cls}


def topic(v, P):
    return np.asarray(v, np.uint64).reshape(P, PW).sum(axis=0, dtype=np.uint64)


def _table(rows):
    """the report's pretty table: cells padded to the column's width, a rule behind every row"""
    widths = [max(len(r[c]) for r in rows) for c in range(len(rows[0]))]
    rule = "+" + "+".join("-" * (w + 2) for w in widths) + "+\n"
    out = rule
    for r in rows:
        out += "|" + "|".join(" " + cell.ljust(w) + " " for cell, w in zip(r, widths)) + "|\n" + rule
    return out


def percent(num, den):
    return "n/a" if den == 0 else "%.2f" % (num * 100.0 / den)


def decimals_clear_of_a_tie(v, P, margin=1e-6):
    """whether every figure the section prints with two decimals lies at least `margin` away from a rounding tie (x.xx5)"""
    def clear(x):
        frac = (x * 100.0) % 1.0
        return abs(frac - 0.5) > margin * 100.0
    rows = [summary(np.asarray(v, np.uint64).reshape(P, PW)[p]) for p in range(P)] + [summary(topic(v, P))]
    for s in rows:
        if not s["bytes"]:
            continue
        figures = [s["entropy_bits"]] + [s[k] * 100.0 / s["bytes"] for k in ("floor_bytes", "printable", "zero", "high", "repeats", "top_count")]
        if not all(clear(x) for x in figures):
            return False
    return True


def section_rows(v, P):
    rows = [["P", "Records", "Values", "Value bytes", "H0 bits/byte", "Order-0 floor %", "Printable %", "Zero %", "High-bit %", "Repeat %", "Distinct",
             "Top byte", "Class"]]
    parts = np.asarray(v, np.uint64).reshape(P, PW)
    for name, w in [(str(p), parts[p]) for p in range(P)] + [("Topic", topic(v, P))]:
        s = summary(w)
        B = s["bytes"]
        rows.append([name, str(s["records"]), str(s["values"]), str(B), "%.2f" % s["entropy_bits"] if B else "n/a", percent(s["floor_bytes"], B),
                     percent(s["printable"], B), percent(s["zero"], B), percent(s["high"], B), percent(s["repeats"], B), str(s["distinct"]),
                     "0x%02X (%s%%)" % (s["top_byte"], percent(s["top_count"], B)) if B else "n/a", s["class"]])
    return rows


def section(v, P) -> str:
    """The kta.value_bytes=1 section."""
    out = "Value bytes: a byte histogram of the record values (kta.value_bytes=1; not part of the reference report)\n"
    out += _table(section_rows(v, P))
    out += ("Class is a heuristic: text = at least 95% printable bytes; dense = at least 65536 bytes and H0 >= 7.5 (compressed, encrypted or random "
            "already); binary otherwise.\n")
    out += ("H0 is the order-0 entropy of the value bytes: it bounds an entropy coder alone.  LZ matching, which is most of what gzip, LZ4 or zstd win "
            "on JSON, is not in it.\n")
    return out + "=" * 120 + "\n"

"""The payload section (KTA_FLAG_PAYLOAD) restated in Python (test infrastructure), from the section's definition and the
Kafka message format v2 — not from csrc/kta_payload.h: the vector u64[24 P + 16 + 2 * 1024 * 34], what one record adds to it,
the identities between its words and the peeling read-off of the schema ids.

A case is a list of (blob, partition, raw, failed): `raw` maps the byte position of a COMPRESSED batch in the blob to the
record bytes the encoder compressed (the restatement inflates nothing), `failed` is the set of byte positions of batches that
the device must fail (a forged count, a stream that does not inflate, a bad CRC under check.crcs): they add nothing."""
import struct

import numpy as np

PW, HIST, ROWS, CELLS, CW = 24, 16, 2, 1024, 34
RECORDS, CLASS, CLASS_BYTES = 0, 1, 6
WITH, HEADERS, HKEY, HVAL, HNULL, BAD, WIRE = 11, 12, 13, 14, 15, 16, 17
NULL, EMPTY, FRAMED, JSON, OTHER = range(5)
M64 = (1 << 64) - 1


def words(P):
    return PW * P + HIST + ROWS * CELLS * CW


def fmix32(x):
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    return x ^ (x >> 16)


def cell(row, x):
    return (x if row == 0 else fmix32(x)) & (CELLS - 1)


def cell_at(P, row, c):
    return PW * P + HIST + (row * CELLS + c) * CW


def unvarint(buf, pos, end):
    """A zig-zag varint of at most ten bytes inside buf[pos:end]: (value, position behind it) or None."""
    v = 0
    for i in range(10):
        if pos >= end:
            return None
        b = buf[pos]
        pos += 1
        v |= (b & 0x7F) << min(7 * i, 63)
        v &= M64
        if not b & 0x80:
            return (v >> 1) ^ -(v & 1), pos
    return None


def walk_headers(buf, pos, end):
    """(count, key bytes, value bytes, null values) of the header section buf[pos:end], or None when it is bad."""
    got = unvarint(buf, pos, end)
    if got is None or got[0] < 0:
        return None
    count, pos = got
    keyb = valb = nulls = 0
    for _ in range(count):
        got = unvarint(buf, pos, end)
        if got is None or got[0] < 0 or got[0] > end - got[1]:
            return None
        keyb += got[0]
        pos = got[1] + got[0]
        got = unvarint(buf, pos, end)
        if got is None or got[0] < -1:
            return None
        vl, pos = got
        if vl < 0:
            nulls += 1
            continue
        if vl > end - pos:
            return None
        valb += vl
        pos += vl
    return (count, keyb, valb, nulls) if pos == end else None


def classify(value):
    if value is None:
        return NULL
    if len(value) == 0:
        return EMPTY
    if len(value) >= 5 and value[0] == 0:
        return FRAMED
    if value[0] in b"{[":
        return JSON
    return OTHER


def records_of(recs, count):
    """The records of a record section as the decode walks them: (ts_delta, value | None, header position, record end, key
    length); the walk ends in front of the first record whose framing fails."""
    pos, end = 0, len(recs)
    for _ in range(count):
        got = unvarint(recs, pos, end)
        if got is None or got[0] < 0 or got[0] > end - got[1]:
            return
        rec_end = got[1] + got[0]
        pos = got[1] + 1                                   # the attributes byte
        if pos > rec_end:
            return
        fields = []
        for _f in range(3):                                # timestampDelta, offsetDelta, keyLength
            got = unvarint(recs, pos, rec_end)
            if got is None:
                return
            fields.append(got[0])
            pos = got[1]
        kl = fields[2]
        if kl < -1 or (kl > 0 and kl > rec_end - pos):
            return
        pos += max(kl, 0)
        got = unvarint(recs, pos, rec_end)
        if got is None:
            return
        vl, pos = got
        if vl < -1 or (vl > 0 and vl > rec_end - pos):
            return
        yield fields[0], (None if vl < 0 else bytes(recs[pos:pos + vl])), pos + max(vl, 0), rec_end, kl
        pos = rec_end


def add_record(vec, P, partition, value, recs, hpos, rec_end):
    w = vec[PW * partition:PW * partition + PW]
    cls = classify(value)
    vb = len(value) if value else 0
    w[RECORDS] += 1
    w[CLASS + cls] += 1
    w[CLASS_BYTES + cls] += vb
    if cls == FRAMED:
        x = struct.unpack(">I", value[1:5])[0]
        for row in range(ROWS):
            c = vec[cell_at(P, row, cell(row, x)):][:CW]
            c[0] += 1
            c[1] += vb
            for b in range(32):
                c[2 + b] += (x >> b) & 1
    h = walk_headers(recs, hpos, rec_end)
    if h is None:
        w[BAD] += 1
        return
    w[WITH] += h[0] != 0
    w[HEADERS] += h[0]
    w[HKEY] += h[1]
    w[HVAL] += h[2]
    w[HNULL] += h[3]
    w[WIRE] += rec_end - hpos
    vec[PW * P + min(h[0], HIST - 1)] += 1


def batches_of(blob):
    """The v2 batches of a blob, by its own walk over the batch headers."""
    out, pos = [], 0
    while pos + 61 <= len(blob):
        base_offset, length = struct.unpack_from(">qi", blob, pos)
        if length < 49 or pos + 12 + length > len(blob):
            break
        magic = blob[pos + 16]
        attributes, lod, base_ts, max_ts, pid, pepoch, seq, count = struct.unpack_from(">hiqqqhii", blob, pos + 21)
        out.append({"pos": pos, "magic": magic, "attributes": attributes, "base_ts": base_ts, "max_ts": max_ts, "count": count,
                    "codec": attributes & 7, "control": bool(attributes & 0x20), "recs": bytes(blob[pos + 61:pos + 12 + length])})
        pos += 12 + length
    return out


def passes(flt, partition, ts):
    if flt is None:
        return True
    lo, hi, parts = flt
    if parts is not None and partition not in parts:
        return False
    if lo is None and hi is None:
        return True
    return ts != -1 and (lo is None or ts >= lo) and (hi is None or ts < hi)


def restate(items, P, flt=None, vec=None, sizes=None):
    """The vector of a case (see the module's text).  flt: None or (from_ms | None, to_ms | None, set of partitions | None).
    sizes: a counter vector u64[7 P + 8] that receives the counted records' total, tombstones and key and value size sums."""
    vec = np.zeros(words(P), np.uint64) if vec is None else vec
    for blob, partition, raw, failed in items:
        if not 0 <= partition < P:
            continue
        for b in batches_of(blob):
            if b["magic"] != 2 or b["control"] or b["codec"] > 4 or b["count"] <= 0 or b["pos"] in failed:
                continue
            recs = raw[b["pos"]] if b["codec"] else b["recs"]
            for ts_delta, value, hpos, rec_end, key_len in records_of(recs, b["count"]):
                ts = b["max_ts"] if b["attributes"] & 8 else b["base_ts"] + ts_delta
                if passes(flt, partition, ts):
                    add_record(vec, P, partition, value, recs, hpos, rec_end)
                    if sizes is not None:
                        sizes[7 * partition + 0] += 1
                        sizes[7 * partition + 1] += value is None
                        sizes[7 * partition + 5] += max(key_len, 0)
                        sizes[7 * partition + 6] += len(value) if value else 0
    return vec


def identities(v, P, counters=None):
    """[(name, holds)].  counters: the counter vector u64[7 P + 8] of the same unfiltered run without failed batches."""
    v = np.asarray(v, np.uint64)
    w = v[:PW * P].reshape(P, PW).astype(object)
    hist = v[PW * P:PW * P + HIST].astype(object)
    table = v[PW * P + HIST:].reshape(ROWS, CELLS, CW).astype(object)
    out = [("classes sum to records", all(sum(w[p, CLASS:CLASS + 5]) == w[p, RECORDS] for p in range(P))),
           ("null and empty have no bytes", all(w[p, CLASS_BYTES + NULL] == 0 and w[p, CLASS_BYTES + EMPTY] == 0 for p in range(P))),
           ("spare words are zero", not w[:, 18:].any()),
           ("histogram sums to records - bad", sum(hist) == sum(w[:, RECORDS]) - sum(w[:, BAD])),
           ("bin 0 is records - with - bad", hist[0] == sum(w[:, RECORDS]) - sum(w[:, WITH]) - sum(w[:, BAD]))]
    for r in range(ROWS):
        out.append((f"row {r} T and B", table[r, :, 0].sum() == sum(w[:, CLASS + FRAMED]) and table[r, :, 1].sum() == sum(w[:, CLASS_BYTES + FRAMED])))
    out.append(("bit counters <= T", bool((table[:, :, 2:] <= table[:, :, :1]).all())))
    if counters is not None:
        c = np.asarray(counters, np.uint64)[:7 * P].reshape(P, 7).astype(object)
        out.append(("records == total_messages", all(w[p, RECORDS] == c[p, 0] for p in range(P))))
        out.append(("null == tombstones", all(w[p, CLASS + NULL] == c[p, 1] for p in range(P))))
    return out


def schema_ids(v, P):
    """([(id, records, bytes)] sorted by records (most first), bytes, id; unresolved records; unresolved bytes): pure cells
    give their ids, recovered ids are peeled from the other row, until nothing changes."""
    t = [[[int(x) for x in np.asarray(v[cell_at(P, r, c):cell_at(P, r, c) + CW])] for c in range(CELLS)] for r in range(ROWS)]
    found, changed = [], True
    while changed:
        changed = False
        for r in range(ROWS):
            for c in range(CELLS):
                cl = t[r][c]
                T = cl[0]
                if T == 0 or any(x not in (0, T) for x in cl[2:]):
                    continue
                x = sum(1 << b for b in range(32) if cl[2 + b])
                if cell(r, x) != c:
                    continue
                other = t[1 - r][cell(1 - r, x)]
                if any(o < m for o, m in zip(other, cl)):
                    continue
                found.append((x, T, cl[1]))
                for k in range(CW):
                    other[k] -= cl[k]
                    cl[k] = 0
                changed = True
    found.sort(key=lambda e: (-e[1], -e[2], e[0]))
    return found, sum(cl[0] for cl in t[0]), sum(cl[1] for cl in t[0])

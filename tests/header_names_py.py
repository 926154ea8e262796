"""The header-name section (KTA_FLAG_HEADER_NAMES) restated in Python (test infrastructure), from the section's definition and
the Kafka message format v2 — not from csrc/kta_header_names.h: the vector u64[8 + 2 * 1024 * 36], what one header occurrence
adds to it, the identities, the peeling read-off of the names and the printed section.  Which records count is payload_py's
(the payload section's rule: batches_of, records_of, passes); the hash, the cell mapping and the peel are this file's own.

A case is a list of (blob, partition, raw, failed), as payload_py takes it."""
import numpy as np

import payload_py as R

GLOBALS, ROWS, CELLS, CW = 8, 2, 1024, 36
WORDS = GLOBALS + ROWS * CELLS * CW
OCC, NAMEB, VALB, NULLS, WITH, LOOKED = range(6)
T, L, V, Z, BITS = 0, 1, 2, 3, 4
KEPT = 48                                      # the bytes of a name that the name table keeps


def fnv1a(name: bytes) -> int:
    """The reference's FNV-32 variant (offset basis and multiplier 0x811c9dc5), as -c hashes keys."""
    h = 0x811C9DC5
    for b in name:
        h = ((h ^ b) * 0x811C9DC5) & 0xFFFFFFFF
    return h


def cell(row, h):
    return (h if row == 0 else R.fmix32(h)) & (CELLS - 1)


def cell_at(row, c):
    return GLOBALS + (row * CELLS + c) * CW


def headers_of(buf, pos, end):
    """[(name, value | None)] of the header section buf[pos:end], or None when it is bad."""
    got = R.unvarint(buf, pos, end)
    if got is None or got[0] < 0:
        return None
    count, pos = got
    out = []
    for _ in range(count):
        got = R.unvarint(buf, pos, end)
        if got is None or got[0] < 0 or got[0] > end - got[1]:
            return None
        name = bytes(buf[got[1]:got[1] + got[0]])
        pos = got[1] + got[0]
        got = R.unvarint(buf, pos, end)
        if got is None or got[0] < -1:
            return None
        vl, pos = got
        if vl < 0:
            out.append((name, None))
            continue
        if vl > end - pos:
            return None
        out.append((name, bytes(buf[pos:pos + vl])))
        pos += vl
    return out if pos == end else None


def add_occurrence(vec, name, value, seen=None):
    h = fnv1a(name)
    vb = len(value) if value else 0
    vec[OCC] += 1
    vec[NAMEB] += len(name)
    vec[VALB] += vb
    vec[NULLS] += value is None
    for row in range(ROWS):
        c = vec[cell_at(row, cell(row, h)):][:CW]
        c[T] += 1
        c[L] += len(name)
        c[V] += vb
        c[Z] += value is None
        for b in range(32):
            c[BITS + b] += (h >> b) & 1
    if seen is not None:
        seen.setdefault(h, set()).add(name)


def restate(items, P, flt=None, vec=None, seen=None):
    """The vector of a case.  flt: as payload_py.restate's.  seen: a dict that receives {hash: the set of names of that hash}."""
    vec = np.zeros(WORDS, np.uint64) if vec is None else vec
    for blob, partition, raw, failed in items:
        if not 0 <= partition < P:
            continue
        for b in R.batches_of(blob):
            if b["magic"] != 2 or b["control"] or b["codec"] > 4 or b["count"] <= 0 or b["pos"] in failed:
                continue
            recs = raw[b["pos"]] if b["codec"] else b["recs"]
            for ts_delta, _value, hpos, rec_end, _key_len in R.records_of(recs, b["count"]):
                ts = b["max_ts"] if b["attributes"] & 8 else b["base_ts"] + ts_delta
                if not R.passes(flt, partition, ts):
                    continue
                hs = headers_of(recs, hpos, rec_end)
                if hs is None:
                    continue
                vec[LOOKED] += 1
                vec[WITH] += len(hs) != 0
                for name, value in hs:
                    add_occurrence(vec, name, value, seen)
    return vec


def identities(v, payload=None, P=0):
    """[(name, holds)].  payload: the payload vector of the same run (P partitions)."""
    v = np.asarray(v, np.uint64)
    g = [int(x) for x in v[:GLOBALS]]
    table = v[GLOBALS:].reshape(ROWS, CELLS, CW).astype(object)
    out = [("spare words are zero", g[6] == 0 and g[7] == 0)]
    for r in range(ROWS):
        out.append((f"row {r} sums", [table[r, :, k].sum() for k in (T, L, V, Z)] == g[:4]))
    out.append(("bit counters <= T", bool((table[:, :, BITS:] <= table[:, :, :1]).all())))
    if payload is not None:
        w = np.asarray(payload, np.uint64)[:R.PW * P].reshape(P, R.PW).astype(object)
        out.append(("occurrences == headers", g[OCC] == w[:, R.HEADERS].sum()))
        out.append(("name bytes == header_key_bytes", g[NAMEB] == w[:, R.HKEY].sum()))
        out.append(("value bytes == header_value_bytes", g[VALB] == w[:, R.HVAL].sum()))
        out.append(("null values == header_null_values", g[NULLS] == w[:, R.HNULL].sum()))
        out.append(("with headers == with_headers", g[WITH] == w[:, R.WITH].sum()))
        out.append(("looked == records - bad_headers", g[LOOKED] == w[:, R.RECORDS].sum() - w[:, R.BAD].sum()))
    return out


def list_names(v):
    """([(hash, occurrences, name length, value bytes, null values)] sorted by occurrences (most first), value bytes, hash;
    unresolved occurrences; unresolved value bytes).  A cell is pure when T > 0, every bit counter is 0 or T, L is a multiple of
    T and the hash so spelled maps to this cell in this row; a recovered hash is taken out of both rows; until nothing changes."""
    t = [[[int(x) for x in np.asarray(v[cell_at(r, c):cell_at(r, c) + CW])] for c in range(CELLS)] for r in range(ROWS)]
    found, changed = [], True
    while changed:
        changed = False
        for r in range(ROWS):
            for c in range(CELLS):
                cl = t[r][c]
                n = cl[T]
                if n == 0 or cl[L] % n or any(x not in (0, n) for x in cl[BITS:]):
                    continue
                h = sum(1 << b for b in range(32) if cl[BITS + b])
                if cell(r, h) != c:
                    continue
                other = t[1 - r][cell(1 - r, h)]
                if any(o < m for o, m in zip(other, cl)):
                    continue
                found.append((h, n, cl[L] // n, cl[V], cl[Z]))
                for k in range(CW):
                    other[k] -= cl[k]
                    cl[k] = 0
                changed = True
    found.sort(key=lambda e: (-e[1], -e[3], e[0]))
    return found, sum(cl[T] for cl in t[0]), sum(cl[V] for cl in t[0])


def name_text(name: bytes, name_len=None) -> str:
    """A name as the section prints it: printable ASCII but the backslash as is, \\xNN else, ... behind 48 bytes."""
    n = len(name) if name_len is None else name_len
    t = "".join(chr(b) if 0x20 <= b < 0x7F and b != 0x5C else "\\x%02X" % b for b in name[:KEPT])
    return t + ("..." if n > KEPT else "")


def _table(rows):
    w = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    sep = "+" + "+".join("-" * (x + 2) for x in w) + "+\n"
    out = sep
    for r in rows:
        out += "|" + "|".join(" " + c.ljust(x) + " " for c, x in zip(r, w)) + "|\n" + sep
    return out


def _ratio(num, den, scale=1.0):
    return "n/a" if den == 0 else "%.2f" % (num * scale / den)


def section(v, names_by_hash=None, max_names=256) -> str:
    """The kta.headers=1 section; names_by_hash: {hash: name bytes} of the exemplars at hand (a hash without one prints #hash)."""
    g = [int(x) for x in v[:GLOBALS]]
    found, uo, uv = list_names(v)
    out = "Header names: a census of the record headers (kta.headers=1; not part of the reference report)\n"
    out += "%d headers in %d of %d records looked at: %d name bytes, %d value bytes, %d null values, %d names listed\n" % (
        g[OCC], g[WITH], g[LOOKED], g[NAMEB], g[VALB], g[NULLS], len(found))
    if found:
        rows = [["#", "Name", "Hash", "Occurrences", "per record with headers", "Name bytes", "Value bytes", "Mean value", "Null values",
                 "Share of header bytes"]]
        for k, (h, n, nl, vb, z) in enumerate(found[:max_names]):
            name = (names_by_hash or {}).get(h)
            rows.append([str(k + 1), "#%08x" % h if name is None else name_text(name, nl), "%08x" % h, str(n), _ratio(n, g[WITH]), str(n * nl), str(vb),
                         _ratio(vb, n - z), str(z), _ratio(n * nl + vb, g[NAMEB] + g[VALB], 100.0)])
        out += _table(rows)
        if len(found) > max_names:
            out += "... and %d more\n" % (len(found) - max_names)
    if uo:
        out += "Unresolved: %d occurrences, %d value bytes in table cells that hold several names\n" % (uo, uv)
    return out + "=" * 120 + "\n"


def table_names(table) -> dict:
    """{hash: name bytes (48 at most)} of the published slots of a structured name table."""
    out = {}
    for e in table:
        if e["state"] == 2:
            out.setdefault(int(e["hash"]), bytes(e["bytes"][:min(int(e["name_len"]), KEPT)]))
    return out


def check_table(table, seen):
    """Every published slot holds the first 48 bytes of a name that occurred, whose hash is the slot's and maps to the slot's cell."""
    for i, e in enumerate(table):
        if e["state"] != 2:
            assert not e["state"] and not e["hash"] and not e["name_len"] and not e["bytes"].any(), i
            continue
        h, n = int(e["hash"]), int(e["name_len"])
        assert cell(i // CELLS, h) == i % CELLS, (i, h)
        stored = bytes(e["bytes"][:min(n, KEPT)])
        assert any(len(name) == n and name[:KEPT] == stored for name in seen.get(h, ())), (i, h, n, stored)
        assert not e["bytes"][min(n, KEPT):].any(), i


def check_missing(table, names):
    """A name that occurred has its exemplar in one of its two slots, or both slots hold other names: the first writer won."""
    have = table_names(table)
    for name in names:
        h = fnv1a(name)
        if h not in have:
            assert all(table[r * CELLS + cell(r, h)]["state"] == 2 and table[r * CELLS + cell(r, h)]["hash"] != h for r in range(ROWS)), name

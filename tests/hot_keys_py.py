"""Independent numpy / Python restatement of the hot-key sketch (include/kta_hip.h, KTA_FLAG_HOT_KEYS): the vector from
columns, from hashes and from (hash, count) pairs, the readout with its bounds, the merge and the kta.hot_keys section.
Shares no code with the library (the FNV and fmix32 restatements are those of tests/key_sketch_py.py)."""
import numpy as np

from key_sketch_py import fmix32, fnv1a, fnv_columns  # noqa: F401  (fnv1a: for the tests)

ROWS, CELLS, WORDS = 2, 1024, 23
BITS = WORDS - 1
FLOOR = 512                      # a candidate is reported when upper * 512 >= keyed
U32 = 0xFFFFFFFF


def title(k):
    return ("Hot keys, at most %d (sums of bit counters over the key hashes, 2 rows of 1024 cells: keys from 1/512 of the "
            "keyed records; kta.hot_keys=%d; not part of the reference report)\n" % (k, k))


def fmix32_inverse(x: int) -> int:
    """h with fmix32(h) == x: the two multipliers inverted mod 2^32 (pow), the shifts-and-xors undone."""
    inv1, inv2 = pow(0x85EBCA6B, -1, 1 << 32), pow(0xC2B2AE35, -1, 1 << 32)
    x ^= x >> 16
    x = (x * inv2) & U32
    x ^= (x >> 13) ^ (x >> 26)
    x = (x * inv1) & U32
    x ^= x >> 16
    return x


def cell_and_rest(x, row):
    """(cell, the 22 other bits) of mixed hashes x (uint64 arrays or ints) in `row`."""
    if row == 0:
        return x & 1023, x >> 10
    return (x >> 10) & 1023, (x & 1023) | ((x >> 20) << 10)


def x_of(row, cell, y):
    """The mixed hash put together from a cell of `row` and the 22 bits y."""
    if row == 0:
        return cell | (y << 10)
    return (y & 1023) | (cell << 10) | ((y >> 10) << 20)


def vector_from_pairs(hashes, counts) -> np.ndarray:
    """u64[2, 1024, 23] of records given as (key hash, how many records) pairs."""
    vec = np.zeros((ROWS, CELLS, WORDS), np.uint64)
    x = fmix32(np.asarray(hashes, np.uint64)).astype(np.uint64)
    n = np.asarray(counts, np.uint64)
    for row in range(ROWS):
        cell, y = cell_and_rest(x, row)
        cell = cell.astype(np.int64)
        np.add.at(vec[row, :, 0], cell, n)
        for b in range(BITS):
            on = ((y >> np.uint64(b)) & np.uint64(1)) == 1
            np.add.at(vec[row, :, 1 + b], cell[on], n[on])
    return vec


def vector_from_hashes(hashes) -> np.ndarray:
    """u64[2, 1024, 23] of one record per key hash."""
    h, n = np.unique(np.asarray(hashes, np.uint64), return_counts=True)
    return vector_from_pairs(h, n)


def keyed_hashes(cols, P) -> np.ndarray:
    """The key hashes of the records the sketch counts: key_len >= 0 and a partition in [0, P)."""
    part = np.asarray(cols["partition"], np.int64)
    kl = np.asarray(cols["key_len"], np.int64)
    keep = (kl >= 0) & (part >= 0) & (part < P)
    return fnv_columns(kl[keep], np.asarray(cols["key_off"])[keep], cols["key_bytes"])


def vector(cols, P) -> np.ndarray:
    return vector_from_hashes(keyed_hashes(cols, P))


def merge(a, b) -> np.ndarray:
    return np.asarray(a, np.uint64) + np.asarray(b, np.uint64)


def bounds(vec, x: int):
    """(upper, lower) on the records whose mixed hash is x."""
    upper, lower = None, 0
    for row in range(ROWS):
        cell, y = cell_and_rest(x, row)
        w = [int(v) for v in vec[row][cell]]
        T = w[0]
        agree = [w[1 + b] if (y >> b) & 1 else T - w[1 + b] for b in range(BITS)]
        u = min([T] + agree)
        upper = u if upper is None else min(upper, u)
        lower = max(lower, T - sum(T - a for a in agree))
    return upper, max(0, lower)


def recover(vec, max_keys):
    """([(hash, upper, lower), ...] ordered by upper descending, then hash ascending, cut at max_keys; keyed records)."""
    vec = np.asarray(vec, np.uint64).reshape(ROWS, CELLS, WORDS)
    keyed = int(vec[0, :, 0].astype(object).sum()) if vec.size else 0
    seen = {}
    for row in range(ROWS):
        for cell in np.nonzero(vec[row, :, 0])[0]:
            w = [int(v) for v in vec[row, cell]]
            y = sum(1 << b for b in range(BITS) if 2 * w[1 + b] > w[0])
            x = x_of(row, int(cell), y)
            if x in seen:
                continue
            u, lo = bounds(vec, x)
            if u * FLOOR >= keyed:
                seen[x] = (fmix32_inverse(x), u, lo)
    out = sorted(seen.values(), key=lambda e: (-e[1], e[0]))
    return out[:max_keys], keyed


def key_text(key: bytes) -> str:
    """A key as the section prints it: printable ASCII but the backslash as is, \\xNN else, ... behind 32 bytes."""
    t = "".join(chr(b) if 0x20 <= b < 0x7F and b != 0x5C else "\\x%02X" % b for b in key[:32])
    return t + ("..." if len(key) > 32 else "")


def _table(rows):
    w = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    sep = "+" + "+".join("-" * (x + 2) for x in w) + "+\n"
    out = sep
    for r in rows:
        out += "|" + "|".join(" " + c.ljust(x) + " " for c, x in zip(r, w)) + "|\n" + sep
    return out


def section(vec, max_keys, keys_by_hash=None) -> str:
    """The kta.hot_keys section; keys_by_hash: {hash: key bytes} of the exemplars at hand (a hash without one prints -)."""
    found, keyed = recover(vec, max_keys)
    if not found:
        return title(max_keys) + "No key holds 1/512 of the %d keyed records.\n" % keyed
    rows = [["#", "Key", "Hash", "Records (at most)", "(at least)", "Share of keyed records"]]
    for k, (h, u, lo) in enumerate(found):
        key = (keys_by_hash or {}).get(h)
        rows.append([str(k + 1), "-" if key is None else key_text(key), "%08x" % h, str(u), str(lo),
                     "%.2f" % (u * 100.0 / keyed)])
    return title(max_keys) + _table(rows) + "=" * 120 + "\n"


def exemplar_keys(table) -> dict:
    """{hash: the (at most 32) key bytes + a marker for longer keys} of a structured exemplar table, as section() takes
    them: a key longer than 32 bytes is padded by one byte so that it prints its `...`."""
    out = {}
    for e in table:
        if e["valid"]:
            n = int(e["key_len"])
            out.setdefault(int(e["hash"]), bytes(e["bytes"][:min(n, 32)]) + (b"." if n > 32 else b""))
    return out

"""The size percentiles (KTA_FLAG_SIZE_QUANTILES, include/kta_hip.h) said again in numpy and plain Python, sharing nothing
with the library: the bin rule, the vector, the nearest-rank read-off and the section text."""
import numpy as np

BINS, QUANTITIES, GLOBALS = 464, 3, 8
PERCENTILES = ((50, 100), (90, 100), (99, 100), (999, 1000))
# both sides of every place where the rule changes, and -1 (None)
BOUNDARY_SIZES = (31, 32, 63, 64, 65534, 65535, 65536, 2**31 - 1, 2**31, 2**32 - 1)


def words(P: int) -> int:
    return P * QUANTITIES * BINS + GLOBALS


def bin_of(v: int) -> int:
    v = int(v)
    assert 0 <= v < 2**32
    if v < 32:
        return v
    e = v.bit_length() - 1
    return 32 + 16 * (e - 5) + ((v >> (e - 4)) & 15)


def lo(b: int) -> int:
    return b if b < 32 else (16 + (b - 32) % 16) << ((b - 32) // 16 + 1)


def hi(b: int) -> int:
    return lo(b + 1) - 1          # (lo(464) = 2^32)


def bins_of(values) -> np.ndarray:
    """bin_of over an array of sizes 0 .. 2^32 - 1"""
    v = np.asarray(values, np.uint64)
    out = v.copy()
    big = v >= 32
    e = np.uint64(4) + sum((v[big] >= np.uint64(1 << k)).astype(np.uint64) for k in range(5, 32))   # floor(log2 v)
    out[big] = 32 + 16 * (e - 5) + ((v[big] >> (e - 4)) & np.uint64(15))
    return out.astype(np.int64)


def vector(cols, P: int) -> np.ndarray:
    """u64[P * 3 * 464 + 8] of the records in cols (partition, key_len, val_len)."""
    part = np.asarray(cols["partition"], np.int64)
    kl = np.asarray(cols["key_len"], np.int64)
    vl = np.asarray(cols["val_len"], np.int64)
    counted = (part >= 0) & (part < P)
    v = np.zeros(words(P), np.uint64)
    h = v[:P * QUANTITIES * BINS].reshape(P, QUANTITIES, BINS)
    keyed, alive = counted & (kl >= 0), counted & (vl >= 0)
    np.add.at(h, (part[keyed], 0, bins_of(kl[keyed])), np.uint64(1))
    np.add.at(h, (part[alive], 1, bins_of(vl[alive])), np.uint64(1))
    np.add.at(h, (part[alive], 2, bins_of((np.maximum(kl[alive], 0) + vl[alive]) & 0xFFFFFFFF)), np.uint64(1))
    g = v[P * QUANTITIES * BINS:]
    g[0], g[1], g[2], g[3] = int(counted.sum()), int((~counted).sum()), int(keyed.sum()), int(alive.sum())
    return v


def merge(a, b):
    return np.asarray(a, np.uint64) + np.asarray(b, np.uint64)          # (numpy wraps)


def counters(cols, P: int) -> np.ndarray:
    """The counter vector's words the identities read (u64[P * 7 + 8], the rest zero): key_non_null, alive, the records
    and the bad-partition records."""
    part = np.asarray(cols["partition"], np.int64)
    kl = np.asarray(cols["key_len"], np.int64)
    vl = np.asarray(cols["val_len"], np.int64)
    c = np.zeros(P * 7 + 8, np.uint64)
    for p in range(P):
        m = part == p
        c[p * 7 + 4] = int((m & (kl >= 0)).sum())
        c[p * 7 + 2] = int((m & (vl >= 0)).sum())
    counted = (part >= 0) & (part < P)
    c[P * 7 + 2] = int(counted.sum())
    c[P * 7 + 0] = int((~counted).sum())
    return c


def identities_hold(vec, counter_vec, P: int) -> bool:
    v = np.asarray(vec, np.uint64).reshape(-1)
    c = np.asarray(counter_vec, np.uint64).reshape(-1)
    h = v[:P * QUANTITIES * BINS].reshape(P, QUANTITIES, BINS).sum(axis=2)
    cc = c[:P * 7].reshape(P, 7)
    g = v[P * QUANTITIES * BINS:]
    return bool((h[:, 0] == cc[:, 4]).all() and (h[:, 1] == cc[:, 2]).all() and (h[:, 2] == cc[:, 2]).all()
                and g[0] == c[P * 7 + 2] and g[1] == c[P * 7 + 0] and not g[4:].any())


def quantile(hist, num: int, den: int):
    """(lo, hi) of the first bin whose running count reaches the nearest rank; None for an empty histogram."""
    h = [int(x) for x in hist]
    n = sum(h)
    if n == 0:
        return None
    r = max(1, -((-num * n) // den))          # ceil, in Python's integers
    run = 0
    for b, c in enumerate(h):
        run += c
        if run >= r:
            return lo(b), hi(b)
    raise AssertionError("unreachable")


def sorted_nearest_rank(sizes, num: int, den: int) -> int:
    """The nearest-rank quantile of the sizes themselves."""
    s = sorted(int(x) for x in sizes)
    r = max(1, -((-num * len(s)) // den))
    return s[r - 1]


TITLE = "Size percentiles per partition, in bytes (kta.percentiles=1; not part of the reference report)\n"
TITLES = ("Key sizes\n", "Value sizes\n", "Message sizes (key + value of the non-tombstones)\n")
BOUND = "Sizes below 32 B are exact; a size of 32 B and more is the upper end of its bin, at most 6.25 % wide.\n"


def _table(rows):
    w = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    sep = "+" + "+".join("-" * (x + 2) for x in w) + "+\n"
    out = sep
    for r in rows:
        out += "|" + "|".join(" " + c.ljust(x) + " " for c, x in zip(r, w)) + "|\n" + sep
    return out


def _row(name, hist):
    h = [int(x) for x in hist]
    n = sum(h)
    row = [name, str(n)]
    for num, den in PERCENTILES:
        q = quantile(h, num, den)
        row.append("-" if q is None else str(q[1]))
    row.append(str(hi(max(b for b in range(BINS) if h[b]))) if n else "-")
    return row


def section(vec, P: int) -> str:
    v = np.asarray(vec, np.uint64).reshape(-1)
    assert len(v) == words(P)
    h = v[:P * QUANTITIES * BINS].reshape(P, QUANTITIES, BINS)
    out = TITLE
    for q in range(QUANTITIES):
        rows = [["P", "Count", "p50", "p90", "p99", "p99.9", "Max"]]
        for p in range(P):
            rows.append(_row(str(p), h[p, q]))
        rows.append(_row("All", [sum(int(h[p, q, b]) for p in range(P)) for b in range(BINS)]))
        out += TITLES[q] + _table(rows)
    return out + BOUND + "=" * 120 + "\n"

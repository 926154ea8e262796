"""Independent restatement of the partitioner pass (KTA_FLAG_PARTITIONER), written from the definition in
include/kta_hip.h and from Kafka's Utils.murmur2 / Utils.toPositive: the hash byte by byte in Python integers, the same
hash over a whole key column in numpy, the vector u64[2 P + 2 Q] from columns, the merge, and the text of the
kta.partitioner section."""
import numpy as np

SEED, M, R = 0x9747B28C, 0x5BD1E995, 24
U32, U64 = 0xFFFFFFFF, (1 << 64) - 1

# Kafka's UtilsTest.testMurmur2 (as signed 32-bit integers), "abc" and the empty key
KNOWN = {b"21": -973932308, b"foobar": -790332482, b"a-little-bit-long-string": -985981536,
         b"a-little-bit-longer-string": -1486304829, b"lkjh234lh9fiuh90y23oiuhsafujhadof229phr9h19h89h8": -58897971,
         b"abc": 479470107, b"": 275646681}


def murmur2(key: bytes) -> int:
    """Utils.murmur2 as a u32."""
    n = len(key)
    h = (SEED ^ n) & U32
    for i in range(n // 4):
        k = key[4 * i] | key[4 * i + 1] << 8 | key[4 * i + 2] << 16 | key[4 * i + 3] << 24
        k = (k * M) & U32
        k ^= k >> R
        k = (k * M) & U32
        h = ((h * M) & U32) ^ k
    i = n & ~3
    if n % 4 == 3:
        h ^= key[i + 2] << 16
    if n % 4 >= 2:
        h ^= key[i + 1] << 8
    if n % 4 >= 1:
        h ^= key[i]
        h = (h * M) & U32
    h ^= h >> 13
    h = (h * M) & U32
    return h ^ (h >> 15)


def to_positive(h: int) -> int:
    return h & 0x7FFFFFFF


def _mul(a, b=M):
    return (a.astype(np.uint64) * np.uint64(b)).astype(np.uint32)        # (the product fits 64 bits)


def murmur2_matrix(keys: np.ndarray) -> np.ndarray:
    """murmur2 of every row of a uint8 matrix [m, L]: u32[m]."""
    m, L = keys.shape
    h = np.full(m, (SEED ^ L) & U32, np.uint32)
    b = keys.astype(np.uint32)
    for i in range(L // 4):
        k = b[:, 4 * i] | b[:, 4 * i + 1] << np.uint32(8) | b[:, 4 * i + 2] << np.uint32(16) | b[:, 4 * i + 3] << np.uint32(24)
        k = _mul(k)
        k ^= k >> np.uint32(R)
        k = _mul(k)
        h = _mul(h) ^ k
    i = L & ~3
    if L % 4 == 3:
        h = h ^ (b[:, i + 2] << np.uint32(16))
    if L % 4 >= 2:
        h = h ^ (b[:, i + 1] << np.uint32(8))
    if L % 4 >= 1:
        h = _mul(h ^ b[:, i])
    h = h ^ (h >> np.uint32(13))
    h = _mul(h)
    return h ^ (h >> np.uint32(15))


def hashes(cols) -> np.ndarray:
    """murmur2 of every record's key: u32[n] (0 where the key is None), the keys gathered by length."""
    kl = np.asarray(cols["key_len"], np.int64)
    ko = np.asarray(cols["key_off"], np.int64)
    kb = np.asarray(cols["key_bytes"], np.uint8)
    out = np.zeros(len(kl), np.uint32)
    for L in np.unique(kl[kl >= 0]):
        idx = np.nonzero(kl == L)[0]
        L = int(L)
        mat = kb[ko[idx][:, None] + np.arange(L)[None, :]] if L else np.zeros((len(idx), 0), np.uint8)
        out[idx] = murmur2_matrix(mat)
    return out


def words(P, Q):
    return 2 * P + 2 * Q


def vector(cols, P, Q=None, h=None) -> np.ndarray:
    """The partitioner vector of the records the metrics handler counts."""
    Q = P if Q is None else Q
    part = np.asarray(cols["partition"], np.int64)
    kl = np.asarray(cols["key_len"], np.int64)
    vl = np.asarray(cols["val_len"], np.int64)
    h = hashes(cols) if h is None else h
    keyed = (kl >= 0) & (part >= 0) & (part < P)
    t = (h[keyed] & np.uint32(0x7FFFFFFF)).astype(np.int64)
    p = part[keyed]
    size = (kl[keyed] + np.maximum(vl[keyed], 0)).astype(np.uint64)
    v = np.zeros(words(P, Q), np.uint64)
    v[0:2 * P:2] = np.bincount(p, minlength=P).astype(np.uint64)
    v[1:2 * P:2] = np.bincount(p[t % P == p], minlength=P).astype(np.uint64)
    v[2 * P::2] = np.bincount(t % Q, minlength=Q).astype(np.uint64)
    tb = np.zeros(Q, np.uint64)
    np.add.at(tb, t % Q, size)
    v[2 * P + 1::2] = tb
    return v


def merge(a, b):
    return np.asarray(a, np.uint64) + np.asarray(b, np.uint64)          # (numpy wraps)


def counters(cols, P) -> np.ndarray:
    """The counter vector's words the section reads (u64[P * 7 + 8], the rest zero): key_null, key_non_null,
    key_size_sum, value_size_sum."""
    part = np.asarray(cols["partition"], np.int64)
    kl = np.asarray(cols["key_len"], np.int64)
    vl = np.asarray(cols["val_len"], np.int64)
    c = np.zeros(P * 7 + 8, np.uint64)
    for p in range(P):
        m = part == p
        c[p * 7 + 3] = int((m & (kl < 0)).sum())
        c[p * 7 + 4] = int((m & (kl >= 0)).sum())
        c[p * 7 + 5] = int(np.maximum(kl[m], 0).sum())
        c[p * 7 + 6] = int(np.maximum(vl[m], 0).sum())
    return c


TITLE = ("Partitioner check: keyed records on the partition Kafka's default partitioner (murmur2) gives their key "
         "(kta.partitioner=murmur2; not part of the reference report)\n")


def _table(rows):
    w = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    sep = "+" + "+".join("-" * (x + 2) for x in w) + "+\n"
    out = sep
    for r in rows:
        out += "|" + "|".join(" " + c.ljust(x) + " " for c, x in zip(r, w)) + "|\n" + sep
    return out


def section(vec, counter_vec, P, Q) -> str:
    v = [int(x) for x in np.asarray(vec, np.uint64).reshape(-1)]
    c = [int(x) for x in np.asarray(counter_vec, np.uint64).reshape(-1)]
    assert len(v) == words(P, Q) and len(c) == P * 7 + 8
    checked, placed = v[0:2 * P:2], v[1:2 * P:2]
    recs, size = v[2 * P::2], v[2 * P + 1::2]

    def pct(x, of):
        return "%.2f" % (float(x) * 100.0 / float(of)) if of else "-"

    def skew(values):
        return "%.2f" % (float(max(values)) * float(len(values)) / float(sum(values))) if sum(values) else "-"

    rows = [["P", "Keyed records", "On murmur2's partition", "%"]]
    for p in range(P):
        rows.append([str(p), str(checked[p]), str(placed[p]) if checked[p] else "-", pct(placed[p], checked[p])])
    ca, pa = sum(checked), sum(placed)
    rows.append(["Topic", str(ca), str(pa) if ca else "-", pct(pa, ca)])
    out = TITLE + _table(rows)
    out += "Records without a key: %d (the default partitioner spreads them without a hash)\n" % sum(c[p * 7 + 3] for p in range(P))
    if ca == 0:
        out += "No record has a key: nothing to check.\n"
    elif pa == ca:
        out += "All keyed records lie on murmur2's partition: the topic is keyed as Kafka's default partitioner keys it.\n"
    elif P > 2 and pa * P <= 2 * ca:
        out += ("No more keyed records lie on murmur2's partition than chance puts there (%s %% against 1/P = %s %%): the topic "
                "was not written by Kafka's default partitioner with %d partitions.\n" % (pct(pa, ca), pct(1, P), P))
    else:
        out += ("%s %% of the keyed records lie on murmur2's partition: the topic is only partly keyed as Kafka's default "
                "partitioner keys it.\n" % pct(pa, ca))
    out += "Repartition what-if: the keyed records over Q = %d partitions by murmur2\n" % Q
    rows = [["Target", "Records", "Records %", "Bytes", "Bytes %"]]
    for q in range(Q):
        rows.append([str(q), str(recs[q]), pct(recs[q], sum(recs)), str(size[q]), pct(size[q], sum(size))])
    out += _table(rows)
    keyed = [c[p * 7 + 4] for p in range(P)]
    volume = [c[p * 7 + 5] + c[p * 7 + 6] for p in range(P)]
    out += ("Largest / mean at Q = %d: records %s, bytes %s; the topic as it is (P = %d): records %s, bytes %s\n"
            % (Q, skew(recs), skew(size), P, skew(keyed), skew(volume)))
    return out + "=" * 120 + "\n"

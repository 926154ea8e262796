"""Independent numpy / math restatement of the key sketch (include/kta_hip.h, KTA_FLAG_KEY_SKETCH): the registers, Ertl's
improved raw estimator, the merge and the kta.distinct_keys section.  Shares no code with the library."""
import math

import numpy as np

LOG2 = 12
M = 1 << LOG2
Q = 32 - LOG2
TITLE = ("Distinct keys per partition, estimated (HyperLogLog of the key hashes, +/-1.6 %; kta.distinct_keys=1; not part "
         "of the reference report)\n")
U32 = np.uint64(0xFFFFFFFF)


def fnv1a(key: bytes) -> int:
    """The reference's FNV variant (fnv32.rs:76-101): the multiplier is the offset basis."""
    h = 0x811C9DC5
    for b in key:
        h = ((h ^ b) * 0x811C9DC5) & 0xFFFFFFFF
    return h


def fnv_columns(key_len, key_off, key_bytes) -> np.ndarray:
    """FNV of every key of columns (uint32; a key None hashes like the empty key, the caller masks it)."""
    kl = np.maximum(np.asarray(key_len, np.int64), 0)
    off = np.asarray(key_off, np.int64)
    kb = np.asarray(key_bytes, np.uint8)
    h = np.full(len(kl), 0x811C9DC5, np.uint64)
    for j in range(int(kl.max()) if len(kl) else 0):
        live = kl > j
        b = kb[off[live] + j].astype(np.uint64)
        h[live] = ((h[live] ^ b) * np.uint64(0x811C9DC5)) & U32
    return h.astype(np.uint32)


def fmix32(h) -> np.ndarray:
    x = np.asarray(h, np.uint64) & U32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & U32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & U32
    x ^= x >> np.uint64(16)
    return x


def register_and_rho(hashes):
    """(register index, rho) of 32-bit key hashes."""
    x = fmix32(hashes)
    j = (x >> np.uint64(32 - LOG2)).astype(np.int64)
    w = (x << np.uint64(LOG2)) & U32
    rho = np.full(len(x), Q + 1, np.int64)
    nz = w != 0
    # clz32(w) + 1 = 32 - floor(log2(w)); floor(log2) exactly via bit_length on the integers
    bl = np.frexp(w[nz].astype(np.float64))[1]          # w < 2^32: exact in a double, frexp's exponent is bit_length
    rho[nz] = 32 - bl + 1
    return j, rho


def sketch_from_hashes(partition, hashes, P) -> np.ndarray:
    """u64[P, 4096] registers of (partition, hash) pairs (partitions already in [0, P))."""
    regs = np.zeros(P * M, np.uint64)
    if len(hashes):
        j, rho = register_and_rho(hashes)
        np.maximum.at(regs, np.asarray(partition, np.int64) * M + j, rho.astype(np.uint64))
    return regs.reshape(P, M)


def sketch(cols, P) -> np.ndarray:
    """The registers the sketch keeps for columns: keyed records (key_len >= 0) with a partition in [0, P)."""
    part = np.asarray(cols["partition"], np.int64)
    kl = np.asarray(cols["key_len"], np.int64)
    keep = (kl >= 0) & (part >= 0) & (part < P)
    h = fnv_columns(kl[keep], np.asarray(cols["key_off"])[keep], cols["key_bytes"])
    return sketch_from_hashes(part[keep], h, P)


def merge(a, b) -> np.ndarray:
    return np.maximum(np.asarray(a, np.uint64), np.asarray(b, np.uint64))


def _sigma(x):
    if x == 1.0:
        return math.inf
    y, z = 1.0, x
    while True:
        x = x * x
        zp = z
        z += x * y
        y *= 2
        if z == zp:
            return z


def _tau(x):
    if x == 0.0 or x == 1.0:
        return 0.0
    y, z = 1.0, 1.0 - x
    while True:
        x = math.sqrt(x)
        zp = z
        y /= 2
        z -= (1 - x) ** 2 * y
        if z == zp:
            return z / 3


def estimate_registers(regs) -> float:
    """Ertl 2017, Algorithm 6, for one partition's 4096 registers."""
    c = [int(x) for x in np.bincount(np.asarray(regs, np.int64).reshape(-1), minlength=Q + 2)]
    assert len(c) == Q + 2, "a register above q + 1"
    z = M * _tau(1 - c[Q + 1] / M)
    for k in range(Q, 0, -1):
        z = (z + c[k]) / 2
    z += M * _sigma(c[0] / M)
    return math.inf if z == 0 else M * M / (2 * math.log(2)) / z


def estimate(sk):
    """(per-partition estimates, topic-wide estimate of the register-wise max)."""
    sk = np.asarray(sk, np.uint64).reshape(-1, M)
    return [estimate_registers(r) for r in sk], estimate_registers(sk.max(axis=0))


def _table(rows):
    w = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    sep = "+" + "+".join("-" * (x + 2) for x in w) + "+\n"
    out = sep
    for r in rows:
        out += "|" + "|".join(" " + c.ljust(x) + " " for c, x in zip(r, w)) + "|\n" + sep
    return out


def section(sk, keyed) -> str:
    """The kta.distinct_keys section: sketch u64[P, 4096], keyed[p] = key_non_null of partition p."""
    per, topic = estimate(sk)

    def count(e):
        return str(int(round(e))) if math.isfinite(e) else "inf"

    def per_key(records, e):
        if not math.isfinite(e) or round(e) == 0:
            return "-"
        return "%.2f" % (records / round(e))

    rows = [["P", "Keyed records", "Distinct keys", "Records per key"]]
    for p, k in enumerate(keyed):
        k = int(k)
        rows.append([str(p), "0", "-", "-"] if k == 0 else [str(p), str(k), count(per[p]), per_key(k, per[p])])
    total = int(sum(int(k) for k in keyed))
    rows.append(["Topic", "0", "-", "-"] if total == 0 else ["Topic", str(total), count(topic), per_key(total, topic)])
    return TITLE + _table(rows) + "=" * 120 + "\n"


# ---- the synthetic topic's key ids (include/kta_synth.h), for laws too large to materialise the key bytes of
MASK64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix64(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def synth_rng(seed, i, s):
    with np.errstate(over="ignore"):
        return _mix64(_mix64(np.uint64(seed) ^ (np.asarray(i, np.uint64) * np.uint64(0xD1B54A32D192ED03))) + np.uint64(s))


def synth_key_ids(spec, first, n):
    """kta_synth_key_id of records [first, first + n): -1 for a key None."""
    i = np.arange(first, first + n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        r0 = synth_rng(int(spec.seed), i, 0)
        null = (r0 % np.uint64(1000)).astype(np.uint32) < np.uint32(spec.key_null_permille)
        kid = ((r0 >> np.uint64(10)) % np.uint64(spec.n_distinct_keys)) if spec.n_distinct_keys else i
    kid = (kid & np.uint64(0x7FFFFFFFFFFFFFFF)).astype(np.int64)
    kid[null] = -1
    return kid


def synth_key_hashes(spec, key_ids):
    """FNV of the keys of `key_ids` (kta_synth_key_len / kta_synth_key_byte)."""
    kid = np.asarray(key_ids, np.uint64)
    with np.errstate(over="ignore"):
        kr = synth_rng(int(spec.seed) ^ 0x6B65795F6C656E, kid, 1)
        lens = np.array([spec.key_lens[k] for k in range(spec.n_key_lens)], np.int64)
        kl = lens[((kr >> np.uint64(10)) % np.uint64(spec.n_key_lens)).astype(np.int64)]
        kl[(kr % np.uint64(1000)).astype(np.uint32) < np.uint32(spec.key_empty_permille)] = 0
        h = np.full(len(kid), 0x811C9DC5, np.uint64)
        for w in range(int((kl.max() + 7) // 8) if len(kl) else 0):
            word = kid if w == 0 else synth_rng(int(spec.seed) ^ 0x6B65795F627974, kid, w)
            for b in range(8):
                live = kl > 8 * w + b
                byte = (word[live] >> np.uint64(8 * b)) & np.uint64(0xFF)
                h[live] = ((h[live] ^ byte) * np.uint64(0x811C9DC5)) & U32
    return h.astype(np.uint32)

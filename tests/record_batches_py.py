"""The record-batch section (KTA_FLAG_RECORD_BATCHES) restated in pure Python (test infrastructure): the blob is parsed with
`struct`, nothing of the library is called.  A batch's inflated size is never measured here: the caller gives the length of the
encoder's own uncompressed record bytes, known by construction (record_batches_blobs.py).  Layout and rule: include/kta_hip.h
above KTA_FLAG_RECORD_BATCHES."""
import math
import struct

import numpy as np

HEADER = 61
PART_WORDS, CODECS, CODEC_WORDS, BINS, MAX_WORDS, REGS = 16, 5, 100, 32, 4, 1024
(BATCHES, RECORDS, WIRE, PAYLOAD, COMPRESSED, C_RECBYTES, C_PAYLOAD, EXTENT, TRANSACTIONAL, IDEMPOTENT, LOG_APPEND, SPAN, FAILED) = range(13)
M64 = (1 << 64) - 1
STD_ERROR = 1.04 / math.sqrt(REGS)


def words(P):
    return 20 * P + 1524


def sum_words(P):
    return 16 * P + 500


def codec_at(P, c):
    return 16 * P + 100 * c


def max_at(P, p):
    return 16 * P + 500 + 4 * p


def sketch_at(P):
    return 20 * P + 500


def bin_of(x):
    return 0 if x == 0 else min(31, x.bit_length())       # 1 + floor(log2 x)


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def register_and_rank(producer_id):
    h = splitmix64(producer_id & M64)
    w = ((h << 10) | (1 << 9)) & M64
    return h >> 54, 1 + (64 - w.bit_length())


def parse(blob):
    """Every whole batch of the blob, in order: a dict of its header fields, `pos` and `total` (12 + batchLength)."""
    out, pos = [], 0
    while pos + 12 <= len(blob):
        base_offset, length = struct.unpack_from(">qi", blob, pos)
        if length < HEADER - 12 or pos + 12 + length > len(blob):
            break
        epoch, magic, crc = struct.unpack_from(">iBI", blob, pos + 12)
        b = {"pos": pos, "total": 12 + length, "base_offset": base_offset, "epoch": epoch, "magic": magic, "crc": crc}
        if magic == 2:
            (b["attributes"], b["last_offset_delta"], b["base_ts"], b["max_ts"], b["producer_id"], b["producer_epoch"], b["base_sequence"],
             b["count"]) = struct.unpack_from(">hiqqqhii", blob, pos + 21)
        out.append(b)
        pos += 12 + length
    return out


def described(b):
    """Whether the host index writes a descriptor for the batch: magic 2, no control batch, a known codec, records."""
    return b["magic"] == 2 and not b["attributes"] & 0x20 and (b["attributes"] & 7) <= 4 and b["count"] > 0


def passes(b, partition, P, flt):
    """flt: None, or (from_ms | None, to_ms | None, set of partitions | None)."""
    if not 0 <= partition < P:
        return False
    if flt is None:
        return True
    lo, hi, parts = flt
    if parts is not None and partition not in parts:
        return False
    if hi is not None and not b["base_ts"] < hi:
        return False
    if lo is not None and not b["max_ts"] >= lo:
        return False
    return True


def add_batch(v, P, partition, b, inflated, failed):
    """One described, counted batch into the vector (a list of Python ints)."""
    pw = 16 * partition
    if failed:
        v[pw + FAILED] += 1
        return
    codec = b["attributes"] & 7
    n, wire = b["count"], b["total"]
    recbytes = wire - HEADER
    payload = recbytes if codec == 0 else inflated
    span = min(max(b["max_ts"] - b["base_ts"], 0), 2 ** 31 - 1)
    extent = max(b["last_offset_delta"] + 1, n)
    idem = b["producer_id"] >= 0
    for k, x in ((BATCHES, 1), (RECORDS, n), (WIRE, wire), (PAYLOAD, payload), (COMPRESSED, int(codec != 0)),
                 (C_RECBYTES, recbytes if codec else 0), (C_PAYLOAD, payload if codec else 0), (EXTENT, extent),
                 (TRANSACTIONAL, int(bool(b["attributes"] & 0x10))), (IDEMPOTENT, int(idem)), (LOG_APPEND, int(bool(b["attributes"] & 0x08))),
                 (SPAN, span)):
        v[pw + k] += x
    cw = codec_at(P, codec)
    for k, x in ((0, 1), (1, n), (2, recbytes), (3, payload), (4 + bin_of(n), 1), (36 + bin_of(wire), 1), (68 + bin_of(span), 1)):
        v[cw + k] += x
    mw = max_at(P, partition)
    for k, x in enumerate((n, wire, b["epoch"] + 1 if b["epoch"] >= 0 else 0, span)):
        v[mw + k] = max(v[mw + k], x)
    if idem:
        reg, rank = register_and_rank(b["producer_id"])
        v[sketch_at(P) + reg] = max(v[sketch_at(P) + reg], rank)


def restate(sets, P, flt=None):
    """sets: [(blob, partition, inflated, failed)] in any order — inflated: the uncompressed record bytes of every batch of the
    blob (one per batch that parse() finds, described or not), failed: the indices (into parse()'s list) of the batches that
    the device must report as failed.  Returns the vector as np.uint64."""
    v = [0] * words(P)
    for blob, partition, inflated, failed in sets:
        for i, b in enumerate(parse(blob)):
            if described(b) and passes(b, partition, P, flt):
                add_batch(v, P, partition, b, inflated[i], i in failed)
    return np.array([x & M64 for x in v], np.uint64)


def restate_parts(blob, partitions, P, inflated, failed=(), flt=None):
    """One blob whose DESCRIBED batches belong to partitions[k] for the k-th described batch (one decode call with the
    partitions interleaved batch by batch)."""
    v = [0] * words(P)
    k = 0
    for i, b in enumerate(parse(blob)):
        if not described(b):
            continue
        if passes(b, partitions[k], P, flt):
            add_batch(v, P, partitions[k], b, inflated[i], i in failed)
        k += 1
    return np.array([x & M64 for x in v], np.uint64)


def merge(a, b, P):
    a, b = [int(x) for x in a], [int(x) for x in b]
    s = sum_words(P)
    return np.array([(x + y) & M64 for x, y in zip(a[:s], b[:s])] + [max(x, y) for x, y in zip(a[s:], b[s:])], np.uint64)


def estimate(regs):
    """HyperLogLog's estimate of regs[1024]: linear counting while the raw estimate is at most 2.5 m and a register is empty."""
    regs = [int(r) for r in regs]
    m = float(REGS)
    empty = sum(1 for r in regs if r == 0)
    if empty == REGS:
        return 0.0
    e = 0.7213 / (1.0 + 1.079 / m) * m * m / sum(2.0 ** -r for r in regs)
    if e <= 2.5 * m and empty:
        return m * math.log(m / empty)
    return e


def sketch_of(ids):
    regs = [0] * REGS
    for x in ids:
        reg, rank = register_and_rank(int(x))
        regs[reg] = max(regs[reg], rank)
    return regs


def identities(v, P, counters_records=None):
    """The identities of the section as a list of (name, holds)."""
    v = [int(x) for x in v]
    part = lambda k: sum(v[16 * p + k] for p in range(P))                                    # noqa: E731
    cod = lambda k, first=0: sum(v[codec_at(P, c) + k] for c in range(first, CODECS))        # noqa: E731
    out = [("batches", cod(0) == part(BATCHES)), ("records", cod(1) == part(RECORDS)), ("payload", cod(3) == part(PAYLOAD)),
           ("compressed batches", cod(0, 1) == part(COMPRESSED)), ("compressed recbytes", cod(2, 1) == part(C_RECBYTES)),
           ("compressed payload", cod(3, 1) == part(C_PAYLOAD)),
           ("zero words", all(v[16 * p + k] == 0 for p in range(P) for k in (13, 14, 15)))]
    for c in range(CODECS):
        at = codec_at(P, c)
        for name, h in (("records", 4), ("wire", 36), ("span", 68)):
            out.append(("hist %s of codec %d" % (name, c), sum(v[at + h:at + h + BINS]) == v[at]))
    if counters_records is not None:
        out.append(("records delivered", part(RECORDS) == counters_records))
    return out

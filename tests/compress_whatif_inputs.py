"""Inputs for the tests of the compression what-if (test infrastructure): the records-section lengths, the byte laws and the
crafted blocks at which the model compressor's kernel can go wrong, and batches whose records section has a given length."""
import numpy as np

import kafka_format as K
import lz4_model_py as M
import payload_blobs as B

LENGTHS = (1, 12, 13, 16, 64, 65, 75, 76, 77, 140, 4096, 65535, 65536, 65537, 65536 + 12, 65536 + 13, 3 * 65536 + 5)
LAWS = ("zeros", "period1", "period2", "period3", "period24", "period63", "period64", "period65", "text", "random")
WORDS = (b"user", b"action", b"click", b"view", b"purchase", b"session", b"timestamp", b"amount", b"currency", b"EUR", b"status", b"ok",
         b"error", b"region", b"eu-west", b"device", b"mobile", b"items")


def rand(n, seed=0):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def text(n, seed=0):
    """JSON-like: words of a small vocabulary, numbers, punctuation."""
    rng, out, size = np.random.default_rng(1000 + seed), [], 0
    while size < n:
        picks = rng.integers(0, len(WORDS), 4)
        rec = b'{"%s":"%s","%s":%d,"%s":%d.%02d},' % (WORDS[picks[0]], WORDS[picks[1]], WORDS[picks[2]], int(rng.integers(0, 100000)),
                                                         WORDS[picks[3]], int(rng.integers(0, 1000)), int(rng.integers(0, 100)))
        out.append(rec)
        size += len(rec)
    return b"".join(out)[:n]


def law(name, n, seed=0):
    if name == "zeros":
        return bytes(n)
    if name == "text":
        return text(n, seed)
    if name == "random":
        return rand(n, seed)
    period = int(name[len("period"):])
    unit = bytes([0x41 + (7 * k + seed) % 26 for k in range(period)]) if period > 1 else b"\xee"
    return (unit * (n // period + 1))[:n]


def _find_collision():
    """Two different dwords with one hash."""
    v1 = 0x64636261
    h = ((v1 * 2654435761) & 0xFFFFFFFF) >> 20
    v2 = v1 + 1
    while ((v2 * 2654435761) & 0xFFFFFFFF) >> 20 != h or any(b == 0 for b in v2.to_bytes(4, "little")):
        v2 += 1
    return v1.to_bytes(4, "little"), v2.to_bytes(4, "little")


def crafted():
    """{name: (block, check)}: check takes the sequences lz4_model_py.sequences gives, [(literal start, literal length, offset,
    match length)], and says whether the block shows what its name says."""
    out = {}
    x = rand(100, 1)
    out["a match that runs exactly to n - 5"] = (x + x, lambda s, n=200: any(off and a + ll + m == n - 5 for a, ll, off, m in s))
    for ll in (14, 15, 16, 269, 270):
        w, gap, tail = rand(8, 10 + ll), rand(ll - 8, 20 + ll), rand(20, 30 + ll)
        out["a literal run of %d" % ll] = (w + gap + w + tail, lambda s, ll=ll: s[0][1] == ll and s[0][2] == ll)      # (the candidate is position 0)
    for m in (18, 19, 273, 274):
        w, gap, tail = rand(m, 40 + m), rand(70, 50 + m), rand(20, 60 + m)
        tail = bytes([gap[0] ^ 0x55]) + tail                                                                          # the byte behind the match differs
        out["a match of 4 + %d" % (m - 4)] = (w + gap + w + tail, lambda s, m=m: any(mm == m for _, _, off, mm in s if off))
    w = b"\x01\x02\x03\x04\x05\x06\x07\x08"
    far = w + bytes(65516) + w[:4] + rand(8, 70)
    assert len(far) == 65536
    out["the farthest candidate of a full block"] = (far, lambda s: any(off == 65524 for _, _, off, _ in s))
    a, b = _find_collision()
    clash = rand(30, 80) + a + b"\xf1\xf2" + b + rand(90, 81) + a + rand(6, 82) + b + rand(30, 83)
    out["two positions of one stride with one hash"] = (clash, lambda s: True)
    w16 = rand(16, 90)
    out["a hit whose candidate is position 0"] = (w16 + rand(100, 91) + w16 + rand(20, 92), lambda s: any(off and a + ll == off for a, ll, off, _ in s))
    out["a second hit inside the first hit's match"] = (rand(5, 93) + w16 + rand(100, 94) + w16 + rand(20, 95),
                                                      lambda s: sum(1 for _, _, off, _ in s if off) == 1)
    w300 = rand(300, 96)
    out["a match longer than a lane's cap, across strides"] = (w300 + rand(70, 97) + w300 + rand(20, 98), lambda s: any(mm >= 300 for _, _, off, mm in s if off))
    out["zeros across strides and a change behind them"] = (bytes(1000) + rand(40, 99), lambda s: any(mm > 900 for _, _, off, mm in s if off))
    return out


def section(n, name, seed=0):
    """Records whose bytes, one after the other, take exactly n bytes (n >= 12): one record, or two when a length varint's step
    leaves n out; the values follow the law.  Returns [record bytes]."""
    for first in (0, 8):
        head = [B.filler(0, first)] if first else []
        rest = n - first
        for key in (None, b"", b"k"):
            for vl in range(max(rest - 12, 0), rest):
                r = B.record(len(head), law(name, vl, seed), key=key)
                if len(r) == rest:
                    return head + [r]
    raise ValueError(n)


def batch(n, name, seed=0, base_offset=0, compression=None, base_ts=B.T0):
    """(batch bytes, its records section of exactly n bytes)."""
    recs = section(n, name, seed)
    b, raw = B.batch(base_offset, recs, base_ts=base_ts, compression=compression)
    assert len(raw) == n
    return b, raw


def want(batches, P):
    """The vector lz4_model_py restates for [(partition, codec, batch bytes, raw)]."""
    return M.restate([(p, c, len(b), raw) for p, c, b, raw in batches], P)

"""Blobs for the tests of the header-name section (test infrastructure), on top of payload_blobs.py: names and values astride
a window's end, names that are hot in every lane, many distinct names, and names found on the CPU to share table cells."""
import functools

import header_names_py as H
import payload_blobs as B

WINDOW = B.WINDOW


def astride(field: str, span=16):
    """(blob, raw, n_records): batch by batch, the second record's first header has a `span`-byte name (field == "name") or
    value (field == "value") whose first byte lies at offset 3056 .. 3071 of the batch's first window: the window's end falls
    behind each of its bytes in turn."""
    marker = bytes(range(0x41, 0x41 + span))
    headers = [(marker, b"v"), (b"null", None)] if field == "name" else [(b"n", marker), (b"null", None)]
    second = B.record(1, b"value", headers=headers)
    at = second.index(marker)
    blob, raw = b"", {}
    for t in range(WINDOW - span, WINDOW):
        payload = len(blob) + 61
        wbase = payload & ~127
        first = B.filler(0, wbase + t - at - payload)
        recs = [first, second] + [B.record(2 + i, b"x" * i, headers=headers[:i % 3]) for i in range(4)]
        b, r = B.batch(0, recs)
        where = payload + len(first) + at
        raw[len(blob)] = r
        blob += b
        assert where == wbase + t and blob[where:where + span] == marker
    return blob, raw, span * 6


def hot_wave(n_batches=8, per_batch=16):
    """A few names on every record of every lane: the same cache slots from all 64 lanes at once."""
    hs = [(b"traceparent", b"00-0123456789abcdef-01"), (b"correlation-id", b"c" * 36), (b"__replicated-from", None)]
    return B.join([B.batch(per_batch * b, [B.record(i, b"v", headers=hs) for i in range(per_batch)]) for b in range(n_batches)])


def distinct_names(n, per_record=4, per_batch=16, prefix=b"name-"):
    """n distinct names, per_record of them on a record, the records in batches of per_batch; a name's value length and
    nullness follow its number.  Returns (blob, raw, [names])."""
    names = [prefix + b"%03d" % i for i in range(n)]
    recs = []
    for r in range((n + per_record - 1) // per_record):
        recs.append(B.record(r % per_batch, b"v", headers=[(nm, None if (r + k) % 7 == 0 else b"x" * ((r + k) % 5))
                                                          for k, nm in enumerate(names[r * per_record:(r + 1) * per_record])]))
    blob, raw = B.join([B.batch(i, recs[i:i + per_batch]) for i in range(0, len(recs), per_batch)])
    return blob, raw, names


@functools.lru_cache(maxsize=None)
def colliding_names():
    """(a pair of names that share their row-0 cell but not their row-1 cell, a pair that shares both), found by search."""
    by_row0, by_both, one, both = {}, {}, None, None
    for i in range(200000):
        name = b"hdr-%d" % i
        h = H.fnv1a(name)
        c0, c1 = H.cell(0, h), H.cell(1, h)
        if both is None and (c0, c1) in by_both and H.fnv1a(by_both[(c0, c1)]) != h:
            both = (by_both[(c0, c1)], name)
        by_both.setdefault((c0, c1), name)
        if one is None and c0 in by_row0 and H.cell(1, H.fnv1a(by_row0[c0])) != c1:
            one = (by_row0[c0], name)
        by_row0.setdefault(c0, name)
        if one and both:
            return one, both
    raise AssertionError("no colliding names among 200000")

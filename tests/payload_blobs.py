"""Blobs for the tests of the payload section (test infrastructure): records with any value, any headers and any — also
malformed — header section, in batches of every codec, and the bookkeeping the restatement (payload_py.py) needs."""
import struct

import kafka_format as K

T0 = 1_600_000_000_000
CODECS = (None, "gzip", "snappy", "lz4", "zstd")

# a header section for every way in which one is bad (the section's definition), by name
BAD_HEADERS = {
    "negative count": K.varint(-1),
    "negative key length": K.varint(1) + K.varint(-1),
    "value length below -1": K.varint(1) + K.varint(1) + b"a" + K.varint(-2),
    "varint past ten bytes": b"\x80" * 10 + b"\x00",
    "key overruns the record": K.varint(1) + K.varint(5) + b"ab",
    "value overruns the record": K.varint(1) + K.varint(1) + b"a" + K.varint(9) + b"xy",
    "count beyond the record": K.varint(2) + K.varint(1) + b"a" + K.varint(1) + b"b",
    "bytes behind the last header": K.varint(0) + b"\x00",
    "absent": b"",
}


def framed(schema_id, body=b"\x02avro"):
    return b"\x00" + struct.pack(">I", schema_id) + body


def header_bytes(headers):
    out = K.varint(len(headers))
    for hk, hv in headers:
        out += K.varint(len(hk)) + hk + (K.varint(-1) if hv is None else K.varint(len(hv)) + hv)
    return out


def record(i, value, key=b"k", headers=(), ts_delta=0, raw_headers=None):
    """One record's bytes; raw_headers: the header section as given, whatever it holds."""
    body = b"\x00" + K.varint(ts_delta) + K.varint(i)
    body += K.varint(-1) if key is None else K.varint(len(key)) + key
    body += K.varint(-1) if value is None else K.varint(len(value)) + value
    body += header_bytes(headers) if raw_headers is None else raw_headers
    return K.varint(len(body)) + body


def value_offset(rec, value, tail):
    """Where the value's bytes begin inside a record that ends with value + tail."""
    return len(rec) - len(tail) - (len(value) if value else 0)


def filler(i, nbytes):
    """A record without headers that takes exactly nbytes (>= 8)."""
    for key_len in range(0, 3):
        for vl in range(max(nbytes - 12, 0), nbytes):
            r = record(i, b"x" * vl, key=b"k" * key_len)
            if len(r) == nbytes:
                return r
    raise ValueError(nbytes)


def batch(base_offset, recs, base_ts=T0, compression=None, attributes=0, max_ts=None, count=None):
    """(batch bytes, the uncompressed record bytes)."""
    raw = b"".join(recs)
    n = len(recs) if count is None else count
    return K.encode_batch(base_offset, [], base_ts, attributes=attributes, max_ts=base_ts if max_ts is None else max_ts, raw_records=raw,
                          count=n, compression=compression, last_offset_delta=max(n - 1, 0)), raw


def join(batches):
    """(blob, raw): raw maps the position of every batch to its uncompressed record bytes."""
    blob, raw = b"", {}
    for b, r in batches:
        raw[len(blob)] = r
        blob += b
    return blob, raw


def mixed_records(n, seed=0, start=0):
    """n records that run through the classes, some ids, keys and header counts."""
    out = []
    for q in range(n):
        i = q + seed
        value = (None, b"", framed(100 + i % 7), b'{"a":%d}' % i, b"plain-%d" % i, framed(5000 + i % 3, b""), b"[1]", b"\x00abc")[i % 8]
        headers = [(b"h%d" % h, (None if (h + i) % 5 == 0 else b"v" * ((h * 3 + i) % 9))) for h in range((i * 7) % 4 if i % 3 else 0)]
        out.append(record(start + q, value, key=None if i % 4 == 0 else b"key-%d" % (i % 11), headers=headers, ts_delta=q))
    return out


def mixed(n_batches, per_batch, seed=0, compression=None, misalign=True):
    """n_batches batches of per_batch (+- a few) mixed records; with `misalign` the batches' sizes vary so that byte_off runs
    through the residues mod 16."""
    out, off = [], 0
    for b in range(n_batches):
        n = max(1, per_batch + (b % 3 - 1 if misalign and per_batch > 1 else 0))
        recs = mixed_records(n, seed + 13 * b)
        if misalign:
            recs.append(record(n, b"p" * (b % 16), key=None))
            n += 1
        out.append(batch(off, recs, compression=compression[b % len(compression)] if isinstance(compression, (list, tuple)) else compression))
        off += n
    return join(out)


WINDOW = 3072                                  # the kernel's window; its windows begin on 128-byte lines


def window_edges(value, tail=((b"h", b"12"), (b"null", None))):
    """(blob, raw, n_records): batch by batch, the second record's value begins at offset 3064 .. 3079 of the batch's first
    window: its first byte is the window's last valid byte (3071), its head lies astride the end, its length varint lies
    astride the end or behind it."""
    tail = list(tail)
    second = record(1, value, headers=tail)
    at = value_offset(second, value, header_bytes(tail))
    blob, raw, where = b"", {}, []
    for t in range(WINDOW - 8, WINDOW + 8):
        payload = len(blob) + 61
        wbase = payload & ~127
        first = filler(0, wbase + t - at - payload)
        recs = [first, second] + [record(2 + i, framed(7, b"x" * i), headers=tail[:i % 3]) for i in range(4)]
        b, r = batch(0, recs)
        where.append((payload + len(first) + at, wbase + t))
        raw[len(blob)] = r
        blob += b
    assert all(a == b for a, b in where) and all(blob[a:a + len(value)] == value for a, _ in where)
    return blob, raw, 16 * 6


def large_records():
    """values larger than a window, records of 8 KiB and more, a null value with headers, a key of the window's size"""
    hs = [(b"trace-id", b"0123456789abcdef"), (b"k" * 300, b""), (b"", None)]
    return [record(0, framed(42, b"v" * 5000), headers=hs),                        # larger than a window, two-byte length
            record(1, b"{" + b"j" * 9000, headers=hs[:1]),                         # 8 KiB and more: a three-byte length, the long way
            record(2, None, headers=hs),                                           # a null value followed by headers
            record(3, framed(43, b"w" * 70000), headers=hs * 5),
            record(4, framed(44), key=b"K" * 3100, headers=hs[:2]),                 # the value length lies behind the window
            record(5, b"x" * 3060, key=None), record(6, framed(45))]               # ... and a record that begins near a window's end

"""Blobs for the record-batch tests (test infrastructure): v2 batches from tests/kafka_format.py with every header field the
section reads under the test's control, and with the length of the encoder's own uncompressed record bytes kept beside each
batch — the inflated size the section must report, known by construction.  kafka_format fixes producerEpoch, baseSequence and
the leader epoch: patch() rewrites header fields in place and recomputes the CRC-32C."""
import struct

import kafka_format as K

CODECS = (None, "gzip", "snappy", "lz4", "zstd")   # codec numbers 0..4


def have_zstd():
    try:
        import pyarrow as pa
        return bool(pa.Codec.is_available("zstd"))
    except Exception:
        return False


def patch(batch, *, epoch=None, attributes=None, last_offset_delta=None, base_ts=None, max_ts=None, producer_id=None, count=None):
    """The batch with the given header fields replaced and its CRC recomputed (the leader epoch lies in front of the CRC's
    range, everything else inside it)."""
    b = bytearray(batch)
    f = list(struct.unpack_from(">hiqqqhii", b, 21))
    for i, x in ((0, attributes), (1, last_offset_delta), (2, base_ts), (3, max_ts), (4, producer_id), (7, count)):
        if x is not None:
            f[i] = x
    struct.pack_into(">hiqqqhii", b, 21, *f)
    if epoch is not None:
        struct.pack_into(">i", b, 12, epoch)
    struct.pack_into(">I", b, 17, K.crc32c(bytes(b[21:])))
    return bytes(b)


def batch(base_offset, n, base_ts, *, value_len=24, key=True, ts_step=1, attributes=0, max_ts=None, producer_id=-1, compression=None,
          last_offset_delta=None, epoch=0):
    """(bytes, raw) of one batch of n records: raw is the length of its uncompressed record bytes."""
    recs = b"".join(K.encode_record(i, i * ts_step, (b"k%d" % (i % 7)) if key else None, bytes((i + j) % 5 + 97 for j in range(value_len)))
                    for i in range(n))
    if max_ts is None:
        max_ts = base_ts + (n - 1) * ts_step if n else base_ts
    b = K.encode_batch(base_offset, [], base_ts, attributes=attributes, max_ts=max_ts, producer_id=producer_id, raw_records=recs,
                       count=n, compression=compression, last_offset_delta=last_offset_delta)
    return (patch(b, epoch=epoch) if epoch != 0 else b), len(recs)


def corrupt_stream(batch_bytes, compression):
    """The compressed batch with a stream that cannot inflate to what it announces, whatever its bytes are: gzip's ISIZE
    trailer and Snappy's length preamble one more than the stream produces (the device's inflate ends short of its slice),
    the LZ4 frame's and the zstd frame's magic number broken (the host's size probe refuses them).  The length stays."""
    b = bytearray(batch_bytes)
    if compression == "gzip":
        struct.pack_into("<I", b, len(b) - 4, struct.unpack_from("<I", b, len(b) - 4)[0] + 1)
    elif compression == "snappy":
        assert b[61] & 0x80 and not b[62] & 0x80 and b[61] & 0x7F != 0x7F      # a two-byte varint whose low digit has room
        b[61] += 1
    else:
        b[61] ^= 0xFF
    return bytes(b)


def join(batches):
    """[(bytes, raw)] -> (blob, [raw per batch])."""
    return b"".join(b for b, _ in batches), [r for _, r in batches]


def mixed(seed, n_batches, *, codecs=None, base_ts=1_600_000_000_000):
    """n_batches batches of 1..9 records with odd value sizes (so that byte_off takes every residue), the codecs, flags,
    producers, epochs and offset holes varied by a small deterministic rule."""
    codecs = [c for c in CODECS if c != "zstd" or have_zstd()] if codecs is None else codecs
    out, off = [], 0
    for i in range(n_batches):
        x = (i * 2654435761 + seed * 40503) & 0xFFFFFFFF
        n = 1 + x % 9
        attrs = (0x08 if x & 0x100 else 0) | (0x10 if x & 0x200 else 0)
        pid = -1 if x & 0x400 else (x >> 12) % 37
        lod = n - 1 + ((x >> 20) % 4 if x & 0x800 else 0)
        out.append(batch(off, n, base_ts + i * 10, value_len=1 + (x >> 3) % 29, ts_step=(x >> 5) % 3, attributes=attrs, producer_id=pid,
                         compression=codecs[i % len(codecs)], last_offset_delta=lod, epoch=(x >> 24) % 6 - 1))
        off += lod + 1
    return join(out)

"""Blobs for the tests of the value-byte section (test infrastructure), on top of payload_blobs.py: values of every length
around a dword, a 16-byte block and a window, values astride a window's end and at every alignment, every byte value at every
position of a dword, one byte in every lane at once, and equal neighbours astride every seam the kernel has."""
import payload_blobs as B

WINDOW = B.WINDOW
LENGTHS = (None, 0, 1, 2, 3, 4, 5, 15, 16, 17, 3071, 3072, 3073, 3 * 3072 + 1, 65539)


def plain(n, salt=0):
    """n bytes whose neighbours always differ (an odd step through the byte values)"""
    return bytes((7 * i + 3 + salt) & 0xFF for i in range(n))


def lengths(which=LENGTHS):
    """(blob, raw): a record for every value length of `which` (None: a null value), each also with a constant value and
    between short records, in batches of a few records; then all of them in one batch"""
    values = [None if n is None else plain(n, n) for n in which] + [bytes([n & 0xFF]) * n for n in which if n]
    out, off = [], 0
    for i, v in enumerate(values):
        recs = [B.record(0, b"ab"), B.record(1, v, key=b"k" * (i % 5)), B.record(2, b"cd", headers=[(b"h", b"v")])]
        out.append(B.batch(off, recs))
        off += 3
    out.append(B.batch(off, [B.record(i, v, key=None) for i, v in enumerate(values)]))
    return B.join(out)


def astride(span=16):
    """(blob, raw, where): batch by batch, the second record's VALUE is a `span`-byte marker whose first byte lies at offset
    3056 .. 3071 of the batch's first window: the window's end falls behind each of its bytes in turn.  where: the markers'
    positions in the blob."""
    marker = bytes(range(0x41, 0x41 + span))
    second = B.record(1, marker, key=b"key")
    at = second.index(marker)
    blob, raw, where = b"", {}, []
    for t in range(WINDOW - span, WINDOW):
        payload = len(blob) + 61
        wbase = payload & ~127
        first = B.filler(0, wbase + t - at - payload)
        recs = [first, second] + [B.record(2 + i, b"x" * i) for i in range(4)]
        b, r = B.batch(0, recs)
        where.append(payload + len(first) + at)
        raw[len(blob)] = r
        blob += b
        assert where[-1] == wbase + t and blob[where[-1]:where[-1] + span] == marker
    return blob, raw, where


def alignments():
    """(blob, raw, starts): values of 1 .. 40 bytes that begin at every position mod 16 of the blob (the key shifts them);
    starts: the residues seen"""
    recs, starts = [], set()
    pos = 61
    for i in range(64):
        r = B.record(i, plain(1 + i % 40, i), key=b"k" * (i % 7))
        starts.add((pos + len(r) - 1 - (1 + i % 40)) % 16)                  # (no headers: the record ends with the byte 0 behind its value)
        pos += len(r)
        recs.append(r)
    blob, raw = B.join([B.batch(0, recs)])
    return blob, raw, starts


def every_byte_at_every_position():
    """(blob, raw, residues): all 256 byte values once, in values that begin at the four positions mod 4 (residues: those
    seen); then the same behind a window's end"""
    recs, residues = [], set()
    pos = 61
    for i in range(8):
        r = B.record(i, bytes(range(256)), key=b"k" * (i % 5))
        residues.add((pos + len(r) - 1 - 256) % 4)
        pos += len(r)
        recs.append(r)
    big = [B.record(8 + i, plain(3100 + i, i) + bytes(range(256)), key=None) for i in range(4)]      # ... in the tail behind the window
    return B.join([B.batch(0, recs), B.batch(8, big)]) + (residues,)


def one_byte_in_every_lane(byte, n=40):
    """four batches of sixteen records whose values are `byte` alone: all 64 lanes add to one bin at once"""
    return B.join([B.batch(16 * g, [B.record(i, bytes([byte]) * (n + i), key=None) for i in range(16)]) for g in range(4)])


def seams():
    """(blob, raw, at): one value of 8 KiB whose neighbours differ but for a pair of equal bytes astride every seam (at: the
    positions in the blob of the pairs' second bytes): byte to
    byte inside a dword, dword to dword, the sixteenth lane's dword to the first lane's next one, the window's end, block to
    block and the sixteenth lane's block to the first lane's next one behind it.  The value begins in the batch's first window."""
    head = B.record(0, b"first", key=None)
    vstart = 61 + len(head) + len(B.record(1, b"v" * 8192, key=None)) - 1 - 8192
    wbase = 61 & ~127
    value = bytearray(plain(8192))
    at = []                                                                  # positions in the blob of a pair's second byte
    at += [vstart + 1, vstart + 2]                                           # the value's first bytes
    at += list(range(256, 256 + 136, 5))                                     # every residue mod 4, two lanes' turns in LDS
    at += [wbase + WINDOW - 1, wbase + WINDOW, wbase + WINDOW + 1]           # the window's last bytes, astride its end, the tail's first
    at += list(range(wbase + WINDOW + 30, wbase + WINDOW + 30 + 600, 7))     # every residue mod 16, two lanes' turns in the tail
    at += [vstart + 8191]                                                    # the value's last byte
    at = [p for p in sorted(set(at)) if vstart < p < vstart + 8192]
    for p in at:                                                             # (ascending: neighbouring seams make a run)
        value[p - vstart] = value[p - vstart - 1]
    recs = [head, B.record(1, bytes(value), key=None), B.record(2, b"last", key=None)]
    blob, raw = B.join([B.batch(0, recs)])
    assert blob[vstart:vstart + 8192] == bytes(value) and all(blob[p] == blob[p - 1] for p in at)
    return blob, raw, at


def neighbours_outside_the_value():
    """values whose first byte equals the byte in front of them — the length varint, behind the key's last byte — and the last
    byte of the record before them: neither is a repeat"""
    recs = [B.record(0, b"\x00x", key=b"kA"),                                 # ends with the byte 0 (no headers)
            B.record(1, b"\x02", key=b"kA"),                                  # the length varint of a one-byte value is 0x02
            B.record(2, b"Ab", key=b"kA"),                                    # the key's last byte, the varint between them
            B.record(3, b"\x00\x01", key=None),                               # the record before it ends with 0x00; a null key is the varint 0x01
            B.record(4, b"\x04\x04x", key=b"")]                               # the varint of three bytes is 0x06; one real repeat
    return B.join([B.batch(0, recs)])


def constant_and_alternating(n=500):
    """(blob, raw): constant values (repeats = bytes - values) and alternating ones (repeats = 0)"""
    const = [B.record(i, bytes([c]) * (n + i), key=None) for i, c in enumerate((0x00, 0xFF, 0x41))]
    alt = [B.record(3 + i, bytes([c, c ^ 0xFF]) * (n + i), key=None) for i, c in enumerate((0x00, 0x55))]
    return B.join([B.batch(0, const)]), B.join([B.batch(0, alt)])

"""The compression what-if's model compressor, restated in Python (test infrastructure): an independent reading of the rule in
include/kta_hip.h (above KTA_FLAG_COMPRESS_WHATIF) and csrc/kta_lz4_model.h — the frame, the block grammar, the match finder
that looks a table of 4096 positions up 64 positions at a time — and of the section's vector u64[8 P + 20]."""
import struct

import numpy as np

BLOCK = 65536
PW, CODECS, CW = 8, 5, 4
BATCHES, BLOCKS, STORED, RAW, NOW, MODEL, SEQUENCES, MATCH_BYTES = range(8)
CODEC_OF = {None: 0, "gzip": 1, "snappy": 2, "lz4": 3, "zstd": 4}
_P1, _P2, _P3, _P4, _P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393
_M = 0xFFFFFFFF


def words(P):
    return PW * P + CODECS * CW


def xxh32(data: bytes, seed=0) -> int:
    """xxHash32, the whole of it (the frame descriptor's HC is its second byte)."""
    rotl = lambda x, r: ((x << r) | (x >> (32 - r))) & _M
    n, i = len(data), 0
    if n >= 16:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed, (seed - _P1) & _M]
        while i + 16 <= n:
            for k in range(4):
                v[k] = (rotl((v[k] + struct.unpack_from("<I", data, i + 4 * k)[0] * _P2) & _M, 13) * _P1) & _M
            i += 16
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & _M
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while i + 4 <= n:
        h = (rotl((h + struct.unpack_from("<I", data, i)[0] * _P3) & _M, 17) * _P4) & _M
        i += 4
    while i < n:
        h = (rotl((h + data[i] * _P5) & _M, 11) * _P1) & _M
        i += 1
    h ^= h >> 15
    h = (h * _P2) & _M
    h ^= h >> 13
    h = (h * _P3) & _M
    return h ^ (h >> 16)


def ext(x):
    return 0 if x < 15 else 1 + (x - 15) // 255


def _ext_bytes(x):
    if x < 15:
        return b""
    x -= 15
    return b"\xff" * (x // 255) + bytes([x % 255])


def sequences(b: bytes):
    """The sequences of model(block): [(literal start, literal length, offset, match length)], the closing one with offset 0."""
    n, out, a = len(b), [], 0
    if n >= 13:
        u = np.frombuffer(b, np.uint8).astype(np.uint32)
        v = u[0:n - 3] | (u[1:n - 2] << 8) | (u[2:n - 1] << 16) | (u[3:n] << 24)                 # le32 at every position
        h = ((v.astype(np.uint64) * 2654435761) & _M) >> 20
        v, h = v.tolist(), h.tolist()
        table = [0] * 4096
        last, i = n - 12, 1
        while i <= last:
            stride = range(i, min(i + 63, last) + 1)
            cand = [table[h[p]] for p in stride]                      # the table as it stood before the stride
            q = i
            for p, c in zip(stride, cand):
                if p < q or not (c < p and v[c] == v[p]):
                    continue
                m = 0
                while p + m < n - 5 and b[c + m] == b[p + m]:
                    m += 1
                out.append((a, p - a, p - c, m))
                a = q = p + m
            for p in stride:
                table[h[p]] = max(table[h[p]], p)
            i = max(i + len(stride), q)
    out.append((a, n - a, 0, 0))
    return out


def block_cost(seqs):
    return sum(1 + ext(ll) + ll + (2 + ext(m - 4) if off else 0) for _, ll, off, m in seqs)


def block_bytes(b: bytes, seqs=None) -> bytes:
    out = bytearray()
    for a, ll, off, m in (sequences(b) if seqs is None else seqs):
        out.append((min(ll, 15) << 4) | (min(m - 4, 15) if off else 0))
        out += _ext_bytes(ll) + b[a:a + ll]
        if off:
            out += struct.pack("<H", off) + _ext_bytes(m - 4)
    return bytes(out)


def frame(data: bytes):
    """(the frame's bytes, [blocks, stored_blocks, sequences, match_bytes]) of one records section."""
    out = bytearray(b"\x04\x22\x4d\x18\x60\x40" + bytes([(xxh32(b"\x60\x40") >> 8) & 0xFF]))
    st = [0, 0, 0, 0]
    for pos in range(0, len(data), BLOCK):
        b = data[pos:pos + BLOCK]
        seqs = sequences(b)
        body = block_bytes(b, seqs)
        assert len(body) == block_cost(seqs)
        stored = len(body) >= len(b)
        out += struct.pack("<I", len(b) | 0x80000000) + b if stored else struct.pack("<I", len(body)) + body
        st[0] += 1
        st[1] += stored
        st[2] += len(seqs) - 1
        st[3] += sum(m for _, _, _, m in seqs)
    out += b"\x00\x00\x00\x00"
    return bytes(out), st


def frame_size(data: bytes) -> int:
    return len(frame(data)[0])


def restate(batches, P):
    """The vector of [(partition, codec name or None, batch_bytes, the records section inflated)]: those that count."""
    vec = np.zeros(words(P), np.uint64)
    for partition, codec, batch_bytes, raw in batches:
        if not 0 <= partition < P:
            continue
        f, (blocks, stored, seqs, mbytes) = frame(raw)
        add = [1, blocks, stored, len(raw), batch_bytes - 61, len(f), seqs, mbytes]
        for k, x in enumerate(add):
            vec[PW * partition + k] += np.uint64(x)
        c = PW * P + CW * CODEC_OF[codec]
        for k, x in enumerate((1, len(raw), batch_bytes - 61, len(f))):
            vec[c + k] += np.uint64(x)
    return vec


def identities(vec, P):
    parts = vec[:PW * P].reshape(P, PW).astype(object)
    codecs = vec[PW * P:].reshape(CODECS, CW).astype(object)
    topic = parts.sum(axis=0)
    yield "codec sums", list(codecs.sum(axis=0)) == [topic[BATCHES], topic[RAW], topic[NOW], topic[MODEL]]
    for w in parts:
        yield "stored <= blocks", w[STORED] <= w[BLOCKS]
        yield "match bytes <= raw", w[MATCH_BYTES] <= w[RAW]
        yield "model bound", w[MODEL] <= w[RAW] + 11 * w[BATCHES] + 4 * w[BLOCKS]
        yield "matches of four", w[MATCH_BYTES] >= 4 * w[SEQUENCES]

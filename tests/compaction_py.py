"""The compaction what-if (KTA_FLAG_COMPACTION, include/kta_hip.h) restated in numpy, independent of the library:
the FNV key hashes as tests/key_sketch_py.py computes them; for every hash the record with the largest sequence number
among the keyed records is the last writer; a replayed record survives when it IS its hash's last writer; the vector
u64[5 P + 6] from that, and the section kta-analyzer prints from the vector."""
import numpy as np

import key_sketch_py as KS

WORDS, GLOBALS = 5, 6
REPLAYED, UNKEYED, UNKNOWN, LIVE_OUTSIDE, TOMBSTONES_OUTSIDE = range(5)
TITLE = "Compaction what-if: the records and bytes log compaction would keep (kta.compaction=1; not part of the reference report)\n"
NOTE = 'Keys are counted by 32-bit hash slot, topic-wide, as "Alive keys" is: a key written to several partitions is kept once.\n'


def words(P):
    return WORDS * P + GLOBALS


def hashes(cols) -> np.ndarray:
    return KS.fnv_columns(cols["key_len"], cols["key_off"], cols["key_bytes"])


def last_writers(cols, seq, h=None):
    """What the first pass leaves: (slots, seq of the slot's last writer, its alive bit), the slots ascending."""
    h = hashes(cols) if h is None else np.asarray(h)
    keyed = np.asarray(cols["key_len"]) >= 0
    hh, s = h[keyed].astype(np.uint64), np.asarray(seq, np.uint64)[keyed]
    alive = np.asarray(cols["val_len"])[keyed] >= 0
    order = np.lexsort((s, hh))
    hh, s, alive = hh[order], s[order], alive[order]
    last = np.ones(len(hh), bool)
    last[:-1] = hh[1:] != hh[:-1]
    return hh[last], s[last], alive[last]


def survivors(cols, seq, table, h=None):
    """Per replayed record: +1 it is its slot's last writer, 0 superseded, -1 the table never saw it; keyed records only
    (an unkeyed record: 0)."""
    slots, wseq, walive = table
    h = (hashes(cols) if h is None else np.asarray(h)).astype(np.uint64)
    seq = np.asarray(seq, np.uint64)
    alive = np.asarray(cols["val_len"]) >= 0
    at = np.searchsorted(slots, h)
    found = (at < len(slots))
    found[found] = slots[at[found]] == h[found]
    at = np.where(found, at, 0)
    ws = np.where(found, wseq[at] if len(slots) else 0, 0).astype(np.uint64)
    wa = np.where(found, walive[at] if len(slots) else False, False)
    out = np.zeros(len(h), np.int64)
    same = found & (ws == seq) & (wa == alive)
    # the order of (seq, alive) pairs is the order of ((seq + 1) << 1) | alive
    newer = ~found | (ws < seq) | ((ws == seq) & ~wa & alive)
    out[same] = 1
    out[newer] = -1
    out[np.asarray(cols["key_len"]) < 0] = 0
    return out


def vector(cols, P, seq=None, table=None, h=None) -> np.ndarray:
    """The compaction vector of a replay of `cols` with the sequence numbers `seq` (None: 0, 1, 2, ...) against `table`
    (None: what a first pass over the very same records leaves)."""
    n = len(cols["partition"])
    seq = np.arange(n, dtype=np.uint64) if seq is None else np.asarray(seq, np.uint64)
    h = hashes(cols) if h is None else h
    table = last_writers(cols, seq, h) if table is None else table
    part = np.asarray(cols["partition"], np.int64)
    kl = np.asarray(cols["key_len"], np.int64)
    vl = np.asarray(cols["val_len"], np.int64)
    k = survivors(cols, seq, table, h)
    inside = (part >= 0) & (part < P)
    live, tomb = (k == 1) & (vl >= 0), (k == 1) & (vl < 0)
    v = np.zeros(words(P), np.uint64)
    for word, mask, weight in ((0, live, None), (1, live, kl), (2, live, vl), (3, tomb, None), (4, tomb, kl)):
        m = mask & inside
        s = np.bincount(part[m], weights=None, minlength=P) if weight is None else _sum_by(part[m], weight[m], P)
        v[word:WORDS * P:WORDS] = s.astype(np.uint64)
    g = v[WORDS * P:]
    g[REPLAYED] = n
    g[UNKEYED] = int((kl < 0).sum())
    g[UNKNOWN] = int((k == -1).sum())
    g[LIVE_OUTSIDE] = int((live & ~inside).sum())
    g[TOMBSTONES_OUTSIDE] = int((tomb & ~inside).sum())
    return v


def _sum_by(part, weight, P):
    out = np.zeros(P, np.int64)          # (integers: bincount's weights are doubles)
    np.add.at(out, part, weight)
    return out


def brute_force(cols, P, seq=None) -> np.ndarray:
    """The same by a dict loop over the records, twice."""
    n = len(cols["partition"])
    seq = list(range(n)) if seq is None else [int(x) for x in seq]
    kb = np.asarray(cols["key_bytes"], np.uint8).tobytes()
    keys = []
    for i in range(n):
        kl = int(cols["key_len"][i])
        keys.append(None if kl < 0 else KS.fnv1a(kb[int(cols["key_off"][i]):int(cols["key_off"][i]) + kl]))
    table = {}
    for i in range(n):
        if keys[i] is None:
            continue
        val = ((seq[i] + 1) << 1) | (1 if int(cols["val_len"][i]) >= 0 else 0)
        if val > table.get(keys[i], 0):
            table[keys[i]] = val
    v = [0] * words(P)
    for i in range(n):
        v[WORDS * P + REPLAYED] += 1
        if keys[i] is None:
            v[WORDS * P + UNKEYED] += 1
            continue
        vl, kl, p = int(cols["val_len"][i]), int(cols["key_len"][i]), int(cols["partition"][i])
        val = ((seq[i] + 1) << 1) | (1 if vl >= 0 else 0)
        entry = table.get(keys[i], 0)
        if entry > val:
            continue
        if entry < val:
            v[WORDS * P + UNKNOWN] += 1
        elif not 0 <= p < P:
            v[WORDS * P + (LIVE_OUTSIDE if vl >= 0 else TOMBSTONES_OUTSIDE)] += 1
        elif vl >= 0:
            v[WORDS * p] += 1
            v[WORDS * p + 1] += kl
            v[WORDS * p + 2] += vl
        else:
            v[WORDS * p + 3] += 1
            v[WORDS * p + 4] += kl
    return np.array(v, np.uint64)


def split(vec, P):
    v = np.asarray(vec, np.uint64).reshape(-1)
    assert len(v) == words(P)
    d = {name: v[k:WORDS * P:WORDS] for k, name in enumerate(("live_records", "live_key_bytes", "live_value_bytes",
                                                               "tombstone_records", "tombstone_key_bytes"))}
    d.update({name: int(v[WORDS * P + k]) for k, name in enumerate(("replayed", "unkeyed", "unknown", "live_outside",
                                                                    "tombstones_outside"))})
    return d


def counters(cols, P) -> np.ndarray:
    """The counter vector's words the section reads (u64[P * 7 + 8], the rest zero): total_messages, key_size_sum,
    value_size_sum per partition, and the globals bad-partition records and records."""
    part = np.asarray(cols["partition"], np.int64)
    kl = np.maximum(np.asarray(cols["key_len"], np.int64), 0)
    vl = np.maximum(np.asarray(cols["val_len"], np.int64), 0)
    inside = (part >= 0) & (part < P)
    c = np.zeros(P * 7 + 8, np.uint64)
    c[0:7 * P:7] = np.bincount(part[inside], minlength=P).astype(np.uint64)
    c[5:7 * P:7] = _sum_by(part[inside], kl[inside], P).astype(np.uint64)
    c[6:7 * P:7] = _sum_by(part[inside], vl[inside], P).astype(np.uint64)
    c[7 * P + 0] = int((~inside).sum())
    c[7 * P + 2] = int(inside.sum())
    return c


def _table(rows):
    w = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    sep = "+" + "+".join("-" * (x + 2) for x in w) + "+\n"
    out = sep
    for r in rows:
        out += "|" + "|".join(" " + c.ljust(x) + " " for c, x in zip(r, w)) + "|\n" + sep
    return out


def matched(vec, counter_vec, P) -> bool:
    v = [int(x) for x in np.asarray(vec, np.uint64).reshape(-1)]
    c = [int(x) for x in np.asarray(counter_vec, np.uint64).reshape(-1)]
    return v[WORDS * P + UNKNOWN] == 0 and v[WORDS * P + REPLAYED] == c[7 * P + 0] + c[7 * P + 2]


def section(vec, counter_vec, P) -> str:
    v = [int(x) for x in np.asarray(vec, np.uint64).reshape(-1)]
    c = [int(x) for x in np.asarray(counter_vec, np.uint64).reshape(-1)]
    assert len(v) == words(P) and len(c) == P * 7 + 8
    g = v[WORDS * P:]
    shown = c[7 * P + 0] + c[7 * P + 2]
    if not matched(vec, counter_vec, P):
        return (TITLE + "The replay did not match the first pass: replayed %d of %d records, %d of them unknown to the table. "
                "Nothing is reported.\n" % (g[REPLAYED], shown, g[UNKNOWN]) + "=" * 120 + "\n")

    def reclaimed(kept, now):
        return "n/a" if now == 0 else "%.2f" % ((now - kept) * 100.0 / now)

    rows = [["P", "Records", "Kept", "Live", "Tombstones", "Records reclaimed %", "Bytes", "Bytes kept", "Bytes reclaimed %"]]
    tot = [0] * 5
    for p in range(P):
        live, lk, lv, tomb, tk = v[WORDS * p:WORDS * p + 5]
        rec, size = c[7 * p], c[7 * p + 5] + c[7 * p + 6]
        kept_bytes = lk + lv + tk
        rows.append([str(p), str(rec), str(live + tomb), str(live), str(tomb), reclaimed(live + tomb, rec), str(size), str(kept_bytes),
                     reclaimed(kept_bytes, size)])
        tot = [a + b for a, b in zip(tot, (rec, live, tomb, size, kept_bytes))]
    rec, live, tomb, size, kept_bytes = tot
    rows.append(["Topic", str(rec), str(live + tomb), str(live), str(tomb), reclaimed(live + tomb, rec), str(size), str(kept_bytes),
                 reclaimed(kept_bytes, size)])
    out = TITLE + _table(rows) + "Records without a key: %d (not kept: compaction goes by key)\n" % g[UNKEYED]
    if g[LIVE_OUTSIDE] or g[TOMBSTONES_OUTSIDE]:
        out += "Kept outside the partition range: %d live, %d tombstones\n" % (g[LIVE_OUTSIDE], g[TOMBSTONES_OUTSIDE])
    return out + NOTE + "=" * 120 + "\n"

"""Independent restatement of the timestamp-order pass (KTA_FLAG_TS_ORDER), written from the definition in
include/kta_hip.h: the sequential loop with a carried `hi`, so that batches can be fed one after another; the merge; and
the text of the kta.ts_order section."""
import numpy as np

HIST = 63
U64 = (1 << 64) - 1


def words(P):
    return 3 * P + 64


class TsOrder:
    """One context's state: hi[p] (None: none) and the vector's parts as Python integers."""

    def __init__(self, P):
        self.P = P
        self.reset()

    def reset(self):
        P = self.P
        self.hi = [None] * P
        self.late, self.late_ms_sum, self.max_late_ms = [0] * P, [0] * P, [0] * P
        self.hist = [0] * HIST
        self.timed = 0

    def feed(self, partition, ts_ms):
        """Records in consumption order (the metrics handler's: which & 1).  Returns self."""
        part = np.asarray(partition, np.int64)
        ts = np.asarray(ts_ms, np.int64)
        ok = (part >= 0) & (part < self.P) & (ts >= 0)
        self.timed += int(ok.sum())
        # per partition the order is the stream's: a stable sort by partition keeps it, and the definition's loop over one
        # partition's records is a running maximum (hi only ever rises: it is set to ts exactly when ts >= hi)
        part, ts = part[ok], ts[ok]
        order = np.argsort(part, kind="stable")
        part, ts = part[order], ts[order]
        cuts = np.searchsorted(part, np.arange(self.P + 1))
        pow2 = np.uint64(1) << np.arange(HIST, dtype=np.uint64)
        for p in range(self.P):
            t = ts[cuts[p]:cuts[p + 1]]
            if not len(t):
                continue
            seed = -1 if self.hi[p] is None else self.hi[p]
            incl = np.maximum.accumulate(np.concatenate([np.array([seed], np.int64), t]))
            prev = incl[:-1]
            late = prev > t
            self.hi[p] = int(incl[-1])
            if late.any():
                d = prev[late].astype(np.uint64) - t[late].astype(np.uint64)      # 1 <= d < 2^63
                self.late[p] += int(late.sum())
                self.late_ms_sum[p] = (self.late_ms_sum[p] + int(np.add.reduce(d))) & U64      # (numpy wraps, as the sum does)
                self.max_late_ms[p] = max(self.max_late_ms[p], int(d.max()))
                k = np.searchsorted(pow2, d, side="right") - 1                      # floor(log2 d)
                for b, c in zip(*np.unique(k, return_counts=True)):
                    self.hist[int(b)] += int(c)
        return self

    def feed_loop(self, partition, ts_ms):
        """The definition's loop, record by record (small inputs: it checks feed())."""
        for p, ts in zip(partition, ts_ms):
            p, ts = int(p), int(ts)
            if not (0 <= p < self.P) or ts < 0:
                continue
            self.timed += 1
            if self.hi[p] is not None and self.hi[p] > ts:
                d = self.hi[p] - ts
                self.late[p] += 1
                self.late_ms_sum[p] = (self.late_ms_sum[p] + d) & U64
                self.max_late_ms[p] = max(self.max_late_ms[p], d)
                self.hist[d.bit_length() - 1] += 1
            else:
                self.hi[p] = ts
        return self

    def vector(self):
        P = self.P
        v = np.zeros(words(P), np.uint64)
        v[0:2 * P:2] = np.array(self.late, np.uint64)
        v[1:2 * P:2] = np.array(self.late_ms_sum, np.uint64)
        v[2 * P:2 * P + HIST] = np.array(self.hist, np.uint64)
        v[2 * P + HIST] = self.timed
        v[2 * P + 64:] = np.array(self.max_late_ms, np.uint64)
        return v


def vector_of(P, partition, ts_ms):
    return TsOrder(P).feed(partition, ts_ms).vector()


def merge(a, b, P):
    """SUM over the first 2 P + 64 words (mod 2^64), signed MAX over the last P."""
    a, b = np.asarray(a, np.uint64).copy(), np.asarray(b, np.uint64)
    s = 2 * P + 64
    a[:s] = a[:s] + b[:s]                       # (numpy wraps)
    a[s:] = np.maximum(a[s:].view(np.int64), b[s:].view(np.int64)).view(np.uint64)
    return a


TITLE = ("Timestamp order: records older than one their partition delivered before them (kta.ts_order=1; not part of the "
         "reference report)\n")


def _table(rows):
    w = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    sep = "+" + "+".join("-" * (x + 2) for x in w) + "+\n"
    out = sep
    for r in rows:
        out += "|" + "|".join(" " + c.ljust(x) + " " for c, x in zip(r, w)) + "|\n" + sep
    return out


def section(vec, records) -> str:
    """The kta.ts_order section: vec u64[3 P + 64], records[p] = total_messages of partition p."""
    P = len(records)
    v = [int(x) for x in np.asarray(vec, np.uint64).reshape(-1)]
    assert len(v) == words(P)
    late, sums = v[0:2 * P:2], v[1:2 * P:2]
    hist, timed, most = v[2 * P:2 * P + HIST], v[2 * P + HIST], v[2 * P + 64:]
    records = [int(r) for r in records]

    def pct(c, of):
        return "%.2f" % (float(c) * 100.0 / float(of) if of else 0.0)

    rows = [["P", "Records", "Late records", "Late %", "Mean lateness ms", "Max lateness ms"]]
    for p in range(P):
        rows.append([str(p), str(records[p]), str(late[p]), pct(late[p], records[p]),
                     str(sums[p] // late[p]) if late[p] else "-", str(most[p]) if late[p] else "-"])
    total, late_all, sum_all = sum(records) & U64, sum(late) & U64, sum(sums) & U64
    rows.append(["Topic", str(total), str(late_all), pct(late_all, total), str(sum_all // late_all) if late_all else "-",
                 str(max(most)) if late_all else "-"])
    out = TITLE + _table(rows)
    out += "Records without a timestamp: %d\n" % ((total - timed) & U64)
    full = [k for k in range(HIST) if hist[k]]
    if not full:
        out += "No record is late.\n"
    else:
        rows = [["Late by", "Records", "Cumulative %"]]
        within = (timed - late_all) & U64
        for k in range(full[0], full[-1] + 1):
            within = (within + hist[k]) & U64
            rows.append(["< %d ms" % (2 << k), str(hist[k]), pct(within, timed)])
        out += _table(rows)
    return out + "=" * 120 + "\n"

"""Independent Python restatement of the additive analytics (KTA_FLAG_ANALYTICS; no reference counterpart):
the analytics vector of a set of records (numpy), its decode, and the section kta-analyzer prints after the
report with --librdkafka kta.analytics=1.  Dates and tables come from the restatement of the reference
report (oracle/oracle_py.py), so the section is written with the report's own formatting."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import oracle_py as OP  # noqa: E402

HIST = 2 * 34
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
U64_MAX = np.iinfo(np.uint64).max


def size_bucket(lengths):
    """[0] None (-1), [1] length 0, [2 + k] 2^k <= length < 2^(k+1)."""
    x = np.asarray(lengths, np.int64)
    b = np.zeros(x.shape, np.int64)
    pos = x > 0
    b[x == 0] = 1
    b[pos] = 2 + np.floor(np.log2(x[pos].astype(np.float64))).astype(np.int64)
    # float log2 is exact at powers of two and monotone; correct the rare rounding just below one
    lo = np.left_shift(np.int64(1), np.maximum(b[pos] - 2, 0))
    b[pos] -= (x[pos] < lo).astype(np.int64)
    return b


def analytics_vector(cols, P):
    """u64[2*34 + 4*P] of the records `cols` (partition, key_len, val_len, ts_ms), in the device layout:
    histograms, then per partition [~min ts_ms, max ts_ms, ~smallest, largest] as int64, INT64_MIN if unwritten."""
    v = np.zeros(HIST + 4 * P, np.int64)
    part = np.asarray(cols["partition"], np.int64)
    kl, vl = np.asarray(cols["key_len"], np.int64), np.asarray(cols["val_len"], np.int64)
    ts = np.asarray(cols["ts_ms"], np.int64)
    ts = np.where(ts == -1, 0, ts)
    v[:34] = np.bincount(size_bucket(kl), minlength=34)
    v[34:HIST] = np.bincount(size_bucket(vl), minlength=34)
    x = np.full((P, 4), I64_MIN, np.int64)
    for p in np.unique(part):
        m = part == p
        x[p, 0] = ~int(ts[m].min())
        x[p, 1] = int(ts[m].max())
        live = m & (vl >= 0)
        if live.any():
            sz = np.maximum(kl[live], 0) + vl[live]
            x[p, 2] = ~int(sz.min())
            x[p, 3] = int(sz.max())
    v[HIST:] = x.ravel()
    return v.view(np.uint64)


def merge(a, b, P):
    """SUM over the histograms, signed MAX over the extrema."""
    out = np.asarray(a, np.uint64).copy()
    out[:HIST] += np.asarray(b, np.uint64)[:HIST]
    out[HIST:] = np.maximum(out[HIST:].view(np.int64), np.asarray(b, np.uint64)[HIST:].view(np.int64)).view(np.uint64)
    return out


def _trunc1000(ms):
    return -((-ms) // 1000) if ms < 0 else ms // 1000


def decode(vec, P):
    """The dict HipMetricHandler.analytics() returns, from a vector."""
    v = np.asarray(vec, np.uint64)
    x = v[HIST:].view(np.int64).reshape(P, 4)
    out = {"key_size_hist": v[:34].copy(), "value_size_hist": v[34:HIST].copy(),
           "part_min_ts_sec": np.zeros(P, np.int64), "part_max_ts_sec": np.zeros(P, np.int64),
           "part_smallest": np.zeros(P, np.uint64), "part_largest": np.zeros(P, np.uint64)}
    for p in range(P):
        seen, live = x[p, 1] != I64_MIN, x[p, 3] != I64_MIN
        out["part_min_ts_sec"][p] = _trunc1000(int(~x[p, 0])) if seen else I64_MAX
        out["part_max_ts_sec"][p] = _trunc1000(int(x[p, 1])) if seen else I64_MIN
        out["part_smallest"][p] = int(~x[p, 2]) if live else U64_MAX
        out["part_largest"][p] = int(x[p, 3]) if live else 0
    return out


def bucket_label(b):
    if b == 0:
        return "None"
    if b == 1:
        return "0"
    if b == 2:
        return "1"
    return "%d-%d" % (1 << (b - 2), (1 << (b - 1)) - 1)


def section(a):
    """The section kta-analyzer prints after the reference report's closing rule, from a decoded dict."""
    kh, vh = [int(x) for x in a["key_size_hist"]], [int(x) for x in a["value_size_hist"]]
    records = sum(kh)
    pct = lambda c: "%.2f" % (c * 100.0 / records if records else 0.0)
    out = "Size histograms and per-partition extrema (kta.analytics=1; not part of the reference report)\n"
    rows = [["Bytes", "Keys", "Keys %", "Values", "Vals %"]]
    for b in range(34):
        if b < 2 or kh[b] or vh[b]:
            rows.append([bucket_label(b), str(kh[b]), pct(kh[b]), str(vh[b]), pct(vh[b])])
    out += OP.prettytable(rows) + "\n"
    rows = [["P", "Earliest", "Latest", "Smallest", "Largest"]]
    for p in range(len(a["part_min_ts_sec"])):
        seen = int(a["part_max_ts_sec"][p]) != I64_MIN
        live = int(a["part_smallest"][p]) != int(U64_MAX) or int(a["part_largest"][p]) != 0
        rows.append([str(p),
                     OP.format_datetime_utc(int(a["part_min_ts_sec"][p]), 0) if seen else "-",
                     OP.format_datetime_utc(int(a["part_max_ts_sec"][p]), 0) if seen else "-",
                     str(int(a["part_smallest"][p])) if live else "-",
                     str(int(a["part_largest"][p])) if live else "-"])
    out += OP.prettytable(rows)
    return out + "=" * 120 + "\n"

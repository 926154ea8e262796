"""Independent Python restatement of the timeline (kta_set_timeline; no reference counterpart): the timeline vector of a
set of records (numpy, exact integer floor division), the host-side merge, and the section kta-analyzer prints after
the report with --librdkafka kta.timeline=<width>.  Dates and tables come from the restatement of the reference report
(oracle/oracle_py.py), so the section is written with the report's own formatting."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import oracle_py as OP  # noqa: E402

COLS = 3
MAX_BUCKETS = 1024


def timeline_vector(cols, P, origin_ms, bucket_ms, n_buckets):
    """np.uint64[n_buckets + 3, 3] of the records `cols` (partition, key_len, val_len, ts_ms): rows [no timestamp,
    before, bucket 0 .. n-1, after] of [records, tombstones, bytes]; records outside [0, P) are left out."""
    part = np.asarray(cols["partition"], np.int64)
    kl, vl = np.asarray(cols["key_len"], np.int64), np.asarray(cols["val_len"], np.int64)
    ts = np.asarray(cols["ts_ms"], np.int64)
    ok = (part >= 0) & (part < P)
    kl, vl, ts = kl[ok], vl[ok], ts[ok]
    row = np.empty(ts.shape, np.int64)
    row[ts < 0] = 0
    row[(ts >= 0) & (ts < origin_ms)] = 1
    inside = ts >= origin_ms
    k = (ts[inside] - np.int64(origin_ms)) // np.int64(bucket_ms)     # ts >= origin >= 0: no overflow
    row[inside] = np.where(k >= n_buckets, n_buckets + 2, 2 + np.minimum(k, n_buckets - 1))
    rows = n_buckets + 3
    out = np.zeros((rows, COLS), np.uint64)
    out[:, 0] = np.bincount(row, minlength=rows).astype(np.uint64)
    out[:, 1] = np.bincount(row[vl == -1], minlength=rows).astype(np.uint64)
    # bytes < 2^32 per record, summed exactly in two 16-bit halves (float64 weights are exact below 2^53: < 2^37 records)
    by = np.maximum(kl, 0) + np.maximum(vl, 0)
    lo = np.bincount(row, weights=(by & 0xFFFF).astype(np.float64), minlength=rows).astype(np.uint64)
    hi = np.bincount(row, weights=(by >> 16).astype(np.float64), minlength=rows).astype(np.uint64)
    out[:, 2] = lo + (hi << np.uint64(16))
    return out


def merge(a, b):
    """Every word is a SUM."""
    return np.asarray(a, np.uint64) + np.asarray(b, np.uint64)


def width_label(w):
    for ms, unit in ((86400000, "d"), (3600000, "h"), (60000, "m"), (1000, "s")):
        if w % ms == 0:
            return "%d%s" % (w // ms, unit)
    return "%dms" % w


def ms_utc(ms):
    return OP.format_datetime_utc(ms // 1000, (ms % 1000) * 1000000)


def section(vec, origin_ms, bucket_ms, n_buckets):
    """The section kta-analyzer prints after the reference report (and the analytics section)."""
    v = [[int(x) for x in r] for r in np.asarray(vec, np.uint64).reshape(n_buckets + 3, COLS)]
    records = sum(r[0] for r in v)
    pct = lambda c: "%.2f" % (c * 100.0 / records if records else 0.0)
    start = ms_utc(origin_ms)
    out = "Timeline, %s buckets from %s (kta.timeline; not part of the reference report)\n" % (width_label(bucket_ms), start)
    rows = [["From", "Records", "Records %", "Tmb", "Bytes"]]
    row = lambda label, r: rows.append([label, str(v[r][0]), pct(v[r][0]), str(v[r][1]), str(v[r][2])])
    row("No timestamp", 0)
    row("Before " + start, 1)
    used = [k for k in range(n_buckets) if v[2 + k][0]]
    if used:
        for k in range(used[0], used[-1] + 1):
            row(ms_utc(origin_ms + k * bucket_ms), 2 + k)
    row("After " + ms_utc(origin_ms + n_buckets * bucket_ms), n_buckets + 2)
    out += OP.prettytable(rows)
    return out + "=" * 120 + "\n"

"""kafka_topic_analyzer_amd — MI355X (gfx950) implementation of kafka-topic-analyzer's per-record
metric-accumulation hot path (reference: /root/reference/src/metric.rs, src/fnv32.rs).

This Python layer is a thin ctypes mirror of the C ABI (include/kta_hip.h) used by the tests and
by bench.py.  Names follow the reference:

    HipMetricHandler                 one `MetricHandler` (kafka.rs:18-20) that feeds both reference
                                     handlers' state on the GPU
    MessageMetrics                   accessor view == metric.rs:104-195
    LogCompactionInMemoryMetrics     accessor view == metric.rs:282-284

All arithmetic happens in libkta_hip.so's HIP kernels; nothing here (or anywhere in this package)
computes metrics on the CPU, and importing works without a GPU but creating a handler does not.
"""
from __future__ import annotations

import ctypes as C
import time
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import _native as N
from ._native import KtaBatch, KtaConfig, KtaResult, KtaSynthSpec  # noqa: F401

__all__ = ["HipMetricHandler", "MessageMetrics", "LogCompactionInMemoryMetrics", "Message", "KtaError",
           "DivideByZeroPanic", "DateTimeRangePanic", "synth_preset", "synth_fill_host", "fnv_reference_kats",
           "decode_analytics", "merge_analytics", "render_analytics", "analytics_max_partitions", "render_timeline",
           "timeline_max_partitions", "estimate_distinct_keys", "merge_key_sketch", "render_distinct_keys",
           "recover_hot_keys", "merge_hot_keys", "render_hot_keys", "render_ts_order", "merge_ts_order",
           "ts_order_max_partitions", "split_ts_order", "render_partitioner", "merge_partitioner",
           "partitioner_max_partitions", "split_partitioner", "murmur2", "render_compaction", "split_compaction",
           "compaction_max_partitions", "split_size_quantiles", "merge_size_quantiles", "render_size_percentiles", "size_bin",
           "size_bin_bounds", "size_quantile", "size_quantiles_max_partitions", "segments_words", "segments_max_partitions",
           "split_segments", "merge_segments", "retention_whatif", "RETENTION_COLUMNS", "render_retention",
           "compact_delete_max_partitions", "split_compact_delete", "compact_delete_whatif", "COMPACT_DELETE_COLUMNS",
           "render_compact_delete", "split_record_batches", "merge_record_batches", "render_record_batches", "estimate_producers",
           "record_batches_identities", "record_batches_host", "RECORD_BATCH_COLUMNS", "RECORD_BATCH_CODECS", "split_payload", "merge_payload",
           "payload_identities", "payload_schema_ids", "payload_host", "render_payload", "PAYLOAD_COLUMNS", "PAYLOAD_CLASSES",
           "split_header_names", "merge_header_names", "header_names_identities", "header_names_list", "header_names_host",
           "render_header_names", "HEADER_NAME_DTYPE", "HEADER_NAMES_GLOBALS", "split_value_bytes", "merge_value_bytes",
           "value_bytes_identities", "value_bytes_summary", "value_bytes_host", "render_value_bytes", "VALUE_BYTES_CLASSES",
           "split_compress_whatif", "merge_compress_whatif", "compress_whatif_identities", "compress_whatif_host", "render_compress_whatif",
           "lz4_model", "lz4_model_size", "COMPRESS_WHATIF_COLUMNS", "COMPRESS_WHATIF_CODECS", "COMPRESS_WHATIF_CODEC_COLUMNS"]

U64_MAX = 0xFFFFFFFFFFFFFFFF


class KtaError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libkta_hip error {code}: {msg}")
        self.code = code


class DivideByZeroPanic(ZeroDivisionError):
    """Where the reference panics with 'attempt to divide by zero' (metric.rs:135,144,153)."""


class DateTimeRangePanic(KtaError):
    """Where the reference panics with 'invalid or out-of-range datetime' (NaiveDateTime::from_timestamp,
    metric.rs:210 / kafka.rs:104): a record's ts / 1000 outside chrono 0.4.19's range.  The library has counted
    the record; kta_finish reports it with KTA_ERR_TIMESTAMP_RANGE."""


class Message(NamedTuple):
    """What the reference handlers read from a BorrowedMessage (metric.rs:208-209,218,233)."""
    partition: int
    timestamp_ms: Optional[int]   # None == Timestamp::to_millis() None
    key: Optional[bytes]          # None == m.key() None
    payload_len: Optional[int]    # None == m.payload() None; the bytes are never read


def _np_ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


def _host_batch(cols: dict) -> KtaBatch:
    """A raw-layout kta_batch over contiguous numpy metric columns (the arrays must outlive its use)."""
    hb = KtaBatch()
    for name in ("partition", "key_len", "val_len", "ts_ms"):
        setattr(hb, name, cols[name].ctypes.data)
    return hb


# Every section's result vector, said once: the u64 words by the section's shape (P; Q, M or n_buckets where it has one) and
# what a length error calls a vector of that shape.  The handler's read-backs, the split_* / render_* / merge_* functions
# and the what-ifs all size and check their vectors here.
_SECTIONS = {
    "counters": (lambda P: P * N.KTA_NCOUNTERS + N.KTA_NGLOBALS, "a counter vector of {} partitions"),
    "analytics": (lambda P: N.KTA_ANALYTICS_HIST + 4 * P, "an analytics vector of {} partitions"),
    "timeline": (lambda n_buckets: (n_buckets + 3) * N.KTA_TIMELINE_COLS, "a timeline of {} buckets"),
    "key_sketch": (lambda P: P * N.KTA_SKETCH_REGISTERS, "a key sketch of {} partitions"),
    "hot_keys": (lambda: N.KTA_HOT_VECTOR_WORDS, "a hot-key vector"),
    "ts_order": (lambda P: 3 * P + 64, "a timestamp-order vector of {} partitions"),
    "partitioner": (lambda P, Q: 2 * P + 2 * Q, "a partitioner vector of {} partitions and {} targets"),
    "size_quantiles": (lambda P: P * N.KTA_SIZE_QUANTITIES * N.KTA_SIZE_BINS + N.KTA_SIZE_GLOBALS, "a size vector of {} partitions"),
    "segments": (lambda P, M: segments_words(P, M), "a segment vector of {} partitions and {} rows"),
    "record_batches": (lambda P: 20 * P + 1524, "a record-batch vector of {} partitions"),
    "payload": (lambda P: 24 * P + 16 + 2 * 1024 * 34, "a payload vector of {} partitions"),
    "header_names": (lambda: N.KTA_HEADER_NAMES_WORDS, "a header-name vector"),
    "value_bytes": (lambda P: N.KTA_VALUE_BYTES_PARTITION_WORDS * P, "a value-byte vector of {} partitions"),
    "compress_whatif": (lambda P: N.KTA_COMPRESS_WHATIF_PARTITION_WORDS * P + N.KTA_COMPRESS_WHATIF_CODECS * N.KTA_COMPRESS_WHATIF_CODEC_WORDS,
                        "a compression what-if vector of {} partitions"),
    "compaction": (lambda P: N.KTA_COMPACTION_WORDS * P + N.KTA_COMPACTION_GLOBALS, "a compaction vector of {} partitions"),
    "compact_delete": (lambda P, M: segments_words(P, M), "a kept vector of {} partitions and {} rows"),
}


def _section_words(name: str, *shape) -> int:
    return _SECTIONS[name][0](*shape)


def _u64_vec(vec, words: int, what: str) -> np.ndarray:
    """`vec` flat, contiguous and as uint64 (an int64 array is viewed, not converted: a merge works in place on it), with
    `words` words; `what` names the vector in the ValueError."""
    a = np.ascontiguousarray(np.asarray(vec).reshape(-1))
    v = a.view(np.uint64) if a.dtype == np.int64 else np.ascontiguousarray(a, np.uint64)
    if v.size != words:
        raise ValueError(f"{what} has {words} words, not {v.size}")
    return v


def _section_vec(name: str, vec, *shape) -> np.ndarray:
    return _u64_vec(vec, _section_words(name, *shape), _SECTIONS[name][1].format(*shape))


def _counter_vec(vec, P: int) -> np.ndarray:
    """The counter vector u64[P * 7 + 8] a render_* function takes beside its section's."""
    c = np.ascontiguousarray(np.asarray(vec).reshape(-1)).view(np.uint64)
    if c.size != _section_words("counters", P):
        raise ValueError(f"a counter vector of {P} partitions has {_section_words('counters', P)} words")
    return c


def _merge(name: str, acc: np.ndarray, other, *shape) -> np.ndarray:
    """kta_merge_<name>(acc, other, *shape), in place on `acc` (contiguous uint64 / int64)."""
    if acc.dtype not in (np.uint64, np.int64) or not acc.flags.c_contiguous:
        raise TypeError("acc must be a contiguous uint64 / int64 array")
    rc = getattr(N.load(), "kta_merge_" + name)(_np_ptr(_section_vec(name, acc, *shape)), _np_ptr(_section_vec(name, other, *shape)), *shape)
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_merge_" + name)
    return acc


# the words every kta_*_info of a pass of the decode call begins with (HipMetricHandler._pass_info)
_PASS_INFO_KEYS = ("launches", "batches", "workgroups", "timed")


class HipMetricHandler:
    """Owns one `kta_ctx`.  `handle_message` == MetricHandler::handle_message (kafka.rs:18-20)."""

    def __init__(self, n_partitions: int, count_alive_keys: bool = False, device: int = 0,
                 batch_capacity: int = 0, key_bytes_capacity: int = 0, n_staging: int = 0,
                 now: Optional[Tuple[int, int]] = None, analytics: bool = False, alive_table: bool = False,
                 seq_column: bool = False, timeline: Optional[Tuple[int, int, int]] = None, key_sketch: bool = False,
                 hot_keys: bool = False, ts_order: bool = False, partitioner: bool = False, repartition: Optional[int] = None,
                 compaction: bool = False, size_quantiles: bool = False, segments: Optional[Tuple[int, int, int]] = None,
                 compact_delete: bool = False, record_batches: bool = False, payload: bool = False, header_names: bool = False,
                 value_bytes: bool = False, compress_whatif: bool = False):
        """alive_table: keep the alive set as the sequence-numbered table (KTA_FLAG_ALIVE_TABLE: batches / shards in
        any order, needed by a rank of a sharded run) instead of the reference's bit set (submission order);
        seq_column: the staging batches carry every record's global sequence number (KTA_FLAG_SEQ_COLUMN);
        timeline: (origin_ms, bucket_ms, n_buckets) — records, tombstones and bytes per time bucket (kta_set_timeline);
        key_sketch: a HyperLogLog sketch of the key hashes per partition (KTA_FLAG_KEY_SKETCH: estimate_distinct_keys);
        hot_keys: the topic-wide hot-key sketch (KTA_FLAG_HOT_KEYS: recover_hot_keys, hot_key_exemplars);
        ts_order: the timestamp-order pass (KTA_FLAG_TS_ORDER: late records per partition, ts_order());
        partitioner: the partitioner pass (KTA_FLAG_PARTITIONER: keyed records on murmur2's partition and their spread
        over `repartition` partitions — n_partitions when None —, partitioner());
        compaction: the compaction what-if (KTA_FLAG_COMPACTION; needs count_alive_keys and implies alive_table: replay the
        records inside compaction_replay(), then compaction());
        size_quantiles: the size-percentile pass (KTA_FLAG_SIZE_QUANTILES: a 464-bin histogram of the key, value and message
        sizes per partition, size_quantiles());
        segments: (segment_bytes, rows_per_partition, record_overhead) — the segment pass of the retention what-if
        (kta_set_segments: segments(), then retention_whatif on the vector);
        compact_delete: the compact,delete what-if (kta_set_compact_delete; needs compaction=True and segments: the replay
        also writes the kept vector, compact_delete(), for compact_delete_whatif);
        record_batches: the record-batch section (KTA_FLAG_RECORD_BATCHES: what the batch headers of the raw-log decode say,
        get_record_batches());
        payload: the payload section (KTA_FLAG_PAYLOAD: value formats, schema-registry ids and record headers of the records of
        the raw-log decode, get_payload());
        header_names: the header-name section (KTA_FLAG_HEADER_NAMES: a census of the names of the record headers of the raw-log
        decode, header_names() and header_name_table());
        value_bytes: the value-byte section (KTA_FLAG_VALUE_BYTES: a byte histogram of the values of the records of the raw-log
        decode per partition, value_bytes());
        compress_whatif: the compression what-if (KTA_FLAG_COMPRESS_WHATIF: the bytes a defined LZ4 compressor would leave of the
        records section of every batch of the raw-log decode, compress_whatif())."""
        self._lib = N.load()
        self._ctx = C.c_void_p()
        self.n_partitions = int(n_partitions)
        self.count_alive_keys = bool(count_alive_keys)
        self.key_sketch_on = bool(key_sketch)
        self.hot_keys_on = bool(hot_keys)
        self.partitioner_on = bool(partitioner)
        self.compaction_on = bool(compaction)
        self.size_quantiles_on = bool(size_quantiles)
        self.record_batches_on = bool(record_batches)
        self.payload_on = bool(payload)
        self.header_names_on = bool(header_names)
        self.value_bytes_on = bool(value_bytes)
        self.compress_whatif_on = bool(compress_whatif)
        cfg = KtaConfig(device, n_partitions, 1 if count_alive_keys else 0, n_staging, batch_capacity,
                        key_bytes_capacity, (N.KTA_FLAG_ANALYTICS if analytics else 0) |
                        (N.KTA_FLAG_KEY_SKETCH if key_sketch else 0) | (N.KTA_FLAG_HOT_KEYS if hot_keys else 0) |
                        (N.KTA_FLAG_TS_ORDER if ts_order else 0) | (N.KTA_FLAG_PARTITIONER if partitioner else 0) |
                        (N.KTA_FLAG_COMPACTION if compaction else 0) | (N.KTA_FLAG_SIZE_QUANTILES if size_quantiles else 0) |
                        (N.KTA_FLAG_RECORD_BATCHES if record_batches else 0) | (N.KTA_FLAG_PAYLOAD if payload else 0) |
                        (N.KTA_FLAG_HEADER_NAMES if header_names else 0) | (N.KTA_FLAG_VALUE_BYTES if value_bytes else 0) |
                        (N.KTA_FLAG_COMPRESS_WHATIF if compress_whatif else 0) |
                        (N.KTA_FLAG_ALIVE_TABLE if alive_table else 0) | (N.KTA_FLAG_SEQ_COLUMN if seq_column else 0), 0)
        rc = self._lib.kta_create(C.byref(cfg), C.byref(self._ctx))
        if rc != N.KTA_OK:
            raise KtaError(rc, self._lib.kta_last_error(None).decode())
        self.timeline_config = None
        if timeline is not None:
            try:
                self.set_timeline(*timeline)
            except KtaError:
                self.close()
                raise
        self.segments_config = None
        if segments is not None:
            try:
                self.set_segments(*segments)
            except KtaError:
                self.close()
                raise
        self.compact_delete_on = False
        if compact_delete:
            try:
                self.set_compact_delete(True)
            except KtaError:
                self.close()
                raise
        self.repartition = self.n_partitions if partitioner else 0
        if partitioner and repartition is not None:
            try:
                self.set_repartition(repartition)
            except KtaError:
                self.close()
                raise
        if now is None:  # Utc::now() at MessageMetrics::new (metric.rs:39)
            t = time.time_ns()
            now = (t // 1_000_000_000, t % 1_000_000_000)
        self.now = now
        self._next_seq = 0

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc: int, allow=()):
        if rc != N.KTA_OK and rc not in allow:
            kind = DateTimeRangePanic if rc == N.KTA_ERR_TIMESTAMP_RANGE else KtaError
            raise kind(rc, self._lib.kta_last_error(self._ctx).decode())
        return rc

    def close(self):
        if self._ctx:
            self._lib.kta_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ record entry points
    def handle_message(self, m: Message) -> None:
        ts = -1 if m.timestamp_ms is None else int(m.timestamp_ms)
        if m.key is None:
            kptr, klen = None, -1
        else:
            kbuf = C.create_string_buffer(m.key, max(len(m.key), 1))
            kptr, klen = C.cast(kbuf, C.c_void_p), len(m.key)
        vlen = -1 if m.payload_len is None else int(m.payload_len)
        self._check(self._lib.kta_handle_message(self._ctx, m.partition, ts, kptr, klen, vlen))

    def flush(self) -> None:
        self._check(self._lib.kta_flush(self._ctx))

    def replay_messages(self, cols: dict, n: Optional[int] = None) -> None:
        """kta_handle_message for every record of host (numpy) columns, as a native loop (kta_replay_messages)."""
        b = KtaBatch()
        keep = []
        for name, dt in (("partition", np.int32), ("key_len", np.int32), ("val_len", np.int32), ("ts_ms", np.int64)):
            a = np.ascontiguousarray(cols[name], dtype=dt)
            keep.append(a)
            setattr(b, name, a.ctypes.data)
        if "key_off" in cols and "key_bytes" in cols:
            ko = np.ascontiguousarray(cols["key_off"], dtype=np.uint32)
            kb = np.ascontiguousarray(cols["key_bytes"], dtype=np.uint8)
            keep += [ko, kb]
            b.key_off, b.key_bytes = ko.ctypes.data, kb.ctypes.data
        m = len(keep[0]) if n is None else int(n)
        if m < 0 or any(m > len(a) for a in keep[:4]) or (len(keep) > 4 and m > len(keep[4])):   # the native loop reads m of each
            raise ValueError(f"replay_messages: n = {m} is not in [0, {min(len(a) for a in keep[:4])}], the records the columns hold")
        self._check(self._lib.kta_replay_messages(self._ctx, C.byref(b), m))

    def handle_message_stats(self) -> dict:
        out = (C.c_uint64 * 4)()
        self._check(self._lib.kta_handle_message_stats(self._ctx, C.byref(out)))
        return {"messages": int(out[0]), "batches": int(out[1]), "submit_ns": int(out[2]), "ring_wait_ns": int(out[3])}

    def submit_columns(self, partition, key_len, val_len, ts_ms, key_off=None, key_bytes=None,
                       base_seq: Optional[int] = None) -> None:
        """Feed a struct-of-arrays batch through the pinned staging ring (chunked to its capacity)."""
        partition = np.ascontiguousarray(partition, dtype=np.int32)
        key_len = np.ascontiguousarray(key_len, dtype=np.int32)
        val_len = np.ascontiguousarray(val_len, dtype=np.int32)
        ts_ms = np.ascontiguousarray(ts_ms, dtype=np.int64)
        n = len(partition)
        keys = self.count_alive_keys or self.key_sketch_on or self.hot_keys_on or self.partitioner_on   # the staging batches carry the keys
        if keys:
            key_off = np.ascontiguousarray(key_off, dtype=np.uint32)
            key_bytes = np.ascontiguousarray(key_bytes, dtype=np.uint8)
        seq0 = self._next_seq if base_seq is None else base_seq
        i = 0
        while i < n:
            b = KtaBatch()
            self._check(self._lib.kta_batch_acquire(self._ctx, C.byref(b)))
            m = min(n - i, b.capacity)
            kb = 0
            if keys:
                # largest prefix whose (packed, monotone) key bytes fit the staging key capacity
                kl = np.maximum(key_len[i:i + m], 0).astype(np.int64)
                ends = np.cumsum(kl)
                fit = int(np.searchsorted(ends, b.key_bytes_capacity, side="right"))
                if fit == 0:
                    raise KtaError(N.KTA_ERR_CAPACITY, "a single key exceeds key_bytes_capacity")
                m = min(m, fit)
                kb = int(ends[m - 1])
                # re-pack this chunk's keys contiguously (input offsets may be arbitrary)
                starts = ends[:m] - kl[:m]
                dst_off = np.frombuffer((C.c_uint32 * m).from_address(b.key_off), dtype=np.uint32)
                dst_off[:] = starts.astype(np.uint32)
                if kb:
                    dst_kb = np.frombuffer((C.c_uint8 * kb).from_address(b.key_bytes), dtype=np.uint8)
                    src_off = key_off[i:i + m].astype(np.int64)
                    if np.array_equal(src_off - src_off[0], starts):  # already packed: one memcpy
                        s0 = int(src_off[0])
                        dst_kb[:] = key_bytes[s0:s0 + kb]
                    else:
                        for j in np.nonzero(kl[:m])[0]:
                            dst_kb[starts[j]:starts[j] + kl[j]] = key_bytes[src_off[j]:src_off[j] + kl[j]]
            C.memmove(b.partition, partition.ctypes.data + 4 * i, 4 * m)
            C.memmove(b.key_len, key_len.ctypes.data + 4 * i, 4 * m)
            C.memmove(b.val_len, val_len.ctypes.data + 4 * i, 4 * m)
            C.memmove(b.ts_ms, ts_ms.ctypes.data + 8 * i, 8 * m)
            self._check(self._lib.kta_batch_submit(self._ctx, m, kb, seq0 + i))
            i += m
        self._next_seq = seq0 + n

    # ------------------------------------------------------------------ device-resident batches
    def device_batch_alloc(self, capacity: int, key_bytes_capacity: int = 0, with_seq: bool = False) -> KtaBatch:
        b = KtaBatch()
        self._check(self._lib.kta_device_batch_alloc(self._ctx, capacity, key_bytes_capacity,
                                                     1 if with_seq else 0, C.byref(b)))
        return b

    def device_batch_free(self, b: KtaBatch) -> None:
        self._check(self._lib.kta_device_batch_free(self._ctx, C.byref(b)))

    def synth_fill_device(self, spec: KtaSynthSpec, first: int, n: int, b: KtaBatch) -> int:
        kb = C.c_uint64(0)
        self._check(self._lib.kta_synth_fill_device(self._ctx, C.byref(spec), first, n, C.byref(b), C.byref(kb)))
        return kb.value

    def submit_device(self, b: KtaBatch, n: int, base_seq: int = 0, which: int = 3) -> None:
        self._check(self._lib.kta_submit_device_ex(self._ctx, C.byref(b), n, base_seq, which))

    def download_batch(self, b: KtaBatch, n: int, n_key_bytes: int = 0):
        """Copy a device batch's columns to numpy arrays in the raw layout (tests; kta_batch_to_raw unpacks the
        tile-compact layout)."""
        out = {name: np.empty(n, dtype=dt) for name, dt in
               (("partition", np.int32), ("key_len", np.int32), ("val_len", np.int32), ("ts_ms", np.int64))}
        if n:
            self._check(self._lib.kta_batch_to_raw(self._ctx, C.byref(b), n, C.byref(_host_batch(out))))
        if b.key_off:
            a = np.empty(n, dtype=np.uint32)
            if n:
                self._check(self._lib.kta_copy_to_host(self._ctx, _np_ptr(a), b.key_off, a.nbytes))
            out["key_off"] = a
            kbs = np.empty(n_key_bytes, dtype=np.uint8)
            if n_key_bytes:
                self._check(self._lib.kta_copy_to_host(self._ctx, _np_ptr(kbs), b.key_bytes, kbs.nbytes))
            out["key_bytes"] = kbs
        if b.seq:
            a = np.empty(n, dtype=np.uint64)
            if n:
                self._check(self._lib.kta_copy_to_host(self._ctx, _np_ptr(a), b.seq, a.nbytes))
            out["seq"] = a
        return out

    def batch_tile_summaries(self, b: KtaBatch, n: int) -> np.ndarray:
        """The tile summaries (kta_tile_sum) of the tiles of records [0, n) of a device batch: a structured array with the
        fields ts_span (u32), part_max (u16) and flags (u16), one entry per tile."""
        out = np.zeros((n + N.KTA_TILE_RECORDS - 1) // N.KTA_TILE_RECORDS,
                       dtype=np.dtype([("ts_span", np.uint32), ("part_max", np.uint16), ("flags", np.uint16)]))
        self._check(self._lib.kta_batch_tile_summaries(self._ctx, C.byref(b), n, _np_ptr(out)))
        return out

    def batch_tile_planes(self, b: KtaBatch, n: int) -> np.ndarray:
        """The plane marks (kta_batch_tile_planes) of the tiles of records [0, n) of a device batch: uint32, one per tile,
        1 where the tile has a scan plane."""
        out = np.zeros((n + N.KTA_TILE_RECORDS - 1) // N.KTA_TILE_RECORDS, dtype=np.uint32)
        self._check(self._lib.kta_batch_tile_planes(self._ctx, C.byref(b), n, _np_ptr(out)))
        return out

    def upload_batch(self, cols: dict, with_keys: bool = False) -> Tuple[KtaBatch, int]:
        """numpy columns -> a new device batch (tests: bypasses the staging ring)."""
        n = len(cols["partition"])
        kbytes = np.ascontiguousarray(cols.get("key_bytes", np.zeros(0, np.uint8)), dtype=np.uint8)
        b = self.device_batch_alloc(max(n, 1), max(len(kbytes), 1) if with_keys else 0, "seq" in cols)
        metric = {name: np.ascontiguousarray(cols[name], dtype=dt) for name, dt in
                  (("partition", np.int32), ("key_len", np.int32), ("val_len", np.int32), ("ts_ms", np.int64))}
        if n:   # kta_batch_from_raw packs the tiles (raw where the compact form cannot hold them)
            self._check(self._lib.kta_batch_from_raw(self._ctx, C.byref(_host_batch(metric)), n, C.byref(b)))
        if with_keys:
            a = np.ascontiguousarray(cols["key_off"], dtype=np.uint32)
            if n:
                self._check(self._lib.kta_copy_to_device(self._ctx, b.key_off, _np_ptr(a), a.nbytes))
            if len(kbytes):
                self._check(self._lib.kta_copy_to_device(self._ctx, b.key_bytes, _np_ptr(kbytes), kbytes.nbytes))
        if "seq" in cols:
            a = np.ascontiguousarray(cols["seq"], dtype=np.uint64)
            if n:
                self._check(self._lib.kta_copy_to_device(self._ctx, b.seq, _np_ptr(a), a.nbytes))
        return b, n

    # ------------------------------------------------------------------ results
    def use_stream(self, hip_stream: Optional[int]) -> None:
        """Run on a caller-owned, CREATED HIP stream (e.g. torch.cuda.Stream().cuda_stream; torch's default
        stream is the null stream, handle 0, which means "restore" here); None restores."""
        self._check(self._lib.kta_set_compute_stream(self._ctx, C.c_void_p(hip_stream) if hip_stream else None))

    def sync(self) -> None:
        self._check(self._lib.kta_sync(self._ctx))

    def reset(self) -> None:
        self._check(self._lib.kta_reset(self._ctx))
        self._next_seq = 0

    def finish(self, allow_bad_partition: bool = False):
        """-> (KtaResult, counters[P,7] uint64)."""
        res = KtaResult()
        counters = np.zeros((self.n_partitions, N.KTA_NCOUNTERS), dtype=np.uint64)
        allow = (N.KTA_ERR_BAD_PARTITION,) if allow_bad_partition else ()
        self._check(self._lib.kta_finish(self._ctx, C.byref(res), _np_ptr(counters)), allow)
        return res, counters

    def finish_device(self) -> None:
        self._check(self._lib.kta_finish_device(self._ctx))

    # ------------------------------------------------------------------ multi-GPU exchange (RCCL, native)
    @staticmethod
    def comm_unique_id() -> bytes:
        """On one rank; hand the bytes to the other ranks out of band."""
        buf = C.create_string_buffer(N.KTA_COMM_ID_BYTES)
        rc = N.load().kta_comm_unique_id(buf)
        if rc != N.KTA_OK:
            raise KtaError(rc, "kta_comm_unique_id (RCCL not loadable?)")
        return buf.raw

    def comm_create(self, nranks: int, rank: int, unique_id: Optional[bytes] = None) -> None:
        self._check(self._lib.kta_comm_create(self._ctx, nranks, rank, unique_id))

    def comm_destroy(self) -> None:
        self._check(self._lib.kta_comm_destroy(self._ctx))

    def exchange(self) -> None:
        """The one exchange step of a partition-sharded run (asynchronous on the compute stream but for the
        two count read-backs of a -c run)."""
        self._check(self._lib.kta_exchange(self._ctx))

    def exchange_result(self, allow_bad_partition: bool = False):
        """-> (KtaResult, counters[P,7]) of the snapshot vector: after exchange(), the whole job's."""
        res = KtaResult()
        counters = np.zeros((self.n_partitions, N.KTA_NCOUNTERS), dtype=np.uint64)
        allow = (N.KTA_ERR_BAD_PARTITION,) if allow_bad_partition else ()
        self._check(self._lib.kta_exchange_result(self._ctx, C.byref(res), _np_ptr(counters)), allow)
        return res, counters

    def comm_allreduce_i64(self, values: np.ndarray, op_max: bool = False) -> np.ndarray:
        a = np.ascontiguousarray(values, dtype=np.int64).copy()
        self._check(self._lib.kta_comm_allreduce_i64(self._ctx, _np_ptr(a), a.size, 1 if op_max else 0))
        return a

    def comm_info(self):
        nr, rk, se, re = C.c_int(), C.c_int(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.kta_comm_info(self._ctx, C.byref(nr), C.byref(rk), C.byref(se), C.byref(re)))
        return nr.value, rk.value, se.value, re.value

    def _pass_info(self, fn, keys) -> dict:
        """What the kta_*_info of a pass of the decode call reports: its words under `keys` (None: a word without a meaning) and
        kernel_ms, the mean duration of the launches timed since the previous call (None without one)."""
        out, ms = (C.c_uint64 * len(keys))(), C.c_float()
        self._check(fn(self._ctx, C.byref(out), C.byref(ms)))
        info = {k: int(v) for k, v in zip(keys, out) if k}
        info["kernel_ms"] = float(ms.value) if ms.value >= 0 else None
        return info

    def _device_vector(self, fn) -> Tuple[int, int]:
        """What a `(kta_ctx *, void **device_ptr, size_t *n_u64)` entry point answers."""
        p, n = C.c_void_p(), C.c_size_t()
        self._check(fn(self._ctx, C.byref(p), C.byref(n)))
        return p.value, n.value

    def _shape(self, name: str) -> Optional[tuple]:
        """The shape of section `name` in this handler, the arguments of its row of _SECTIONS; None: a timeline that was
        never configured."""
        P = self.n_partitions
        if name == "timeline":
            return (self.timeline_config[2],) if self.timeline_config else None
        if name in ("segments", "compact_delete"):
            if self.segments_config is None:
                raise KtaError(N.KTA_ERR_INVALID, "the handler has no segments (segments=...)")
            return (P, self.segments_config[1])
        if name == "partitioner":
            return (P, self.repartition)
        if name in ("hot_keys", "header_names"):
            return ()
        return (P,)

    def _read_section(self, name: str, fn) -> np.ndarray:
        """What a `(kta_ctx *, uint64_t *out, size_t n_u64)` read-back of section `name` (kta_get_* / kta_exchange_*) answers."""
        shape = self._shape(name)
        words = 0 if shape is None else _section_words(name, *shape)   # (no words: the library says that the section is off)
        out = np.zeros(max(words, 1), dtype=np.uint64)
        self._check(fn(self._ctx, _np_ptr(out), words))
        return out if words else out[:0]

    def result_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the counter vector (for collectives)."""
        return self._device_vector(self._lib.kta_result_vector)

    def result_vector_host(self) -> np.ndarray:
        p, n = self.result_vector()
        a = np.empty(n, dtype=np.uint64)
        self._check(self._lib.kta_copy_to_host(self._ctx, _np_ptr(a), C.c_void_p(p), a.nbytes))
        return a

    def alive_table(self) -> Tuple[int, int]:
        return self._device_vector(self._lib.kta_alive_table)

    def analytics(self) -> dict:
        """Additive analytics (not in the reference): size histograms + per-partition extrema of this
        context's live accumulator."""
        return self._analytics(self._lib.kta_get_analytics)

    def exchange_analytics(self) -> dict:
        """As analytics(), of the snapshot finish() / exchange() took: after exchange(), the whole job's."""
        return self._analytics(self._lib.kta_exchange_analytics)

    def _analytics(self, fn) -> dict:
        a = N.KtaAnalytics()
        out = _analytics_arrays(self.n_partitions)
        self._check(fn(self._ctx, C.byref(a), *[_np_ptr(out[k]) for k in _PART_KEYS]))
        return _analytics_dict(a, out)

    def analytics_result_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the analytics snapshot (for collectives: allreduce_analytics_vector)."""
        return self._device_vector(self._lib.kta_analytics_result_vector)

    def set_timeline(self, origin_ms: int, bucket_ms: int, n_buckets: int) -> None:
        """kta_set_timeline: only before the context has been handed any record (since creation / reset())."""
        self._check(self._lib.kta_set_timeline(self._ctx, int(origin_ms), int(bucket_ms), int(n_buckets)))
        self.timeline_config = (int(origin_ms), int(bucket_ms), int(n_buckets))

    def timeline(self) -> np.ndarray:
        """The live timeline, np.uint64[n_buckets + 3, 3]: rows [no timestamp, before, buckets..., after] of
        [records, tombstones, bytes] (kta_get_timeline; staged messages are flushed first)."""
        return self._read_section("timeline", self._lib.kta_get_timeline).reshape(-1, N.KTA_TIMELINE_COLS)

    def exchange_timeline(self) -> np.ndarray:
        """As timeline(), of the snapshot finish() / exchange() took: after exchange(), the whole job's."""
        return self._read_section("timeline", self._lib.kta_exchange_timeline).reshape(-1, N.KTA_TIMELINE_COLS)

    def timeline_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the live timeline."""
        return self._device_vector(self._lib.kta_timeline_vector)

    def timeline_result_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the timeline snapshot (for collectives: allreduce_timeline_vector)."""
        return self._device_vector(self._lib.kta_timeline_result_vector)

    def key_sketch(self) -> np.ndarray:
        """The live key sketch, np.uint64[P, 4096]: register j of partition p (kta_get_key_sketch; staged messages are
        flushed first)."""
        return self._read_section("key_sketch", self._lib.kta_get_key_sketch).reshape(self.n_partitions, N.KTA_SKETCH_REGISTERS)

    def exchange_key_sketch(self) -> np.ndarray:
        """As key_sketch(), of the snapshot finish() / exchange() took: after exchange(), the whole job's."""
        return self._read_section("key_sketch", self._lib.kta_exchange_key_sketch).reshape(self.n_partitions, N.KTA_SKETCH_REGISTERS)

    def key_sketch_result_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the key sketch snapshot (for collectives: allreduce_key_sketch_vector)."""
        return self._device_vector(self._lib.kta_key_sketch_result_vector)

    def key_sketch_info(self) -> dict:
        """Work counters of the sketch kernel since creation / reset() (kta_key_sketch_info)."""
        out = (C.c_uint64 * 4)()
        self._check(self._lib.kta_key_sketch_info(self._ctx, C.byref(out)))
        return {"keyed": int(out[0]), "reads": int(out[1]), "atomics": int(out[2]), "launches": int(out[3])}

    def hot_keys(self) -> np.ndarray:
        """The live hot-key vector, np.uint64[2, 1024, 23]: per row and cell the total and the 22 bit counts
        (kta_get_hot_keys; staged messages are flushed first)."""
        return self._read_section("hot_keys", self._lib.kta_get_hot_keys).reshape(N.KTA_HOT_ROWS, N.KTA_HOT_CELLS, N.KTA_HOT_WORDS)

    def exchange_hot_keys(self) -> np.ndarray:
        """As hot_keys(), of the snapshot finish() / exchange() took: after exchange(), the whole job's."""
        return self._read_section("hot_keys", self._lib.kta_exchange_hot_keys).reshape(N.KTA_HOT_ROWS, N.KTA_HOT_CELLS, N.KTA_HOT_WORDS)

    def hot_keys_result_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the hot-key snapshot (for collectives: allreduce_hot_keys_vector)."""
        return self._device_vector(self._lib.kta_hot_keys_result_vector)

    def hot_keys_info(self) -> dict:
        """Work counters of the hot-key pass since creation / reset() (kta_hot_keys_info)."""
        out = (C.c_uint64 * 6)()
        self._check(self._lib.kta_hot_keys_info(self._ctx, C.byref(out)))
        return dict(zip(("keyed", "groups", "flushes", "launches", "exemplars", "workgroups"), (int(x) for x in out)))

    def set_hot_flush_rounds(self, rounds: int) -> None:
        """Tests: a workgroup of the hot-key pass flushes its LDS counters every `rounds` rounds (0: the default)."""
        self._check(self._lib.kta_set_hot_flush_rounds(self._ctx, int(rounds)))

    def hot_key_exemplars(self) -> np.ndarray:
        """This context's exemplar table (kta_get_hot_key_exemplars): a structured array [2048] with the fields hash,
        key_len, valid, pad, bytes[32]; render_hot_keys and hot_key_exemplar_of read it."""
        out = np.zeros(N.KTA_HOT_ROWS * N.KTA_HOT_CELLS, dtype=HOT_EXEMPLAR_DTYPE)
        self._check(self._lib.kta_get_hot_key_exemplars(self._ctx, _np_ptr(out), out.size))
        return out

    def ts_order(self) -> dict:
        """The live timestamp-order vector as a dict of np.uint64 arrays: late[P], late_ms_sum[P], max_late_ms[P], hist[63],
        timed (kta_get_ts_order; staged messages are flushed first); "vector" is the whole u64[3 P + 64]."""
        return split_ts_order(self._read_section("ts_order", self._lib.kta_get_ts_order), self.n_partitions)

    def exchange_ts_order(self) -> dict:
        """As ts_order(), of the snapshot finish() / exchange() took: after exchange(), the whole job's."""
        return split_ts_order(self._read_section("ts_order", self._lib.kta_exchange_ts_order), self.n_partitions)

    def ts_order_result_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the timestamp-order snapshot (for collectives: allreduce_ts_order_vector)."""
        return self._device_vector(self._lib.kta_ts_order_result_vector)

    def ts_order_info(self) -> dict:
        """Work counters of the timestamp-order pass since creation / reset() (kta_ts_order_info)."""
        out = (C.c_uint64 * 6)()
        self._check(self._lib.kta_ts_order_info(self._ctx, C.byref(out)))
        return dict(zip(("launches", "chunks", "instructions", "one_partition", "groups", "chunk_records"), (int(x) for x in out)))

    def set_segments(self, segment_bytes: int, rows_per_partition: int, record_overhead: int = 0) -> None:
        """kta_set_segments: turn the segment pass of the retention what-if on (before the first record since creation /
        reset())."""
        self._check(self._lib.kta_set_segments(self._ctx, int(segment_bytes), int(rows_per_partition), int(record_overhead)))
        self.segments_config = (int(segment_bytes), int(rows_per_partition), int(record_overhead))
        self.compact_delete_on = False   # (another configuration: kta_set_segments turns the compact,delete what-if off)

    def set_compact_delete(self, on: bool = True) -> None:
        """kta_set_compact_delete: the compact,delete what-if on or off (after set_segments, before the first record since
        creation / reset(); needs compaction=True)."""
        self._check(self._lib.kta_set_compact_delete(self._ctx, 1 if on else 0))
        self.compact_delete_on = bool(on)

    def compact_delete(self) -> dict:
        """The live kept vector (kta_get_compact_delete; staged messages are flushed first) as split_compact_delete gives it."""
        return split_compact_delete(self._read_section("compact_delete", self._lib.kta_get_compact_delete), *self._shape("compact_delete"))

    def compact_delete_info(self) -> dict:
        """Work counters of the kept-row kernels since the replay began (kta_compact_delete_info)."""
        out = (C.c_uint64 * 4)()
        self._check(self._lib.kta_compact_delete_info(self._ctx, C.byref(out)))
        return {"launches": int(out[0]), "chunks": int(out[1]), "chunks_applied": int(out[2]), "scratch_bytes": int(out[3])}

    def segments(self) -> dict:
        """The live segment vector (kta_get_segments; staged messages are flushed first) as split_segments gives it: "rows"
        [P][M][4], "totals" [P][4], "globals" [8] and "vector", the whole u64[(P M + P) 4 + 8]."""
        return split_segments(self._read_section("segments", self._lib.kta_get_segments), *self._shape("segments"))

    def exchange_segments(self) -> dict:
        """As segments(), of the snapshot finish() / exchange() took: after exchange(), the whole job's."""
        return split_segments(self._read_section("segments", self._lib.kta_exchange_segments), *self._shape("segments"))

    def segments_result_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the segment snapshot (for collectives: allreduce_segments_vector)."""
        return self._device_vector(self._lib.kta_segments_result_vector)

    def segments_info(self) -> dict:
        """Work counters of the segment pass since creation / reset() (kta_segments_info)."""
        out = (C.c_uint64 * 6)()
        self._check(self._lib.kta_segments_info(self._ctx, C.byref(out)))
        return {"chunks": out[0], "chunk_records": out[1], "launches": out[2], "chunks_applied": out[3], "chunks_skipped": out[4],
                "groups": out[5]}

    def set_segments_chunk(self, records: int) -> None:
        """Tests: records per chunk of the segment pass (a multiple of 64; 0: the default)."""
        self._check(self._lib.kta_set_segments_chunk(self._ctx, int(records)))

    def set_ts_order_chunk(self, records: int) -> None:
        """Tests: the records per chunk of the timestamp-order pass, a multiple of 64 (0: the default)."""
        self._check(self._lib.kta_set_ts_order_chunk(self._ctx, int(records)))

    def set_repartition(self, q: int) -> None:
        """The what-if partition count Q of the partitioner pass (kta_set_repartition): only while the context has been
        handed no record since creation / reset()."""
        self._check(self._lib.kta_set_repartition(self._ctx, int(q)))
        self.repartition = int(q)

    def partitioner(self) -> dict:
        """The live partitioner vector as a dict of np.uint64 arrays: checked[P], placed[P], target_records[Q],
        target_bytes[Q] (kta_get_partitioner; staged messages are flushed first); "vector" is the whole u64[2 P + 2 Q]."""
        return split_partitioner(self._read_section("partitioner", self._lib.kta_get_partitioner), *self._shape("partitioner"))

    def exchange_partitioner(self) -> dict:
        """As partitioner(), of the snapshot finish() / exchange() took: after exchange(), the whole job's."""
        return split_partitioner(self._read_section("partitioner", self._lib.kta_exchange_partitioner), *self._shape("partitioner"))

    def partitioner_result_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the partitioner snapshot (for collectives: allreduce_partitioner_vector)."""
        return self._device_vector(self._lib.kta_partitioner_result_vector)

    def partitioner_info(self) -> dict:
        """Work counters of the partitioner pass since creation / reset() (kta_partitioner_info)."""
        out = (C.c_uint64 * 6)()
        self._check(self._lib.kta_partitioner_info(self._ctx, C.byref(out)))
        return dict(zip(("keyed_records", "launches", "partition_adds", "target_adds", "workgroups", "lds_bytes"), (int(x) for x in out)))

    def size_quantiles(self) -> dict:
        """The live size vector as a dict of np.uint64 arrays: key[P][464], value[P][464], message[P][464], the globals
        records, bad_partition, keyed, alive (kta_get_size_quantiles; staged messages are flushed first); "vector" is the
        whole u64[P * 3 * 464 + 8]."""
        return split_size_quantiles(self._read_section("size_quantiles", self._lib.kta_get_size_quantiles), self.n_partitions)

    def exchange_size_quantiles(self) -> dict:
        """As size_quantiles(), of the snapshot finish() / exchange() took: after exchange(), the whole job's."""
        return split_size_quantiles(self._read_section("size_quantiles", self._lib.kta_exchange_size_quantiles), self.n_partitions)

    def size_quantiles_result_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the size-percentile snapshot (for collectives: allreduce_size_quantiles_vector)."""
        return self._device_vector(self._lib.kta_size_quantiles_result_vector)

    def get_record_batches(self) -> dict:
        """The live record-batch vector as split_record_batches gives it (kta_get_record_batches; staged messages are
        flushed first)."""
        return split_record_batches(self._read_section("record_batches", self._lib.kta_get_record_batches), self.n_partitions)

    def exchange_record_batches(self) -> dict:
        """As get_record_batches(), of the snapshot finish() / exchange() took: after exchange(), the whole job's."""
        return split_record_batches(self._read_section("record_batches", self._lib.kta_exchange_record_batches), self.n_partitions)

    def record_batches_result_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the record-batch snapshot (for collectives: allreduce_record_batches_vector)."""
        return self._device_vector(self._lib.kta_record_batches_result_vector)

    def record_batches_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the live record-batch vector."""
        return self._device_vector(self._lib.kta_record_batches_vector)

    def record_batches_info(self) -> dict:
        """The record-batch pass's work since creation (kta_record_batches_info); kernel_ms is the mean duration of the
        launches timed since the previous call, None without one (set_timing(True))."""
        return self._pass_info(self._lib.kta_record_batches_info, _PASS_INFO_KEYS)

    def get_payload(self) -> dict:
        """The live payload vector as split_payload gives it (kta_get_payload; staged messages are flushed first)."""
        return split_payload(self._read_section("payload", self._lib.kta_get_payload), self.n_partitions)

    def exchange_payload(self) -> dict:
        """As get_payload(), of the snapshot finish() / exchange() took: after exchange(), the whole job's."""
        return split_payload(self._read_section("payload", self._lib.kta_exchange_payload), self.n_partitions)

    def payload_result_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the payload snapshot (for collectives: allreduce_payload_vector)."""
        return self._device_vector(self._lib.kta_payload_result_vector)

    def payload_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the live payload vector."""
        return self._device_vector(self._lib.kta_payload_vector)

    def payload_info(self) -> dict:
        """The payload pass's work since creation (kta_payload_info); kernel_ms is the mean duration of the launches timed
        since the previous call, None without one (set_timing(True))."""
        return self._pass_info(self._lib.kta_payload_info, _PASS_INFO_KEYS)

    def header_names(self) -> dict:
        """The live header-name vector as split_header_names gives it, with this context's name table (kta_get_header_names;
        staged messages are flushed first)."""
        return split_header_names(self._read_section("header_names", self._lib.kta_get_header_names), self.header_name_table())

    def exchange_header_names(self) -> dict:
        """As header_names(), of the snapshot finish() / exchange() took: after exchange(), the whole job's vector; the name
        table stays this context's own."""
        return split_header_names(self._read_section("header_names", self._lib.kta_exchange_header_names), self.header_name_table())

    def header_name_table(self) -> np.ndarray:
        """This context's name table (kta_get_header_name_table): a structured array [2048] of HEADER_NAME_DTYPE; a slot that is
        not published is all zeros."""
        out = np.zeros(N.KTA_HEADER_NAMES_SLOTS, dtype=HEADER_NAME_DTYPE)
        self._check(self._lib.kta_get_header_name_table(self._ctx, _np_ptr(out), out.size))
        return out

    def header_names_result_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the header-name snapshot (for collectives: allreduce_header_names_vector)."""
        return self._device_vector(self._lib.kta_header_names_result_vector)

    def header_names_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the live header-name vector."""
        return self._device_vector(self._lib.kta_header_names_vector)

    def header_names_info(self) -> dict:
        """The header-name pass's work (kta_header_names_info): launches, batches, workgroups and timed launches since creation;
        spills (occurrences that went past the workgroup's cache), claims and early cache flushes since creation / reset();
        kernel_ms as payload_info's."""
        return self._pass_info(self._lib.kta_header_names_info, _PASS_INFO_KEYS + ("spills", "claims", "cache_flushes", None))

    def value_bytes(self) -> dict:
        """The live value-byte vector as split_value_bytes gives it: the vector, the partitions' words and the summaries per
        partition and of the topic (kta_get_value_bytes; staged messages are flushed first)."""
        return split_value_bytes(self._read_section("value_bytes", self._lib.kta_get_value_bytes), self.n_partitions)

    def exchange_value_bytes(self) -> dict:
        """As value_bytes(), of the snapshot finish() / exchange() took: after exchange(), the whole job's."""
        return split_value_bytes(self._read_section("value_bytes", self._lib.kta_exchange_value_bytes), self.n_partitions)

    def value_bytes_result_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the value-byte snapshot (for collectives: allreduce_value_bytes_vector)."""
        return self._device_vector(self._lib.kta_value_bytes_result_vector)

    def value_bytes_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the live value-byte vector."""
        return self._device_vector(self._lib.kta_value_bytes_vector)

    def value_bytes_info(self) -> dict:
        """The value-byte pass's work (kta_value_bytes_info): launches, batches and workgroups since creation; mid_flushes, the
        flushes of a workgroup's bins in the middle of a pass, since creation / reset(); kernel_ms as payload_info's."""
        return self._pass_info(self._lib.kta_value_bytes_info, _PASS_INFO_KEYS[:3] + ("mid_flushes",))

    def compress_whatif(self) -> dict:
        """The live compression what-if vector as split_compress_whatif gives it (kta_get_compress_whatif; staged messages are
        flushed first)."""
        return split_compress_whatif(self._read_section("compress_whatif", self._lib.kta_get_compress_whatif), self.n_partitions)

    def exchange_compress_whatif(self) -> dict:
        """As compress_whatif(), of the snapshot finish() / exchange() took: after exchange(), the whole job's."""
        return split_compress_whatif(self._read_section("compress_whatif", self._lib.kta_exchange_compress_whatif), self.n_partitions)

    def compress_whatif_result_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the what-if snapshot (for collectives: allreduce_compress_whatif_vector)."""
        return self._device_vector(self._lib.kta_compress_whatif_result_vector)

    def compress_whatif_vector(self) -> Tuple[int, int]:
        """(device pointer, length in u64) of the live what-if vector."""
        return self._device_vector(self._lib.kta_compress_whatif_vector)

    def compress_whatif_info(self) -> dict:
        """The what-if pass's work since creation (kta_compress_whatif_info): launches, batches, the workgroups of the last
        launch, the timed launches; kernel_ms their mean duration (None without one: set_timing(True))."""
        return self._pass_info(self._lib.kta_compress_whatif_info, _PASS_INFO_KEYS)

    def size_quantiles_info(self) -> dict:
        """The plan of the size-percentile pass for this context and its work since creation / reset() (kta_size_quantiles_info)."""
        out = (C.c_uint64 * 6)()
        self._check(self._lib.kta_size_quantiles_info(self._ctx, C.byref(out)))
        return dict(zip(("slice", "slices", "lds_bytes", "threads", "workgroups", "lds_adds"), (int(x) for x in out)))

    def set_size_quantiles_slice(self, partitions: int) -> None:
        """Tests: the partitions of a slice of the size-percentile pass, 1 .. 28 (0: the plan's own)."""
        self._check(self._lib.kta_set_size_quantiles_slice(self._ctx, int(partitions)))

    def compaction_replay(self, on: bool = True):
        """Replay mode of the compaction what-if on or off (kta_compaction_replay): while it is on every submission path
        hands its batches to the compaction pass and to nothing else.  Either a pair of calls, or
        `with h.compaction_replay(): ...`, which turns the mode off at the end."""
        self._check(self._lib.kta_compaction_replay(self._ctx, 1 if on else 0))
        return _CompactionReplay(self)

    def compaction(self) -> dict:
        """The live compaction vector as a dict (split_compaction; kta_get_compaction; staged messages are flushed first)."""
        return split_compaction(self._read_section("compaction", self._lib.kta_get_compaction), self.n_partitions)

    def compaction_info(self) -> dict:
        """Work counters of the compaction pass since creation / reset() (kta_compaction_info)."""
        out = (C.c_uint64 * 6)()
        self._check(self._lib.kta_compaction_info(self._ctx, C.byref(out)))
        return dict(zip(("keyed_records", "launches", "workgroups", "lds_adds", "lds_bytes", "reserved"), (int(x) for x in out)))

    def set_filter(self, from_ms: Optional[int] = None, to_ms: Optional[int] = None, partitions=None) -> None:
        """Analyse only the records with from_ms <= ts_ms < to_ms (None: no bound on that side) whose partition is one of
        `partitions` (None: all).  Only before the first record; reset() keeps it (kta_set_filter).  All None: no filter."""
        bitmap, words = None, 0
        if partitions is not None:
            bitmap = partition_bitmap(partitions, self.n_partitions)
            words = len(bitmap)
        self._check(self._lib.kta_set_filter(self._ctx, N.KTA_FILTER_NO_FROM if from_ms is None else int(from_ms),
                                             N.KTA_FILTER_NO_TO if to_ms is None else int(to_ms),
                                             None if bitmap is None else _np_ptr(bitmap), words))

    def set_filter_slice(self, records: int) -> None:
        """Tuning / tests: the filter's slice, a multiple of 1024 records (0: the default)."""
        self._check(self._lib.kta_set_filter_slice(self._ctx, records))

    def filter_info(self) -> dict:
        out = (C.c_uint64 * 6)()
        self._check(self._lib.kta_filter_info(self._ctx, C.byref(out)))
        return {"seen": int(out[0]), "passed": int(out[1]), "tiles_summary_none": int(out[2]), "tiles_summary_all": int(out[3]),
                "tiles_read": int(out[4]), "slices": int(out[5])}

    def alive_export_entries(self) -> Tuple[int, int, int]:
        """(device ptr slots u32[n], device ptr values u64[n], n): the entries ever written."""
        ps, pv, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._check(self._lib.kta_alive_export_entries(self._ctx, C.byref(ps), C.byref(pv), C.byref(n)))
        return ps.value or 0, pv.value or 0, n.value

    def alive_export_entries_host(self) -> Tuple[np.ndarray, np.ndarray]:
        ps, pv, n = self.alive_export_entries()
        slots, vals = np.empty(n, np.uint32), np.empty(n, np.uint64)
        if n:
            self._check(self._lib.kta_copy_to_host(self._ctx, _np_ptr(slots), C.c_void_p(ps), slots.nbytes))
            self._check(self._lib.kta_copy_to_host(self._ctx, _np_ptr(vals), C.c_void_p(pv), vals.nbytes))
        return slots, vals

    def alive_import_entries(self, d_slots: int, d_vals: int, n: int) -> None:
        self._check(self._lib.kta_alive_import_entries(self._ctx, C.c_void_p(d_slots), C.c_void_p(d_vals), n))

    def alive_count_range(self, slot_lo: int, slot_hi: int) -> int:
        """Alive keys whose hash slot is in [slot_lo, slot_hi) (the owner's share of a hash range)."""
        n = C.c_uint64()
        self._check(self._lib.kta_alive_count_range(self._ctx, slot_lo, slot_hi, C.byref(n)))
        return n.value

    def alive_table_modified(self) -> None:
        self._check(self._lib.kta_alive_table_modified(self._ctx))

    def export_alive_bitmap(self) -> np.ndarray:
        """The alive set as a 2^32-bit bitmap: uint32[2^27], bit h%32 of word h//32."""
        bm = np.empty(1 << 27, dtype=np.uint32)
        self._check(self._lib.kta_export_alive_bitmap(self._ctx, _np_ptr(bm)))
        return bm

    def fnv32(self, keys) -> np.ndarray:
        """Hash a list of byte strings on the device with the reference FNV variant."""
        lens = np.array([len(k) for k in keys], dtype=np.int32)
        offs = np.zeros(len(keys), dtype=np.uint32)
        if len(keys):
            offs[1:] = np.cumsum(lens[:-1])
        blob = np.frombuffer(b"".join(keys), dtype=np.uint8).copy()
        out = np.zeros(len(keys), dtype=np.uint32)
        self._check(self._lib.kta_fnv32_device(self._ctx, _np_ptr(blob) if len(blob) else None, _np_ptr(offs),
                                               _np_ptr(lens), len(keys), len(blob), _np_ptr(out)))
        return out

    def set_timing(self, on: bool) -> None:
        self._check(self._lib.kta_set_timing(self._ctx, 1 if on else 0))

    def kernel_time_stats(self):
        """-> ([avg ms scan, fold, alive], [launch counts]) since the previous call (syncs)."""
        a, c = (C.c_float * 3)(), (C.c_uint64 * 3)()
        self._check(self._lib.kta_kernel_time_stats(self._ctx, C.byref(a), C.byref(c)))
        return list(a), list(c)

    def last_kernel_ms(self):
        return self.kernel_time_stats()[0]

    def set_tuning(self, scan_workgroups=0, scan_variant=16, alive_workgroups=0, alive_variant=3) -> None:
        self._check(self._lib.kta_set_tuning(self._ctx, scan_workgroups, scan_variant, alive_workgroups,
                                             alive_variant))

    # views with the reference's accessor names
    def set_fuse(self, on: bool) -> None:
        """Both handlers of a batch in one pass where possible (default) or always as two passes; same results."""
        self._check(self._lib.kta_set_fuse(self._ctx, 1 if on else 0))

    def alive_pass_info(self) -> dict:
        """Host-side counters of the partitioned alive-key pass since create / reset (kta_alive_pass_info)."""
        out = (C.c_uint64 * 6)()
        self._check(self._lib.kta_alive_pass_info(self._ctx, C.byref(out)))
        return {"slice": int(out[0]), "slices": int(out[1]), "fused": int(out[2]), "scanned": int(out[3]),
                "failed_buckets": int(out[4]), "fuse": bool(out[5])}

    def metrics(self) -> "MessageMetrics":
        res, counters = self.finish()
        return MessageMetrics(res, counters, self.now)

    def log_compaction(self) -> "LogCompactionInMemoryMetrics":
        res, _ = self.finish()
        return LogCompactionInMemoryMetrics(res)


class MessageMetrics:
    """Accessors of metric.rs:104-195 over a finished counter vector."""

    def __init__(self, res: KtaResult, counters: np.ndarray, now: Tuple[int, int]):
        self._c = counters
        self._res = res
        # metric.rs:39-40 sentinels merged with the device extrema exactly as
        # cmp_and_set_message_timestamp would have (metric.rs:65-72)
        self._earliest = now
        self._latest = (0, 0)
        if res.any_records:
            if self._earliest > (res.min_ts_sec, 0):
                self._earliest = (res.min_ts_sec, 0)
            if self._latest < (res.max_ts_sec, 0):
                self._latest = (res.max_ts_sec, 0)

    def _m(self, p: int, c: int) -> int:  # metric.rs:198-203
        return int(self._c[p, c]) if 0 <= p < self._c.shape[0] else 0

    def total(self, p): return self._m(p, N.KTA_C_TOTAL)
    def tombstones(self, p): return self._m(p, N.KTA_C_TOMBSTONES)
    def alive(self, p): return self._m(p, N.KTA_C_ALIVE)
    def key_null(self, p): return self._m(p, N.KTA_C_KEY_NULL)
    def key_non_null(self, p): return self._m(p, N.KTA_C_KEY_NON_NULL)
    def key_size_sum(self, p): return self._m(p, N.KTA_C_KEY_SIZE_SUM)
    def value_size_sum(self, p): return self._m(p, N.KTA_C_VALUE_SIZE_SUM)

    def _avg(self, s: int, p: int) -> int:  # metric.rs:132-157
        if s > 0:
            if self.alive(p) == 0:
                raise DivideByZeroPanic("attempt to divide by zero")
            return s // self.alive(p)
        return 0

    def key_size_avg(self, p): return self._avg(self.key_size_sum(p), p)
    def value_size_avg(self, p): return self._avg(self.value_size_sum(p), p)
    def message_size_avg(self, p): return self._avg(self.key_size_sum(p) + self.value_size_sum(p), p)

    def dirty_ratio(self, p) -> float:  # metric.rs:159-167, f32 with two roundings
        t, tm = self.tombstones(p), self.total(p)
        if tm > 0 and t > 0:
            return float(np.float32(t) / (np.float32(tm) / np.float32(100.0)))
        return 0.0

    def earliest_message(self): return self._earliest
    def latest_message(self): return self._latest

    def smallest_message(self) -> int:  # metric.rs:177-183
        s = int(self._res.smallest_message)
        return 0 if s == U64_MAX else s

    def largest_message(self) -> int: return int(self._res.largest_message)
    def overall_count(self) -> int: return int(self._res.overall_count)
    def overall_size(self) -> int: return int(self._res.overall_size)


class LogCompactionInMemoryMetrics:
    def __init__(self, res: KtaResult):
        self._res = res

    def sum_all_alive(self) -> int:  # metric.rs:282-284
        return int(self._res.alive_keys)


# ---------------------------------------------------------------------- analytics vectors (host side)
_PART_KEYS = ("part_min_ts_sec", "part_max_ts_sec", "part_smallest", "part_largest")


def _analytics_arrays(P: int) -> dict:
    return {"part_min_ts_sec": np.zeros(P, np.int64), "part_max_ts_sec": np.zeros(P, np.int64),
            "part_smallest": np.zeros(P, np.uint64), "part_largest": np.zeros(P, np.uint64)}


def _analytics_dict(a: "N.KtaAnalytics", parts: dict) -> dict:
    return {"key_size_hist": np.array(a.key_size_hist[:], dtype=np.uint64),
            "value_size_hist": np.array(a.value_size_hist[:], dtype=np.uint64), **parts}


def decode_analytics(vec, n_partitions: int) -> dict:
    """kta_decode_analytics: an analytics vector u64[2*34 + 4*P] -> the dict HipMetricHandler.analytics() returns."""
    v = _section_vec("analytics", vec, n_partitions)
    a = N.KtaAnalytics()
    out = _analytics_arrays(n_partitions)
    rc = N.load().kta_decode_analytics(_np_ptr(v), n_partitions, C.byref(a), *[_np_ptr(out[k]) for k in _PART_KEYS])
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_decode_analytics")
    return _analytics_dict(a, out)


def merge_analytics(acc: np.ndarray, other, n_partitions: int) -> np.ndarray:
    """kta_merge_analytics, in place on `acc` (uint64 or int64): SUM over the histograms, signed MAX over the extrema."""
    return _merge("analytics", acc, other, n_partitions)


def _render(fn, *args) -> str:
    """A two-call renderer `fn(*args, buf, cap, &needed)`: ask for the size, allocate, call again."""
    n = C.c_size_t()
    buf = None
    for _ in range(2):
        rc = fn(*args, buf, len(buf) if buf else 0, C.byref(n))
        if rc != N.KTA_OK:
            raise KtaError(rc, fn.__name__)
        buf = buf or C.create_string_buffer(n.value + 1)
    return buf.value.decode()


def render_analytics(vec, n_partitions: int) -> str:
    """kta_render_analytics: the section kta-analyzer prints after the report with --librdkafka kta.analytics=1."""
    v = _section_vec("analytics", vec, n_partitions)
    return _render(N.load().kta_render_analytics, _np_ptr(v), n_partitions)


def analytics_max_partitions() -> int:
    """The largest P a context with analytics may have (the analytics scan's LDS plan on gfx950)."""
    return int(N.load().kta_analytics_max_partitions())


def render_timeline(vec, origin_ms: int, bucket_ms: int, n_buckets: int) -> str:
    """kta_render_timeline: the section kta-analyzer prints after the report with --librdkafka kta.timeline=<width>,
    from a timeline vector (u64[(n_buckets + 3) * 3], or its [n_buckets + 3, 3] shape)."""
    v = _section_vec("timeline", vec, n_buckets)
    return _render(N.load().kta_render_timeline, _np_ptr(v), origin_ms, bucket_ms, n_buckets)


def timeline_max_partitions(n_buckets: int, analytics: bool = False) -> int:
    """The largest P a context (with analytics or not) may have with a timeline of n_buckets buckets."""
    return int(N.load().kta_timeline_max_partitions(N.KTA_FLAG_ANALYTICS if analytics else 0, n_buckets))


def estimate_distinct_keys(vec, n_partitions: int) -> Tuple[np.ndarray, float]:
    """kta_key_sketch_estimate: a key sketch (u64[P * 4096] or [P, 4096]) -> (per-partition estimates float64[P], the
    topic-wide estimate of the register-wise max over the partitions)."""
    v = _section_vec("key_sketch", vec, n_partitions)
    per = np.zeros(n_partitions, np.float64)
    topic = C.c_double()
    rc = N.load().kta_key_sketch_estimate(_np_ptr(v), n_partitions, _np_ptr(per), C.byref(topic))
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_key_sketch_estimate")
    return per, topic.value


def merge_key_sketch(acc: np.ndarray, other, n_partitions: int) -> np.ndarray:
    """kta_merge_key_sketch, in place on `acc` (contiguous uint64 / int64): the register-wise max."""
    return _merge("key_sketch", acc, other, n_partitions)


def render_distinct_keys(sketch_vec, counter_vec, n_partitions: int) -> str:
    """kta_render_distinct_keys: the section kta-analyzer prints after the report with --librdkafka kta.distinct_keys=1,
    from a key sketch and the counter vector u64[P * 7 + 8] of the same records."""
    v, c = _section_vec("key_sketch", sketch_vec, n_partitions), _counter_vec(counter_vec, n_partitions)
    return _render(N.load().kta_render_distinct_keys, _np_ptr(v), _np_ptr(c), n_partitions)


HOT_EXEMPLAR_DTYPE = np.dtype([("hash", np.uint32), ("key_len", np.uint32), ("valid", np.uint32), ("pad", np.uint32),
                               ("bytes", np.uint8, (N.KTA_HOT_EXEMPLAR_BYTES,))])


def recover_hot_keys(vec, max_keys: int = N.KTA_HOT_MAX_REPORTED) -> Tuple[list, int]:
    """kta_hot_keys_recover: a hot-key vector -> ([(hash, upper, lower), ...] by upper descending then hash, at most
    max_keys of them, the keyed records)."""
    v = _section_vec("hot_keys", vec)
    out = (N.KtaHotKey * max(int(max_keys), 1))()
    n, keyed = C.c_uint32(), C.c_uint64()
    rc = N.load().kta_hot_keys_recover(_np_ptr(v), int(max_keys), C.byref(out), C.byref(n), C.byref(keyed))
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_hot_keys_recover")
    return [(int(out[k].hash), int(out[k].upper), int(out[k].lower)) for k in range(n.value)], int(keyed.value)


def merge_hot_keys(acc: np.ndarray, other) -> np.ndarray:
    """kta_merge_hot_keys, in place on `acc` (contiguous uint64 / int64): the word-wise sum."""
    return _merge("hot_keys", acc, other)


def render_hot_keys(vec, exemplars=None, max_keys: int = 10) -> str:
    """kta_render_hot_keys: the section kta-analyzer prints last with --librdkafka kta.hot_keys=K, from a hot-key vector
    and an exemplar table (HipMetricHandler.hot_key_exemplars(), or None)."""
    v = _section_vec("hot_keys", vec)
    ex = None
    if exemplars is not None:
        ex = np.ascontiguousarray(exemplars, dtype=HOT_EXEMPLAR_DTYPE)
        if ex.size != N.KTA_HOT_ROWS * N.KTA_HOT_CELLS:
            raise ValueError("an exemplar table has 2048 slots")
    return _render(N.load().kta_render_hot_keys, _np_ptr(v), _np_ptr(ex) if ex is not None else None, int(max_keys))


def split_ts_order(vec, n_partitions: int) -> dict:
    """A timestamp-order vector u64[3 P + 64] as a dict: late[P], late_ms_sum[P], hist[63], timed, max_late_ms[P], and the
    vector itself under "vector"."""
    P = n_partitions
    v = _section_vec("ts_order", vec, P)
    return {"late": v[0:2 * P:2].copy(), "late_ms_sum": v[1:2 * P:2].copy(), "hist": v[2 * P:2 * P + N.KTA_TS_ORDER_HIST].copy(),
            "timed": int(v[2 * P + N.KTA_TS_ORDER_HIST]), "max_late_ms": v[2 * P + 64:].copy(), "vector": v}


def merge_ts_order(acc: np.ndarray, other, n_partitions: int) -> np.ndarray:
    """kta_merge_ts_order, in place on `acc` (contiguous uint64 / int64): SUM over the first 2 P + 64 words, MAX over the
    last P.  Exact when every partition's records went through one of the two contexts, in order."""
    return _merge("ts_order", acc, other, n_partitions)


def render_ts_order(vec, counter_vec, n_partitions: int) -> str:
    """kta_render_ts_order: the section kta-analyzer prints with --librdkafka kta.ts_order=1, from a timestamp-order vector
    and the counter vector u64[P * 7 + 8] of the same records."""
    v, c = _section_vec("ts_order", vec, n_partitions), _counter_vec(counter_vec, n_partitions)
    return _render(N.load().kta_render_ts_order, _np_ptr(v), _np_ptr(c), n_partitions)


def split_partitioner(vec, n_partitions: int, repartition: int) -> dict:
    """A partitioner vector u64[2 P + 2 Q] as a dict: checked[P], placed[P], target_records[Q], target_bytes[Q], and the
    vector itself under "vector"."""
    P = n_partitions
    v = _section_vec("partitioner", vec, P, repartition)
    return {"checked": v[0:2 * P:2].copy(), "placed": v[1:2 * P:2].copy(), "target_records": v[2 * P::2].copy(),
            "target_bytes": v[2 * P + 1::2].copy(), "vector": v}


def merge_partitioner(acc: np.ndarray, other, n_partitions: int, repartition: int) -> np.ndarray:
    """kta_merge_partitioner, in place on `acc` (contiguous uint64 / int64): every word a sum."""
    return _merge("partitioner", acc, other, n_partitions, repartition)


def render_partitioner(vec, counter_vec, n_partitions: int, repartition: int) -> str:
    """kta_render_partitioner: the section kta-analyzer prints with --librdkafka kta.partitioner=murmur2, from a partitioner
    vector and the counter vector u64[P * 7 + 8] of the same records."""
    v, c = _section_vec("partitioner", vec, n_partitions, repartition), _counter_vec(counter_vec, n_partitions)
    return _render(N.load().kta_render_partitioner, _np_ptr(v), _np_ptr(c), n_partitions, repartition)


def split_size_quantiles(vec, n_partitions: int) -> dict:
    """A size vector u64[P * 3 * 464 + 8] as a dict: key[P][464], value[P][464], message[P][464], the globals records,
    bad_partition, keyed, alive, and the vector itself under "vector"."""
    P = n_partitions
    v = _section_vec("size_quantiles", vec, P)
    h = v[:P * N.KTA_SIZE_QUANTITIES * N.KTA_SIZE_BINS].reshape(P, N.KTA_SIZE_QUANTITIES, N.KTA_SIZE_BINS)
    g = v[P * N.KTA_SIZE_QUANTITIES * N.KTA_SIZE_BINS:]
    return {"key": h[:, 0, :].copy(), "value": h[:, 1, :].copy(), "message": h[:, 2, :].copy(), "records": int(g[0]),
            "bad_partition": int(g[1]), "keyed": int(g[2]), "alive": int(g[3]), "vector": v}


def merge_size_quantiles(acc: np.ndarray, other, n_partitions: int) -> np.ndarray:
    """kta_merge_size_quantiles, in place on `acc` (contiguous uint64 / int64): every word a sum."""
    return _merge("size_quantiles", acc, other, n_partitions)


def render_size_percentiles(vec, counter_vec, n_partitions: int) -> str:
    """kta_render_size_percentiles: the section kta-analyzer prints with --librdkafka kta.percentiles=1, from a size vector
    and the counter vector u64[P * 7 + 8] of the same records (KtaError when the two do not describe the same records)."""
    v, c = _section_vec("size_quantiles", vec, n_partitions), _counter_vec(counter_vec, n_partitions)
    return _render(N.load().kta_render_size_percentiles, _np_ptr(v), _np_ptr(c), n_partitions)


RECORD_BATCH_COLUMNS = ("batches", "records", "wire", "payload", "compressed", "compressed_recbytes", "compressed_payload", "extent",
                        "transactional", "idempotent", "log_append_time", "span_ms", "failed")
RECORD_BATCH_CODECS = ("none", "gzip", "snappy", "lz4", "zstd")


def split_record_batches(vec, n_partitions: int) -> dict:
    """A record-batch vector u64[20 P + 1524] as a dict, split by its layout (kta_hip.h, above KTA_FLAG_RECORD_BATCHES):
    "partitions" [P][16] (columns RECORD_BATCH_COLUMNS, then three zeros); "codecs" [5][4] batches, records, recbytes,
    payload (rows RECORD_BATCH_CODECS) with "hist_records", "hist_wire" and "hist_span" [5][32]; "maxima" [P][4] the largest
    n_records, wire, leader epoch + 1 and span_ms; "sketch" [1024]; "producers" the estimate; the vector under "vector"."""
    P = n_partitions
    v = _section_vec("record_batches", vec, P)
    c = v[16 * P:16 * P + 500].reshape(N.KTA_RB_CODECS, N.KTA_RB_CODEC_WORDS)
    return {"partitions": v[:16 * P].reshape(P, 16).copy(), "codecs": c[:, :4].copy(), "hist_records": c[:, 4:36].copy(),
            "hist_wire": c[:, 36:68].copy(), "hist_span": c[:, 68:100].copy(),
            "maxima": v[16 * P + 500:20 * P + 500].reshape(P, 4).copy(), "sketch": v[20 * P + 500:].copy(),
            "producers": estimate_producers(v, P), "vector": v}


def merge_record_batches(acc: np.ndarray, other, n_partitions: int) -> np.ndarray:
    """kta_merge_record_batches, in place on `acc` (contiguous uint64 / int64): sums over the first 16 P + 500 words, unsigned
    maxima behind them."""
    return _merge("record_batches", acc, other, n_partitions)


def estimate_producers(vec, n_partitions: int) -> float:
    """kta_record_batches_estimate_producers: the distinct producer ids read off a record-batch vector's sketch (standard
    error 3.25 %; exact linear counting while few registers are set)."""
    out = C.c_double()
    rc = N.load().kta_record_batches_estimate_producers(_np_ptr(_section_vec("record_batches", vec, n_partitions)), n_partitions, C.byref(out))
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_record_batches_estimate_producers")
    return float(out.value)


def record_batches_identities(vec, n_partitions: int) -> bool:
    """kta_record_batches_identities: whether the identities between the words of one record-batch vector hold."""
    rc = N.load().kta_record_batches_identities(_np_ptr(_section_vec("record_batches", vec, n_partitions)), n_partitions)
    if rc < 0:
        raise KtaError(rc, "kta_record_batches_identities")
    return rc == 1


def record_batches_host(blob: bytes, partition: int, n_partitions: int, inflated=None, vec=None) -> np.ndarray:
    """kta_record_batches_host: the section's rule over the batches of `blob` on the host, added to `vec` (a new vector when
    None).  inflated: the exact inflated size of every batch that gets a descriptor, or None for the index's own value."""
    v = np.zeros(_section_words("record_batches", n_partitions), np.uint64) if vec is None else _section_vec("record_batches", vec, n_partitions)
    inf = None if inflated is None else np.ascontiguousarray(inflated, np.uint64)
    rc = N.load().kta_record_batches_host(bytes(blob), len(blob), int(partition), None if inf is None else _np_ptr(inf), _np_ptr(v), n_partitions)
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_record_batches_host")
    return v


def render_record_batches(vec, n_partitions: int, filtered: bool = False, skipped=None) -> str:
    """kta_render_record_batches: the section kta-analyzer prints with --librdkafka kta.record_batches=1.  skipped: the
    host index's (control batches, magic 0/1 sets, unknown codecs) over the run, zeros when None."""
    v = _section_vec("record_batches", vec, n_partitions)
    sk = None if skipped is None else np.ascontiguousarray(skipped, np.uint64)
    if sk is not None and sk.size != 3:
        raise ValueError("skipped has three words: control batches, magic 0/1 sets, unknown codecs")
    return _render(N.load().kta_render_record_batches, _np_ptr(v), n_partitions, 1 if filtered else 0, None if sk is None else _np_ptr(sk))


PAYLOAD_CLASSES = ("null", "empty", "framed", "json", "other")
PAYLOAD_COLUMNS = ("records",) + PAYLOAD_CLASSES + tuple(c + "_bytes" for c in PAYLOAD_CLASSES) + \
    ("with_headers", "headers", "header_key_bytes", "header_value_bytes", "header_null_values", "bad_headers", "header_wire_bytes")


def split_payload(vec, n_partitions: int) -> dict:
    """A payload vector u64[24 P + 16 + 2 * 1024 * 34] as a dict, split by its layout (kta_hip.h, above KTA_FLAG_PAYLOAD):
    "partitions" [P][24] (columns PAYLOAD_COLUMNS, then six zeros); "headers_hist" [16]; "table" [2][1024][34] (T, B, 32 bit
    counters); "schema_ids" what payload_schema_ids reads off it; the vector under "vector"."""
    P = n_partitions
    v = _section_vec("payload", vec, P)
    return {"partitions": v[:24 * P].reshape(P, 24).copy(), "headers_hist": v[24 * P:24 * P + 16].copy(),
            "table": v[24 * P + 16:].reshape(2, 1024, 34).copy(), "schema_ids": payload_schema_ids(v, P), "vector": v}


def merge_payload(acc: np.ndarray, other, n_partitions: int) -> np.ndarray:
    """kta_merge_payload, in place on `acc` (contiguous uint64 / int64): every word a sum."""
    return _merge("payload", acc, other, n_partitions)


def payload_identities(vec, n_partitions: int, counter_vec=None) -> bool:
    """kta_payload_identities: whether the identities between the words of one payload vector hold; with counter_vec (the
    counter vector u64[7 P + 8] of the same unfiltered run without failed batches) also records == total_messages and
    null == tombstones per partition."""
    c = None if counter_vec is None else np.ascontiguousarray(counter_vec, np.uint64)
    if c is not None and c.size != 7 * n_partitions + 8:
        raise ValueError(f"a counter vector of {n_partitions} partitions has {7 * n_partitions + 8} words, not {c.size}")
    rc = N.load().kta_payload_identities(_np_ptr(_section_vec("payload", vec, n_partitions)), None if c is None else _np_ptr(c), n_partitions)
    if rc < 0:
        raise KtaError(rc, "kta_payload_identities")
    return rc == 1


def payload_schema_ids(vec, n_partitions: int) -> dict:
    """kta_payload_schema_ids: the schema ids read off a payload vector's table — "ids" [(id, records, bytes)] sorted by
    records (most first), exact; "unresolved_records" / "unresolved_bytes": what remains in cells that hold several ids."""
    v = _section_vec("payload", vec, n_partitions)
    lib, n, ur, ub = N.load(), C.c_size_t(), C.c_uint64(), C.c_uint64()
    rc = lib.kta_payload_schema_ids(_np_ptr(v), n_partitions, None, None, None, 0, C.byref(n), C.byref(ur), C.byref(ub))
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_payload_schema_ids")
    cap = max(n.value, 1)
    ids, rec, byt = np.zeros(cap, np.uint32), np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
    rc = lib.kta_payload_schema_ids(_np_ptr(v), n_partitions, _np_ptr(ids), _np_ptr(rec), _np_ptr(byt), cap, C.byref(n), C.byref(ur), C.byref(ub))
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_payload_schema_ids")
    return {"ids": [(int(ids[i]), int(rec[i]), int(byt[i])) for i in range(n.value)], "unresolved_records": int(ur.value),
            "unresolved_bytes": int(ub.value)}


def payload_host(blob: bytes, partition: int, n_partitions: int, vec=None) -> np.ndarray:
    """kta_payload_host: the section's rule over the records of `blob` on the host (compressed batches inflated), added to
    `vec` (a new vector when None)."""
    v = np.zeros(_section_words("payload", n_partitions), np.uint64) if vec is None else _section_vec("payload", vec, n_partitions)
    rc = N.load().kta_payload_host(bytes(blob), len(blob), int(partition), _np_ptr(v), n_partitions)
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_payload_host")
    return v


def render_payload(vec, n_partitions: int, counter_vec=None) -> str:
    """kta_render_payload: the section kta-analyzer prints with --librdkafka kta.payload=1.  counter_vec: the counter vector
    (its key and value size sums give the header bytes' share), `n/a` in that column when None."""
    v = _section_vec("payload", vec, n_partitions)
    c = None if counter_vec is None else np.ascontiguousarray(counter_vec, np.uint64)
    if c is not None and c.size != 7 * n_partitions + 8:
        raise ValueError(f"a counter vector of {n_partitions} partitions has {7 * n_partitions + 8} words, not {c.size}")
    return _render(N.load().kta_render_payload, _np_ptr(v), None if c is None else _np_ptr(c), n_partitions)


HEADER_NAMES_GLOBALS = ("occurrences", "name_bytes", "value_bytes", "null_values", "with_headers", "looked")
HEADER_NAME_DTYPE = np.dtype([("hash", np.uint32), ("name_len", np.uint32), ("state", np.uint32), ("reserved", np.uint32),
                              ("bytes", np.uint8, (N.KTA_HEADER_NAME_BYTES,))])
_HEADER_NAME_ROW_DTYPE = np.dtype([("hash", np.uint32), ("has_name", np.uint32), ("occurrences", np.uint64), ("name_len", np.uint64),
                                   ("value_bytes", np.uint64), ("null_values", np.uint64), ("name", np.uint8, (N.KTA_HEADER_NAME_BYTES,))])


def _name_table(table) -> Optional[np.ndarray]:
    if table is None:
        return None
    t = np.ascontiguousarray(table, dtype=HEADER_NAME_DTYPE).reshape(-1)
    if t.size != N.KTA_HEADER_NAMES_SLOTS:
        raise ValueError(f"a name table has {N.KTA_HEADER_NAMES_SLOTS} slots, not {t.size}")
    return t


def split_header_names(vec, table=None) -> dict:
    """A header-name vector u64[8 + 2 * 1024 * 36] as a dict, split by its layout (kta_hip.h, above KTA_FLAG_HEADER_NAMES): the
    six globals by HEADER_NAMES_GLOBALS; "table" [2][1024][36] (T, L, V, Z, 32 bit counters); "names" what header_names_list
    reads off it with the name table `table` (or None); the vector under "vector"."""
    v = _section_vec("header_names", vec)
    out = {name: int(v[i]) for i, name in enumerate(HEADER_NAMES_GLOBALS)}
    out.update({"table": v[N.KTA_HEADER_NAMES_GLOBALS:].reshape(2, 1024, 36).copy(), "names": header_names_list(v, table), "vector": v})
    return out


def merge_header_names(acc: np.ndarray, other) -> np.ndarray:
    """kta_merge_header_names, in place on `acc` (contiguous uint64 / int64): every word a sum."""
    return _merge("header_names", acc, other)


def header_names_identities(vec, payload_vec=None, n_partitions: int = 0) -> bool:
    """kta_header_names_identities: whether the identities between the words of one header-name vector hold; with payload_vec
    (the payload vector of the same run, of n_partitions partitions) also those between the two sections."""
    p = None if payload_vec is None else _section_vec("payload", payload_vec, n_partitions)
    rc = N.load().kta_header_names_identities(_np_ptr(_section_vec("header_names", vec)), None if p is None else _np_ptr(p), n_partitions)
    if rc < 0:
        raise KtaError(rc, "kta_header_names_identities")
    return rc == 1


def header_names_list(vec, table=None) -> dict:
    """kta_header_names_list: the names read off a header-name vector's table — "names" [(hash, occurrences, name length,
    value bytes, null values, name)] sorted by occurrences (most first), value bytes, hash; exact; name: the first 48 bytes at
    most, or None without a published slot in `table`; "unresolved_occurrences" / "unresolved_value_bytes": what remains in
    cells that hold several names."""
    v, t = _section_vec("header_names", vec), _name_table(table)
    lib, n, uo, ub = N.load(), C.c_size_t(), C.c_uint64(), C.c_uint64()
    tp = None if t is None else _np_ptr(t)
    rc = lib.kta_header_names_list(_np_ptr(v), tp, None, 0, C.byref(n), C.byref(uo), C.byref(ub))
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_header_names_list")
    rows = np.zeros(max(n.value, 1), dtype=_HEADER_NAME_ROW_DTYPE)
    rc = lib.kta_header_names_list(_np_ptr(v), tp, _np_ptr(rows), rows.size, C.byref(n), C.byref(uo), C.byref(ub))
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_header_names_list")
    names = [(int(r["hash"]), int(r["occurrences"]), int(r["name_len"]), int(r["value_bytes"]), int(r["null_values"]),
              bytes(r["name"][:min(int(r["name_len"]), N.KTA_HEADER_NAME_BYTES)]) if r["has_name"] else None) for r in rows[:n.value]]
    return {"names": names, "unresolved_occurrences": int(uo.value), "unresolved_value_bytes": int(ub.value)}


def header_names_host(blob: bytes, partition: int, n_partitions: int, vec=None, table=None):
    """kta_header_names_host: the section's rule over the records of `blob` on the host (compressed batches inflated), added to
    `vec` and `table` (new ones when None).  Returns (vec, table)."""
    v = np.zeros(N.KTA_HEADER_NAMES_WORDS, np.uint64) if vec is None else _section_vec("header_names", vec)
    t = np.zeros(N.KTA_HEADER_NAMES_SLOTS, dtype=HEADER_NAME_DTYPE) if table is None else _name_table(table)
    rc = N.load().kta_header_names_host(bytes(blob), len(blob), int(partition), _np_ptr(v), _np_ptr(t), n_partitions)
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_header_names_host")
    return v, t


def render_header_names(vec, table=None, max_names: int = 256) -> str:
    """kta_render_header_names: the section kta-analyzer prints with --librdkafka kta.headers=1."""
    t = _name_table(table)
    return _render(N.load().kta_render_header_names, _np_ptr(_section_vec("header_names", vec)), None if t is None else _np_ptr(t), int(max_names))


VALUE_BYTES_CLASSES = ("none", "text", "dense", "binary")


def value_bytes_summary(words) -> dict:
    """kta_value_bytes_summary: the read-off of one partition's 264 words of a value-byte vector, or of their sum over the
    topic: records, values, bytes, repeats, distinct, entropy_bits (H0), floor_bytes, printable, zero, high, top_byte,
    top_count and class (a heuristic: one of VALUE_BYTES_CLASSES)."""
    w = _u64_vec(words, N.KTA_VALUE_BYTES_PARTITION_WORDS, "the words of one partition of a value-byte vector")
    out = N.KtaValueBytesSummary()
    rc = N.load().kta_value_bytes_summary(_np_ptr(w), C.byref(out))
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_value_bytes_summary")
    d = {name: getattr(out, name) for name, _ in N.KtaValueBytesSummary._fields_ if name != "cls"}
    d["class"] = VALUE_BYTES_CLASSES[out.cls]
    return d


def split_value_bytes(vec, n_partitions: int) -> dict:
    """A value-byte vector u64[264 P] as a dict, split by its layout (kta_hip.h, above KTA_FLAG_VALUE_BYTES): "partitions"
    [P][264] (256 bins, records, values, bytes, repeats, four zeros); "summaries" [P] and "topic" what value_bytes_summary reads
    off each partition and off their sum; the vector under "vector"."""
    P = n_partitions
    v = _section_vec("value_bytes", vec, P)
    parts = v.reshape(P, N.KTA_VALUE_BYTES_PARTITION_WORDS).copy()
    return {"partitions": parts, "summaries": [value_bytes_summary(parts[p]) for p in range(P)],
            "topic": value_bytes_summary(parts.sum(axis=0, dtype=np.uint64)), "vector": v}


def merge_value_bytes(acc: np.ndarray, other, n_partitions: int) -> np.ndarray:
    """kta_merge_value_bytes, in place on `acc` (contiguous uint64 / int64): every word a sum."""
    return _merge("value_bytes", acc, other, n_partitions)


def value_bytes_identities(vec, n_partitions: int, payload_vec=None, counter_vec=None) -> bool:
    """kta_value_bytes_identities: whether the identities between the words of one value-byte vector hold; with payload_vec
    (the payload vector of the same run) also those between the two sections; with counter_vec (the counter vector
    u64[7 P + 8] of the same unfiltered run without failed batches) also records == total_messages per partition."""
    p = None if payload_vec is None else _section_vec("payload", payload_vec, n_partitions)
    c = None if counter_vec is None else _counter_vec(counter_vec, n_partitions)
    rc = N.load().kta_value_bytes_identities(_np_ptr(_section_vec("value_bytes", vec, n_partitions)), n_partitions,
                                             None if p is None else _np_ptr(p), None if c is None else _np_ptr(c))
    if rc < 0:
        raise KtaError(rc, "kta_value_bytes_identities")
    return rc == 1


def value_bytes_host(blob: bytes, partition: int, n_partitions: int, vec=None) -> np.ndarray:
    """kta_value_bytes_host: the section's rule over the records of `blob` on the host (compressed batches inflated), added to
    `vec` (a new vector when None)."""
    v = np.zeros(_section_words("value_bytes", n_partitions), np.uint64) if vec is None else _section_vec("value_bytes", vec, n_partitions)
    rc = N.load().kta_value_bytes_host(bytes(blob), len(blob), int(partition), _np_ptr(v), n_partitions)
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_value_bytes_host")
    return v


def render_value_bytes(vec, n_partitions: int) -> str:
    """kta_render_value_bytes: the section kta-analyzer prints with --librdkafka kta.value_bytes=1."""
    return _render(N.load().kta_render_value_bytes, _np_ptr(_section_vec("value_bytes", vec, n_partitions)), n_partitions)


COMPRESS_WHATIF_COLUMNS = ("batches", "blocks", "stored_blocks", "raw_bytes", "now_bytes", "model_bytes", "sequences", "match_bytes")
COMPRESS_WHATIF_CODECS = ("none", "gzip", "snappy", "lz4", "zstd")
COMPRESS_WHATIF_CODEC_COLUMNS = ("batches", "raw_bytes", "now_bytes", "model_bytes")


def split_compress_whatif(vec, n_partitions: int) -> dict:
    """A compression what-if vector u64[8 P + 20] as a dict, split by its layout (kta_hip.h, above KTA_FLAG_COMPRESS_WHATIF):
    "partitions" [P][8] (COMPRESS_WHATIF_COLUMNS), "topic" [8] their sum, "codecs" [5][4] (COMPRESS_WHATIF_CODECS by
    COMPRESS_WHATIF_CODEC_COLUMNS); the vector under "vector"."""
    P = n_partitions
    v = _section_vec("compress_whatif", vec, P)
    pw = N.KTA_COMPRESS_WHATIF_PARTITION_WORDS
    parts = v[:pw * P].reshape(P, pw).copy()
    return {"partitions": parts, "topic": parts.sum(axis=0, dtype=np.uint64),
            "codecs": v[pw * P:].reshape(N.KTA_COMPRESS_WHATIF_CODECS, N.KTA_COMPRESS_WHATIF_CODEC_WORDS).copy(), "vector": v}


def merge_compress_whatif(acc: np.ndarray, other, n_partitions: int) -> np.ndarray:
    """kta_merge_compress_whatif, in place on `acc` (contiguous uint64 / int64): every word a sum."""
    return _merge("compress_whatif", acc, other, n_partitions)


def compress_whatif_identities(vec, n_partitions: int) -> bool:
    """kta_compress_whatif_identities: whether the identities between the words of one what-if vector hold."""
    rc = N.load().kta_compress_whatif_identities(_np_ptr(_section_vec("compress_whatif", vec, n_partitions)), n_partitions)
    if rc < 0:
        raise KtaError(rc, "kta_compress_whatif_identities")
    return rc == 1


def compress_whatif_host(blob: bytes, partition: int, n_partitions: int, vec=None) -> np.ndarray:
    """kta_compress_whatif_host: the section's rule over the batches of `blob` on the host (compressed batches inflated), added
    to `vec` (a new vector when None)."""
    v = np.zeros(_section_words("compress_whatif", n_partitions), np.uint64) if vec is None else _section_vec("compress_whatif", vec, n_partitions)
    rc = N.load().kta_compress_whatif_host(bytes(blob), len(blob), int(partition), _np_ptr(v), n_partitions)
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_compress_whatif_host")
    return v


def render_compress_whatif(vec, n_partitions: int) -> str:
    """kta_render_compress_whatif: the section kta-analyzer prints with --librdkafka kta.compress_whatif=lz4."""
    return _render(N.load().kta_render_compress_whatif, _np_ptr(_section_vec("compress_whatif", vec, n_partitions)), n_partitions)


def lz4_model_size(data: bytes) -> int:
    """kta_lz4_model_host without a destination: the size of the model compressor's frame of `data` (one records section)."""
    data = bytes(data)
    n = int(N.load().kta_lz4_model_host(data, len(data), None, 0))
    if n < 0:
        raise KtaError(N.KTA_ERR_INVALID, "kta_lz4_model_host")
    return n


def lz4_model(data: bytes) -> bytes:
    """kta_lz4_model_host: the model compressor's frame of `data` (one records section), an LZ4 frame any decoder reads."""
    data = bytes(data)
    n = lz4_model_size(data)
    out = (C.c_uint8 * n)()
    got = int(N.load().kta_lz4_model_host(data, len(data), out, n))
    if got != n:
        raise KtaError(N.KTA_ERR_INVALID, "kta_lz4_model_host")
    return bytes(out)


def size_bin(size: int) -> int:
    """kta_size_bin: the bin, 0 .. 463, of a size 0 .. 2^32 - 1."""
    return int(N.load().kta_size_bin(int(size)))


def size_bin_bounds(b: int) -> Tuple[int, int]:
    """kta_size_bin_bounds: the least and the largest size of bin b."""
    lo, hi = C.c_uint64(), C.c_uint64()
    rc = N.load().kta_size_bin_bounds(int(b), C.byref(lo), C.byref(hi))
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_size_bin_bounds")
    return int(lo.value), int(hi.value)


def size_quantile(hist, num: int, den: int) -> Optional[Tuple[int, int]]:
    """kta_size_quantile: the bounds (lo, hi) of the bin that holds the num/den quantile of a histogram u64[464] by nearest
    rank; None for an empty histogram."""
    h = np.ascontiguousarray(np.asarray(hist).reshape(-1), np.uint64)
    if h.size != N.KTA_SIZE_BINS:
        raise ValueError(f"a size histogram has {N.KTA_SIZE_BINS} bins, not {h.size}")
    lo, hi = C.c_uint64(), C.c_uint64()
    rc = N.load().kta_size_quantile(_np_ptr(h), int(num), int(den), C.byref(lo), C.byref(hi))
    if rc < 0:
        raise KtaError(rc, "kta_size_quantile")
    return (int(lo.value), int(hi.value)) if rc == 1 else None


def size_quantiles_max_partitions() -> int:
    """The largest P of a context with the size-percentile pass."""
    return int(N.load().kta_size_quantiles_max_partitions())


class _CompactionReplay:
    """What HipMetricHandler.compaction_replay returns: as a context manager it turns replay mode off at the end."""

    def __init__(self, handler):
        self._h = handler

    def __enter__(self):
        return self._h

    def __exit__(self, *exc):
        self._h.compaction_replay(False)
        return False


_COMPACTION_GLOBALS = ("replayed", "unkeyed", "unknown", "live_outside", "tombstones_outside")


def split_compaction(vec, n_partitions: int) -> dict:
    """A compaction vector u64[5 P + 6] as a dict: live_records[P], live_key_bytes[P], live_value_bytes[P],
    tombstone_records[P], tombstone_key_bytes[P], the globals replayed, unkeyed, unknown, live_outside, tombstones_outside as
    ints, and the vector itself under "vector"."""
    P, W = n_partitions, N.KTA_COMPACTION_WORDS
    v = _section_vec("compaction", vec, P)
    d = {name: v[k:W * P:W].copy() for k, name in enumerate(("live_records", "live_key_bytes", "live_value_bytes", "tombstone_records",
                                                              "tombstone_key_bytes"))}
    d.update({name: int(v[W * P + k]) for k, name in enumerate(_COMPACTION_GLOBALS)})
    d["vector"] = v
    return d


def render_compaction(vec, counter_vec, n_partitions: int) -> str:
    """kta_render_compaction: the section kta-analyzer prints with -c --librdkafka kta.compaction=1, from a compaction vector
    and the first pass's counter vector u64[P * 7 + 8].  KtaError (KTA_ERR_INVALID) when the replay did not match the first
    pass; the section that says so is the error's `text`."""
    v, c = _section_vec("compaction", vec, n_partitions), _counter_vec(counter_vec, n_partitions)
    fn = N.load().kta_render_compaction
    n = C.c_size_t()
    fn(_np_ptr(v), _np_ptr(c), n_partitions, None, 0, C.byref(n))
    buf = C.create_string_buffer(n.value + 1)
    rc = fn(_np_ptr(v), _np_ptr(c), n_partitions, buf, len(buf), C.byref(n))
    if rc != N.KTA_OK:
        err = KtaError(rc, "kta_render_compaction: the replay did not match the first pass")
        err.text = buf.value.decode()
        raise err
    return buf.value.decode()


def compaction_max_partitions() -> int:
    """The largest P of a context with the compaction what-if."""
    return int(N.load().kta_compaction_max_partitions())


def render_filter(n_partitions: int, seen: int, passed: int, from_ms: Optional[int] = None, to_ms: Optional[int] = None,
                  partitions=None) -> str:
    """kta_render_filter: the section kta-analyzer prints after everything else with --librdkafka kta.from / kta.to /
    kta.partitions, from the filter as given and the first two counts of filter_info()."""
    bm = None if partitions is None else partition_bitmap(partitions, n_partitions)
    return _render(N.load().kta_render_filter, N.KTA_FILTER_NO_FROM if from_ms is None else int(from_ms),
                   N.KTA_FILTER_NO_TO if to_ms is None else int(to_ms), None if bm is None else _np_ptr(bm), n_partitions, seen, passed)


def partitioner_max_partitions() -> int:
    """The largest P, and the largest Q, of a context with the partitioner pass."""
    return int(N.load().kta_partitioner_max_partitions())


def murmur2(key: bytes) -> int:
    """Kafka's murmur2 of `key` as a u32 (kta_murmur2; host only)."""
    key = bytes(key)
    return int(N.load().kta_murmur2(key, len(key)))


def partition_bitmap(partitions, n_partitions: int) -> np.ndarray:
    """The u32 bitmap kta_set_filter and kta_filter_host take: bit p & 31 of word p // 32 for every p of `partitions`.
    A partition outside [0, 2^32) cannot be written down and raises; one at or beyond n_partitions is the library's to refuse."""
    ps = [int(p) for p in partitions]
    if any(p < 0 or p >= 2**32 for p in ps):
        raise ValueError("a partition of a filter's set must be >= 0")
    words = max((n_partitions + 31) // 32, max(ps, default=0) // 32 + 1, 1)
    bm = np.zeros(words, dtype=np.uint32)
    for p in ps:
        bm[p // 32] |= np.uint32(1 << (p % 32))
    return bm


def filter_host(partition, ts_ms, n_partitions: int, from_ms: Optional[int] = None, to_ms: Optional[int] = None,
                partitions=None) -> np.ndarray:
    """The indices of the records that a filter passes, ascending (kta_filter_host: the library's own predicate on the host)."""
    lib = N.load()
    p = np.ascontiguousarray(partition, dtype=np.int32)
    t = np.ascontiguousarray(ts_ms, dtype=np.int64)
    bm = None if partitions is None else partition_bitmap(partitions, n_partitions)
    idx = np.zeros(len(p), dtype=np.uint64)
    m = C.c_uint64(0)
    rc = lib.kta_filter_host(_np_ptr(p), _np_ptr(t), len(p), n_partitions, N.KTA_FILTER_NO_FROM if from_ms is None else int(from_ms),
                             N.KTA_FILTER_NO_TO if to_ms is None else int(to_ms), None if bm is None else _np_ptr(bm),
                             0 if bm is None else len(bm), _np_ptr(idx), C.byref(m))
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_filter_host")
    return idx[:m.value].copy()


def segments_words(n_partitions: int, rows_per_partition: int) -> int:
    """kta_segments_words: (P M + P) 4 + 8"""
    w = int(N.load().kta_segments_words(int(n_partitions), int(rows_per_partition)))
    if w == 0:
        raise KtaError(N.KTA_ERR_INVALID, "kta_segments_words: P >= 1, M >= 2 and P * M <= 2^20")
    return w


def segments_max_partitions() -> int:
    """The largest n_partitions a handler with segments may have (kta_segments_max_partitions)."""
    return int(N.load().kta_segments_max_partitions())


def _segments_vec(vec, P: int, M: int) -> np.ndarray:
    v = np.ascontiguousarray(vec).view(np.uint64) if isinstance(vec, np.ndarray) else np.array(vec, dtype=np.uint64)
    if v.shape != (segments_words(P, M),):
        raise KtaError(N.KTA_ERR_INVALID, f"a segment vector of {P} partitions and {M} rows has {segments_words(P, M)} words")
    return v


def split_segments(vec, n_partitions: int, rows_per_partition: int) -> dict:
    """The parts of a segment vector u64[(P M + P) 4 + 8] (views): "rows" [P][M][4] = {C, B, T, H + 1}, "totals" [P][4],
    "globals" [8] = counted, outside [0, P), rows closed, S, M, overhead, 0, 0."""
    P, M = int(n_partitions), int(rows_per_partition)
    v = _segments_vec(vec, P, M)
    return {"rows": v[:P * M * 4].reshape(P, M, 4), "totals": v[P * M * 4:(P * M + P) * 4].reshape(P, 4),
            "globals": v[(P * M + P) * 4:], "vector": v}


def merge_segments(acc: np.ndarray, other, n_partitions: int, rows_per_partition: int) -> np.ndarray:
    """kta_merge_segments, in place on `acc` (contiguous uint64): SUM over every word but S, M and overhead, which must
    agree (KtaError otherwise, acc unchanged)."""
    a = _segments_vec(acc, n_partitions, rows_per_partition)
    rc = N.load().kta_merge_segments(_np_ptr(a), _np_ptr(_segments_vec(other, n_partitions, rows_per_partition)), n_partitions,
                                     rows_per_partition)
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_merge_segments: bad bounds, or the vectors' S / M / overhead differ")
    return acc


RETENTION_COLUMNS = ("segments", "records", "bytes", "tombstones", "records_kept", "bytes_kept", "tombstones_kept",
                     "segments_deleted", "rule", "clamped")


def retention_whatif(vec, n_partitions: int, rows_per_partition: int, now_ms: int, retention_ms: int = -1,
                     retention_bytes: int = -1) -> np.ndarray:
    """kta_retention_whatif (pure host): u64[P + 1][10], a row per partition and one for the topic, columns
    RETENTION_COLUMNS; -1 turns a rule off."""
    P, M = int(n_partitions), int(rows_per_partition)
    v = _segments_vec(vec, P, M)
    out = np.zeros((P + 1, len(RETENTION_COLUMNS)), np.uint64)
    rc = N.load().kta_retention_whatif(_np_ptr(v), P, M, int(now_ms), int(retention_ms), int(retention_bytes), _np_ptr(out), out.size)
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_retention_whatif: bad arguments, or not a segment vector of this shape")
    return out


def render_retention(vec, n_partitions: int, rows_per_partition: int, now_ms: int, retention_ms: int = -1, retention_bytes: int = -1) -> str:
    """kta_render_retention: the section kta-analyzer prints with --librdkafka kta.segments=<size>, from a segment vector."""
    v = _segments_vec(vec, n_partitions, rows_per_partition)
    return _render(N.load().kta_render_retention, _np_ptr(v), int(n_partitions), int(rows_per_partition), int(now_ms), int(retention_ms),
                   int(retention_bytes))


def compact_delete_max_partitions() -> int:
    """The largest n_partitions a handler with the compact,delete what-if may have (kta_compact_delete_max_partitions)."""
    return int(N.load().kta_compact_delete_max_partitions())


def split_compact_delete(vec, n_partitions: int, rows_per_partition: int) -> dict:
    """The parts of a kept vector u64[(P M + P) 4 + 8] (views): "rows" [P][M][4] = {L, B, T, K}, "totals" [P][4], "globals"
    [8] = counted, outside [0, P), rows closed, S, M, overhead, 0, 0."""
    return split_segments(vec, n_partitions, rows_per_partition)


COMPACT_DELETE_COLUMNS = ("records", "bytes", "compacted_records", "compacted_bytes", "kept_records", "kept_bytes", "kept_tombstones",
                          "segments_deleted", "rule", "clamped")


def compact_delete_whatif(seg_vec, kept_vec, comp_vec, n_partitions: int, rows_per_partition: int, now_ms: int, retention_ms: int = -1,
                          retention_bytes: int = -1) -> np.ndarray:
    """kta_compact_delete_whatif (pure host) from the first pass's segment vector, the replay's kept vector and the replay's
    compaction vector: u64[P + 1][10], a row per partition and one for the topic, columns COMPACT_DELETE_COLUMNS; -1 turns
    a rule off.  KtaError (KTA_ERR_INVALID) for bad arguments and when the replay did not match the first pass."""
    P, M = int(n_partitions), int(rows_per_partition)
    s, k, c = _segments_vec(seg_vec, P, M), _segments_vec(kept_vec, P, M), _section_vec("compaction", comp_vec, P)
    out = np.zeros((P + 1, len(COMPACT_DELETE_COLUMNS)), np.uint64)
    rc = N.load().kta_compact_delete_whatif(_np_ptr(s), _np_ptr(k), _np_ptr(c), P, M, int(now_ms), int(retention_ms), int(retention_bytes),
                                            _np_ptr(out), out.size)
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_compact_delete_whatif: bad arguments, or the replay did not match the first pass")
    return out


def render_compact_delete(seg_vec, kept_vec, comp_vec, n_partitions: int, rows_per_partition: int, now_ms: int, retention_ms: int = -1,
                          retention_bytes: int = -1) -> str:
    """kta_render_compact_delete: the section kta-analyzer prints with kta.compact_delete=1.  KtaError (KTA_ERR_INVALID) when
    the replay did not match the first pass; the section that says so is the error's `text` ("" for other bad arguments)."""
    P, M = int(n_partitions), int(rows_per_partition)
    s, k, c = _segments_vec(seg_vec, P, M), _segments_vec(kept_vec, P, M), _section_vec("compaction", comp_vec, P)
    fn = N.load().kta_render_compact_delete
    args = (_np_ptr(s), _np_ptr(k), _np_ptr(c), P, M, int(now_ms), int(retention_ms), int(retention_bytes))
    n = C.c_size_t()
    fn(*args, None, 0, C.byref(n))
    buf = C.create_string_buffer(n.value + 1)
    rc = fn(*args, buf, len(buf), C.byref(n))
    if rc != N.KTA_OK:
        err = KtaError(rc, "kta_render_compact_delete: bad arguments, or the replay did not match the first pass")
        err.text = buf.value.decode()
        raise err
    return buf.value.decode()


def ts_order_max_partitions() -> int:
    """The largest P a context with the timestamp-order pass may have."""
    return int(N.load().kta_ts_order_max_partitions())


# ---------------------------------------------------------------------- synthetic topic helpers
def synth_preset(name: str) -> Tuple[KtaSynthSpec, int]:
    lib = N.load()
    sp, n = KtaSynthSpec(), C.c_uint64()
    rc = lib.kta_synth_preset(name.encode(), C.byref(sp), C.byref(n))
    if rc != N.KTA_OK:
        raise KtaError(rc, f"unknown preset {name!r}")
    return sp, n.value


def synth_fill_host(spec: KtaSynthSpec, first: int, n: int, with_keys: bool = False, with_seq: bool = False,
                    key_bytes_capacity: Optional[int] = None) -> dict:
    """Generate records [first, first+n) of the synthetic topic on the host (no GPU needed)."""
    lib = N.load()
    cols = {"partition": np.empty(n, np.int32), "key_len": np.empty(n, np.int32),
            "val_len": np.empty(n, np.int32), "ts_ms": np.empty(n, np.int64)}
    b = KtaBatch()
    b.partition, b.key_len = cols["partition"].ctypes.data, cols["key_len"].ctypes.data
    b.val_len, b.ts_ms = cols["val_len"].ctypes.data, cols["ts_ms"].ctypes.data
    b.capacity = n
    if with_seq:
        cols["seq"] = np.empty(n, np.uint64)
        b.seq = cols["seq"].ctypes.data
    kb = C.c_uint64(0)
    if with_keys:
        if key_bytes_capacity is None:  # first pass: count
            rc = lib.kta_synth_fill_host(C.byref(spec), first, n, C.byref(b), C.byref(kb))
            if rc != N.KTA_OK:
                raise KtaError(rc, "kta_synth_fill_host")
            key_bytes_capacity = kb.value
        cols["key_off"] = np.empty(n, np.uint32)
        cols["key_bytes"] = np.empty(max(key_bytes_capacity, 1), np.uint8)
        b.key_off, b.key_bytes = cols["key_off"].ctypes.data, cols["key_bytes"].ctypes.data
        b.key_bytes_capacity = key_bytes_capacity
    rc = lib.kta_synth_fill_host(C.byref(spec), first, n, C.byref(b), C.byref(kb))
    if rc != N.KTA_OK:
        raise KtaError(rc, "kta_synth_fill_host")
    if with_keys:
        cols["key_bytes"] = cols["key_bytes"][:kb.value]
    cols["n_key_bytes"] = kb.value
    return cols


def fnv_reference_kats():
    """Known-answer vectors of the reference FNV variant (fnv32.rs:92-101), SURVEY.md §8c."""
    return [(b"", 0x811C9DC5), (b"a", 0xC9A2E334), (b"b", 0x4CF8BC83), (b"foobar", 0xFFF67B86),
            (b"\x00", 0x6E533999), (b"\xff", 0x53C98FA2), (b"key-0", 0x7ECF789B), (b"key-1", 0xFDB2DAD6),
            (bytes(range(64)), 0x626AD045), (b"k" * 256, 0x7975FBC5)]

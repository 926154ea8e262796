"""ctypes binding of libkta_hip.so (include/kta_hip.h, include/kta_synth.h).

The library is built in-tree by kafka_topic_analyzer_amd/build.py.  There is deliberately no
fallback: if the shared object is missing, loading raises, and if no gfx950 device is visible
`kta_create` fails with KTA_ERR_NO_DEVICE.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KTA_LIB_PATH") or os.path.join(HERE, "libkta_hip.so")   # (KTA_LIB_PATH: another build of the library, tools/build_variant.sh)

KTA_OK = 0
KTA_ERR_INVALID = -1
KTA_ERR_HIP = -2
KTA_ERR_NOMEM = -3
KTA_ERR_NO_DEVICE = -4
KTA_ERR_BAD_PARTITION = -5
KTA_ERR_CAPACITY = -6
KTA_ERR_DIV_BY_ZERO = -7
KTA_ERR_COMM = -8
KTA_ERR_TIMESTAMP_RANGE = -9
KTA_CHRONO_MIN_SEC = -8334632851200
KTA_CHRONO_MAX_SEC = 8210298412799
KTA_COMM_ID_BYTES = 128

KTA_NCOUNTERS = 7
KTA_NGLOBALS = 8
(KTA_C_TOTAL, KTA_C_TOMBSTONES, KTA_C_ALIVE, KTA_C_KEY_NULL, KTA_C_KEY_NON_NULL,
 KTA_C_KEY_SIZE_SUM, KTA_C_VALUE_SIZE_SUM) = range(7)
(KTA_G_BAD_PARTITION, KTA_G_ALIVE_KEYS, KTA_G_RECORDS, KTA_G_RESERVED, KTA_G_NOT_MIN_TS_MS,
 KTA_G_MAX_TS_MS, KTA_G_NOT_SMALLEST, KTA_G_LARGEST) = range(8)
KTA_NSUM_GLOBALS = 4

KTA_PART_RANDOM, KTA_PART_KEY_AFFINE, KTA_PART_RUNS = 0, 1, 2
KTA_VAL_FIXED, KTA_VAL_EXP = 0, 1


class KtaConfig(C.Structure):
    _fields_ = [("device_id", C.c_int32), ("n_partitions", C.c_int32),
                ("count_alive_keys", C.c_int32), ("n_staging", C.c_int32),
                ("batch_capacity", C.c_uint64), ("key_bytes_capacity", C.c_uint64),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


KTA_FLAG_ANALYTICS = 1
KTA_FLAG_SEQ_COLUMN = 2
KTA_FLAG_ALIVE_TABLE = 4
KTA_HIST_BUCKETS = 34
KTA_ANALYTICS_HIST = 2 * KTA_HIST_BUCKETS   # analytics vector: u64[2*34 + 4*P]
KTA_TIMELINE_MAX_BUCKETS = 1024             # timeline vector: u64[(n_buckets + 3) * KTA_TIMELINE_COLS]
KTA_TIMELINE_COLS = 3
KTA_FLAG_KEY_SKETCH = 8
KTA_SKETCH_LOG2 = 12
KTA_SKETCH_REGISTERS = 1 << KTA_SKETCH_LOG2   # key sketch vector: u64[P * 4096], one register per word
KTA_SKETCH_MAX_PARTITIONS = 16384
KTA_FLAG_HOT_KEYS = 16
KTA_FLAG_TS_ORDER = 32
KTA_FLAG_PARTITIONER = 64         # partitioner vector: u64[2 P + 2 Q] = [P][2] checked, placed | [Q][2] target records, bytes
KTA_FLAG_COMPACTION = 128         # compaction vector: u64[5 P + 6] = [P][5] live records, key bytes, value bytes, tombstones, their key bytes | 6 globals
KTA_COMPACTION_WORDS, KTA_COMPACTION_GLOBALS = 5, 6
KTA_FLAG_SIZE_QUANTILES = 256     # size vector: u64[P * 3 * 464 + 8] = [P][3: key, value, message][464 bins] | 8 globals
KTA_SIZE_BINS, KTA_SIZE_QUANTITIES, KTA_SIZE_GLOBALS = 464, 3, 8
# record-batch vector: u64[20 P + 1524] = [P][16] sums | [5 codecs][100] sums and histograms | [P][4] maxima | 1024 sketch registers
KTA_FLAG_RECORD_BATCHES = 512
KTA_RB_PARTITION_WORDS, KTA_RB_CODECS, KTA_RB_CODEC_WORDS, KTA_RB_HIST_BINS, KTA_RB_MAX_WORDS, KTA_RB_SKETCH_REGISTERS = 16, 5, 100, 32, 4, 1024
# payload vector: u64[24 P + 16 + 2 * 1024 * 34] = [P][24] sums | 16 histogram bins | [2 rows][1024 cells][34: T, B, 32 bit counters]
KTA_FLAG_PAYLOAD = 1024
KTA_PAYLOAD_PARTITION_WORDS, KTA_PAYLOAD_CLASSES, KTA_PAYLOAD_HIST_BINS, KTA_PAYLOAD_ROWS, KTA_PAYLOAD_CELLS, KTA_PAYLOAD_CELL_WORDS = 24, 5, 16, 2, 1024, 34
# header-name vector: u64[8 + 2 * 1024 * 36] = 8 globals | [2 rows][1024 cells][36: T, L, V, Z, 32 bit counters]; beside it the name table [2 * 1024]
KTA_FLAG_HEADER_NAMES = 2048
KTA_HEADER_NAMES_GLOBALS, KTA_HEADER_NAMES_ROWS, KTA_HEADER_NAMES_CELLS, KTA_HEADER_NAMES_CELL_WORDS = 8, 2, 1024, 36
KTA_HEADER_NAMES_WORDS, KTA_HEADER_NAMES_SLOTS, KTA_HEADER_NAME_BYTES, KTA_HEADER_NAME_PUBLISHED = 8 + 2 * 1024 * 36, 2 * 1024, 48, 2
# value-byte vector: u64[264 P] = [P][264: 256 bins, records, values, bytes, repeats, 4 zero words]
KTA_FLAG_VALUE_BYTES = 4096
KTA_VALUE_BYTES_BINS, KTA_VALUE_BYTES_PARTITION_WORDS = 256, 264
KTA_VALUE_BYTES_NONE, KTA_VALUE_BYTES_TEXT, KTA_VALUE_BYTES_DENSE, KTA_VALUE_BYTES_BINARY = 0, 1, 2, 3
# compression what-if vector: u64[8 P + 20] = [P][8: batches, blocks, stored_blocks, raw_bytes, now_bytes, model_bytes, sequences,
# match_bytes] | [5 codecs][4: batches, raw_bytes, now_bytes, model_bytes]
KTA_FLAG_COMPRESS_WHATIF = 8192
KTA_COMPRESS_WHATIF_PARTITION_WORDS, KTA_COMPRESS_WHATIF_CODECS, KTA_COMPRESS_WHATIF_CODEC_WORDS = 8, 5, 4
KTA_TS_ORDER_HIST = 63            # timestamp-order vector: u64[3 P + 64] = [P][2] | hist[63] | timed | max_late_ms[P]
KTA_HOT_ROWS, KTA_HOT_CELLS, KTA_HOT_WORDS = 2, 1024, 23
KTA_HOT_VECTOR_WORDS = KTA_HOT_ROWS * KTA_HOT_CELLS * KTA_HOT_WORDS   # hot-key vector: u64[2][1024][23]
KTA_HOT_EXEMPLAR_BYTES = 32
KTA_HOT_MAX_REPORTED = 64


class KtaHotExemplar(C.Structure):
    _fields_ = [("hash", C.c_uint32), ("key_len", C.c_uint32), ("valid", C.c_uint32), ("pad", C.c_uint32),
                ("bytes", C.c_uint8 * KTA_HOT_EXEMPLAR_BYTES)]


class KtaHeaderName(C.Structure):
    _fields_ = [("hash", C.c_uint32), ("name_len", C.c_uint32), ("state", C.c_uint32), ("reserved", C.c_uint32),
                ("bytes", C.c_uint8 * KTA_HEADER_NAME_BYTES)]


class KtaHeaderNameRow(C.Structure):
    _fields_ = [("hash", C.c_uint32), ("has_name", C.c_uint32), ("occurrences", C.c_uint64), ("name_len", C.c_uint64),
                ("value_bytes", C.c_uint64), ("null_values", C.c_uint64), ("name", C.c_uint8 * KTA_HEADER_NAME_BYTES)]


class KtaValueBytesSummary(C.Structure):
    _fields_ = [("records", C.c_uint64), ("values", C.c_uint64), ("bytes", C.c_uint64), ("repeats", C.c_uint64), ("distinct", C.c_uint64),
                ("floor_bytes", C.c_uint64), ("printable", C.c_uint64), ("zero", C.c_uint64), ("high", C.c_uint64), ("top_count", C.c_uint64),
                ("entropy_bits", C.c_double), ("top_byte", C.c_uint32), ("cls", C.c_uint32)]


class KtaHotKey(C.Structure):
    _fields_ = [("hash", C.c_uint32), ("pad", C.c_uint32), ("upper", C.c_uint64), ("lower", C.c_uint64)]


class KtaAnalytics(C.Structure):
    _fields_ = [("key_size_hist", C.c_uint64 * 34), ("value_size_hist", C.c_uint64 * 34)]


KTA_LAYOUT_RAW, KTA_LAYOUT_TILE_COMPACT = 0, 1   # kta_batch.layout (include/kta_hip.h)
KTA_TILE_RECORDS = 1024
KTA_TILE_RAW, KTA_TILE_COMPACT = 0, 1             # kta_tile_hdr.mode
KTA_TILE_LENS_I32, KTA_TILE_LENS_U16 = 0, 1        # kta_tile_hdr.lens
KTA_TILE_SUM_VALID, KTA_TILE_SUM_TIMED, KTA_TILE_SUM_UNTIMED = 1, 2, 4   # kta_tile_sum.flags
KTA_COMPACT_PART_NONE = 0xFFFF
KTA_FILTER_NO_FROM, KTA_FILTER_NO_TO = -2**63, 2**63 - 1   # kta_set_filter: no bound on that side (INT64_MIN / INT64_MAX)
KTA_FILTER_TILE_READ, KTA_FILTER_TILE_NONE, KTA_FILTER_TILE_ALL = 0, 1, 2   # kta_filter_tile_host


class KtaTileSum(C.Structure):
    _fields_ = [("ts_span", C.c_uint32), ("part_max", C.c_uint16), ("flags", C.c_uint16)]


class KtaBatch(C.Structure):
    _fields_ = [("partition", C.c_void_p), ("key_len", C.c_void_p), ("val_len", C.c_void_p),
                ("ts_ms", C.c_void_p), ("key_off", C.c_void_p), ("key_bytes", C.c_void_p),
                ("seq", C.c_void_p), ("capacity", C.c_uint64), ("key_bytes_capacity", C.c_uint64),
                ("tile_hdr", C.c_void_p), ("layout", C.c_uint32), ("reserved", C.c_uint32)]


class KtaResult(C.Structure):
    _fields_ = [("n_partitions", C.c_uint32), ("any_records", C.c_uint32), ("any_live", C.c_uint32),
                ("count_alive_keys", C.c_uint32), ("min_ts_sec", C.c_int64), ("max_ts_sec", C.c_int64),
                ("smallest_message", C.c_uint64), ("largest_message", C.c_uint64),
                ("overall_count", C.c_uint64), ("overall_size", C.c_uint64), ("alive_keys", C.c_uint64),
                ("bad_partition_records", C.c_uint64)]


class KtaSynthSpec(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("n_partitions", C.c_uint32), ("shard_index", C.c_uint32),
                ("shard_count", C.c_uint32), ("part_mode", C.c_uint32), ("part_run_len", C.c_uint32),
                ("key_null_permille", C.c_uint32), ("key_empty_permille", C.c_uint32),
                ("n_key_lens", C.c_uint32), ("key_lens", C.c_uint32 * 8), ("n_distinct_keys", C.c_uint64),
                ("tombstone_permille", C.c_uint32), ("val_empty_permille", C.c_uint32),
                ("val_mode", C.c_uint32), ("val_mean", C.c_uint32), ("val_cap", C.c_uint32),
                ("ts_missing_permille", C.c_uint32), ("ts_base_ms", C.c_int64), ("ts_step_us", C.c_uint32),
                ("ts_jitter_ms", C.c_uint32)]


class KtaKafkaBatchDesc(C.Structure):
    _fields_ = [("byte_off", C.c_uint64), ("record_base", C.c_uint64), ("crc", C.c_uint32), ("status", C.c_uint32),
                ("payload_off", C.c_uint64), ("payload_end", C.c_uint64),
                ("base_offset", C.c_int64), ("base_ts_ms", C.c_int64), ("max_ts_ms", C.c_int64),
                ("batch_bytes", C.c_uint32), ("partition", C.c_int32), ("n_records", C.c_int32),
                ("flags", C.c_uint32), ("scratch_end", C.c_uint64)]


class KtaKafkaIndexStats(C.Structure):
    _fields_ = [("n_batches", C.c_uint64), ("n_records", C.c_uint64), ("n_control_batches", C.c_uint64),
                ("n_compressed", C.c_uint64), ("n_snappy", C.c_uint64), ("n_lz4", C.c_uint64),
                ("inflate_bytes", C.c_uint64),
                ("n_old_magic", C.c_uint64), ("trailing_bytes", C.c_uint64),
                ("bytes_consumed", C.c_uint64), ("n_gzip", C.c_uint64), ("n_zstd", C.c_uint64),
                ("first_offset", C.c_int64), ("next_offset", C.c_int64), ("any_offsets", C.c_uint64)]


# every symbol include/kta_hip.h, kta_synth.h and kta_kafka.h declare: (restype, argtypes)
_P = C.c_void_p
SIGNATURES = {
    "kta_abi_version": (C.c_int, []),
    "kta_create": (C.c_int, [C.POINTER(KtaConfig), C.POINTER(_P)]),
    "kta_destroy": (None, [_P]),
    "kta_last_error": (C.c_char_p, [_P]),
    "kta_reset": (C.c_int, [_P]),
    "kta_handle_message": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_int64]),
    "kta_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "kta_flush": (C.c_int, [_P]),
    "kta_replay_messages": (C.c_int, [_P, C.c_void_p, C.c_uint64]),
    "kta_handle_message_stats": (C.c_int, [_P, C.POINTER(C.c_uint64 * 4)]),
    "kta_seek_seq": (C.c_int, [_P, C.c_uint64]),
    "kta_batch_acquire": (C.c_int, [_P, C.POINTER(KtaBatch)]),
    "kta_batch_submit": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint64]),
    "kta_submit_device": (C.c_int, [_P, C.POINTER(KtaBatch), C.c_uint64, C.c_uint64]),
    "kta_submit_device_ex": (C.c_int, [_P, C.POINTER(KtaBatch), C.c_uint64, C.c_uint64, C.c_int]),
    "kta_device_batch_alloc": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(KtaBatch)]),
    "kta_device_batch_free": (C.c_int, [_P, C.POINTER(KtaBatch)]),
    "kta_batch_from_raw": (C.c_int, [_P, C.POINTER(KtaBatch), C.c_uint64, C.POINTER(KtaBatch)]),
    "kta_batch_to_raw": (C.c_int, [_P, C.POINTER(KtaBatch), C.c_uint64, C.POINTER(KtaBatch)]),
    "kta_batch_tile_summaries": (C.c_int, [_P, C.POINTER(KtaBatch), C.c_uint64, C.c_void_p]),
    "kta_batch_tile_planes": (C.c_int, [_P, C.POINTER(KtaBatch), C.c_uint64, C.c_void_p]),
    "kta_copy_to_device": (C.c_int, [_P, C.c_void_p, C.c_void_p, C.c_size_t]),
    "kta_copy_to_host": (C.c_int, [_P, C.c_void_p, C.c_void_p, C.c_size_t]),
    "kta_set_compute_stream": (C.c_int, [_P, C.c_void_p]),
    "kta_sync": (C.c_int, [_P]),
    "kta_finish": (C.c_int, [_P, C.POINTER(KtaResult), C.c_void_p]),
    "kta_result_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_finish_device": (C.c_int, [_P]),
    "kta_comm_unique_id": (C.c_int, [C.c_char_p]),
    "kta_comm_create": (C.c_int, [_P, C.c_int, C.c_int, C.c_char_p]),
    "kta_comm_destroy": (C.c_int, [_P]),
    "kta_exchange": (C.c_int, [_P]),
    "kta_exchange_result": (C.c_int, [_P, C.POINTER(KtaResult), C.c_void_p]),
    "kta_comm_allreduce_i64": (C.c_int, [_P, C.c_void_p, C.c_size_t, C.c_int]),
    "kta_comm_info": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kta_decode_vector": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(KtaResult), C.c_void_p]),
    "kta_merge_vectors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "kta_get_analytics": (C.c_int, [_P, C.POINTER(KtaAnalytics), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kta_analytics_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_exchange_analytics": (C.c_int, [_P, C.POINTER(KtaAnalytics), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kta_analytics_result_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_decode_analytics": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(KtaAnalytics), C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "kta_merge_analytics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "kta_analytics_max_partitions": (C.c_int, []),
    "kta_render_analytics": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kta_set_timeline": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_uint32]),
    "kta_timeline_max_partitions": (C.c_int, [C.c_uint32, C.c_uint32]),
    "kta_get_timeline": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_timeline_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_exchange_timeline": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_timeline_result_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_render_timeline": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_uint32, C.c_char_p, C.c_size_t,
                                      C.POINTER(C.c_size_t)]),
    "kta_get_key_sketch": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_exchange_key_sketch": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_key_sketch_result_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_merge_key_sketch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "kta_key_sketch_estimate": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "kta_key_sketch_info": (C.c_int, [_P, C.POINTER(C.c_uint64 * 4)]),
    "kta_get_hot_keys": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_exchange_hot_keys": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_hot_keys_result_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_merge_hot_keys": (C.c_int, [C.c_void_p, C.c_void_p]),
    "kta_hot_keys_recover": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "kta_get_hot_key_exemplars": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_hot_keys_info": (C.c_int, [_P, C.POINTER(C.c_uint64 * 6)]),
    "kta_set_hot_flush_rounds": (C.c_int, [_P, C.c_uint32]),
    "kta_render_hot_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kta_get_ts_order": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_exchange_ts_order": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_ts_order_result_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_merge_ts_order": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "kta_ts_order_max_partitions": (C.c_int, []),
    "kta_ts_order_info": (C.c_int, [_P, C.POINTER(C.c_uint64 * 6)]),
    "kta_set_ts_order_chunk": (C.c_int, [_P, C.c_uint64]),
    "kta_render_ts_order": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kta_set_repartition": (C.c_int, [_P, C.c_uint32]),
    "kta_get_partitioner": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_exchange_partitioner": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_partitioner_result_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_merge_partitioner": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    "kta_partitioner_max_partitions": (C.c_int, []),
    "kta_partitioner_info": (C.c_int, [_P, C.POINTER(C.c_uint64 * 6)]),
    "kta_get_size_quantiles": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_exchange_size_quantiles": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_size_quantiles_result_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_merge_size_quantiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "kta_size_quantiles_max_partitions": (C.c_int, []),
    "kta_size_quantiles_info": (C.c_int, [_P, C.POINTER(C.c_uint64 * 6)]),
    "kta_set_size_quantiles_slice": (C.c_int, [_P, C.c_uint32]),
    "kta_size_bin": (C.c_uint32, [C.c_uint32]),
    "kta_size_bin_bounds": (C.c_int, [C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kta_size_quantile": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kta_get_record_batches": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_exchange_record_batches": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_record_batches_result_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_record_batches_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_merge_record_batches": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "kta_record_batches_estimate_producers": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double)]),
    "kta_record_batches_identities": (C.c_int, [C.c_void_p, C.c_uint32]),
    "kta_record_batches_host": (C.c_int, [C.c_char_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint32]),
    "kta_record_batches_info": (C.c_int, [_P, C.POINTER(C.c_uint64 * 4), C.POINTER(C.c_float)]),
    "kta_render_record_batches": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kta_get_payload": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_exchange_payload": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_payload_result_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_payload_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_merge_payload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "kta_payload_identities": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "kta_payload_schema_ids": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kta_payload_host": (C.c_int, [C.c_char_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_uint32]),
    "kta_payload_info": (C.c_int, [_P, C.POINTER(C.c_uint64 * 4), C.POINTER(C.c_float)]),
    "kta_render_payload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kta_get_header_names": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_exchange_header_names": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_header_names_result_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_header_names_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_merge_header_names": (C.c_int, [C.c_void_p, C.c_void_p]),
    "kta_get_header_name_table": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_header_names_identities": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "kta_header_names_list": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_uint64)]),
    "kta_header_names_host": (C.c_int, [C.c_char_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint32]),
    "kta_header_names_info": (C.c_int, [_P, C.POINTER(C.c_uint64 * 8), C.POINTER(C.c_float)]),
    "kta_render_header_names": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kta_get_value_bytes": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_exchange_value_bytes": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_value_bytes_result_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_value_bytes_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_merge_value_bytes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "kta_value_bytes_identities": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "kta_value_bytes_summary": (C.c_int, [C.c_void_p, C.POINTER(KtaValueBytesSummary)]),
    "kta_value_bytes_host": (C.c_int, [C.c_char_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_uint32]),
    "kta_value_bytes_info": (C.c_int, [_P, C.POINTER(C.c_uint64 * 4), C.POINTER(C.c_float)]),
    "kta_render_value_bytes": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kta_get_compress_whatif": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_exchange_compress_whatif": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_compress_whatif_result_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_compress_whatif_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_merge_compress_whatif": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "kta_compress_whatif_identities": (C.c_int, [C.c_void_p, C.c_uint32]),
    "kta_compress_whatif_host": (C.c_int, [C.c_char_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_uint32]),
    "kta_compress_whatif_info": (C.c_int, [_P, C.POINTER(C.c_uint64 * 4), C.POINTER(C.c_float)]),
    "kta_render_compress_whatif": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kta_lz4_model_host": (C.c_int64, [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64]),
    "kta_render_size_percentiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kta_set_segments": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_uint32]),
    "kta_segments_words": (C.c_uint32, [C.c_uint32, C.c_uint32]),
    "kta_get_segments": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_exchange_segments": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_segments_result_vector": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_segments_max_partitions": (C.c_int, []),
    "kta_segments_info": (C.c_int, [_P, C.POINTER(C.c_uint64 * 6)]),
    "kta_set_segments_chunk": (C.c_int, [_P, C.c_uint64]),
    "kta_merge_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    "kta_retention_whatif": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t]),
    "kta_render_retention": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int64, C.c_int64, C.c_int64, C.c_char_p, C.c_size_t,
                                       C.POINTER(C.c_size_t)]),
    "kta_murmur2": (C.c_uint32, [C.c_void_p, C.c_size_t]),
    "kta_compaction_replay": (C.c_int, [_P, C.c_int]),
    "kta_get_compaction": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_compaction_max_partitions": (C.c_int, []),
    "kta_compaction_info": (C.c_int, [_P, C.POINTER(C.c_uint64 * 6)]),
    "kta_set_compact_delete": (C.c_int, [_P, C.c_int]),
    "kta_compact_delete_max_partitions": (C.c_int, []),
    "kta_get_compact_delete": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
    "kta_compact_delete_info": (C.c_int, [_P, C.POINTER(C.c_uint64 * 4)]),
    "kta_compact_delete_whatif": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int64, C.c_int64, C.c_int64,
                                            C.c_void_p, C.c_size_t]),
    "kta_render_compact_delete": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int64, C.c_int64, C.c_int64,
                                            C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kta_render_compaction": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kta_set_filter": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_void_p, C.c_uint32]),
    "kta_filter_info": (C.c_int, [_P, C.POINTER(C.c_uint64 * 6)]),
    "kta_set_filter_slice": (C.c_int, [_P, C.c_uint64]),
    "kta_filter_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int64, C.c_int64, C.c_void_p, C.c_uint32,
                                  C.c_void_p, C.POINTER(C.c_uint64)]),
    "kta_filter_tile_host": (C.c_int, [C.c_uint32, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "kta_render_partitioner": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t,
                                         C.POINTER(C.c_size_t)]),
    "kta_render_filter": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_char_p, C.c_size_t,
                                    C.POINTER(C.c_size_t)]),
    "kta_render_distinct_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t,
                                           C.POINTER(C.c_size_t)]),
    "kta_export_alive_bitmap": (C.c_int, [_P, C.c_void_p]),
    "kta_alive_table": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "kta_alive_export_entries": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "kta_alive_import_entries": (C.c_int, [_P, C.c_void_p, C.c_void_p, C.c_uint64]),
    "kta_alive_count_range": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    "kta_alive_table_modified": (C.c_int, [_P]),
    "kta_fnv32_device": (C.c_int, [_P, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "kta_render_report": (C.c_int, [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.c_int64, C.c_uint32,
                                    C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    "kta_set_timing": (C.c_int, [_P, C.c_int]),
    "kta_kernel_time_stats": (C.c_int, [_P, C.POINTER(C.c_float * 3), C.POINTER(C.c_uint64 * 3)]),
    "kta_set_tuning": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int]),
    "kta_set_fuse": (C.c_int, [_P, C.c_int]),
    "kta_alive_pass_info": (C.c_int, [_P, C.POINTER(C.c_uint64 * 6)]),
    "kta_synth_fill_host": (C.c_int, [C.POINTER(KtaSynthSpec), C.c_uint64, C.c_uint64, C.POINTER(KtaBatch),
                                      C.POINTER(C.c_uint64)]),
    "kta_synth_fill_device": (C.c_int, [_P, C.POINTER(KtaSynthSpec), C.c_uint64, C.c_uint64,
                                        C.POINTER(KtaBatch), C.POINTER(C.c_uint64)]),
    "kta_synth_preset": (C.c_int, [C.c_char_p, C.POINTER(KtaSynthSpec), C.POINTER(C.c_uint64)]),
    "kta_kafka_index_host": (C.c_int, [C.c_char_p, C.c_uint64, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64,
                                       C.POINTER(KtaKafkaBatchDesc), C.c_uint64, C.POINTER(KtaKafkaIndexStats)]),
    "kta_zstd_inflate_host": (C.c_int64, [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]),
    "kta_zstd_inflate_host_small": (C.c_int64, [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]),
    "kta_gzip_inflate_host": (C.c_int64, [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]),
    "kta_gzip_inflate_lane_host": (C.c_int64, [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]),
    "kta_lz4_inflate_host": (C.c_int64, [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]),
    "kta_snappy_inflate_host": (C.c_int64, [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]),
    "kta_kafka_decode_device": (C.c_int, [_P, C.c_void_p, C.c_uint64, C.POINTER(KtaKafkaBatchDesc), C.c_uint64,
                                          C.c_uint64, C.POINTER(KtaBatch), C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint64)]),
    "kta_kafka_decode_rounds_host": (C.c_int, [C.c_char_p, C.c_uint64, C.POINTER(KtaKafkaBatchDesc), C.c_uint64,
                                               C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "kta_kafka_configure": (C.c_int, [_P, C.c_uint64, C.c_int]),
    "kta_kafka_blob_acquire": (C.c_int, [_P, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "kta_kafka_blob_submit": (C.c_int, [_P, C.c_uint64, C.c_int32, C.POINTER(KtaKafkaIndexStats)]),
    "kta_kafka_consume": (C.c_int, [_P, C.c_char_p, C.c_uint64, C.c_int32, C.POINTER(KtaKafkaIndexStats)]),
    "kta_kafka_encode_synth_host": (C.c_int, [C.POINTER(KtaSynthSpec), C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p,
                                              C.c_uint64, C.POINTER(C.c_uint64)]),
    "kta_kafka_encode_synth_host_ex": (C.c_int, [C.POINTER(KtaSynthSpec), C.c_uint64, C.c_uint64, C.c_uint32, C.c_int,
                                                 C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "kta_kafka_set_variant": (C.c_int, [_P, C.c_int]),
    "kta_kafka_set_inflate_limit": (C.c_int, [_P, C.c_uint64]),
    "kta_kafka_set_check_crcs": (C.c_int, [_P, C.c_int]),
    "kta_kafka_crc_errors": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "kta_crc32c_host": (C.c_uint32, [C.c_char_p, C.c_uint64]),
    "kta_kafka_time_stats": (C.c_int, [_P, C.POINTER(C.c_float * 2), C.POINTER(C.c_uint64 * 2)]),
}

_lib = None


KTA_ABI_VERSION = 7  # include/kta_hip.h


def load() -> C.CDLL:
    """Load libkta_hip.so; raise loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: run `python -m kafka_topic_analyzer_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.kta_abi_version() != KTA_ABI_VERSION:   # struct layouts below must match the library's
        raise ImportError(f"libkta_hip.so has ABI version {lib.kta_abi_version()}, this package expects "
                          f"{KTA_ABI_VERSION}: rebuild with `python -m kafka_topic_analyzer_amd.build`")
    _lib = lib
    return lib

"""Partition-sharded multi-GPU plumbing over torch.distributed (backend "nccl" is RCCL over xGMI on ROCm,
"gloo" on CPU in the tests).  The PRODUCT path of the exchange is native — kta_comm_create / kta_exchange
(csrc/kta_comm.hip, include/kta_hip.h) — and needs no torch; this module is the same exchange written on
torch collectives, kept as the harness the world-size-2/3 gloo tests drive on CPU and as a cross-check of
the native one.

The reference is single-process (src/kafka.rs:92-135), but every per-partition counter depends only
on its own partition's records (src/metric.rs:74-100) and the globals are min/max/sum, so Kafka
partitions shard across ranks with no data-path collective and ONE exchange step at the end:

    C1  all-reduce SUM  over vec[0 : P*7 + 4]      (counters + SUM-type globals; i64 wrap == u64 wrap)
    C2  all-reduce MAX  over vec[P*7 + 4 : P*7+8]  (~min ts, max ts, ~smallest, largest; signed)

The alive-key set is global and order dependent (src/metric.rs:262-264, 289-304): each rank keeps the
last-writer table for its partitions (entry = ((seq+1)<<1)|alive with seq the GLOBAL consumption
index), and an element-wise MAX across ranks is exactly "the last writer in consumption order wins".
"""
from __future__ import annotations

import copy

from . import _native as N


def shard_spec(spec, rank: int, world: int):
    """The synthetic-topic shard of `rank`: partitions p with p % world == rank."""
    s = copy.copy(spec)
    s.shard_index, s.shard_count = rank, world
    return s


def partition_owner(partition: int, world: int) -> int:
    return partition % world


def sum_prefix_len(n_partitions: int) -> int:
    return n_partitions * N.KTA_NCOUNTERS + N.KTA_NSUM_GLOBALS


def _allreduce_sum_max(vec, sum_words: int, group) -> None:
    """The rule of every result vector, in place: all-reduce SUM over vec[:sum_words], all-reduce MAX over the rest
    (a half of no words is left out)."""
    import torch.distributed as dist
    if sum_words:
        dist.all_reduce(vec[:sum_words], op=dist.ReduceOp.SUM, group=group)
    if sum_words < vec.numel():
        dist.all_reduce(vec[sum_words:], op=dist.ReduceOp.MAX, group=group)


def allreduce_counter_vector(vec, n_partitions: int, group=None, alive_keys: str = "share") -> None:
    """In-place exchange step over an int64 view of the SNAPSHOT counter vector (kta_result_vector: device
    tensor, or a CPU tensor in the tests) — the live accumulator is never reduced.

    KTA_G_ALIVE_KEYS sits in the SUM prefix, so what every rank contributes must add up to the job's count:
    "share"  — each rank's word is the count of a DISJOINT share of the slots (the hash range it owns after
               exchange_alive_by_hash_range; what kta_exchange does natively); the default;
    "merged" — the tables were fully merged first (exchange_alive_entries / allreduce_alive_table), every rank
               holds the global count: all ranks but 0 contribute zero."""
    import torch.distributed as dist
    assert vec.numel() == n_partitions * N.KTA_NCOUNTERS + N.KTA_NGLOBALS
    assert alive_keys in ("share", "merged")
    if alive_keys == "merged" and dist.get_rank(group) != 0:
        vec[n_partitions * N.KTA_NCOUNTERS + N.KTA_G_ALIVE_KEYS] = 0
    _allreduce_sum_max(vec, sum_prefix_len(n_partitions), group)


def allreduce_analytics_vector(avec, n_partitions: int, group=None) -> None:
    """In-place exchange of an int64 view of the analytics SNAPSHOT (kta_analytics_result_vector: device tensor,
    or a CPU tensor in the tests) — what kta_exchange does natively when the contexts have KTA_FLAG_ANALYTICS:
    all-reduce SUM over the 2 x 34 histogram words (i64 wrap == u64 wrap) and all-reduce MAX over the 4 * P extrema
    words ([~min ts, max ts, ~smallest, largest] per partition; INT64_MIN where a rank saw nothing)."""
    assert avec.numel() == N.KTA_ANALYTICS_HIST + 4 * n_partitions
    _allreduce_sum_max(avec, N.KTA_ANALYTICS_HIST, group)


def allreduce_timeline_vector(tvec, group=None) -> None:
    """In-place exchange of an int64 view of the timeline SNAPSHOT (kta_timeline_result_vector: device tensor, or a
    CPU tensor in the tests) — what kta_exchange does natively for a context with a timeline: all-reduce SUM over
    every word (i64 wrap == u64 wrap).  Every rank must have the same timeline configuration."""
    assert tvec.numel() % N.KTA_TIMELINE_COLS == 0
    _allreduce_sum_max(tvec, tvec.numel(), group)


def allreduce_hot_keys_vector(hvec, group=None) -> None:
    """In-place exchange of an int64 view of the hot-key SNAPSHOT (kta_hot_keys_result_vector: device tensor, or a CPU
    tensor in the tests) — what kta_exchange does natively when the contexts have KTA_FLAG_HOT_KEYS: all-reduce SUM over
    all of its 2 * 1024 * 23 words.  Exemplars are not moved."""
    assert hvec.numel() == N.KTA_HOT_VECTOR_WORDS
    _allreduce_sum_max(hvec, hvec.numel(), group)


def allreduce_ts_order_vector(ovec, n_partitions: int, group=None) -> None:
    """In-place exchange of an int64 view of the timestamp-order SNAPSHOT (kta_ts_order_result_vector: device tensor, or a
    CPU tensor in the tests) — what kta_exchange does natively when the contexts have KTA_FLAG_TS_ORDER: all-reduce SUM over
    the first 2 P + 64 words (i64 wrap == u64 wrap) and all-reduce MAX over the last P (never negative).  Exact when every
    partition's records went through ONE rank in order (partition p on rank p % N)."""
    assert ovec.numel() == 3 * n_partitions + 64
    _allreduce_sum_max(ovec, 2 * n_partitions + 64, group)


def allreduce_partitioner_vector(pvec, n_partitions: int, repartition: int, group=None) -> None:
    """In-place exchange of an int64 view of the partitioner SNAPSHOT (kta_partitioner_result_vector: device tensor, or a CPU
    tensor in the tests) — what kta_exchange does natively when the contexts have KTA_FLAG_PARTITIONER: all-reduce SUM over
    all of its 2 P + 2 Q words (i64 wrap == u64 wrap).  Every rank must have the same Q."""
    assert pvec.numel() == 2 * n_partitions + 2 * repartition
    _allreduce_sum_max(pvec, pvec.numel(), group)


def allreduce_size_quantiles_vector(qvec, n_partitions: int, group=None) -> None:
    """In-place exchange of an int64 view of the size-percentile SNAPSHOT (kta_size_quantiles_result_vector: device tensor, or
    a CPU tensor in the tests) — what kta_exchange does natively when the contexts have KTA_FLAG_SIZE_QUANTILES: all-reduce SUM
    over all of its P * 3 * 464 + 8 words (i64 wrap == u64 wrap)."""
    assert qvec.numel() == n_partitions * N.KTA_SIZE_QUANTITIES * N.KTA_SIZE_BINS + N.KTA_SIZE_GLOBALS
    _allreduce_sum_max(qvec, qvec.numel(), group)


def allreduce_record_batches_vector(bvec, n_partitions: int, group=None) -> None:
    """In-place exchange of an int64 view of the record-batch SNAPSHOT (kta_record_batches_result_vector: device tensor, or a
    CPU tensor in the tests) — what kta_exchange does natively when the contexts have KTA_FLAG_RECORD_BATCHES: all-reduce SUM
    over the first 16 P + 500 words (i64 wrap == u64 wrap) and all-reduce MAX over the 4 P + 1024 words behind them — counts,
    bytes, leader epochs + 1, clamped spans and sketch ranks, all below 2^63, so signed MAX == unsigned MAX."""
    assert bvec.numel() == 20 * n_partitions + 1524
    _allreduce_sum_max(bvec, 16 * n_partitions + 500, group)


def allreduce_payload_vector(lvec, n_partitions: int, group=None) -> None:
    """In-place exchange of an int64 view of the payload SNAPSHOT (kta_payload_result_vector: device tensor, or a CPU tensor in
    the tests) — what kta_exchange does natively when the contexts have KTA_FLAG_PAYLOAD: one all-reduce SUM over all
    24 P + 16 + 2 * 1024 * 34 words (i64 wrap == u64 wrap)."""
    assert lvec.numel() == 24 * n_partitions + 16 + 2 * 1024 * 34
    _allreduce_sum_max(lvec, lvec.numel(), group)


def allreduce_header_names_vector(nvec, group=None) -> None:
    """In-place exchange of an int64 view of the header-name SNAPSHOT (kta_header_names_result_vector: device tensor, or a CPU
    tensor in the tests) — what kta_exchange does natively when the contexts have KTA_FLAG_HEADER_NAMES: one all-reduce SUM over
    all 8 + 2 * 1024 * 36 words (i64 wrap == u64 wrap).  The name tables stay on their ranks."""
    assert nvec.numel() == 8 + 2 * 1024 * 36
    _allreduce_sum_max(nvec, nvec.numel(), group)


def allreduce_value_bytes_vector(yvec, n_partitions: int, group=None) -> None:
    """In-place exchange of an int64 view of the value-byte SNAPSHOT (kta_value_bytes_result_vector: device tensor, or a CPU
    tensor in the tests) — what kta_exchange does natively when the contexts have KTA_FLAG_VALUE_BYTES: one all-reduce SUM over
    all 264 * P words (i64 wrap == u64 wrap)."""
    assert yvec.numel() == 264 * n_partitions
    _allreduce_sum_max(yvec, yvec.numel(), group)


def allreduce_compress_whatif_vector(wvec, n_partitions: int, group=None) -> None:
    """In-place exchange of an int64 view of the compression what-if SNAPSHOT (kta_compress_whatif_result_vector: device
    tensor, or a CPU tensor in the tests) — what kta_exchange does natively when the contexts have KTA_FLAG_COMPRESS_WHATIF:
    one all-reduce SUM over all 8 * P + 20 words (i64 wrap == u64 wrap)."""
    assert wvec.numel() == 8 * n_partitions + 20
    _allreduce_sum_max(wvec, wvec.numel(), group)


def allreduce_segments_vector(gvec, n_partitions: int, rows_per_partition: int, group=None) -> None:
    """In-place exchange of an int64 view of the segment SNAPSHOT (kta_segments_result_vector: device tensor, or a CPU
    tensor in the tests) — what kta_exchange does natively for contexts with segments (kta_set_segments): all-reduce SUM
    over every word but the last five (i64 wrap == u64 wrap) and all-reduce MAX over those — S, M, overhead and two zero
    words, which every rank must have alike.  Exact when every partition's records went through ONE rank in order
    (partition p on rank p % N)."""
    words = (n_partitions * rows_per_partition + n_partitions) * 4 + 8
    assert gvec.numel() == words
    _allreduce_sum_max(gvec, words - 5, group)


def allreduce_key_sketch_vector(svec, group=None) -> None:
    """In-place exchange of an int64 view of the key sketch SNAPSHOT (kta_key_sketch_result_vector: device tensor, or a
    CPU tensor in the tests) — what kta_exchange does natively when the contexts have KTA_FLAG_KEY_SKETCH: all-reduce
    MAX over every word (registers are 0..21, so signed MAX == unsigned MAX).  Every rank must have the flag."""
    assert svec.numel() % N.KTA_SKETCH_REGISTERS == 0
    _allreduce_sum_max(svec, 0, group)


def allreduce_alive_table(table, group=None, chunk_elems: int = 1 << 28) -> None:
    """Element-wise MAX of the last-writer tables, in place, chunked (2 GiB of int64 per call) so
    RCCL's staging stays bounded.  Values are < 2^63, so signed MAX == unsigned MAX."""
    import torch.distributed as dist
    n = table.numel()
    for lo in range(0, n, chunk_elems):
        dist.all_reduce(table[lo:min(lo + chunk_elems, n)], op=dist.ReduceOp.MAX, group=group)


def gather_entries(slots, vals, group=None):
    """all_gather of variable-length (slot u32-as-i32, value u64-as-i64) entry lists -> per-rank lists.
    Works on device tensors (RCCL) and CPU tensors (gloo).  Shorter lists are zero padded: value 0 means
    "never written" and is ignored by the import kernel."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    n = torch.tensor([slots.numel()], dtype=torch.int64, device=slots.device)
    sizes = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(sizes, n, group=group)
    sizes = [int(s.item()) for s in sizes]
    m = max(max(sizes), 1)
    ps = torch.zeros(m, dtype=slots.dtype, device=slots.device)
    pv = torch.zeros(m, dtype=vals.dtype, device=vals.device)
    ps[:slots.numel()] = slots
    pv[:vals.numel()] = vals
    gs = [torch.empty_like(ps) for _ in range(world)]
    gv = [torch.empty_like(pv) for _ in range(world)]
    dist.all_gather(gs, ps, group=group)
    dist.all_gather(gv, pv, group=group)
    return gs, gv, sizes


class _DevArray:
    """Zero-copy torch view of library-owned device memory."""

    def __init__(self, ptr: int, n: int, typestr: str):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def exchange_alive_entries(handler, device, group=None) -> int:
    """Merge the alive-key state of all ranks into every rank, compactly: each rank exports the table
    entries it ever wrote (<= one per distinct key hash: 12 B each), the lists are all-gathered, and every
    rank imports the foreign entries with atomicMax — the element-wise MAX of the tables without moving
    32 GiB per rank.  Returns the number of foreign entries imported."""
    import torch
    import torch.distributed as dist
    rank = dist.get_rank(group)
    ps, pv, n = handler.alive_export_entries()
    dev = torch.device("cuda", device)
    if n:
        slots = torch.as_tensor(_DevArray(ps, n, "<i4"), device=dev)
        vals = torch.as_tensor(_DevArray(pv, n, "<i8"), device=dev)
    else:
        slots = torch.zeros(0, dtype=torch.int32, device=dev)
        vals = torch.zeros(0, dtype=torch.int64, device=dev)
    gs, gv, sizes = gather_entries(slots, vals, group)
    torch.cuda.synchronize(dev)            # gathered lists complete before the library's stream reads them
    imported = 0
    for r, k in enumerate(sizes):
        if r != rank and k:
            handler.alive_import_entries(gs[r].data_ptr(), gv[r].data_ptr(), k)
            imported += k
    handler.sync()                         # the gathered tensors may be freed after this
    return imported


# ---- hash-range exchange (option ii) ------------------------------------------------
# exchange_alive_entries leaves the WHOLE merged table on every rank: every rank receives and imports
# every other rank's entries (traffic and atomics grow with the world size).  When only the number of
# alive keys is wanted — which is all the report prints (src/main.rs:141-147) — a hash range per rank
# suffices: rank r owns the slots [ceil(r * 2^32 / world), ceil((r+1) * 2^32 / world)), receives only the
# entries of its range (all-to-all: every link carries 1/world of the entries, all 7 xGMI links in
# parallel), merges them by MAX, counts its range and the counts are summed.

def hash_range(rank: int, world: int):
    """Slots owned by `rank`: owner(slot) == (slot * world) >> 32."""
    lo = -((-rank * (1 << 32)) // world)
    hi = -((-(rank + 1) * (1 << 32)) // world)
    return lo, hi


def route_entries_by_hash_range(slots, vals, group=None):
    """all-to-all of (slot u32-as-i32, value u64-as-i64) entries: each entry goes to the rank that owns
    its slot.  Returns (slots, vals) received by this rank (its own entries of its range included).
    Works on device tensors (RCCL) and CPU tensors (gloo)."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    owner = ((slots.to(torch.int64) & 0xFFFFFFFF) * world) >> 32
    order = torch.argsort(owner, stable=True)
    send_slots, send_vals = slots[order].contiguous(), vals[order].contiguous()
    send_counts = torch.bincount(owner, minlength=world).to(torch.int64)
    recv_counts = torch.empty_like(send_counts)
    dist.all_to_all_single(recv_counts, send_counts, group=group)
    ss, rs = send_counts.tolist(), recv_counts.tolist()
    recv_slots = torch.empty(sum(rs), dtype=slots.dtype, device=slots.device)
    recv_vals = torch.empty(sum(rs), dtype=vals.dtype, device=vals.device)
    dist.all_to_all_single(recv_slots, send_slots, rs, ss, group=group)
    dist.all_to_all_single(recv_vals, send_vals, rs, ss, group=group)
    return recv_slots, recv_vals


def exchange_alive_by_hash_range(handler, device, group=None) -> int:
    """The global number of alive keys of a partition-sharded run (every rank gets the same number).
    Afterwards a rank's table is merged for its own hash range only."""
    import torch
    import torch.distributed as dist
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    ps, pv, n = handler.alive_export_entries()
    dev = torch.device("cuda", device)
    if n:
        slots = torch.as_tensor(_DevArray(ps, n, "<i4"), device=dev)
        vals = torch.as_tensor(_DevArray(pv, n, "<i8"), device=dev)
    else:
        slots = torch.zeros(0, dtype=torch.int32, device=dev)
        vals = torch.zeros(0, dtype=torch.int64, device=dev)
    rslots, rvals = route_entries_by_hash_range(slots, vals, group)
    torch.cuda.synchronize(dev)            # received lists complete before the library's stream reads them
    if rslots.numel():                     # own entries are among them: atomicMax makes that a no-op
        handler.alive_import_entries(rslots.data_ptr(), rvals.data_ptr(), rslots.numel())
    lo, hi = hash_range(rank, world)
    mine = handler.alive_count_range(lo, hi)   # synchronous: the received tensors may be freed after this
    total = torch.tensor([mine], dtype=torch.int64, device=dev)
    dist.all_reduce(total, op=dist.ReduceOp.SUM, group=group)
    return int(total.item())

// kta_internal.h — what the host code of libkta_hip.so shares between its translation units (kta_api.hip,
// kta_comm.hip, kta_kafka.hip, kta_synth.hip): the context's internal accessors, the HIP-error macro, the owners
// of device and pinned memory, streams and events, the event-pair timing pool, the description of the result
// vectors and the blob passes of the decode call (a new pass: a kind and a launch function there, a row in
// kta_kafka.hip's table).  Host code only; not installed, not part of the ABI.  The library is linked with -z defs: a
// declaration here without a definition fails the build.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "kta_hip.h"
#include "kta_kafka.h"

namespace kta {
struct WrittenList;   // kta_kernels.h
}

// ---- the context, as the other translation units see it (defined in kta_api.hip) ----------------------------------
// Sets the context's message and returns `code`.  ctx null: the thread's kta_create message (kta_last_error(NULL)).
int kta_internal_fail(kta_ctx *ctx, int code, const std::string &msg);
void kta_internal_set_error(kta_ctx *ctx, const char *msg);
void **kta_internal_ext_slot(kta_ctx *ctx, void (*free_fn)(void *));    // kta_kafka.hip's state
void **kta_internal_comm_slot(kta_ctx *ctx, void (*free_fn)(void *));   // kta_comm.hip's state
int kta_internal_device(kta_ctx *ctx);
hipStream_t kta_internal_stream(kta_ctx *ctx);
hipStream_t kta_internal_copy_stream(kta_ctx *ctx);
bool kta_internal_timing(kta_ctx *ctx);
uint32_t kta_internal_partitions(kta_ctx *ctx);
bool kta_internal_want_keys(kta_ctx *ctx);   // -c, the key sketch, the hot keys or the partitioner: the handlers read key_off / key_bytes
bool kta_internal_count_alive(kta_ctx *ctx);
bool kta_internal_alive_table(kta_ctx *ctx);
bool kta_internal_compaction(kta_ctx *ctx);    // KTA_FLAG_COMPACTION
uint64_t *kta_internal_table(kta_ctx *ctx);
int64_t *kta_internal_running(kta_ctx *ctx);
bool kta_internal_written(kta_ctx *ctx, kta::WrittenList *out);
uint64_t kta_internal_take_seq(kta_ctx *ctx, uint64_t n);
// ---- the blob passes ------------------------------------------------------------------------------------------------
// The passes that the decode call (kta_kafka.hip's kta_kafka_decode_device) runs over its descriptors and blob behind the
// decode kernel, one per opt-in section, in the order they are enqueued on the stream.  A new pass adds a kind here, a case
// in kta_internal_blob_pass, a launch function of the signature below and a row in kta_kafka.hip's table (blob_passes): the
// decode call's loop, the timers and the pass's kta_*_info go by that row.
enum kta_blob_pass_kind {
    KTA_PASS_RECORD_BATCHES = 0,   // KTA_FLAG_RECORD_BATCHES  (kta_record_batches.hip)
    KTA_PASS_PAYLOAD,              // KTA_FLAG_PAYLOAD         (kta_payload.hip)
    KTA_PASS_HEADER_NAMES,         // KTA_FLAG_HEADER_NAMES    (kta_header_names.hip)
    KTA_PASS_VALUE_BYTES,          // KTA_FLAG_VALUE_BYTES     (kta_value_bytes.hip)
    KTA_PASS_COMPRESS_WHATIF,      // KTA_FLAG_COMPRESS_WHATIF (kta_lz4_model.hip)
    KTA_PASS_KINDS
};
// What the decode call needs of a pass.  info: the pass's work counters u64[4] on the device (header names: spills, claims,
// cache flushes, 0; value bytes: mid-pass flushes, partition flushes, 0, 0), null where the pass has none.  names: the
// header-name section's table kta_header_name[2][1024] on the device, null for every other pass.  variant: the form of the
// value-byte pass's LDS add, the A/B switch of tools/bench_value_bytes.py (KTA_VALUE_BYTES_VARIANT, read when a context is
// created): 0 a dword of four equal bytes is one add, 1 every byte its own add, 2 whichever bytes of a dword are equal are
// added once; 0 for every other pass.
struct kta_internal_pass {
    bool on;         // the section's flag alone
    uint64_t *vec;   // the live vector (device)
    uint64_t *info;
    void *names;
    int variant;
};
// Returns whether the pass runs now: the flag on and no compaction replay (the replay reads the source a second time;
// batches and records are counted once).
bool kta_internal_blob_pass(kta_ctx *ctx, int kind, kta_internal_pass *out);
// The context's filter (kta_set_filter: INT64_MIN / INT64_MAX no bound; the partition set on the device, null without one)
// and its device's compute units, the same for every pass.
struct kta_internal_pass_env {
    int64_t from_ms, to_ms;
    const uint32_t *bitmap;
    int cu_count;
};
kta_internal_pass_env kta_internal_blob_pass_env(kta_ctx *ctx);
// One pass over `n` descriptors (device memory, after the call's inflate and decode kernels) and the blob they index, its
// inflate area included.  Each launch function reads the fields it uses, checks them (the record walks want the blob
// 16-byte aligned) and has its own grid rule.  *workgroups = the grid.
namespace kta {
struct BlobPassArgs {
    const kta_kafka_batch_desc *descs;
    uint64_t n;
    const uint8_t *blob;
    uint64_t blob_len;
    uint32_t P;
    int64_t from_ms, to_ms;   // kta_internal_pass_env
    const uint32_t *bitmap;
    uint64_t *vec, *info;     // kta_internal_pass
    void *names;
    int cu_count, variant;
};
typedef hipError_t BlobPassLaunch(const BlobPassArgs &a, uint32_t *workgroups, hipStream_t s);
BlobPassLaunch launch_record_batches, launch_payload, launch_header_names, launch_value_bytes, launch_lz4_model;
}
// Before a producer stores the raw layout into records [0, n) of a device batch: the tiles of a tile-compact
// allocation that the range overlaps become raw (partition, ts_ms and, in a keyless allocation, the lengths), on the
// compute stream.
int kta_internal_prepare_raw(kta_ctx *ctx, const kta_batch *d, uint64_t n);
// A device batch resolved: the allocation's columns and the batch's first record there (hdr null: the raw layout, the
// batch's own columns) — what kta_api.hip itself works with and builds the kernels' column structs from.
// keyless: an allocation of the context's without key columns — the only kind whose tiles may hold u16 lengths.
struct kta_internal_columns {
    int32_t *partition, *key_len, *val_len;
    int64_t *ts_ms;
    kta_tile_hdr *hdr;
    uint64_t rec0;
    bool keyless;
    uint64_t rows;       // records the allocation's columns hold (whole tiles); 0 unless an allocation of the context's
    kta_tile_sum *sum;   // the allocation's tile summaries (kta_tile.h: behind its headers), entry t beside hdr[t]; null for
                         // everything but an allocation of the context's: the raw layout, a hand-built batch's own tile_hdr
    uint32_t *mark;      // the allocation's plane marks (kta_tile.h: behind its summaries), entry t beside sum[t]; null where sum is
    uint32_t *size;      // the allocation's size extrema (kta_tile.h: behind its marks), two words per tile; null where mark is
};
int kta_internal_resolve(kta_ctx *ctx, const kta_batch *d, kta_internal_columns *out);

// ---- result vectors -----------------------------------------------------------------------------------------------
// Every section of the result is a u64 vector of the shape below.  The kinds before KTA_RV_KINDS have a snapshot that
// kta_finish_device takes and kta_exchange reduces in place: words [0, sum_words) with u64 SUM, words [sum_words, words)
// with MAX (i64 when max_signed, else u64).  The kinds behind it are live only: read back, never exchanged.  A new opt-in
// section adds a kind here and a row in kta_api.hip's section table (sections_of), which is all the host layer reads:
// create, reset, the snapshot, the read-back and kta_internal_result_vectors go by that row.
//
//   kind        u64 words          SUM prefix     MAX suffix
//   counters    P*7 + 8            P*7 + 4        4      (i64)
//   analytics   68 + 4*P           68             4*P    (i64)
//   timeline    (n_buckets+3)*3    all            none
//   key sketch  P*4096             none           all    (u64)
//   hot keys    2*1024*23          all            none
//   ts order    3*P + 64           2*P + 64       P      (i64)
//   partitioner 2*P + 2*Q          all            none
//   size quant. P*3*464 + 8        all            none
//   segments    (P*M + P)*4 + 8    all but 5      5      (u64: S, M, overhead and two zero words, equal on every rank)
//   rec.batches 20*P + 1524        16*P + 500     4*P + 1024 (u64: the partitions' maxima and the producer sketch)
//   payload     24*P + 69648       all            none
//   hdr. names  73736              all            none   (the name table beside it stays on its rank)
//   value bytes 264*P              all            none
//   compr. w.-if 8*P + 20          all            none
//   compaction  5*P + 6            (live only: the replay's vector, kta_get_compaction)
//   kept        (P*M + P)*4 + 8    (live only: the replay's kept vector, kta_get_compact_delete; the segments' shape)
struct ResultVector {
    uint64_t *out;     // the snapshot (device); null: the context has no such section
    size_t words, sum_words;
    bool max_signed;
};
enum { KTA_RV_COUNTERS = 0, KTA_RV_ANALYTICS, KTA_RV_TIMELINE, KTA_RV_KEY_SKETCH, KTA_RV_HOT_KEYS, KTA_RV_TS_ORDER, KTA_RV_PARTITIONER,
       KTA_RV_SIZE_QUANTILES, KTA_RV_SEGMENTS, KTA_RV_RECORD_BATCHES, KTA_RV_PAYLOAD, KTA_RV_HEADER_NAMES, KTA_RV_VALUE_BYTES,
       KTA_RV_COMPRESS_WHATIF, KTA_RV_KINDS,
       KTA_SEC_COMPACTION = KTA_RV_KINDS, KTA_SEC_KEPT, KTA_SEC_KINDS };
// The snapshot kinds of the section table; a section that is off has out == nullptr and words == 0.
void kta_internal_result_vectors(kta_ctx *ctx, ResultVector rv[KTA_RV_KINDS]);
// The refusal of an entry point whose section (a kind above) is off: KTA_ERR_INVALID with the section table's message.
int kta_internal_section_off(kta_ctx *ctx, int kind);

// ---- errors -------------------------------------------------------------------------------------------------------
static inline int fail(kta_ctx *ctx, int code, const std::string &msg) { return kta_internal_fail(ctx, code, msg); }

// "<what>: <hipGetErrorString>"; out of memory is KTA_ERR_NOMEM, everything else KTA_ERR_HIP
static inline int hip_fail(kta_ctx *ctx, hipError_t e, const char *what)
{
    return fail(ctx, e == hipErrorOutOfMemory ? KTA_ERR_NOMEM : KTA_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// a step that fails ends the function, reported under `what`
#define KTA_HIP_AS(ctx, call, what)                                \
    do {                                                           \
        hipError_t e__ = (call);                                   \
        if (e__ != hipSuccess) return hip_fail(ctx, e__, what);    \
    } while (0)
#define KTA_HIP(ctx, call) KTA_HIP_AS(ctx, call, #call)

// ---- owners -------------------------------------------------------------------------------------------------------
// Move-only owner of `size()` elements of device (hipMalloc) or pinned host (hipHostMalloc) memory.
template <class T, bool Pinned> class HipBuf {
    T *p_ = nullptr;
    size_t n_ = 0;

public:
    HipBuf() = default;
    HipBuf(const HipBuf &) = delete;
    HipBuf &operator=(const HipBuf &) = delete;
    HipBuf(HipBuf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    HipBuf &operator=(HipBuf &&o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_, n_ = o.n_;
            o.p_ = nullptr, o.n_ = 0;
        }
        return *this;
    }
    ~HipBuf() { reset(); }
    T *get() const { return p_; }
    size_t size() const { return n_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset()
    {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr, n_ = 0;
    }
    // The growth policy of every buffer here: release first, then allocate n elements (the caller chooses n, and waits
    // for whatever may still read the old memory).  Goes inside KTA_HIP; after a failure the owner is empty.
    hipError_t alloc(size_t n)
    {
        reset();
        void *p = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&p, n * sizeof(T));
        if (e == hipSuccess) p_ = static_cast<T *>(p), n_ = n;
        return e;
    }
};
template <class T> using DeviceBuf = HipBuf<T, false>;
template <class T> using PinnedBuf = HipBuf<T, true>;

// Move-only owner of a stream or an event: `Create(x.put(), ...)` fills it.
template <class H, hipError_t (*Destroy)(H)> class HipHandle {
    H h_ = nullptr;

public:
    HipHandle() = default;
    HipHandle(const HipHandle &) = delete;
    HipHandle &operator=(const HipHandle &) = delete;
    HipHandle(HipHandle &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    HipHandle &operator=(HipHandle &&o) noexcept
    {
        if (this != &o) {
            reset();
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    ~HipHandle() { reset(); }
    H get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }
    H *put()
    {
        reset();
        return &h_;
    }
    void reset()
    {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }
};
using Stream = HipHandle<hipStream_t, hipStreamDestroy>;
using Event = HipHandle<hipEvent_t, hipEventDestroy>;

// ---- timing ---------------------------------------------------------------------------------------------------------
// HIP-event pairs recorded around the kernels of `Kinds` kinds on one stream (no host synchronisation while recording),
// drained into a sum and a count per kind.  A kind holds at most max_events events before it drains.
template <int Kinds> struct TimerPool {
    size_t max_events;
    std::vector<Event> ev[Kinds];
    size_t used[Kinds] = {};
    double ms_sum[Kinds] = {};
    uint64_t ms_cnt[Kinds] = {};

    explicit TimerPool(size_t max_events_) : max_events(max_events_) {}

    int drain(kta_ctx *ctx, hipStream_t s)
    {
        KTA_HIP(ctx, hipStreamSynchronize(s));
        for (int k = 0; k < Kinds; k++) {
            for (size_t i = 0; i + 1 < used[k]; i += 2) {
                float ms = 0.f;
                KTA_HIP(ctx, hipEventElapsedTime(&ms, ev[k][i].get(), ev[k][i + 1].get()));
                ms_sum[k] += ms;
                ms_cnt[k] += 1;
            }
            used[k] = 0;
        }
        return KTA_OK;
    }

    // next (start, stop) event pair of kernel kind k
    int pair(kta_ctx *ctx, hipStream_t s, int k, hipEvent_t *a, hipEvent_t *b)
    {
        if (used[k] + 2 > max_events) {
            int rc = drain(ctx, s);
            if (rc != KTA_OK) return rc;
        }
        while (ev[k].size() < used[k] + 2) {
            Event e;
            KTA_HIP(ctx, hipEventCreate(e.put()));
            ev[k].push_back(std::move(e));
        }
        *a = ev[k][used[k]].get();
        *b = ev[k][used[k] + 1].get();
        used[k] += 2;
        return KTA_OK;
    }

    // drain, report the averages (-1: no launch) and start over
    int stats(kta_ctx *ctx, hipStream_t s, float *avg_ms, uint64_t *launches)
    {
        int rc = drain(ctx, s);
        if (rc != KTA_OK) return rc;
        for (int k = 0; k < Kinds; k++) {
            launches[k] = ms_cnt[k];
            avg_ms[k] = ms_cnt[k] ? (float)(ms_sum[k] / (double)ms_cnt[k]) : -1.f;
            ms_sum[k] = 0;
            ms_cnt[k] = 0;
        }
        return KTA_OK;
    }
};

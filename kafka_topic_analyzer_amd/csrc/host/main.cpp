// main.cpp — `kta-analyzer`: the reference's command line (src/main.rs:29-180) in front of the
// MI355X metric-accumulation path.  Flags, defaults and the printed report are the reference's:
//
//   -t, --topic <TOPIC>                         (required)           main.rs:37-44
//   -b, --bootstrap-server <BOOTSTRAP_SERVER>   (required)           main.rs:45-52
//       --librdkafka <LIBRDKAFKA>               k=v,k=v              main.rs:53-59, 84-92
//   -c, --count-alive-keys                                           main.rs:60-66, 77-80
//   -h/--help, -V/--version ("0.4.1", main.rs:35)
//
// The record source is chosen by the scheme of --bootstrap-server:
//     <host:port,...>                    a Kafka cluster, through the reference's consume loop (src/kafka.rs)
//                                        over librdkafka, which is bound at run time (host/rdkafka_source.hpp);
//                                        "Consumer creation failed" when the library is not installed
//     synthetic://<c1..c5>[?records=N]   the synthetic topic of include/kta_synth.h
//     dump://<path>                      a KTADUMP1 topic dump (host/dump.hpp)
//     segment://<f0>[,<f1>...]           raw Kafka log segments (`*.log` files of a broker, record-batch
//                                        v2; uncompressed, gzip, Snappy, LZ4, zstd): file k is partition k; decoded ON THE GPU
//                                        (include/kta_kafka.h), the host only walks batch headers
// Extra knobs travel in --librdkafka as kta.* keys (kta.device=N, kta.gpus=N,
// kta.batch=N, kta.write_dump=<path>, kta.per_message=1, kta.analytics=1, kta.timeline=<width>, kta.distinct_keys=1, kta.hot_keys=K,
// kta.ts_order=1, kta.partitioner=murmur2, kta.repartition=Q), so
// no flag is added or renamed.
// kta.gpus=N (synthetic:// and segment:// sources) shards the topic's partitions over N GPUs, partition p on
// rank p % N, one host thread + one context + one communicator rank per GPU (device (kta.device + r) mod the
// visible devices), and replaces "the report reads the handlers" by ONE exchange step (kta_exchange: RCCL).
// kta.per_message=1 drives the handler exactly like the reference's loop (kafka.rs:107-109): one
// MetricHandler::handle_message call per record instead of filling columns.
// kta.analytics=1 (every source, kta.gpus=N included) accumulates the additive analytics as well (KTA_FLAG_ANALYTICS:
// key / value size histograms, per-partition timestamp and size extrema; no reference counterpart) and prints them
// in a section of their own AFTER the reference report, which stays byte for byte what it is without the knob.
// kta.timeline=<width> (30s, 15m, 1h, 1d; a bare number is seconds; every source, kta.gpus=N included) accumulates a
// timeline as well (kta_set_timeline: records, tombstones and bytes per time bucket; no reference counterpart):
// kta.timeline.buckets=N buckets (default 168), from kta.timeline.start=<unix seconds> or else so that the last
// bucket holds the run's start time.  Printed in a section of its own after the report (and the analytics).
// kta.distinct_keys=1 (every source, kta.gpus=N included) keeps a HyperLogLog sketch of the key hashes per partition as well
// (KTA_FLAG_KEY_SKETCH; no reference counterpart) and prints the estimated distinct keys per partition and of the topic in a
// section of its own after the report (and the analytics and the timeline).
// kta.percentiles=1 (0: off; every source, kta.per_message=1 and kta.gpus=N included) runs the size-percentile pass as well
// (KTA_FLAG_SIZE_QUANTILES; no reference counterpart) and prints, after the report's closing rule and the analytics, p50,
// p90, p99, p99.9 and the largest of the key, value and message sizes per partition and of the topic.
// kta.segments=<size> (1g, 512m, 64k or bytes; every source, kta.per_message=1 and kta.gpus=N included) runs the segment pass of
// the retention what-if as well (kta_set_segments; no reference counterpart) and prints, after the partitioner and compaction
// sections and before the filter's, every partition's model segments, records and bytes and — with kta.retention.ms=<duration>
// and / or kta.retention.bytes=<size>, at kta.retention.now=<unix seconds> (default: the run's start) — what the policy would
// keep.  kta.segments.rows=M (default 1024, lowered so that P * M <= 2^20) and kta.segments.overhead=B (default 0) set the model.
// kta.record_batches=1 (0: off; segment:// sources only, kta.gpus=N and -c included, not with kta.per_message=1: the other
// sources deliver records, not batches) runs the record-batch pass as well (KTA_FLAG_RECORD_BATCHES) and prints its section
// behind every other one: records and bytes per batch, compression per codec, offset holes, producers.
// kta.payload=1 (0: off; segment:// sources only, kta.gpus=N and -c included, not with kta.per_message=1: the pass reads the record
// bytes of the raw log) runs the payload pass as well (KTA_FLAG_PAYLOAD) and prints its section behind every other one: value
// formats, schema-registry ids, record headers.
// kta.headers=1 (0: off; the same sources and refusals as kta.payload=1, with or without it) runs the header-name pass as well
// (KTA_FLAG_HEADER_NAMES) and prints its section behind the payload section's position: the names of the record headers with
// their occurrences, bytes and null values.  Under kta.gpus=N a listed name comes from the lowest rank that holds it.
// kta.value_bytes=1 (0: off; the same sources and refusals as kta.payload=1, with or without it) runs the value-byte pass as well
// (KTA_FLAG_VALUE_BYTES) and prints its section behind the header-name section's position: per partition and for the topic a
// byte histogram's read-off — H0, the order-0 floor, the printable, zero, high-bit and repeat shares and a class.
// kta.compress_whatif=lz4 (the same sources and refusals as kta.payload=1, with or without the sections above; any other value
// is refused) runs the compression what-if as well (KTA_FLAG_COMPRESS_WHATIF) and prints its section behind the value-byte
// section's position: per partition, for the topic and by the batches' current codec the bytes a defined LZ4 compressor would
// leave of the records sections, beside what they take on disk now.
// kta.ts_order=1 (0: off; every source, kta.per_message=1 and kta.gpus=N included) runs the timestamp-order pass as well
// (KTA_FLAG_TS_ORDER; no reference counterpart) and prints, after those sections and before the hot keys, the late records
// per partition — older than one their partition delivered before them — and a histogram of their lateness.
// kta.partitioner=murmur2 (every source, kta.per_message=1 and kta.gpus=N included; any other value is refused — crc32, the
// hash of librdkafka's own default partitioner, may follow) runs the partitioner pass as well (KTA_FLAG_PARTITIONER; no
// reference counterpart) and prints, last of all, how many keyed records lie on the partition Kafka's default partitioner
// gives their key, and how the keyed records and bytes would spread over Q partitions: kta.repartition=Q (a decimal in
// [1, kta_partitioner_max_partitions()]; needs kta.partitioner), P when it is not given.
// kta.from=<epoch seconds>, kta.to=<epoch seconds> (the unit of kta.timeline.start) and kta.partitions=0,3-5 (every source,
// kta.per_message=1 and kta.gpus=N included: every rank gets the same filter) analyse only the records with
// from <= timestamp < to of the partitions named (kta_set_filter): the report and every opt-in section describe those
// records and no others, and one more section after everything else says what the filter was and how many records it
// was shown and let pass (summed over the ranks).  The items of kta.partitions are separated by commas, which also separate
// --librdkafka's pairs: a piece without '=' that follows kta.partitions and is a number or a range belongs to it.
// kta.compact_delete=1 (0: off; with kta.compaction=1 and kta.segments=<size>; it inherits the compaction knob's refusals) joins
// the two what-ifs: the replay also counts the survivors per model segment (kta_set_compact_delete), and a section after the
// retention section says what cleanup.policy=compact,delete would keep under the kta.retention.* policy.
// kta.compaction=1 (0: off; with -c; synthetic://, segment:// and dump:// sources, one GPU, not with kta.per_message=1) answers
// what log compaction would keep (KTA_FLAG_COMPACTION; no reference counterpart): after the first pass the source is fed a
// second time in replay mode, and a section with the records and bytes kept per partition is printed after the
// partitioner section and before the filter section.
// kta.hot_keys=K (1 <= K <= 64; every source, kta.gpus=N included) keeps the hot-key sketch as well (KTA_FLAG_HOT_KEYS; no
// reference counterpart) and prints, last of all, the at most K keys that hold 1/512 of the keyed records and more, with
// bounds on their records and, where the device caught one, the key's bytes (with kta.gpus=N from the lowest rank that
// has them).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <string>
#include <mutex>
#include <thread>
#include <vector>

#include "dump.hpp"
#include "kta_kafka.h"
#include "kta_synth.h"
#include "metric.hpp"
#include "rdkafka_source.hpp"

namespace {

// kta.timeline=<width>: a positive number with an optional unit s, m, h or d (none: seconds) -> ms; 0 when malformed
int64_t parse_timeline_width(const std::string &v)
{
    size_t i = 0;
    while (i < v.size() && v[i] >= '0' && v[i] <= '9') i++;
    if (i == 0 || i > 15) return 0;
    const std::string unit = v.substr(i);
    int64_t mult = 0;
    if (unit.empty() || unit == "s") mult = 1000;
    else if (unit == "m") mult = 60000;
    else if (unit == "h") mult = 3600000;
    else if (unit == "d") mult = 86400000;
    else return 0;
    const int64_t n = strtoll(v.substr(0, i).c_str(), nullptr, 10);
    if (n <= 0 || n > INT64_MAX / mult) return 0;
    return n * mult;
}

// a non-negative decimal integer of at most `digits` digits, else -1
int64_t parse_decimal(const std::string &v, size_t digits)
{
    if (v.empty() || v.size() > digits) return -1;
    for (char ch : v)
        if (ch < '0' || ch > '9') return -1;
    return strtoll(v.c_str(), nullptr, 10);
}

// a size as kta.segments and kta.retention.bytes take it: bytes, or a number of k / m / g (powers of 1024); -1 when malformed
int64_t parse_size(const std::string &v)
{
    size_t i = 0;
    while (i < v.size() && v[i] >= '0' && v[i] <= '9') i++;
    if (i == 0 || i > 15) return -1;
    const std::string unit = v.substr(i);
    int shift = 0;
    if (unit.empty()) shift = 0;
    else if (unit == "k" || unit == "K") shift = 10;
    else if (unit == "m" || unit == "M") shift = 20;
    else if (unit == "g" || unit == "G") shift = 30;
    else return -1;
    const int64_t n = strtoll(v.substr(0, i).c_str(), nullptr, 10);
    if (n > (INT64_MAX >> shift)) return -1;
    return n << shift;
}

// kta.segments=<size> with kta.segments.rows / kta.segments.overhead, and the policy kta.retention.ms / .bytes / .now
struct SegmentsConfig {
    bool on = false;
    uint64_t S = 0;
    uint32_t M = 0, overhead = 0;
    int64_t retention_ms = -1, retention_bytes = -1, now_ms = 0;
};

// kta.from / kta.to / kta.partitions as kta_set_filter takes them
struct FilterConfig {
    bool on = false, has_set = false;
    int64_t from_ms = INT64_MIN, to_ms = INT64_MAX;
    std::vector<uint32_t> bitmap;   // ceil(P / 32) words
};

bool is_partition_item(const std::string &v)
{
    if (v.empty()) return false;
    for (char ch : v)
        if ((ch < '0' || ch > '9') && ch != '-') return false;
    return true;
}

// kta.partitions=0,3-5: numbers and inclusive ranges below P; false when malformed
bool parse_partitions(const std::string &v, uint32_t P, std::vector<uint32_t> *bitmap)
{
    bitmap->assign((P + 31u) / 32u, 0u);
    size_t pos = 0;
    while (true) {
        const size_t comma = v.find(',', pos);
        const std::string item = v.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos);
        const size_t dash = item.find('-');
        const int64_t lo = parse_decimal(item.substr(0, dash), 9);
        const int64_t hi = dash == std::string::npos ? lo : parse_decimal(item.substr(dash + 1), 9);
        if (lo < 0 || hi < lo || hi >= (int64_t)P) return false;
        for (int64_t p = lo; p <= hi; p++) (*bitmap)[(size_t)p >> 5] |= 1u << (p & 31);
        if (comma == std::string::npos) return true;
        pos = comma + 1;
    }
}

void apply_filter(kta_ctx *ctx, const FilterConfig &f);

// key_non_null of partitions [0, P): the keyed records of the kta.distinct_keys section
std::vector<uint64_t> keyed_records(const kta::MessageMetrics &m, uint32_t P)
{
    std::vector<uint64_t> keyed(P);
    for (uint32_t p = 0; p < P; p++) keyed[p] = m.key_non_null((int32_t)p);
    return keyed;
}

// total_messages of partitions [0, P): the records of the kta.ts_order section
std::vector<uint64_t> total_records(const kta::MessageMetrics &m, uint32_t P)
{
    std::vector<uint64_t> total(P);
    for (uint32_t p = 0; p < P; p++) total[p] = m.total((int32_t)p);
    return total;
}

// the per-partition words of the counter vector that the kta.partitioner section reads
std::vector<uint64_t> partitioner_counters(const kta::MessageMetrics &m, uint32_t P)
{
    std::vector<uint64_t> c((size_t)P * KTA_NCOUNTERS + KTA_NGLOBALS, 0);
    for (uint32_t p = 0; p < P; p++) {
        uint64_t *r = c.data() + (size_t)p * KTA_NCOUNTERS;
        r[KTA_C_KEY_NULL] = m.key_null((int32_t)p), r[KTA_C_KEY_NON_NULL] = m.key_non_null((int32_t)p);
        r[KTA_C_KEY_SIZE_SUM] = m.key_size_sum((int32_t)p), r[KTA_C_VALUE_SIZE_SUM] = m.value_size_sum((int32_t)p);
    }
    return c;
}

constexpr uint32_t kHeaderNamesShown = 256;   // kta.headers=1: the rows of the section's table at most

// murmur3's finaliser: x = hot_fmix32(hash) places a key hash in the hot-key sketch (kta_hip.h)
uint32_t hot_fmix32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}

const char *kAbout = "Kafka Topic Analyzer 0.4.1";

void print_help()
{
    printf("%s\n\nUSAGE:\n    kafka-topic-analyzer [FLAGS] [OPTIONS] --bootstrap-server <BOOTSTRAP_SERVER> --topic <TOPIC>\n\n"
           "FLAGS:\n"
           "    -c, --count-alive-keys    Counts the effective number of alive keys in a log compacted topic by saving the "
           "state for each key in a local file and counting the result at the end of the read operation.A key is 'alive' "
           "when it is present and has a non-null value in it's latest-offset version\n"
           "    -h, --help                Prints help information\n"
           "    -V, --version             Prints version information\n\n"
           "OPTIONS:\n"
           "    -b, --bootstrap-server <BOOTSTRAP_SERVER>    Bootstrap server(s) to work with, comma separated\n"
           "        --librdkafka <LIBRDKAFKA>                Options to pass into the underlying librdkafka, comma "
           "seperated key=value pairs\n"
           "    -t, --topic <TOPIC>                          The topic to analyze\n",
           kAbout);
}

[[noreturn]] void usage_error(const std::string &msg)
{
    fprintf(stderr, "error: %s\n\nUSAGE:\n    kafka-topic-analyzer [FLAGS] [OPTIONS] --bootstrap-server "
                    "<BOOTSTRAP_SERVER> --topic <TOPIC>\n\nFor more information try --help\n", msg.c_str());
    exit(1);
}

std::mutex g_rank_panic_mutex;           // a panic of a rank thread of a sharded run, kept for the main thread
bool g_rank_panicked = false;
std::string g_rank_panic_msg, g_rank_panic_loc;

[[noreturn]] void rust_panic(const std::string &msg, const std::string &loc)
{
    fprintf(stderr, "thread 'main' panicked at '%s', %s\n", msg.c_str(), loc.c_str());
    exit(101);
}

struct Args {
    std::string topic, bootstrap, librdkafka;
    bool has_topic = false, has_bootstrap = false, has_librdkafka = false;
    int count_alive_occurrences = 0;
};

Args parse_args(int argc, char **argv)
{
    Args a;
    auto take = [&](int &i, const std::string &name, const char *inline_val) -> std::string {
        if (inline_val) return inline_val;
        if (i + 1 >= argc) usage_error("The argument '" + name + "' requires a value but none was supplied");
        return argv[++i];
    };
    for (int i = 1; i < argc; i++) {
        std::string s = argv[i];
        const char *eq = nullptr;
        std::string name = s;
        if (s.rfind("--", 0) == 0) {
            size_t p = s.find('=');
            if (p != std::string::npos) { name = s.substr(0, p); eq = argv[i] + p + 1; }
        } else if (s.size() > 2 && s[0] == '-' && s[1] != '-') {
            name = s.substr(0, 2);
            eq = argv[i] + 2;
            if (name == "-c" || name == "-h" || name == "-V") { eq = nullptr; name = s; }
        }
        if (name == "-t" || name == "--topic") { a.topic = take(i, "--topic <TOPIC>", eq); a.has_topic = true; }
        else if (name == "-b" || name == "--bootstrap-server") { a.bootstrap = take(i, "--bootstrap-server <BOOTSTRAP_SERVER>", eq); a.has_bootstrap = true; }
        else if (name == "--librdkafka") { a.librdkafka = take(i, "--librdkafka <LIBRDKAFKA>", eq); a.has_librdkafka = true; }
        else if (name == "-c" || name == "--count-alive-keys") {
            if (++a.count_alive_occurrences > 1)   // clap 2: a flag that is not `multiple(true)` may appear once
                usage_error("The argument '--count-alive-keys' was provided more than once, but cannot be used multiple times");
        }
        else if (name == "-h" || name == "--help") { print_help(); exit(0); }
        else if (name == "-V" || name == "--version") { printf("%s\n", kAbout); exit(0); }
        else usage_error("Found argument '" + s + "' which wasn't expected, or isn't valid in this context");
    }
    if (!a.has_topic || !a.has_bootstrap) {
        std::string m = "The following required arguments were not provided:";
        if (!a.has_bootstrap) m += "\n    --bootstrap-server <BOOTSTRAP_SERVER>";
        if (!a.has_topic) m += "\n    --topic <TOPIC>";
        usage_error(m);
    }
    return a;
}

// main.rs:84-92: split(",") then split('=') taking the first two pieces; a pair without '=' panics
std::map<std::string, std::string> parse_librdkafka(const Args &a)
{
    std::map<std::string, std::string> m;
    if (!a.has_librdkafka) return m;
    size_t pos = 0;
    const std::string &s = a.librdkafka;
    std::string last_key;
    while (true) {
        size_t comma = s.find(',', pos);
        std::string kv = s.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos);
        size_t eq = kv.find('=');
        if (eq == std::string::npos && last_key == "kta.partitions" && is_partition_item(kv)) {   // kta.partitions=0,3-5: the next item
            m[last_key] += "," + kv;
            if (comma == std::string::npos) break;
            pos = comma + 1;
            continue;
        }
        if (eq == std::string::npos)
            rust_panic("called `Option::unwrap()` on a `None` value", "src/main.rs:89:48");
        last_key = kv.substr(0, eq);
        size_t eq2 = kv.find('=', eq + 1);
        m[kv.substr(0, eq)] = kv.substr(eq + 1, eq2 == std::string::npos ? std::string::npos : eq2 - eq - 1);
        if (comma == std::string::npos) break;
        pos = comma + 1;
    }
    return m;
}

void check(int rc, kta_ctx *ctx, const char *what)
{
    if (rc != KTA_OK) {
        fprintf(stderr, "%s failed: %s\n", what, kta_last_error(ctx));
        exit(2);
    }
}

void apply_filter(kta_ctx *ctx, const FilterConfig &f)
{
    if (f.on) check(kta_set_filter(ctx, f.from_ms, f.to_ms, f.has_set ? f.bitmap.data() : nullptr, (uint32_t)f.bitmap.size()), ctx, "kta_set_filter");
}

// ---- kta.gpus=N: one rank per GPU ------------------------------------------------------------------------
struct ShardedJob {
    std::string topic;
    bool count_alive = false, synthetic = false, check_crcs = false;
    int device = 0, nranks = 1;
    uint64_t batch = 1ull << 20;
    uint32_t P = 0;
    kta_synth_spec spec{};
    bool oversubscribe = false;                        // kta.oversubscribe=1: several ranks may share a device (test doubles of RCCL)
    bool analytics = false;                            // kta.analytics=1: every rank's context, exchanged with the counters
    kta::TimelineConfig timeline;                      // kta.timeline=<width>: derived once, the same on every rank
    bool distinct_keys = false;                        // kta.distinct_keys=1: every rank's context, exchanged with the counters
    uint32_t hot_keys = 0;                             // kta.hot_keys=K: likewise; the exemplars stay on their ranks
    bool ts_order = false;                             // kta.ts_order=1: likewise (a partition's records stay on one rank)
    bool partitioner = false;                          // kta.partitioner=murmur2: likewise
    uint32_t repartition = 0;                          //   kta.repartition=Q (0: P)
    bool percentiles = false;                          // kta.percentiles=1: likewise
    bool record_batches = false;                       // kta.record_batches=1: likewise (segment:// only)
    uint64_t rb_skipped[3] = {0, 0, 0};                //   control batches, magic 0/1 sets, unknown codecs: the host index's, whole topic
    bool payload = false;                              // kta.payload=1: likewise (segment:// only)
    bool headers = false;                              // kta.headers=1: likewise (segment:// only); the name tables stay on their ranks
    bool value_bytes = false;                          // kta.value_bytes=1: likewise (segment:// only)
    bool compress_whatif = false;                      // kta.compress_whatif=lz4: likewise (segment:// only)
    FilterConfig filter;                              // kta.from / kta.to / kta.partitions: the same on every rank
    SegmentsConfig segments;                           // kta.segments=<size>: every rank's context (a partition's records stay on one rank)
    uint64_t n_records = 0;
    std::vector<std::vector<uint8_t>> segment_bytes;   // segment:// : file k is partition k
    std::vector<uint64_t> base_seq;                    //   global sequence number of each partition's first record
    std::vector<int64_t> start_offsets, end_offsets;
};

// What one rank consumes: the partitions p with p % nranks == rank, every record with its GLOBAL sequence
// number (the position the single-GPU run consumes it at), then the exchange.
void run_rank(const ShardedJob &job, int rank, const uint8_t *uid, int ndev, kta::HipMetricHandler **out, int64_t *filter_counts /* [2] */)
{
    try {
        // a rank's records are not consecutive in consumption order: global sequence numbers, table state
        const uint32_t flags = (job.count_alive ? (job.synthetic ? KTA_FLAG_SEQ_COLUMN : KTA_FLAG_ALIVE_TABLE) : 0u) |
                               (job.analytics ? KTA_FLAG_ANALYTICS : 0u) | (job.distinct_keys ? KTA_FLAG_KEY_SKETCH : 0u) |
                               (job.hot_keys ? KTA_FLAG_HOT_KEYS : 0u) | (job.ts_order ? KTA_FLAG_TS_ORDER : 0u) |
                               (job.partitioner ? KTA_FLAG_PARTITIONER : 0u) | (job.percentiles ? KTA_FLAG_SIZE_QUANTILES : 0u) |
                               (job.record_batches ? KTA_FLAG_RECORD_BATCHES : 0u) | (job.payload ? KTA_FLAG_PAYLOAD : 0u) |
                               (job.headers ? KTA_FLAG_HEADER_NAMES : 0u) | (job.value_bytes ? KTA_FLAG_VALUE_BYTES : 0u) |
                               (job.compress_whatif ? KTA_FLAG_COMPRESS_WHATIF : 0u);
        const bool keys = job.count_alive || job.distinct_keys || job.hot_keys || job.partitioner;   // the staging batches carry key_off / key_bytes
        kta::HipMetricHandler *h = new kta::HipMetricHandler((int32_t)job.P, job.count_alive, (job.device + rank) % ndev,
                                                             job.batch, 0, flags, job.timeline, job.repartition);
        kta_ctx *ctx = h->ctx();
        if (job.segments.on) h->set_segments(job.segments.S, job.segments.M, job.segments.overhead);
        apply_filter(ctx, job.filter);
        h->comm_create(job.nranks, rank, uid);
        if (job.synthetic) {
            // every rank enumerates the whole topic in consumption order and keeps its partitions
            std::vector<int32_t> part(job.batch), kl(job.batch), vl(job.batch);
            std::vector<int64_t> ts(job.batch);
            std::vector<uint32_t> ko(job.batch);
            std::vector<uint8_t> kbuf;
            kta_batch hb{};
            bool open = false;
            uint64_t fill = 0, fill_kb = 0;
            auto submit = [&]() {
                if (open) check(kta_batch_submit(ctx, fill, fill_kb, 0), ctx, "kta_batch_submit");
                open = false;
                fill = fill_kb = 0;
            };
            for (uint64_t at = 0; at < job.n_records;) {
                uint64_t n = std::min<uint64_t>(job.batch, job.n_records - at), kb = 0;
                kta_batch tmp{};
                tmp.partition = part.data(); tmp.key_len = kl.data(); tmp.val_len = vl.data(); tmp.ts_ms = ts.data();
                tmp.capacity = n;
                if (keys) {
                    check(kta_synth_fill_host(&job.spec, at, n, &tmp, &kb), ctx, "kta_synth_fill_host");   // key bytes needed
                    kbuf.resize(kb + 16);
                    tmp.key_off = ko.data(); tmp.key_bytes = kbuf.data(); tmp.key_bytes_capacity = kb;
                }
                check(kta_synth_fill_host(&job.spec, at, n, &tmp, &kb), ctx, "kta_synth_fill_host");
                for (uint64_t i = 0; i < n; i++) {
                    if (part[i] % job.nranks != rank) continue;
                    const uint64_t klen = keys && kl[i] > 0 ? (uint64_t)kl[i] : 0;
                    if (open && (fill == hb.capacity || fill_kb + klen > hb.key_bytes_capacity)) submit();
                    if (!open) {
                        check(kta_batch_acquire(ctx, &hb), ctx, "kta_batch_acquire");
                        open = true;
                    }
                    hb.partition[fill] = part[i]; hb.key_len[fill] = kl[i]; hb.val_len[fill] = vl[i]; hb.ts_ms[fill] = ts[i];
                    if (keys) {
                        hb.key_off[fill] = (uint32_t)fill_kb;
                        if (klen) memcpy(hb.key_bytes + fill_kb, kbuf.data() + ko[i], klen);
                        fill_kb += klen;
                    }
                    if (job.count_alive) hb.seq[fill] = at + i;
                    fill++;
                }
                at += n;
            }
            submit();
        } else {
            check(kta_kafka_set_check_crcs(ctx, job.check_crcs ? 1 : 0), ctx, "kta_kafka_set_check_crcs");
            for (uint32_t p = (uint32_t)rank; p < job.P; p += (uint32_t)job.nranks) {
                if (job.segment_bytes[p].empty()) continue;
                kta_kafka_index_stats ist;
                check(kta_seek_seq(ctx, job.base_seq[p]), ctx, "kta_seek_seq");
                check(kta_kafka_consume(ctx, job.segment_bytes[p].data(), job.segment_bytes[p].size(), (int32_t)p, &ist), ctx,
                      "kta_kafka_consume");
                if (ist.n_compressed || ist.n_old_magic)
                    fprintf(stderr, "[WARN] Kafka error: partition %u: %llu unknown-codec and %llu pre-v2 batches skipped\n", p,
                            (unsigned long long)ist.n_compressed, (unsigned long long)ist.n_old_magic);
            }
        }
        h->exchange(!job.synthetic);
        if (job.filter.on) {   // records seen and passed, summed over the ranks
            uint64_t info[6];
            check(kta_filter_info(ctx, info), ctx, "kta_filter_info");
            filter_counts[0] = (int64_t)info[0], filter_counts[1] = (int64_t)info[1];
            check(kta_comm_allreduce_i64(ctx, filter_counts, 2, 0), ctx, "kta_comm_allreduce_i64");
        }
        *out = h;
    } catch (const kta::RustPanic &p) {
        // Every rank sees the job's extrema after the exchange, so all of them end here — and exit() is not to be
        // called from several threads at once (handlers run at exit, the HIP runtime is torn down).  The panic is
        // kept for the main thread, which prints it once after joining the ranks, like the reference's one line.
        std::lock_guard<std::mutex> lock(g_rank_panic_mutex);
        if (!g_rank_panicked) {
            g_rank_panicked = true;
            g_rank_panic_msg = p.what();
            g_rank_panic_loc = p.location;
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "rank %d: %s\n", rank, e.what());
        exit(2);   // before the exchange: the other ranks would wait for this one for ever
    }
}

int run_sharded(ShardedJob &job, const std::chrono::steady_clock::time_point start_time)
{
    int ndev = 0;
    if (kta_device_count(&ndev) != KTA_OK) {
        fprintf(stderr, "kta_create failed: no HIP device visible (libkta_hip has no CPU fallback)\n");
        return 2;
    }
    // one rank per device: two ranks on one GPU would each take a 32 GiB table under -c, and real RCCL refuses
    // the second one ("duplicate GPU") while the first is still blocked in its init
    if (job.nranks > ndev && !job.oversubscribe) {
        fprintf(stderr, "kta.gpus=%d: only %d HIP device(s) visible\n", job.nranks, ndev);
        return 2;
    }
    uint8_t uid[KTA_COMM_ID_BYTES];
    if (kta_comm_unique_id(uid) != KTA_OK) {
        fprintf(stderr, "kta.gpus=%d: RCCL is not loadable (KTA_RCCL_LIBRARY)\n", job.nranks);
        return 2;
    }
    printf("Subscribing to %s\n", job.topic.c_str());                              // kafka.rs:88
    printf("Starting message consumption...\n");                                   // kafka.rs:91
    fflush(stdout);
    std::vector<kta::HipMetricHandler *> handlers(job.nranks, nullptr);
    std::vector<std::thread> threads;
    std::vector<int64_t> filter_counts(2 * (size_t)job.nranks, 0);
    for (int r = 0; r < job.nranks; r++) threads.emplace_back(run_rank, std::cref(job), r, uid, ndev, &handlers[r], &filter_counts[2 * (size_t)r]);
    for (auto &t : threads) t.join();
    if (g_rank_panicked) rust_panic(g_rank_panic_msg, g_rank_panic_loc);           // once, from the main thread
    fprintf(stderr, "done\n");                                                     // kafka.rs:136 (spinner)
    kta::HipMetricHandler *h0 = handlers[0];            // after the exchange every rank holds the whole job's result
    uint64_t undelivered = 0;
    for (auto *h : handlers) undelivered = std::max(undelivered, h->undelivered_records());
    if (!job.synthetic && undelivered)
        fprintf(stderr, "[WARN] Kafka error: %llu record(s) of corrupt batches were not delivered\n", (unsigned long long)undelivered);
    const kta::MessageMetrics &metrics = h0->metrics();
    if (job.synthetic)
        for (uint32_t p = 0; p < job.P; p++) job.end_offsets[p] = (int64_t)metrics.total((int32_t)p);
    std::vector<int32_t> partitions(job.P);
    for (uint32_t p = 0; p < job.P; p++) partitions[p] = (int32_t)p;
    const uint64_t duration_secs = (uint64_t)std::chrono::duration_cast<std::chrono::seconds>(
                                       std::chrono::steady_clock::now() - start_time).count();
    try {
        std::string text = kta::render_report(job.topic, duration_secs, metrics, h0->log_compaction(), partitions,
                                              job.start_offsets, job.end_offsets);
        if (job.analytics) text += kta::render_analytics(*h0->analytics());   // the exchanged snapshot, printed once
        if (job.percentiles) text += kta::render_size_percentiles(h0->size_quantiles()->data(), job.P);   // likewise
        if (job.timeline.n_buckets)
            text += kta::render_timeline(h0->timeline()->data(), job.timeline.origin_ms, job.timeline.bucket_ms,
                                         job.timeline.n_buckets);
        if (job.distinct_keys) text += kta::render_distinct_keys(h0->key_sketch()->data(), keyed_records(metrics, job.P));
        if (job.ts_order) text += kta::render_ts_order(h0->ts_order()->data(), total_records(metrics, job.P));
        if (job.hot_keys) {
            // a slot a lower rank filled stays: every reported hash gets its exemplar from the lowest rank that has it
            std::vector<kta_hot_exemplar> merged = *h0->hot_key_exemplars();
            for (size_t r = 1; r < handlers.size(); r++) {
                const std::vector<kta_hot_exemplar> &ex = *handlers[r]->hot_key_exemplars();
                std::vector<kta_hot_key> keys(job.hot_keys);
                uint32_t n = 0;
                if (kta_hot_keys_recover(h0->hot_keys()->data(), job.hot_keys, keys.data(), &n, nullptr) != KTA_OK) n = 0;
                for (uint32_t k = 0; k < n; k++) {
                    const uint32_t x = hot_fmix32(keys[k].hash);
                    const size_t at[2] = {x & 1023u, KTA_HOT_CELLS + ((x >> 10) & 1023u)};
                    const bool have = (merged[at[0]].valid && merged[at[0]].hash == keys[k].hash) ||
                                      (merged[at[1]].valid && merged[at[1]].hash == keys[k].hash);
                    for (size_t a : at)
                        if (!have && ex[a].valid && ex[a].hash == keys[k].hash) {
                            merged[a] = ex[a];
                            break;
                        }
                }
            }
            text += kta::render_hot_keys(h0->hot_keys()->data(), merged.data(), job.hot_keys);
        }
        if (job.partitioner)
            text += kta::render_partitioner(h0->partitioner()->data(), partitioner_counters(metrics, job.P).data(), job.P, h0->repartition());
        if (job.segments.on)
            text += kta::render_retention(h0->segments()->data(), job.P, job.segments.M, job.segments.now_ms, job.segments.retention_ms,
                                          job.segments.retention_bytes);
        if (job.filter.on)
            text += kta::render_filter(job.filter.from_ms, job.filter.to_ms, job.filter.has_set ? job.filter.bitmap.data() : nullptr, job.P,
                                       (uint64_t)filter_counts[0], (uint64_t)filter_counts[1]);
        if (job.record_batches) text += kta::render_record_batches(h0->record_batches()->data(), job.P, job.filter.on, job.rb_skipped);
        if (job.payload) text += kta::render_payload(h0->payload()->data(), partitioner_counters(metrics, job.P).data(), job.P);
        if (job.headers) {
            // a slot a lower rank published stays: every listed hash gets its name from the lowest rank that has it
            std::vector<kta_header_name> merged = *h0->header_name_table();
            size_t n = 0;
            if (kta_header_names_list(h0->header_names()->data(), nullptr, nullptr, 0, &n, nullptr, nullptr) != KTA_OK) n = 0;
            std::vector<kta_header_name_row> listed(n);
            if (n && kta_header_names_list(h0->header_names()->data(), nullptr, listed.data(), n, &n, nullptr, nullptr) != KTA_OK) n = 0;
            for (size_t r = 1; r < handlers.size(); r++) {
                const std::vector<kta_header_name> &tab = *handlers[r]->header_name_table();
                for (size_t k = 0; k < n; k++) {
                    const uint32_t h = listed[k].hash;
                    const size_t at[2] = {h & 1023u, KTA_HEADER_NAMES_CELLS + (hot_fmix32(h) & 1023u)};
                    const bool have = (merged[at[0]].state == KTA_HEADER_NAME_PUBLISHED && merged[at[0]].hash == h) ||
                                      (merged[at[1]].state == KTA_HEADER_NAME_PUBLISHED && merged[at[1]].hash == h);
                    for (size_t a : at)
                        if (!have && tab[a].state == KTA_HEADER_NAME_PUBLISHED && tab[a].hash == h) {
                            merged[a] = tab[a];
                            break;
                        }
                }
            }
            text += kta::render_header_names(h0->header_names()->data(), merged.data(), kHeaderNamesShown);
        }
        if (job.value_bytes) text += kta::render_value_bytes(h0->value_bytes()->data(), job.P);
        if (job.compress_whatif) text += kta::render_compress_whatif(h0->compress_whatif()->data(), job.P);
        fputs(text.c_str(), stdout);
    } catch (const kta::RustPanic &p) {
        rust_panic(p.what(), p.location);
    }
    for (auto *h : handlers) delete h;
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    Args args = parse_args(argc, argv);
    const auto start_time = std::chrono::steady_clock::now();                       // main.rs:69
    const bool count_alive = args.count_alive_occurrences == 1;                     // main.rs:77-80
    std::map<std::string, std::string> cfg = parse_librdkafka(args);                // main.rs:84-92
    const int device = cfg.count("kta.device") ? atoi(cfg["kta.device"].c_str()) : 0;
    const uint64_t batch = cfg.count("kta.batch") ? strtoull(cfg["kta.batch"].c_str(), nullptr, 10) : (1ull << 20);
    int gpus = 1;
    if (cfg.count("kta.gpus")) {   // strictly a positive decimal number
        const std::string &g = cfg["kta.gpus"];
        char *end = nullptr;
        const long v = strtol(g.c_str(), &end, 10);
        if (g.empty() || *end || v < 1 || v > 1024) {
            fprintf(stderr, "kta.gpus=%s: expected a number of GPUs >= 1\n", g.c_str());
            return 2;
        }
        gpus = (int)v;
    }
    const bool oversubscribe = cfg.count("kta.oversubscribe") && cfg["kta.oversubscribe"] == "1";

    // ---- the record source (stands in for TopicAnalyzer, src/kafka.rs) ------------------------------
    const std::string &b = args.bootstrap;
    bool synthetic = b.rfind("synthetic://", 0) == 0, dump = b.rfind("dump://", 0) == 0;
    const bool segment = b.rfind("segment://", 0) == 0;
    const bool kafka = !synthetic && !dump && !segment;   // a broker list: the reference's own path
    // kta.record_batches: the section is about batches, and only raw log segments have them
    bool record_batches = false;
    if (cfg.count("kta.record_batches")) {
        const std::string &v = cfg["kta.record_batches"];
        if (v != "0" && v != "1") {
            fprintf(stderr, "kta.record_batches=%s: expected 0 or 1\n", v.c_str());
            return 2;
        }
        record_batches = v == "1";
        if (record_batches && (!segment || (cfg.count("kta.per_message") && cfg["kta.per_message"] == "1"))) {   // before a broker or a device is asked for anything
            fprintf(stderr, "kta.record_batches=1: needs a segment:// source without kta.per_message=1 (synthetic://, dump://, a broker "
                            "list and kta.per_message=1 deliver records, not batches)\n");
            return 2;
        }
    }
    // kta.payload: the section is about the record bytes, and only raw log segments hold them on the device
    bool payload = false;
    if (cfg.count("kta.payload")) {
        const std::string &v = cfg["kta.payload"];
        if (v != "0" && v != "1") {
            fprintf(stderr, "kta.payload=%s: expected 0 or 1\n", v.c_str());
            return 2;
        }
        payload = v == "1";
        if (payload && (!segment || (cfg.count("kta.per_message") && cfg["kta.per_message"] == "1"))) {   // before a broker or a device is asked for anything
            fprintf(stderr, "kta.payload=1: needs a segment:// source without kta.per_message=1 (synthetic://, dump://, a broker "
                            "list and kta.per_message=1 deliver records, not the bytes of the log)\n");
            return 2;
        }
    }
    // kta.headers: likewise
    bool headers = false;
    if (cfg.count("kta.headers")) {
        const std::string &v = cfg["kta.headers"];
        if (v != "0" && v != "1") {
            fprintf(stderr, "kta.headers=%s: expected 0 or 1\n", v.c_str());
            return 2;
        }
        headers = v == "1";
        if (headers && (!segment || (cfg.count("kta.per_message") && cfg["kta.per_message"] == "1"))) {   // before a broker or a device is asked for anything
            fprintf(stderr, "kta.headers=1: needs a segment:// source without kta.per_message=1 (synthetic://, dump://, a broker "
                            "list and kta.per_message=1 deliver records, not the bytes of the log)\n");
            return 2;
        }
    }
    // kta.value_bytes: likewise
    bool value_bytes = false;
    if (cfg.count("kta.value_bytes")) {
        const std::string &v = cfg["kta.value_bytes"];
        if (v != "0" && v != "1") {
            fprintf(stderr, "kta.value_bytes=%s: expected 0 or 1\n", v.c_str());
            return 2;
        }
        value_bytes = v == "1";
        if (value_bytes && (!segment || (cfg.count("kta.per_message") && cfg["kta.per_message"] == "1"))) {   // before a broker or a device is asked for anything
            fprintf(stderr, "kta.value_bytes=1: needs a segment:// source without kta.per_message=1 (synthetic://, dump://, a broker "
                            "list and kta.per_message=1 deliver records, not the bytes of the log)\n");
            return 2;
        }
    }
    // kta.compress_whatif: likewise; the value names the codec asked about, and lz4 is the one there is a model of
    bool compress_whatif = false;
    if (cfg.count("kta.compress_whatif")) {
        const std::string &v = cfg["kta.compress_whatif"];
        if (v != "lz4") {
            fprintf(stderr, "kta.compress_whatif=%s: expected lz4 (the codec the what-if has a model of)\n", v.c_str());
            return 2;
        }
        compress_whatif = true;
        if (!segment || (cfg.count("kta.per_message") && cfg["kta.per_message"] == "1")) {   // before a broker or a device is asked for anything
            fprintf(stderr, "kta.compress_whatif=lz4: needs a segment:// source without kta.per_message=1 (synthetic://, dump://, a broker "
                            "list and kta.per_message=1 deliver records, not the bytes of the log)\n");
            return 2;
        }
    }
    // kta.compaction: what needs no partition count is refused here, before a broker or a device is asked for anything
    bool compaction = false;
    if (cfg.count("kta.compaction")) {
        const std::string &v = cfg["kta.compaction"];
        if (v != "0" && v != "1") {
            fprintf(stderr, "kta.compaction=%s: expected 0 or 1\n", v.c_str());
            return 2;
        }
        compaction = v == "1";
        if (compaction && !count_alive) {
            fprintf(stderr, "kta.compaction=1: needs -c (the pass reads the alive-key table)\n");
            return 2;
        }
        if (compaction && gpus > 1) {
            fprintf(stderr, "kta.compaction=1: not with kta.gpus=%d (after the exchange a rank holds only its hash range's entries)\n", gpus);
            return 2;
        }
        if (compaction && cfg.count("kta.per_message") && cfg["kta.per_message"] == "1") {
            fprintf(stderr, "kta.compaction=1: not with kta.per_message=1\n");
            return 2;
        }
        if (compaction && kafka) {
            fprintf(stderr, "kta.compaction=1: needs a synthetic://, segment:// or dump:// source (a broker's topic cannot be read a second time here)\n");
            return 2;
        }
    }
    // kta.compact_delete: the join of the two what-ifs needs both of them (and so inherits the compaction knob's refusals above)
    bool compact_delete = false;
    if (cfg.count("kta.compact_delete")) {
        const std::string &v = cfg["kta.compact_delete"];
        if (v != "0" && v != "1") {
            fprintf(stderr, "kta.compact_delete=%s: expected 0 or 1\n", v.c_str());
            return 2;
        }
        compact_delete = v == "1";
        if (compact_delete && !compaction) {
            fprintf(stderr, "kta.compact_delete=1: needs kta.compaction=1 (the survivors come from the compaction replay)\n");
            return 2;
        }
        if (compact_delete && !cfg.count("kta.segments")) {
            fprintf(stderr, "kta.compact_delete=1: needs kta.segments=<size> (the survivors are counted per model segment)\n");
            return 2;
        }
    }
    kta::TopicAnalyzer *topic_analyzer = nullptr;
    std::map<int32_t, int64_t> kafka_start, kafka_end;
    if (kafka) {
        try {
            topic_analyzer = kta::TopicAnalyzer::new_from_bootstrap_servers(b, cfg);      // main.rs:93
            topic_analyzer->get_topic_offsets(args.topic, &kafka_start, &kafka_end);      // main.rs:94-96
        } catch (const kta::RustPanic &p) {
            rust_panic(p.what(), p.location);
        }
    }
    std::vector<std::string> segment_files;
    if (segment) {
        std::string rest = b.substr(strlen("segment://"));
        size_t p0 = 0;
        while (true) {
            size_t c = rest.find(',', p0);
            segment_files.push_back(rest.substr(p0, c == std::string::npos ? std::string::npos : c - p0));
            if (c == std::string::npos) break;
            p0 = c + 1;
        }
    }
    kta_synth_spec spec{};
    uint64_t n_records = 0;
    kta::DumpHeader hdr;
    kta::DumpReader *reader = nullptr;
    if (synthetic) {
        std::string rest = b.substr(strlen("synthetic://"));
        std::string preset = rest.substr(0, rest.find('?'));
        if (kta_synth_preset(preset.c_str(), &spec, &n_records) != KTA_OK) {
            fprintf(stderr, "Error fetching metadata: unknown synthetic topic '%s'\n", preset.c_str());
            return 101;
        }
        size_t q = rest.find("records=");
        if (q != std::string::npos) n_records = strtoull(rest.c_str() + q + 8, nullptr, 10);
        hdr.n_partitions = spec.n_partitions;
        hdr.n_records = n_records;
    } else if (segment) {
        hdr.n_partitions = (uint32_t)segment_files.size();
        n_records = 1;  // unknown until decoded; non-zero so the emptiness test below looks at the files
    } else if (kafka) {
        hdr.n_partitions = kafka_end.empty() ? 0u : (uint32_t)(kafka_end.rbegin()->first + 1);   // ids are dense
    } else {
        reader = new kta::DumpReader(b.substr(strlen("dump://")));
        if (!reader->ok() || !reader->read_header(&hdr)) {
            fprintf(stderr, "Error fetching metadata: cannot read topic dump '%s'\n", b.c_str() + 7);
            return 101;
        }
    }
    const uint32_t P = hdr.n_partitions;
    const bool analytics = cfg.count("kta.analytics") && cfg["kta.analytics"] == "1";
    if (analytics && P > (uint32_t)kta_analytics_max_partitions()) {   // before any context, so before any kernel
        fprintf(stderr, "kta.analytics=1: the topic has %u partitions, the analytics scan admits at most %d "
                        "(its per-partition extrema live in LDS)\n", P, kta_analytics_max_partitions());
        return 2;
    }
    const bool distinct_keys = cfg.count("kta.distinct_keys") && cfg["kta.distinct_keys"] == "1";
    if (distinct_keys && P > KTA_SKETCH_MAX_PARTITIONS) {   // before any context, so before any kernel
        fprintf(stderr, "kta.distinct_keys=1: the topic has %u partitions, the key sketch admits at most %d "
                        "(4096 registers per partition)\n", P, KTA_SKETCH_MAX_PARTITIONS);
        return 2;
    }
    bool percentiles = false;
    if (cfg.count("kta.percentiles")) {
        const std::string &v = cfg["kta.percentiles"];
        if (v != "0" && v != "1") {
            fprintf(stderr, "kta.percentiles=%s: expected 0 or 1\n", v.c_str());
            return 2;
        }
        percentiles = v == "1";
        if (percentiles && P > (uint32_t)kta_size_quantiles_max_partitions()) {   // before any context, so before any kernel
            fprintf(stderr, "kta.percentiles=1: the topic has %u partitions, the size-percentile pass admits at most %d\n", P,
                    kta_size_quantiles_max_partitions());
            return 2;
        }
    }
    bool ts_order = false;
    if (cfg.count("kta.ts_order")) {
        const std::string &v = cfg["kta.ts_order"];
        if (v != "0" && v != "1") {
            fprintf(stderr, "kta.ts_order=%s: expected 0 or 1\n", v.c_str());
            return 2;
        }
        ts_order = v == "1";
        if (ts_order && P > (uint32_t)kta_ts_order_max_partitions()) {   // before any context, so before any kernel
            fprintf(stderr, "kta.ts_order=1: the topic has %u partitions, the timestamp-order pass admits at most %d\n", P,
                    kta_ts_order_max_partitions());
            return 2;
        }
    }
    bool partitioner = false;
    uint32_t repartition = 0;
    if (cfg.count("kta.partitioner")) {
        const std::string &v = cfg["kta.partitioner"];
        if (v != "murmur2") {
            fprintf(stderr, "kta.partitioner=%s: expected murmur2 (Kafka's default partitioner; the only hash there is so far)\n", v.c_str());
            return 2;
        }
        partitioner = true;
        if (P > (uint32_t)kta_partitioner_max_partitions()) {   // before any context, so before any kernel
            fprintf(stderr, "kta.partitioner=murmur2: the topic has %u partitions, the partitioner pass admits at most %d\n", P,
                    kta_partitioner_max_partitions());
            return 2;
        }
    }
    if (compaction && P > (uint32_t)kta_compaction_max_partitions()) {   // before any context, so before any kernel
        fprintf(stderr, "kta.compaction=1: the topic has %u partitions, the compaction pass admits at most %d\n", P, kta_compaction_max_partitions());
        return 2;
    }
    if (cfg.count("kta.repartition")) {
        if (!partitioner) {
            fprintf(stderr, "kta.repartition=%s: needs kta.partitioner=murmur2\n", cfg["kta.repartition"].c_str());
            return 2;
        }
        const int64_t q = parse_decimal(cfg["kta.repartition"], 9);
        if (q < 1 || q > kta_partitioner_max_partitions()) {
            fprintf(stderr, "kta.repartition=%s: expected a partition count, 1 to %d\n", cfg["kta.repartition"].c_str(),
                    kta_partitioner_max_partitions());
            return 2;
        }
        repartition = (uint32_t)q;
    }
    uint32_t hot_keys = 0;
    if (cfg.count("kta.hot_keys")) {
        const int64_t k = parse_decimal(cfg["kta.hot_keys"], 3);
        if (k < 1 || k > KTA_HOT_MAX_REPORTED) {
            fprintf(stderr, "kta.hot_keys=%s: expected the number of keys to report, 1 to %d\n", cfg["kta.hot_keys"].c_str(),
                    KTA_HOT_MAX_REPORTED);
            return 2;
        }
        hot_keys = (uint32_t)k;
    }
    kta::TimelineConfig timeline;   // kta.timeline=<width>: refused here, before any context, when it cannot be had
    if (cfg.count("kta.timeline")) {
        const std::string &wv = cfg["kta.timeline"];
        const int64_t width = parse_timeline_width(wv);
        if (width == 0) {
            fprintf(stderr, "kta.timeline=%s: expected a bucket width such as 30s, 15m, 1h or 1d (a bare number is seconds)\n",
                    wv.c_str());
            return 2;
        }
        int64_t n = 168;
        if (cfg.count("kta.timeline.buckets")) {
            n = parse_decimal(cfg["kta.timeline.buckets"], 5);
            if (n < 1 || n > KTA_TIMELINE_MAX_BUCKETS) {
                fprintf(stderr, "kta.timeline.buckets=%s: expected a bucket count in [1, %d]\n",
                        cfg["kta.timeline.buckets"].c_str(), KTA_TIMELINE_MAX_BUCKETS);
                return 2;
            }
        }
        int64_t origin = 0;
        if (cfg.count("kta.timeline.start")) {
            const int64_t sec = parse_decimal(cfg["kta.timeline.start"], 15);
            if (sec < 0) {
                fprintf(stderr, "kta.timeline.start=%s: expected unix seconds >= 0\n", cfg["kta.timeline.start"].c_str());
                return 2;
            }
            origin = sec * 1000;
        } else {   // the last bucket holds the run's start time
            const int64_t now_ms = (int64_t)std::chrono::duration_cast<std::chrono::milliseconds>(
                                       std::chrono::system_clock::now().time_since_epoch()).count();
            origin = std::max<int64_t>(0, (now_ms / width - (n - 1)) * width);
        }
        if (width > (INT64_MAX - origin) / n) {
            fprintf(stderr, "kta.timeline=%s: %lld buckets from %lld ms overflow the int64 millisecond range\n", wv.c_str(),
                    (long long)n, (long long)origin);
            return 2;
        }
        const int pmax = kta_timeline_max_partitions(analytics ? KTA_FLAG_ANALYTICS : 0u, (uint32_t)n);
        if (P > (uint32_t)pmax) {
            fprintf(stderr, "kta.timeline=%s: the topic has %u partitions, the scan with %lld timeline buckets%s admits at "
                            "most %d (its rows live in LDS)\n", wv.c_str(), P, (long long)n,
                    analytics ? " and the analytics" : "", pmax);
            return 2;
        }
        timeline = kta::TimelineConfig{origin, width, (uint32_t)n};
    }

    SegmentsConfig segments;   // kta.segments=<size> and the policy: refused here, before any context, when they cannot be had
    for (const char *key : {"kta.retention.ms", "kta.retention.bytes", "kta.retention.now", "kta.segments.rows", "kta.segments.overhead"})
        if (cfg.count(key) && !cfg.count("kta.segments")) {
            fprintf(stderr, "%s=%s: needs kta.segments=<size> (the what-if is read off the model's segments)\n", key, cfg[key].c_str());
            return 2;
        }
    if (cfg.count("kta.segments")) {
        const int64_t size = parse_size(cfg["kta.segments"]);
        if (size < 1 || size > (1ll << 40)) {
            fprintf(stderr, "kta.segments=%s: expected a segment size of 1 byte to 1024g, such as 1g, 512m, 64k or a number of bytes\n",
                    cfg["kta.segments"].c_str());
            return 2;
        }
        if (P > (uint32_t)kta_segments_max_partitions()) {
            fprintf(stderr, "kta.segments=%s: the topic has %u partitions, the segment pass admits at most %d\n", cfg["kta.segments"].c_str(), P,
                    kta_segments_max_partitions());
            return 2;
        }
        int64_t rows = std::min<int64_t>(1024, (1ll << 20) / (int64_t)P);
        if (cfg.count("kta.segments.rows")) {
            rows = parse_decimal(cfg["kta.segments.rows"], 7);
            if (rows < 2 || rows * (int64_t)P > (1ll << 20)) {
                fprintf(stderr, "kta.segments.rows=%s: expected the rows kept per partition, 2 to %lld for %u partitions\n",
                        cfg["kta.segments.rows"].c_str(), (long long)((1ll << 20) / (int64_t)P), P);
                return 2;
            }
        }
        int64_t overhead = 0;
        if (cfg.count("kta.segments.overhead")) {
            overhead = parse_decimal(cfg["kta.segments.overhead"], 10);
            if (overhead < 0 || overhead > (int64_t)UINT32_MAX) {
                fprintf(stderr, "kta.segments.overhead=%s: expected a number of bytes below 2^32\n", cfg["kta.segments.overhead"].c_str());
                return 2;
            }
        }
        segments.on = true;
        segments.S = (uint64_t)size, segments.M = (uint32_t)rows, segments.overhead = (uint32_t)overhead;
        if (cfg.count("kta.retention.ms")) {
            segments.retention_ms = parse_timeline_width(cfg["kta.retention.ms"]);
            if (segments.retention_ms == 0) {
                fprintf(stderr, "kta.retention.ms=%s: expected a duration such as 30s, 15m, 1h or 7d (a bare number is seconds)\n",
                        cfg["kta.retention.ms"].c_str());
                return 2;
            }
        }
        if (cfg.count("kta.retention.bytes")) {
            segments.retention_bytes = parse_size(cfg["kta.retention.bytes"]);
            if (segments.retention_bytes < 0) {
                fprintf(stderr, "kta.retention.bytes=%s: expected a size such as 10g, 512m, 64k or a number of bytes\n",
                        cfg["kta.retention.bytes"].c_str());
                return 2;
            }
        }
        if (cfg.count("kta.retention.now")) {
            const int64_t sec = parse_decimal(cfg["kta.retention.now"], 15);
            if (sec < 0) {
                fprintf(stderr, "kta.retention.now=%s: expected unix seconds >= 0\n", cfg["kta.retention.now"].c_str());
                return 2;
            }
            segments.now_ms = sec * 1000;
        } else {   // the run's start time, as the timeline takes it
            segments.now_ms = (int64_t)std::chrono::duration_cast<std::chrono::milliseconds>(
                                  std::chrono::system_clock::now().time_since_epoch()).count();
        }
    }

    FilterConfig filter;   // kta.from / kta.to / kta.partitions: refused here, before any context, when malformed
    for (const char *key : {"kta.from", "kta.to"}) {
        if (!cfg.count(key)) continue;
        const int64_t sec = parse_decimal(cfg[key], 15);
        if (sec < 0) {
            fprintf(stderr, "%s=%s: expected unix seconds >= 0\n", key, cfg[key].c_str());
            return 2;
        }
        (key[4] == 'f' ? filter.from_ms : filter.to_ms) = sec * 1000;
        filter.on = true;
    }
    if (filter.from_ms >= filter.to_ms) {
        fprintf(stderr, "kta.from=%s,kta.to=%s: expected kta.from below kta.to\n", cfg["kta.from"].c_str(), cfg["kta.to"].c_str());
        return 2;
    }
    if (cfg.count("kta.partitions")) {
        if (!parse_partitions(cfg["kta.partitions"], P, &filter.bitmap)) {
            fprintf(stderr, "kta.partitions=%s: expected partitions and ranges of the topic's %u, such as 0,3-5\n", cfg["kta.partitions"].c_str(), P);
            return 2;
        }
        filter.on = filter.has_set = true;
    }

    // librdkafka options are forwarded as in the reference (kafka.rs:38-42); the one this build can
    // honour for raw segments is check.crcs (default false): verify every batch's CRC-32C on the GPU
    const bool check_crcs = cfg.count("check.crcs") && cfg["check.crcs"] == "true";
    if (gpus > 1 && !synthetic && !segment) {
        fprintf(stderr, "kta.gpus=%d needs a synthetic:// or segment:// source\n", gpus);
        return 2;
    }
    std::vector<int64_t> start_offsets(P, 0), end_offsets(P, 0);
    if (dump) { start_offsets = hdr.start_offsets; end_offsets = hdr.end_offsets; }
    if (kafka)
        for (const auto &kv : kafka_end) {
            start_offsets[(size_t)kv.first] = kafka_start[kv.first];
            end_offsets[(size_t)kv.first] = kv.second;
        }
    std::vector<std::vector<uint8_t>> segment_bytes;
    std::vector<uint64_t> segment_base_seq;   // records of the partitions before each one (consumption order: file by file)
    uint64_t segment_records = 0;
    uint64_t rb_skipped[3] = {0, 0, 0};       // kta.record_batches=1: what the host index counts and the section cannot
    if (segment) {  // watermarks = first / last offset found in each partition's segment (kafka.rs:60-72)
        for (uint32_t p = 0; p < P; p++) {
            std::vector<uint8_t> bytes;
            FILE *f = fopen(segment_files[p].c_str(), "rb");
            if (!f) {
                fprintf(stderr, "Error fetching metadata: cannot read log segment '%s'\n", segment_files[p].c_str());
                return 101;
            }
            fseek(f, 0, SEEK_END);
            long sz = ftell(f);
            fseek(f, 0, SEEK_SET);
            bytes.resize((size_t)sz + 64, 0);
            if (sz > 0 && fread(bytes.data(), 1, (size_t)sz, f) != (size_t)sz) { fclose(f); return 101; }
            fclose(f);
            bytes.resize((size_t)sz);
            kta_kafka_index_stats ist;
            std::vector<kta_kafka_batch_desc> descs(1);
            int rc = kta_kafka_index_host(bytes.data(), bytes.size(), (int32_t)p, 0, 0, 0, descs.data(), descs.size(), &ist);
            if (rc == KTA_ERR_CAPACITY) {
                descs.resize(ist.n_batches);
                rc = kta_kafka_index_host(bytes.data(), bytes.size(), (int32_t)p, 0, 0, 0, descs.data(), descs.size(), &ist);
            }
            if (rc == KTA_OK && ist.any_offsets) {   // what the broker would answer: log start / log end offset,
                start_offsets[p] = ist.first_offset;  // control batches and compacted-away offsets included
                end_offsets[p] = ist.next_offset;
            }
            segment_base_seq.push_back(segment_records);
            if (rc == KTA_OK) segment_records += ist.n_records;
            if (rc == KTA_OK) rb_skipped[0] += ist.n_control_batches, rb_skipped[1] += ist.n_old_magic, rb_skipped[2] += ist.n_compressed;
            segment_bytes.push_back(std::move(bytes));
        }
    }
    else if (synthetic && n_records > 0) {
        // offsets of a synthetic topic: 0 .. per-partition record count; known only after the scan,
        // so the emptiness test of main.rs:98-101 uses the record count
        std::fill(end_offsets.begin(), end_offsets.end(), 1);
    }
    if (std::all_of(end_offsets.begin(), end_offsets.end(), [](int64_t v) { return v == 0; })) {  // main.rs:98-101
        fprintf(stderr, "[ERROR] Given topic has no content, no analysis possible. Exiting.\n");
        return 254;  // exit(-2)
    }
    std::vector<int32_t> partitions(P);                                             // main.rs:103-106
    for (uint32_t p = 0; p < P; p++) partitions[p] = (int32_t)p;

    if (gpus > 1) {   // kta.gpus=N: partition p on rank p % N, one exchange step before the report
        ShardedJob job;
        job.topic = args.topic;
        job.count_alive = count_alive;
        job.synthetic = synthetic;
        job.check_crcs = check_crcs;
        job.device = device;
        job.nranks = gpus;
        job.oversubscribe = oversubscribe;
        job.analytics = analytics;
        job.timeline = timeline;
        job.distinct_keys = distinct_keys;
        job.hot_keys = hot_keys;
        job.ts_order = ts_order;
        job.partitioner = partitioner;
        job.repartition = repartition;
        job.percentiles = percentiles;
        job.record_batches = record_batches;
        job.payload = payload;
        job.headers = headers;
        job.value_bytes = value_bytes;
        job.compress_whatif = compress_whatif;
        std::copy(rb_skipped, rb_skipped + 3, job.rb_skipped);
        job.filter = filter;
        job.segments = segments;
        job.batch = batch;
        job.P = P;
        job.spec = spec;
        job.n_records = n_records;
        job.segment_bytes = std::move(segment_bytes);
        job.base_seq = segment_base_seq;
        job.start_offsets = start_offsets;
        job.end_offsets = end_offsets;
        return run_sharded(job, start_time);
    }
    // the handlers are created only now: MessageMetrics::new / LogCompactionInMemoryMetrics::new come after the
    // "no content" exit in the reference as well (main.rs:77-82 build them, but nothing is allocated there; here
    // -c means a 32 GiB table)
    kta::HipMetricHandler *handler = nullptr;
    try {
        handler = new kta::HipMetricHandler((int32_t)P, count_alive, device, batch, 0,
                                            (analytics ? KTA_FLAG_ANALYTICS : 0u) | (distinct_keys ? KTA_FLAG_KEY_SKETCH : 0u) |
                                                (hot_keys ? KTA_FLAG_HOT_KEYS : 0u) | (ts_order ? KTA_FLAG_TS_ORDER : 0u) |
                                                (partitioner ? KTA_FLAG_PARTITIONER : 0u) | (compaction ? KTA_FLAG_COMPACTION : 0u) |
                                                (percentiles ? KTA_FLAG_SIZE_QUANTILES : 0u) | (record_batches ? KTA_FLAG_RECORD_BATCHES : 0u) |
                                                (payload ? KTA_FLAG_PAYLOAD : 0u) | (headers ? KTA_FLAG_HEADER_NAMES : 0u) |
                                                (value_bytes ? KTA_FLAG_VALUE_BYTES : 0u) | (compress_whatif ? KTA_FLAG_COMPRESS_WHATIF : 0u),
                                            timeline, repartition);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 2;
    }
    kta_ctx *ctx = handler->ctx();
    try {
        if (segments.on) handler->set_segments(segments.S, segments.M, segments.overhead);
        if (compact_delete) handler->set_compact_delete(true);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 2;
    }
    apply_filter(ctx, filter);
    if (segment) check(kta_kafka_set_check_crcs(ctx, check_crcs ? 1 : 0), ctx, "kta_kafka_set_check_crcs");

    if (!kafka) {
        printf("Subscribing to %s\n", args.topic.c_str());                          // kafka.rs:88
        printf("Starting message consumption...\n");                                // kafka.rs:91
        fflush(stdout);
    }

    kta::DumpWriter *writer = nullptr;
    std::vector<kta::DumpBatch> to_write;
    const bool write_dump = cfg.count("kta.write_dump") != 0;

    uint64_t seq = 0;
    const bool per_message = cfg.count("kta.per_message") && cfg["kta.per_message"] == "1";
    if (kafka) {
        // the reference's loop: every polled message goes to every handler (kafka.rs:92-135); the handler
        // stages it into pinned columns and the device accumulates batch by batch
        topic_analyzer->add_metric_handler(handler);                               // main.rs:108-115
        try {
            seq = topic_analyzer->read_topic_into_metrics(args.topic, kafka_end);  // main.rs:117
        } catch (const kta::RustPanic &p) {
            rust_panic(p.what(), p.location);
        } catch (const std::exception &e) {
            fprintf(stderr, "%s\n", e.what());
            return 2;
        }
        delete topic_analyzer;                                                     // end of the block, main.rs:118
        topic_analyzer = nullptr;
    } else if (synthetic && per_message) {
        // the reference's shape: for every polled message, every handler's handle_message (kafka.rs:107-109)
        std::vector<kta::MetricHandler *> metric_handlers{handler};
        std::vector<uint8_t> key;
        for (; seq < n_records; seq++) {
            kta::Message m;
            int32_t p, kl, vl;
            int64_t ts;
            kta_synth_record(&spec, seq, &p, &kl, &vl, &ts);
            m.partition = p;
            m.offset = (int64_t)seq;
            m.timestamp_ms = ts;
            m.payload_len = vl;
            if (kl >= 0) {
                key.resize((size_t)kl + 1);
                const uint64_t kid = (uint64_t)kta_synth_key_id(&spec, seq);
                for (int32_t j = 0; j < kl; j++) key[(size_t)j] = kta_synth_key_byte(&spec, kid, (uint32_t)j);
                m.key = key.data();   // non-null even for an empty key: Some(&[])
                m.key_len = kl;
            }
            try {
                for (auto *mh : metric_handlers) mh->handle_message(m);
            } catch (const kta::RustPanic &p) {
                rust_panic(p.what(), p.location);
            } catch (const std::exception &e) {
                fprintf(stderr, "%s\n", e.what());
                return 2;
            }
        }
    }
    // The synthetic://, segment:// and dump:// feed loops: once for the first pass, and with kta.compaction=1 a second time
    // in replay mode, with the sequence numbers of the first.  Returns an exit code, 0 to go on.
    auto feed = [&](bool replay) -> int {
        seq = 0;
        if (replay && reader) {   // the dump from its first batch again
            delete reader;
            reader = new kta::DumpReader(b.substr(strlen("dump://")));
            kta::DumpHeader again;
            if (!reader->ok() || !reader->read_header(&again)) {
                fprintf(stderr, "kta.compaction=1: cannot read topic dump '%s' a second time\n", b.c_str() + 7);
                return 2;
            }
        }
        if (synthetic) {
            while (seq < n_records) {
                kta_batch hb;
                check(kta_batch_acquire(ctx, &hb), ctx, "kta_batch_acquire");
                uint64_t n = std::min<uint64_t>(hb.capacity, n_records - seq), kb = 0;
                if (!count_alive && !distinct_keys && !hot_keys && !partitioner && !write_dump) { hb.key_off = nullptr; hb.key_bytes = nullptr; }
                int rc = kta_synth_fill_host(&spec, seq, n, &hb, &kb);
                while (rc == KTA_ERR_CAPACITY && n > 1) {  // key bytes did not fit: shrink the batch
                    n /= 2;
                    rc = kta_synth_fill_host(&spec, seq, n, &hb, &kb);
                }
                check(rc, ctx, "kta_synth_fill_host");
                if (write_dump && !replay) {
                    kta::DumpBatch db;
                    db.n = n; db.n_key_bytes = hb.key_bytes ? kb : 0;
                    db.partition.assign(hb.partition, hb.partition + n);
                    db.key_len.assign(hb.key_len, hb.key_len + n);
                    db.val_len.assign(hb.val_len, hb.val_len + n);
                    db.ts_ms.assign(hb.ts_ms, hb.ts_ms + n);
                    if (hb.key_off) db.key_off.assign(hb.key_off, hb.key_off + n); else db.key_off.assign(n, 0);
                    if (hb.key_bytes) db.key_bytes.assign(hb.key_bytes, hb.key_bytes + kb);
                    to_write.push_back(std::move(db));
                }
                check(kta_batch_submit(ctx, n, kb, seq), ctx, "kta_batch_submit");
                seq += n;
            }
        } else if (segment) {
            for (uint32_t p = 0; p < P; p++) {
                if (segment_bytes[p].empty()) continue;
                kta_kafka_index_stats ist;
                check(kta_kafka_consume(ctx, segment_bytes[p].data(), segment_bytes[p].size(), (int32_t)p, &ist), ctx,
                      "kta_kafka_consume");
                if (!replay && (ist.n_compressed || ist.n_old_magic))
                    fprintf(stderr, "[WARN] Kafka error: partition %u: %llu unknown-codec and %llu pre-v2 batches skipped\n", p,
                            (unsigned long long)ist.n_compressed, (unsigned long long)ist.n_old_magic);   // kafka.rs:95-97
                seq += ist.n_records;
            }
        } else {
            kta::DumpBatch db;
            for (uint64_t bi = 0; bi < hdr.n_batches; bi++) {
                if (!reader->read_batch(&db)) {
                    if (!replay) fprintf(stderr, "[WARN] Kafka error: truncated topic dump\n");      // kafka.rs:95-97: warn and go on
                    break;
                }
                uint64_t done = 0;
                while (done < db.n) {
                    kta_batch hb;
                    check(kta_batch_acquire(ctx, &hb), ctx, "kta_batch_acquire");
                    uint64_t n = std::min<uint64_t>(hb.capacity, db.n - done), kb = 0;
                    if (count_alive || distinct_keys || hot_keys || partitioner) {  // re-pack this chunk's keys
                        uint64_t m = 0;
                        for (; m < n; m++) {
                            const uint64_t kl = db.key_len[done + m] > 0 ? (uint64_t)db.key_len[done + m] : 0;
                            if (kb + kl > hb.key_bytes_capacity) break;
                            hb.key_off[m] = (uint32_t)kb;
                            if (kl) memcpy(hb.key_bytes + kb, db.key_bytes.data() + db.key_off[done + m], kl);
                            kb += kl;
                        }
                        n = m;
                        if (n == 0) { fprintf(stderr, "key larger than the staging capacity\n"); return 2; }
                    }
                    memcpy(hb.partition, db.partition.data() + done, 4 * n);
                    memcpy(hb.key_len, db.key_len.data() + done, 4 * n);
                    memcpy(hb.val_len, db.val_len.data() + done, 4 * n);
                    memcpy(hb.ts_ms, db.ts_ms.data() + done, 8 * n);
                    check(kta_batch_submit(ctx, n, kb, seq), ctx, "kta_batch_submit");
                    seq += n;
                    done += n;
                }
            }
        }
        return 0;
    };
    if (!kafka && !(synthetic && per_message)) {
        const int rc = feed(false);
        if (rc) return rc;
    }
    if (!kafka) fprintf(stderr, "done\n");                                          // kafka.rs:136 (spinner)

    try {
        handler->finish(segment);                // where main.rs:121 is: the trait has no end-of-stream hook
    } catch (const kta::RustPanic &p) {          // a timestamp outside chrono's range: the reference died on that record
        rust_panic(p.what(), p.location);
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 2;
    }
    if (segment && handler->undelivered_records()) {                               // kafka.rs:95-97: warn, go on
        uint64_t crc_errors = 0;
        (void)kta_kafka_crc_errors(ctx, &crc_errors);
        fprintf(stderr, "[WARN] Kafka error: %llu record(s) of corrupt batches were not delivered (%llu CRC failure(s))\n",
                (unsigned long long)handler->undelivered_records(), (unsigned long long)crc_errors);
    }
    // kta.compaction=1: whatever the report prints from the first pass has been read (the snapshot finish() took, the CRC
    // errors, the undelivered records; the filter's counts are read here) before the replay starts
    uint64_t filter_info[6] = {0, 0, 0, 0, 0, 0};
    if (filter.on) check(kta_filter_info(ctx, filter_info), ctx, "kta_filter_info");
    std::vector<uint64_t> compaction_vec, kept_vec;
    if (compaction) {
        try {
            handler->replay_compaction(true);
            const int rc = feed(true);
            if (rc) return rc;
            handler->replay_compaction(false);
            compaction_vec = handler->compaction();
            if (compact_delete) kept_vec = handler->compact_delete();
        } catch (const std::exception &e) {
            fprintf(stderr, "%s\n", e.what());
            return 2;
        }
    }
    const kta::MessageMetrics &metrics = handler->metrics();
    if (synthetic)
        for (uint32_t p = 0; p < P; p++) end_offsets[p] = (int64_t)metrics.total((int32_t)p);
    if (write_dump) {
        writer = new kta::DumpWriter(cfg["kta.write_dump"]);
        kta::DumpHeader wh = hdr;
        wh.n_batches = to_write.size();
        wh.start_offsets = start_offsets;
        wh.end_offsets = end_offsets;
        bool ok = writer->ok() && writer->write_header(wh);
        for (auto &db : to_write)
            ok = ok && writer->write_batch(db.n, db.n_key_bytes, db.partition.data(), db.key_len.data(),
                                           db.val_len.data(), db.ts_ms.data(), db.key_off.data(), db.key_bytes.data());
        delete writer;
        if (!ok) fprintf(stderr, "[WARN] could not write topic dump %s\n", cfg["kta.write_dump"].c_str());
    }

    const uint64_t duration_secs = (uint64_t)std::chrono::duration_cast<std::chrono::seconds>(
                                       std::chrono::steady_clock::now() - start_time).count();  // main.rs:121
    try {
        std::string text = kta::render_report(args.topic, duration_secs, metrics, handler->log_compaction(),
                                              partitions, start_offsets, end_offsets);
        if (analytics) text += kta::render_analytics(*handler->analytics());
        if (percentiles) text += kta::render_size_percentiles(handler->size_quantiles()->data(), P);
        if (timeline.n_buckets)
            text += kta::render_timeline(handler->timeline()->data(), timeline.origin_ms, timeline.bucket_ms, timeline.n_buckets);
        if (distinct_keys) text += kta::render_distinct_keys(handler->key_sketch()->data(), keyed_records(metrics, P));
        if (ts_order) text += kta::render_ts_order(handler->ts_order()->data(), total_records(metrics, P));
        if (hot_keys) text += kta::render_hot_keys(handler->hot_keys()->data(), handler->hot_key_exemplars()->data(), hot_keys);
        if (partitioner)
            text += kta::render_partitioner(handler->partitioner()->data(), partitioner_counters(metrics, P).data(), P, handler->repartition());
        if (compaction) {
            std::vector<uint64_t> cv = partitioner_counters(metrics, P);
            uint64_t records = 0;
            for (uint32_t p = 0; p < P; p++) {
                cv[(size_t)p * KTA_NCOUNTERS + KTA_C_TOTAL] = metrics.total((int32_t)p);
                records += metrics.total((int32_t)p);
            }
            cv[(size_t)P * KTA_NCOUNTERS + KTA_G_RECORDS] = records;
            cv[(size_t)P * KTA_NCOUNTERS + KTA_G_BAD_PARTITION] = handler->undelivered_records();
            text += kta::render_compaction(compaction_vec.data(), cv.data(), P);
        }
        if (segments.on)
            text += kta::render_retention(handler->segments()->data(), P, segments.M, segments.now_ms, segments.retention_ms,
                                          segments.retention_bytes);
        if (compact_delete)
            text += kta::render_compact_delete(handler->segments()->data(), kept_vec.data(), compaction_vec.data(), P, segments.M, segments.now_ms,
                                               segments.retention_ms, segments.retention_bytes);
        if (filter.on)
            text += kta::render_filter(filter.from_ms, filter.to_ms, filter.has_set ? filter.bitmap.data() : nullptr, P, filter_info[0],
                                       filter_info[1]);
        if (record_batches) text += kta::render_record_batches(handler->record_batches()->data(), P, filter.on, rb_skipped);
        if (payload) text += kta::render_payload(handler->payload()->data(), partitioner_counters(metrics, P).data(), P);
        if (headers) text += kta::render_header_names(handler->header_names()->data(), handler->header_name_table()->data(), kHeaderNamesShown);
        if (value_bytes) text += kta::render_value_bytes(handler->value_bytes()->data(), P);
        if (compress_whatif) text += kta::render_compress_whatif(handler->compress_whatif()->data(), P);
        fputs(text.c_str(), stdout);
    } catch (const kta::RustPanic &p) {
        rust_panic(p.what(), p.location);
    }
    delete handler;
    delete reader;
    return 0;
}

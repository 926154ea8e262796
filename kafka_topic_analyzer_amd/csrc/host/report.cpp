// report.cpp — the report the reference prints after the scan (src/main.rs:123-178), byte for
// byte: fixed text block, chrono `DateTime<Utc>` Display, Rust `{:.4}` of an f32 and the
// prettytable-rs 0.8 default table format.  Also exported through the C ABI (kta_render_report)
// so that it can be tested without a GPU.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "kta_compact_delete.h"
#include "kta_compaction.h"
#include "kta_header_names.h"
#include "kta_payload.h"
#include "kta_record_batches.h"
#include "kta_segments.h"
#include "kta_value_bytes.h"
#include "kta_lz4_model.h"
#include "kta_size_bins.h"
#include "metric.hpp"

namespace kta {

static void days_to_civil(int64_t z, int64_t *y, unsigned *m, unsigned *d)
{
    z += 719468;
    const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
    const unsigned doe = (unsigned)(z - era * 146097);
    const unsigned yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
    const int64_t yy = (int64_t)yoe + era * 400;
    const unsigned doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
    const unsigned mp = (5 * doy + 2) / 153;
    *d = doy - (153 * mp + 2) / 5 + 1;
    *m = mp < 10 ? mp + 3 : mp - 9;
    *y = yy + (*m <= 2);
}

// chrono 0.4.19: `impl Display for DateTime<Tz>` writes "{naive_local} {offset}"; NaiveDate prints
// {:04}-{:02}-{:02} for years 0..=9999 (else {:+05}), NaiveTime prints {:02}:{:02}:{:02} followed by
// .{:03} / .{:06} / .{:09} when the nanosecond part is non-zero; Utc prints "UTC".
std::string format_datetime_utc(int64_t sec, uint32_t ns)
{
    int64_t days = sec / 86400, rem = sec % 86400;
    if (rem < 0) { rem += 86400; days -= 1; }
    int64_t y; unsigned mo, d;
    days_to_civil(days, &y, &mo, &d);
    char buf[96];
    int n;
    if (y >= 0 && y <= 9999) n = snprintf(buf, sizeof buf, "%04lld", (long long)y);
    else n = snprintf(buf, sizeof buf, "%+05lld", (long long)y);
    n += snprintf(buf + n, sizeof buf - n, "-%02u-%02u %02lld:%02lld:%02lld", mo, d, (long long)(rem / 3600),
                  (long long)((rem % 3600) / 60), (long long)(rem % 60));
    if (ns != 0) {
        if (ns % 1000000 == 0) n += snprintf(buf + n, sizeof buf - n, ".%03u", ns / 1000000);
        else if (ns % 1000 == 0) n += snprintf(buf + n, sizeof buf - n, ".%06u", ns / 1000);
        else n += snprintf(buf + n, sizeof buf - n, ".%09u", ns);
    }
    snprintf(buf + n, sizeof buf - n, " UTC");
    return buf;
}

// Rust formats the exact decimal expansion of the f32 rounded to 4 places; printf("%.4f") of the
// float promoted to double prints the same digits (the promotion is exact, glibc rounds the exact
// value half-to-even).
std::string format_f32_4(float x)
{
    char buf[64];
    snprintf(buf, sizeof buf, "%.4f", (double)x);
    return buf;
}

// prettytable-rs 0.8.0, FORMAT_DEFAULT (what Table::new() + printstd() use): a `+---+` line above
// the first row and below every row, `|` column separators and borders, one space of padding on
// both sides, cells left-aligned.
static std::string pretty_table(const std::vector<std::vector<std::string>> &rows)
{
    size_t ncol = 0;
    for (auto &r : rows) ncol = std::max(ncol, r.size());
    std::vector<size_t> w(ncol, 0);
    for (auto &r : rows)
        for (size_t i = 0; i < r.size(); i++) w[i] = std::max(w[i], r[i].size());
    std::string sep = "+";
    for (size_t i = 0; i < ncol; i++) sep += std::string(w[i] + 2, '-') + "+";
    sep += "\n";
    std::string out = sep;
    for (auto &r : rows) {
        out += "|";
        for (size_t i = 0; i < ncol; i++) {
            const std::string &c = i < r.size() ? r[i] : std::string();
            out += " " + c + std::string(w[i] - c.size(), ' ') + " |";
        }
        out += "\n" + sep;
    }
    return out;
}

std::string render_report(const std::string &topic, uint64_t duration_secs, const MessageMetrics &m,
                          const LogCompactionInMemoryMetrics *lc, const std::vector<int32_t> &partitions,
                          const std::vector<int64_t> &start_offsets, const std::vector<int64_t> &end_offsets)
{
    auto u = [](uint64_t v) { return std::to_string(v); };
    const std::string eq(120, '='), dash(120, '-');
    std::string o;
    o += "\n";                                                                     // main.rs:125
    o += eq + "\n";                                                                // :126
    o += "Calculating statistics...\n";                                            // :127
    o += "Topic " + topic + "\n";                                                  // :128
    o += "Scanning took: " + u(duration_secs) + " seconds\n";                      // :129
    o += "Estimated Msg/s: " + u(m.overall_count() / std::max<uint64_t>(duration_secs, 1)) + "\n";  // :130
    o += dash + "\n";                                                              // :131
    o += "Earliest Message: " + format_datetime_utc(m.earliest_message().sec, m.earliest_message().ns) + "\n";
    o += "Latest Message: " + format_datetime_utc(m.latest_message().sec, m.latest_message().ns) + "\n";
    o += dash + "\n";                                                              // :134
    o += "Largest Message: " + u(m.largest_message()) + " bytes\n";                // :135
    o += "Smallest Message: " + u(m.smallest_message()) + " bytes\n";              // :136
    o += "Topic Size: " + u(m.overall_size()) + " bytes\n";                        // :137
    if (lc) {                                                                      // :139-146
        o += dash + "\n";
        o += "Alive keys: " + u(lc->sum_all_alive()) + "\n";
        o += dash + "\n";
    }
    o += eq + "\n";                                                                // :148
    std::vector<std::vector<std::string>> rows;
    rows.push_back({"P", "< OS", "> OS", "Total", "Alive", "Tmb", "DR", "K Null", "K !Null", "P-Bytes", "K-Bytes",
                    "V-Bytes", "A K-Sz", "A V-Sz", "A M-Sz"});                     // :150
    for (size_t i = 0; i < partitions.size(); i++) {                               // :153-172
        const int32_t p = partitions[i];
        const uint64_t key_size_avg = m.key_size_avg(p);  // first, as in main.rs:154 (may panic)
        rows.push_back({std::to_string(p), std::to_string(start_offsets[i]), std::to_string(end_offsets[i]),
                        u(m.total(p)), u(m.alive(p)), u(m.tombstones(p)), format_f32_4(m.dirty_ratio(p)),
                        u(m.key_null(p)), u(m.key_non_null(p)), u(m.key_size_sum(p) + m.value_size_sum(p)),
                        u(m.key_size_sum(p)), u(m.value_size_sum(p)), u(key_size_avg), u(m.value_size_avg(p)),
                        u(m.message_size_avg(p))});
    }
    o += "| K = Key, V = Value, P = Partition, Tmb = Tombstone(s), Sz = Size\n";    // :174
    o += "| DR = Dirty Ratio, A = Average, Lst = last, < OS = start offset, > OS = end offset\n";  // :175
    o += pretty_table(rows);                                                       // :176
    o += "\n";                                                                     // :177
    o += eq + "\n";                                                                // :178
    return o;
}

// The opt-in analytics section (kta.analytics=1): no reference counterpart, printed after the reference report's
// closing rule so that the report itself stays byte for byte the reference's.
std::string render_analytics(const Analytics &a)
{
    auto u = [](uint64_t v) { return std::to_string(v); };
    const uint64_t records = a.records();
    auto pct = [&](uint64_t count) {
        char buf[32];
        snprintf(buf, sizeof buf, "%.2f", records ? (double)count * 100.0 / (double)records : 0.0);
        return std::string(buf);
    };
    std::string o;
    o += "Size histograms and per-partition extrema (kta.analytics=1; not part of the reference report)\n";
    std::vector<std::vector<std::string>> rows;
    rows.push_back({"Bytes", "Keys", "Keys %", "Values", "Vals %"});
    for (int b = 0; b < KTA_HIST_BUCKETS; b++) {
        const uint64_t k = a.hist.key_size_hist[b], v = a.hist.value_size_hist[b];
        if (b >= 2 && k == 0 && v == 0) continue;   // None and 0 always, a log2 bucket when somebody is in it
        std::string label;
        if (b == 0) label = "None";
        else if (b == 1) label = "0";
        else if (b == 2) label = "1";
        else label = u(1ull << (b - 2)) + "-" + u((2ull << (b - 2)) - 1);
        rows.push_back({label, u(k), pct(k), u(v), pct(v)});
    }
    o += pretty_table(rows);
    o += "\n";
    rows.clear();
    rows.push_back({"P", "Earliest", "Latest", "Smallest", "Largest"});
    for (size_t p = 0; p < a.min_ts_sec.size(); p++) {
        const bool seen = a.max_ts_sec[p] != INT64_MIN, live = a.largest[p] != 0 || a.smallest[p] != UINT64_MAX;
        rows.push_back({std::to_string(p), seen ? format_datetime_utc(a.min_ts_sec[p], 0) : "-",
                        seen ? format_datetime_utc(a.max_ts_sec[p], 0) : "-", live ? u(a.smallest[p]) : "-",
                        live ? u(a.largest[p]) : "-"});
    }
    o += pretty_table(rows);
    o += std::string(120, '=') + "\n";
    return o;
}

// A width in ms as kta.timeline takes it: the largest of d, h, m, s that divides it, else ms.
std::string format_width_ms(int64_t w)
{
    static const struct { int64_t ms; const char *unit; } units[] = {{86400000, "d"}, {3600000, "h"}, {60000, "m"}, {1000, "s"}};
    for (const auto &u : units)
        if (w % u.ms == 0) return std::to_string(w / u.ms) + u.unit;
    return std::to_string(w) + "ms";
}

static std::string format_ms_utc(int64_t ms)   // ms >= 0
{
    return format_datetime_utc(ms / 1000, (uint32_t)(ms % 1000) * 1000000u);
}

// The opt-in timeline section (kta.timeline=<width>): no reference counterpart, printed after the reference report's
// closing rule (and after the analytics section).  vec: u64[(n_buckets + 3) * 3] (kta_hip.h).
std::string render_timeline(const uint64_t *vec, int64_t origin_ms, int64_t bucket_ms, uint32_t n_buckets)
{
    auto u = [](uint64_t v) { return std::to_string(v); };
    const uint32_t rows_n = n_buckets + 3u;
    uint64_t records = 0;
    for (uint32_t r = 0; r < rows_n; r++) records += vec[(size_t)r * KTA_TIMELINE_COLS];
    auto pct = [&](uint64_t count) {
        char buf[32];
        snprintf(buf, sizeof buf, "%.2f", records ? (double)count * 100.0 / (double)records : 0.0);
        return std::string(buf);
    };
    const std::string start = format_ms_utc(origin_ms);
    std::string o;
    o += "Timeline, " + format_width_ms(bucket_ms) + " buckets from " + start +
         " (kta.timeline; not part of the reference report)\n";
    std::vector<std::vector<std::string>> rows;
    rows.push_back({"From", "Records", "Records %", "Tmb", "Bytes"});
    auto row = [&](const std::string &label, uint32_t r) {
        const uint64_t *x = vec + (size_t)r * KTA_TIMELINE_COLS;
        rows.push_back({label, u(x[0]), pct(x[0]), u(x[1]), u(x[2])});
    };
    row("No timestamp", 0);
    row("Before " + start, 1);
    uint32_t first = n_buckets, last = 0;
    for (uint32_t k = 0; k < n_buckets; k++)
        if (vec[(size_t)(2 + k) * KTA_TIMELINE_COLS] != 0) {
            first = std::min(first, k);
            last = k;
        }
    for (uint32_t k = first; k < n_buckets && k <= last; k++) row(format_ms_utc(origin_ms + (int64_t)k * bucket_ms), 2 + k);
    row("After " + format_ms_utc(origin_ms + (int64_t)n_buckets * bucket_ms), n_buckets + 2);
    o += pretty_table(rows);
    o += std::string(120, '=') + "\n";
    return o;
}

// The opt-in key sketch section (kta.distinct_keys=1): no reference counterpart, printed after the reference report's
// closing rule (and after the analytics and timeline sections).
std::string render_distinct_keys(const uint64_t *sketch, const std::vector<uint64_t> &keyed)
{
    const uint32_t P = (uint32_t)keyed.size();
    std::vector<double> est(P);
    double topic = 0.0;
    if (kta_key_sketch_estimate(sketch, P, est.data(), &topic) != KTA_OK) return std::string();
    auto u = [](uint64_t v) { return std::to_string(v); };
    auto count = [](double e) { return std::isfinite(e) ? std::to_string((uint64_t)std::llround(e)) : std::string("inf"); };
    auto per_key = [](uint64_t records, double e) {
        if (!std::isfinite(e) || std::llround(e) == 0) return std::string("-");
        char buf[48];
        snprintf(buf, sizeof buf, "%.2f", (double)records / (double)std::llround(e));
        return std::string(buf);
    };
    std::string o;
    o += "Distinct keys per partition, estimated (HyperLogLog of the key hashes, +/-1.6 %; kta.distinct_keys=1; not part of the "
         "reference report)\n";
    std::vector<std::vector<std::string>> rows;
    rows.push_back({"P", "Keyed records", "Distinct keys", "Records per key"});
    uint64_t all = 0;
    for (uint32_t p = 0; p < P; p++) {
        all += keyed[p];
        if (keyed[p] == 0) rows.push_back({std::to_string(p), "0", "-", "-"});
        else rows.push_back({std::to_string(p), u(keyed[p]), count(est[p]), per_key(keyed[p], est[p])});
    }
    if (all == 0) rows.push_back({"Topic", "0", "-", "-"});
    else rows.push_back({"Topic", u(all), count(topic), per_key(all, topic)});
    o += pretty_table(rows);
    o += std::string(120, '=') + "\n";
    return o;
}

// The opt-in timestamp-order section (kta.ts_order=1): no reference counterpart, printed after the analytics, timeline and
// distinct-key sections and before the hot keys.  vec: u64[3 P + 64] (kta_hip.h), records[p] = total_messages.
std::string render_ts_order(const uint64_t *vec, const std::vector<uint64_t> &records)
{
    const uint32_t P = (uint32_t)records.size();
    const uint64_t *hist = vec + 2 * (size_t)P, timed = vec[2 * (size_t)P + KTA_TS_ORDER_HIST], *most = vec + 2 * (size_t)P + 64;
    auto u = [](uint64_t v) { return std::to_string(v); };
    auto pct = [](uint64_t count, uint64_t of) {
        char buf[32];
        snprintf(buf, sizeof buf, "%.2f", of ? (double)count * 100.0 / (double)of : 0.0);
        return std::string(buf);
    };
    std::string o;
    o += "Timestamp order: records older than one their partition delivered before them (kta.ts_order=1; not part of the "
         "reference report)\n";
    std::vector<std::vector<std::string>> rows;
    rows.push_back({"P", "Records", "Late records", "Late %", "Mean lateness ms", "Max lateness ms"});
    uint64_t all = 0, late_all = 0, sum_all = 0, most_all = 0;
    for (uint32_t p = 0; p < P; p++) {
        const uint64_t late = vec[2 * (size_t)p], sum = vec[2 * (size_t)p + 1];
        all += records[p], late_all += late, sum_all += sum, most_all = std::max(most_all, most[p]);
        rows.push_back({std::to_string(p), u(records[p]), u(late), pct(late, records[p]), late ? u(sum / late) : "-", late ? u(most[p]) : "-"});
    }
    rows.push_back({"Topic", u(all), u(late_all), pct(late_all, all), late_all ? u(sum_all / late_all) : "-", late_all ? u(most_all) : "-"});
    o += pretty_table(rows);
    o += "Records without a timestamp: " + u(all - timed) + "\n";
    uint32_t first = KTA_TS_ORDER_HIST, last = 0;
    for (uint32_t k = 0; k < KTA_TS_ORDER_HIST; k++)
        if (hist[k] != 0) {
            first = std::min(first, k);
            last = k;
        }
    if (first == KTA_TS_ORDER_HIST) {
        o += "No record is late.\n";
    } else {
        rows.clear();
        rows.push_back({"Late by", "Records", "Cumulative %"});
        uint64_t within = timed - late_all;   // in order
        for (uint32_t k = first; k <= last; k++) {
            within += hist[k];
            rows.push_back({"< " + u(2ull << k) + " ms", u(hist[k]), pct(within, timed)});
        }
        o += pretty_table(rows);
    }
    o += std::string(120, '=') + "\n";
    return o;
}

// The opt-in retention section (kta.segments=<size>): no reference counterpart, printed after the partitioner and compaction
// sections and before the filter's.  vec: u64[(P M + P) 4 + 8] (kta_hip.h); retention -1: the rule is off, and with both
// off the segment columns alone.
std::string render_retention(const uint64_t *vec, uint32_t P, uint32_t M, int64_t now_ms, int64_t retention_ms, int64_t retention_bytes)
{
    std::vector<uint64_t> w((size_t)(P + 1) * kRetWords);
    if (kta_retention_whatif(vec, P, M, now_ms, retention_ms, retention_bytes, w.data(), w.size()) != KTA_OK) return std::string();
    const uint64_t *g = vec + segments_globals_at(P, M);
    const bool policy = retention_ms >= 0 || retention_bytes >= 0;
    auto u = [](uint64_t v) { return std::to_string(v); };
    auto rule = [](int64_t v) { return v < 0 ? std::string("-") : std::to_string(v); };
    std::string o = "Retention what-if: model log segments of " + u(g[kSegGlobalS]) + " bytes per partition (kta.segments), ";
    if (policy) o += "retention.ms=" + rule(retention_ms) + ", retention.bytes=" + rule(retention_bytes) + ", now=" + std::to_string(now_ms) + " ms";
    else o += "no retention policy given";
    o += " (not part of the reference report)\n";
    std::vector<std::vector<std::string>> rows;
    if (policy) rows.push_back({"P", "Segments", "Records", "Bytes", "Records kept", "Bytes kept", "Reclaimed %", "Rule"});
    else rows.push_back({"P", "Segments", "Records", "Bytes"});
    for (uint32_t p = 0; p <= P; p++) {
        const uint64_t *r = w.data() + (size_t)p * kRetWords;
        const bool all = p == P;
        std::vector<std::string> row{all ? "All" : std::to_string(p), u(r[kRetSegments]) + (!all && r[kRetClamped] ? "+" : ""), u(r[kRetRecords]),
                                     u(r[kRetBytes])};
        if (policy) {
            char buf[32];
            snprintf(buf, sizeof buf, "%.2f", r[kRetBytes] ? (double)(r[kRetBytes] - r[kRetBytesKept]) * 100.0 / (double)r[kRetBytes] : 0.0);
            const char *const names[4] = {"-", "time", "size", "time+size"};
            row.insert(row.end(), {u(r[kRetRecordsKept]), u(r[kRetBytesKept]), r[kRetBytes] ? buf : "-", names[r[kRetRule] & 3u]});
        }
        rows.push_back(row);
    }
    o += pretty_table(rows);
    const uint64_t clamped = w[(size_t)P * kRetWords + kRetClamped];
    if (clamped)
        o += u(clamped) + " partition(s) outgrew the " + u(M) + " rows kept per partition (Segments ends in +): the last row holds the rest and "
             "counts as the active segment (kta.segments.rows).\n";
    o += "Model: a segment ends with the record whose bytes reach its size, so a boundary can differ from the broker's by one record per "
         "segment; segment.ms is not modelled; a record's size is key + value + " + u(g[kSegGlobalOverhead]) + " bytes, not bytes on disk (no batch "
         "headers, no compression); the active segment is never deleted, and a prefix without any timestamp is not deleted by time.\n";
    o += std::string(120, '=') + "\n";
    return o;
}

// The opt-in partitioner section (kta.partitioner=murmur2): no reference counterpart, printed last of all.  vec: u64[2 P + 2 Q]
// (kta_hip.h), counters: the counter vector's per-partition words.
std::string render_partitioner(const uint64_t *vec, const uint64_t *counters, uint32_t P, uint32_t Q)
{
    auto u = [](uint64_t v) { return std::to_string(v); };
    auto pct = [](uint64_t count, uint64_t of) {
        if (!of) return std::string("-");
        char buf[32];
        snprintf(buf, sizeof buf, "%.2f", (double)count * 100.0 / (double)of);
        return std::string(buf);
    };
    // largest / mean of n values whose sum is `sum`
    auto skew = [](uint64_t largest, uint64_t sum, uint32_t n) {
        if (!sum) return std::string("-");
        char buf[32];
        snprintf(buf, sizeof buf, "%.2f", (double)largest * (double)n / (double)sum);
        return std::string(buf);
    };
    std::string o;
    o += "Partitioner check: keyed records on the partition Kafka's default partitioner (murmur2) gives their key "
         "(kta.partitioner=murmur2; not part of the reference report)\n";
    std::vector<std::vector<std::string>> rows;
    rows.push_back({"P", "Keyed records", "On murmur2's partition", "%"});
    uint64_t checked_all = 0, placed_all = 0, no_key = 0, keyed_most = 0, keyed_sum = 0, bytes_most = 0, bytes_sum = 0;
    for (uint32_t p = 0; p < P; p++) {
        const uint64_t checked = vec[2 * (size_t)p], placed = vec[2 * (size_t)p + 1];
        const uint64_t *c = counters + (size_t)p * KTA_NCOUNTERS;
        const uint64_t bytes = c[KTA_C_KEY_SIZE_SUM] + c[KTA_C_VALUE_SIZE_SUM];
        checked_all += checked, placed_all += placed, no_key += c[KTA_C_KEY_NULL];
        keyed_sum += c[KTA_C_KEY_NON_NULL], keyed_most = std::max(keyed_most, c[KTA_C_KEY_NON_NULL]);
        bytes_sum += bytes, bytes_most = std::max(bytes_most, bytes);
        rows.push_back({std::to_string(p), u(checked), checked ? u(placed) : "-", pct(placed, checked)});
    }
    rows.push_back({"Topic", u(checked_all), checked_all ? u(placed_all) : "-", pct(placed_all, checked_all)});
    o += pretty_table(rows);
    o += "Records without a key: " + u(no_key) + " (the default partitioner spreads them without a hash)\n";
    if (checked_all == 0) {
        o += "No record has a key: nothing to check.\n";
    } else if (placed_all == checked_all) {
        o += "All keyed records lie on murmur2's partition: the topic is keyed as Kafka's default partitioner keys it.\n";
    } else if (P > 2 && (unsigned __int128)placed_all * P <= (unsigned __int128)checked_all * 2) {
        o += "No more keyed records lie on murmur2's partition than chance puts there (" + pct(placed_all, checked_all) + " % against 1/P = " +
             pct(1, P) + " %): the topic was not written by Kafka's default partitioner with " + u(P) + " partitions.\n";
    } else {
        o += pct(placed_all, checked_all) + " % of the keyed records lie on murmur2's partition: the topic is only partly keyed as "
             "Kafka's default partitioner keys it.\n";
    }
    o += "Repartition what-if: the keyed records over Q = " + u(Q) + " partitions by murmur2\n";
    const uint64_t *t = vec + 2 * (size_t)P;
    uint64_t rec_sum = 0, rec_most = 0, tb_sum = 0, tb_most = 0;
    for (uint32_t q = 0; q < Q; q++) {
        rec_sum += t[2 * (size_t)q], rec_most = std::max(rec_most, t[2 * (size_t)q]);
        tb_sum += t[2 * (size_t)q + 1], tb_most = std::max(tb_most, t[2 * (size_t)q + 1]);
    }
    rows.clear();
    rows.push_back({"Target", "Records", "Records %", "Bytes", "Bytes %"});
    for (uint32_t q = 0; q < Q; q++)
        rows.push_back({std::to_string(q), u(t[2 * (size_t)q]), pct(t[2 * (size_t)q], rec_sum), u(t[2 * (size_t)q + 1]), pct(t[2 * (size_t)q + 1], tb_sum)});
    o += pretty_table(rows);
    o += "Largest / mean at Q = " + u(Q) + ": records " + skew(rec_most, rec_sum, Q) + ", bytes " + skew(tb_most, tb_sum, Q) +
         "; the topic as it is (P = " + u(P) + "): records " + skew(keyed_most, keyed_sum, P) + ", bytes " + skew(bytes_most, bytes_sum, P) + "\n";
    o += std::string(120, '=') + "\n";
    return o;
}

// The opt-in size-percentile section (kta.percentiles=1): no reference counterpart, printed after the report's closing rule
// and the analytics section.  vec: u64[P * 3 * 464 + 8] (kta_hip.h; the layout and the read-off are kta_size_bins.h's).
std::string render_size_percentiles(const uint64_t *vec, uint32_t P)
{
    static const char *const kTitles[kSizeQuantities] = {"Key sizes", "Value sizes", "Message sizes (key + value of the non-tombstones)"};
    static const uint64_t kQuantiles[4][2] = {{50, 100}, {90, 100}, {99, 100}, {999, 1000}};
    auto row_of = [](const std::string &name, const uint64_t *hist) {
        uint64_t count = 0;
        uint32_t last = 0;
        for (uint32_t b = 0; b < kSizeBins; b++)
            if (hist[b]) count += hist[b], last = b;
        std::vector<std::string> row{name, std::to_string(count)};
        for (const auto &q : kQuantiles) {
            uint32_t bin = 0;
            row.push_back(size_quantile(hist, q[0], q[1], &bin) ? std::to_string(size_bin_hi(bin)) : "-");
        }
        row.push_back(count ? std::to_string(size_bin_hi(last)) : "-");
        return row;
    };
    std::string o;
    o += "Size percentiles per partition, in bytes (kta.percentiles=1; not part of the reference report)\n";
    for (uint32_t q = 0; q < kSizeQuantities; q++) {
        o += std::string(kTitles[q]) + "\n";
        std::vector<std::vector<std::string>> rows;
        rows.push_back({"P", "Count", "p50", "p90", "p99", "p99.9", "Max"});
        std::vector<uint64_t> all(kSizeBins, 0);
        for (uint32_t p = 0; p < P; p++) {
            const uint64_t *hist = vec + size_quantiles_word(p, q, 0);
            for (uint32_t b = 0; b < kSizeBins; b++) all[b] += hist[b];
            rows.push_back(row_of(std::to_string(p), hist));
        }
        rows.push_back(row_of("All", all.data()));
        o += pretty_table(rows);
    }
    o += "Sizes below 32 B are exact; a size of 32 B and more is the upper end of its bin, at most 6.25 % wide.\n";
    o += std::string(120, '=') + "\n";
    return o;
}

// The opt-in compaction section (-c with kta.compaction=1): no reference counterpart, printed after the partitioner section
// and before the filter section.  vec: u64[5 P + 6] (kta_hip.h; the layout is kta_compaction.h's), counters: the first
// pass's counter vector with its globals.
std::string render_compaction(const uint64_t *vec, const uint64_t *counters, uint32_t P, bool *matched)
{
    auto u = [](uint64_t v) { return std::to_string(v); };
    // the share of `now` that is not kept
    auto reclaimed = [](uint64_t kept, uint64_t now) {
        if (!now) return std::string("n/a");
        char buf[32];
        snprintf(buf, sizeof buf, "%.2f", ((double)now - (double)kept) * 100.0 / (double)now);
        return std::string(buf);
    };
    const uint64_t *g = vec + (size_t)kCompactionWords * P, *cg = counters + (size_t)P * KTA_NCOUNTERS;
    const uint64_t shown = cg[KTA_G_RECORDS] + cg[KTA_G_BAD_PARTITION];
    const bool ok = g[kCompactionUnknownRecords] == 0 && g[kCompactionReplayed] == shown;
    if (matched) *matched = ok;
    std::string o;
    o += "Compaction what-if: the records and bytes log compaction would keep (kta.compaction=1; not part of the reference report)\n";
    if (!ok) {
        o += "The replay did not match the first pass: replayed " + u(g[kCompactionReplayed]) + " of " + u(shown) + " records, " +
             u(g[kCompactionUnknownRecords]) + " of them unknown to the table. Nothing is reported.\n";
        o += std::string(120, '=') + "\n";
        return o;
    }
    std::vector<std::vector<std::string>> rows;
    rows.push_back({"P", "Records", "Kept", "Live", "Tombstones", "Records reclaimed %", "Bytes", "Bytes kept", "Bytes reclaimed %"});
    uint64_t rec_all = 0, live_all = 0, tomb_all = 0, bytes_all = 0, kept_bytes_all = 0;
    for (uint32_t p = 0; p < P; p++) {
        const uint64_t *w = vec + (size_t)kCompactionWords * p, *c = counters + (size_t)p * KTA_NCOUNTERS;
        const uint64_t live = w[kCompactionLiveRecords], tomb = w[kCompactionTombstoneRecords];
        const uint64_t kept_bytes = w[kCompactionLiveKeyBytes] + w[kCompactionLiveValueBytes] + w[kCompactionTombstoneKeyBytes];
        const uint64_t bytes = c[KTA_C_KEY_SIZE_SUM] + c[KTA_C_VALUE_SIZE_SUM];
        rec_all += c[KTA_C_TOTAL], live_all += live, tomb_all += tomb, bytes_all += bytes, kept_bytes_all += kept_bytes;
        rows.push_back({std::to_string(p), u(c[KTA_C_TOTAL]), u(live + tomb), u(live), u(tomb), reclaimed(live + tomb, c[KTA_C_TOTAL]), u(bytes),
                        u(kept_bytes), reclaimed(kept_bytes, bytes)});
    }
    rows.push_back({"Topic", u(rec_all), u(live_all + tomb_all), u(live_all), u(tomb_all), reclaimed(live_all + tomb_all, rec_all), u(bytes_all),
                    u(kept_bytes_all), reclaimed(kept_bytes_all, bytes_all)});
    o += pretty_table(rows);
    o += "Records without a key: " + u(g[kCompactionUnkeyedRecords]) + " (not kept: compaction goes by key)\n";
    if (g[kCompactionLiveOutsideRecords] || g[kCompactionTombstonesOutsideRecords])
        o += "Kept outside the partition range: " + u(g[kCompactionLiveOutsideRecords]) + " live, " + u(g[kCompactionTombstonesOutsideRecords]) +
             " tombstones\n";
    o += "Keys are counted by 32-bit hash slot, topic-wide, as \"Alive keys\" is: a key written to several partitions is kept once.\n";
    o += std::string(120, '=') + "\n";
    return o;
}

// The opt-in compact,delete section (kta.compact_delete=1): no reference counterpart, printed after the retention section and
// before the filter's.  seg / kept: u64[(P M + P) 4 + 8], comp: u64[5 P + 6] (kta_hip.h); retention -1: the rule is off.
std::string render_compact_delete(const uint64_t *seg, const uint64_t *kept, const uint64_t *comp, uint32_t P, uint32_t M, int64_t now_ms,
                                  int64_t retention_ms, int64_t retention_bytes, bool *matched)
{
    if (matched) *matched = false;
    if (!seg || !kept || !comp || !segments_config_ok(1, M, P) || P > kCompactDeleteMaxPartitions || retention_ms < -1 || retention_bytes < -1)
        return std::string();
    const uint64_t *g = seg + segments_globals_at(P, M);
    if (g[kSegGlobalM] != M || !segments_config_ok(g[kSegGlobalS], M, P)) return std::string();
    auto u = [](uint64_t v) { return std::to_string(v); };
    auto rule = [](int64_t v) { return v < 0 ? std::string("-") : std::to_string(v); };
    std::string o = "Compact,delete what-if: cleanup.policy=compact,delete over model log segments of " + u(g[kSegGlobalS]) +
                    " bytes per partition (kta.compact_delete), retention.ms=" + rule(retention_ms) + ", retention.bytes=" + rule(retention_bytes) +
                    ", now=" + (retention_ms < 0 ? std::string("-") : std::to_string(now_ms)) +
                    " ms; the active segment is not cleaned (not part of the reference report)\n";
    std::vector<uint64_t> w((size_t)(P + 1) * kCdWords);
    if (kta_compact_delete_whatif(seg, kept, comp, P, M, now_ms, retention_ms, retention_bytes, w.data(), w.size()) != KTA_OK) {
        o += "The replay did not match the first pass. Nothing is reported.\n";
        o += std::string(120, '=') + "\n";
        return o;
    }
    if (matched) *matched = true;
    std::vector<std::vector<std::string>> rows;
    rows.push_back({"P", "Records", "Bytes", "Compacted records", "Compacted bytes", "Kept records", "Kept bytes", "Tombstones kept", "Reclaimed %",
                    "Rule"});
    for (uint32_t p = 0; p <= P; p++) {
        const uint64_t *r = w.data() + (size_t)p * kCdWords;
        const bool all = p == P;
        char buf[32];
        snprintf(buf, sizeof buf, "%.2f", r[kCdBytes] ? ((double)r[kCdBytes] - (double)r[kCdKeptBytes]) * 100.0 / (double)r[kCdBytes] : 0.0);
        const char *const names[4] = {"-", "time", "size", "time+size"};
        rows.push_back({all ? "All" : std::to_string(p) + (r[kCdClamped] ? "+" : ""), u(r[kCdRecords]), u(r[kCdBytes]), u(r[kCdCompactedRecords]),
                        u(r[kCdCompactedBytes]), u(r[kCdKeptRecords]), u(r[kCdKeptBytes]), u(r[kCdKeptTombstones]), r[kCdBytes] ? buf : "-",
                        names[r[kCdRule] & 3u]});
    }
    o += pretty_table(rows);
    const uint64_t clamped = w[(size_t)P * kCdWords + kCdClamped];
    if (clamped)
        o += u(clamped) + " partition(s) outgrew the " + u(M) + " rows kept per partition (P ends in +): the last row holds the rest and counts as "
             "the active segment (kta.segments.rows).\n";
    o += "Model: a segment ends with the record whose bytes reach its size, so a boundary can differ from the broker's by one record per "
         "segment; segment.ms is not modelled; a record's size is key + value + " + u(g[kSegGlobalOverhead]) + " bytes, not bytes on disk (no batch "
         "headers, no compression); the active segment is never cleaned and never deleted, and a prefix without any timestamp is not deleted by "
         "time. Keys are counted by 32-bit hash slot, topic-wide, as \"Alive keys\" is: a key written to several partitions is kept once. The "
         "time rule uses the largest timestamp of all records up to a segment's end, cleaned away or not, so it keeps at least what the broker "
         "keeps. delete.retention.ms, min.compaction.lag.ms and min.cleanable.dirty.ratio are not modelled: every tombstone that survives is "
         "kept, and every closed segment counts as cleaned.\n";
    o += std::string(120, '=') + "\n";
    return o;
}

// The section of a filtered run (kta.from, kta.to, kta.partitions): no reference counterpart, printed after everything else.
// The filter as given — bounds in epoch seconds as the keys take them, the set as ascending ranges — then the records
// the run was handed and the records that passed.  bitmap null: no set; else ceil(P / 32) words (kta_set_filter).
std::string render_filter(int64_t from_ms, int64_t to_ms, const uint32_t *bitmap, uint32_t P, uint64_t seen, uint64_t passed)
{
    auto bound = [](int64_t ms) {
        std::string t = std::to_string(ms / 1000);
        if (ms % 1000) {                                    // (set through the library, not the keys: whole milliseconds)
            char buf[8];
            snprintf(buf, sizeof buf, ".%03d", (int)((ms % 1000 + 1000) % 1000));
            t += buf;
        }
        return t + " s (" + std::to_string(ms) + " ms)";
    };
    std::string set = "all";
    if (bitmap) {
        set.clear();
        for (uint32_t p = 0; p < P;) {
            if (!((bitmap[p >> 5] >> (p & 31u)) & 1u)) { p++; continue; }
            uint32_t q = p;
            while (q + 1 < P && ((bitmap[(q + 1) >> 5] >> ((q + 1) & 31u)) & 1u)) q++;
            if (!set.empty()) set += ",";
            set += std::to_string(p);
            if (q > p) set += "-" + std::to_string(q);
            p = q + 1;
        }
        if (set.empty()) set = "none";
    }
    std::string share = "-";
    if (seen) {
        char buf[32];
        snprintf(buf, sizeof buf, "%.2f", (double)passed * 100.0 / (double)seen);
        share = buf;
    }
    std::string o;
    o += "Record filter: everything above describes the records that passed, and no others "
         "(kta.from, kta.to, kta.partitions; not part of the reference report)\n";
    std::vector<std::vector<std::string>> rows;
    rows.push_back({"Filter", "Value"});
    rows.push_back({"From (timestamp >=)", from_ms == INT64_MIN ? "-" : bound(from_ms)});
    rows.push_back({"To (timestamp <)", to_ms == INT64_MAX ? "-" : bound(to_ms)});
    rows.push_back({"Partitions", set});
    rows.push_back({"Records seen", std::to_string(seen)});
    rows.push_back({"Records passed", std::to_string(passed)});
    rows.push_back({"Passed %", share});
    o += pretty_table(rows);
    o += std::string(120, '=') + "\n";
    return o;
}

// The opt-in record-batch section (kta.record_batches=1): no reference counterpart, printed after everything else.  vec:
// u64[20 P + 1524] (kta_hip.h; the layout is kta_record_batches.h's).  skipped: the host index's control batches, magic 0/1
// sets and batches of an unknown codec over the run.  A figure whose denominator is 0 is `n/a`.
std::string render_record_batches(const uint64_t *vec, uint32_t P, bool filtered, const uint64_t skipped[3])
{
    auto ratio = [](uint64_t num, uint64_t den, double scale) -> std::string {
        if (den == 0) return "n/a";
        char buf[48];
        snprintf(buf, sizeof buf, "%.2f", (double)num * scale / (double)den);
        return buf;
    };
    // the upper end of the bin in which a histogram reaches num/den of its count (nearest rank)
    auto bin_quantile = [](const uint64_t *hist, uint64_t num, uint64_t den) -> std::string {
        uint64_t count = 0;
        for (uint32_t b = 0; b < kRbHistBins; b++) count += hist[b];
        if (count == 0) return "n/a";
        uint64_t rank = (count * num + den - 1) / den, run = 0;
        if (rank == 0) rank = 1;
        for (uint32_t b = 0; b < kRbHistBins; b++) {
            run += hist[b];
            if (run >= rank) return b == 0 ? "0" : (b == kRbHistBins - 1 ? ">=" + std::to_string(1ull << 30) : std::to_string((1ull << b) - 1));
        }
        return "n/a";
    };
    auto row_of = [&](const std::string &name, const uint64_t *w, const uint64_t *mx) {
        const uint64_t batches = w[kRbBatches], holes = w[kRbExtent] - w[kRbRecords];
        return std::vector<std::string>{name,
                                        std::to_string(batches),
                                        ratio(w[kRbRecords], batches, 1.0),
                                        std::to_string(mx[kRbMaxRecords]),
                                        ratio(w[kRbWire], batches, 1.0),
                                        std::to_string(mx[kRbMaxWire]),
                                        ratio(w[kRbSpanMs], batches, 1.0),
                                        ratio(w[kRbCompressed], batches, 100.0),
                                        ratio(w[kRbCompressedPayload], w[kRbCompressedRecbytes], 1.0),
                                        std::to_string(holes),
                                        ratio(holes, w[kRbExtent], 100.0),
                                        ratio(w[kRbIdempotent], batches, 100.0),
                                        ratio(w[kRbTransactional], batches, 100.0),
                                        ratio(w[kRbLogAppendTime], batches, 100.0),
                                        mx[kRbMaxEpoch1] ? std::to_string(mx[kRbMaxEpoch1] - 1) : "-",
                                        std::to_string(w[kRbFailed])};
    };
    std::string o;
    o += "Record batches: what the batch headers of the log say (kta.record_batches=1; not part of the reference report)\n";
    std::vector<std::vector<std::string>> rows;
    rows.push_back({"P", "Batches", "Rec/batch", "Largest", "B/batch", "Largest", "Span ms", "Compressed %", "Ratio", "Holes", "Holes %",
                    "Idempotent %", "Transactional %", "LogAppendTime %", "Epoch", "Failed"});
    uint64_t all[kRbPartitionWords] = {}, all_mx[kRbMaxWords] = {};
    for (uint32_t p = 0; p < P; p++) {
        const uint64_t *w = vec + (size_t)kRbPartitionWords * p, *mx = vec + rb_max_at(P, p);
        for (uint32_t k = 0; k < kRbPartitionWords; k++) all[k] += w[k];
        for (uint32_t k = 0; k < kRbMaxWords; k++) all_mx[k] = std::max(all_mx[k], mx[k]);
        rows.push_back(row_of(std::to_string(p), w, mx));
    }
    rows.push_back(row_of("Topic", all, all_mx));
    o += pretty_table(rows);
    static const char *const kCodecNames[kRbCodecs] = {"none", "gzip", "snappy", "lz4", "zstd"};
    rows.clear();
    rows.push_back({"Codec", "Batches", "Records", "Bytes on disk", "Inflated bytes", "Ratio", "Rec/batch p50", "p90", "B/batch p50", "p90"});
    for (uint32_t c = 0; c < kRbCodecs; c++) {
        const uint64_t *cw = vec + rb_codec_at(P, c);
        rows.push_back({kCodecNames[c], std::to_string(cw[kRbCodecBatches]), std::to_string(cw[kRbCodecRecords]), std::to_string(cw[kRbCodecRecbytes]),
                        std::to_string(cw[kRbCodecPayload]), ratio(cw[kRbCodecPayload], cw[kRbCodecRecbytes], 1.0),
                        bin_quantile(cw + kRbCodecHistRecords, 50, 100), bin_quantile(cw + kRbCodecHistRecords, 90, 100),
                        bin_quantile(cw + kRbCodecHistWire, 50, 100), bin_quantile(cw + kRbCodecHistWire, 90, 100)});
    }
    o += pretty_table(rows);
    o += "Percentiles are the upper ends of power-of-two bins; bytes on disk and inflated bytes are the records alone, without the 61-byte headers.\n";
    char buf[96];
    snprintf(buf, sizeof buf, "Producers (estimated from the idempotent batches, +/- %.2f %%): %.0f\n", kRbStdError * 100.0, rb_estimate(vec + rb_sketch_at(P)));
    o += buf;
    o += "Not counted: control batches (" + std::to_string(skipped[0]) + "), magic 0/1 message sets (" + std::to_string(skipped[1]) +
         "), batches of an unknown codec (" + std::to_string(skipped[2]) + ") and batches without records; a failed batch adds to Failed alone.\n";
    if (filtered) o += "With the record filter: these are the batches that overlap the window on the selected partitions, not the records that passed.\n";
    o += std::string(120, '=') + "\n";
    return o;
}

// The opt-in payload section (kta.payload=1): no reference counterpart, printed after everything else.  vec: u64[24 P + 69648]
// (kta_hip.h; the layout is kta_payload.h's).  counters: the counter vector (key_size_sum and value_size_sum are read), or
// nullptr.  A figure whose denominator is 0 is `n/a`.
std::string render_payload(const uint64_t *vec, const uint64_t *counters, uint32_t P)
{
    auto ratio = [](uint64_t num, uint64_t den, double scale) -> std::string {
        if (den == 0) return "n/a";
        char buf[48];
        snprintf(buf, sizeof buf, "%.2f", (double)num * scale / (double)den);
        return buf;
    };
    auto row_of = [&](const std::string &name, const uint64_t *w, bool sized, uint64_t key_value) {
        const uint64_t records = w[kPlRecords], wire = w[kPlHeaderWireBytes];
        std::vector<std::string> r{name, std::to_string(records)};
        for (uint32_t c = 0; c < kPlClasses; c++) r.push_back(ratio(w[kPlClass + c], records, 100.0));
        r.push_back(std::to_string(w[kPlWithHeaders]));
        r.push_back(ratio(w[kPlHeaders], records - w[kPlBadHeaders], 1.0));
        r.push_back(sized ? ratio(wire, key_value + wire, 100.0) : "n/a");
        r.push_back(std::to_string(w[kPlBadHeaders]));
        return r;
    };
    std::string o;
    o += "Payload: value formats, schema-registry ids and record headers (kta.payload=1; not part of the reference report)\n";
    std::vector<std::vector<std::string>> rows;
    rows.push_back({"P", "Records", "Null %", "Empty %", "Framed %", "JSON %", "Other %", "With headers", "Headers/rec", "Header bytes %", "Bad headers"});
    uint64_t all[kPlPartitionWords] = {}, all_kv = 0;
    for (uint32_t p = 0; p < P; p++) {
        const uint64_t *w = vec + (size_t)kPlPartitionWords * p;
        const uint64_t kv = counters ? counters[(size_t)KTA_NCOUNTERS * p + KTA_C_KEY_SIZE_SUM] + counters[(size_t)KTA_NCOUNTERS * p + KTA_C_VALUE_SIZE_SUM] : 0;
        for (uint32_t k = 0; k < kPlPartitionWords; k++) all[k] += w[k];
        all_kv += kv;
        rows.push_back(row_of(std::to_string(p), w, counters != nullptr, kv));
    }
    rows.push_back(row_of("Topic", all, counters != nullptr, all_kv));
    o += pretty_table(rows);
    rows.clear();
    rows.push_back({"Headers", "Records"});
    for (uint32_t b = 0; b < kPlHistBins; b++)
        rows.push_back({b == kPlHistBins - 1 ? ">=" + std::to_string(b) : std::to_string(b), std::to_string(vec[payload_hist_at(P) + b])});
    o += pretty_table(rows);
    uint64_t unresolved_records = 0, unresolved_bytes = 0;
    const std::vector<PayloadSchemaId> ids = payload_schema_ids(vec, P, &unresolved_records, &unresolved_bytes);
    constexpr size_t kShown = 64;
    if (ids.empty() && unresolved_records == 0) {
        o += "Schema ids: none (no value begins with the byte 0x00 and is five bytes or longer)\n";
    } else {
        rows.clear();
        rows.push_back({"Schema id", "Records", "Bytes", "B/record"});
        for (size_t i = 0; i < ids.size() && i < kShown; i++)
            rows.push_back({std::to_string(ids[i].id), std::to_string(ids[i].records), std::to_string(ids[i].bytes), ratio(ids[i].bytes, ids[i].records, 1.0)});
        o += pretty_table(rows);
        if (ids.size() > kShown) o += "... and " + std::to_string(ids.size() - kShown) + " more\n";
        if (unresolved_records)
            o += "Unresolved: " + std::to_string(unresolved_records) + " records, " + std::to_string(unresolved_bytes) +
                 " bytes in table cells that hold several ids\n";
    }
    o += "Framed is a heuristic of two conditions (first byte 0x00, five bytes or more); the ids are the topic's, not a subject's; header names are "
         "not listed; failed batches are not described.\n";
    o += std::string(120, '=') + "\n";
    return o;
}

// murmur3's finaliser, as the device puts it behind the key hash (kta_hip.h, KTA_FLAG_KEY_SKETCH)
static uint32_t fmix32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x85ebca6bu;
    x ^= x >> 13;
    x *= 0xc2b2ae35u;
    x ^= x >> 16;
    return x;
}

// The first min(len, kept) bytes of a key or a name as the sections print them: printable ASCII but the backslash as it is,
// every other byte as \xHH; `...` behind one that was longer than what is kept.
static std::string escaped_bytes(const uint8_t *bytes, uint64_t len, uint32_t kept)
{
    std::string t;
    const uint32_t shown = (uint32_t)std::min<uint64_t>(len, kept);
    for (uint32_t b = 0; b < shown; b++) {
        const uint8_t ch = bytes[b];
        if (ch >= 0x20 && ch < 0x7f && ch != '\\') {
            t += (char)ch;
        } else {
            char buf[8];
            snprintf(buf, sizeof buf, "\\x%02X", ch);
            t += buf;
        }
    }
    if (len > kept) t += "...";
    return t;
}

// The opt-in hot-key section (kta.hot_keys=K): no reference counterpart, printed after every other section.
std::string render_hot_keys(const uint64_t *vec, const kta_hot_exemplar *exemplars, uint32_t max_keys)
{
    std::vector<kta_hot_key> keys(max_keys);
    uint32_t n = 0;
    uint64_t keyed = 0;
    if (kta_hot_keys_recover(vec, max_keys, keys.data(), &n, &keyed) != KTA_OK) return std::string();
    std::string o;
    o += "Hot keys, at most " + std::to_string(max_keys) + " (sums of bit counters over the key hashes, 2 rows of 1024 cells: keys from "
         "1/512 of the keyed records; kta.hot_keys=" + std::to_string(max_keys) + "; not part of the reference report)\n";
    if (n == 0) {
        o += "No key holds 1/512 of the " + std::to_string(keyed) + " keyed records.\n";
        return o;
    }
    auto key_text = [&](uint32_t hash) {
        if (!exemplars) return std::string("-");
        const uint32_t x = fmix32(hash);
        const kta_hot_exemplar *found = nullptr;
        for (const kta_hot_exemplar *e : {exemplars + (x & 1023u), exemplars + KTA_HOT_CELLS + ((x >> 10) & 1023u)})
            if (!found && e->valid && e->hash == hash) found = e;
        if (!found) return std::string("-");
        return escaped_bytes(found->bytes, found->key_len, KTA_HOT_EXEMPLAR_BYTES);
    };
    std::vector<std::vector<std::string>> rows;
    rows.push_back({"#", "Key", "Hash", "Records (at most)", "(at least)", "Share of keyed records"});
    for (uint32_t k = 0; k < n; k++) {
        char hash[16], share[32];
        snprintf(hash, sizeof hash, "%08x", keys[k].hash);
        snprintf(share, sizeof share, "%.2f", (double)keys[k].upper * 100.0 / (double)keyed);
        rows.push_back({std::to_string(k + 1), key_text(keys[k].hash), hash, std::to_string(keys[k].upper),
                        std::to_string(keys[k].lower), share});
    }
    o += pretty_table(rows);
    o += std::string(120, '=') + "\n";
    return o;
}

// The opt-in header-name section (kta.headers=1): no reference counterpart, printed behind the payload section's position.
// vec: u64[73736] (kta_hip.h; the layout and the read-off are kta_header_names.h's); table: kta_header_name[2048] or nullptr.
std::string render_header_names(const uint64_t *vec, const kta_header_name *table, uint32_t max_names)
{
    auto ratio = [](uint64_t num, uint64_t den, double scale) -> std::string {
        if (den == 0) return "n/a";
        char buf[48];
        snprintf(buf, sizeof buf, "%.2f", (double)num * scale / (double)den);
        return buf;
    };
    uint64_t unresolved = 0, unresolved_bytes = 0;
    const std::vector<HnListed> names = hn_list(vec, reinterpret_cast<const HnSlot *>(table), &unresolved, &unresolved_bytes);
    std::string o;
    o += "Header names: a census of the record headers (kta.headers=1; not part of the reference report)\n";
    o += std::to_string(vec[kHnOccurrences]) + " headers in " + std::to_string(vec[kHnWithHeaders]) + " of " + std::to_string(vec[kHnLooked]) +
         " records looked at: " + std::to_string(vec[kHnNameBytes]) + " name bytes, " + std::to_string(vec[kHnValueBytes]) + " value bytes, " +
         std::to_string(vec[kHnNullValues]) + " null values, " + std::to_string(names.size()) + " names listed\n";
    if (!names.empty()) {
        std::vector<std::vector<std::string>> rows;
        rows.push_back({"#", "Name", "Hash", "Occurrences", "per record with headers", "Name bytes", "Value bytes", "Mean value", "Null values",
                        "Share of header bytes"});
        for (size_t i = 0; i < names.size() && i < max_names; i++) {
            const HnListed &n = names[i];
            char hash[16];
            snprintf(hash, sizeof hash, "%08x", n.hash);
            const uint64_t name_bytes = n.occurrences * n.name_len;
            rows.push_back({std::to_string(i + 1), n.name ? escaped_bytes(n.name->bytes, n.name->name_len, kHnExemplarBytes) : std::string("#") + hash, hash,
                            std::to_string(n.occurrences), ratio(n.occurrences, vec[kHnWithHeaders], 1.0), std::to_string(name_bytes),
                            std::to_string(n.value_bytes), ratio(n.value_bytes, n.occurrences - n.null_values, 1.0), std::to_string(n.null_values),
                            ratio(name_bytes + n.value_bytes, vec[kHnNameBytes] + vec[kHnValueBytes], 100.0)});
        }
        o += pretty_table(rows);
        if (names.size() > max_names) o += "... and " + std::to_string(names.size() - max_names) + " more\n";
    }
    if (unresolved)
        o += "Unresolved: " + std::to_string(unresolved) + " occurrences, " + std::to_string(unresolved_bytes) +
             " value bytes in table cells that hold several names\n";
    o += std::string(120, '=') + "\n";
    return o;
}

// The opt-in value-byte section (kta.value_bytes=1): no reference counterpart, printed behind the header-name section's
// position.  vec: u64[264 P] (kta_hip.h; the layout and the read-off are kta_value_bytes.h's).
std::string render_value_bytes(const uint64_t *vec, uint32_t P)
{
    auto percent = [](uint64_t num, uint64_t den) -> std::string {
        if (den == 0) return "n/a";
        char buf[48];
        snprintf(buf, sizeof buf, "%.2f", (double)num * 100.0 / (double)den);
        return buf;
    };
    auto row_of = [&](const std::string &name, const uint64_t *words) {
        const ValueBytesSummary s = value_bytes_summary(words);
        char h0[48], top[64];
        snprintf(h0, sizeof h0, "%.2f", s.entropy_bits);
        snprintf(top, sizeof top, "0x%02X (%s%%)", s.top_byte, percent(s.top_count, s.bytes).c_str());
        return std::vector<std::string>{name, std::to_string(s.records), std::to_string(s.values), std::to_string(s.bytes),
                                        s.bytes ? std::string(h0) : std::string("n/a"), percent(s.floor_bytes, s.bytes), percent(s.printable, s.bytes),
                                        percent(s.zero, s.bytes), percent(s.high, s.bytes), percent(s.repeats, s.bytes), std::to_string(s.distinct),
                                        s.bytes ? std::string(top) : std::string("n/a"), value_bytes_class_name(s.cls)};
    };
    std::string o;
    o += "Value bytes: a byte histogram of the record values (kta.value_bytes=1; not part of the reference report)\n";
    std::vector<std::vector<std::string>> rows;
    rows.push_back({"P", "Records", "Values", "Value bytes", "H0 bits/byte", "Order-0 floor %", "Printable %", "Zero %", "High-bit %", "Repeat %",
                    "Distinct", "Top byte", "Class"});
    for (uint32_t p = 0; p < P; p++) rows.push_back(row_of(std::to_string(p), vec + (size_t)kVbPartitionWords * p));
    uint64_t topic[kVbPartitionWords];
    value_bytes_topic(vec, P, topic);
    rows.push_back(row_of("Topic", topic));
    o += pretty_table(rows);
    o += "Class is a heuristic: text = at least 95% printable bytes; dense = at least 65536 bytes and H0 >= 7.5 (compressed, encrypted or random "
         "already); binary otherwise.\n";
    o += "H0 is the order-0 entropy of the value bytes: it bounds an entropy coder alone.  LZ matching, which is most of what gzip, LZ4 or zstd win "
         "on JSON, is not in it.\n";
    o += std::string(120, '=') + "\n";
    return o;
}

// The opt-in compression what-if section (kta.compress_whatif=lz4): no reference counterpart, printed behind the value-byte
// section's position.  vec: u64[8 P + 20] (kta_hip.h; the layout is kta_lz4_model.h's).
std::string render_compress_whatif(const uint64_t *vec, uint32_t P)
{
    auto ratio = [](uint64_t num, uint64_t den, double scale) -> std::string {
        if (den == 0) return "n/a";
        char buf[48];
        snprintf(buf, sizeof buf, "%.2f", (double)num * scale / (double)den);
        return buf;
    };
    auto saving = [](uint64_t model, uint64_t now) -> std::string {            // 1 - model / now, in percent; negative: larger
        if (now == 0) return "n/a";
        char buf[48];
        snprintf(buf, sizeof buf, "%.2f", 100.0 - (double)model * 100.0 / (double)now);
        return buf;
    };
    auto row_of = [&](const std::string &name, const uint64_t *w) {
        return std::vector<std::string>{name, std::to_string(w[kCwBatches]), ratio(w[kCwRawBytes], w[kCwBatches], 1.0), std::to_string(w[kCwRawBytes]),
                                        std::to_string(w[kCwNowBytes]), ratio(w[kCwRawBytes], w[kCwNowBytes], 1.0), std::to_string(w[kCwModelBytes]),
                                        ratio(w[kCwRawBytes], w[kCwModelBytes], 1.0), saving(w[kCwModelBytes], w[kCwNowBytes]),
                                        ratio(w[kCwStoredBlocks], w[kCwBlocks], 100.0), ratio(w[kCwMatchBytes], w[kCwRawBytes], 100.0)};
    };
    std::string o;
    o += "Compression what-if: what compression.type=lz4 would leave of the record bytes (kta.compress_whatif=lz4; not part of the reference report)\n";
    std::vector<std::vector<std::string>> rows;
    rows.push_back({"P", "Batches", "Record bytes/batch", "Record bytes", "On disk now", "Now ratio", "LZ4 model", "Model ratio", "Saving vs now %",
                    "Stored blocks %", "Match %"});
    for (uint32_t p = 0; p < P; p++) rows.push_back(row_of(std::to_string(p), vec + (size_t)kCwPartitionWords * p));
    uint64_t topic[kCwPartitionWords];
    compress_whatif_topic(vec, P, topic);
    rows.push_back(row_of("Topic", topic));
    o += pretty_table(rows);
    o += "By the batches' current codec:\n";
    std::vector<std::vector<std::string>> codecs;
    codecs.push_back({"Codec", "Batches", "Record bytes", "On disk now", "Now ratio", "LZ4 model", "Model ratio"});
    for (uint32_t c = 0; c < kCwCodecs; c++) {
        const uint64_t *w = vec + (size_t)kCwPartitionWords * P + (size_t)kCwCodecWords * c;
        codecs.push_back({compress_whatif_codec_name(c), std::to_string(w[kCwCodecBatches]), std::to_string(w[kCwCodecRawBytes]),
                          std::to_string(w[kCwCodecNowBytes]), ratio(w[kCwCodecRawBytes], w[kCwCodecNowBytes], 1.0), std::to_string(w[kCwCodecModelBytes]),
                          ratio(w[kCwCodecRawBytes], w[kCwCodecModelBytes], 1.0)});
    }
    o += pretty_table(codecs);
    o += "The model is an LZ4 frame of every batch's inflated record bytes: independent blocks of 64 KiB, a greedy match finder with a table of 4096 "
         "positions that is looked up 64 positions at a time, a block that does not shrink stored.\n";
    o += "It is a floor of what compression would win: liblz4 itself finds matches the model does not see, gzip and zstd do better still.\n";
    o += "The 61 header bytes of a batch are on neither side: record bytes, on disk now and the model are all without them.\n";
    o += "The ratios hold at the topic's present batching: small batches compress badly (see Record bytes/batch), and a larger batch.size or "
         "linger.ms would change them.\n";
    o += std::string(120, '=') + "\n";
    return o;
}

}  // namespace kta

extern "C" int kta_render_compress_whatif(const uint64_t *vec, uint32_t n_partitions, char *out, size_t out_cap, size_t *out_len)
{
    if (!vec || !out_len || n_partitions == 0) return KTA_ERR_INVALID;
    const std::string text = kta::render_compress_whatif(vec, n_partitions);
    *out_len = text.size();
    if (out && out_cap > 0) {
        const size_t n = std::min(out_cap - 1, text.size());
        memcpy(out, text.data(), n);
        out[n] = 0;
    }
    return KTA_OK;
}

extern "C" int kta_render_value_bytes(const uint64_t *vec, uint32_t n_partitions, char *out, size_t out_cap, size_t *out_len)
{
    if (!vec || !out_len || n_partitions == 0) return KTA_ERR_INVALID;
    const std::string text = kta::render_value_bytes(vec, n_partitions);
    *out_len = text.size();
    if (out && out_cap > 0) {
        const size_t n = std::min(out_cap - 1, text.size());
        memcpy(out, text.data(), n);
        out[n] = 0;
    }
    return KTA_OK;
}

extern "C" int kta_render_header_names(const uint64_t *vec, const kta_header_name *table, uint32_t max_names, char *out, size_t out_cap,
                                       size_t *out_len)
{
    if (!vec || !out_len || max_names == 0) return KTA_ERR_INVALID;
    const std::string text = kta::render_header_names(vec, table, max_names);
    *out_len = text.size();
    if (out && out_cap > 0) {
        const size_t n = std::min(out_cap - 1, text.size());
        memcpy(out, text.data(), n);
        out[n] = 0;
    }
    return KTA_OK;
}

extern "C" int kta_render_hot_keys(const uint64_t *vec, const kta_hot_exemplar *exemplars, uint32_t max_keys, char *out,
                                   size_t out_cap, size_t *out_len)
{
    if (!vec || !out_len || max_keys < 1 || max_keys > KTA_HOT_MAX_REPORTED) return KTA_ERR_INVALID;
    const std::string text = kta::render_hot_keys(vec, exemplars, max_keys);
    if (text.empty()) return KTA_ERR_INVALID;   // (a vector no record set leaves)
    *out_len = text.size();
    if (out && out_cap > 0) {
        const size_t n = std::min(out_cap - 1, text.size());
        memcpy(out, text.data(), n);
        out[n] = 0;
    }
    return KTA_OK;
}

extern "C" int kta_render_ts_order(const uint64_t *vec, const uint64_t *counter_vec, uint32_t n_partitions, char *out,
                                   size_t out_cap, size_t *out_len)
{
    if (!vec || !counter_vec || !out_len || n_partitions == 0 || (int)n_partitions > kta_ts_order_max_partitions()) return KTA_ERR_INVALID;
    std::vector<uint64_t> records(n_partitions);
    for (uint32_t p = 0; p < n_partitions; p++) records[p] = counter_vec[(size_t)p * KTA_NCOUNTERS + KTA_C_TOTAL];
    const std::string text = kta::render_ts_order(vec, records);
    *out_len = text.size();
    if (out && out_cap > 0) {
        const size_t n = std::min(out_cap - 1, text.size());
        memcpy(out, text.data(), n);
        out[n] = 0;
    }
    return KTA_OK;
}

extern "C" int kta_render_retention(const uint64_t *vec, uint32_t n_partitions, uint32_t rows_per_partition, int64_t now_ms, int64_t retention_ms,
                                    int64_t retention_bytes, char *out, size_t out_cap, size_t *out_len)
{
    if (!vec || !out_len) return KTA_ERR_INVALID;
    const std::string text = kta::render_retention(vec, n_partitions, rows_per_partition, now_ms, retention_ms, retention_bytes);
    if (text.empty()) return KTA_ERR_INVALID;   // (kta_retention_whatif refused the arguments)
    *out_len = text.size();
    if (out && out_cap > 0) {
        const size_t n = std::min(out_cap - 1, text.size());
        memcpy(out, text.data(), n);
        out[n] = 0;
    }
    return KTA_OK;
}

extern "C" int kta_render_partitioner(const uint64_t *vec, const uint64_t *counter_vec, uint32_t n_partitions, uint32_t q, char *out,
                                      size_t out_cap, size_t *out_len)
{
    const uint32_t lim = (uint32_t)kta_partitioner_max_partitions();
    if (!vec || !counter_vec || !out_len || n_partitions == 0 || n_partitions > lim || q == 0 || q > lim) return KTA_ERR_INVALID;
    const std::string text = kta::render_partitioner(vec, counter_vec, n_partitions, q);
    *out_len = text.size();
    if (out && out_cap > 0) {
        const size_t n = std::min(out_cap - 1, text.size());
        memcpy(out, text.data(), n);
        out[n] = 0;
    }
    return KTA_OK;
}

extern "C" int kta_render_size_percentiles(const uint64_t *vec, const uint64_t *counter_vec, uint32_t n_partitions, char *out, size_t out_cap,
                                           size_t *out_len)
{
    if (!vec || !counter_vec || !out_len || n_partitions == 0 || (int)n_partitions > kta_size_quantiles_max_partitions()) return KTA_ERR_INVALID;
    // a vector that does not describe the counter vector's records is refused
    if (!kta::size_quantiles_match(vec, counter_vec, n_partitions, KTA_NCOUNTERS, KTA_C_KEY_NON_NULL, KTA_C_ALIVE, KTA_G_RECORDS,
                                   KTA_G_BAD_PARTITION))
        return KTA_ERR_INVALID;
    const std::string text = kta::render_size_percentiles(vec, n_partitions);
    *out_len = text.size();
    if (out && out_cap > 0) {
        const size_t n = std::min(out_cap - 1, text.size());
        memcpy(out, text.data(), n);
        out[n] = 0;
    }
    return KTA_OK;
}

extern "C" int kta_render_record_batches(const uint64_t *vec, uint32_t n_partitions, int filtered, const uint64_t *skipped, char *out,
                                         size_t out_cap, size_t *out_len)
{
    if (!vec || !out_len || n_partitions == 0 || n_partitions > 4096) return KTA_ERR_INVALID;
    static const uint64_t kNone[3] = {0, 0, 0};
    const std::string text = kta::render_record_batches(vec, n_partitions, filtered != 0, skipped ? skipped : kNone);
    *out_len = text.size();
    if (out && out_cap > 0) {
        const size_t n = std::min(out_cap - 1, text.size());
        memcpy(out, text.data(), n);
        out[n] = 0;
    }
    return KTA_OK;
}

extern "C" int kta_render_payload(const uint64_t *vec, const uint64_t *counter_vec, uint32_t n_partitions, char *out, size_t out_cap, size_t *out_len)
{
    if (!vec || !out_len || n_partitions == 0 || n_partitions > 4096) return KTA_ERR_INVALID;
    const std::string text = kta::render_payload(vec, counter_vec, n_partitions);
    *out_len = text.size();
    if (out && out_cap > 0) {
        const size_t n = std::min(out_cap - 1, text.size());
        memcpy(out, text.data(), n);
        out[n] = 0;
    }
    return KTA_OK;
}

extern "C" int kta_render_compaction(const uint64_t *vec, const uint64_t *counter_vec, uint32_t n_partitions, char *out, size_t out_cap,
                                     size_t *out_len)
{
    if (!vec || !counter_vec || !out_len || n_partitions == 0 || (int)n_partitions > kta_compaction_max_partitions()) return KTA_ERR_INVALID;
    bool matched = false;
    const std::string text = kta::render_compaction(vec, counter_vec, n_partitions, &matched);
    *out_len = text.size();
    if (out && out_cap > 0) {
        const size_t n = std::min(out_cap - 1, text.size());
        memcpy(out, text.data(), n);
        out[n] = 0;
    }
    return matched ? KTA_OK : KTA_ERR_INVALID;
}

extern "C" int kta_render_compact_delete(const uint64_t *seg_vec, const uint64_t *kept_vec, const uint64_t *comp_vec, uint32_t n_partitions,
                                         uint32_t rows_per_partition, int64_t now_ms, int64_t retention_ms, int64_t retention_bytes, char *out,
                                         size_t out_cap, size_t *out_len)
{
    if (!out_len) return KTA_ERR_INVALID;
    bool matched = false;
    const std::string text = kta::render_compact_delete(seg_vec, kept_vec, comp_vec, n_partitions, rows_per_partition, now_ms, retention_ms,
                                                        retention_bytes, &matched);
    *out_len = text.size();
    if (text.empty()) return KTA_ERR_INVALID;
    if (out && out_cap > 0) {
        const size_t n = std::min(out_cap - 1, text.size());
        memcpy(out, text.data(), n);
        out[n] = 0;
    }
    return matched ? KTA_OK : KTA_ERR_INVALID;
}

extern "C" int kta_render_filter(int64_t from_ms, int64_t to_ms, const uint32_t *partition_bitmap, uint32_t n_partitions, uint64_t seen,
                                 uint64_t passed, char *out, size_t out_cap, size_t *out_len)
{
    if (!out_len || n_partitions == 0 || from_ms >= to_ms) return KTA_ERR_INVALID;
    const std::string text = kta::render_filter(from_ms, to_ms, partition_bitmap, n_partitions, seen, passed);
    *out_len = text.size();
    if (out && out_cap > 0) {
        const size_t n = std::min(out_cap - 1, text.size());
        memcpy(out, text.data(), n);
        out[n] = 0;
    }
    return KTA_OK;
}

extern "C" int kta_render_distinct_keys(const uint64_t *sketch_vec, const uint64_t *counter_vec, uint32_t n_partitions,
                                        char *out, size_t out_cap, size_t *out_len)
{
    if (!sketch_vec || !counter_vec || !out_len || n_partitions == 0 || n_partitions > KTA_SKETCH_MAX_PARTITIONS)
        return KTA_ERR_INVALID;
    std::vector<uint64_t> keyed(n_partitions);
    for (uint32_t p = 0; p < n_partitions; p++) keyed[p] = counter_vec[(size_t)p * KTA_NCOUNTERS + KTA_C_KEY_NON_NULL];
    int rc = kta_key_sketch_estimate(sketch_vec, n_partitions, nullptr, nullptr);   // (a register above 21: refused)
    if (rc != KTA_OK) return rc;
    const std::string text = kta::render_distinct_keys(sketch_vec, keyed);
    *out_len = text.size();
    if (out && out_cap > 0) {
        const size_t n = std::min(out_cap - 1, text.size());
        memcpy(out, text.data(), n);
        out[n] = 0;
    }
    return KTA_OK;
}

extern "C" int kta_render_timeline(const uint64_t *vec, int64_t origin_ms, int64_t bucket_ms, uint32_t n_buckets,
                                   char *out, size_t out_cap, size_t *out_len)
{
    if (!vec || !out_len || origin_ms < 0 || bucket_ms < 1 || n_buckets < 1 || n_buckets > KTA_TIMELINE_MAX_BUCKETS ||
        bucket_ms > (INT64_MAX - origin_ms) / (int64_t)n_buckets)
        return KTA_ERR_INVALID;
    const std::string text = kta::render_timeline(vec, origin_ms, bucket_ms, n_buckets);
    *out_len = text.size();
    if (out && out_cap > 0) {
        const size_t n = std::min(out_cap - 1, text.size());
        memcpy(out, text.data(), n);
        out[n] = 0;
    }
    return KTA_OK;
}

extern "C" int kta_render_analytics(const uint64_t *vec, uint32_t n_partitions, char *out, size_t out_cap,
                                    size_t *out_len)
{
    if (!vec || !out_len || n_partitions == 0) return KTA_ERR_INVALID;
    kta::Analytics a;
    a.min_ts_sec.resize(n_partitions);
    a.max_ts_sec.resize(n_partitions);
    a.smallest.resize(n_partitions);
    a.largest.resize(n_partitions);
    int rc = kta_decode_analytics(vec, n_partitions, &a.hist, a.min_ts_sec.data(), a.max_ts_sec.data(),
                                  a.smallest.data(), a.largest.data());
    if (rc != KTA_OK) return rc;
    const std::string text = kta::render_analytics(a);
    *out_len = text.size();
    if (out && out_cap > 0) {
        const size_t n = std::min(out_cap - 1, text.size());
        memcpy(out, text.data(), n);
        out[n] = 0;
    }
    return KTA_OK;
}

extern "C" int kta_render_report(const char *topic, uint64_t duration_secs, const uint64_t *vec,
                                 uint32_t n_partitions, int count_alive_keys, int64_t now_sec, uint32_t now_ns,
                                 const int64_t *start_offsets, const int64_t *end_offsets, char *out,
                                 size_t out_cap, size_t *out_len)
{
    if (!topic || !vec || !out_len || n_partitions == 0) return KTA_ERR_INVALID;
    kta_result r;
    std::vector<uint64_t> counters((size_t)n_partitions * KTA_NCOUNTERS);
    int rc = kta_decode_vector(vec, n_partitions, count_alive_keys, &r, counters.data());
    if (rc != KTA_OK && rc != KTA_ERR_BAD_PARTITION) return rc;
    kta::MessageMetrics mm(r, std::move(counters), kta::DateTimeUtc{now_sec, now_ns});
    kta::LogCompactionInMemoryMetrics lc(r);
    std::vector<int32_t> parts(n_partitions);
    std::vector<int64_t> so(n_partitions), eo(n_partitions);
    for (uint32_t p = 0; p < n_partitions; p++) {
        parts[p] = (int32_t)p;
        so[p] = start_offsets ? start_offsets[p] : 0;
        eo[p] = end_offsets ? end_offsets[p] : (int64_t)mm.total((int32_t)p);
    }
    std::string text;
    try {
        text = kta::render_report(topic, duration_secs, mm, count_alive_keys ? &lc : nullptr, parts, so, eo);
    } catch (const kta::RustPanic &) {
        return KTA_ERR_DIV_BY_ZERO;  // the reference panics here (metric.rs:135,144,153)
    }
    *out_len = text.size();
    if (out && out_cap > 0) {
        const size_t n = std::min(out_cap - 1, text.size());
        memcpy(out, text.data(), n);
        out[n] = 0;
    }
    return KTA_OK;
}

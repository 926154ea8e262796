// payload_check.cpp — csrc/kta_payload.h run natively (a program of its own; tests/test_payload_host.py builds it with
// -fsanitize=address,undefined and runs it): the value classes, the header walk on hand-built header sections, on every
// truncation of them and with every varint forced long, the record walk of a batch, the identities and the schema-id
// read-off.  Every buffer is heap memory of the exact size, so a read past a record's end is a sanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "kta_payload.h"

using namespace kta;

static int failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            failures++;                                             \
        }                                                           \
    } while (0)

typedef std::vector<uint8_t> Bytes;

// zig-zag varint; `width` > 0 forces that many bytes (continuation bits over zero groups)
static void put_varint(Bytes &o, long long v, uint32_t width = 0)
{
    unsigned long long z = ((unsigned long long)v << 1) ^ (unsigned long long)(v >> 63);
    uint32_t n = 0;
    do {
        uint8_t b = z & 0x7F;
        z >>= 7;
        n++;
        const bool more = z != 0 || n < width;
        o.push_back(more ? b | 0x80 : b);
        if (!more) break;
    } while (true);
}

struct Header {
    std::string key;
    long long value_len;   // -1: null
};

static Bytes section(const std::vector<Header> &hs, uint32_t width = 0)
{
    Bytes o;
    put_varint(o, (long long)hs.size(), width);
    for (const Header &h : hs) {
        put_varint(o, (long long)h.key.size(), width);
        o.insert(o.end(), h.key.begin(), h.key.end());
        put_varint(o, h.value_len, width);
        for (long long i = 0; i < h.value_len; i++) o.push_back((uint8_t)('a' + i % 26));
    }
    return o;
}

// the walk over an exact-size heap copy of `s`, placed at offset `lead` of the buffer
static PayloadHeaders walk(const Bytes &s, size_t lead = 0)
{
    uint8_t *buf = (uint8_t *)malloc(lead + s.size() ? lead + s.size() : 1);
    memset(buf, 0xEE, lead);
    if (!s.empty()) memcpy(buf + lead, s.data(), s.size());
    PayloadBytes src{buf};
    const PayloadHeaders h = payload_walk_headers(src, lead, lead + s.size());
    free(buf);
    return h;
}

static void check_classes()
{
    CHECK(payload_class(-1, 0) == kPlNull && payload_class(0, 0) == kPlEmpty);
    for (long long len : {1ll, 4ll, 5ll, 1000ll}) {
        CHECK(payload_class(len, 0x00) == (len >= 5 ? kPlFramed : kPlOther));
        CHECK(payload_class(len, '{') == kPlJson && payload_class(len, '[') == kPlJson);
        CHECK(payload_class(len, 'x') == kPlOther && payload_class(len, 0x01) == kPlOther);
    }
    CHECK(payload_schema_id(0x12, 0x34, 0x56, 0x78) == 0x12345678u && payload_schema_id(0xFF, 0xFF, 0xFF, 0xFF) == 0xFFFFFFFFu);
    CHECK(payload_cell(0, 1024 + 7) == 7 && payload_cell(1, 5) == (payload_fmix32(5) & 1023u) && payload_fmix32(0) == 0);
    CHECK(payload_len(3) == 24 * 3 + 16 + 2 * 1024 * 34);
}

static void check_headers()
{
    const std::vector<std::vector<Header>> cases = {
        {}, {{"k", 1}}, {{"", 0}}, {{"trace", -1}}, {{"a", 3}, {"bb", -1}, {"", 40}}, {{std::string(300, 'K'), 200}},
    };
    for (const auto &hs : cases) {
        uint64_t keyb = 0, valb = 0, nulls = 0;
        for (const Header &h : hs) keyb += h.key.size(), valb += h.value_len > 0 ? h.value_len : 0, nulls += h.value_len < 0;
        for (uint32_t width : {0u, 2u, 5u, 10u}) {                       // every varint forced long: still good up to ten bytes
            const Bytes s = section(hs, width);
            for (size_t lead : {0u, 3u}) {
                const PayloadHeaders h = walk(s, lead);
                CHECK(!h.bad && h.count == hs.size() && h.key_bytes == keyb && h.value_bytes == valb && h.null_values == nulls);
            }
            for (size_t cut = 0; cut < s.size(); cut++) {                  // truncated at every byte: bad, and nothing read behind the cut
                const PayloadHeaders h = walk(Bytes(s.begin(), s.begin() + cut));
                CHECK(h.bad && h.count == 0 && h.key_bytes == 0 && h.value_bytes == 0 && h.null_values == 0);
            }
            Bytes longer = s;
            longer.push_back(0);                                           // a byte behind the last header
            CHECK(walk(longer).bad);
        }
        CHECK(walk(section(hs, 11)).bad);                                  // a varint of eleven bytes
    }
    Bytes s;
    put_varint(s, -1);
    CHECK(walk(s).bad);                                                    // negative count
    s.clear(), put_varint(s, 1), put_varint(s, -1);
    CHECK(walk(s).bad);                                                    // negative key length
    s.clear(), put_varint(s, 1), put_varint(s, 1), s.push_back('a'), put_varint(s, -2);
    CHECK(walk(s).bad);                                                    // value length below -1
    s.clear(), put_varint(s, 1), put_varint(s, 0x7FFFFFFFFFFFFFFFll);
    CHECK(walk(s).bad);                                                    // a key length beyond everything
    s.clear(), put_varint(s, 0x7FFFFFFFFFFFFFFFll);
    CHECK(walk(s).bad);                                                    // a count beyond everything: ends at the record's end
    s.assign(10, 0x80), s.push_back(0);
    CHECK(walk(s).bad);
    s.assign(9, 0x80), s.push_back(0);                                     // ten bytes: the count 0
    CHECK(!walk(s).bad && walk(s).count == 0);
    CHECK(walk(Bytes()).bad);                                              // absent
    for (uint64_t n : {0ull, 1ull, 14ull, 15ull, 16ull, 200ull}) CHECK(payload_hist_bin(n) == (n < 15 ? n : 15));
}

static Bytes record(long long ts, const std::string &key, int key_null, const Bytes *value, const Bytes &headers)
{
    Bytes body;
    body.push_back(0);
    put_varint(body, ts), put_varint(body, 0);
    put_varint(body, key_null ? -1 : (long long)key.size());
    body.insert(body.end(), key.begin(), key.end());
    put_varint(body, value ? (long long)value->size() : -1);
    if (value) body.insert(body.end(), value->begin(), value->end());
    body.insert(body.end(), headers.begin(), headers.end());
    Bytes o;
    put_varint(o, (long long)body.size());
    o.insert(o.end(), body.begin(), body.end());
    return o;
}

static void check_batch_and_table()
{
    const uint32_t P = 3;
    std::vector<uint64_t> vec(payload_len(P), 0);
    auto framed = [](uint32_t id, size_t extra) {
        Bytes v{0, (uint8_t)(id >> 24), (uint8_t)(id >> 16), (uint8_t)(id >> 8), (uint8_t)id};
        v.insert(v.end(), extra, 7);
        return v;
    };
    // a, b share a cell of row 0; the pair c, d collides in both rows (searched)
    const uint32_t a = 500, b = 500 + 1024;                                 // (the 300 ids below take the cells 976 .. 1023 and 0 .. 251 of row 0)
    uint32_t c = 600, d = 0;
    for (uint32_t k = 1; !d; k++)
        if (payload_cell(1, c + 1024 * k) == payload_cell(1, c)) d = c + 1024 * k;
    Bytes batch;
    uint64_t n = 0;
    auto add = [&](const Bytes &r) { batch.insert(batch.end(), r.begin(), r.end()), n++; };
    const Bytes none = section({}), two = section({{"x", 2}, {"yy", -1}}), json{'{', '}'}, other{'h', 'i'}, empty;
    for (uint32_t i = 0; i < 300; i++) { const Bytes v = framed(2000 + i, i % 5); add(record(i, "k", 0, &v, none)); }
    for (uint32_t id : {a, a, b, c, d, d}) { const Bytes v = framed(id, 3); add(record(1, "", 1, &v, two)); }
    add(record(2, "k", 0, nullptr, two));
    add(record(3, "k", 0, &empty, none));
    add(record(4, "k", 0, &json, none));
    add(record(5, "k", 0, &other, Bytes()));                                // headers absent: bad
    const uint64_t good = n;
    Bytes broken = record(6, "k", 0, &other, none);
    broken[0] = (uint8_t)(broken[0] + 40);                                  // a length that overruns the batch: the walk ends here
    add(broken);
    add(record(7, "k", 0, &other, none));
    uint8_t *heap = (uint8_t *)malloc(batch.size());
    memcpy(heap, batch.data(), batch.size());
    payload_batch_host(vec.data(), P, 1, heap, 0, batch.size(), n, [](long long) { return true; });
    const uint64_t *w = vec.data() + kPlPartitionWords;
    CHECK(w[kPlRecords] == good && w[kPlClass + kPlFramed] == 306 && w[kPlClass + kPlNull] == 1 && w[kPlClass + kPlEmpty] == 1);
    CHECK(w[kPlClass + kPlJson] == 1 && w[kPlClass + kPlOther] == 1 && w[kPlBadHeaders] == 1 && w[kPlWithHeaders] == 7 && w[kPlHeaders] == 14);
    CHECK(w[kPlHeaderNullValues] == 7 && w[kPlHeaderKeyBytes] == 21 && w[kPlHeaderValueBytes] == 14);
    CHECK(vec[payload_hist_at(P) + 0] == good - 8 && vec[payload_hist_at(P) + 2] == 7);
    CHECK(payload_identities_hold(vec.data(), P));
    // a filter that drops every second record halves nothing it should not
    std::vector<uint64_t> half(payload_len(P), 0);
    payload_batch_host(half.data(), P, 0, heap, 0, batch.size(), n, [](long long ts) { return ts % 2 == 0; });
    CHECK(half[kPlRecords] == 150 + 1 + 1 && payload_identities_hold(half.data(), P));
    // truncated at every byte: never a read behind the cut, the identities always hold
    for (size_t cut = 0; cut < batch.size(); cut += 7) {
        uint8_t *part = (uint8_t *)malloc(cut ? cut : 1);
        memcpy(part, batch.data(), cut);
        std::vector<uint64_t> v2(payload_len(P), 0);
        payload_batch_host(v2.data(), P, 2, part, 0, cut, n, [](long long) { return true; });
        CHECK(payload_identities_hold(v2.data(), P) && v2[2 * kPlPartitionWords + kPlRecords] <= good);
        free(part);
    }
    free(heap);

    uint64_t ur = 0, ub = 0;
    const std::vector<PayloadSchemaId> ids = payload_schema_ids(vec.data(), P, &ur, &ub);
    CHECK(ids.size() == 302);                                               // 300 consecutive + a and b (peeled through row 1); c, d stay
    CHECK(ur == 3 && ub == 3 * 8);
    bool has_a = false, has_b = false, has_cd = false;
    for (const PayloadSchemaId &e : ids) {
        has_a |= e.id == a && e.records == 2 && e.bytes == 16;
        has_b |= e.id == b && e.records == 1 && e.bytes == 8;
        has_cd |= e.id == c || e.id == d;
    }
    CHECK(has_a && has_b && !has_cd && ids[0].id == a);
    // every identity breaks by one flipped word
    for (size_t at : {(size_t)kPlPartitionWords + kPlRecords, (size_t)kPlPartitionWords + kPlClassBytes + kPlNull, (size_t)kPlPartitionWords + 20,
                      payload_hist_at(P) + 0, payload_hist_at(P) + 3, payload_cell_at(P, 0, a) + kPlCellT, payload_cell_at(P, 1, 9) + kPlCellBits + 4}) {
        std::vector<uint64_t> v2 = vec;
        v2[at] += 1000;
        CHECK(!payload_identities_hold(v2.data(), P));
    }
    // a cell whose bit counts spell an id of another cell is not pure
    std::vector<uint64_t> v3(payload_len(P), 0);
    uint64_t *cell = v3.data() + payload_cell_at(P, 0, 9);
    cell[kPlCellT] = 4, cell[kPlCellB] = 40, cell[kPlCellBits + 1] = 4;      // spells id 2, which belongs to cell 2
    uint32_t spelled = 0;
    CHECK(!payload_cell_pure(cell, 0, 9, spelled) && spelled == 2);
    CHECK(payload_schema_ids(v3.data(), P, &ur, &ub).empty() && ur == 4 && ub == 40);
}

int main()
{
    check_classes();
    check_headers();
    check_batch_and_table();
    if (failures) return 1;
    printf("OK payload_check\n");
    return 0;
}

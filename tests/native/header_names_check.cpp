// header_names_check.cpp — test infrastructure: csrc/kta_header_names.h (and through it kta_payload.h's peel and walks) driven
// natively with boundary tables, a program of its own so that it can be built with -fsanitize=address,undefined and run
// directly (tests/test_header_names_host.py).  It checks the rule, the peel and the list on: an empty vector, one name, 1024
// names, a pair of names that collides in both rows, and a cell whose L is not a multiple of its T.  (The rendered section
// lives in host/report.cpp, which needs the library: tests/test_header_names_host.py holds it against the restatement on the
// same boundary tables.)  Exit status 0 and "OK" when every check holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "kta_header_names.h"

using namespace kta;

static int failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);        \
            failures++;                                             \
        }                                                           \
    } while (0)

static uint32_t hash_of(const std::string &name)
{
    uint32_t h = kHnFnvInit;
    for (unsigned char c : name) h = hn_fnv_byte(h, c);
    return h;
}

static void add(std::vector<uint64_t> &vec, std::vector<HnSlot> &table, const std::string &name, long long val_len)
{
    hn_add_occurrence(vec.data(), table.data(), reinterpret_cast<const uint8_t *>(name.data()), name.size(), val_len);
}

int main()
{
    // empty
    {
        std::vector<uint64_t> vec(kHnWords, 0);
        std::vector<HnSlot> table(kHnSlots, HnSlot{});
        uint64_t uo = 7, uv = 7;
        CHECK(hn_list(vec.data(), table.data(), &uo, &uv).empty() && uo == 0 && uv == 0);
        CHECK(hn_list(vec.data(), nullptr, nullptr, nullptr).empty());
        CHECK(hn_identities_hold(vec.data()));
    }
    // one name: an empty one with a null value, then values
    {
        std::vector<uint64_t> vec(kHnWords, 0);
        std::vector<HnSlot> table(kHnSlots, HnSlot{});
        add(vec, table, "", -1), add(vec, table, "", 5), add(vec, table, "", 0);
        uint64_t uo = 7, uv = 7;
        const std::vector<HnListed> l = hn_list(vec.data(), table.data(), &uo, &uv);
        CHECK(l.size() == 1 && l[0].hash == kHnFnvInit && l[0].occurrences == 3 && l[0].name_len == 0 && l[0].value_bytes == 5 && l[0].null_values == 1);
        CHECK(l.size() == 1 && l[0].name && l[0].name->name_len == 0 && uo == 0 && uv == 0);
        CHECK(hn_identities_hold(vec.data()) && vec[kHnOccurrences] == 3 && vec[kHnNullValues] == 1);
        CHECK(hn_list(vec.data(), nullptr, nullptr, nullptr).size() == 1 && hn_list(vec.data(), nullptr, nullptr, nullptr)[0].name == nullptr);
    }
    // 1024 names (a 300-byte one among them): whatever is listed is exact, and listed + remainder == everything
    {
        std::vector<uint64_t> vec(kHnWords, 0);
        std::vector<HnSlot> table(kHnSlots, HnSlot{});
        std::vector<std::string> names;
        for (int i = 0; i < 1023; i++) names.push_back("header-" + std::to_string(i));
        names.push_back(std::string(300, 'k'));
        for (size_t i = 0; i < names.size(); i++)
            for (size_t k = 0; k <= i % 3; k++) add(vec, table, names[i], (long long)(i % 5) - 1);
        uint64_t uo = 0, uv = 0;
        const std::vector<HnListed> l = hn_list(vec.data(), table.data(), &uo, &uv);
        uint64_t occ = uo, vb = uv;
        for (const HnListed &n : l) {
            occ += n.occurrences, vb += n.value_bytes;
            size_t i = 0;
            while (i < names.size() && hash_of(names[i]) != n.hash) i++;
            CHECK(i < names.size());
            if (i == names.size()) continue;
            CHECK(n.occurrences == i % 3 + 1 && n.name_len == names[i].size());
            CHECK(n.value_bytes == (i % 5 > 1 ? (i % 5 - 1) * (i % 3 + 1) : 0) && n.null_values == (i % 5 == 0 ? i % 3 + 1 : 0));
            if (n.name) CHECK(n.name->hash == n.hash && n.name->name_len == names[i].size() &&
                              !memcmp(n.name->bytes, names[i].data(), std::min<size_t>(names[i].size(), kHnExemplarBytes)));
        }
        CHECK(occ == vec[kHnOccurrences] && vb == vec[kHnValueBytes] && l.size() > 512 && hn_identities_hold(vec.data()));
        for (size_t i = 1; i < l.size(); i++) CHECK(l[i - 1].occurrences >= l[i].occurrences);
    }
    // two names that share both cells: neither is listed, the remainder is their sums; a third name is
    {
        std::vector<std::string> pair;
        std::vector<std::pair<uint32_t, std::string>> seen;
        for (int i = 0; pair.empty() && i < 400000; i++) {
            const std::string name = "n" + std::to_string(i);
            const uint32_t h = hash_of(name), key = payload_cell(0, h) << 10 | payload_cell(1, h);
            for (const auto &s : seen)
                if (s.first == key && hash_of(s.second) != h) pair = {s.second, name};
            seen.emplace_back(key, name);
            if (seen.size() > 4000) seen.erase(seen.begin(), seen.begin() + 1);   // (a window of candidates keeps the search linear enough)
        }
        CHECK(pair.size() == 2);
        if (pair.size() == 2) {
            std::vector<uint64_t> vec(kHnWords, 0);
            std::vector<HnSlot> table(kHnSlots, HnSlot{});
            for (int k = 0; k < 5; k++) add(vec, table, pair[0], 3), add(vec, table, pair[1], 4);
            add(vec, table, "third", 9);
            uint64_t uo = 0, uv = 0;
            const std::vector<HnListed> l = hn_list(vec.data(), table.data(), &uo, &uv);
            CHECK(l.size() == 1 && l[0].hash == hash_of("third") && uo == 10 && uv == 35);
        }
    }
    // an inconsistent L: a cell that spells one hash but whose name bytes are no multiple of its occurrences is not pure
    {
        std::vector<uint64_t> vec(kHnWords, 0);
        std::vector<HnSlot> table(kHnSlots, HnSlot{});
        add(vec, table, "abc", 2), add(vec, table, "abc", 2);
        CHECK(hn_list(vec.data(), table.data(), nullptr, nullptr).size() == 1);
        const uint32_t h = hash_of("abc");
        for (uint32_t r = 0; r < kPlRows; r++) vec[hn_cell_at(r, payload_cell(r, h)) + kHnCellL] += 1;   // 7 name bytes in 2 occurrences
        uint64_t uo = 0, uv = 0;
        CHECK(hn_list(vec.data(), table.data(), &uo, &uv).empty() && uo == 2 && uv == 4);
        CHECK(!hn_identities_hold(vec.data()));                                    // (and the rows no longer sum to the globals)
    }
    // the host walk: a record section with a good and a bad header section
    {
        const uint8_t recs[] = {// record 0: length 10; attributes, tsDelta, offsetDelta, key -1, value length 0, 1 header "a" -> "b"
                                20, 0, 0, 0, 1, 0, 2, 2, 'a', 2, 'b',
                                // record 1: length 7; ... headers: count 1, key length 5 overruns
                                14, 0, 0, 2, 1, 0, 2, 10};
        std::vector<uint64_t> vec(kHnWords, 0);
        std::vector<HnSlot> table(kHnSlots, HnSlot{});
        hn_batch_host(vec.data(), table.data(), recs, 0, sizeof recs, 2, [](long long) { return true; });
        CHECK(vec[kHnLooked] == 1 && vec[kHnOccurrences] == 1 && vec[kHnNameBytes] == 1 && vec[kHnValueBytes] == 1 && vec[kHnWithHeaders] == 1);
    }
    if (failures) return 1;
    printf("OK\n");
    return 0;
}

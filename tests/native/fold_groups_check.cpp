// csrc/kta_fold_groups.h on the CPU (tests/test_fold_groups_host.py builds this once per candidate group size, with
// -DKTA_FOLD_GROUP_ROWS=G, and once with the header's own): for every number of rows from 1 to 4096 every row lies in
// exactly one group, the one fold_group_of names; the groups are consecutive, their sizes sum to the rows, every group
// but the last is full and the last has the remainder.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "kta_fold_groups.h"

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            fprintf(stderr, "fold_groups_check: %s failed at line %d (rows %u)\n", #cond, __LINE__, rows); \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

int main()
{
    const uint32_t G = kta::kFoldGroupRows;
    for (uint32_t rows = 1; rows <= 4096; rows++) {
        const uint32_t groups = kta::fold_groups(rows);
        CHECK(groups >= 1 && (uint64_t)(groups - 1) * G < rows && (uint64_t)groups * G >= rows);
        std::vector<uint32_t> seen(rows, 0);
        uint32_t sum = 0, next = 0;
        for (uint32_t g = 0; g < groups; g++) {
            uint32_t r0 = ~0u, r1 = ~0u;
            kta::fold_group_rows(g, rows, r0, r1);
            CHECK(r0 == next && r0 < r1 && r1 <= rows);
            const uint32_t want = g + 1 < groups ? G : rows - (groups - 1) * G;   // the last group: what is left, 1 .. G
            CHECK(r1 - r0 == want && want >= 1 && want <= G);
            for (uint32_t r = r0; r < r1; r++) {
                CHECK(kta::fold_group_of(r) == g);
                seen[r]++;
            }
            sum += r1 - r0;
            next = r1;
        }
        CHECK(sum == rows && next == rows);
        for (uint32_t r = 0; r < rows; r++) CHECK(seen[r] == 1);
    }
    printf("fold_groups_check OK (group rows %u)\n", G);
    return 0;
}

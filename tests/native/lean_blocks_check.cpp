// csrc/kta_lean_blocks.h on the CPU: the block rule of the lean scan kernel — 64 steps at a time, from two ballots —
// against a step-by-step restatement of the rule the kernel had before: walk the workgroup's steps in order; a step
// that is neither a plane tile nor a lean tile goes on the list while the list has room, and the first one that does
// not fit is handed over with everything behind it.  Compared: the taken plane and lean steps, the list words, the
// handover and the end.  Built with AddressSanitizer + UBSan by tests/test_lean_blocks_host.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "kta_lean_blocks.h"

using namespace kta;

namespace {

constexpr uint32_t kListed = 4;   // kta_kernels.hip: kLeanListed
enum Class : uint8_t { OTHER = 0, PLANE = 1, LEAN = 2 };

struct Outcome {
    std::vector<uint8_t> taken;   // per step: PLANE, LEAN or 0
    uint64_t list_a = 0, list_b = 0;
    uint32_t handover = 0, end = 0;
};

int failures = 0;
#define CHECK(cond, ...)                                                                                                  \
    do {                                                                                                                  \
        if (!(cond)) {                                                                                                    \
            printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond);                                                        \
            printf(__VA_ARGS__);                                                                                          \
            printf("\n");                                                                                                 \
            if (++failures > 20) exit(1);                                                                                 \
        }                                                                                                                 \
    } while (0)

Outcome naive(const std::vector<uint8_t> &cls)
{
    Outcome o;
    o.taken.assign(cls.size(), 0);
    o.end = (uint32_t)cls.size();
    uint32_t listed = 0;
    for (uint32_t s = 0; s < cls.size(); s++) {
        if (cls[s] != OTHER) {
            o.taken[s] = cls[s];
            continue;
        }
        if (listed == kListed) {
            o.handover = s + 1u;
            o.end = s;
            break;
        }
        const uint64_t e = (uint64_t)(s + 1u) << (32u * (listed & 1u));
        if (listed < 2) o.list_a |= e;
        else o.list_b |= e;
        listed++;
    }
    return o;
}

// The kernel's drive: a block's ballots hold one vote per lane, and a lane past the end votes on a clamped tile —
// here: whatever `junk` says, both masks at once included.
Outcome blocks(const std::vector<uint8_t> &cls, uint64_t junk)
{
    Outcome o;
    o.taken.assign(cls.size(), 0);
    LeanBlocks st;
    st.end = (uint32_t)cls.size();
    for (uint32_t base = 0; base < st.end; base += kLeanBlockSteps) {
        uint64_t plane = 0, lean = 0;
        for (uint32_t l = 0; l < kLeanBlockSteps; l++) {
            const uint64_t step = (uint64_t)base + l;
            if (step < cls.size()) {
                plane |= (uint64_t)(cls[step] == PLANE) << l;
                lean |= (uint64_t)(cls[step] == LEAN) << l;
            } else {
                plane |= ((junk >> (l & 31u)) & 1ull) << l;
                lean |= ((junk >> (32u + (l & 31u))) & 1ull) << l;
            }
        }
        const uint32_t end_before = st.end;
        lean_block(st, base, kListed, plane, lean);
        CHECK((plane & lean) == 0, "a step in both masks, base %u", base);
        CHECK(st.end <= end_before, "the end grew");
        for (uint32_t l = 0; l < kLeanBlockSteps; l++) {
            const uint8_t t = (plane >> l) & 1 ? PLANE : (lean >> l) & 1 ? LEAN : 0;
            if ((uint64_t)base + l < cls.size()) o.taken[base + l] = t;
            else CHECK(t == 0, "a step past the end is taken: base %u lane %u", base, l);
        }
    }
    o.list_a = st.list_a, o.list_b = st.list_b, o.handover = st.handover, o.end = st.end;
    return o;
}

uint64_t cases = 0;
void compare(const std::vector<uint8_t> &cls, const char *what)
{
    const Outcome a = naive(cls);
    for (uint64_t junk : {0ull, ~0ull, 0x5A5A5A5AA5A5A5A5ull}) {
        const Outcome b = blocks(cls, junk);
        CHECK(a.taken == b.taken, "%s: taken steps differ (%zu steps)", what, cls.size());
        CHECK(a.list_a == b.list_a && a.list_b == b.list_b, "%s: list %llx %llx, expected %llx %llx", what, (unsigned long long)b.list_a,
              (unsigned long long)b.list_b, (unsigned long long)a.list_a, (unsigned long long)a.list_b);
        CHECK(a.handover == b.handover && a.end == b.end, "%s: handover %u end %u, expected %u %u", what, b.handover, b.end, a.handover, a.end);
    }
    cases++;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

std::vector<uint8_t> filled(uint32_t steps, int form)   // form 0: all plane, 1: all lean, 2: alternating, 3: switching at 64
{
    std::vector<uint8_t> c(steps);
    for (uint32_t s = 0; s < steps; s++) c[s] = form == 0 ? PLANE : form == 1 ? LEAN : form == 2 ? (s & 1 ? LEAN : PLANE) : (s < 64 ? PLANE : LEAN);
    return c;
}

}   // namespace

int main()
{
    // Exhaustive: others among steps 62..66 and among 126..130, behind 0..6 earlier others.
    for (int form = 0; form < 4; form++)
        for (uint32_t before = 0; before <= 6; before++)
            for (uint32_t m1 = 0; m1 < 32; m1++)
                for (uint32_t m2 = 0; m2 < 32; m2++) {
                    std::vector<uint8_t> c = filled(140, form);
                    for (uint32_t i = 0; i < before; i++) c[3 + 9 * i] = OTHER;   // steps 3 .. 48
                    for (uint32_t j = 0; j < 5; j++) {
                        if ((m1 >> j) & 1) c[62 + j] = OTHER;
                        if ((m2 >> j) & 1) c[126 + j] = OTHER;
                    }
                    compare(c, "exhaustive");
                }
    // An end inside a block, at a block's last and first step; with and without others at the edge.
    for (uint32_t steps : {1u, 2u, 37u, 63u, 64u, 65u, 100u, 127u, 128u, 129u, 191u, 192u, 193u})
        for (int form = 0; form < 4; form++) {
            std::vector<uint8_t> c = filled(steps, form);
            compare(c, "end");
            c[steps - 1] = OTHER;
            compare(c, "end, other last");
            for (uint32_t s = 0; s < steps && s < 5; s++) c[s] = OTHER;
            compare(c, "end, five others first");
            for (uint32_t s = 0; s < steps; s++) c[s] = OTHER;
            compare(c, "end, all others");
        }
    // Random patterns of 1 to 300 steps, others from rare to frequent.
    for (uint32_t it = 0; it < 20000; it++) {
        const uint32_t steps = 1u + rnd() % 300u, rate = 1u + rnd() % 64u;
        std::vector<uint8_t> c(steps);
        for (auto &x : c) x = rnd() % rate == 0 ? OTHER : (rnd() & 1 ? PLANE : LEAN);
        compare(c, "random");
    }
    // A workgroup's steps: the first tile past the end gives none; otherwise as counted one by one.
    CHECK(lean_steps(8, 8, 3) == 0 && lean_steps(3, 8, 3) == 0 && lean_steps(2, 8, 3) == 1 && lean_steps(0, 8, 1) == 1, "lean_steps at the end");
    for (uint32_t grid = 1; grid <= 9; grid++)
        for (uint64_t ntiles = 0; ntiles <= 200; ntiles++)
            for (uint32_t wg = 0; wg < grid; wg++) {
                uint32_t nsteps = 0;
                for (uint64_t t = wg; t < ntiles; t += grid) nsteps++;
                CHECK(lean_steps(wg, grid, ntiles) == nsteps, "lean_steps(%u, %u, %llu)", wg, grid, (unsigned long long)ntiles);
            }
    {   // a workgroup without a step opens no block: nothing taken, nothing listed
        const Outcome b = blocks(std::vector<uint8_t>(), ~0ull);
        CHECK(b.end == 0 && b.handover == 0 && b.list_a == 0 && b.list_b == 0, "an empty workgroup");
    }
    // 2^31 - 1 tiles on one workgroup: the last block, an other at the very last step and a full list before it.
    {
        const uint32_t steps = 0x7FFFFFFFu;
        CHECK(lean_steps(0, 1, steps) == steps, "2^31 - 1 steps");
        LeanBlocks st;
        st.end = steps;
        st.listed = kListed;
        const uint32_t base = steps / kLeanBlockSteps * kLeanBlockSteps;
        uint64_t plane = ~0ull >> 2, lean = 0;   // lanes 0..61 plane, step base + 62 = steps - 1 an other, lane 63 past the end
        lean_block(st, base, kListed, plane, lean);
        CHECK(st.handover == steps && st.end == steps - 1u && plane == ~0ull >> 2 && lean == 0, "the last block of 2^31 - 1 steps");
        LeanBlocks s2;
        s2.end = steps;
        plane = ~0ull, lean = 0;
        lean_block(s2, base, kListed, plane, lean);
        CHECK(s2.handover == 0 && s2.end == steps && plane == ~0ull >> 1, "the last block, all plane");
    }
    if (failures) {
        printf("lean_blocks_check: %d failure(s)\n", failures);
        return 1;
    }
    printf("lean_blocks_check OK (%llu patterns)\n", (unsigned long long)cases);
    return 0;
}

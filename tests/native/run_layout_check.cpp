// run_layout_check.cpp -- gx_pr_runs.h on the host (tests/test_pr_runs.py builds it with
// -fsanitize=address,undefined and runs it): random lists of run lengths laid out by the
// RunCursor that k_run_emit walks its entries with (place an entry, end a run), each code stored
// at run_slot(position).  Checks that every entry gets a distinct code position inside
// its own run's groups, that the padding after a run is exactly its round-up to a whole group,
// and that no position or slot passes the region's end.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "gx_pr_runs.h"

using namespace gx;

static int fail(const char *what, int t, uint64_t a, uint64_t b) {
    std::printf("FAIL trial %d: %s (%llu, %llu)\n", t, what, (unsigned long long)a, (unsigned long long)b);
    return 1;
}

int main() {
    std::mt19937_64 rng(12345);
    for (int t = 0; t < 2000; t++) {
        // lengths around the group size, a few long runs, a few of one entry
        const int nruns = 1 + (int)(rng() % 40);
        std::vector<uint64_t> len(nruns);
        for (auto &l : len) {
            switch (rng() % 4) {
                case 0: l = 1 + rng() % 3; break;
                case 1: l = kRunGroup * (1 + rng() % 4) + (rng() % 3) - 1; break;
                case 2: l = 1 + rng() % 200; break;
                default: l = 1 + rng() % 3000; break;
            }
        }
        // the region's end may cut the last run (the prefix R is counted in supergroups of entries)
        uint64_t entries = 0;
        for (uint64_t l : len) entries += l;
        if (t % 3 == 0 && len.back() > 1) {
            const uint64_t cut = 1 + rng() % (len.back() - 1);
            len.back() -= cut;
            entries -= cut;
        }
        uint64_t e = 0;
        RunCursor cur{0};
        // the region's size as the plan computes it: the position just past the last entry, rounded
        uint64_t pad_all = 0;
        for (uint64_t l : len) pad_all += run_pad(l);
        uint64_t last_pad_before = pad_all - run_pad(len.back());
        const uint64_t codes = run_region_codes(run_code_pos(entries, last_pad_before));
        if (codes != entries + pad_all) return fail("region codes", t, codes, entries + pad_all);
        const uint64_t stored = (codes + kRunSg - 1) / kRunSg * kRunSg;
        std::vector<uint8_t> pos_used(codes, 0), slot_used(stored, 0);
        for (uint64_t l : len) {
            const uint64_t start = cur.place(e);
            if (start % kRunGroup) return fail("a run starts inside a group", t, start, l);
            const uint64_t pad = run_pad(l);
            if (pad >= (uint64_t)kRunGroup || (l + pad) % kRunGroup) return fail("padding is not the round-up", t, l, pad);
            if (l + pad != (l + kRunGroup - 1) / kRunGroup * kRunGroup) return fail("padding is not the round-up", t, l, pad);
            for (uint64_t k = 0; k < l; k++, e++) {
                const uint64_t pos = cur.place(e);
                if (pos >= codes) return fail("position past the region", t, pos, codes);
                if (pos != start + k) return fail("position not in sorted order", t, pos, start + k);
                if (run_group_of(pos) < run_group_of(start) || run_group_of(pos) >= run_group_of(start + l + pad))
                    return fail("position outside its run's groups", t, pos, start);
                if (pos_used[pos]++) return fail("position taken twice", t, pos, 0);
                const uint64_t s = run_slot(pos);
                if (s >= stored) return fail("slot past the region", t, s, stored);
                if (s / kRunSg != pos / kRunSg) return fail("slot outside its supergroup", t, s, pos);
                // lane-major: the code of group k of the supergroup, lane l, at l * 8 + k
                if (s % kRunSg != (pos % kRunGroup) * kRunSgGroups + (pos % kRunSg) / kRunGroup)
                    return fail("slot is not lane-major", t, s, pos);
                if (slot_used[s]++) return fail("slot taken twice", t, s, 0);
            }
            cur.end_run(l);
        }
        if (e != entries) return fail("entries", t, e, entries);
        // after the last run the cursor stands at the region's end
        if (cur.place(e) != codes) return fail("the cursor does not end at the region's end", t, cur.place(e), codes);
    }
    std::printf("ok\n");
    return 0;
}

// Host check of the bank-aware deal inside a column run (csrc/gx_pr_bank.h), built and run by
// tests/test_pr_bank_order.py.  For hand-made runs: the deal is a bijection, it orders the
// entries by (rank in class, class), every window of 16 dealt entries holds 16 distinct classes
// while every class still has entries left, and the tail of uneven counts holds each remaining
// class once per round.  The pair form sends the first half of the deal to the even positions.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gx_pr_bank.h"

using gx::bank_deal_pos;
using gx::bank_pair_pos;
using gx::kBankClasses;

static int fails = 0;
#define EXPECT(c)                                                   \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAIL line %d: %s\n", __LINE__, #c);        \
            fails++;                                                \
        }                                                           \
    } while (0)

// The dealt order of a run given by its rows: out[pos] = index of the entry placed there.
static std::vector<int> deal(const std::vector<int> &rows) {
    uint32_t cnt[kBankClasses] = {};
    for (int r : rows) cnt[r & 15]++;
    uint32_t seen[kBankClasses] = {};
    std::vector<int> out(rows.size(), -1);
    for (size_t i = 0; i < rows.size(); i++) {
        const uint32_t b = (uint32_t)rows[i] & 15u, t = seen[b]++;
        const uint32_t pos = bank_deal_pos(cnt, b, t);
        EXPECT(pos < rows.size());
        if (pos < rows.size()) {
            EXPECT(out[pos] == -1);   // a bijection
            out[pos] = (int)i;
        }
    }
    for (int v : out) EXPECT(v >= 0);
    return out;
}

static void check_run(const std::vector<int> &rows) {
    const std::vector<int> out = deal(rows);
    uint32_t cnt[kBankClasses] = {};
    for (int r : rows) cnt[r & 15]++;
    uint32_t mincnt = ~0u;
    for (uint32_t c : cnt) mincnt = c < mincnt ? c : mincnt;
    // rounds: round t holds every class with more than t entries once, in class order
    size_t pos = 0;
    for (uint32_t t = 0; pos < out.size(); t++) {
        for (uint32_t b = 0; b < (uint32_t)kBankClasses; b++) {
            if (cnt[b] <= t) continue;
            EXPECT(pos < out.size() && (uint32_t)(rows[out[pos]] & 15) == b);
            pos++;
        }
    }
    // entries of one class keep their order (ascending rows stay ascending inside a class)
    int last[kBankClasses];
    for (int &v : last) v = -1;
    for (int i : out) {
        EXPECT(i > last[rows[i] & 15]);
        last[rows[i] & 15] = i;
    }
    // while all 16 classes have entries left, any 16 consecutive dealt entries are distinct
    const size_t full = (size_t)mincnt * kBankClasses;
    for (size_t w = 0; w + 16 <= full; w++) {
        uint32_t mask = 0;
        for (size_t j = w; j < w + 16; j++) mask |= 1u << (rows[out[j]] & 15);
        EXPECT(mask == 0xffffu);
    }
}

int main() {
    // 64 consecutive rows: four of every class
    std::vector<int> rows;
    for (int r = 0; r < 64; r++) rows.push_back(r);
    check_run(rows);
    const std::vector<int> d = deal(rows);
    for (int k = 0; k < 64; k++) EXPECT(d[k] == (k & 15) + 16 * (k >> 4) || d[k] == k);   // consecutive rows: already dealt
    // every row in one class: nothing to spread, the order stays
    rows.clear();
    for (int r = 0; r < 40; r++) rows.push_back(16 * r);
    check_run(rows);
    const std::vector<int> same = deal(rows);
    for (int k = 0; k < 40; k++) EXPECT(same[k] == k);
    // ascending rows with runs of one class next to each other: 0,16,32,48, 1,17,33,49, ...
    rows.clear();
    for (int b = 0; b < 16; b++)
        for (int q = 0; q < 4; q++) rows.push_back(b + 16 * q);
    check_run(rows);
    // uneven counts: class 3 nine times, class 5 twice, class 9 once; the tail is class 3 alone
    rows = {3, 19, 35, 5, 51, 9, 67, 83, 21, 99, 115, 131};
    check_run(rows);
    const std::vector<int> un = deal(rows);
    const int want[12] = {0, 3, 5, 1, 8, 2, 4, 6, 7, 9, 10, 11};   // rounds: {3,5,9}, {3,5}, {3}, ...
    for (int k = 0; k < 12; k++) EXPECT(un[k] == want[k]);
    // lengths 1 .. 15 and a pseudo-random long run
    for (int n = 1; n <= 15; n++) {
        rows.clear();
        for (int i = 0; i < n; i++) rows.push_back((7 * i * i + 3 * i) % 61);
        check_run(rows);
    }
    rows.clear();
    uint32_t s = 12345;
    for (int i = 0; i < 64; i++) {
        s = s * 1664525u + 1013904223u;
        rows.push_back((int)(s >> 18));
    }
    check_run(rows);
    // the pair form: a bijection of [0, n), first half of the deal on the even positions in order
    for (uint32_t n = 1; n <= 64; n++) {
        std::vector<int> hit(n, 0);
        const uint32_t h = (n + 1) / 2;
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t p = bank_pair_pos(k, n);
            EXPECT(p < n);
            if (p < n) hit[p]++;
            EXPECT(k < h ? p == 2 * k : p == 2 * (k - h) + 1);
        }
        for (int v : hit) EXPECT(v == 1);
    }
    if (fails) return 1;
    std::printf("bank order ok\n");
    return 0;
}

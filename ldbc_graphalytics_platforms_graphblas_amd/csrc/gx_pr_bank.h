// gx_pr_bank.h -- the bank-aware order inside a column run of a sorted block (GX_PR_BANK_ORDER,
// k_bank_order in gx_pr_plan.hip).  Plain C++ so that a host test can call it.
//
// A 64-bit LDS add is served in groups of 16 consecutive lanes, and two rows of one group
// collide when they are equal mod 16 (their bank slot class).  The entries of one
// column (or column pair) gather the same x, so their order is free: they are dealt round-robin
// over their 16 classes, round t taking one entry of every class that still has more than t.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GX_BANK_HD __host__ __device__ __forceinline__
#else
#define GX_BANK_HD inline
#endif

namespace gx {

constexpr int kBankClasses = 16;

// Position, in the dealt run, of the entry of class b that has t entries of its class before it,
// when class k holds cnt[k] entries: the entries ordered by (t, b).
GX_BANK_HD uint32_t bank_deal_pos(const uint32_t (&cnt)[kBankClasses], uint32_t b, uint32_t t) {
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kBankClasses; k++) pos += (cnt[k] < t ? cnt[k] : t) + ((k < b && cnt[k] > t) ? 1u : 0u);
    return pos;
}

// A run of n entries in the pair prefix: a slot's first half comes from the even positions and
// its second half from the odd ones, and one add instruction takes the same half of consecutive
// slots.  Dealt entry k of n therefore goes to the k-th even position, or past the ceil(n / 2)
// even ones to the odd positions, so that each half sees a contiguous piece of the deal.
GX_BANK_HD uint32_t bank_pair_pos(uint32_t k, uint32_t n) {
    const uint32_t h = (n + 1) / 2;
    return k < h ? 2 * k : 2 * (k - h) + 1;
}

}  // namespace gx

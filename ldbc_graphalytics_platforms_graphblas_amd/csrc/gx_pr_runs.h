// gx_pr_runs.h -- the layout arithmetic of the run region of a sorted block (GX_PR_RUNS; k_run_cost,
// k_run_emit in gx_pr_plan.hip, gather_runs in gx_pr_sorted.hip).  Plain C++ so that a host test can call it.
//
// The region holds the block's first column-sorted entries, one 2-byte code each.  The entries of
// one column pair (columns 2p and 2p + 1) are consecutive, a run; a run's codes start on a group
// of kRunGroup codes and its last group is padded, so every group names one pair.  Eight groups
// make a supergroup of kRunSg codes, stored lane-major like a narrow supergroup: lane l of a wave
// holds codes l + 64 k, so the wave's instruction k is group k.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GX_RUN_HD __host__ __device__ __forceinline__
#else
#define GX_RUN_HD inline
#endif

namespace gx {

constexpr int kRunGroup = 64;                       // codes of a group: one per lane
constexpr int kRunSg = 512;                         // codes of a supergroup: one 16-B load per lane
constexpr int kRunSgGroups = kRunSg / kRunGroup;    // groups (header words) of a supergroup

// Padding codes after a run of len entries.
GX_RUN_HD uint32_t run_pad(uint64_t len) { return (uint32_t)((0 - len) & (uint64_t)(kRunGroup - 1)); }

// Code position, inside the region, of the entry at sorted position e of the region when the runs
// that end before e were followed by pad_before padding codes in all: the codes keep the sorted
// order, so the entry moves back by exactly that padding.
GX_RUN_HD uint64_t run_code_pos(uint64_t e, uint64_t pad_before) { return e + pad_before; }

// Where the entries go, walking the region's sorted entries in order: place(e) is the code
// position of the entry at sorted position e, and end_run(len) follows the last entry of a run
// of len entries (a run cut by the region's end included), whose padding every later entry
// then moves back by.  k_run_emit walks a lane's entries with it, starting from the padding
// before the lane's first entry; k_run_cost sums the same run_pad per supergroup.
struct RunCursor {
    uint64_t pad;   // padding codes of the runs that ended before the next entry
    GX_RUN_HD uint64_t place(uint64_t e) const { return run_code_pos(e, pad); }
    GX_RUN_HD void end_run(uint64_t len) { pad += run_pad(len); }
};

// The group (header word) of a code position.
GX_RUN_HD uint64_t run_group_of(uint64_t pos) { return pos / kRunGroup; }

// Where the code at position pos is stored: lane-major inside its supergroup.
GX_RUN_HD uint64_t run_slot(uint64_t pos) {
    return (pos & ~(uint64_t)(kRunSg - 1)) + (pos & (uint64_t)(kRunGroup - 1)) * kRunSgGroups +
           ((pos / kRunGroup) & (uint64_t)(kRunSgGroups - 1));
}

// Codes of a region given the code position that an entry just past its last one would take: the
// last run, cut there or not, is padded to a whole group like every other.
GX_RUN_HD uint64_t run_region_codes(uint64_t end_pos) { return (end_pos + kRunGroup - 1) / kRunGroup * kRunGroup; }

}  // namespace gx

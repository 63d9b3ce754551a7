// gx_pr_sorted.hip -- PageRank pull SpMV over column-sorted row blocks (k_pr_pull_units).
//
// Same iteration as k_pr_pull (gx_pr.hip; Graphalytics PR, LAGr_PageRankGX pr.cpp:61):
//     r(v) = teleport + sum_{u in in(v)} x(u);   x'(v) = r(v) / (outdeg(v)/d)
// but the x gathers are issued in column order.
//
// Why: gathering row by row, a 64-lane instruction covered 1.33 gathers per 128-B line of x on
// SYN-7_5 (44.7 M L2 requests per launch).  Sorting the entries of a block of rows by column
// puts equal and neighbouring columns into the same instruction, and each block sweeps x in
// increasing address order.
//
// This file owns the iteration: SortedArgs, the epilogue and gather_* helpers, k_pr_combine,
// k_pr_pull_units and pr_step_sorted.  The plan that builds every table named below
// (pr_plan_sorted and its kernels) is gx_pr_plan.hip; gx_pr.h holds what both need.
//
// Layout (built once per plan on the device by a radix sort of (segment, column) keys, in groups
// of segments whose keys fit 32 bits):
//   spk[e]   uint32 : (column - group base) << 14 | row of the entry within its block
//   gbase[g] uint32 : base column of 64-entry group g; bit 31 set = escape: the group spans
//                     >= 2^18 columns and reads them from sci
//   sci[e]   int32  : the columns of the escape groups
// A block keeps the CSR range [rp[row_begin], rp[row_end]) of its rows and streams 4 B per
// entry, like the CSR column index.  Inside every full 64-entry group the entries are then
// permuted (k_sorted_laneperm) so that each LDS-add instruction hits distinct banks; the
// group's column set, hence its gathers' lines, is unchanged.
// A block's column-sorted entries are then recoded from the front: its run region as 2-byte
// codes in groups of 64 of one 16-byte pair of x (rpk / rpair, gather_runs: one x load per wave
// and 8 groups, gx_pr_runs.h), its pair prefix as 4-byte slots of two entries of one 16-byte pair
// of x (ppk / pbase, gather_pairs: one 16-B x load per two entries), the dense columns after it as
// 2-byte narrow codes (npk / nbase, gather_narrow); spk / gbase / sci serve the wide remainder
// (gather_units).  Before the recoding, the entries of each column's (column pair's) run in the
// three prefixes are put in a bank-aware order (k_bank_order): the run's 16 consecutive entries
// that one lane group of an LDS add covers then hold rows of different bank slots where it can.
// Gathered values are added into LDS row accumulators (ds_add_f64) in wave-arrival order:
// scores agree with the row-order sum to ~1e-15 relative but are not bit-reproducible run to
// run (the parity bar is 1e-12 relative, tests/test_gpu_parity.py).
//
// Each sorted block is cut into interleaved units (one work item each, LDS accumulators for
// every row of the block); a multi-unit block's units combine through write-through slabs and
// an arrival ticket.  Items run one workgroup each, or, on launches of >= 2 items per CU, from
// a device work queue drained by one resident workgroup per CU (k_pr_pull_units QUEUE).  Rows
// longer than `long_nnz` take the LONG path (a workgroup per 8192-entry segment, in row order);
// their workgroups come first.  A block without any entry (isolated vertices: 29.5 % of SYN-7_5's
// rows) runs only the epilogue.  Its rows were also tried as 64 Ki-row blocks at the end of the
// grid: a CU streams one such block's epilogue at ~100 GB/s, ~15 us, which lengthened the launch.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gx_pr.h"
#include "gx_pr_runs.h"

namespace gx {
namespace {

constexpr int kCombRows = (1 << kRowBits) / kBS;   // rows per thread in a slab combine (16)

struct SortedArgs {
    const RowBlock *blocks;
    const int32_t *ci;       // row-order columns (LONG rows)
    const int32_t *sci;      // block-sorted columns (escape groups)
    const uint32_t *spk;     // packed entries
    const uint32_t *gbase;   // per 64-entry group: base column, bit 31 = escape
    const int32_t *outdeg;
    const double *x_in;
    double *x_out;
    double *rank_out;
    int64_t chunk;
    int nranks;
    int zero_slot;
    int32_t zero_col;        // a padding slot of x that holds 0.0 (chunk - 2)
    double teleport0, damping_over_n, damping;
    const int32_t *long_first;
    const int32_t *long_nseg;
    double *long_part;
    uint32_t *long_ticket;
    uint32_t nlong, nlong_pad;
    // fused dangling sum: per block slot or -1, partials, ticket
    const int32_t *dslot;
    double *dpart;
    uint32_t *dticket;
    uint32_t ndblocks;
    // isolated rows in closed form (GX_PR_ISO_CLOSED): rows of blocks left out of this launch, each
    // of score teleport, added to the dangling sum by whoever writes it
    double iso_rows;
    // split blocks
    const SortedUnit *units;
    uint32_t nunits;
    double *uslab;
    uint32_t *uticket;
    uint64_t *utimes;        // debug (GX_PR_UNIT_TIMES): per workgroup start, gather end, end, XCC
    const uint16_t *npk;     // narrow codes
    const uint32_t *nbase;   // per narrow supergroup: the column before its first code
    uint32_t null_sg;        // all-padding supergroup (base = zero_col)
    uint32_t nt_col;         // CP bit 2: narrow supergroups from this column on gathered non-temporally
    const uint32_t *ppk;     // pair slots
    const uint32_t *pbase;   // per pair supergroup: the pair index before its first slot
    uint32_t pnull_sg;       // all-padding pair supergroup (base = the pair of zero_col)
    const uint16_t *rpk;     // run codes
    const uint32_t *rpair;   // per run group: its column pair (8 per run supergroup)
    uint32_t rnull_sg;       // all-padding run supergroup (every group the pair of zero_col)
    double *xd;              // x of the rows past `live` (store_x, gx_pr.h)
    int64_t live;
    // work queue (GX_PR_QUEUE): [0] next work item, [1] workgroups done (reset by the last)
    uint32_t *queue;
    // combine kernel (PrPart::comb_kernel): the units of multi-unit blocks only store their slabs
    int comb;
    const CombStripe *cstripes;
};

// Returns the row's score if the row is dangling (out-degree 0), else 0.
__device__ __forceinline__ double sorted_epilogue(const SortedArgs &a, int64_t row, double s, double teleport) {
    const double r = teleport + s;
    if (a.rank_out) a.rank_out[row] = r;
    const int32_t deg = a.outdeg[row];
    store_x(a.x_out, a.xd, a.live, row, deg > 0 ? r / ((double)deg / a.damping) : r);
    return deg > 0 ? 0.0 : r;
}

// The epilogue of rows [r0, r0 + nrows) of a block, thread tid taking rows tid, tid + kBS, ...:
// eight out-degree loads issued before any store, since the compiler cannot move a load of
// outdeg above a store to x_out (they might alias) and the row-by-row loop paid one memory
// latency per row a thread handles (16 for SYN-8_5's 16 320-row blocks).  acc null: sums 0.
// Returns the thread's dangling-score sum.
__device__ __forceinline__ double epilogue_rows(const SortedArgs &a, int64_t r0, int nrows, const double *acc,
                                                double teleport) {
    constexpr int kB = 8;
    double d = 0.0;
    for (int i0 = threadIdx.x; i0 < nrows; i0 += kB * kBS) {
        int32_t deg[kB];
#pragma unroll
        for (int q = 0; q < kB; q++) {
            const int i = i0 + q * kBS;
            deg[q] = i < nrows ? a.outdeg[r0 + i] : 1;
        }
#pragma unroll
        for (int q = 0; q < kB; q++) {
            const int i = i0 + q * kBS;
            if (i >= nrows) break;
            const double r = teleport + (acc ? acc[i] : 0.0);
            if (a.rank_out) a.rank_out[r0 + i] = r;
            store_x(a.x_out, a.xd, a.live, r0 + i, deg[q] > 0 ? r / ((double)deg[q] / a.damping) : r);
            if (deg[q] == 0) d += r;
        }
    }
    return d;
}

// Fused dangling sum: the block's dangling scores d (one value per thread) are reduced, the
// block publishes its partial in its slot (agent scope) and takes a ticket; the last of the
// ndblocks participants adds the partials up with the whole workgroup (thread t takes slots
// t, t + kBS, ...; fixed tree, so the order is fixed) into the chunk's last x slot.
template <int BS = kBS>
__device__ __forceinline__ void dangling_publish(const SortedArgs &a, int32_t slot, double d, double *wred, int *last,
                                                 double teleport) {
    const int tid = threadIdx.x;
    d = wave_sum(d);
    __syncthreads();   // wred may still be read by an earlier reduction
    if ((tid & (kWave - 1)) == 0) wred[tid / kWave] = d;
    __syncthreads();
    if (tid == 0) {
        double tot = 0.0;
#pragma unroll
        for (int w = 0; w < BS / kWave; w++) tot += wred[w];
        __hip_atomic_store(&a.dpart[slot], tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t t = __hip_atomic_fetch_add(a.dticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *last = t == a.ndblocks - 1;
    }
    __syncthreads();
    if (!*last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    double v = 0.0;
    for (uint32_t j = tid; j < a.ndblocks; j += BS) v += __hip_atomic_load(&a.dpart[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    v = wave_sum(v);
    __syncthreads();
    if ((tid & (kWave - 1)) == 0) wred[tid / kWave] = v;
    __syncthreads();
    if (tid == 0) {
        double all = 0.0;
#pragma unroll
        for (int w = 0; w < BS / kWave; w++) all += wred[w];
        __hip_atomic_store(a.dticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.x_out[a.chunk - 1] = all + a.iso_rows * teleport;
    }
}

// LONG: one segment of one long row (row order), a whole workgroup; segments of one row are
// combined by the last arriver (agent-scope release/acquire ticket).
__device__ __forceinline__ void long_segment(const SortedArgs &a, const RowBlock &b, double *wred, double teleport) {
    const int tid = threadIdx.x;
    const int64_t zb = b.nz_begin, ze = b.nz_end;
    double s0 = 0.0, s1 = 0.0;
    for (int64_t k0 = zb + tid; k0 < ze; k0 += (int64_t)kU * kBS) {
        int32_t c[kU];
#pragma unroll
        for (int u = 0; u < kU; u++) c[u] = __builtin_nontemporal_load(a.ci + min(k0 + (int64_t)u * kBS, ze - 1));
        double g[kU];
#pragma unroll
        for (int u = 0; u < kU; u++) g[u] = a.x_in[c[u]];
#pragma unroll
        for (int u = 0; u < kU; u++)
            if (k0 + (int64_t)u * kBS < ze) ((u & 1) ? s1 : s0) += g[u];
    }
    const double s = wave_sum(s0 + s1);
    if ((tid & (kWave - 1)) == 0) wred[tid / kWave] = s;
    __syncthreads();
    if (tid != 0) return;
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < kBS / kWave; w++) tot += wred[w];
    const int32_t sp = b.split;
    const int32_t nseg = a.long_nseg[sp];
    if (nseg == 1) {
        sorted_epilogue(a, b.row_begin, tot, teleport);
        return;
    }
    const int32_t first = a.long_first[sp];
    // publish the partial (agent scope), then take a ticket; the last arriver combines
    __hip_atomic_store(&a.long_part[first + b.seg], tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t t = __hip_atomic_fetch_add(&a.long_ticket[sp], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t != (uint32_t)(nseg - 1)) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    double all = 0.0;
    for (int j = 0; j < nseg; j++)
        all += __hip_atomic_load(&a.long_part[first + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.long_ticket[sp], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sorted_epilogue(a, b.row_begin, all, teleport);
}

// Adds x(column) of the sorted entries [lo, hi) of block b into the LDS row accumulators,
// taking every (step / kRound)-th round of kRound entries from the one holding lo (the
// interleaved units of a split block; lo - nz_begin is a multiple of kRound).
//
// Four entries per lane from one 16-B index load (X4): what bounds the launch is the CU's
// vector memory and LDS instruction stream (timing probes).  Wave w takes the
// kU / 4 256-entry supergroups [R + 256 (w kU/4 + v), +256) of round R; lane l holds entries
// 4l .. 4l+3 of each.  A supergroup has one base column, a scalar load, so a lane's columns are
// base + (entry >> 14) with no per-lane select.  Pipelined across rounds: round k+1's gathers
// are issued before round k's LDS adds, the index loads two rounds ahead, buffers A/B
// alternating (a copy of a pending load would wait for it).  Positions are block-relative
// 32-bit values.  An entry outside [lo, hi) gathers the zero padding slot x[zero_col] and adds
// 0.0 to whatever row its (clamped or neighbouring) index word names -- below 16 Ki, and the
// launch reserves 16 Ki accumulators -- so the hot path has no 64-bit compares or masks.  The
// columns of escape supergroups (spanning >= 2^18 ids) come from sci inside a uniform branch
// that consumes its loads there: a load merged into the columns after the branch made the
// compiler drain every outstanding load (s_waitcnt vmcnt(0)) each round.
template <int CP>   // CP bit 0: index loads non-temporal (bit 2: gather_narrow)
__device__ __forceinline__ void gather_units(const SortedArgs &a, const RowBlock &b, int64_t lo64, int64_t hi64,
                                             double *acc, int64_t step64) {
    const int tid = threadIdx.x;
    const int64_t z0 = b.nz_begin;
    const int32_t lo = (int32_t)(lo64 - z0), hi = (int32_t)(hi64 - z0), step = (int32_t)step64;
    if (lo >= hi) return;
    const int32_t last = (int32_t)(b.nz_end - z0) - 1;
    const int32_t nsg = (last >> 8) + 1;   // supergroups of the block
    const uint32_t span = (uint32_t)(hi - lo);
    const uint32_t *spk = a.spk + z0;
    const int32_t *sci = a.sci + z0;
    const uint32_t *sgb = a.gbase + b.seg;
    const int32_t zc = a.zero_col;
    const char *xb = reinterpret_cast<const char *>(a.x_in);
    const int lane = tid & (kWave - 1);
    constexpr int V = kU / 4;
    const int wave = tid >> 6;
    struct Rd {
        uint4 q[V];
        uint32_t bq;   // lane l: the base of supergroup l mod V (a vector load, see below)
    };
    struct Gt {
        double g[kU];
        uint32_t r[kU];
    };
    // The supergroup bases come in through one vector load per round (lanes l mod V) read back
    // with v_readlane: a scalar load's wait (lgkmcnt) would also wait for the LDS adds in flight.
    auto load = [&](Rd &d, int32_t R) {
        const int32_t sg0 = R + wave * V * 256;
#pragma unroll
        for (int v = 0; v < V; v++) {
            const int32_t sg = sg0 + v * 256;
            // clamped into the block; spk's allocation slack covers the 3 entries past `last`;
            // the address is a CSR offset, only 4-B aligned (gx_u32x4)
            const gx_u32x4 *qa = reinterpret_cast<const gx_u32x4 *>(spk + min(sg + 4 * lane, last));
            const gx_u32x4 q4 = (CP & 1) ? __builtin_nontemporal_load(qa) : *qa;
            d.q[v] = make_uint4(q4.x, q4.y, q4.z, q4.w);
        }
        d.bq = sgb[min((sg0 >> 8) + (lane & (V - 1)), nsg - 1)];
    };
    auto issue = [&](const Rd &d, int32_t R, Gt &t) {
        int32_t c[kU];
        uint32_t sb[V], esc = 0;
#pragma unroll
        for (int v = 0; v < V; v++) {
            sb[v] = __builtin_amdgcn_readlane(d.bq, v);
            esc |= sb[v];
        }
#pragma unroll
        for (int v = 0; v < V; v++) {
            const uint32_t w4[4] = {d.q[v].x, d.q[v].y, d.q[v].z, d.q[v].w};
            const int32_t d0 = R + (wave * V + v) * 256 + 4 * lane - lo;
            const uint32_t base = sb[v] & 0x7fffffffu;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int i = 4 * v + j;
                const bool ok = (uint32_t)(d0 + j) < span;
                t.r[i] = w4[j] & ((1u << kRowBits) - 1);
                // materialised here: sunk to the adds, the rows would keep this buffer's index
                // registers live past its reload, and the allocator copies at the loop latch
                asm volatile("" : "+v"(t.r[i]));
                c[i] = ok ? (int32_t)(base + (w4[j] >> kRowBits)) : zc;
            }
        }
        if (esc & 0x80000000u) {   // uniform: an escape supergroup in this round
#pragma unroll
            for (int v = 0; v < V; v++) {
                if (!(sb[v] & 0x80000000u)) continue;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int i = 4 * v + j;
                    const int32_t pos = R + (wave * V + v) * 256 + 4 * lane + j;
                    if ((uint32_t)(pos - lo) < span) c[i] = sci[pos];
                }
            }
            // consume the loads here: a column register still waiting on one at the branch's end
            // makes the compiler wait for every load in flight (vmcnt(0)) on both paths
            __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0)
        }
#pragma unroll
        for (int i = 0; i < kU; i++) t.g[i] = *reinterpret_cast<const double *>(xb + ((uint32_t)c[i] << 3));
    };
    auto add = [&](const Gt &t) {
#pragma unroll
        for (int i = 0; i < kU; i++) atomicAdd(&acc[t.r[i]], t.g[i]);
    };
    // Two rounds per trip of a counted loop with a single exit.  The stages are fenced from
    // the scheduler and the exits are not shared: a load hoisted above the issue that still
    // reads its buffer, or one exit block adding "tA or tB", makes the register allocator copy
    // a buffer at the loop latch, and a copy waits for the loads in flight.
    const int32_t nr = (hi - lo + step - 1) / step;   // rounds of this unit
    if (nr <= 0) return;
    Rd dA, dB;
    Gt tA, tB;
    int32_t R = lo;
    load(dA, R);
    load(dB, R + step);
    issue(dA, R, tA);
    __builtin_amdgcn_sched_barrier(0);
    load(dA, R + 2 * step);
    int32_t k = 1;
    for (; k + 1 < nr; k += 2) {
        __builtin_amdgcn_sched_barrier(0);
        issue(dB, R + step, tB);
        __builtin_amdgcn_sched_barrier(0);
        load(dB, R + 3 * step);
        __builtin_amdgcn_sched_barrier(0);
        add(tA);
        __builtin_amdgcn_sched_barrier(0);
        issue(dA, R + 2 * step, tA);
        __builtin_amdgcn_sched_barrier(0);
        load(dA, R + 4 * step);
        __builtin_amdgcn_sched_barrier(0);
        add(tB);
        R += 2 * step;
    }
    if (k < nr) {
        issue(dB, R + step, tB);
        add(tA);
        add(tB);
    } else {
        add(tA);
    }
}

// The narrow prefix of a block: 2-byte codes (delta << 14) | row, delta = the column step from
// the previous code (0..3; a larger step is split by filler codes of step 3 whose rows are
// junk accumulators >= kJunkRow).  A narrow supergroup of 512 codes is one wave-load of 16 B
// per lane (lane l: codes l + 64 k, stored lane-major), decoded by two packed DPP scans (issue
// below).  Round i of the unit is
// the workgroup's 16 supergroups (j + i k) * 16 + wave; a supergroup past the block reads the
// null supergroup (padding codes, base = x's zero slot), so the loop has no range checks.
// Same pipeline as gather_units: round i+1's gathers issue before round i's LDS adds, the
// loads two rounds ahead, buffers A/B alternating.
template <int CP>
__device__ __forceinline__ void gather_narrow(const SortedArgs &a, const SortedUnit &u, double *acc) {
    constexpr int W = kBS / kWave;   // supergroups per round
    const int32_t nrounds = (u.nsg + W - 1) / W;
    if (u.unit >= nrounds) return;
    const int32_t nr = (nrounds - u.unit + u.nunits - 1) / u.nunits;   // rounds of this unit
    if (nr <= 0) return;
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = tid >> 6;
    const uint32_t sg0 = (uint32_t)(u.nbeg / kNSg);
    const char *xb = reinterpret_cast<const char *>(a.x_in);
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // 16-B aligned (512-code runs)
    struct Rd {
        u32x4 q;
        uint32_t base;
    };
    struct Gt {
        double g[kU];
        uint32_t r[kU];
    };
    auto load = [&](Rd &d, int32_t i) {
        const int32_t sg = (u.unit + i * u.nunits) * W + wave;
        const uint32_t g = sg < u.nsg ? sg0 + (uint32_t)sg : a.null_sg;
        const u32x4 *qa = reinterpret_cast<const u32x4 *>(a.npk + (size_t)g * kNSg) + lane;
        d.q = (CP & 1) ? __builtin_nontemporal_load(qa) : *qa;
        d.base = a.nbase[g];
    };
    // Lane l holds the codes of entries l + 64 k (k < 8) of the supergroup, so instruction k
    // gathers 64 consecutive sorted entries (3x fewer distinct lines per instruction than 8
    // consecutive entries per lane on SYN-8_5).  The eight lane scans run packed, four 8-bit
    // fields per register (a field's sum is at most 64 x 3), in two DPP scans; entry 64 k + l
    // sits at base + (the column steps of instructions < k) + field k of the scan.
    auto issue = [&](const Rd &d, Gt &t) {
        const uint32_t w[4] = {d.q.x, d.q.y, d.q.z, d.q.w};
        uint32_t pk[2] = {0u, 0u};
#pragma unroll
        for (int k = 0; k < kU; k++) {
            const uint32_t c = (k & 1) ? (w[k >> 1] >> 16) : (w[k >> 1] & 0xffffu);
            pk[k >> 2] |= (c >> kRowBits) << (8 * (k & 3));
            t.r[k] = c & ((1u << kRowBits) - 1);
            asm volatile("" : "+v"(t.r[k]));
        }
        const uint32_t s0 = wave_scan_incl(pk[0]), s1 = wave_scan_incl(pk[1]);
        const uint32_t t0 = (uint32_t)__builtin_amdgcn_readlane((int)s0, kWave - 1);
        const uint32_t t1 = (uint32_t)__builtin_amdgcn_readlane((int)s1, kWave - 1);
        uint32_t bk = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.base);
        const uint32_t b0 = bk;
        uint32_t col[kU];
#pragma unroll
        for (int k = 0; k < kU; k++) {
            const uint32_t sk = k < 4 ? s0 : s1, tk = k < 4 ? t0 : t1;
            col[k] = bk + ((sk >> (8 * (k & 3))) & 255u);
            bk += (tk >> (8 * (k & 3))) & 255u;
        }
        if ((CP & 4) && b0 >= a.nt_col) {   // past the hub lines: streamed (GX_PR_CP bit 2)
#pragma unroll
            for (int k = 0; k < kU; k++) t.g[k] = __builtin_nontemporal_load(reinterpret_cast<const double *>(xb + (col[k] << 3)));
        } else {
#pragma unroll
            for (int k = 0; k < kU; k++) t.g[k] = *reinterpret_cast<const double *>(xb + (col[k] << 3));
        }
    };
    auto add = [&](const Gt &t) {
#pragma unroll
        for (int k = 0; k < kU; k++) atomicAdd(&acc[t.r[k]], t.g[k]);
    };
    Rd dA, dB;
    Gt tA, tB;
    load(dA, 0);
    load(dB, 1);
    issue(dA, tA);
    __builtin_amdgcn_sched_barrier(0);
    load(dA, 2);
    int32_t k = 1;
    for (; k + 1 < nr; k += 2) {
        __builtin_amdgcn_sched_barrier(0);
        issue(dB, tB);
        __builtin_amdgcn_sched_barrier(0);
        load(dB, k + 2);
        __builtin_amdgcn_sched_barrier(0);
        add(tA);
        __builtin_amdgcn_sched_barrier(0);
        issue(dA, tA);
        __builtin_amdgcn_sched_barrier(0);
        load(dA, k + 3);
        __builtin_amdgcn_sched_barrier(0);
        add(tB);
    }
    if (k < nr) {
        issue(dB, tB);
        add(tA);
        add(tB);
    } else {
        add(tA);
    }
}

// The pair prefix of a block: 4-byte slots of two entries whose columns lie in one 16-byte
// aligned pair of x (columns 2p and 2p + 1), so one 16-B load per lane serves two entries:
//     step << 30 | (selA << 14 | rowA) << 15 | (selB << 14 | rowB)
// step = the pair index step from the previous slot (0..3; a larger one is split by filler slots
// of step 3 with two junk rows), sel = the column's low bit, row = the row in the block.  A column
// pair holding an odd number of the prefix's entries ends in a slot whose second half is a junk
// row.  A pair supergroup of 256 slots is one wave-load of 16 B per lane (lane l: slots l + 64 k,
// stored lane-major), decoded by one packed DPP scan; rounds, null supergroup and pipeline as in
// gather_narrow.  x_in must be 16-byte aligned and the chunk even (pr_plan_sorted, pr_step_sorted).
template <int CP>
__device__ __forceinline__ void gather_pairs(const SortedArgs &a, const SortedUnit &u, double *acc) {
    constexpr int W = kBS / kWave;   // supergroups per round
    constexpr int kS = kU / 2;       // slots per lane and round
    const int32_t nrounds = (u.psg + W - 1) / W;
    if (u.unit >= nrounds) return;
    const int32_t nr = (nrounds - u.unit + u.nunits - 1) / u.nunits;
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = tid >> 6;
    const uint32_t sg0 = (uint32_t)(u.pbeg / kPSg);
    const char *xb = reinterpret_cast<const char *>(a.x_in);
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // 16-B aligned (256-slot runs)
    typedef double d2 __attribute__((ext_vector_type(2)));
    struct Rd {
        u32x4 q;
        uint32_t base;
    };
    struct Gt {
        d2 g[kS];
        uint32_t r[kS];   // the slot's two (sel, row) halves
    };
    auto load = [&](Rd &d, int32_t i) {
        const int32_t sg = (u.unit + i * u.nunits) * W + wave;
        const uint32_t g = sg < u.psg ? sg0 + (uint32_t)sg : a.pnull_sg;
        const u32x4 *qa = reinterpret_cast<const u32x4 *>(a.ppk + (size_t)g * kPSg) + lane;
        d.q = (CP & 1) ? __builtin_nontemporal_load(qa) : *qa;
        d.base = a.pbase[g];
    };
    // Lane l holds slots l + 64 k (k < 4), so instruction k gathers 64 consecutive slots; the four
    // lane scans run packed in one register (a field's sum is at most 64 x 3).
    auto issue = [&](const Rd &d, Gt &t) {
        const uint32_t w[kS] = {d.q.x, d.q.y, d.q.z, d.q.w};
        uint32_t pk = 0u;
#pragma unroll
        for (int k = 0; k < kS; k++) {
            pk |= (w[k] >> 30) << (8 * k);
            t.r[k] = w[k] & 0x3fffffffu;
            asm volatile("" : "+v"(t.r[k]));
        }
        const uint32_t sc = wave_scan_incl(pk);
        const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)sc, kWave - 1);
        uint32_t bk = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.base);
        const uint32_t b0 = bk;
        uint32_t pr[kS];
#pragma unroll
        for (int k = 0; k < kS; k++) {
            pr[k] = bk + ((sc >> (8 * k)) & 255u);
            bk += (tot >> (8 * k)) & 255u;
        }
        if ((CP & 4) && 2u * b0 >= a.nt_col) {   // past the hub lines: streamed (GX_PR_CP bit 2)
#pragma unroll
            for (int k = 0; k < kS; k++) t.g[k] = __builtin_nontemporal_load(reinterpret_cast<const d2 *>(xb + (pr[k] << 4)));
        } else {
#pragma unroll
            for (int k = 0; k < kS; k++) t.g[k] = *reinterpret_cast<const d2 *>(xb + (pr[k] << 4));
        }
    };
    auto add = [&](const Gt &t) {
#pragma unroll
        for (int k = 0; k < kS; k++) {
            const uint32_t r = t.r[k];
            atomicAdd(&acc[(r >> 15) & ((1u << kRowBits) - 1)], (r & (1u << 29)) ? t.g[k].y : t.g[k].x);
            atomicAdd(&acc[r & ((1u << kRowBits) - 1)], (r & (1u << kRowBits)) ? t.g[k].y : t.g[k].x);
        }
    };
    Rd dA, dB;
    Gt tA, tB;
    load(dA, 0);
    load(dB, 1);
    issue(dA, tA);
    __builtin_amdgcn_sched_barrier(0);
    load(dA, 2);
    int32_t k = 1;
    for (; k + 1 < nr; k += 2) {
        __builtin_amdgcn_sched_barrier(0);
        issue(dB, tB);
        __builtin_amdgcn_sched_barrier(0);
        load(dB, k + 2);
        __builtin_amdgcn_sched_barrier(0);
        add(tA);
        __builtin_amdgcn_sched_barrier(0);
        issue(dA, tA);
        __builtin_amdgcn_sched_barrier(0);
        load(dA, k + 3);
        __builtin_amdgcn_sched_barrier(0);
        add(tB);
    }
    if (k < nr) {
        issue(dB, tB);
        add(tA);
        add(tB);
    } else {
        add(tA);
    }
}

// The run region of a block, ahead of its pair prefix (gx_pr_runs.h): 2-byte codes sel << 14 | row
// in groups of 64 codes of one column pair (columns 2p and 2p + 1; sel = the column's low bit).  A
// pair's run starts on a group and its last group ends in padding codes (sel 0, the lane's junk
// row).  A run supergroup of 512 codes is one wave-load of 16 B per lane (lane l: codes l + 64 k,
// stored lane-major, so instruction k is group k) and has a header of 8 pair indices, rpair.  The
// wave gets the 8 pairs of x by one 16-B load per lane (lane l: the pair of group l mod 8) and reads
// group k's two values back from lane k (v_readlane): no per-lane gather and no scan.  The header
// and x come by vector loads: a scalar load's wait (lgkmcnt) would also wait for the LDS adds in
// flight.  Rounds, null supergroup and pipeline as in gather_narrow.  x_in must be 16-byte aligned
// and the chunk even (pr_plan_sorted, pr_step_sorted).
template <int CP>
__device__ __forceinline__ void gather_runs(const SortedArgs &a, const SortedUnit &u, double *acc) {
    constexpr int W = kBS / kWave;   // supergroups per round
    const int32_t nrounds = (u.rsg + W - 1) / W;
    if (u.unit >= nrounds) return;
    const int32_t nr = (nrounds - u.unit + u.nunits - 1) / u.nunits;
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = tid >> 6;
    const uint32_t sg0 = (uint32_t)(u.rbeg / kRunSg);
    const char *xb = reinterpret_cast<const char *>(a.x_in);
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // 16-B aligned (512-code runs)
    typedef double d2 __attribute__((ext_vector_type(2)));
    struct Rd {
        u32x4 q;
        uint32_t pair;   // lane l: the pair of group l mod 8
    };
    struct Gt {
        d2 g;            // lane l: x of the pair of group l mod 8
        uint32_t c[4];   // the lane's 8 codes, decoded by the adds
    };
    auto load = [&](Rd &d, int32_t i) {
        const int32_t sg = (u.unit + i * u.nunits) * W + wave;
        const uint32_t g = sg < u.rsg ? sg0 + (uint32_t)sg : a.rnull_sg;
        const u32x4 *qa = reinterpret_cast<const u32x4 *>(a.rpk + (size_t)g * kRunSg) + lane;
        d.q = (CP & 1) ? __builtin_nontemporal_load(qa) : *qa;
        d.pair = a.rpair[(size_t)g * kRunSgGroups + (lane & (kRunSgGroups - 1))];
    };
    // the hub lines: default cache policy
    auto issue = [&](const Rd &d, Gt &t) {
        const uint32_t w[4] = {d.q.x, d.q.y, d.q.z, d.q.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            t.c[k] = w[k];
            asm volatile("" : "+v"(t.c[k]));
        }
        t.g = *reinterpret_cast<const d2 *>(xb + (d.pair << 4));
    };
    auto add = [&](const Gt &t) {
        const int xl = __double2loint(t.g.x), xh = __double2hiint(t.g.x);
        const int yl = __double2loint(t.g.y), yh = __double2hiint(t.g.y);
#pragma unroll
        for (int k = 0; k < kRunSgGroups; k++) {
            const double xk = __hiloint2double(__builtin_amdgcn_readlane(xh, k), __builtin_amdgcn_readlane(xl, k));
            const double yk = __hiloint2double(__builtin_amdgcn_readlane(yh, k), __builtin_amdgcn_readlane(yl, k));
            const uint32_t c = (k & 1) ? (t.c[k >> 1] >> 16) : (t.c[k >> 1] & 0xffffu);
            atomicAdd(&acc[c & ((1u << kRowBits) - 1)], (c & (1u << kRowBits)) ? yk : xk);
        }
    };
    Rd dA, dB;
    Gt tA, tB;
    load(dA, 0);
    load(dB, 1);
    issue(dA, tA);
    __builtin_amdgcn_sched_barrier(0);
    load(dA, 2);
    int32_t k = 1;
    for (; k + 1 < nr; k += 2) {
        __builtin_amdgcn_sched_barrier(0);
        issue(dB, tB);
        __builtin_amdgcn_sched_barrier(0);
        load(dB, k + 2);
        __builtin_amdgcn_sched_barrier(0);
        add(tA);
        __builtin_amdgcn_sched_barrier(0);
        issue(dA, tA);
        __builtin_amdgcn_sched_barrier(0);
        load(dA, k + 3);
        __builtin_amdgcn_sched_barrier(0);
        add(tB);
    }
    if (k < nr) {
        issue(dB, tB);
        add(tA);
        add(tB);
    } else {
        add(tA);
    }
}

// One iteration's SpMV over split blocks.  Work items: [0, nlong_pad) LONG row segments (padded
// to a multiple of 8), then the units (largest first; the blocks of rows without entries last).  A multi-unit block's units store their row sums write-through (sc1) to
// their own slab, drain them (vmcnt(0)) and take a ticket; the last arriver adds the slabs in
// unit order with sc1 loads and runs the epilogue (MI355X_MICROARCH.md "Valid forms": sc1 stores
// drained before the counter add, sc1 loads by the workgroup whose add came last).
// TIMES: debug build with per-workgroup timestamps (GX_PR_UNIT_TIMES).
template <bool TIMES, int CP>
__device__ __forceinline__ void pull_item(const SortedArgs &a, const uint32_t w, double *acc, double *wred, int &last,
                                          const double teleport) {
    const int tid = threadIdx.x;
    __shared__ uint64_t ts[2];   // TIMES: start, gather end (LDS, so no registers are held)
    if (TIMES && tid == 0) ts[0] = __builtin_amdgcn_s_memrealtime();
    auto stamp = [&]() {
        if (TIMES && tid == 0) {
            a.utimes[4 * w + 0] = ts[0];
            a.utimes[4 * w + 1] = ts[1];
            a.utimes[4 * w + 2] = __builtin_amdgcn_s_memrealtime();
            a.utimes[4 * w + 3] = (uint64_t)__builtin_amdgcn_s_getreg((3 << 11) | 20);   // HW_REG_XCC_ID[3:0]
        }
    };
    // no block publishes a dangling partial: item 0 writes the sum, 0 or the left-out rows' scores
    if (a.zero_slot && w == 0 && tid == 0) a.x_out[a.chunk - 1] = a.iso_rows * teleport;
    if (w < a.nlong_pad) {
        if (w < a.nlong) long_segment(a, a.blocks[w], wred, teleport);
        stamp();
        return;
    }
    const SortedUnit u = a.units[w - a.nlong_pad];
    const RowBlock b = {u.z0, u.z1, u.r0, u.r1, -1, u.seg};
    const int nrows = b.row_end - b.row_begin;
    // a block without entries (the isolated vertices a hub-first undirected graph puts last):
    // r = teleport, no accumulators, no gathers
    const bool empty = b.nz_begin == b.nz_end;
    if (!empty) {
        for (int i = tid; i < nrows; i += kBS) acc[i] = 0.0;
        __syncthreads();
        gather_runs<CP>(a, u, acc);
        gather_pairs<CP>(a, u, acc);
        gather_narrow<CP>(a, u, acc);
        gather_units<CP>(a, b, u.lo, u.hi, acc, u.step);
        __syncthreads();
    }
    if (TIMES && tid == 0) ts[1] = __builtin_amdgcn_s_memrealtime();
    if (u.nunits > 1 && a.comb) {
        // the combine kernel adds the slabs after this launch (the launch boundary orders them)
        double *mine = a.uslab + u.slab + (int64_t)u.unit * nrows;
        for (int i = tid; i < nrows; i += kBS) mine[i] = acc[i];
        stamp();
        return;
    }
    if (u.nunits > 1) {
        double *mine = a.uslab + u.slab + (int64_t)u.unit * nrows;
        for (int i = tid; i < nrows; i += kBS)
            __hip_atomic_store(&mine[i], acc[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            const uint32_t t = __hip_atomic_fetch_add(&a.uticket[u.part], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last = t == (uint32_t)(u.nunits - 1);
            if (last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(&a.uticket[u.part], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();
        if (!last) {
            stamp();
            return;
        }
        // after tid 0's acquire (this CU's L1 invalidated) and the barrier, plain loads see the
        // other units' slabs.  All kCombRows rows of a thread at once (a block's 16 Ki rows in
        // one pass), so a slab costs one round trip: the slabs live beyond this XCD's L2, and
        // four rows at a time made the combine of 5 slabs ~30 us of a 1/8 piece's 80
        // (tools/unit_times.py).  The adds keep unit order.
        const double *slabs = a.uslab + u.slab;
        if (2 * nrows <= kBS) {
            // few rows (the longest rows' blocks, split into up to 256 units): S threads per
            // row, thread g summing slabs g, g + S, ... 16 loads at a time, then the S partials
            // added in group order through LDS above the block's rows -- a row-per-thread loop
            // would take one round trip per slab (256 on a 1/8 piece's first block)
            int S = 2;
            while (4 * S * nrows <= 2 * kBS && S < u.nunits) S *= 2;
            double *part = acc + (1 << (kRowBits - 1));
            const int r = tid % nrows, g = tid / nrows;
            if (g < S) {
                double s = 0.0;
                for (int j0 = g; j0 < u.nunits; j0 += kCombRows * S) {
                    double v[kCombRows];
#pragma unroll
                    for (int q = 0; q < kCombRows; q++) {
                        const int j = j0 + q * S;
                        v[q] = j < u.nunits ? slabs[(int64_t)j * nrows + r] : 0.0;
                    }
#pragma unroll
                    for (int q = 0; q < kCombRows; q++) s += v[q];
                }
                part[g * nrows + r] = s;
            }
            __syncthreads();
            if (tid < nrows) {
                double s = 0.0;
                for (int q = 0; q < S; q++) s += part[q * nrows + tid];
                acc[tid] = s;
            }
        } else
        for (int i0 = tid; i0 < nrows; i0 += kCombRows * kBS) {
            double s[kCombRows];
#pragma unroll
            for (int q = 0; q < kCombRows; q++) s[q] = 0.0;
            for (int j = 0; j < u.nunits; j++) {
                const double *sl = slabs + (int64_t)j * nrows;
                double v[kCombRows];
#pragma unroll
                for (int q = 0; q < kCombRows; q++) v[q] = i0 + q * kBS < nrows ? sl[i0 + q * kBS] : 0.0;
#pragma unroll
                for (int q = 0; q < kCombRows; q++) s[q] += v[q];
            }
#pragma unroll
            for (int q = 0; q < kCombRows; q++)
                if (i0 + q * kBS < nrows) acc[i0 + q * kBS] = s[q];
        }
        // each thread reads back only the acc entries it wrote: no barrier needed
    }
    double d = 0.0;
    if (empty)
        d = epilogue_rows(a, b.row_begin, nrows, nullptr, teleport);
    else
        d = epilogue_rows(a, b.row_begin, nrows, acc, teleport);
    if (a.dslot) {
        const int32_t slot = a.dslot[u.blk];
        if (slot >= 0) dangling_publish(a, slot, d, wred, &last, teleport);
    }
    stamp();
}

// The slabs of the multi-unit blocks (GX_PR_COMBINE=1), one workgroup per row stripe of at
// most kCombBS rows: S threads per row (S = 1 for full stripes, up to kCombBS / rows for the
// few-row blocks of the longest rows), thread g adding slabs g, g + S, ... in order, 16 loads in
// flight, then the S partials in group order; the row's epilogue; the stripe's dangling partial.
// Spread over the chip instead of one last-arriving workgroup per block, whose k round trips to
// the slabs (a 1/8 piece's 33 Mi-entry block: 75 units of 9 Ki rows) outlasted the launch.
__global__ __launch_bounds__(kCombBS) void k_pr_combine(SortedArgs a) {
    __shared__ double part[kCombBS];
    __shared__ double wred[kCombBS / kWave];
    __shared__ int last;
    double dsum = 0.0;
    for (int k = 0; k < a.nranks; k++) dsum += a.x_in[(int64_t)k * a.chunk + a.chunk - 1];
    const double teleport = a.teleport0 + a.damping_over_n * dsum;
    const CombStripe c = a.cstripes[blockIdx.x];
    const int rows = c.s1 - c.s0;
    int S = 1;
    while (2 * S * rows <= kCombBS && S < c.k) S *= 2;
    const int tid = threadIdx.x, r = tid % rows, g = tid / rows;
    double s = 0.0;
    if (g < S) {
        const double *sl = a.uslab + c.slab + c.s0 + r;
        for (int j0 = g; j0 < c.k; j0 += 16 * S) {
            double v[16];
#pragma unroll
            for (int q = 0; q < 16; q++) {
                const int j = j0 + q * S;
                v[q] = j < c.k ? sl[(int64_t)j * c.nrows] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < 16; q++) s += v[q];
        }
    }
    if (S > 1) {
        if (g < S) part[g * rows + r] = s;
        __syncthreads();
        if (tid < rows) {
            s = 0.0;
            for (int q = 0; q < S; q++) s += part[q * rows + tid];
        }
    }
    double d = 0.0;
    if (tid < rows) d = sorted_epilogue(a, (int64_t)c.r0 + c.s0 + tid, s, teleport);
    if (c.dslot >= 0) dangling_publish<kCombBS>(a, c.dslot, d, wred, &last, teleport);
}

// The next work item for the whole workgroup, with no divergent branch anywhere: wave 0 takes
// it (a scalar branch: readfirstlane of the thread id) by an add in which lane 0 adds 1 and the
// other lanes 0, so lane 0's return value is the item; readfirstlane makes it a scalar, which
// wave 0 stores to LDS and every wave reads back through readfirstlane again.  The caller's
// `w >= total` loop exit is therefore a uniform scalar branch.  Round 4's version took the item
// under `threadIdx.x == 0`, a divergent branch: inlined, the compiler turned that branch into
// the exit of an inner loop which the other lanes of wave 0 kept running, barriers and all,
// while lane 0 waited to fetch, and the launch never ended (a __noinline__ hid it; reading the
// slot through readfirstlane alone did not: the divergent branch was still there).
__device__ __forceinline__ uint32_t queue_fetch(uint32_t *q, uint32_t *slot) {
    if (__builtin_amdgcn_readfirstlane(threadIdx.x) < (uint32_t)kWave) {
        const uint32_t v = __hip_atomic_fetch_add(q, (threadIdx.x & (kWave - 1)) == 0 ? 1u : 0u, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_AGENT);
        *slot = __builtin_amdgcn_readfirstlane(v);
    }
    __syncthreads();
    const uint32_t w = __builtin_amdgcn_readfirstlane(*slot);
    __syncthreads();   // every wave has read the slot before the next fetch rewrites it
    return w;
}

// One workgroup per work item, or (QUEUE, GX_PR_QUEUE=1) one resident workgroup per CU taking
// items from a device counter in the same order: the dispatcher deals workgroups to the XCDs
// round-robin, so an item whose XCD has no free CU waits even while other XCDs idle; from a
// queue every CU takes the next item the moment it is free.
template <bool TIMES, int CP = 0, bool QUEUE = false>
__global__ __launch_bounds__(kBS, TIMES ? 1 : 4) void k_pr_pull_units(SortedArgs a) {
    extern __shared__ double acc[];
    __shared__ double wred[kBS / kWave];
    __shared__ int last;
    double dsum = 0.0;
    for (int k = 0; k < a.nranks; k++) dsum += a.x_in[(int64_t)k * a.chunk + a.chunk - 1];
    const double teleport = a.teleport0 + a.damping_over_n * dsum;
    if constexpr (!QUEUE) {
        pull_item<TIMES, CP>(a, blockIdx.x, acc, wred, last, teleport);
    } else {
        __shared__ uint32_t item;
        const uint32_t total = a.nlong_pad + a.nunits;
        for (;;) {
            const uint32_t w = queue_fetch(a.queue, &item);   // (its barriers: the last item's LDS is free)
            if (w >= total) break;
            pull_item<TIMES, CP>(a, w, acc, wred, last, teleport);
        }
        if (threadIdx.x == 0 &&
            __hip_atomic_fetch_add(&a.queue[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
            __hip_atomic_store(&a.queue[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&a.queue[1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// The kernel of one launch, over one workgroup per item or (QUEUE) the resident workgroups of the
// work queue.  The cache policy picks CP 5 or 1, any other value CP 0; the per-item stamps
// (times, GX_PR_UNIT_TIMES) run without the cache policy.
using PullKernel = void (*)(SortedArgs);
template <bool QUEUE>
PullKernel pull_kernel(bool times, int cache_policy) {
    if (times) return k_pr_pull_units<true, 0, QUEUE>;
    if (cache_policy == 5) return k_pr_pull_units<false, 5, QUEUE>;
    if (cache_policy == 1) return k_pr_pull_units<false, 1, QUEUE>;
    return k_pr_pull_units<false, 0, QUEUE>;
}

// The kernels' view of plan p for one launch over every item, without per-item stamps.
SortedArgs sorted_args(const PrPart *p, const double *x_full, double *x_local, double *rank_out) {
    const double dn = (double)p->n_global;
    SortedArgs a;
    a.blocks = p->blocks.p;
    a.ci = p->ci;
    a.sci = p->sci.p;
    a.spk = p->spk.p;
    a.gbase = p->gbase.p;
    a.outdeg = p->outdeg;
    a.x_in = x_full;
    a.x_out = x_local;
    a.rank_out = rank_out;
    a.chunk = (int64_t)p->chunk;
    a.nranks = p->nranks;
    a.zero_slot = p->nd == 0 ? 1 : 0;
    a.zero_col = (int32_t)p->chunk - 2;
    a.teleport0 = (1.0 - p->damping) / dn;
    a.damping_over_n = p->damping / dn;
    a.damping = p->damping;
    a.long_first = p->long_first.p;
    a.long_nseg = p->long_nseg.p;
    a.long_part = p->long_part.p;
    a.long_ticket = p->long_ticket.p;
    a.nlong = p->nlong_blocks;
    a.nlong_pad = p->nlong_pad;
    a.dslot = p->fused_dangling ? p->dslot.p : nullptr;
    a.dpart = p->fdpart.p;
    a.dticket = p->fdticket.p;
    a.ndblocks = p->ndblocks;
    a.iso_rows = 0.0;
    a.units = p->units.p;
    a.nunits = p->nunits;
    a.uslab = p->uslab.p;
    a.uticket = p->uticket.p;
    a.comb = p->ncstripes > 0 ? 1 : 0;
    a.cstripes = p->cstripes.p;
    a.xd = p->xd.p;
    a.live = (int64_t)p->live;
    a.utimes = nullptr;
    a.npk = p->npk.p;
    a.nbase = p->nbase.p;
    a.null_sg = p->null_sg;
    a.nt_col = p->nt_col;
    a.ppk = p->ppk.p;
    a.pbase = p->pbase.p;
    a.pnull_sg = p->pnull_sg;
    a.rpk = p->rpk.p;
    a.rpair = p->rpair.p;
    a.rnull_sg = p->rnull_sg;
    a.queue = p->queue.p;
    return a;
}

// Debug (GX_PR_UNIT_TIMES): the stamps of the launch of nw items just issued on s, a line per
// workgroup, to the file `path_fmt` names; a "%d" in it numbers the plans that get here.
int dump_unit_times(const PrPart *p, uint32_t nw, const char *path_fmt, hipStream_t s) {
    std::vector<uint64_t> t(4 * (size_t)nw);
    std::vector<SortedUnit> us(p->nunits);
    std::vector<RowBlock> bs(p->nblocks);
    GX_HIP_TRY(hipStreamSynchronize(s));
    GX_HIP_TRY(hipMemcpy(t.data(), p->utimes.p, t.size() * 8, hipMemcpyDeviceToHost));
    if (p->nunits) GX_HIP_TRY(hipMemcpy(us.data(), p->units.p, us.size() * sizeof(SortedUnit), hipMemcpyDeviceToHost));
    if (p->nblocks) GX_HIP_TRY(hipMemcpy(bs.data(), p->blocks.p, bs.size() * sizeof(RowBlock), hipMemcpyDeviceToHost));
    static std::atomic<int> ndump{0};
    char path[512];
    std::snprintf(path, sizeof path, path_fmt, ndump.fetch_add(1));
    FILE *f = std::fopen(path, "w");
    if (!f) return GX_SUCCESS;
    std::fprintf(f, "wg kind blk unit nunits entries rows t0 tgather t1 xcc\n");
    for (size_t w = 0; w < nw; w++) {
        if (w >= p->nlong_blocks && w < p->nlong_pad) continue;
        const bool lng = w < p->nlong_blocks;
        long long ents = 0, nrows = 0;
        int blk = -1, unit = 0, nunits = 1;
        if (lng) {
            ents = bs[w].nz_end - bs[w].nz_begin;
            nrows = 1;
            blk = (int)w;
        } else {
            const SortedUnit &u = us[w - p->nlong_pad];
            for (int64_t k0 = u.lo; k0 < u.hi; k0 += u.step) ents += std::min<int64_t>(u.step / u.nunits, u.hi - k0);
            for (int64_t r = u.unit; r * 16 < u.nsg; r += u.nunits)   // narrow codes (fillers included)
                ents += std::min<int64_t>(16, u.nsg - r * 16) * kNSg;
            for (int64_t r = u.unit; r * 16 < u.rsg; r += u.nunits)   // run codes (padding included)
                ents += std::min<int64_t>(16, u.rsg - r * 16) * kRunSg;
            for (int64_t r = u.unit; r * 16 < u.psg; r += u.nunits)   // pair slots, two entries each
                ents += std::min<int64_t>(16, u.psg - r * 16) * kPSg * 2;
            blk = u.blk;
            unit = u.unit;
            nunits = u.nunits;
            nrows = bs[u.blk].row_end - bs[u.blk].row_begin;
        }
        std::fprintf(f, "%zu %s %d %d %d %lld %lld %llu %llu %llu %llu\n", w, lng ? "long" : "unit", blk, unit, nunits,
                     ents, nrows, (unsigned long long)t[4 * w], (unsigned long long)t[4 * w + 1],
                     (unsigned long long)t[4 * w + 2], (unsigned long long)t[4 * w + 3]);
    }
    std::fclose(f);
    return GX_SUCCESS;
}

}  // namespace

int pr_step_sorted(PrPart *p, const double *x_full, double *x_local, double *rank_out, hipStream_t s,
                   const PrScalars *ov) {
    SortedArgs a = sorted_args(p, x_full, x_local, rank_out);
    if (ov) {   // pr_first_build's S mode: the same launch with other scalars
        a.teleport0 = ov->teleport0;
        a.damping_over_n = ov->damping_over_n;
        a.damping = ov->damping;
    }
    // a pair slot's one load reads x[2p] and x[2p + 1]
    if ((p->npair || p->nrun) && (reinterpret_cast<uintptr_t>(x_full) & 15))
        return fail(GX_INVALID_VALUE, "pr_step_sorted: pair slots and run groups need x 16-byte aligned");
    // Isolated rows in closed form: a launch whose scores nobody asks for leaves the closed-form
    // blocks (the last iso_units items, the last iso_dblocks dangling slots) out and has the
    // dangling sum's writer add their rows * teleport: the last of the remaining publishers, or
    // item 0 when none is left.  The run's last launch writes their scores and keeps every item.
    if (!rank_out && p->fused_dangling && p->iso_units) {
        a.nunits -= p->iso_units;
        a.ndblocks -= p->iso_dblocks;
        a.iso_rows = (double)p->iso_rows;
        if (a.ndblocks == 0) a.zero_slot = 1;
    }
    const char *times_path = std::getenv("GX_PR_UNIT_TIMES");   // debug: not under graph capture
    const uint32_t nw = p->nlong_pad + a.nunits;
    if (times_path && nw) {
        if (!p->utimes.p) GX_TRY(p->utimes.alloc(4 * (size_t)(p->nlong_pad + p->nunits)));
        a.utimes = p->utimes.p;
    }
    if (nw) {
        KTimer kt(p->ctx, "pr_pull", s);   // one iteration's SpMV (+ fused dangling sum)
        // One 1024-thread workgroup per CU, 16 Ki accumulators (128 KiB of LDS) whatever the block's
        // rows: an entry outside its unit's range adds 0.0 to any row below 16 Ki (gather_units).
        // One workgroup per CU also keeps fewer concurrent sweeps of x: SYN-7_5 ran 100-104 us per
        // launch against 109-125 with two (round 2, tools/pr_units_sweep.sh).
        const size_t lds = (size_t)(1 << kRowBits) * sizeof(double);
        // (by the plan's items, so that every launch of a run takes the same kernel)
        const bool use_queue = p->queue_on == 1 || (p->queue_on == -1 && p->nlong_pad + p->nunits >=
                                                                              2u * (unsigned)std::max(1, p->ctx->num_cus));
        const unsigned nq = std::min<unsigned>(nw, (unsigned)std::max(1, p->ctx->num_cus));
        // (narrow gathers three rounds deep ran the same: SYN-8_5 752-753 against 753-754
        // us, SYN-7_5 72.1-73.2 against 71.5-72.4; tools/r03_depth_ab.sh)
        const PullKernel k = use_queue ? pull_kernel<true>(a.utimes != nullptr, p->cache_policy)
                                       : pull_kernel<false>(a.utimes != nullptr, p->cache_policy);
        // queued: one resident workgroup per CU (the LDS allows no second), never more than the items
        hipLaunchKernelGGL(k, dim3(use_queue ? nq : nw), dim3(kBS), lds, s, a);
        // (inside the iteration's timer: the SpMV is both launches)
        if (p->ncstripes) hipLaunchKernelGGL(k_pr_combine, dim3(p->ncstripes), dim3(kCombBS), 0, s, a);
        if (a.utimes && ++p->utimes_launch == env_int("GX_PR_UNIT_TIMES_LAUNCH", 5, 1, 1 << 30))
            GX_TRY(dump_unit_times(p, nw, times_path, s));
    } else if (a.zero_slot) {
        GX_HIP_TRY(hipMemsetAsync(x_local + p->chunk - 1, 0, sizeof(double), s));
    }
    GX_TRY(check_launch("k_pr_pull_units"));
    return p->fused_dangling ? GX_SUCCESS : pr_dangling(p, x_local, s);
}

}  // namespace gx

GX_MODULE_WARMER(pr_sorted)

// gx_pr.h -- PageRank pull plan (row blocks of the pull matrix of one rank).
#pragma once

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include <algorithm>

#include "gx_device.h"

namespace gx {

// GX_PLAN_TIMES=1: the host-side phase times of a plan build on stderr (the stream is
// synchronised at every mark, so device phases are attributed too).  Diagnostics only.
// GX_PLAN_TIMES=2: host time only, no stream synchronisation (the phases' host-side cost,
// without perturbing a call whose upload overlaps its plan).  host_only: a build that runs
// on no stream (pr_multi_blocks), timed by the host clock at either level.
struct PlanClock {
    bool on = false, sync = true;
    hipStream_t s = nullptr;
    const char *what = "";
    std::chrono::steady_clock::time_point t;
    static int level() {   // 0 off, 1 synchronised marks, 2 host time only
        const char *e = std::getenv("GX_PLAN_TIMES");
        const int v = e ? std::atoi(e) : 0;
        return v == 0 ? 0 : v == 2 ? 2 : 1;
    }
    PlanClock(const char *w, hipStream_t st, bool host_only = false) : s(st), what(w) {
        const int l = level();
        on = l != 0;
        sync = l != 2 && !host_only;
        if (on) {
            if (sync) (void)hipStreamSynchronize(s);
            t = std::chrono::steady_clock::now();
        }
    }
    void mark(const char *phase) {
        if (!on) return;
        if (sync) (void)hipStreamSynchronize(s);
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[plan %s] %-28s %8.2f ms\n", what, phase,
                     std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

// One workgroup's share of the pull SpMV (the CSR-Adaptive split):
//   split <  0 : STREAM  -- rows [row_begin, row_end), all of them short, <= kStreamNnz
//                 entries in total; staged through LDS, reduced per row.
//   split >= 0 : LONG    -- entries [nz_begin, nz_end) of the single row row_begin;
//                 rows longer than kSegNnz are cut into several segments whose partial
//                 sums are combined by the last-arriving workgroup (ticket per row).
struct RowBlock {
    int64_t nz_begin;
    int64_t nz_end;
    int32_t row_begin;
    int32_t row_end;
    int32_t split;      // -1 stream; else index into the per-long-row ticket/partials
    int32_t seg;        // segment number within the long row
};

// One workgroup's share of a column-sorted block (k_pr_pull_units, gx_pr_sorted.hip): the
// sorted entries [lo, hi) of block `blk` in rounds of the kernel's U * BS entries, taking
// every (step / (U * BS))-th round (interleaved units: every unit sweeps the block's whole
// column range, so the units of a block move through x together).  A block cut into
// nunits > 1 units sums its rows through per-unit partial slabs (slab + unit * rows doubles);
// the last unit to arrive (ticket[part]) adds them in unit order and runs the epilogue.
// The block's column-sorted prefix of dense columns is stored as narrow 2-byte codes (nbeg,
// nsg: the block's first code in PrPart::npk and its 512-code supergroups); [lo, hi) is the
// wide 4-byte remainder.  Unit j of k takes narrow rounds j, j + k, ... as well.
// Before the narrow codes, the block's pair prefix (pbeg, psg: its first slot in PrPart::ppk and
// its 256-slot supergroups), in rounds dealt to the units the same way, and before those the
// block's run region (rbeg, rsg: its first code in PrPart::rpk and its 512-code supergroups).
struct SortedUnit {
    int64_t lo;
    int64_t hi;
    int64_t step;
    int64_t slab;       // first double of the block's slabs in PrPart::uslab
    int64_t nbeg;       // first narrow code of the block (a multiple of 512)
    int32_t nsg;        // narrow supergroups (512 codes each) of the block
    int32_t blk;        // index into PrPart::blocks
    int32_t part;       // ticket index of a multi-unit block, -1 when nunits == 1
    int32_t unit;       // this unit's number within the block
    int32_t nunits;
    int32_t seg;        // the block's fields (RowBlock), so a workgroup's first loads are
    int64_t z0, z1;     //   independent: its block's entries [z0, z1), rows [r0, r1), first
    int32_t r0, r1;     //   supergroup seg
    int64_t pbeg;       // first pair slot of the block (a multiple of 256)
    int32_t psg;        // pair supergroups (256 slots each) of the block
    int32_t rsg;        // run supergroups (512 codes each) of the block, ahead of the pair prefix
    int64_t rbeg;       // first run code of the block in PrPart::rpk (a multiple of 512)
};

// A row stripe of a multi-unit block, combined by k_pr_combine after the units' launch
// (PrPart::comb_kernel): rows [s0, s1) of the block whose rows start at local row r0 and whose
// k slabs of nrows doubles begin at uslab[slab]; dslot its dangling partial's slot or -1.
struct CombStripe {
    int64_t slab;
    int32_t r0, nrows, s0, s1, k, dslot;
};

// x of local row `row`: rows [0, live) sit in the exchanged chunk, the rest (out-degree 0, so
// no rank ever gathers them) in the rank-private xd, so that only the gathered prefix of each
// rank's rows travels in the all-gather (gx_pr_part_create_live).
__device__ __forceinline__ void store_x(double *x_out, double *xd, int64_t live, int64_t row, double v) {
    if (row < live) x_out[row] = v;
    else xd[row - live] = v;
}

constexpr int kPullBlock = 256;      // 4 waves
constexpr int kStreamNnz = 2048;     // LDS stage: 16 KiB of fp64 per workgroup
constexpr int kStreamRows = 256;     // at most one row per lane in stream mode
constexpr int kSegNnz = 8192;        // entries per LONG segment

struct PrPart {
    gx_ctx *ctx = nullptr;
    uint64_t n_global = 0;
    int nranks = 1, rank = 0;
    uint64_t rows = 0;       // local rows
    uint64_t chunk = 0;      // doubles per rank chunk (last one = dangling slot)
    uint64_t live = ~0ull;   // local rows kept in the chunk; rows [live, rows) have x in xd (~0: all)
    DBuf<double> xd;         // x of the rows past `live` (out-degree 0, never gathered)
    double damping = 0.85;
    // pull matrix of the local rows (column ids already in the padded chunk layout)
    DBuf<int64_t> rp_own;    // when the plan owns its matrix
    DBuf<int32_t> ci_own;
    const int64_t *rp = nullptr;
    const int32_t *ci = nullptr;
    DBuf<int32_t> outdeg_own;
    const int32_t *outdeg = nullptr;   // out-degree of each local row's vertex
    // row blocks
    DBuf<RowBlock> blocks;
    uint32_t nblocks = 0;
    uint32_t nlong_blocks = 0;   // LONG blocks come first in `blocks`
    DBuf<int32_t> long_first;  // per long row: index of its first partial
    DBuf<int32_t> long_nseg;   // per long row: number of segments
    DBuf<double> long_part;    // per segment partial sum
    DBuf<uint32_t> long_ticket;
    uint32_t nlong = 0, nsegs = 0;
    // dangling rows (out-degree 0) of this rank
    DBuf<int32_t> dlist;      // only when the dangling rows are not one contiguous range
    uint64_t nd = 0;
    bool d_range = false;
    int64_t d0 = 0;
    uint32_t dgrid = 0;
    DBuf<double> dpart;
    DBuf<uint32_t> dticket;
    // column-sorted blocks (k_pr_pull_units, gx_pr_sorted.hip; the default)
    DBuf<int32_t> sci;           // columns sorted within each block
    DBuf<uint32_t> spk;          // packed (column - group base) << 14 | row
    DBuf<uint32_t> gbase;        // base column per 256-entry supergroup (bit 31: escape to sci)
    // narrow codes (gx_pr_sorted.hip): (column delta 0..3) << 14 | row, per block a 512-aligned
    // run; the column of a code is its 512-code supergroup's base plus the deltas up to it
    DBuf<uint16_t> npk;
    DBuf<uint32_t> nbase;        // per narrow supergroup: the column before its first code
    uint64_t nnarrow = 0;        // narrow entries (without the delta-only fillers)
    uint64_t ncodes = 0;         // narrow codes, fillers and padding included
    uint32_t null_sg = 0;        // an all-padding supergroup gathering x's zero slot
    // pair slots (gx_pr_sorted.hip gather_pairs): two entries of one 16-byte aligned pair of x
    // (columns 2p, 2p + 1) per 4-byte slot, per block a 256-aligned run before its narrow codes
    DBuf<uint32_t> ppk;
    DBuf<uint32_t> pbase;        // per pair supergroup: the pair index before its first slot
    uint64_t npair = 0;          // entries held in pair slots
    uint64_t npfill = 0;         // filler halves of the slots (odd column pairs, steps above 3)
    uint64_t npslots = 0;        // slots, fillers and padding included
    uint32_t pnull_sg = 0;       // an all-padding pair supergroup (the pair of x's zero slot)
    // run groups (gx_pr_sorted.hip gather_runs, gx_pr_runs.h): 64 two-byte codes (sel << 14 | row)
    // of one column pair, 8 groups per 512-code supergroup, per block a 512-aligned run ahead of
    // its pair prefix
    DBuf<uint16_t> rpk;
    DBuf<uint32_t> rpair;        // per run group: its column pair (8 per supergroup)
    uint64_t nrun = 0;           // entries held in run codes
    uint64_t nrpad = 0;          // padding codes that round the runs up to whole groups
    uint64_t nrcodes = 0;        // run codes, padding and the null supergroup included
    uint32_t rnull_sg = 0;       // an all-padding run supergroup (the pair of x's zero slot)
    int sorted_nnz = 65536;      // entries per block
    int sorted_rows = 4096;      // rows per block (LDS accumulators)
    int64_t unit_nnz = 0;        // target entries per unit
    DBuf<SortedUnit> units;      // one workgroup per unit, after the LONG blocks
    uint32_t nunits = 0;
    DBuf<double> uslab;          // partial row sums of the multi-unit blocks
    DBuf<uint32_t> uticket;      // per multi-unit block: arrivals of the current iteration
    // GX_PR_COMBINE=1: the multi-unit blocks' slabs are added up and their epilogue run by a
    // second kernel over row stripes (k_pr_combine), not by each block's last arriving unit
    bool comb_kernel = false;
    bool force_huge = false;     // the huge-graph plan whatever the size (a block partition's rank)
    DBuf<CombStripe> cstripes;
    uint32_t ncstripes = 0;
    DBuf<uint64_t> utimes;       // debug (GX_PR_UNIT_TIMES): per-workgroup timestamps
    int utimes_launch = 0;
    int long_nnz = 65536;        // longer rows take the LONG segment path
    int sorted_lds = 0;          // dynamic LDS bytes of the launch
    int cache_policy = 0;        // k_pr_pull_units CP: 1 index stream non-temporal, 5 also the narrow
                                 // gathers from column nt_col on (x larger than the L2s)
    uint32_t nt_col = 65536;
    uint32_t nsorted = 0, nlong_pad = 0;
    bool rows_desc = false;      // row lengths non-increasing (an undirected hub-first plan): the
                                 // block cut jumps by binary search
    int queue_on = -1;           // GX_PR_QUEUE: one resident workgroup per CU pulling work items (-1 auto)
    DBuf<uint32_t> queue;        // its counters (k_pr_pull_units QUEUE)
    // dangling-score sum fused into the kernel: blocks holding out-degree-0 rows publish a
    // partial, the last of them adds them up in slot order
    bool fused_dangling = false;
    DBuf<int32_t> dslot;         // per block: its partial's slot, -1 = no dangling rows
    DBuf<double> fdpart;
    DBuf<uint32_t> fdticket;
    uint32_t ndblocks = 0;
    // isolated rows in closed form (GX_PR_ISO_CLOSED, pr_plan_sorted): the last iso_units units are
    // blocks without entries whose rows all lie past `live` (score teleport, x never gathered).
    // They hold the last iso_dblocks dangling slots, and every launch but a run's last leaves
    // them out and adds iso_rows * teleport to the dangling sum instead
    uint32_t iso_units = 0, iso_dblocks = 0;
    uint64_t iso_rows = 0;
    int kernel = 2;              // 1 = k_pr_pull (CSR-Adaptive, GX_PR_KERNEL=adaptive), 2 = k_pr_pull_units;
                                 // set by the plan that lays the matrix out (pr_new_part), obeyed by pr_plan
    // first iteration in closed form (GX_PR_FIRST, pr_first_build / pr_first): S[i] = the sum of
    // 1 / outdeg over row i's in-neighbours, S[rows] = the sum of S over the dangling rows.  It
    // depends on the graph alone, so a resident plan builds it in its first run and every run
    // starts from r1 = t1 + d/n S in one streaming kernel instead of k_pr_init + an SpMV.
    bool first_on = true;        // GX_PR_FIRST (pr_new_part); off once S cannot be allocated
    bool first_ready = false;    // S holds the plan's values
    DBuf<double> S;              // rows + 1 doubles, allocated by the first run (pr_first_alloc)
    // where the sorted plan reads its entries: local row i is row order[i] of (src_rp, src_ci)
    // with every column c renamed perm[c] (gx_pagerank's hub-first plan), or row i itself with
    // its columns as stored (order / perm null: a partition already in its final order)
    const int64_t *src_rp = nullptr;
    const int32_t *src_ci = nullptr;
    const int32_t *src_order = nullptr;
    const int32_t *src_perm = nullptr;
    UploadJob *job = nullptr;  // the source columns still arriving (gx_pagerank_csr): the plan's key
                               // pass scatters each chunk from the source order once it has landed
    DBuf<int32_t> order;       // hub-first position -> old vertex id (gx_pagerank)
    // single-GPU driver buffers (gx_pagerank): vertices relabelled hub-first
    DBuf<double> xa, xb, rank_out, result;
    DBuf<int32_t> perm;        // old vertex id -> position in the hub-first order
};

// A non-increasing sequence of n row lengths as its runs of equal values: run k covers
// positions [pos[k], pos[k+1]) with length val[k], and base[k] entries come before it.  The row
// pointers and lengths of an undirected graph's hub-first rows, known from the device's sorted
// degrees without moving 12 n bytes to the host (pr_single_plan).
struct LengthRuns {
    std::vector<int64_t> pos, val, base;
    uint64_t n = 0;
    int64_t total = 0;
    size_t run(uint64_t i) const {
        return (size_t)(std::upper_bound(pos.begin(), pos.end(), (int64_t)i) - pos.begin()) - 1;
    }
    int64_t prefix(uint64_t i) const {
        if (i >= n) return total;
        const size_t k = run(i);
        return base[k] + ((int64_t)i - pos[k]) * val[k];
    }
    int64_t length(uint64_t i) const { return val[run(i)]; }
};

// Read-only host array (a std::vector, or a buffer the plan filled without zeroing it), or the
// row pointers (prefix) / lengths of a LengthRuns.  Elements are values, not references.
template <typename T>
struct HostView {
    const T *p = nullptr;
    size_t n = 0;
    const LengthRuns *runs = nullptr;
    bool prefix = false;
    template <typename Alloc>
    HostView(const std::vector<T, Alloc> &v) : p(v.data()), n(v.size()) {}
    HostView(const T *ptr, size_t count) : p(ptr), n(count) {}
    HostView(const LengthRuns *r, bool pre) : n(pre ? r->n + 1 : r->n), runs(r), prefix(pre) {}
    size_t size() const { return n; }
    T operator[](size_t i) const { return p ? p[i] : (T)(prefix ? runs->prefix(i) : runs->length(i)); }
};

// Build the row-block plan and dangling list from a local pull CSR (host row pointers
// h_rp, device rp/ci) and device out-degrees, for the kernel the part records (p->kernel; the
// adaptive one needs d_ci, the sorted one reads its entries through p->src_*).  Borrowed device
// pointers must outlive it.
int pr_plan(PrPart *p, HostView<int64_t> h_rp, const int64_t *d_rp,
            const int32_t *d_ci, const int32_t *d_outdeg, HostView<int32_t> h_outdeg);

// Column-sorted block plan (gx_pr_plan.hip) and its iteration (k_pr_pull_units, gx_pr_sorted.hip).
int pr_plan_sorted(PrPart *p, HostView<int64_t> h_rp, HostView<int32_t> h_outdeg);
// The scalars of one launch when they are not the plan's own (pr_first_build's S mode).
struct PrScalars {
    double teleport0, damping_over_n, damping;
};
int pr_step_sorted(PrPart *p, const double *x_full, double *x_local, double *rank_out, hipStream_t s,
                   const PrScalars *ov = nullptr);
// Dangling-score sum of this rank into x_local's last chunk slot.
int pr_dangling(PrPart *p, double *x_local, hipStream_t s);

int pr_init(PrPart *p, double *x_local, hipStream_t s);
struct PrKnobs;
// gx_pagerank's single-rank plan of a graph: its pull matrix (A' when directed, which must be
// built) relabelled hub-first, column-sorted blocks (k.adaptive: the relabelled CSR itself), x
// buffers and the hub-first perm.
int pr_single_plan(gx_graph *g, const PrKnobs &k, PrPart **out);
// Rows of a huge graph's sorted block (kMaxBlockRows below) and its entries.
constexpr int kPlanBlockRows = 16320;
constexpr int64_t kPlanBlockNnz = 32 << 20;

// What the sorted-block iteration (gx_pr_sorted.hip) and its plan (gx_pr_plan.hip) share: the
// geometry of a k_pr_pull_units workgroup and of the code regions, which the plan lays the tables
// out for and the kernel decodes.
constexpr int kRowBits = 14;     // packed entry: (column - group base) << kRowBits | row in block
constexpr int kBS = 1024;        // threads of a k_pr_pull_units workgroup (16 waves, one per CU)
constexpr int kCombBS = 256;     // threads of a k_pr_combine workgroup: rows of a stripe
constexpr int kU = 8;            // entries per lane and round (two 16-B index loads)
constexpr int kRound = kBS * kU; // entries of one round of a workgroup
constexpr int kNSg = 512;        // codes of a narrow supergroup: one wave's 16-B load per lane
constexpr int kPSg = 256;        // slots of a pair supergroup: one wave's 16-B load per lane
constexpr int kRunFillCost = 32;  // GX_PR_RUN_FILL_COST: quarters of an entry per padding code
constexpr int kRunCost = 2;       // GX_PR_RUN_COST: quarters of a narrow entry's cost per run code
constexpr int kJunkRow = (1 << kRowBits) - kWave;   // accumulators [16320, 16384) absorb fillers
constexpr int kMaxBlockRows = kJunkRow;             // rows of a sorted block
static_assert(kMaxBlockRows == kPlanBlockRows, "gx_pr.h block rows");

// Inclusive prefix sum over the 64 lanes by DPP moves (row_shr 1/2/4/8 inside each 16-lane
// row, then row_bcast:15 and row_bcast:31 across rows); lanes whose source is out of range or
// whose row is masked add the `old` operand, 0.
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return v;
}

// An integer knob from the environment: dflt when unset or outside [lo, hi].
inline int env_int(const char *name, int dflt, int lo, int hi) {
    if (const char *e = std::getenv(name)) {
        const long long v = std::atoll(e);
        if (v >= lo && v <= hi) return (int)v;
    }
    return dflt;
}

// The PageRank driver's knobs, read once at the top of each entry call (the tests flip them
// between calls of one process) and passed down; nothing below reads the environment for them.
struct PrKnobs {
    bool adaptive;       // GX_PR_KERNEL = sorted (default) | adaptive (CSR-Adaptive k_pr_pull: row-order
                         // sums, bitwise deterministic, ~3x slower)
    bool first_on;       // GX_PR_FIRST=0: every run starts with k_pr_init and a full first iteration (no cached S)
    bool fused;          // GX_PR_FUSED=0: gx_pagerank_csr uploads the whole graph before it plans
    int plan_times;      // GX_PLAN_TIMES (PlanClock::level)
    int block_rows;      // GX_PR_MULTI_BLOCK_ROWS / _NNZ: pr_multi_blocks' caps, shrunk by tests
    int block_nnz;
};
inline PrKnobs pr_knobs() {
    PrKnobs k;
    const char *e = std::getenv("GX_PR_KERNEL");
    k.adaptive = e && std::strcmp(e, "adaptive") == 0;
    k.first_on = env_int("GX_PR_FIRST", 1, 0, 1) == 1;
    k.fused = env_int("GX_PR_FUSED", 1, 0, 1) == 1;
    k.plan_times = PlanClock::level();
    k.block_rows = env_int("GX_PR_MULTI_BLOCK_ROWS", kPlanBlockRows, 1, kPlanBlockRows);
    k.block_nnz = env_int("GX_PR_MULTI_BLOCK_NNZ", (int)kPlanBlockNnz, 1, 1 << 30);
    return k;
}

// A part with its identity: whose rows (rank of nranks over n_global vertices), its exchange
// chunk and live prefix (~0: every row), and the kernel its creator lays the matrix out for.
inline std::unique_ptr<PrPart> pr_new_part(gx_ctx *ctx, uint64_t n_global, int nranks, int rank, uint64_t chunk,
                                           uint64_t live, double damping, bool force_huge, const PrKnobs &k) {
    std::unique_ptr<PrPart> p(new PrPart());
    p->ctx = ctx;
    p->n_global = n_global;
    p->nranks = nranks;
    p->rank = rank;
    p->chunk = chunk;
    p->live = live;
    p->damping = damping;
    p->force_huge = force_huge;
    p->kernel = k.adaptive ? 1 : 2;
    p->first_on = k.first_on;
    return p;
}

// Doubles of a rank's chunk: its live rows, a zero padding slot (chunk - 2) and the dangling
// slot (chunk - 1), rounded up to 32.  The exchanged vector's slots are int32 column ids.
inline uint64_t pr_chunk(uint64_t live_rows) { return (live_rows + 2 + 31) / 32 * 32; }
inline bool pr_chunk_fits(uint64_t chunk, int nranks) { return chunk * (uint64_t)nranks < (1ull << 31); }

// First position of a non-increasing out-degree sequence that holds 0 (hub-first rows: the
// dangling rows are a suffix, the rows before it the live prefix); its size when there is none.
inline uint64_t first_zero(HostView<int32_t> outdeg) {
    uint64_t lo = 0, hi = outdeg.size();
    while (lo < hi) {
        const uint64_t mid = (lo + hi) / 2;
        if (outdeg[mid] == 0) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// gx_pagerank_multi's block partition (pr_partition.block_relabel restated): the hub-first
// order cut into the single-GPU plan's blocks, dealt whole to the devices largest first (LPT);
// per device its hub-first positions in order, per hub-first position its exchange slot
// (owner * chunk + local row).
struct MultiBlocks {
    std::vector<std::vector<int32_t>> pos;
    std::vector<int32_t> slot;
    uint64_t chunk = 0;
    std::vector<int32_t> order, perm;   // the host hub-first order: position -> vertex, vertex -> position
};
int pr_multi_blocks(const gx_csr *A, int directed, int ndev, const PrKnobs &k, MultiBlocks *out);
// The interleaved partition in the same form: hub-first position h to rank h % ndev as its
// local row h / ndev (pr_partition.interleaved_relabel).
int pr_multi_interleave(const gx_csr *A, int ndev, MultiBlocks *out);

// gx_pagerank_multi's plan of device d of ndev from its copy of the graph (A' built when
// directed): hub-first positions d, d + ndev, ... as rows (or mb's blocks), columns in the
// exchange layout.
int pr_multi_plan(gx_graph *g, int ndev, int d, uint64_t chunk, double damping, const MultiBlocks *mb,
                  const PrKnobs &k, PrPart **out);
// A rank's plan from its local pull rows (h_rp from 0) with columns already in the exchange
// layout (ci), the out-degree of each row's vertex, and its live prefix (gx_pr_part_create_live).
// force_huge: plan with the whole graph's block cut (a rank of a block partition).
int pr_part_build(gx_ctx *ctx, uint64_t n_global, int nranks, int rank, uint64_t chunk, uint64_t live,
                  const std::vector<int64_t> &h_rp, const std::vector<int32_t> &ci, const std::vector<int32_t> &h_outdeg,
                  double damping, const PrKnobs &k, PrPart **out, bool force_huge = false);
// gx_pagerank_multi's partitioned upload: a rank's rows `rows` (vertex ids of A, an undirected
// graph's pull rows) picked from the host CSR A straight into the staging buffers (original
// column ids, narrowed and checked), renamed to the exchange layout by the plan's key pass
// through colmap (device, n entries: vertex -> owner * chunk + local row).
int pr_part_build_rows(gx_ctx *ctx, const gx_csr *A, int nranks, int rank, uint64_t chunk,
                       const std::vector<int32_t> &rows, const int32_t *colmap, double damping, bool force_huge,
                       const PrKnobs &k, PrPart **out);
int pr_step(PrPart *p, const double *x_full, double *x_local, double *rank_out, hipStream_t s,
            const PrScalars *ov = nullptr);

// The first iteration in closed form (PrPart::S).  A runner whose pieces all answer true to
// pr_first_alloc builds S once, outside any stream capture: pr_first_init for every piece, its
// exchange of the chunks, then pr_first_step for every piece (x_local: any chunk the runner may
// overwrite); pr_first_build is both for a plan that is its own exchange.  From then on
// pr_first starts a run: x of iteration 1 into x_local, its dangling slot included (nd_total: the
// dangling rows of all pieces), and the scores into rank_out when it is not null.
bool pr_first_alloc(PrPart *p);
int pr_first_init(PrPart *p, double *x_local, hipStream_t s);
int pr_first_step(PrPart *p, const double *x_full, double *x_local, hipStream_t s);
int pr_first_build(PrPart *p, double *x_in, double *x_out, hipStream_t s);
int pr_first(PrPart *p, uint64_t nd_total, double *x_local, double *rank_out, hipStream_t s);

}  // namespace gx

// gx_cdlp.h -- what the CDLP files share: constants, the kernels' argument block and device
// helpers, the host-side plan / step / check types.  gx_cdlp.hip is the driver (active set,
// first iteration, relabelling, cache), gx_cdlp_tiers.hip one iteration (tier and sparse
// kernels, cdlp_plan, cdlp_iteration), gx_cdlp_keep.hip the own-label check.
#pragma once

#include <cstdlib>
#include <vector>

#include "gx_device.h"

namespace gx {

constexpr int kCdlpBlock = 256;
constexpr int kLdsHash = 1024;   // slots per wave (8 KiB per wave of int32 key + int32 count)
constexpr int kLightSlots = 256; // slots per wave for light vertices of degree <= 128
constexpr uint32_t kEmpty = 0xffffffffu;

struct CdlpArgs {
    const int64_t *rpA;
    const int32_t *ciA;
    const int64_t *rpT;   // null for undirected graphs
    const int32_t *ciT;
    const int32_t *lab;
    int32_t *nxt;
    int64_t n;
    int *changed;
    int64_t v0, v1;       // vertices updated by this call (the whole graph, or one rank's range)
    // active set (gx_cdlp, from the third iteration): a vertex none of whose neighbours changed
    // label in the previous iteration keeps its label, so only vertices with act[v] == stamp
    // are recomputed, unless *dense (too many changes) or act is null (every vertex)
    const int32_t *act;
    int32_t stamp;
    const int *dense;
    // first iteration of an undirected graph: labels are still the vertex ids, so every label
    // occurs once and the result is the smallest neighbour label (the fork's
    // cdlp_first_iteration_findmin, cdlp_kernel.cu:76-116, without its directed-graph error)
    int first;
    // sparse iteration: k_cdlp_sparse_wave / _group recompute the active vertices of degree
    // <= kMidMax from the lists k_cdlp_mark built, and the tier kernels (the huge ones aside)
    // have nothing to do unless *dense
    int sparse;
    int cshards;   // *changed is cshards words kFlagStride apart (raise_flag_sharded)
    // own-label check of a dense active iteration ran (k_cdlp_keep_*): k_cdlp_tiny recomputes
    // every tiny vertex although the iteration is sparse (null: never)
    const int *keep = nullptr;
    // recount bound (gx_cdlp; null: off): the count of v's label among its neighbour entries is
    // at least vlb[v] - vchg[v] -- vlb the count when v's label was last computed, vchg the
    // changed neighbour entries k_cdlp_mark has counted since
    int32_t *vlb = nullptr;
    int32_t *vchg = nullptr;
    const int *hvalid = nullptr;   // k_cdlp_mark counted every change (the change list was complete)
};

// v's label was computed with at least c occurrences in this iteration's input.
__device__ __forceinline__ void bound_set(const CdlpArgs &a, int64_t v, uint32_t c) {
    if (a.vlb) {
        a.vlb[v] = (int32_t)c;
        a.vchg[v] = 0;
    }
}

// An active iteration whose change list was complete: v's label still holds a strict majority
// (each changed entry lowers its count by at most one), so it is the unique mode and v keeps it.
__device__ __forceinline__ bool bound_keeps(const CdlpArgs &a, int64_t v, int64_t d) {
    return a.vlb && a.sparse && *a.hvalid && 2 * ((int64_t)a.vlb[v] - a.vchg[v]) > d;
}

__device__ __forceinline__ bool tier_idle(const CdlpArgs &a) { return a.sparse && *a.dense == 0; }

__device__ __forceinline__ bool keep_on(const CdlpArgs &a) { return a.keep && *a.keep != 0; }

// Uniform per launch: whether every vertex is recomputed.
__device__ __forceinline__ bool all_active(const CdlpArgs &a) { return !a.act || *a.dense; }

__device__ __forceinline__ bool active(const CdlpArgs &a, bool all, int64_t v) { return all || a.act[v] == a.stamp; }

__device__ __forceinline__ int32_t label_at(const CdlpArgs &a, int64_t ob, int64_t od, int64_t ib,
                                            int64_t k) {
    return k < od ? a.lab[a.ciA[ob + k]] : a.lab[a.ciT[ib + (k - od)]];
}

// Where a vertex's labels come from: out-edges [ob, ob + od) of A, then in-edges [ib, ib + id)
// of A' (directed graphs).
struct VMeta {
    int64_t ob, ib;
    int32_t od, id;
};

__device__ __forceinline__ VMeta vmeta(const CdlpArgs &a, int64_t v) {
    VMeta m;
    m.ob = a.rpA[v];
    m.od = (int32_t)(a.rpA[v + 1] - m.ob);
    m.ib = 0;
    m.id = 0;
    if (a.rpT) {
        m.ib = a.rpT[v];
        m.id = (int32_t)(a.rpT[v + 1] - m.ib);
    }
    return m;
}

// An inactive vertex reads as degree 0 (no label loads; it keeps its label).
__device__ __forceinline__ VMeta vmeta_act(const CdlpArgs &a, bool all, int64_t v) {
    if (active(a, all, v)) return vmeta(a, v);
    VMeta m;
    m.ob = m.ib = 0;
    m.od = m.id = 0;
    return m;
}

__device__ __forceinline__ int32_t col_at(const CdlpArgs &a, const VMeta &m, int64_t k) {
    return k < m.od ? a.ciA[m.ob + k] : a.ciT[m.ib + (k - m.od)];
}

__device__ __forceinline__ uint32_t hash_slot(uint32_t l, int log2ts) {
    return (l * 2654435761u) >> (32 - log2ts);
}

// Adds `c` occurrences of label l to an open-addressing LDS table of 2^log2ts slots.
__device__ __forceinline__ void lds_table_add(uint32_t *K, uint32_t *C, uint32_t l, uint32_t c, int log2ts) {
    const uint32_t mask = (1u << log2ts) - 1u;
    uint32_t h = hash_slot(l, log2ts);
    for (;;) {
        const uint32_t prev = atomicCAS(&K[h], kEmpty, l);
        if (prev == kEmpty || prev == l) {
            atomicAdd(&C[h], c);
            return;
        }
        h = (h + 1) & mask;
    }
}

// Wave-uniform call (every lane of the wave reaches it; `valid` marks lanes holding a label).
// In each of kPeel rounds, the lanes whose label equals the first remaining lane's go in as
// one add of their count. The wave's most repeated labels - the common case once CDLP's labels
// start to agree - then do not serialise up to 64 same-address LDS atomics. The other lanes
// insert one at a time.
template <int kPeel = 1>
__device__ __forceinline__ void lds_table_add_wave(uint32_t *K, uint32_t *C, uint32_t l, bool valid, int log2ts) {
    const int lane = (int)(threadIdx.x & (kWave - 1));
#pragma unroll
    for (int r = 0; r < kPeel; r++) {
        const unsigned long long act = __ballot(valid);
        if (!act) return;
        const int first = __ffsll((long long)act) - 1;
        const uint32_t lead = __shfl(l, first, kWave);
        const bool same = valid && l == lead;
        const unsigned long long grp = __ballot(same);
        if (lane == first) lds_table_add(K, C, lead, (uint32_t)__popcll(grp), log2ts);
        valid = valid && !same;
    }
    if (valid) lds_table_add(K, C, l, 1u, log2ts);
}

__device__ __forceinline__ unsigned long long pack(uint32_t count, uint32_t label) {
    return ((unsigned long long)count << 32) | (unsigned long long)(kEmpty - label);
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unsigned long long o = __shfl_xor(v, off, kWave);
        v = o > v ? o : v;
    }
    return v;
}

// ---- strict-majority fast path -------------------------------------------------------
// A label held by more than half of a vertex's d neighbours is its unique most frequent
// label, so it is the CDLP result whatever the tie rule.  Boyer-Moore voting finds the only
// possible candidate in one pass; pairwise merges of (candidate, count) in any order keep it
// (each merge cancels pairs of different labels); counting the candidate exactly then
// decides.  Once CDLP labels settle, almost every vertex has such a label (SYN-7_5 from the
// third iteration on: every vertex of degree > 16, 61 % of those <= 16), and the hash table,
// the shuffle counts or the register compares are skipped.
struct Vote {
    uint32_t c;   // candidate label (kEmpty: none)
    uint32_t n;   // surplus
};

__device__ __forceinline__ Vote vote_add(Vote v, uint32_t l, bool valid) {
    if (!valid) return v;
    if (v.n == 0) return {l, 1u};
    return v.c == l ? Vote{v.c, v.n + 1u} : Vote{v.c, v.n - 1u};
}

__device__ __forceinline__ Vote vote_merge(Vote a, Vote b) {
    if (a.c == b.c) return {a.c, a.n + b.n};
    return a.n >= b.n ? Vote{a.c, a.n - b.n} : Vote{b.c, b.n - a.n};
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, (uint32_t)__shfl_xor(v, off, kWave));
    return v;
}

// Merge down to lane 0 (xor butterflies would leave different candidates in different lanes).
__device__ __forceinline__ Vote wave_vote(Vote v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        Vote o;
        o.c = __shfl_down(v.c, off, kWave);
        o.n = __shfl_down(v.n, off, kWave);
        v = vote_merge(v, o);
    }
    return v;
}

constexpr int kTiny = 32;   // k_cdlp_tiny: one thread per vertex up to this degree

// Medium-tier shapes (k_cdlp_mid, gx_cdlp_tiers.hip): 1024 threads / 16K slots (128 KiB, one workgroup
// per CU) for deg <= 8192, 512 / 8K for deg <= 4096 and 256 / 4K (32 KiB, four workgroups per
// CU) for deg <= 2048, which keeps four vertices in flight per CU for the many mid vertices
// near the bottom of the range.
constexpr int kMidBlock = 1024;
constexpr int kMidSlots = 16384;
constexpr int64_t kMidMax = kMidSlots / 2;
constexpr int kMid2Block = 256;
constexpr int kMid2Slots = 4096;
constexpr int64_t kMid2Max = kMid2Slots / 2;
constexpr int kMid4Block = 512;   // deg <= 4096: 8K slots (64 KiB), two workgroups per CU
constexpr int kMid4Slots = 8192;
constexpr int64_t kMid4Max = kMid4Slots / 2;

// The active set's lists (k_cdlp_changed / k_cdlp_mark, gx_cdlp.hip): every list is kCdlpSubs
// shards with a counter each, the counters kCntStride words apart.
constexpr int kCdlpSubs = 256;
constexpr int kCntStride = 32;             // 128 bytes between two counters
constexpr int kCdlpLists = 4;              // change chunks, then the three activation lists
constexpr int64_t kMarkChunk = 2048;
constexpr int64_t kSparseWaveMax = 512;    // wave per vertex, 1024-slot tables
constexpr int64_t kSparseG2Max = kMid2Max; // 256-thread workgroup, 4K slots
// the rest up to kMidMax: 1024-thread workgroup, 16K slots

__device__ __forceinline__ int64_t cdlp_degree(const int64_t *rpA, const int64_t *rpT, int64_t v) {
    int64_t d = rpA[v + 1] - rpA[v];
    if (rpT) d += rpT[v + 1] - rpT[v];
    return d;
}

__device__ __forceinline__ unsigned int shard_count(const unsigned int *count, int j, int64_t cap) {
    return (unsigned int)min((int64_t)count[j * kCntStride], cap);
}

// The graph CDLP runs on: the caller's (partitioned API, GX_CDLP_RELABEL=0) or its hub-first
// relabelling (gx_cdlp).  Label VALUES stay the caller's vertex ids either way, so the
// smallest-label tie rule is unchanged.
struct CdlpGraph {
    gx_ctx *ctx = nullptr;
    int64_t n = 0;
    bool directed = false;
    const int64_t *rpA = nullptr, *rpT = nullptr;
    const int32_t *ciA = nullptr, *ciT = nullptr;
    const int64_t *h_rpA = nullptr, *h_rpT = nullptr;
    int64_t nnzA = 0, nnzT = 0;
};

// Tier lists of the vertices in [v0, v1): medium vertices (LDS table per workgroup) and huge
// ones (chunked global hash segments); light vertices are found by k_cdlp_light itself.
struct CdlpPlan {
    int64_t v0 = 0, v1 = 0;
    size_t n_light = 0, n_mid2 = 0, n_mid = 0, n_huge = 0, n_chunks = 0;
    int64_t total = 0;
    DBuf<int32_t> d_hv, d_hl, d_mv, d_cvert, d_lv, d_mv2, d_sv, d_mv4;
    size_t n_small = 0, n_mid4 = 0, n_light_s = 0;
    DBuf<int32_t> d_lvs;                // light vertices with degree <= kLightSlots / 2
    DBuf<int32_t> d_wall;               // every vertex of degree <= kSparseWaveMax (sparse fallback)
    size_t n_wall = 0;
    DBuf<int64_t> d_hoff, d_cbeg;
    DBuf<unsigned long long> gtab;      // huge vertices' global tables (k_cdlp_huge_insert's words)
    uint32_t epoch = 0;                 // the last iteration's table epoch (1..kHugeEpochs)
    DBuf<unsigned long long> vkey;      // per huge vertex best key (zero between iterations)
};

// The recount bound's arrays (gx_cdlp, CdlpArgs::vlb / vchg / hvalid).
struct CdlpBound {
    int32_t *vlb, *vchg;
    int *hvalid;
};

// Switches read at every call (tests flip them within one process); unset means `dflt`.
inline bool env_on(const char *name, bool dflt = true) {
    const char *e = std::getenv(name);
    return e ? std::atoi(e) != 0 : dflt;
}

// The active vertices of a sparse iteration (k_cdlp_mark): kCdlpSubs shards of asub entries.
struct SparseLists {
    const int32_t *al;            // kCdlpLists - 1 lists of kCdlpSubs shards of asub entries
    int64_t asub;
    const unsigned int *counts;   // the change list's counters, then the three lists'
    bool only;                    // sparse-only: no tier kernels but the huge ones
    int32_t *redo;                // k_cdlp_sparse_group's vertices for the 16K-slot instance
    unsigned int *rcount;         // this iteration's redo count (zero at its start)
};

// The own-label check's edge-parallel layout of one CSR (gx_cdlp_keep.hip).
struct KeepCsr {
    DBuf<unsigned long long> bits;
    DBuf<int32_t> sne, ne;
    // column-sorted blocks (k_cdlp_keep_sorted): block b's entries are scol / srow
    // [bstart[b], bstart[b + 1]), its rows start at brow0[b]
    DBuf<int64_t> bstart;
    DBuf<int32_t> brow0, scol;
    DBuf<uint16_t> srow;
    int64_t nb = 0;
};

// The own-label check's state on a graph: the layouts of A (and A'), its counters and flags
// (keep, kover); built by the first call that needs it (keep_build).
struct CdlpKeep {
    KeepCsr A, T;
    bool sorted = false;   // A / T hold column-sorted blocks
    DBuf<uint32_t> kcnt;
    DBuf<int> kflags;
    bool built = false;
    // entries the check reads: with the hub-first copy (rows by total degree, descending) the
    // rows of degree <= kTiny, which it skips, hold every entry from here on
    int64_t nnzA = 0, nnzT = 0;
};

// gx_cdlp's per-call knobs, read once at the top of a call (cdlp_knobs, gx_cdlp.hip) and at
// every call: tests flip them within one process.  Two knobs are read where a cache is built
// instead: GX_CDLP_ASUB (cdlp_cache) and the layout half of GX_CDLP_KEEP_SORTED (keep_build).
struct CdlpKnobs {
    bool relabel;        // GX_CDLP_RELABEL: 0 never, 1 from the first call; unset: from the second
    bool active;         // GX_CDLP_ACTIVE (and more than two iterations): the active set from iteration 2
    bool first_sorted;   // GX_CDLP_FIRST_SORTED=0: iteration 0 by the tier kernels even when rows are sorted
    bool sparse;         // GX_CDLP_SPARSE=0: active vertices found by the tier kernels' act checks, not lists
    int sparse_only;     // GX_CDLP_SPARSE_ONLY: 0 idle tier launches in sparse iterations too, 1 by the flags,
                         // 2 every active iteration sparse-only (a test of the fallback lists)
    int lag;             // GX_CDLP_LAG=1: the fixed-point exit one iteration late; else two
    bool keep;           // GX_CDLP_KEEP=0: a dense active iteration runs every tier, not the own-label check
    bool keep_sorted;    // GX_CDLP_KEEP_SORTED=0: the check on slabs even where sorted blocks are built
    bool bound;          // GX_CDLP_BOUND=0: no recount bound
    int first_small;     // GX_CDLP_FIRST_SMALL = 4 / 8 (default) / 16: k_cdlp_first_dir's longest one-lane row
    int first_med;       // GX_CDLP_FIRST_MED (32; 0: off): its longest row merged by a 16-lane group
};

// What one iteration does beside the plain pass over the plan's vertices; the default is the
// partitioned API's step (every vertex, one flag word).
struct CdlpStep {
    const int32_t *act = nullptr;       // CdlpArgs::act / stamp / dense: the active set
    int32_t stamp = 0;
    const int *dense = nullptr;
    bool first = false;                 // iteration 0 on duplicate-free rows (CdlpArgs::first, undirected only)
    const SparseLists *sl = nullptr;    // a sparse iteration's lists
    int cshards = 1;                    // words of *changed (CdlpArgs::cshards)
    const int *keep = nullptr;          // the own-label check's flag (CdlpArgs::keep)
    const CdlpBound *bd = nullptr;      // the recount bound
};

// gx_cdlp_tiers.hip
int cdlp_plan(const CdlpGraph &g, int64_t v0, int64_t v1, CdlpPlan &P, hipStream_t s);
int cdlp_iteration(const CdlpGraph &g, CdlpPlan &P, const int32_t *cur, int32_t *nxt, int *changed, hipStream_t s,
                   const CdlpStep &st);

// gx_cdlp_keep.hip
int keep_build(const CdlpGraph &G, bool relabel, CdlpKeep &K, hipStream_t s);
// The check of iteration `it` on labels cur, where *dense: the own-label counts (sorted blocks
// or slabs), then apply and finish; `lists` are the iteration's counters (SparseLists::counts).
int keep_check(const CdlpGraph &G, CdlpKeep &K, bool sorted, const int32_t *cur, int *dense, int32_t *act, int32_t it,
               unsigned int *lists, int32_t *al, int64_t asub, const CdlpBound *bd, hipStream_t s);

}  // namespace gx

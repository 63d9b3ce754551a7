// gx_truss.hip -- k-truss and truss numbers (the roles of LAGraph_KTruss and LAGraph_AllKTruss).
//
// LAGraph's loop is C<C> = C*C', select >= k-2, until nothing changes.  Here the graph stays where
// it is and its edges die in place:
//   prep    : once per graph (gx_graph::truss): a row-sorted view of A (A itself when its rows are
//             sorted, else a sorted copy with every entry's original position), the row of every
//             entry, rev[e] = the position of the reverse entry (a binary search in row j; a miss
//             is the symmetry failure) and one tier byte per entry.  The entry with i < j owns its
//             edge: tier 0 = not an owner (the reverse direction, a diagonal entry), 1 / 2 / 3 = the
//             owner's work is one thread's, one wave's, one workgroup's, by the SHORTER of rows i, j.
//   state   : alive[e] (0 dead, 1 alive, 2 dying), an int32 support per entry, a dirty byte per
//             owner entry.
//   support : k_truss_list gathers the alive owners that need a count (all of them, or the dirty
//             ones) into one compact list per tier; k_truss_support<tier> counts, for the owner
//             (i, j), the columns of the shorter row that are alive there and alive in the longer
//             row (binary search), and stores the count at the entry and at its reverse.  Nobody
//             else writes an edge's count: no atomics on supports.
//   prune   : alive owners with support < k-2 turn both their entries to dying; the number leaves
//             as one atomic per wave.  The host reads it (the one readback of a round).
//   mark    : for every dying edge {u, v} the third vertices w of its triangles in the graph the
//             round started from (alive or dying in both rows) are enumerated with the same tiers,
//             and the owners of {u, w} and {v, w} get a dirty byte: plain stores of 1.  Only these
//             edges lost a triangle, so only they are recounted.  k_truss_commit then turns dying
//             into dead: the next count reads flags that no kernel is writing.  When a round
//             removed more than GX_TRUSS_SHARE percent of the alive edges the marking is skipped
//             and every alive edge is recounted.
// A round is exactly one synchronous pruning round of LAGraph's loop, whichever edges were
// recounted, so stats[2] is that loop's count.  gx_truss_all keeps flags and supports from k to
// k + 1: nothing changes between two values of k, so nothing is recounted there.
// Integers only; a result is the same bit for bit on every run.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gx_device.h"

namespace gx {
namespace {

using u64 = unsigned long long;

constexpr int kTrBlock = 256;
constexpr int kTrWaves = kTrBlock / kWave;
constexpr unsigned kTrGrid = 1024;        // cap of the entry-sweeping grids (4 workgroups per CU)
constexpr unsigned kTrItemGrid = 8192;    // cap of the work-item grids
constexpr int kTrPer = 32;                // entries per thread and tile of k_truss_list
constexpr int64_t kTrTile = (int64_t)kTrBlock * kTrPer;
// An owner whose shorter row has at most kTrussShort entries is one thread's, at most kTrussLong
// one wave's, a longer one a workgroup's (GX_TRUSS_SHORT / GX_TRUSS_LONG; mirrored in
// algorithms.py).  The first count of SYN-g500-22 takes 703 / 639 / 640 / 645 ms at 8:256 / 16:1 024 /
// 32:2 048 / 64:4 096 (profiles/ktruss_share_ab.txt); DESIGN.md section 4 "k-truss" has the reasons.
constexpr int kTrussShort = 16;
constexpr int kTrussLong = 1024;
// recount every alive edge when a round removed more than this percent of them (GX_TRUSS_SHARE).
// SYN-g500-22, gx_ktruss at k = 4 / k = kmax = 546 (rounds 1 and 2 remove 23 % / 97 % and 51 %):
// 10 1 280 / 1 283 ms, 25 775 / 1 281, 50 776 / 1 283, 75 776 / 1 225; always marked 775 / 1 755,
// always all 5 518 / 2 044 (profiles/ktruss_share_ab.txt)
constexpr int kTrussShare = 75;

static_assert(kTrWaves == 4, "the LDS reduction below takes four waves");

// counters of one round (uint32 words): the count lists per tier, the dying lists per tier, removed
enum { kCntCount = 0, kCntDying = 3, kCntRemoved = 6, kCntWords = 8 };

struct TrussView {
    const int64_t *rp;
    const int32_t *ci;     // row-sorted columns
    const int32_t *row;    // row of every entry
    const uint32_t *rev;   // position of the reverse entry
    int64_t nnz;
};

// the shorter row's entries [sb, se) (vertex sv) and the longer row's [lb, le) (vertex lv)
struct Rows {
    int64_t sb, se, lb, le;
    int32_t sv, lv;
};

__device__ __forceinline__ Rows rows_of(const TrussView &G, uint32_t e) {
    const int32_t i = G.row[e], j = G.ci[e];
    Rows r{G.rp[i], G.rp[i + 1], G.rp[j], G.rp[j + 1], i, j};
    if (r.se - r.sb > r.le - r.lb) r = Rows{r.lb, r.le, r.sb, r.se, j, i};
    return r;
}

// first position in [lo, hi) whose column is >= v
__device__ __forceinline__ int64_t lower(const int32_t *__restrict__ ci, int64_t lo, int64_t hi, int32_t v) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ci[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t wave_add_u32(uint32_t x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
    return x;
}

// The columns common to the two rows of every listed owner entry, TIER lanes wide.  F: want(k) =
// the shorter row's entry k takes part; hit(k, p, r) = its partner p in the longer row does too
// (counted when true); done(e, c) once per item with the count.
template <int TIER, class F>
__device__ __forceinline__ void tier_items(const TrussView &G, const uint32_t *__restrict__ list, uint32_t count, F f) {
    if constexpr (TIER == 1) {
        for (uint32_t x = blockIdx.x * kTrBlock + threadIdx.x; x < count; x += gridDim.x * kTrBlock) {
            const uint32_t e = list[x];
            const Rows r = rows_of(G, e);
            int32_t c = 0;
            int64_t lo = r.lb;   // both rows ascend: the search never looks back
            for (int64_t k = r.sb; k < r.se && lo < r.le; k++) {
                if (!f.want(k)) continue;
                const int32_t w = G.ci[k];
                lo = lower(G.ci, lo, r.le, w);
                if (lo < r.le && G.ci[lo] == w) c += f.hit(k, lo, r);
            }
            f.done(e, c);
        }
    } else if constexpr (TIER == 2) {
        const int lane = threadIdx.x & (kWave - 1);
        const uint32_t wave = (blockIdx.x * kTrBlock + threadIdx.x) / kWave;
        const uint32_t nwaves = gridDim.x * kTrWaves;
        for (uint32_t x = wave; x < count; x += nwaves) {
            const uint32_t e = list[x];
            const Rows r = rows_of(G, e);
            int32_t c = 0;
            for (int64_t kb = r.sb; kb < r.se; kb += kWave) {
                const int64_t k = kb + lane;
                bool h = false;
                if (k < r.se && f.want(k)) {
                    const int32_t w = G.ci[k];
                    const int64_t p = lower(G.ci, r.lb, r.le, w);
                    h = p < r.le && G.ci[p] == w && f.hit(k, p, r);
                }
                c += __popcll(__ballot(h));
            }
            if (lane == 0) f.done(e, c);
        }
    } else {
        __shared__ int32_t red[kTrWaves];
        const int lane = threadIdx.x & (kWave - 1), w4 = threadIdx.x / kWave;
        for (uint32_t x = blockIdx.x; x < count; x += gridDim.x) {
            const uint32_t e = list[x];
            const Rows r = rows_of(G, e);
            int32_t c = 0;
            for (int64_t kb = r.sb; kb < r.se; kb += kTrBlock) {
                const int64_t k = kb + threadIdx.x;
                bool h = false;
                if (k < r.se && f.want(k)) {
                    const int32_t w = G.ci[k];
                    const int64_t p = lower(G.ci, r.lb, r.le, w);
                    h = p < r.le && G.ci[p] == w && f.hit(k, p, r);
                }
                c += __popcll(__ballot(h));
            }
            if (lane == 0) red[w4] = c;
            __syncthreads();
            if (threadIdx.x == 0) f.done(e, (red[0] + red[1]) + (red[2] + red[3]));
            __syncthreads();
        }
    }
}

// support: a common column counts when its entries are alive in both rows (a diagonal entry never
// is, so neither endpoint counts as a third vertex)
struct CountF {
    const uint8_t *alive;
    int32_t *sup;
    const uint32_t *rev;
    __device__ __forceinline__ bool want(int64_t k) const { return alive[k] == 1; }
    __device__ __forceinline__ bool hit(int64_t, int64_t p, const Rows &) const { return alive[p] == 1; }
    __device__ __forceinline__ void done(uint32_t e, int32_t c) const {
        sup[e] = c;
        sup[rev[e]] = c;
    }
};

// mark: the triangle {sv, lv, w} existed when the round began (alive or dying on both sides); its
// two other edges, where they survive, lost it.  The mark goes to the edge's owner entry.
struct MarkF {
    const uint8_t *alive;
    uint8_t *dirty;
    const int32_t *ci;
    const uint32_t *rev;
    __device__ __forceinline__ bool want(int64_t k) const { return alive[k] != 0; }
    __device__ __forceinline__ bool hit(int64_t k, int64_t p, const Rows &r) const {
        if (alive[p] == 0) return false;
        const int32_t w = ci[k];
        if (alive[k] == 1) dirty[r.sv < w ? (uint32_t)k : rev[k]] = 1;
        if (alive[p] == 1) dirty[r.lv < w ? (uint32_t)p : rev[p]] = 1;
        return false;
    }
    __device__ __forceinline__ void done(uint32_t, int32_t) const {}
};

template <int TIER>
__global__ __launch_bounds__(kTrBlock) void k_truss_support(TrussView G, const uint32_t *__restrict__ list,
                                                            const uint32_t *__restrict__ count, CountF f) {
    tier_items<TIER>(G, list, *count, f);
}

template <int TIER>
__global__ __launch_bounds__(kTrBlock) void k_truss_mark(TrussView G, const uint32_t *__restrict__ list,
                                                         const uint32_t *__restrict__ count, MarkF f) {
    tier_items<TIER>(G, list, *count, f);
}

// ---- prep ----

// row[k] = i for every entry of row i (one wave per row); flags[0] raised when a row is not
// strictly ascending.
__global__ __launch_bounds__(kTrBlock) void k_truss_rows(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                         int64_t n, int32_t *__restrict__ row, int *flags) {
    const int lane = threadIdx.x & (kWave - 1);
    for (int64_t i = ((int64_t)blockIdx.x * kTrBlock + threadIdx.x) / kWave; i < n;
         i += (int64_t)gridDim.x * kTrWaves) {
        const int64_t b = rp[i], e = rp[i + 1];
        bool bad = false;
        for (int64_t k = b + lane; k < e; k += kWave) {
            row[k] = (int32_t)i;
            bad |= k > b && ci[k - 1] >= ci[k];
        }
        if (bad) raise_flag(flags);
    }
}

__global__ __launch_bounds__(kTrBlock) void k_truss_keys(const int32_t *__restrict__ row, const int32_t *__restrict__ ci,
                                                         int64_t nnz, uint64_t *__restrict__ keys,
                                                         uint32_t *__restrict__ idx) {
    for (int64_t e = (int64_t)blockIdx.x * kTrBlock + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kTrBlock) {
        keys[e] = ((uint64_t)(uint32_t)row[e] << 32) | (uint32_t)ci[e];
        idx[e] = (uint32_t)e;
    }
}

__global__ __launch_bounds__(kTrBlock) void k_truss_cols(const uint64_t *__restrict__ keys, int64_t nnz,
                                                         int32_t *__restrict__ ci) {
    for (int64_t e = (int64_t)blockIdx.x * kTrBlock + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kTrBlock)
        ci[e] = (int32_t)(uint32_t)keys[e];
}

// rev[e] for the sorted entry e = (i, j): where row j holds i.  flags[1] is raised when it does
// not (the graph is not symmetric) or when a row repeats a column; rev[e] = e then, and for a
// diagonal entry, so every later read through rev stays inside the arrays.
__global__ __launch_bounds__(kTrBlock) void k_truss_rev(TrussView G, uint32_t *__restrict__ rev, int *flags) {
    for (int64_t e = (int64_t)blockIdx.x * kTrBlock + threadIdx.x; e < G.nnz; e += (int64_t)gridDim.x * kTrBlock) {
        const int32_t i = G.row[e], j = G.ci[e];
        uint32_t r = (uint32_t)e;
        bool bad = e > G.rp[i] && G.ci[e - 1] == j;
        if (i != j) {
            const int64_t lb = G.rp[j], le = G.rp[j + 1];
            const int64_t p = lower(G.ci, lb, le, i);
            if (p < le && G.ci[p] == i) r = (uint32_t)p;
            else bad = true;
        }
        rev[e] = r;
        if (bad) raise_flag(flags + 1);
    }
}

// tier[e] (see the head of the file) and the number of owners per tier: tcount[1..3].
__global__ __launch_bounds__(kTrBlock) void k_truss_tier(TrussView G, int short_len, int long_len,
                                                         uint8_t *__restrict__ tier, uint32_t *tcount) {
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t c1 = 0, c2 = 0, c3 = 0;
    for (int64_t e = (int64_t)blockIdx.x * kTrBlock + threadIdx.x; e < G.nnz; e += (int64_t)gridDim.x * kTrBlock) {
        const int32_t i = G.row[e], j = G.ci[e];
        uint8_t t = 0;
        if (i < j) {
            const int64_t len = min(G.rp[i + 1] - G.rp[i], G.rp[j + 1] - G.rp[j]);
            t = len <= short_len ? 1 : (len <= long_len ? 2 : 3);
            c1 += t == 1;
            c2 += t == 2;
            c3 += t == 3;
        }
        tier[e] = t;
    }
    c1 = wave_add_u32(c1);
    c2 = wave_add_u32(c2);
    c3 = wave_add_u32(c3);
    if (lane == 0) {
        if (c1) atomicAdd(&tcount[1], c1);
        if (c2) atomicAdd(&tcount[2], c2);
        if (c3) atomicAdd(&tcount[3], c3);
    }
}

// ---- a call's state ----

__global__ __launch_bounds__(kTrBlock) void k_truss_init(TrussView G, uint8_t *__restrict__ alive,
                                                         uint8_t *__restrict__ dirty, int32_t *__restrict__ sup,
                                                         int32_t *__restrict__ tr) {
    for (int64_t e = (int64_t)blockIdx.x * kTrBlock + threadIdx.x; e < G.nnz; e += (int64_t)gridDim.x * kTrBlock) {
        alive[e] = G.row[e] != G.ci[e];
        dirty[e] = 0;
        sup[e] = 0;
        if (tr) tr[e] = 0;
    }
}

// The compact lists per tier (tier t's from list + off[t]; a tier's list never outgrows its
// owners): DYING = the dying owners, else the alive owners that are dirty (or all of them); the
// dirty byte of a listed owner is cleared.  A workgroup takes a tile of kTrTile entries, kTrPer per
// thread as one bit mask per tier, scans the threads' counts (three 21-bit fields of one word) and
// reserves its part of each list with one atomic per tier and tile: one per wave and 64 entries
// would be 2 M atomics on one word for SYN-g500-22's count of every edge.
template <bool DYING>
__global__ __launch_bounds__(kTrBlock) void k_truss_list(int64_t nnz, const uint8_t *__restrict__ tier,
                                                         const uint8_t *__restrict__ alive, uint8_t *__restrict__ dirty,
                                                         bool all, uint32_t off2, uint32_t off3,
                                                         uint32_t *__restrict__ list, uint32_t *cnt) {
    __shared__ u64 wtot[kTrWaves];
    __shared__ uint32_t base[3];
    constexpr u64 kField = (1ull << 21) - 1;
    static_assert(kTrTile <= (int64_t)kField, "a tile's count fits a field");
    const int lane = threadIdx.x & (kWave - 1), w4 = threadIdx.x / kWave;
    for (int64_t t0 = (int64_t)blockIdx.x * kTrTile; t0 < nnz; t0 += (int64_t)gridDim.x * kTrTile) {
        uint32_t m1 = 0, m2 = 0, m3 = 0;
#pragma unroll 4
        for (int j = 0; j < kTrPer; j++) {
            const int64_t e = t0 + (int64_t)j * kTrBlock + threadIdx.x;
            uint8_t t = 0;
            if (e < nnz) {
                t = tier[e];
                if (t) {
                    const uint8_t a = alive[e];
                    if (DYING) {
                        if (a != 2) t = 0;
                    } else if (a != 1) {
                        t = 0;
                    } else if (dirty[e]) {
                        dirty[e] = 0;
                    } else if (!all) {
                        t = 0;
                    }
                }
            }
            m1 |= (uint32_t)(t == 1) << j;
            m2 |= (uint32_t)(t == 2) << j;
            m3 |= (uint32_t)(t == 3) << j;
        }
        const u64 mine = (u64)__popc(m1) | ((u64)__popc(m2) << 21) | ((u64)__popc(m3) << 42);
        u64 x = mine;   // inclusive scan over the wave
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const u64 y = __shfl_up(x, off, kWave);
            if (lane >= off) x += y;
        }
        if (lane == kWave - 1) wtot[w4] = x;
        __syncthreads();
        if (threadIdx.x == 0) {
            const u64 tot = (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
            const uint32_t c1 = (uint32_t)(tot & kField), c2 = (uint32_t)((tot >> 21) & kField), c3 = (uint32_t)(tot >> 42);
            base[0] = c1 ? atomicAdd(cnt + 0, c1) : 0;
            base[1] = c2 ? atomicAdd(cnt + 1, c2) : 0;
            base[2] = c3 ? atomicAdd(cnt + 2, c3) : 0;
        }
        __syncthreads();
        u64 before = x - mine;
        for (int k = 0; k < w4; k++) before += wtot[k];
        uint32_t p1 = base[0] + (uint32_t)(before & kField);
        uint32_t p2 = off2 + base[1] + (uint32_t)((before >> 21) & kField);
        uint32_t p3 = off3 + base[2] + (uint32_t)(before >> 42);
        const uint32_t e0 = (uint32_t)t0 + threadIdx.x;   // nnz < 2^32
        for (; m1; m1 &= m1 - 1) list[p1++] = e0 + (uint32_t)(__ffs(m1) - 1) * kTrBlock;
        for (; m2; m2 &= m2 - 1) list[p2++] = e0 + (uint32_t)(__ffs(m2) - 1) * kTrBlock;
        for (; m3; m3 &= m3 - 1) list[p3++] = e0 + (uint32_t)(__ffs(m3) - 1) * kTrBlock;
        __syncthreads();   // wtot and base are the next tile's too
    }
}

// Alive owners with support < need: both entries dying.  An owner reads and writes its own two
// entries only.
__global__ __launch_bounds__(kTrBlock) void k_truss_prune(int64_t nnz, const uint8_t *__restrict__ tier,
                                                          uint8_t *__restrict__ alive, const int32_t *__restrict__ sup,
                                                          const uint32_t *__restrict__ rev, int64_t need,
                                                          uint32_t *removed) {
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t c = 0;
    for (int64_t e = (int64_t)blockIdx.x * kTrBlock + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kTrBlock) {
        if (tier[e] && alive[e] == 1 && (int64_t)sup[e] < need) {
            alive[e] = 2;
            alive[rev[e]] = 2;
            c++;
        }
    }
    c = wave_add_u32(c);
    if (lane == 0 && c) atomicAdd(removed, c);
}

// dying -> dead; gx_truss_all records the truss number of what died while pruning for k.
__global__ __launch_bounds__(kTrBlock) void k_truss_commit(int64_t nnz, uint8_t *__restrict__ alive,
                                                           int32_t *__restrict__ tr, int32_t number) {
    for (int64_t e = (int64_t)blockIdx.x * kTrBlock + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kTrBlock) {
        if (alive[e] == 2) {
            alive[e] = 0;
            if (tr) tr[e] = number;
        }
    }
}

// sum of the alive owners' supports = 3 x the triangles of what is left
__global__ __launch_bounds__(kTrBlock) void k_truss_sum(int64_t nnz, const uint8_t *__restrict__ tier,
                                                        const uint8_t *__restrict__ alive, const int32_t *__restrict__ sup,
                                                        u64 *total) {
    const int lane = threadIdx.x & (kWave - 1);
    u64 c = 0;
    for (int64_t e = (int64_t)blockIdx.x * kTrBlock + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kTrBlock)
        if (tier[e] && alive[e] == 1) c += (u64)sup[e];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, kWave);
    if (lane == 0 && c) atomicAdd(total, c);
}

// back to A's entry order: the support of an alive entry or -1 / the truss number
__global__ __launch_bounds__(kTrBlock) void k_truss_out(int64_t nnz, const uint32_t *__restrict__ pos,
                                                        const uint8_t *__restrict__ alive, const int32_t *__restrict__ val,
                                                        int64_t *__restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * kTrBlock + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kTrBlock) {
        const int64_t v = alive ? (alive[e] == 1 ? (int64_t)val[e] : -1) : (int64_t)val[e];
        out[pos ? pos[e] : (uint32_t)e] = v;
    }
}

// What a graph keeps between calls (gx_graph::truss).
struct TrussCache {
    DBuf<int32_t> ci_sorted, row;   // ci_sorted stays empty when A's rows are sorted
    DBuf<uint32_t> pos, rev;        // pos likewise: a sorted entry's position in A
    const int32_t *ci = nullptr;
    DBuf<uint8_t> tier, alive, dirty;
    DBuf<int32_t> sup, tr;
    DBuf<uint32_t> list, cnt, tcount;
    DBuf<u64> total;
    int short_len = -1, long_len = -1;   // what tier was built with
    uint32_t owners[4] = {0, 0, 0, 0};   // per tier
    uint64_t edges = 0;
};

struct TrussKnobs {
    int short_len = kTrussShort, long_len = kTrussLong, share = kTrussShare;
    int form = 0;   // 0 by the share, 1 recount all, 2 recount the marked
    bool verbose = false;
};

// The only place that reads a knob, once per call.
TrussKnobs truss_knobs() {
    TrussKnobs k;
    if (const char *e = std::getenv("GX_TRUSS_SHORT")) k.short_len = std::max(1, std::atoi(e));
    if (const char *e = std::getenv("GX_TRUSS_LONG")) k.long_len = std::atoi(e);
    k.long_len = std::max(k.long_len, k.short_len);
    if (const char *e = std::getenv("GX_TRUSS_SHARE")) k.share = std::min(100, std::max(0, std::atoi(e)));
    if (const char *e = std::getenv("GX_TRUSS_RECOUNT"))
        k.form = std::strcmp(e, "all") == 0 ? 1 : (std::strcmp(e, "marked") == 0 ? 2 : 0);
    k.verbose = std::getenv("GX_TRUSS_VERBOSE") != nullptr;
    return k;
}

// One gx_ktruss / gx_truss_all call and its stages, in the order the entry points run them.
struct TrussCall {
    gx_graph *g;
    const char *fn;
    TrussKnobs kn;
    gx_ctx *ctx;
    hipStream_t s;
    int64_t nnz;
    TrussCache *C = nullptr;
    TrussView G{};
    uint32_t off[4] = {0, 0, 0, 0};   // tier t's list starts at off[t]
    uint64_t alive_edges = 0;
    enum class Need { None, Marked, All } need = Need::All;   // what the next count takes

    TrussCall(gx_graph *g_, const char *fn_)
        : g(g_), fn(fn_), kn(truss_knobs()), ctx(g_->ctx), s(g_->ctx->stream), nnz((int64_t)g_->nnz) {}

    unsigned sweep_grid() const { return grid_for((uint64_t)nnz, kTrBlock, kTrGrid); }
    unsigned list_grid() const { return grid_for((uint64_t)nnz, (int)kTrTile, kTrGrid); }

    // Stage 1: the cache.  Built on the first call; only the tier bytes depend on a knob.
    int prep() {
        C = static_cast<TrussCache *>(g->truss.get());
        if (!C) {
            auto fresh = std::make_shared<TrussCache>();
            GX_TRY(build(*fresh));
            g->truss = fresh;
            C = fresh.get();
        }
        G = TrussView{g->A.rp.p, C->ci, C->row.p, C->rev.p, nnz};
        if (C->short_len != kn.short_len || C->long_len != kn.long_len) GX_TRY(build_tiers());
        off[1] = 0;
        off[2] = C->owners[1];
        off[3] = C->owners[1] + C->owners[2];
        return GX_SUCCESS;
    }

    int build(TrussCache &c) {
        const int64_t n = (int64_t)g->n;
        int *h_flags = static_cast<int *>(ctx->staging[0]);
        DBuf<int> flags;
        GX_TRY(flags.alloc(2));
        GX_TRY(c.row.alloc(nnz));
        GX_TRY(c.rev.alloc(nnz));
        GX_HIP_TRY(hipMemsetAsync(flags.p, 0, 2 * sizeof(int), s));
        hipLaunchKernelGGL(k_truss_rows, dim3(grid_for((uint64_t)n * kWave, kTrBlock, kTrItemGrid)), dim3(kTrBlock), 0, s,
                           g->A.rp.p, g->A.ci.p, n, c.row.p, flags.p);
        GX_TRY(check_launch("k_truss_rows"));
        GX_HIP_TRY(hipMemcpyAsync(h_flags, flags.p, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
        GX_HIP_TRY(hipStreamSynchronize(s));
        if (h_flags[0] == 0) {
            c.ci = g->A.ci.p;
        } else {   // a sorted copy, as gx_mxm_masked makes it; the rows keep their lengths
            DBuf<uint64_t> k0, k1;
            DBuf<uint32_t> i0;
            GX_TRY(k0.alloc(nnz));
            GX_TRY(k1.alloc(nnz));
            GX_TRY(i0.alloc(nnz));
            GX_TRY(c.pos.alloc(nnz));
            GX_TRY(c.ci_sorted.alloc(nnz, 16));
            hipLaunchKernelGGL(k_truss_keys, dim3(sweep_grid()), dim3(kTrBlock), 0, s, c.row.p, g->A.ci.p, nnz, k0.p, i0.p);
            GX_TRY(check_launch("k_truss_keys"));
            int bits = 1;
            while ((1ull << bits) < (uint64_t)n) bits++;
            GX_TRY(sort_pairs_u64_u32(k0.p, k1.p, i0.p, c.pos.p, (size_t)nnz, 32 + bits, s));
            hipLaunchKernelGGL(k_truss_cols, dim3(sweep_grid()), dim3(kTrBlock), 0, s, k1.p, nnz, c.ci_sorted.p);
            GX_TRY(check_launch("k_truss_cols"));
            GX_HIP_TRY(hipStreamSynchronize(s));   // the temporaries go out of scope here
            c.ci = c.ci_sorted.p;
        }
        const TrussView V{g->A.rp.p, c.ci, c.row.p, c.rev.p, nnz};
        hipLaunchKernelGGL(k_truss_rev, dim3(sweep_grid()), dim3(kTrBlock), 0, s, V, c.rev.p, flags.p);
        GX_TRY(check_launch("k_truss_rev"));
        GX_HIP_TRY(hipMemcpyAsync(h_flags, flags.p, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
        GX_HIP_TRY(hipStreamSynchronize(s));
        if (h_flags[1])
            return fail(GX_INVALID_VALUE, std::string(fn) + ": a stored (i, j) without its (j, i), or a repeated column; "
                                                            "the graph must be undirected with both directions stored");
        GX_TRY(c.tier.alloc(nnz));
        GX_TRY(c.alive.alloc(nnz));
        GX_TRY(c.dirty.alloc(nnz));
        GX_TRY(c.sup.alloc(nnz));
        GX_TRY(c.cnt.alloc(kCntWords));
        GX_TRY(c.tcount.alloc(4));
        GX_TRY(c.total.alloc(1));
        return GX_SUCCESS;
    }

    int build_tiers() {
        uint32_t *h = static_cast<uint32_t *>(ctx->staging[0]);
        GX_HIP_TRY(hipMemsetAsync(C->tcount.p, 0, 4 * sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_truss_tier, dim3(sweep_grid()), dim3(kTrBlock), 0, s, G, kn.short_len, kn.long_len,
                           C->tier.p, C->tcount.p);
        GX_TRY(check_launch("k_truss_tier"));
        GX_HIP_TRY(hipMemcpyAsync(h, C->tcount.p, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        GX_HIP_TRY(hipStreamSynchronize(s));
        C->edges = 0;
        for (int t = 1; t <= 3; t++) {
            C->owners[t] = h[t];
            C->edges += h[t];
        }
        if (C->edges * 2 > (uint64_t)nnz) return fail(GX_PANIC, std::string(fn) + ": more owners than half the entries");
        if (C->list.n < C->edges) GX_TRY(C->list.alloc(C->edges));
        C->short_len = kn.short_len;
        C->long_len = kn.long_len;
        return GX_SUCCESS;
    }

    // Stage 2: every edge alive, nothing counted yet.
    int start(bool numbers) {
        if (numbers && C->tr.n < (size_t)nnz) GX_TRY(C->tr.alloc(nnz));
        hipLaunchKernelGGL(k_truss_init, dim3(sweep_grid()), dim3(kTrBlock), 0, s, G, C->alive.p, C->dirty.p, C->sup.p,
                           numbers ? C->tr.p : nullptr);
        GX_TRY(check_launch("k_truss_init"));
        alive_edges = C->edges;
        need = Need::All;
        return GX_SUCCESS;
    }

    unsigned item_grid(int t, uint64_t items) const {
        if (t == 1) return grid_for(items, kTrBlock, kTrItemGrid);
        if (t == 2) return grid_for(items * kWave, kTrBlock, kTrItemGrid);
        return (unsigned)std::min<uint64_t>(std::max<uint64_t>(items, 1), kTrItemGrid);
    }

    // The counts that are due: the lists, then one kernel per tier that owns an edge at all.
    int count() {
        if (need == Need::None) return GX_SUCCESS;
        KTimer kt(ctx, "truss_support", s);
        uint32_t *cnt = C->cnt.p + kCntCount;
        hipLaunchKernelGGL(k_truss_list<false>, dim3(list_grid()), dim3(kTrBlock), 0, s, nnz, C->tier.p, C->alive.p,
                           C->dirty.p, need == Need::All, off[2], off[3], C->list.p, cnt);
        const CountF f{C->alive.p, C->sup.p, C->rev.p};
        const uint64_t cap = alive_edges;   // no list is longer than what is alive
        if (C->owners[1])
            hipLaunchKernelGGL(k_truss_support<1>, dim3(item_grid(1, std::min<uint64_t>(C->owners[1], cap))),
                               dim3(kTrBlock), 0, s, G, C->list.p + off[1], cnt + 0, f);
        if (C->owners[2])
            hipLaunchKernelGGL(k_truss_support<2>, dim3(item_grid(2, std::min<uint64_t>(C->owners[2], cap))),
                               dim3(kTrBlock), 0, s, G, C->list.p + off[2], cnt + 1, f);
        if (C->owners[3])
            hipLaunchKernelGGL(k_truss_support<3>, dim3(item_grid(3, std::min<uint64_t>(C->owners[3], cap))),
                               dim3(kTrBlock), 0, s, G, C->list.p + off[3], cnt + 2, f);
        need = Need::None;
        return check_launch("k_truss_support");
    }

    // One synchronous round for k: count what is due, prune, read the round's counters (the one
    // readback), then mark and commit.  *removed = the edges the round took.
    int round(uint32_t k, int round_no, uint64_t *removed) {
        uint32_t *h = static_cast<uint32_t *>(ctx->staging[0]);
        GX_HIP_TRY(hipMemsetAsync(C->cnt.p, 0, kCntWords * sizeof(uint32_t), s));
        GX_TRY(count());
        {
            KTimer kt(ctx, "truss_prune", s);
            hipLaunchKernelGGL(k_truss_prune, dim3(sweep_grid()), dim3(kTrBlock), 0, s, nnz, C->tier.p, C->alive.p,
                               C->sup.p, C->rev.p, (int64_t)k - 2, C->cnt.p + kCntRemoved);
            GX_TRY(check_launch("k_truss_prune"));
        }
        GX_HIP_TRY(hipMemcpyAsync(h, C->cnt.p, kCntWords * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        GX_HIP_TRY(hipStreamSynchronize(s));
        const uint64_t gone = h[kCntRemoved];
        if (gone > alive_edges) return fail(GX_PANIC, std::string(fn) + ": a round removed more edges than were alive");
        const bool all = kn.form == 1 || (kn.form == 0 && gone * 100 > alive_edges * (uint64_t)kn.share);
        if (kn.verbose)
            std::fprintf(stderr, "%s: k %u round %d alive %llu recounted %llu removed %llu next %s\n", fn, k, round_no,
                         (u64)alive_edges, (u64)h[0] + h[1] + h[2], (u64)gone, !gone ? "-" : all ? "all" : "marked");
        *removed = gone;
        if (!gone) return GX_SUCCESS;
        if (!all) GX_TRY(mark(gone));
        alive_edges -= gone;
        need = all ? Need::All : Need::Marked;
        return GX_SUCCESS;
    }

    // The edges that lose a triangle to the `gone` dying ones.
    int mark(uint64_t gone) {
        KTimer kt(ctx, "truss_mark", s);
        uint32_t *cnt = C->cnt.p + kCntDying;
        hipLaunchKernelGGL(k_truss_list<true>, dim3(list_grid()), dim3(kTrBlock), 0, s, nnz, C->tier.p, C->alive.p,
                           C->dirty.p, false, off[2], off[3], C->list.p, cnt);
        const MarkF f{C->alive.p, C->dirty.p, C->ci, C->rev.p};
        const uint64_t cap = gone;
        if (C->owners[1])
            hipLaunchKernelGGL(k_truss_mark<1>, dim3(item_grid(1, std::min<uint64_t>(C->owners[1], cap))), dim3(kTrBlock),
                               0, s, G, C->list.p + off[1], cnt + 0, f);
        if (C->owners[2])
            hipLaunchKernelGGL(k_truss_mark<2>, dim3(item_grid(2, std::min<uint64_t>(C->owners[2], cap))), dim3(kTrBlock),
                               0, s, G, C->list.p + off[2], cnt + 1, f);
        if (C->owners[3])
            hipLaunchKernelGGL(k_truss_mark<3>, dim3(item_grid(3, std::min<uint64_t>(C->owners[3], cap))), dim3(kTrBlock),
                               0, s, G, C->list.p + off[3], cnt + 2, f);
        return check_launch("k_truss_mark");
    }

    int commit(int32_t number) {
        KTimer kt(ctx, "truss_commit", s);
        hipLaunchKernelGGL(k_truss_commit, dim3(sweep_grid()), dim3(kTrBlock), 0, s, nnz, C->alive.p,
                           number ? C->tr.p : nullptr, number);
        return check_launch("k_truss_commit");
    }

    // Stage 3: rounds for k until one removes nothing.  *rounds counts those that removed an edge.
    // The supports are exact on leaving (need == None), also when the last edge has gone.
    int fixed_point(uint32_t k, bool numbers, uint64_t *rounds) {
        for (int r = 1;; r++) {
            uint64_t gone = 0;
            GX_TRY(round(k, r, &gone));
            if (!gone) return GX_SUCCESS;
            GX_TRY(commit(numbers ? (int32_t)(k - 1) : 0));
            (*rounds)++;
            if (alive_edges == 0) {
                need = Need::None;
                return GX_SUCCESS;
            }
        }
    }

    // Stage 4: the sum of the supports (3 x the triangles left).
    int triangles(uint64_t *out) {
        u64 *h = static_cast<u64 *>(ctx->staging[0]);
        GX_HIP_TRY(hipMemsetAsync(C->total.p, 0, sizeof(u64), s));
        hipLaunchKernelGGL(k_truss_sum, dim3(sweep_grid()), dim3(kTrBlock), 0, s, nnz, C->tier.p, C->alive.p, C->sup.p,
                           C->total.p);
        GX_TRY(check_launch("k_truss_sum"));
        GX_HIP_TRY(hipMemcpyAsync(h, C->total.p, sizeof(u64), hipMemcpyDeviceToHost, s));
        GX_HIP_TRY(hipStreamSynchronize(s));
        *out = (uint64_t)(h[0] / 3);
        return GX_SUCCESS;
    }

    // Stage 5: the per-entry result in A's entry order (supports with -1 for the dead, or the
    // truss numbers), into a buffer the caller allocated before the device bracket.
    int scatter(bool numbers, int64_t *d_out) {
        hipLaunchKernelGGL(k_truss_out, dim3(sweep_grid()), dim3(kTrBlock), 0, s, nnz, C->pos.n ? C->pos.p : nullptr,
                           numbers ? nullptr : C->alive.p, numbers ? C->tr.p : C->sup.p, d_out);
        return check_launch("k_truss_out");
    }
};

// The checks both entry points share; GX_SUCCESS with *empty set: nothing to compute.
int truss_enter(gx_graph *g, const char *fn, bool *empty) {
    if (g->directed) return fail(GX_INVALID_VALUE, std::string(fn) + ": the graph is directed");
    if (g->nnz >= (1ull << 32)) return fail(GX_NOT_IMPLEMENTED, std::string(fn) + ": 2^32 entries or more");
    *empty = g->nnz == 0;
    return GX_SUCCESS;
}

}  // namespace
}  // namespace gx

using namespace gx;

extern "C" int gx_ktruss(gx_graph *g, uint32_t k, int64_t *support, uint64_t *stats) {
    if (!g || (!support && !stats)) return fail(GX_NULL_POINTER, "gx_ktruss: null argument");
    if (k < 2) return fail(GX_INVALID_VALUE, "gx_ktruss: k < 2");
    bool empty = false;
    GX_TRY(truss_enter(g, "gx_ktruss", &empty));
    if (empty) {
        if (stats) stats[0] = stats[1] = stats[2] = 0;
        return GX_SUCCESS;
    }
    gx_ctx *ctx = g->ctx;
    GX_HIP_TRY(hipSetDevice(ctx->device));
    TrussCall c(g, "gx_ktruss");
    DBuf<int64_t> d_out;
    if (support) GX_TRY(d_out.alloc(c.nnz));
    GX_TRY(device_begin(ctx));
    GX_TRY(c.prep());
    GX_TRY(c.start(false));
    uint64_t rounds = 0, tri = 0;
    GX_TRY(c.fixed_point(k, false, &rounds));
    if (stats) GX_TRY(c.triangles(&tri));
    if (support) GX_TRY(c.scatter(false, d_out.p));
    GX_TRY(device_end(ctx));
    if (support) GX_TRY(download(ctx, support, d_out.p, (uint64_t)c.nnz, Xfer::Raw64));
    if (stats) {
        stats[0] = c.alive_edges;
        stats[1] = tri;
        stats[2] = rounds;
    }
    return GX_SUCCESS;
}

extern "C" int gx_truss_all(gx_graph *g, int64_t *truss, uint64_t *kmax) {
    if (!g || (!truss && !kmax)) return fail(GX_NULL_POINTER, "gx_truss_all: null argument");
    bool empty = false;
    GX_TRY(truss_enter(g, "gx_truss_all", &empty));
    if (empty) {
        if (kmax) *kmax = 0;
        return GX_SUCCESS;
    }
    gx_ctx *ctx = g->ctx;
    GX_HIP_TRY(hipSetDevice(ctx->device));
    TrussCall c(g, "gx_truss_all");
    DBuf<int64_t> d_out;
    if (truss) GX_TRY(d_out.alloc(c.nnz));
    GX_TRY(device_begin(ctx));
    GX_TRY(c.prep());
    GX_TRY(c.start(true));
    // what dies while pruning for k was in the (k-1)-truss and is in no larger one
    uint64_t rounds = 0, top = 0;
    for (uint32_t k = 3; c.alive_edges > 0; k++) {
        const uint64_t before = rounds;
        GX_TRY(c.fixed_point(k, true, &rounds));
        if (rounds != before) top = k - 1;
    }
    if (truss) GX_TRY(c.scatter(true, d_out.p));
    GX_TRY(device_end(ctx));
    if (truss) GX_TRY(download(ctx, truss, d_out.p, (uint64_t)c.nnz, Xfer::Raw64));
    if (kmax) *kmax = top;
    return GX_SUCCESS;
}

GX_MODULE_WARMER(truss)

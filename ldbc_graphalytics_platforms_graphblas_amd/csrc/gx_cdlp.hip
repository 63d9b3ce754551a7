// gx_cdlp.hip -- community detection by synchronous label propagation (Graphalytics CDLP).
//
// Replaces LAGraph_cdlp (cdlp.cpp:54-67; semantics LAGraph_cdlp.c:37-121) and the fork's
// CUDA_CDLP::LAGraph_cdlp_gpu (cdlp_cuda.cu:118-251, kernels cdlp_kernel.cu:449-1140).
// Every iteration each vertex takes min(argmax_l #neighbour labels == l) over its
// out-neighbours and, for directed graphs, its in-neighbours too (a reciprocal edge counts
// twice, LAGraph_cdlp.c:47-50).  A vertex without neighbours keeps its label.
// Unlike the reference CUDA kernels this is exact and deterministic: counts are built with
// atomics that never lose an update (the reference's LDS insert is unlocked,
// cdlp_kernel.cu:685-694), in-edges are included for directed graphs, and degree-0 vertices
// are written (cdlp_kernel.cu:108-112, 1060-1063).
//   deg <= 32        : one thread per vertex, labels in registers (vote, else a register sort).
//   deg <= 64        : one wave per vertex, labels in registers, counts by ballots.
//   deg <= kLdsHash/2: one wave per vertex, open-addressing hash table in that wave's LDS
//   (kLightSlots slots for deg <= kLightSlots/2, kLdsHash slots above).
//   deg <= 2048      : one 256-thread workgroup per vertex, 4K-slot LDS table (4 per CU).
//   deg <= 4096      : one 512-thread workgroup per vertex, 8K-slot LDS table (2 per CU).
//   deg <= 8192      : one 1024-thread workgroup per vertex, 16K-slot hash table in LDS
//                      (workgroups loop over the medium-vertex list, one per CU).
//   larger           : 4096-label chunks histogrammed in LDS by separate workgroups, merged
//                      into a per-vertex global table (2*deg slots, cleared per iteration),
//                      then one reduce workgroup per vertex.
// The winner is the maximum of the 64-bit key (count << 32) | ~label, i.e. the highest
// count and among equal counts the smallest label.
//
// This file is the driver: the active-set kernels, the first-iteration shortcuts, the row-order
// check, the relabelled copy, the cache on the graph, gx_cdlp and the partitioned entry points.
// One iteration's kernels and launches are gx_cdlp_tiers.hip, the own-label check gx_cdlp_keep.hip,
// what they share gx_cdlp.h.
#include <algorithm>
#include <cstdlib>
#include <memory>
#include <vector>

#include "gx_cdlp.h"

using namespace gx;

namespace gx {
namespace {

__global__ void k_cdlp_fill_u32(uint32_t *p, uint32_t v, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        p[i] = v;
}

// The iteration's changed flag to pinned host memory: one lane's store over PCIe, instead of a
// 4-byte hipMemcpyAsync, which ran as a ~40 us blit kernel (profiles/r01_cdlp_kernel_stats.csv).
// Bit 0: a label changed; bit 1: the iteration's active set overflowed (*dense).
__global__ void k_cdlp_flag_out(const int *__restrict__ changed, int shards, const int *dense, int *hflag) {
    const int t = threadIdx.x;   // one lane per shard (shards <= kWave)
    const bool set = t < shards && changed[t * kFlagStride] != 0;
    const bool any = __ballot(set) != 0;
    if (t == 0) *hflag = (any ? 1 : 0) | (dense && *dense ? 2 : 0);
}

// Active set of the next iteration (gx_cdlp).  k_cdlp_changed lists the vertices whose label
// changed in the last iteration (prev != cur), as chunks of kMarkChunk neighbours, and sets
// prev = cur for them: prev (the buffer the iteration writes) then equals cur everywhere, so
// a sparse iteration writes only its active vertices.  k_cdlp_mark gives every in- and
// out-neighbour in a listed chunk act = stamp and appends each newly marked vertex of degree
// <= kMidMax to one of three lists by degree (<= 512, <= 2048, <= 8192), which
// k_cdlp_sparse_wave / k_cdlp_sparse_group recompute; huge vertices keep their tier kernels,
// which skip inactive ones.  SYN-7_5 from the fifth iteration on: ~500 changes and ~780 active
// vertices (3 % of the entries).
// Every list is kCdlpSubs shards with a counter each, the counters kCntStride words apart:
// device-scope atomics on one address serialise (one counter for all: ~23 K wave atomics,
// ~700 us on SYN-cit), and so do counters that share a 128-byte line.  An overflowing shard
// sets *dense, and the tier kernels recompute every vertex.
// Shard j of a list is read by the waves (workgroups) w with w % kCdlpSubs == j: every
// shard gets the same share of the grid (a whole-grid sweep of each shard in turn left all
// but a few waves idle and cost a dependent-load chain per shard: ~120 us on SYN-7_5).
// One reservation per workgroup and 256 vertices.
__global__ __launch_bounds__(256) void k_cdlp_changed(int32_t *__restrict__ prev, const int32_t *__restrict__ cur,
                                                      const int64_t *__restrict__ rpA, const int64_t *__restrict__ rpT,
                                                      int64_t n, uint64_t *list, int64_t sub, unsigned int *count,
                                                      int *dense) {
    __shared__ uint32_t wtot[256 / kWave];
    __shared__ uint32_t bbase;
    const int lane = threadIdx.x & (kWave - 1);
    const int wv = threadIdx.x / kWave;
    if (blockIdx.x == 0 && threadIdx.x == 0) *dense = 0;   // k_cdlp_mark only ever raises it
    for (int64_t b0 = (int64_t)blockIdx.x * 256; b0 < n; b0 += (int64_t)gridDim.x * 256) {
        const int64_t v = b0 + threadIdx.x;
        const int32_t cv = v < n ? cur[v] : 0;
        const bool ch = v < n && prev[v] != cv;
        if (ch) prev[v] = cv;
        const uint32_t chunks = ch ? (uint32_t)((cdlp_degree(rpA, rpT, v) + kMarkChunk - 1) / kMarkChunk) : 0u;
        uint32_t pre = chunks;   // inclusive prefix within the wave
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const uint32_t t = __shfl_up(pre, off, kWave);
            if (lane >= off) pre += t;
        }
        if (lane == kWave - 1) wtot[wv] = pre;
        pre -= chunks;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 256 / kWave; w++) {
            const uint32_t t = wtot[w];
            before += w < wv ? t : 0u;
            total += t;
        }
        if (total) {
            if (threadIdx.x == 0) {
                const int j = (int)((b0 / 256) % kCdlpSubs);
                unsigned int *cnt = count + j * kCntStride;
                // past capacity only the overflow matters: stop adding
                unsigned int base = __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (base <= (unsigned int)sub) base = atomicAdd(cnt, total);
                bbase = base;
            }
            __syncthreads();
            const unsigned int base = bbase + before + pre;
            const int j = (int)((b0 / 256) % kCdlpSubs);
            for (uint32_t c = 0; c < chunks; c++)
                if (base + c < (unsigned int)sub) list[(int64_t)j * sub + base + c] = ((uint64_t)v << 32) | c;
        }
        __syncthreads();   // wtot and bbase are free again
    }
}

// One wave per listed chunk; appends go to shard (wave index mod kCdlpSubs) of their list, one
// reservation per wave, list and 64 neighbours.
__global__ __launch_bounds__(256) void k_cdlp_mark(const int64_t *__restrict__ rpA, const int32_t *__restrict__ ciA,
                                                   const int64_t *__restrict__ rpT, const int32_t *__restrict__ ciT,
                                                   const uint64_t *__restrict__ list, int64_t sub,
                                                   unsigned int *counts, int32_t *act, int32_t stamp, int *dense,
                                                   int32_t *al, int64_t asub, int32_t *vchg, int *hvalid) {
    __shared__ int over;
    if (threadIdx.x == 0) over = 0;
    __syncthreads();
    if (counts[threadIdx.x * kCntStride] > (unsigned int)sub) over = 1;   // kCdlpSubs == blockDim.x
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0 && hvalid) *hvalid = over ? 0 : 1;
    if (over) {
        if (blockIdx.x == 0 && threadIdx.x == 0) *dense = 1;
        return;
    }
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t gw = ((int64_t)blockIdx.x * 256 + threadIdx.x) / kWave;
    const int64_t nw = (int64_t)gridDim.x * (256 / kWave);   // a multiple of kCdlpSubs
    const int j = (int)(gw % kCdlpSubs);
    const int64_t c = counts[j * kCntStride];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t i = gw / kCdlpSubs; i < c; i += nw / kCdlpSubs) {
        const uint64_t e = list[(int64_t)j * sub + i];
        const int64_t u = (int64_t)(e >> 32);
        const int64_t ob = rpA[u], od = rpA[u + 1] - ob;
        const int64_t ib = rpT ? rpT[u] : 0, id = rpT ? rpT[u + 1] - ib : 0;
        const int64_t k0 = (int64_t)(uint32_t)e * kMarkChunk, k1 = min(k0 + kMarkChunk, od + id);
        for (int64_t kb = k0; kb < k1; kb += kWave) {
            const int64_t k = kb + lane;
            int64_t w = -1;
            if (k < k1) w = k < od ? ciA[ob + k] : ciT[ib + (k - od)];
            const bool fresh = w >= 0 && atomicExch(&act[w], stamp) != stamp;
            // the recount bound: every changed neighbour entry of w
            if (vchg && w >= 0) atomicAdd(&vchg[w], 1);
            const int64_t dw = fresh ? cdlp_degree(rpA, rpT, w) : 0;
            // activation list 1 + L: L = 0 (wave), 1 (256-thread group), 2 (1024-thread group)
            const int L = !fresh || dw > kMidMax ? -1 : dw <= kSparseWaveMax ? 0 : dw <= kSparseG2Max ? 1 : 2;
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const unsigned long long m = __ballot(L == q);
                if (!m) continue;
                unsigned int b = 0;
                if (lane == 0) b = atomicAdd(&counts[((1 + q) * kCdlpSubs + j) * kCntStride], (unsigned int)__popcll(m));
                b = __shfl(b, 0, kWave);
                if (L == q) {
                    const unsigned int idx = b + (unsigned int)__popcll(m & below);
                    if (idx < (unsigned int)asub) al[((int64_t)q * kCdlpSubs + j) * asub + idx] = (int32_t)w;
                    else *dense = 1;
                }
            }
        }
    }
}

// First iteration of an undirected graph whose rows are sorted by column: every label is still
// its vertex id, so the result is the row's first column (the smallest neighbour), one load per
// vertex instead of a pass over every label (~470 us of tier kernels on SYN-7_5).
__global__ __launch_bounds__(256) void k_cdlp_first_sorted(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                           int64_t v0, int64_t v1, int32_t *nxt, int *changed,
                                                           int cshards) {
    bool any = false;
    for (int64_t v = v0 + (int64_t)blockIdx.x * 256 + threadIdx.x; v < v1; v += (int64_t)gridDim.x * 256) {
        const int64_t b = rp[v];
        const int32_t l = rp[v + 1] > b ? ci[b] : (int32_t)v;
        nxt[v] = l;
        any |= l != (int32_t)v;
    }
    if (__ballot(any) && (threadIdx.x & (kWave - 1)) == 0) raise_flag_sharded(changed, cshards);
}

// First iteration of a directed graph whose rows (A and A') are strictly sorted: every label is
// still its vertex id, a neighbour's label occurs once per direction, so the mode is the
// smallest reciprocal neighbour (out and in: count 2) if there is one, else the smallest
// neighbour of either direction.  Replaces the tiers' counting pass over every label (~0.45 ms
// of SYN-cit's first iteration: a random label gather per entry).  A wave takes 64 consecutive
// vertices: rows of at most kFirstSmall entries each are compared pair by pair in one lane's
// registers, rows up to `medmax` entries afterwards by 16-lane groups (four rows at once), longer
// ones by the whole wave (first_dir_merge).  (A list of the long rows for a second kernel cost
// 0.69 ms: returning atomics on one counter.)  SYN-cit: 0.14 ms against the tiers' ~0.45.

// Both rows of v merged G entries at a time by G lanes (each out-entry looked up among the
// in-chunk by a log2(G)-step search over the group's lanes), the chunk with the smaller last
// entry advanced.  Every common entry is met in the round that retires its chunk, and chunks
// retire in ascending order, so the first round with a hit holds the smallest one.  SYN-cit: at
// most 13 rounds of 64, 1.4 per long row (a reciprocal neighbour is usually near the front).
// Group-uniform: every lane of the group calls it (gl = lane within the group).  Returns the
// label: that entry, else the smallest entry of either row (from the first chunks).
template <int G>
__device__ __forceinline__ int32_t first_dir_merge(const int32_t *__restrict__ xr, int64_t od,
                                                   const int32_t *__restrict__ yr, int64_t id, int gl) {
    int64_t i = 0, j = 0;
    int32_t xa = gl < od ? xr[gl] : INT32_MAX;   // ids < n <= INT32_MAX
    int32_t yb = gl < id ? yr[gl] : INT32_MAX;
    const int32_t lo = min(__shfl(xa, 0, G), __shfl(yb, 0, G));
    while (i < od && j < id) {
        int pos = 0;   // entries of the in-chunk below xa
#pragma unroll
        for (int st = G / 2; st; st >>= 1) pos += __shfl(yb, pos + st - 1, G) < xa ? st : 0;
        const int32_t at = __shfl(yb, pos & (G - 1), G);
        uint32_t h = pos < G && at == xa && xa != INT32_MAX ? (uint32_t)xa : 0xffffffffu;
        if constexpr (G == kWave) {
            h = wave_min_u32(h);
        } else {
#pragma unroll
            for (int o = G / 2; o; o >>= 1) h = min(h, (uint32_t)__shfl_xor((int)h, o, G));
        }
        if (h != 0xffffffffu) return (int32_t)h;
        const int32_t xm = __shfl(xa, G - 1, G), ym = __shfl(yb, G - 1, G);
        if (xm <= ym) {
            i += G;
            xa = i + gl < od ? xr[i + gl] : INT32_MAX;
        }
        if (ym <= xm) {
            j += G;
            yb = j + gl < id ? yr[j + gl] : INT32_MAX;
        }
    }
    return lo;
}

template <int kFirstSmall>
__global__ __launch_bounds__(256) void k_cdlp_first_dir(const int64_t *__restrict__ rpA, const int32_t *__restrict__ ciA,
                                                        const int64_t *__restrict__ rpT, const int32_t *__restrict__ ciT,
                                                        int64_t n, int32_t *out, int *changed, int cshards, int medmax) {
    const int lane = threadIdx.x & (kWave - 1);
    bool any = false;
    // wave-uniform trips: v0 is the wave's first vertex
    for (int64_t v0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~(kWave - 1)); v0 < n; v0 += (int64_t)gridDim.x * 256) {
        const int64_t v = v0 + lane;
        const bool in = v < n;
        const int64_t ob = in ? rpA[v] : 0, od = in ? rpA[v + 1] - ob : 0;
        const int64_t ib = in ? rpT[v] : 0, id = in ? rpT[v + 1] - ib : 0;
        const int64_t wide = od > id ? od : id;
        const bool lng = wide > kFirstSmall;
        if (in && !lng) {
            // loads clamped into the row (or to entry 0: rows_sorted implies nnz > 0) and
            // issued four at a time while any lane's rows reach that far
            int32_t x[kFirstSmall], y[kFirstSmall];
            const int64_t ra = od ? ob : 0, rb = id ? ib : 0, la = od ? od - 1 : 0, lb = id ? id - 1 : 0;
#pragma unroll
            for (int k = 0; k < kFirstSmall; k++) {
                x[k] = -1;
                y[k] = -2;   // the paddings match nothing
            }
#pragma unroll
            for (int k0 = 0; k0 < kFirstSmall; k0 += 4) {
                if (!__any(wide > k0)) break;
#pragma unroll
                for (int k = k0; k < k0 + 4; k++) {
                    const int32_t a = ciA[ra + min((int64_t)k, la)], b = ciT[rb + min((int64_t)k, lb)];
                    x[k] = k < od ? a : -1;
                    y[k] = k < id ? b : -2;
                }
            }
            int32_t m = INT32_MAX;
#pragma unroll
            for (int i = 0; i < kFirstSmall; i++)
#pragma unroll
                for (int j = 0; j < kFirstSmall; j++) m = x[i] == y[j] ? min(m, x[i]) : m;
            const int32_t lo = min(od ? x[0] : INT32_MAX, id ? y[0] : INT32_MAX);
            const int32_t l = m != INT32_MAX ? m : od + id ? lo : (int32_t)v;
            out[v] = l;
            any |= l != (int32_t)v;
        }
        // rows of at most medmax entries each: four at a time, 16 lanes each; group g takes the
        // wave's g-th, (g+4)-th, ... such row (the shuffles of the row extents run wave-wide)
        const int grp = lane >> 4, gl = lane & 15;
        uint64_t mb = __ballot(in && lng && wide <= medmax);
        for (int k = 0; k < grp; k++) mb &= mb - 1;
        while (__ballot(mb != 0)) {
            const int b = mb ? __builtin_ctzll(mb) : 0;
            const int64_t uob = __shfl(ob, b), uod = __shfl(od, b), uib = __shfl(ib, b), uid = __shfl(id, b);
            if (mb) {
                const int32_t l = first_dir_merge<16>(ciA + uob, uod, ciT + uib, uid, gl);
                if (gl == 0) {
                    out[v0 + b] = l;
                    any |= l != (int32_t)(v0 + b);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) mb &= mb - 1;
        }
        // the longer rows, one after the other, by the whole wave
        for (uint64_t bal = __ballot(in && lng && wide > medmax); bal; bal &= bal - 1) {
            const int b = __builtin_ctzll(bal);
            const int64_t u = v0 + b;
            const int64_t uob = __shfl(ob, b), uod = __shfl(od, b), uib = __shfl(ib, b), uid = __shfl(id, b);
            const int32_t l = first_dir_merge<kWave>(ciA + uob, uod, ciT + uib, uid, lane);
            if (lane == 0) {
                out[u] = l;
                any |= l != (int32_t)u;
            }
        }
    }
    if (__ballot(any) && (threadIdx.x & (kWave - 1)) == 0) raise_flag_sharded(changed, cshards);
}

// Whether every row of a CSR is sorted by column (strictly: rows hold no duplicates): the row
// starts as a bitmap over the entries, then one compare per entry.
__global__ __launch_bounds__(256) void k_row_start_bits(const int64_t *__restrict__ rp, int64_t n, uint32_t *bits) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        const int64_t b = rp[v];
        if (rp[v + 1] > b) atomicOr(&bits[b >> 5], 1u << (b & 31));
    }
}

__global__ __launch_bounds__(256) void k_rows_sorted(const int32_t *__restrict__ ci, int64_t nnz,
                                                     const uint32_t *__restrict__ bits, int *sorted) {
    bool bad = false;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k + 1 < nnz; k += (int64_t)gridDim.x * 256) {
        const int64_t k1 = k + 1;
        bad |= ci[k1] <= ci[k] && !((bits[k1 >> 5] >> (k1 & 31)) & 1u);
    }
    if (__ballot(bad) && (threadIdx.x & (kWave - 1)) == 0) *sorted = 0;
}

// Hub-first relabelling of a CSR: keys[e] = perm[row] << 32 | perm[col], sorted into the
// relabelled CSR (the PageRank plan's transform, gx_pr_order.hip).
__global__ void k_cdlp_permute_keys(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, int64_t n,
                                    int64_t nnz, const int32_t *__restrict__ perm, uint64_t *__restrict__ keys) {
    constexpr int kPer = 16;
    const int64_t e0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * kPer;
    if (e0 >= nnz) return;
    const int64_t e1 = min(e0 + kPer, nnz);
    int64_t r = row_of_edge(rp, n, e0);
    for (int64_t e = e0; e < e1; e++) {
        while (rp[r + 1] <= e) r++;
        keys[e] = ((uint64_t)(uint32_t)perm[r] << 32) | (uint32_t)perm[ci[e]];
    }
}

// out[v] = in[idx[v]]
__global__ void k_cdlp_gather_i32(const int32_t *__restrict__ in, const int32_t *__restrict__ idx, int64_t n,
                                  int32_t *__restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x)
        out[v] = in[idx[v]];
}

CdlpGraph cdlp_view(gx_graph *g) {
    CdlpGraph v;
    v.ctx = g->ctx;
    v.n = (int64_t)g->n;
    v.directed = g->directed;
    v.rpA = g->A.rp.p;
    v.ciA = g->A.ci.p;
    v.h_rpA = g->A.h_rp.data();
    v.nnzA = (int64_t)g->A.nnz;
    if (g->directed) {
        v.rpT = g->AT.rp.p;
        v.ciT = g->AT.ci.p;
        v.h_rpT = g->AT.h_rp.data();
        v.nnzT = (int64_t)g->AT.nnz;
    }
    return v;
}

// The initial labels: every vertex its own id.
__global__ void k_cdlp_iota(int32_t *a, int64_t n) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n;
         v += (int64_t)gridDim.x * blockDim.x)
        a[v] = (int32_t)v;
}

// What gx_cdlp keeps on the graph between calls (gx_graph::cdlp): the hub-first relabelled
// graph, the tier lists (built on the host from the row pointers: ~3 ms of
// idle device per call on SYN-7_5 when rebuilt) and the label, flag and active-set buffers.
// Iteration-count-sized buffers grow on demand.
struct CdlpCache {
    bool relabel = false;
    CdlpGraph G;                          // the graph the iterations run on
    DBuf<int64_t> rpA, rpT;               // relabelled copies (relabel)
    DBuf<int32_t> ciA, ciT;
    std::vector<int64_t> h_rpA, h_rpT;
    DBuf<int32_t> order, perm;            // order[p]: the caller's vertex at p; perm = its inverse
    CdlpPlan P;
    DBuf<int32_t> la, lb, act, al, tmp;
    DBuf<uint64_t> clist;
    DBuf<int> changed, dense;
    DBuf<unsigned int> ccount;
    int *hflag = nullptr, *dflag = nullptr;
    int cap_iters = 0;
    int64_t sub = 0, asub = 0;
    bool rows_sorted = false;   // A's rows (and A''s, directed) sorted by column (k_rows_sorted)
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    CdlpKeep keep;              // the own-label check's layouts and counters (gx_cdlp_keep.hip)
    DBuf<int32_t> vlb, vchg;    // the recount bound (GX_CDLP_BOUND)
    DBuf<int> hvalid;
    DBuf<int32_t> redo;         // k_cdlp_sparse_group's vertices for the 16K-slot instance
    DBuf<unsigned int> rcnt;    // one redo count per iteration
    ~CdlpCache() {
        if (hflag) (void)hipHostFree(hflag);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// Relabel one CSR of the graph by perm into (rp, ci).
int cdlp_relabel_csr(const DevCSR &M, int64_t n, const int32_t *perm, DBuf<int64_t> &rp, DBuf<int32_t> &ci,
                     hipStream_t s) {
    GX_TRY(rp.alloc(n + 1));
    GX_TRY(ci.alloc(M.nnz, 16));
    DBuf<uint64_t> keys, scratch;
    GX_TRY(keys.alloc(M.nnz));
    GX_TRY(scratch.alloc(M.nnz));
    if (M.nnz) {
        hipLaunchKernelGGL(k_cdlp_permute_keys, dim3(grid_for((M.nnz + 15) / 16, 256, 1u << 30)), dim3(256), 0, s,
                           M.rp.p, M.ci.p, n, (int64_t)M.nnz, perm, keys.p);
        GX_TRY(check_launch("k_cdlp_permute_keys"));
    }
    GX_TRY(sort_keys_to_csr(keys, scratch, M.nnz, n, rp.p, ci.p, s));
    GX_HIP_TRY(hipStreamSynchronize(s));   // keys die at return
    return GX_SUCCESS;
}

// Hub-first order by total degree (out + in), ties by id: the most gathered labels share the
// first lines of the label array (the PageRank plan's order, gx_pr_order.hip hub_order).
int cdlp_relabel(gx_graph *g, CdlpCache &C, hipStream_t s) {
    const int64_t n = (int64_t)g->n;
    std::vector<int64_t> deg(n);
    int64_t maxd = 0;
    for (int64_t v = 0; v < n; v++) {
        deg[v] = g->A.h_rp[v + 1] - g->A.h_rp[v];
        if (g->directed) deg[v] += g->AT.h_rp[v + 1] - g->AT.h_rp[v];
        maxd = std::max(maxd, deg[v]);
    }
    std::vector<int64_t> start((size_t)maxd + 2, 0);
    for (int64_t v = 0; v < n; v++) start[(size_t)(maxd - deg[v]) + 1]++;
    for (size_t k = 1; k < start.size(); k++) start[k] += start[k - 1];
    std::vector<int32_t> order(n), perm(n);
    for (int64_t v = 0; v < n; v++) {
        const int64_t pos = start[(size_t)(maxd - deg[v])]++;
        order[pos] = (int32_t)v;
        perm[v] = (int32_t)pos;
    }
    auto new_rp = [&](const HostRowPtr &h, std::vector<int64_t> &out) {
        out.assign(n + 1, 0);
        for (int64_t i = 0; i < n; i++) out[i + 1] = out[i] + (h[order[i] + 1] - h[order[i]]);
    };
    new_rp(g->A.h_rp, C.h_rpA);
    if (g->directed) new_rp(g->AT.h_rp, C.h_rpT);
    GX_TRY(C.order.alloc(n));
    GX_TRY(C.perm.alloc(n));
    GX_HIP_TRY(hipMemcpyAsync(C.order.p, order.data(), n * 4, hipMemcpyHostToDevice, s));
    GX_HIP_TRY(hipMemcpyAsync(C.perm.p, perm.data(), n * 4, hipMemcpyHostToDevice, s));
    GX_TRY(cdlp_relabel_csr(g->A, n, C.perm.p, C.rpA, C.ciA, s));
    if (g->directed) GX_TRY(cdlp_relabel_csr(g->AT, n, C.perm.p, C.rpT, C.ciT, s));
    C.G.rpA = C.rpA.p;
    C.G.ciA = C.ciA.p;
    C.G.h_rpA = C.h_rpA.data();
    if (g->directed) {
        C.G.rpT = C.rpT.p;
        C.G.ciT = C.ciT.p;
        C.G.h_rpT = C.h_rpT.data();
    }
    return GX_SUCCESS;
}

// The graph's cache, built by its first call (or rebuilt when GX_CDLP_RELABEL changed), with room
// for `iters` iterations' flags and counters.
int cdlp_cache(gx_graph *g, int iters, bool relabel, CdlpCache **out, hipStream_t s) {
    const int64_t n = (int64_t)g->n;
    auto *C = static_cast<CdlpCache *>(g->cdlp.get());
    if (C && C->relabel != relabel) {
        g->cdlp.reset();   // GX_CDLP_RELABEL changed between calls
        C = nullptr;
    }
    if (!C) {
        auto fresh = std::make_shared<CdlpCache>();
        fresh->relabel = relabel;
        GX_TRY(ensure_host_rp(g->ctx, g->A));
        fresh->G = cdlp_view(g);
        if (relabel) GX_TRY(cdlp_relabel(g, *fresh, s));
        GX_TRY(cdlp_plan(fresh->G, 0, n, fresh->P, s));
        GX_TRY(fresh->la.alloc(n));
        GX_TRY(fresh->lb.alloc(n));
        GX_TRY(fresh->act.alloc(n));
        fresh->sub = std::max<int64_t>(16, n / 32 / kCdlpSubs);   // entries per sub-list
        GX_TRY(fresh->clist.alloc((size_t)fresh->sub * kCdlpSubs));
        // active vertices per shard and list (GX_CDLP_ASUB: a test's small capacity, so lists overflow;
        // read here, when the cache is built, and not again)
        fresh->asub = std::max<int64_t>(16, n / 8 / kCdlpSubs);
        if (const char *e = std::getenv("GX_CDLP_ASUB")) fresh->asub = std::max<int64_t>(1, std::atoll(e));
        GX_TRY(fresh->al.alloc((size_t)fresh->asub * kCdlpSubs * (kCdlpLists - 1)));
        GX_TRY(fresh->dense.alloc(1));
        GX_TRY(fresh->redo.alloc(std::max<size_t>(1, fresh->P.n_mid4 + fresh->P.n_mid)));
        // the caller's rows sorted (A, and A' for a directed graph): the first iteration is each
        // row's first column (undirected, k_cdlp_first_sorted) or the smallest reciprocal
        // neighbour (directed, k_cdlp_first_dir), on the caller's graph, then moved to the
        // relabelled order
        auto sorted_rows = [&](const DevCSR &M, bool *ok) -> int {
            const int64_t nnz = (int64_t)M.nnz;
            *ok = true;
            if (nnz == 0) return GX_SUCCESS;
            DBuf<uint32_t> bits;
            DBuf<int> flag;
            GX_TRY(bits.alloc((size_t)(nnz + 31) / 32));
            GX_TRY(flag.alloc(1));
            GX_HIP_TRY(hipMemsetAsync(bits.p, 0, (size_t)(nnz + 31) / 32 * 4, s));
            const int one = 1;
            GX_HIP_TRY(hipMemcpyAsync(flag.p, &one, sizeof(int), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_row_start_bits, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, M.rp.p, n, bits.p);
            GX_TRY(check_launch("k_row_start_bits"));
            hipLaunchKernelGGL(k_rows_sorted, dim3(grid_for(nnz, 256, 8192)), dim3(256), 0, s, M.ci.p, nnz, bits.p,
                               flag.p);
            GX_TRY(check_launch("k_rows_sorted"));
            int sorted = 0;
            GX_HIP_TRY(hipMemcpyAsync(&sorted, flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
            GX_HIP_TRY(hipStreamSynchronize(s));
            *ok = sorted != 0;
            return GX_SUCCESS;
        };
        if (g->nnz > 0 && (!g->directed || g->AT.built)) {
            GX_TRY(fresh->tmp.alloc(n));
            bool okA = false, okT = true;
            GX_TRY(sorted_rows(g->A, &okA));
            if (g->directed && okA) GX_TRY(sorted_rows(g->AT, &okT));
            fresh->rows_sorted = okA && okT;
        }
        for (hipEvent_t &e : fresh->ev) GX_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        g->cdlp = fresh;
        C = fresh.get();
    }
    if (iters > C->cap_iters) {
        const int cap = std::max(iters, 16);
        GX_TRY(C->changed.alloc((size_t)cap * kFlagShards * kFlagStride));
        GX_TRY(C->ccount.alloc((size_t)cap * kCdlpLists * kCdlpSubs * kCntStride));
        GX_TRY(C->rcnt.alloc((size_t)cap));
        if (C->hflag) (void)hipHostFree(C->hflag);
        C->hflag = nullptr;
        GX_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&C->hflag), sizeof(int) * cap, hipHostMallocMapped));
        GX_HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&C->dflag), C->hflag, 0));
        C->cap_iters = cap;
    }
    *out = C;
    return GX_SUCCESS;
}

// The only place that reads a per-call knob (CdlpKnobs, gx_cdlp.h), once per call.
CdlpKnobs cdlp_knobs(int calls, int iters) {
    CdlpKnobs k;
    const char *re = std::getenv("GX_CDLP_RELABEL");
    k.relabel = re ? std::atoi(re) != 0 : calls >= 2;
    k.active = env_on("GX_CDLP_ACTIVE") && iters > 2;
    k.first_sorted = env_on("GX_CDLP_FIRST_SORTED");
    k.sparse = env_on("GX_CDLP_SPARSE");
    const char *so = std::getenv("GX_CDLP_SPARSE_ONLY");
    k.sparse_only = !k.sparse ? 0 : so ? std::atoi(so) : 1;
    const char *lg = std::getenv("GX_CDLP_LAG");
    k.lag = lg && std::atoi(lg) == 1 ? 1 : 2;
    k.keep = k.active && k.sparse && env_on("GX_CDLP_KEEP");
    k.keep_sorted = env_on("GX_CDLP_KEEP_SORTED");
    k.bound = env_on("GX_CDLP_BOUND");
    const char *fs = std::getenv("GX_CDLP_FIRST_SMALL");
    const int small = fs ? std::atoi(fs) : 8;
    k.first_small = small == 4 || small == 16 ? small : 8;
    const char *fm = std::getenv("GX_CDLP_FIRST_MED");
    k.first_med = fm ? std::atoi(fm) : 32;
    return k;
}

// What an iteration does.  Active: from iteration 2 on, the changes of the last iteration are
// listed (up to n / 32 of them) and their neighbours marked with the iteration's stamp before
// the kernels run.  Shortcut: iteration 0 on the caller's sorted rows.  Full: every tier, every vertex.
enum class IterKind { Shortcut, Full, Active };

IterKind iter_kind(int it, const CdlpKnobs &k, const CdlpCache &C) {
    if (k.active && it >= 2) return IterKind::Active;   // never before 2: prepare_active's invariant
    return it == 0 && C.rows_sorted && k.first_sorted ? IterKind::Shortcut : IterKind::Full;
}

// One gx_cdlp call and its stages, in the order gx_cdlp runs them.
struct CdlpCall {
    gx_graph *g;
    CdlpKnobs k;
    hipStream_t s;
    int iters;
    int64_t n;
    CdlpCache *C = nullptr;
    int32_t *cur = nullptr, *nxt = nullptr;        // an iteration reads cur and writes nxt
    CdlpBound bound{nullptr, nullptr, nullptr};    // the recount bound's arrays, null when off
    const CdlpBound *bd() const { return bound.vlb ? &bound : nullptr; }

    int start_labels() {
        if (k.relabel) {   // labels are the caller's vertex ids, at the relabelled positions
            GX_HIP_TRY(hipMemcpyAsync(C->la.p, C->order.p, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
        } else {
            hipLaunchKernelGGL(k_cdlp_iota, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, C->la.p, n);
            GX_TRY(check_launch("k_cdlp_iota"));
        }
        cur = C->la.p;
        nxt = C->lb.p;
        return GX_SUCCESS;
    }

    // The own-label check's layouts on first need, the active set's stamps and counters, and the
    // recount bound's arrays (an active iteration skips the vertices whose label provably keeps a
    // strict majority).
    // vlb / vchg / hvalid live in the cache and are zeroed only when allocated: a call starts with
    // the last call's values in them.  That is safe because of two things, which must stay true
    // together: (1) the bound is read only by sparse iterations (bound_keeps tests a.sparse), and
    // those start at it >= 2 (the first line of iter_kind above; k_cdlp_mark writes hvalid before
    // them); (2) iteration it = 1 is a full one (act = nullptr), in which every tier kernel calls
    // bound_set for every vertex of degree > 0 -- iteration 0's shortcuts (k_cdlp_first_sorted /
    // k_cdlp_first_dir) write neither array.  A vertex of degree 0 is never active.  If active
    // iterations ever start before it = 2, or a tier stops calling bound_set, clear vchg and
    // hvalid here instead.  tests/test_call_history.py sequence (c) guards the histories: calls of
    // 0 to 40 iterations mixed on one graph (short after long, after an early exit, the cache
    // dropped in between), every result against the oracle.  It is not known to catch an edit
    // that breaks (2): a trial build whose iteration 1 skipped bound_set still passed it (any
    // dense iteration sets every bound anew, which may be what hides the stale values).
    int prepare_active() {
        if (k.keep && !C->keep.built) GX_TRY(keep_build(C->G, C->relabel, C->keep, s));
        if (k.active) {
            hipLaunchKernelGGL(k_cdlp_fill_u32, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s,
                               reinterpret_cast<uint32_t *>(C->act.p), 0xffffffffu, n);   // stamp -1: never active
            GX_TRY(check_launch("k_cdlp_fill_u32"));
            GX_HIP_TRY(hipMemsetAsync(C->ccount.p, 0, sizeof(unsigned int) * kCdlpLists * kCdlpSubs * kCntStride * iters, s));
            GX_HIP_TRY(hipMemsetAsync(C->rcnt.p, 0, sizeof(unsigned int) * iters, s));
        }
        if (!k.bound) return GX_SUCCESS;
        if (C->vlb.n < (size_t)n) {
            GX_TRY(C->vlb.alloc(n));
            GX_TRY(C->vchg.alloc(n));
            GX_TRY(C->hvalid.alloc(1));
            GX_HIP_TRY(hipMemsetAsync(C->vlb.p, 0, (size_t)n * 4, s));
            GX_HIP_TRY(hipMemsetAsync(C->vchg.p, 0, (size_t)n * 4, s));
            GX_HIP_TRY(hipMemsetAsync(C->hvalid.p, 0, sizeof(int), s));
        }
        bound = CdlpBound{C->vlb.p, C->vchg.p, C->hvalid.p};
        return GX_SUCCESS;
    }

    // Iteration 0 by the shortcut kernels, on the caller's graph and vertex order (whose rows
    // cdlp_cache found sorted), then moved to the relabelled order.
    int first_iteration(int *changed) {
        KTimer kt(g->ctx, "cdlp_first", s);
        int32_t *out = k.relabel ? C->tmp.p : nxt;
        if (g->directed) {
            const auto kern = k.first_small == 4    ? k_cdlp_first_dir<4>
                              : k.first_small == 16 ? k_cdlp_first_dir<16>
                                                    : k_cdlp_first_dir<8>;
            // one wave per 64 vertices, no grid-stride trips (SYN-cit: 0.147 ms against 0.150
            // with 8192 blocks, 0.157 with 2048)
            hipLaunchKernelGGL(kern, dim3(grid_for(n, 256)), dim3(256), 0, s, g->A.rp.p, g->A.ci.p, g->AT.rp.p,
                               g->AT.ci.p, n, out, changed, kFlagShards, k.first_med);
            GX_TRY(check_launch("k_cdlp_first_dir"));
        } else {
            hipLaunchKernelGGL(k_cdlp_first_sorted, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, g->A.rp.p,
                               g->A.ci.p, (int64_t)0, n, out, changed, kFlagShards);
            GX_TRY(check_launch("k_cdlp_first_sorted"));
        }
        if (k.relabel) {   // nxt[p] = result of the caller's vertex order[p]
            hipLaunchKernelGGL(k_cdlp_gather_i32, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, C->tmp.p, C->order.p,
                               n, nxt);
            GX_TRY(check_launch("k_cdlp_gather_i32"));
        }
        return GX_SUCCESS;
    }

    // The changes of iteration it - 1 (nxt still holds its input, cur its output) as the active
    // set of iteration `it`; cnt are the iteration's list counters.
    int mark_changes(int it, unsigned int *cnt) {
        const CdlpGraph &G = C->G;
        KTimer kt(G.ctx, "cdlp_mark", s);
        hipLaunchKernelGGL(k_cdlp_changed, dim3(grid_for(n, 256, 4096)), dim3(256), 0, s, nxt, cur, G.rpA, G.rpT, n,
                           C->clist.p, C->sub, cnt, C->dense.p);
        GX_TRY(check_launch("k_cdlp_changed"));
        // 32 waves per shard of the change list (the grid must be a multiple of kCdlpSubs waves)
        hipLaunchKernelGGL(k_cdlp_mark, dim3(8 * kCdlpSubs), dim3(kCdlpSubs), 0, s, G.rpA, G.ciA, G.rpT, G.ciT,
                           C->clist.p, C->sub, cnt, C->act.p, (int32_t)it, C->dense.p, C->al.p, C->asub,
                           bound.vchg, bound.hvalid);
        return check_launch("k_cdlp_mark");
    }

    int active_iteration(int it, int *changed) {
        unsigned int *cnt = C->ccount.p + (size_t)it * kCdlpLists * kCdlpSubs * kCntStride;
        GX_TRY(mark_changes(it, cnt));
        // sparse-only (no idle tier launches, ~60 us per iteration on SYN-7_5) when iteration
        // it-1-lag, the last whose flags the host has seen, did not overflow its lists: changes
        // shrink as labels settle.  A wrong guess costs the fallback lists' full pass.
        const bool only =
            k.sparse_only == 2 || (k.sparse_only == 1 && it >= 3 + k.lag && (C->hflag[it - 1 - k.lag] & 2) == 0);
        // the own-label check where the iteration may be dense (in a sparse-only one its three
        // idle launches cost more than the rare dense case's fallback pass)
        int *kf = k.keep && (!only || k.sparse_only == 2) ? C->keep.kflags.p : nullptr;
        if (kf)
            GX_TRY(keep_check(C->G, C->keep, k.keep_sorted, cur, C->dense.p, C->act.p, (int32_t)it, cnt, C->al.p,
                              C->asub, bd(), s));
        const SparseLists sl{C->al.p, C->asub, cnt, only, C->redo.p, C->rcnt.p + it};
        CdlpStep st;
        st.act = C->act.p;
        st.stamp = (int32_t)it;
        st.dense = C->dense.p;
        st.sl = k.sparse ? &sl : nullptr;
        st.cshards = kFlagShards;
        st.keep = kf;
        st.bd = bd();
        return cdlp_iteration(C->G, C->P, cur, nxt, changed, s, st);
    }

    // Every tier, every vertex.  Iteration 0: labels are the caller's vertex ids.  The
    // smallest-neighbour shortcut (`first`) assumes no row repeats a column; k_rows_sorted found
    // the caller's rows strictly ascending, i.e. duplicate-free (else the counting path runs).
    int full_iteration(int it, int *changed) {
        CdlpStep st;
        st.first = it == 0 && C->rows_sorted;
        st.cshards = kFlagShards;
        st.bd = bd();
        return cdlp_iteration(C->G, C->P, cur, nxt, changed, s, st);
    }

    // Early exit at a fixed point (LAGraph_cdlp.c:328-332), checked `lag` iterations late:
    // iteration it is queued before the host waits for iteration it-lag's flag, so the check
    // never drains the stream.  An iteration run after a fixed point changes no label.  Lag 2
    // (GX_CDLP_LAG=1: one) keeps two iterations queued: sparse iterations of ~60 us are shorter
    // than the host's launches for one.  *fixed: iteration it-lag changed no label.
    int publish_flag_and_check_exit(int it, const int *changed, bool with_dense, bool *fixed) {
        hipLaunchKernelGGL(k_cdlp_flag_out, dim3(1), dim3(kWave), 0, s, changed, kFlagShards,
                           with_dense ? C->dense.p : nullptr, C->dflag + it);
        GX_TRY(check_launch("k_cdlp_flag_out"));
        GX_HIP_TRY(hipEventRecord(C->ev[it % 3], s));
        if (it >= k.lag) {
            GX_HIP_TRY(hipEventSynchronize(C->ev[(it - k.lag) % 3]));
            *fixed = !(C->hflag[it - k.lag] & 1);
        }
        return GX_SUCCESS;
    }

    // cur back in the caller's vertex order, and to the host.
    int finish(uint64_t *labels) {
        if (k.relabel) {
            hipLaunchKernelGGL(k_cdlp_gather_i32, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, cur, C->perm.p, n, nxt);
            GX_TRY(check_launch("k_cdlp_gather_i32"));
            cur = nxt;
        }
        GX_TRY(device_end(g->ctx));
        return download(g->ctx, labels, cur, (uint64_t)n, Xfer::Widen32);
    }
};

}  // namespace
}  // namespace gx

extern "C" int gx_cdlp(gx_graph *g, int iters, uint64_t *labels) {
    if (!g || !labels) return fail(GX_NULL_POINTER, "gx_cdlp: null argument");
    if (iters < 0) return fail(GX_INVALID_VALUE, "gx_cdlp: negative iteration count");
    gx_ctx *ctx = g->ctx;
    GX_HIP_TRY(hipSetDevice(ctx->device));
    if (g->n == 0) return GX_SUCCESS;
    GX_TRY(device_begin(ctx));
    if (g->directed) GX_TRY(ensure_transpose(g));
    // The relabelled copy costs ~90 ms to build on SYN-cit (4.2 M vertices) and saves ~1.3 ms
    // per call, so, like BFS's transpose, it is built once the graph serves a second CDLP run:
    // a one-off run (the Graphalytics executable's) stays in the caller's order.
    g->cdlp_calls++;
    CdlpCall c{g, cdlp_knobs(g->cdlp_calls, iters), ctx->stream, iters, (int64_t)g->n};
    GX_TRY(cdlp_cache(g, std::max(iters, 1), c.k.relabel, &c.C, c.s));
    CdlpCache *C = c.C;
    GX_HIP_TRY(hipMemsetAsync(C->changed.p, 0, sizeof(int) * kFlagShards * kFlagStride * std::max(iters, 1), c.s));
    GX_TRY(c.start_labels());
    GX_TRY(c.prepare_active());
    for (int it = 0; it < iters; it++) {
        int *changed = C->changed.p + (size_t)it * kFlagShards * kFlagStride;
        const IterKind kind = iter_kind(it, c.k, *C);
        switch (kind) {
        case IterKind::Shortcut: GX_TRY(c.first_iteration(changed)); break;
        case IterKind::Full: GX_TRY(c.full_iteration(it, changed)); break;
        case IterKind::Active: GX_TRY(c.active_iteration(it, changed)); break;
        }
        bool fixed = false;
        GX_TRY(c.publish_flag_and_check_exit(it, changed, kind == IterKind::Active, &fixed));
        std::swap(c.cur, c.nxt);
        if (fixed) break;   // iteration it-lag was a fixed point, so is cur
    }
    return c.finish(labels);
}

// ---- partitioned CDLP (one rank's vertex range; the caller exchanges labels) ----
struct gx_cdlp_part {
    gx_graph *g = nullptr;
    gx::CdlpPlan plan;
};

extern "C" int gx_cdlp_part_create(gx_graph *g, uint64_t v0, uint64_t v1, gx_cdlp_part **part) {
    if (!g || !part) return fail(GX_NULL_POINTER, "gx_cdlp_part_create: null argument");
    if (v0 > v1 || v1 > g->n) return fail(GX_INVALID_INDEX, "gx_cdlp_part_create: bad vertex range");
    GX_HIP_TRY(hipSetDevice(g->ctx->device));
    if (g->directed) GX_TRY(ensure_transpose(g));
    GX_TRY(ensure_host_rp(g->ctx, g->A));
    auto p = std::make_unique<gx_cdlp_part>();
    p->g = g;
    GX_TRY(cdlp_plan(cdlp_view(g), (int64_t)v0, (int64_t)v1, p->plan, g->ctx->stream));
    *part = p.release();
    return GX_SUCCESS;
}

extern "C" int gx_cdlp_part_init(gx_cdlp_part *part, int32_t *labels, void *stream) {
    if (!part || !labels) return fail(GX_NULL_POINTER, "gx_cdlp_part_init: null argument");
    gx_graph *g = part->g;
    GX_HIP_TRY(hipSetDevice(g->ctx->device));
    hipStream_t s = (hipStream_t)stream;   // NULL = the null stream (torch's default)
    if (g->n) {
        hipLaunchKernelGGL(k_cdlp_iota, dim3(grid_for(g->n, 256, 8192)), dim3(256), 0, s, labels, (int64_t)g->n);
        GX_TRY(check_launch("k_cdlp_iota"));
    }
    return GX_SUCCESS;
}

extern "C" int gx_cdlp_part_step(gx_cdlp_part *part, const int32_t *labels, int32_t *next, int *changed,
                                 void *stream) {
    if (!part || !labels || !next || !changed) return fail(GX_NULL_POINTER, "gx_cdlp_part_step: null argument");
    gx_graph *g = part->g;
    GX_HIP_TRY(hipSetDevice(g->ctx->device));
    hipStream_t s = (hipStream_t)stream;   // NULL = the null stream (torch's default)
    return cdlp_iteration(cdlp_view(g), part->plan, labels, next, changed, s, CdlpStep{});
}

extern "C" int gx_cdlp_part_free(gx_cdlp_part *part) {
    delete part;
    return GX_SUCCESS;
}

GX_MODULE_WARMER(cdlp)

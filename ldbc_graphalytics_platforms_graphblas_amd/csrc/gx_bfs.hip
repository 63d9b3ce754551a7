// gx_bfs.hip -- level-synchronous BFS (Graphalytics BFS = hop levels over out-edges).
//
// Replaces LA_BFS -> LAGr_BreadthFirstSearch(&level, NULL, G, src) (bfs.cpp:70-83), which
// SuiteSparse runs as a masked vxm per level over the boolean semiring.  Here:
//   top-down  : one wave per frontier vertex walks its out-row; an unvisited neighbour is
//               claimed with atomicCAS(level, -1, d+1) and appended to the next queue with
//               one wave-aggregated atomic (ballot + mbcnt).
//   bottom-up : (when the in-edges are resident: undirected graphs, or a directed graph
//               whose transpose is already built) one thread per unvisited vertex scans its
//               in-row, probing a bitmap of the current level (n/8 bytes, L2-resident) four
//               neighbours at a time, until it meets a frontier vertex.
// Direction switching follows Beamer's heuristic (alpha = 14, beta = 24).  Levels are
// unique, so the result is bit-exact whatever the traversal order.
// gx_bfs_parent (LAGr_BreadthFirstSearch with its parent output) runs the same levels, then one
// pass over the edges that gives every reached vertex its smallest parent (below, "parents").
#include <algorithm>
#include <cstdlib>
#include <memory>
#include <vector>

#include "gx_device.h"

namespace gx {
namespace {

constexpr int kBfsBlock = 256;
constexpr int kChunk = 256;   // edges per top-down work item (4 per lane)

// Frontier work items: (vertex << 32) | chunk, one item per kChunk out-edges, so a hub's
// adjacency is spread over many waves.  Appends are wave-aggregated: an inclusive scan of
// the lanes' item counts, one atomicAdd per wave.
__device__ __forceinline__ void wave_append(bool take, int32_t v, uint32_t nch, uint64_t *queue,
                                            uint32_t *qcount) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t k = take ? nch : 0u;
    uint32_t x = k;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const uint32_t y = __shfl_up(x, off, kWave);
        if (lane >= off) x += y;
    }
    const uint32_t total = __shfl(x, kWave - 1, kWave);
    if (total == 0) return;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(qcount, total);
    base = __shfl(base, 0, kWave);
    const uint32_t excl = x - k;
    for (uint32_t j = 0; j < k; j++) queue[base + excl + j] = ((uint64_t)(uint32_t)v << 32) | j;
}

__device__ __forceinline__ uint32_t chunks_of(int64_t deg) {
    return (uint32_t)((deg + kChunk - 1) / kChunk);
}

// top-down: one wave per work item (<= kChunk edges of one frontier vertex)
__device__ __forceinline__ void bfs_topdown(const int64_t *__restrict__ rp,
                                                           const int32_t *__restrict__ ci,
                                                           const uint64_t *__restrict__ qin,
                                                           uint32_t qsize, int32_t *level,
                                                           int32_t depth, uint64_t *qout,
                                                           uint32_t *qcount,
                                                           unsigned long long *next_edges, uint32_t bid,
                                                           uint32_t nblk) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = (bid * kBfsBlock + threadIdx.x) / kWave;
    const uint32_t nwaves = nblk * (kBfsBlock / kWave);
    unsigned long long edges = 0;
    for (uint32_t f = wave; f < qsize; f += nwaves) {
        const uint64_t item = qin[f];
        const int32_t u = (int32_t)(item >> 32);
        const int64_t e = rp[u + 1];
        const int64_t b = rp[u] + (int64_t)(uint32_t)item * kChunk;
        const int64_t end = min(e, b + kChunk);
#pragma unroll
        for (int i = 0; i < kChunk / kWave; i++) {
            const int64_t k = b + lane + (int64_t)i * kWave;
            bool take = false;
            int32_t v = 0;
            int64_t dv = 0;
            if (k < end) {
                v = ci[k];
                if (level[v] < 0 && atomicCAS(&level[v], -1, depth + 1) == -1) {
                    take = true;
                    dv = rp[v + 1] - rp[v];
                    edges += (unsigned long long)dv;
                }
            }
            wave_append(take, v, chunks_of(dv), qout, qcount);
        }
    }
    // one atomic per wave for the next frontier's edge count (direction heuristic)
    for (int off = 32; off > 0; off >>= 1) edges += __shfl_xor(edges, off, kWave);
    if (lane == 0 && edges) atomicAdd(next_edges, edges);
}

__global__ __launch_bounds__(kBfsBlock) void k_bfs_topdown(const int64_t *__restrict__ rp,
                                                           const int32_t *__restrict__ ci,
                                                           const uint64_t *__restrict__ qin, uint32_t qsize,
                                                           int32_t *level, int32_t depth, uint64_t *qout,
                                                           uint32_t *qcount, unsigned long long *next_edges) {
    bfs_topdown(rp, ci, qin, qsize, level, depth, qout, qcount, next_edges, blockIdx.x, gridDim.x);
}

// bottom-up: one thread per vertex; in-edges in (rpi, cii)
// Frontier bitmap for bottom-up steps: bit u set iff level[u] == depth.  One 64-bit word per
// wave (ballot over 64 consecutive vertices); n/8 bytes, so it stays resident in every XCD's
// L2 while the bottom-up probes hit it at random (the int32 level array does not).
__device__ __forceinline__ void bfs_bitmap(const int32_t *__restrict__ level, int64_t n, int32_t depth,
                                           uint64_t *fb, uint32_t bid, uint32_t nblk) {
    const int64_t stride = (int64_t)nblk * kBfsBlock;
    const int64_t nround = (n + stride - 1) / stride;
    for (int64_t r = 0; r < nround; r++) {
        const int64_t v = r * stride + (int64_t)bid * kBfsBlock + threadIdx.x;
        const uint64_t m = __ballot(v < n && level[v] == depth);
        if ((threadIdx.x & (kWave - 1)) == 0 && v < n) fb[v >> 6] = m;
    }
}

__global__ __launch_bounds__(kBfsBlock) void k_bfs_bitmap(const int32_t *__restrict__ level, int64_t n,
                                                          int32_t depth, uint64_t *fb) {
    bfs_bitmap(level, n, depth, fb, blockIdx.x, gridDim.x);
}

__device__ __forceinline__ uint32_t in_frontier(const uint64_t *__restrict__ fb, int32_t u) {
    return (uint32_t)((fb[u >> 6] >> (u & 63)) & 1ull);
}

// bottom-up: one thread per unvisited vertex scans its in-row, 4 neighbours per step (four
// independent bitmap probes in flight), until it meets a frontier vertex.  The next frontier
// is left in `level` (no queue: a queue append per wave is one same-address atomic per wave,
// ~11 ns each serialised, which dominated); found vertices and their out-edges are summed
// per workgroup and leave as one atomic each.
__device__ __forceinline__ void bfs_bottomup(const int64_t *__restrict__ rpi,
                                                            const int32_t *__restrict__ cii,
                                                            const int64_t *__restrict__ rpo,
                                                            const uint64_t *__restrict__ fb, int64_t n,
                                                            int32_t *level, int32_t depth,
                                                            unsigned long long *counters /* found, edges */,
                                                            uint64_t *fbn, uint32_t bid, uint32_t nblk) {
    __shared__ unsigned long long red[2][kBfsBlock / kWave];
    unsigned long long edges = 0, found = 0;
    // uniform trip count: a wave covers 64 aligned consecutive vertices per round, so with fbn
    // its ballot of the vertices found is the next level's frontier word (no bitmap pass)
    const int64_t stride = (int64_t)nblk * kBfsBlock;
    const int64_t nround = (n + stride - 1) / stride;
    for (int64_t r = 0; r < nround; r++) {
        const int64_t v = r * stride + (int64_t)bid * kBfsBlock + threadIdx.x;
        bool take = false;
        if (v < n && level[v] < 0) {
            const int64_t b = rpi[v], e = rpi[v + 1];
            for (int64_t k = b; k < e && !take; k += 4) {
                const int32_t u0 = cii[k];
                const int32_t u1 = cii[min(k + 1, e - 1)];
                const int32_t u2 = cii[min(k + 2, e - 1)];
                const int32_t u3 = cii[min(k + 3, e - 1)];
                // all four probes issue (no short-circuit), then one test
                take = (in_frontier(fb, u0) | in_frontier(fb, u1) | in_frontier(fb, u2) | in_frontier(fb, u3)) != 0;
            }
            if (take) {
                level[v] = depth + 1;
                edges += (unsigned long long)(rpo[v + 1] - rpo[v]);
                found++;
            }
        }
        if (fbn) {
            const uint64_t m = __ballot(take);
            if ((threadIdx.x & (kWave - 1)) == 0 && v < n) fbn[v >> 6] = m;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        edges += __shfl_xor(edges, off, kWave);
        found += __shfl_xor(found, off, kWave);
    }
    const int w = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        red[0][w] = found;
        red[1][w] = edges;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long f = 0, ed = 0;
        for (int i = 0; i < kBfsBlock / kWave; i++) {
            f += red[0][i];
            ed += red[1][i];
        }
        if (f) atomicAdd(&counters[0], f);
        if (ed) atomicAdd(&counters[1], ed);
    }
}

__global__ __launch_bounds__(kBfsBlock) void k_bfs_bottomup(const int64_t *__restrict__ rpi,
                                                            const int32_t *__restrict__ cii,
                                                            const int64_t *__restrict__ rpo,
                                                            const uint64_t *__restrict__ fb, int64_t n,
                                                            int32_t *level, int32_t depth,
                                                            unsigned long long *counters) {
    bfs_bottomup(rpi, cii, rpo, fb, n, level, depth, counters, nullptr, blockIdx.x, gridDim.x);
}

// Top-down queue of the vertices at `depth` (after bottom-up steps), built per tile of
// kQTile consecutive vertices: count the tile's items, one atomicAdd for its base, write.
constexpr int64_t kQTile = 4096;

// With fb (the frontier bitmap a bottom-up level left) the frontier test reads n/8 bytes of
// bitmap words (one line per wave) instead of the n int32 levels, twice.
__device__ __forceinline__ void bfs_level_queue(const int64_t *__restrict__ rp, const int32_t *__restrict__ level,
                                                int64_t n, int32_t depth, uint64_t *queue, uint32_t *qcount,
                                                const uint64_t *__restrict__ fb, uint32_t bid, uint32_t nblk) {
    auto at_depth = [&](int64_t v) -> bool {
        return fb ? ((fb[v >> 6] >> (v & 63)) & 1ull) != 0 : level[v] == depth;
    };
    __shared__ uint32_t wsum[kBfsBlock / kWave];
    __shared__ uint32_t tile_base;
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    for (int64_t t0 = (int64_t)bid * kQTile; t0 < n; t0 += (int64_t)nblk * kQTile) {
        const int64_t t1 = min(t0 + kQTile, n);
        uint32_t mine = 0;
        for (int64_t v = t0 + threadIdx.x; v < t1; v += kBfsBlock)
            if (at_depth(v)) mine += chunks_of(rp[v + 1] - rp[v]);
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, kWave);
        if (lane == 0) wsum[w] = mine;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t tot = 0;
            for (int i = 0; i < kBfsBlock / kWave; i++) tot += wsum[i];
            tile_base = tot ? atomicAdd(qcount, tot) : 0u;
        }
        __syncthreads();
        // second pass: ordered positions inside the tile, one 256-vertex step at a time
        uint32_t base = tile_base;
        for (int64_t v0 = t0; v0 < t1; v0 += kBfsBlock) {
            const int64_t v = v0 + threadIdx.x;
            const uint32_t k = (v < t1 && at_depth(v)) ? chunks_of(rp[v + 1] - rp[v]) : 0u;
            uint32_t x = k;   // inclusive scan over the workgroup: waves, then wave totals
#pragma unroll
            for (int off = 1; off < kWave; off <<= 1) {
                const uint32_t y = __shfl_up(x, off, kWave);
                if (lane >= off) x += y;
            }
            if (lane == kWave - 1) wsum[w] = x;
            __syncthreads();
            uint32_t before = 0, step = 0;
            for (int i = 0; i < kBfsBlock / kWave; i++) {
                if (i < w) before += wsum[i];
                step += wsum[i];
            }
            const uint32_t pos = base + before + x - k;
            for (uint32_t j = 0; j < k; j++) queue[pos + j] = ((uint64_t)(uint32_t)v << 32) | j;
            base += step;
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kBfsBlock) void k_bfs_level_queue(const int64_t *__restrict__ rp,
                                                               const int32_t *__restrict__ level, int64_t n,
                                                               int32_t depth, uint64_t *queue, uint32_t *qcount) {
    bfs_level_queue(rp, level, n, depth, queue, qcount, nullptr, blockIdx.x, gridDim.x);
}

// ---- device-driven levels ----------------------------------------------------------------
// The host-driven loop read the frontier counts back after every level to choose the
// direction: ~30-50 us of idle device per level (SYN-g500-22: ~7 levels, 0.48 ms per BFS of
// which ~0.25 ms kernels).  Here a one-thread plan kernel consumes the last level's counts,
// applies Beamer's rule and selects the level's kernels; the others exit at once.  The host
// queues levels in batches and reads the done flag one batch late.
struct BfsState {
    int32_t depth;
    int32_t mode;          // 0 done / idle, 1 top-down, 2 bottom-up
    int32_t done;
    int32_t started;
    int32_t qi;            // top-down input queue q[qi], its count qcnt[qi]
    int32_t have_queue;    // the frontier is in q[qi] (else only in `level`)
    int32_t need_queue;    // this top-down level first rebuilds q[qi] from `level`
    int32_t bottom_up;
    int32_t has_in;
    int32_t fbi;           // bottom-up reads frontier bitmap fb[fbi] and writes the next into fb[fbi ^ 1]
    int32_t fb_ready;      // fb[fbi] already holds this level's frontier (the last level was bottom-up)
    int32_t nextbits;      // bottom-up writes the next bitmap (GX_BFS_NEXTBITS, default on)
    int32_t qbits;         // a top-down queue rebuild reads that bitmap (GX_BFS_QBITS, default on)
    int32_t pad2;
    unsigned long long alpha, beta;   // Beamer's switch thresholds (GX_BFS_ALPHA / GX_BFS_BETA)
    unsigned long long mf, mu, fsize, n;
    uint32_t qcnt[2];
    unsigned long long nedges;
    unsigned long long bucnt[2];   // bottom-up: found, their out-edges
};

__global__ void k_bfs_plan(BfsState *st) {
    if (st->done) {
        st->mode = 0;
        return;
    }
    if (st->started) {   // the last level's results
        unsigned long long next_edges, next_size;
        if (st->mode == 2) {
            next_size = st->bucnt[0];
            next_edges = st->bucnt[1];
            st->have_queue = 0;
            if (st->nextbits) {
                st->fbi ^= 1;
                st->fb_ready = 1;
            }
        } else {
            st->fb_ready = 0;
            st->qi ^= 1;
            next_size = st->qcnt[st->qi];
            next_edges = st->nedges;
            st->have_queue = 1;
        }
        st->mu = st->mu > st->mf ? st->mu - st->mf : 0ull;
        st->mf = next_edges;
        st->fsize = next_size;
        st->depth++;
    }
    st->started = 1;
    if (st->fsize == 0) {
        st->done = 1;
        st->mode = 0;
        return;
    }
    // Beamer: TD -> BU when the frontier's edges exceed the unexplored ones / 14; BU -> TD when
    // the frontier shrinks below n / 24
    if (st->has_in) {
        if (!st->bottom_up && st->mf > st->mu / st->alpha) st->bottom_up = 1;
        else if (st->bottom_up && (long long)st->fsize < (long long)(st->n / st->beta)) st->bottom_up = 0;
    }
    if (st->bottom_up) {
        st->mode = 2;
        st->bucnt[0] = st->bucnt[1] = 0;
    } else {
        st->mode = 1;
        st->need_queue = !st->have_queue;
        if (st->need_queue) st->qcnt[st->qi] = 0;
        st->qcnt[st->qi ^ 1] = 0;
        st->nedges = 0;
    }
}

__global__ __launch_bounds__(kBfsBlock) void k_bfs_bitmap_dev(const int32_t *__restrict__ level, int64_t n,
                                                              const BfsState *st, uint64_t *fb0, uint64_t *fb1) {
    if (st->mode != 2 || st->fb_ready) return;
    bfs_bitmap(level, n, st->depth, st->fbi ? fb1 : fb0, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(kBfsBlock) void k_bfs_bottomup_dev(const int64_t *__restrict__ rpi,
                                                                const int32_t *__restrict__ cii,
                                                                const int64_t *__restrict__ rpo,
                                                                uint64_t *fb0, uint64_t *fb1, int64_t n,
                                                                int32_t *level, BfsState *st) {
    if (st->mode != 2) return;
    const int i = st->fbi;
    bfs_bottomup(rpi, cii, rpo, i ? fb1 : fb0, n, level, st->depth, st->bucnt,
                 st->nextbits ? (i ? fb0 : fb1) : nullptr, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(kBfsBlock) void k_bfs_level_queue_dev(const int64_t *__restrict__ rp,
                                                                   const int32_t *__restrict__ level, int64_t n,
                                                                   BfsState *st, uint64_t *q0, uint64_t *q1,
                                                                   const uint64_t *fb0, const uint64_t *fb1) {
    if (st->mode != 1 || !st->need_queue) return;
    const int qi = st->qi;
    bfs_level_queue(rp, level, n, st->depth, qi ? q1 : q0, &st->qcnt[qi],
                    st->fb_ready && st->qbits ? (st->fbi ? fb1 : fb0) : nullptr, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(kBfsBlock) void k_bfs_topdown_dev(const int64_t *__restrict__ rp,
                                                               const int32_t *__restrict__ ci, int32_t *level,
                                                               BfsState *st, uint64_t *q0, uint64_t *q1) {
    if (st->mode != 1) return;
    const int qi = st->qi;
    bfs_topdown(rp, ci, qi ? q1 : q0, st->qcnt[qi], level, st->depth, qi ? q0 : q1, &st->qcnt[qi ^ 1],
                &st->nedges, blockIdx.x, gridDim.x);
}

// A level in two launches instead of four (GX_BFS_FUSED, the default): the frontier phase
// (bottom-up: the bitmap unless the last level left it; top-down: the queue rebuild when
// needed) and the expansion (bottom-up or top-down), each branching on the plan's mode, so
// the direction not taken costs no idle launch.  Blocks past a phase's own grid exit, and the
// phase runs on exactly the grid its separate kernel had.
__global__ __launch_bounds__(kBfsBlock) void k_bfs_frontier_dev(const int64_t *__restrict__ rp,
                                                                const int32_t *__restrict__ level, int64_t n,
                                                                BfsState *st, uint64_t *fb0, uint64_t *fb1,
                                                                uint64_t *q0, uint64_t *q1, uint32_t vgrid,
                                                                uint32_t qgrid) {
    const int mode = st->mode;
    if (mode == 2) {
        if (st->fb_ready || blockIdx.x >= vgrid) return;
        bfs_bitmap(level, n, st->depth, st->fbi ? fb1 : fb0, blockIdx.x, vgrid);
    } else if (mode == 1) {
        if (!st->need_queue || blockIdx.x >= qgrid) return;
        const int qi = st->qi;
        bfs_level_queue(rp, level, n, st->depth, qi ? q1 : q0, &st->qcnt[qi],
                        st->fb_ready && st->qbits ? (st->fbi ? fb1 : fb0) : nullptr, blockIdx.x, qgrid);
    }
}

__global__ __launch_bounds__(kBfsBlock) void k_bfs_expand_dev(const int64_t *__restrict__ rpi,
                                                              const int32_t *__restrict__ cii,
                                                              const int64_t *__restrict__ rp,
                                                              const int32_t *__restrict__ ci, int32_t *level,
                                                              int64_t n, BfsState *st, uint64_t *fb0, uint64_t *fb1,
                                                              uint64_t *q0, uint64_t *q1, uint32_t bu_grid,
                                                              uint32_t tgrid) {
    const int mode = st->mode;
    if (mode == 2) {
        if (blockIdx.x >= bu_grid) return;
        const int i = st->fbi;
        bfs_bottomup(rpi, cii, rp, i ? fb1 : fb0, n, level, st->depth, st->bucnt,
                     st->nextbits ? (i ? fb0 : fb1) : nullptr, blockIdx.x, bu_grid);
    } else if (mode == 1) {
        if (blockIdx.x >= tgrid) return;
        const int qi = st->qi;
        bfs_topdown(rp, ci, qi ? q1 : q0, st->qcnt[qi], level, st->depth, qi ? q0 : q1, &st->qcnt[qi ^ 1],
                    &st->nedges, blockIdx.x, tgrid);
    }
}

__global__ void k_bfs_seed(const int64_t *__restrict__ rp, int32_t *level, uint64_t *queue, uint32_t *qcount,
                           int32_t src) {
    level[src] = 0;
    const uint32_t nch = chunks_of(rp[src + 1] - rp[src]);
    for (uint32_t j = threadIdx.x; j < nch; j += blockDim.x) queue[j] = ((uint64_t)(uint32_t)src << 32) | j;
    if (threadIdx.x == 0) *qcount = nch;
}

// ---- parents from the finished levels (gx_bfs_parent) ------------------------------------
// parent[v] = the smallest candidate u with A(u,v) stored and level[u] == level[v] - 1, where
// the candidate of u is its id in the caller's vertex order (order[u] on a hub-first copy, so
// the minimum is the same on the copy as on the graph itself).  The level kernels cannot give
// it: the top-down claim is first-come and the bottom-up scan stops at its first hit.
//   pull : (in-edges resident, as for bottom-up) every reached v scans its whole in-row -- rows
//          are not sorted in the candidates' id space, so the first hit is not the minimum.  A
//          row of at most kParentShort entries is one thread's work; a longer one becomes
//          (vertex, chunk) items of kChunk entries, one wave each, like the top-down frontier:
//          the wave reduces its minimum and stores it (one chunk) or atomicMin's it (several).
//   push : (a directed graph without its transpose) every reached u walks its out-row, same
//          split, and offers its candidate to each v one level down with atomicMin, behind a
//          plain read of parent[v]: candidates only fall, so a stale read costs one atomic at
//          most, and most offers lose to an earlier smaller one without leaving the CU.
// Unreached vertices read -1; in push the identity INT32_MAX stands until k_bfs_parent_fin.
constexpr int kParentShort = 64;   // GX_BFS_PARENT_SHORT overrides (16-256 within 7 % on a copy)
constexpr int32_t kNoParent = INT32_MAX;

__device__ __forceinline__ int32_t parent_cand(const int32_t *__restrict__ order, int32_t u) {
    return order ? order[u] : u;
}

// pull: is u a parent of a vertex whose level is lv1 + 1?  push: is v a child of one at lv1 - 1?
template <bool PUSH>
__device__ __forceinline__ void parent_edge(const int32_t *__restrict__ level,
                                            const int32_t *__restrict__ order, int32_t x, int32_t lv1,
                                            int32_t mine, int32_t *parent, int32_t &m) {
    if (level[x] != lv1) return;
    if constexpr (PUSH) {
        if (parent[x] > mine) atomicMin(&parent[x], mine);
    } else {
        m = min(m, parent_cand(order, x));
    }
}

// One thread per vertex: the short rows whole, the long ones queued as items for
// k_bfs_parent_long (a wave covers 64 consecutive vertices per round: wave_append shuffles).
template <bool PUSH>
__global__ __launch_bounds__(kBfsBlock) void k_bfs_parent_rows(const int64_t *__restrict__ rp,
                                                               const int32_t *__restrict__ ci,
                                                               const int32_t *__restrict__ level,
                                                               const int32_t *__restrict__ order, int64_t n,
                                                               int32_t *parent, uint64_t *items,
                                                               uint32_t *nitems, int short_deg) {
    const int64_t stride = (int64_t)gridDim.x * kBfsBlock;
    const int64_t nround = (n + stride - 1) / stride;
    for (int64_t r = 0; r < nround; r++) {
        const int64_t v = r * stride + (int64_t)blockIdx.x * kBfsBlock + threadIdx.x;
        uint32_t nch = 0;
        if (v < n) {
            const int32_t lv = level[v];
            if (!PUSH && lv <= 0) {
                parent[v] = lv < 0 ? -1 : parent_cand(order, (int32_t)v);   // unreached; the source
            } else if (lv >= 0) {
                const int64_t b = rp[v], e = rp[v + 1];
                if (e - b > short_deg) {
                    nch = chunks_of(e - b);
                    if (!PUSH) parent[v] = kNoParent;
                } else {
                    const int32_t lv1 = PUSH ? lv + 1 : lv - 1;
                    const int32_t mine = PUSH ? parent_cand(order, (int32_t)v) : 0;
                    int32_t m = kNoParent;
                    for (int64_t k = b; k < e; k += 4) {   // four independent level probes in flight
                        const int32_t x0 = ci[k];
                        const int32_t x1 = ci[min(k + 1, e - 1)];
                        const int32_t x2 = ci[min(k + 2, e - 1)];
                        const int32_t x3 = ci[min(k + 3, e - 1)];
                        parent_edge<PUSH>(level, order, x0, lv1, mine, parent, m);
                        parent_edge<PUSH>(level, order, x1, lv1, mine, parent, m);
                        parent_edge<PUSH>(level, order, x2, lv1, mine, parent, m);
                        parent_edge<PUSH>(level, order, x3, lv1, mine, parent, m);
                    }
                    if (!PUSH) parent[v] = m;
                }
            }
        }
        wave_append(nch != 0, (int32_t)v, nch, items, nitems);
    }
}

// One wave per (vertex, chunk) item of a long row.
template <bool PUSH>
__global__ __launch_bounds__(kBfsBlock) void k_bfs_parent_long(const int64_t *__restrict__ rp,
                                                               const int32_t *__restrict__ ci,
                                                               const int32_t *__restrict__ level,
                                                               const int32_t *__restrict__ order,
                                                               const uint64_t *__restrict__ items,
                                                               const uint32_t *__restrict__ nitems,
                                                               int32_t *parent) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = (blockIdx.x * kBfsBlock + threadIdx.x) / kWave;
    const uint32_t nwaves = gridDim.x * (kBfsBlock / kWave);
    const uint32_t count = *nitems;
    for (uint32_t f = wave; f < count; f += nwaves) {
        const uint64_t item = items[f];
        const int32_t v = (int32_t)(item >> 32);
        const int64_t b0 = rp[v], e = rp[v + 1];
        const int64_t b = b0 + (int64_t)(uint32_t)item * kChunk;
        const int64_t end = min(e, b + kChunk);
        const int32_t lv1 = PUSH ? level[v] + 1 : level[v] - 1;
        const int32_t mine = PUSH ? parent_cand(order, v) : 0;
        int32_t m = kNoParent;
#pragma unroll
        for (int i = 0; i < kChunk / kWave; i++) {
            const int64_t k = b + lane + (int64_t)i * kWave;
            if (k < end) parent_edge<PUSH>(level, order, ci[k], lv1, mine, parent, m);
        }
        if constexpr (!PUSH) {
            for (int off = 32; off > 0; off >>= 1) m = min(m, __shfl_xor(m, off, kWave));
            if (lane == 0) {
                if (e - b0 <= kChunk) parent[v] = m;   // the row's only chunk
                else if (m != kNoParent) atomicMin(&parent[v], m);
            }
        }
    }
}

// push: the atomicMin identity everywhere but at the source, and back to -1 where it stood
__global__ __launch_bounds__(kBfsBlock) void k_bfs_parent_init(const int32_t *__restrict__ level,
                                                               const int32_t *__restrict__ order, int64_t n,
                                                               int32_t *__restrict__ parent) {
    for (int64_t v = (int64_t)blockIdx.x * kBfsBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBfsBlock)
        parent[v] = level[v] == 0 ? parent_cand(order, (int32_t)v) : kNoParent;
}

__global__ __launch_bounds__(kBfsBlock) void k_bfs_parent_fin(int64_t n, int32_t *__restrict__ parent) {
    for (int64_t v = (int64_t)blockIdx.x * kBfsBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBfsBlock)
        if (parent[v] == kNoParent) parent[v] = -1;
}

// The buffers of one BFS: owned by the entry point, so they are released after its download.
struct BfsWork {
    DBuf<int32_t> level;   // the result, in g's vertex order: -1 = unreached
    DBuf<uint64_t> q0, q1;
    DBuf<uint32_t> qcount;
    DBuf<unsigned long long> nedges;
    DBuf<uint64_t> fbits;
    DBuf<unsigned long long> bucnt;
    DBuf<BfsState> st;
    std::unique_ptr<int32_t, void (*)(int32_t *)> done_guard{nullptr, [](int32_t *p) { (void)hipHostFree(p); }};
    std::unique_ptr<ihipEvent_t, void (*)(hipEvent_t)> ev_guard{nullptr, [](hipEvent_t e) { (void)hipEventDestroy(e); }};
    const DevCSR *in = nullptr;   // the in-edges the bottom-up levels read (nullptr: none resident)
};

// The levels of a BFS of g (not a graph with a hub-first copy to run on: the entry points go
// through hub_for first) from src, left on the device in w.level; device_begin is called, the
// caller ends the bracket.  tail(early) queues the caller's work behind the last level (the
// results' remap, the parent pass) and returns whether it did: with early set it is queued
// behind the levels expected to be the last, before the host knows they are, and is asked for
// again if they were not.  bracket = false: the caller has opened the device bracket itself
// (gx_betweenness: one bracket over a batch of sources).
template <typename Tail>
int bfs_levels(gx_graph *g, uint64_t src, BfsWork &w, Tail &&tail, bool bracket = true) {
    gx_ctx *ctx = g->ctx;
    GX_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t n = (int64_t)g->n;
    int64_t src_rp[2] = {0, 0};   // the source's out-degree (the host row pointers are lazy)
    GX_HIP_TRY(hipMemcpy(src_rp, g->A.rp.p + src, sizeof(src_rp), hipMemcpyDeviceToHost));
    const int64_t src_deg = src_rp[1] - src_rp[0];
    DBuf<int32_t> &level = w.level;
    DBuf<uint64_t> &q0 = w.q0, &q1 = w.q1;
    DBuf<uint32_t> &qcount = w.qcount;
    DBuf<unsigned long long> &nedges = w.nedges;
    DBuf<uint64_t> &fbits = w.fbits;
    DBuf<unsigned long long> &bucnt = w.bucnt;
    // a work set that already served a BFS of this graph (gx_betweenness: one per batch) keeps its buffers
    auto sized = [](auto &buf, size_t count) -> int { return buf.p && buf.n == count ? GX_SUCCESS : buf.alloc(count); };
    GX_TRY(sized(fbits, 2 * ((n + 63) / 64)));   // two bitmaps: the device-driven path alternates them
    uint64_t *const fb1 = fbits.p + (n + 63) / 64;
    GX_TRY(sized(bucnt, 2));
    const uint64_t qcap = (uint64_t)n + g->nnz / kChunk + 64;   // sum over vertices of ceil(deg / kChunk)
    GX_TRY(sized(level, n));
    GX_TRY(sized(q0, qcap));
    GX_TRY(sized(q1, qcap));
    GX_TRY(sized(qcount, 1));
    GX_TRY(sized(nedges, 1));
    if (bracket) GX_TRY(device_begin(ctx));
    // in-edges: the graph itself when undirected; for a directed graph the transpose, built on
    // the device and cached once the graph serves a second BFS (a one-off run, like the
    // Graphalytics executable's, would not win back the build).  GX_BFS_TRANSPOSE = 0 never,
    // 1 from the second run (default), 2 from the first.
    g->bfs_calls++;
    if (g->directed && !g->AT.built) {
        const char *e = std::getenv("GX_BFS_TRANSPOSE");
        const int mode = e ? std::atoi(e) : 1;
        if (mode == 2 || (mode == 1 && g->bfs_calls >= 2)) GX_TRY(ensure_transpose(g));
    }
    const DevCSR *in = g->directed ? (g->AT.built ? &g->AT : nullptr) : &g->A;
    w.in = in;
    GX_HIP_TRY(hipMemsetAsync(level.p, 0xff, n * 4, s));
    const unsigned bu_grid = (unsigned)std::min<int64_t>(grid_for(n, kBfsBlock, 8192), 1024);
    const char *de = std::getenv("GX_BFS_DEVICE");
    if (!de || std::atoi(de) != 0) {
        // device-driven levels (k_bfs_plan), queued in batches; the done flag is read one
        // batch late
        DBuf<BfsState> &st = w.st;
        GX_TRY(sized(st, 1));
        BfsState h{};
        const int64_t dsrc = src_deg;
        h.have_queue = 1;
        h.has_in = in != nullptr;
        h.n = (unsigned long long)n;
        h.mf = (unsigned long long)dsrc;
        h.mu = g->nnz;
        h.fsize = (unsigned long long)((dsrc + kChunk - 1) / kChunk);
        const char *nb = std::getenv("GX_BFS_NEXTBITS");
        h.nextbits = !nb || std::atoi(nb) != 0;
        const char *qb = std::getenv("GX_BFS_QBITS");
        h.qbits = !qb || std::atoi(qb) != 0;
        const char *ae = std::getenv("GX_BFS_ALPHA"), *be = std::getenv("GX_BFS_BETA");
        h.alpha = (unsigned long long)std::max(1, ae ? std::atoi(ae) : 14);
        // beta 48 on undirected graphs (SYN-7_5 0.203-0.209 -> 0.186-0.192 ms, SYN-g500-22 ~1 %),
        // 24 on directed ones (SYN-cit 2-6 % slower at 48): profiles/r05_bfs_beta_ab.txt
        h.beta = (unsigned long long)std::max(1, be ? std::atoi(be) : (g->directed ? 24 : 48));
        GX_HIP_TRY(hipMemcpyAsync(st.p, &h, sizeof(h), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_bfs_seed, dim3(1), dim3(256), 0, s, g->A.rp.p, level.p, q0.p, &st.p->qcnt[0],
                           (int32_t)src);
        GX_TRY(check_launch("k_bfs_seed"));
        int32_t *h_done = w.done_guard.get();
        hipEvent_t ev = w.ev_guard.get();
        if (!h_done) {
            GX_HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&h_done), 4 * sizeof(int32_t), hipHostMallocDefault));
            w.done_guard.reset(h_done);
        }
        if (!ev) {
            GX_HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            w.ev_guard.reset(ev);
        }
        // grids of the kernels that run idle on the levels of the other direction: an idle
        // 8192-workgroup launch cost 2.6-3.0 us, a 2048 one 0.9 (r04_bfs_kernel_stats.csv);
        // every kernel is a grid-stride loop (GX_BFS_GRID overrides)
        const char *ge = std::getenv("GX_BFS_GRID");
        const unsigned gcap = ge ? (unsigned)std::max(1, std::atoi(ge)) : 2048u;
        const unsigned vgrid = grid_for(n, kBfsBlock, gcap);
        const unsigned tgrid = std::min(8192u, gcap);
        const unsigned qgrid = (unsigned)std::min<int64_t>((n + kQTile - 1) / kQTile, 2048);
        const char *fe = std::getenv("GX_BFS_FUSED");
        const bool fused = !fe || std::atoi(fe) != 0;
        auto enqueue = [&](int k) -> int {
            for (int i = 0; i < k; i++) {
                hipLaunchKernelGGL(k_bfs_plan, dim3(1), dim3(1), 0, s, st.p);
                if (fused) {
                    if (in) {
                        KTimer kt(ctx, "bfs_frontier", s);
                        hipLaunchKernelGGL(k_bfs_frontier_dev, dim3(std::max(vgrid, qgrid)), dim3(kBfsBlock), 0, s,
                                           g->A.rp.p, level.p, n, st.p, fbits.p, fb1, q0.p, q1.p, vgrid, qgrid);
                    }
                    KTimer kt(ctx, "bfs_expand", s);
                    hipLaunchKernelGGL(k_bfs_expand_dev, dim3(std::max(in ? bu_grid : 0u, tgrid)), dim3(kBfsBlock), 0,
                                       s, in ? in->rp.p : nullptr, in ? in->ci.p : nullptr, g->A.rp.p, g->A.ci.p,
                                       level.p, n, st.p, fbits.p, fb1, q0.p, q1.p, in ? bu_grid : 0u, tgrid);
                    continue;
                }
                if (in) {
                    KTimer kt(ctx, "bfs_bottomup", s);
                    hipLaunchKernelGGL(k_bfs_bitmap_dev, dim3(vgrid), dim3(kBfsBlock), 0, s, level.p, n, st.p,
                                       fbits.p, fb1);
                    hipLaunchKernelGGL(k_bfs_bottomup_dev, dim3(bu_grid), dim3(kBfsBlock), 0, s, in->rp.p, in->ci.p,
                                       g->A.rp.p, fbits.p, fb1, n, level.p, st.p);
                }
                KTimer kt(ctx, "bfs_topdown", s);
                if (in)
                    hipLaunchKernelGGL(k_bfs_level_queue_dev, dim3(qgrid), dim3(kBfsBlock), 0, s, g->A.rp.p, level.p,
                                       n, st.p, q0.p, q1.p, fbits.p, fb1);
                hipLaunchKernelGGL(k_bfs_topdown_dev, dim3(tgrid), dim3(kBfsBlock), 0, s, g->A.rp.p, g->A.ci.p,
                                   level.p, st.p, q0.p, q1.p);
            }
            return check_launch("k_bfs_topdown_dev");
        };
        // A first batch of levels, then batches of kBatch with the done flag read one batch
        // late; a level queued past the end costs ~20 us (five launches that exit at once).
        // The first batch is the number of steps the last BFS on this graph took (a repeated
        // or nearby source needs the same: SYN-g500-22 8), else kFirst; when it was enough,
        // the host waits for it and queues nothing more.
        // The hint is capped (kMaxFirst): after a deep BFS (a long chain) a shallow one would
        // otherwise queue thousands of idle levels at ~20 us each.
        constexpr int kFirst = 6, kBatch = 2, kMaxFirst = 24;
        const int first = g->bfs_steps_hint > 0 ? std::min(g->bfs_steps_hint, kMaxFirst) : kFirst;
        // h_done[0..2] = depth, mode, done of the state (one copy)
        auto read_state = [&]() -> int {
            GX_HIP_TRY(hipMemcpyAsync(h_done, &st.p->depth, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            GX_HIP_TRY(hipEventRecord(ev, s));
            return GX_SUCCESS;
        };
        bool queued = false;
        GX_TRY(enqueue(first));
        int64_t levels = first;
        GX_TRY(read_state());
        if (g->bfs_steps_hint > 0) {
            // the tail (the results' remap) is queued behind the levels it expects to be the
            // last, so it runs while the host reads the flag (queued again below if they were not)
            GX_TRY(tail(true, queued));
            GX_HIP_TRY(hipEventSynchronize(ev));
        } else {
            GX_TRY(enqueue(kBatch));
            levels += kBatch;
            GX_HIP_TRY(hipEventSynchronize(ev));
        }
        const bool more = !h_done[2];
        while (!h_done[2]) {
            GX_TRY(read_state());
            GX_TRY(enqueue(kBatch));
            levels += kBatch;
            GX_HIP_TRY(hipEventSynchronize(ev));
            if (levels > n + 2 * kFirst + 8) return fail(GX_PANIC, "gx_bfs: level loop did not end");
        }
        // steps this BFS needed: its levels plus the plan step that found the frontier empty
        g->bfs_steps_hint = h_done[0] + 1;
        if (!queued || more) GX_TRY(tail(false, queued));
        return GX_SUCCESS;
    }
    hipLaunchKernelGGL(k_bfs_seed, dim3(1), dim3(256), 0, s, g->A.rp.p, level.p, q0.p, qcount.p, (int32_t)src);
    GX_TRY(check_launch("k_bfs_seed"));
    uint32_t qsize = 0;
    GX_HIP_TRY(hipMemcpyAsync(&qsize, qcount.p, 4, hipMemcpyDeviceToHost, s));
    GX_HIP_TRY(hipStreamSynchronize(s));
    unsigned long long mf = (unsigned long long)src_deg;
    unsigned long long mu = g->nnz;
    bool bottom_up = false;
    int32_t depth = 0;
    struct Counters {
        uint32_t q;
        uint32_t pad;
        unsigned long long e;
    };
    // frontier: qsize vertices (top-down steps keep them as work items in q0; after a
    // bottom-up step they are only in `level` until a top-down step needs the queue)
    bool have_queue = true;
    uint64_t fsize = qsize;
    while (fsize > 0) {
        // Beamer switch: TD -> BU when the frontier's edges exceed the unexplored ones / 14;
        // BU -> TD when the frontier shrinks below n / 24.
        if (in) {
            if (!bottom_up && mf > mu / 14) bottom_up = true;
            else if (bottom_up && (int64_t)fsize < n / 24) bottom_up = false;
        }
        unsigned long long next_edges = 0;
        uint64_t next_size = 0;
        if (bottom_up) {
            KTimer kt(ctx, "bfs_bottomup", s);
            GX_HIP_TRY(hipMemsetAsync(bucnt.p, 0, 16, s));
            hipLaunchKernelGGL(k_bfs_bitmap, dim3(grid_for(n, kBfsBlock, 8192)), dim3(kBfsBlock), 0, s, level.p, n,
                               depth, fbits.p);
            hipLaunchKernelGGL(k_bfs_bottomup, dim3(bu_grid), dim3(kBfsBlock), 0, s, in->rp.p, in->ci.p, g->A.rp.p,
                               fbits.p, n, level.p, depth, bucnt.p);
            GX_TRY(check_launch("k_bfs_bottomup"));
            unsigned long long c[2] = {0, 0};
            GX_HIP_TRY(hipMemcpyAsync(c, bucnt.p, 16, hipMemcpyDeviceToHost, s));
            GX_HIP_TRY(hipStreamSynchronize(s));
            next_size = c[0];
            next_edges = c[1];
            have_queue = false;
        } else {
            KTimer kt(ctx, "bfs_topdown", s);
            if (!have_queue) {
                GX_HIP_TRY(hipMemsetAsync(qcount.p, 0, 4, s));
                hipLaunchKernelGGL(k_bfs_level_queue, dim3((unsigned)std::min<int64_t>((n + kQTile - 1) / kQTile, 2048)),
                                   dim3(kBfsBlock), 0, s, g->A.rp.p, level.p, n, depth, q0.p, qcount.p);
                GX_TRY(check_launch("k_bfs_level_queue"));
                GX_HIP_TRY(hipMemcpyAsync(&qsize, qcount.p, 4, hipMemcpyDeviceToHost, s));
                GX_HIP_TRY(hipStreamSynchronize(s));
                have_queue = true;
            }
            GX_HIP_TRY(hipMemsetAsync(qcount.p, 0, 4, s));
            GX_HIP_TRY(hipMemsetAsync(nedges.p, 0, 8, s));
            hipLaunchKernelGGL(k_bfs_topdown, dim3(grid_for((uint64_t)qsize * kWave, kBfsBlock, 8192)),
                               dim3(kBfsBlock), 0, s, g->A.rp.p, g->A.ci.p, q0.p, qsize, level.p, depth, q1.p,
                               qcount.p, nedges.p);
            GX_TRY(check_launch("k_bfs_topdown"));
            Counters c{};
            GX_HIP_TRY(hipMemcpyAsync(&c.q, qcount.p, 4, hipMemcpyDeviceToHost, s));
            GX_HIP_TRY(hipMemcpyAsync(&c.e, nedges.p, 8, hipMemcpyDeviceToHost, s));
            GX_HIP_TRY(hipStreamSynchronize(s));
            qsize = c.q;
            next_size = c.q;   // work items (~ vertices; a hub counts once per 256 edges)
            next_edges = c.e;
            std::swap(q0.p, q1.p);
        }
        mu = mu > mf ? mu - mf : 0;
        mf = next_edges;
        fsize = next_size;
        depth++;
    }
    bool queued = false;
    return tail(false, queued);
}

// The parent pass over w's finished levels into parent (n words, g's vertex order, candidates
// in the caller's ids); the items of the long rows reuse the level loop's queue.
int bfs_parents(gx_graph *g, BfsWork &w, int32_t *parent, hipStream_t s) {
    const int64_t n = (int64_t)g->n;
    const unsigned vgrid = grid_for(n, kBfsBlock, 8192), lgrid = 2048;
    const char *se = std::getenv("GX_BFS_PARENT_SHORT");   // rows up to this length are one thread's
    const int short_deg = se ? std::max(0, std::atoi(se)) : kParentShort;
    KTimer kt(g->ctx, "bfs_parents", s);
    GX_HIP_TRY(hipMemsetAsync(w.qcount.p, 0, 4, s));
    // pull wherever gx_bfs would go bottom-up; GX_BFS_PARENT_PUSH=1 takes push there too (A/B)
    const char *pe = std::getenv("GX_BFS_PARENT_PUSH");
    if (w.in && !(pe && std::atoi(pe) != 0)) {
        hipLaunchKernelGGL(k_bfs_parent_rows<false>, dim3(vgrid), dim3(kBfsBlock), 0, s, w.in->rp.p, w.in->ci.p,
                           w.level.p, g->out_order, n, parent, w.q0.p, w.qcount.p, short_deg);
        hipLaunchKernelGGL(k_bfs_parent_long<false>, dim3(lgrid), dim3(kBfsBlock), 0, s, w.in->rp.p, w.in->ci.p,
                           w.level.p, g->out_order, w.q0.p, w.qcount.p, parent);
        return check_launch("k_bfs_parent_long");
    }
    hipLaunchKernelGGL(k_bfs_parent_init, dim3(vgrid), dim3(kBfsBlock), 0, s, w.level.p, g->out_order, n, parent);
    hipLaunchKernelGGL(k_bfs_parent_rows<true>, dim3(vgrid), dim3(kBfsBlock), 0, s, g->A.rp.p, g->A.ci.p, w.level.p,
                       g->out_order, n, parent, w.q0.p, w.qcount.p, short_deg);
    hipLaunchKernelGGL(k_bfs_parent_long<true>, dim3(lgrid), dim3(kBfsBlock), 0, s, g->A.rp.p, g->A.ci.p, w.level.p,
                       g->out_order, w.q0.p, w.qcount.p, parent);
    hipLaunchKernelGGL(k_bfs_parent_fin, dim3(vgrid), dim3(kBfsBlock), 0, s, n, parent);
    return check_launch("k_bfs_parent_fin");
}

// ---- betweenness centrality (gx_betweenness) ---------------------------------------------
// Brandes' algorithm, one source after the other, on the finished levels of bfs_levels:
//   buckets : the reached vertices counting-sorted by (level, row tier) into one n-word order
//             array (k_bc_bucket: histogram, k_bc_scan, k_bc_bucket again as the scatter), so a
//             per-level launch touches that level's vertices only and each tier gets a launch
//             of its own, sized on the host from the offsets.  Positions inside a bucket come
//             from integer atomics and differ run to run; no value depends on them.
//   sigma   : d = 1..depth, every v in bucket d pulls sigma[u] over its in-row, level[u] == d - 1.
//   delta   : d = depth-1..1, every u in bucket d pulls coef[w] = (1 + delta[w]) / sigma[w] over
//             its out-row, level[w] == d + 1, times sigma[u]; the same thread adds it to
//             centrality[u] and leaves coef[u] (level 0 holds the source alone, whose own entry
//             takes nothing).
//   probes  : a bucket of at least GX_BC_BITS rows (kBcBitsRows) tests "x is at the level pulled
//             from" in a bitmap of that level, set and cleared from that level's bucket; a
//             smaller one reads level[x].  Both see the same edges in the same order.
// A row is one thread's (at most GX_BC_SHORT entries), one wave's (at most GX_BC_LONG) or one
// workgroup's; the lane of an entry depends on its offset in the row alone and the partial sums
// meet in a fixed tree, so no floating-point atomic is needed and a result is the same bit for
// bit on every run.
constexpr int kBcShort = 32;    // GX_BC_SHORT overrides
constexpr int kBcLong = 2048;   // GX_BC_LONG overrides
constexpr uint32_t kBcBins = 768;   // (level, tier) keys counted in LDS: the first 256 levels
constexpr int64_t kBcTile = 4096;   // vertices per workgroup step of the bucket kernels
constexpr uint32_t kBcBitsRows = 1024;   // a bucket of this many rows probes a level bitmap (GX_BC_BITS overrides)

__global__ __launch_bounds__(kBfsBlock) void k_bc_depth(const int32_t *__restrict__ level, int64_t n,
                                                        int32_t *maxlevel) {
    int32_t m = 0;
    for (int64_t v = (int64_t)blockIdx.x * kBfsBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBfsBlock)
        m = max(m, level[v]);
    for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0 && m > 0) atomicMax(maxlevel, m);
}

// key of v: 3 * level + tier of its row in rp; nk (no bucket) when unreached
__device__ __forceinline__ uint32_t bc_key(const int32_t *__restrict__ level, const int64_t *__restrict__ rp,
                                           int64_t v, int32_t maxlevel, int sh, int lg, uint32_t nk) {
    const int32_t lv = level[v];
    if (lv < 0 || lv > maxlevel) return nk;
    const int64_t len = rp[v + 1] - rp[v];
    return 3u * (uint32_t)lv + (len <= sh ? 0u : (len <= lg ? 1u : 2u));
}

// SCATTER = false: cnt[key] += the vertices of each key.  SCATTER = true: cnt holds each key's
// running position (its exclusive offset at the start); order[position] = v.  A tile's keys are
// counted in LDS first, so a level's thousands of vertices cost one global atomic per tile.
template <bool SCATTER>
__global__ __launch_bounds__(kBfsBlock) void k_bc_bucket(const int32_t *__restrict__ level,
                                                         const int64_t *__restrict__ rp, int64_t n,
                                                         int32_t maxlevel, int sh, int lg, uint32_t *cnt,
                                                         int32_t *order) {
    __shared__ uint32_t bins[kBcBins];
    const uint32_t nk = 3u * (uint32_t)(maxlevel + 1);
    const uint32_t nb = min(nk, kBcBins);
    for (int64_t t0 = (int64_t)blockIdx.x * kBcTile; t0 < n; t0 += (int64_t)gridDim.x * kBcTile) {
        const int64_t t1 = min(t0 + kBcTile, n);
        for (uint32_t b = threadIdx.x; b < nb; b += kBfsBlock) bins[b] = 0;
        __syncthreads();
        for (int64_t v = t0 + threadIdx.x; v < t1; v += kBfsBlock) {
            const uint32_t key = bc_key(level, rp, v, maxlevel, sh, lg, nk);
            if (key < nb) atomicAdd(&bins[key], 1u);
            else if (!SCATTER && key < nk) atomicAdd(&cnt[key], 1u);
        }
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < nb; b += kBfsBlock) {
            const uint32_t c = bins[b];
            if (c) {
                const uint32_t base = atomicAdd(&cnt[b], c);
                if (SCATTER) bins[b] = base;
            }
        }
        if constexpr (SCATTER) {
            __syncthreads();
            for (int64_t v = t0 + threadIdx.x; v < t1; v += kBfsBlock) {
                const uint32_t key = bc_key(level, rp, v, maxlevel, sh, lg, nk);
                if (key >= nk) continue;
                const uint32_t pos = key < nb ? atomicAdd(&bins[key], 1u) : atomicAdd(&cnt[key], 1u);
                if ((int64_t)pos < n) order[pos] = (int32_t)v;
            }
        }
        __syncthreads();
    }
}

// One workgroup: off[0..nk] = exclusive scan of cnt[0..nk), and cnt becomes the scatter's cursors.
__global__ __launch_bounds__(kBfsBlock) void k_bc_scan(uint32_t *cnt, uint32_t *off, uint32_t nk) {
    __shared__ uint32_t wsum[kBfsBlock / kWave];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    uint32_t carry = 0;
    for (uint32_t i0 = 0; i0 < nk; i0 += kBfsBlock) {
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t c = i < nk ? cnt[i] : 0u;
        uint32_t x = c;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const uint32_t y = __shfl_up(x, o, kWave);
            if (lane >= o) x += y;
        }
        if (lane == kWave - 1) wsum[w] = x;
        __syncthreads();
        uint32_t before = 0, step = 0;
        for (int j = 0; j < kBfsBlock / kWave; j++) {
            if (j < w) before += wsum[j];
            step += wsum[j];
        }
        if (i < nk) {
            const uint32_t excl = carry + before + x - c;
            off[i] = excl;
            cnt[i] = excl;
        }
        carry += step;
        __syncthreads();
    }
    if (threadIdx.x == 0) off[nk] = carry;
}

__global__ void k_bc_seed(double *sigma, double *coef, int32_t src) {
    sigma[src] = 1.0;
    coef[src] = 1.0;
}

// The bits of a bucket's vertices in the level bitmap: set (integer atomicOr) before the pulls
// that probe that level, cleared word by word after them, so the cost follows the bucket and
// never n.
__global__ __launch_bounds__(kBfsBlock) void k_bc_bits(const int32_t *__restrict__ order, uint32_t count,
                                                       unsigned long long *fb, int set) {
    for (uint32_t i = blockIdx.x * kBfsBlock + threadIdx.x; i < count; i += gridDim.x * kBfsBlock) {
        const int32_t v = order[i];
        if (set) atomicOr(&fb[v >> 6], 1ull << (v & 63));
        else fb[v >> 6] = 0ull;
    }
}

// Four entries of a row, `step` apart from k (k < e): the four membership probes issue before any
// is tested; val[x] is gathered for the x at level lv1 only.  BITS: the probe reads the bitmap of
// that level (n/8 bytes, L2-resident: the bottom-up BFS's argument) instead of level[x].
template <bool BITS>
__device__ __forceinline__ double bc_quad(const int32_t *__restrict__ ci, const int32_t *__restrict__ level,
                                          const unsigned long long *__restrict__ fb, const double *val, int64_t k,
                                          int64_t step, int64_t e, int32_t lv1) {
    const int64_t last = e - 1;
    const int64_t k1 = k + step, k2 = k + 2 * step, k3 = k + 3 * step;
    const int32_t x0 = ci[k];
    const int32_t x1 = ci[min(k1, last)];
    const int32_t x2 = ci[min(k2, last)];
    const int32_t x3 = ci[min(k3, last)];
    bool h0, h1, h2, h3;
    if constexpr (BITS) {
        const unsigned long long w0 = fb[x0 >> 6], w1 = fb[x1 >> 6], w2 = fb[x2 >> 6], w3 = fb[x3 >> 6];
        h0 = (w0 >> (x0 & 63)) & 1ull;
        h1 = (w1 >> (x1 & 63)) & 1ull;
        h2 = (w2 >> (x2 & 63)) & 1ull;
        h3 = (w3 >> (x3 & 63)) & 1ull;
    } else {
        const int32_t l0 = level[x0], l1 = level[x1], l2 = level[x2], l3 = level[x3];
        h0 = l0 == lv1;
        h1 = l1 == lv1;
        h2 = l2 == lv1;
        h3 = l3 == lv1;
    }
    const double t0 = h0 ? val[x0] : 0.0;
    const double t1 = (h1 && k1 < e) ? val[x1] : 0.0;
    const double t2 = (h2 && k2 < e) ? val[x2] : 0.0;
    const double t3 = (h3 && k3 < e) ? val[x3] : 0.0;
    return (t0 + t1) + (t2 + t3);
}

// coef[w] = (1 + delta[w]) / sigma[w], what a parent u of w adds to delta[u] / sigma[u]: one
// division per vertex, when its delta is final (1 / sigma[w] until then: delta = 0 at the deepest
// level), and one gather per tree edge in the delta pull.  delta itself is never stored.
template <bool BACK>
__device__ __forceinline__ void bc_store(double acc, int32_t v, double *sigma, double *coef, double *cent) {
    if constexpr (BACK) {
        const double sg = sigma[v], d = sg * acc;
        coef[v] = (1.0 + d) / sg;
        cent[v] += d;
    } else {
        sigma[v] = acc;
        coef[v] = 1.0 / acc;
    }
}

// One thread per row of the bucket order[0..count).
template <bool BACK, bool BITS>
__global__ __launch_bounds__(kBfsBlock) void k_bc_rows(const int64_t *__restrict__ rp,
                                                       const int32_t *__restrict__ ci,
                                                       const int32_t *__restrict__ level,
                                                       const unsigned long long *__restrict__ fb,
                                                       const int32_t *__restrict__ order, uint32_t count,
                                                       int32_t lv1, double *sigma, double *coef, double *cent) {
    const double *val = BACK ? coef : sigma;
    for (uint32_t i = blockIdx.x * kBfsBlock + threadIdx.x; i < count; i += gridDim.x * kBfsBlock) {
        const int32_t v = order[i];
        const int64_t b = rp[v], e = rp[v + 1];
        double acc = 0.0;
        for (int64_t k = b; k < e; k += 4) acc += bc_quad<BITS>(ci, level, fb, val, k, 1, e, lv1);
        bc_store<BACK>(acc, v, sigma, coef, cent);
    }
}

// One wave per row: lane l takes the entries l, l + 64, ... of the row, then a fixed xor tree.
template <bool BACK, bool BITS>
__global__ __launch_bounds__(kBfsBlock) void k_bc_wave(const int64_t *__restrict__ rp,
                                                       const int32_t *__restrict__ ci,
                                                       const int32_t *__restrict__ level,
                                                       const unsigned long long *__restrict__ fb,
                                                       const int32_t *__restrict__ order, uint32_t count,
                                                       int32_t lv1, double *sigma, double *coef, double *cent) {
    const double *val = BACK ? coef : sigma;
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = (blockIdx.x * kBfsBlock + threadIdx.x) / kWave;
    const uint32_t nwaves = gridDim.x * (kBfsBlock / kWave);
    for (uint32_t i = wave; i < count; i += nwaves) {
        const int32_t v = order[i];
        const int64_t b = rp[v], e = rp[v + 1];
        double acc = 0.0;
        for (int64_t k = b + lane; k < e; k += 4 * kWave) acc += bc_quad<BITS>(ci, level, fb, val, k, kWave, e, lv1);
        acc = wave_sum(acc);
        if (lane == 0) bc_store<BACK>(acc, v, sigma, coef, cent);
    }
}

// One workgroup per row: thread t takes the entries t, t + 256, ...; each wave's xor tree, then
// the four wave sums from LDS in a fixed order.
template <bool BACK, bool BITS>
__global__ __launch_bounds__(kBfsBlock) void k_bc_block(const int64_t *__restrict__ rp,
                                                        const int32_t *__restrict__ ci,
                                                        const int32_t *__restrict__ level,
                                                        const unsigned long long *__restrict__ fb,
                                                        const int32_t *__restrict__ order, uint32_t count,
                                                        int32_t lv1, double *sigma, double *coef, double *cent) {
    static_assert(kBfsBlock / kWave == 4, "the LDS tree below adds four wave sums");
    __shared__ double red[kBfsBlock / kWave];
    const double *val = BACK ? coef : sigma;
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        const int32_t v = order[i];
        const int64_t b = rp[v], e = rp[v + 1];
        double acc = 0.0;
        for (int64_t k = b + threadIdx.x; k < e; k += 4 * kBfsBlock)
            acc += bc_quad<BITS>(ci, level, fb, val, k, kBfsBlock, e, lv1);
        acc = wave_sum(acc);
        if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = acc;
        __syncthreads();
        if (threadIdx.x == 0) bc_store<BACK>((red[0] + red[1]) + (red[2] + red[3]), v, sigma, coef, cent);
        __syncthreads();
    }
}

struct BcWork {
    DBuf<double> sigma, coef, cent;
    DBuf<int32_t> order_in, order_out;   // bucketed by the tiers of the in-rows / the out-rows
    DBuf<unsigned long long> bits;       // level bitmap, all clear between launches
    DBuf<uint32_t> cnt, off;
    DBuf<int32_t> maxlevel;
    std::vector<uint32_t> h_off_in, h_off_out;
    int sh = kBcShort, lg = kBcLong;
    uint32_t bits_rows = kBcBitsRows;
};

// order / h_off: the reached vertices of `level` by (level, tier of their row in rp); h_off has
// 3 * (maxlevel + 1) + 1 entries.  Synchronises the stream (the offsets size the launches).
int bc_buckets(gx_graph *g, const int32_t *level, const int64_t *rp, int32_t maxlevel, BcWork &b, int32_t *order,
               std::vector<uint32_t> &h_off, hipStream_t s) {
    const int64_t n = (int64_t)g->n;
    const uint32_t nk = 3u * (uint32_t)(maxlevel + 1);
    if (b.cnt.n < (size_t)nk + 1) {
        GX_TRY(b.cnt.alloc(2 * (size_t)nk + 1));
        GX_TRY(b.off.alloc(2 * (size_t)nk + 1));
    }
    const unsigned grid = (unsigned)std::min<int64_t>((n + kBcTile - 1) / kBcTile, 1024);
    GX_HIP_TRY(hipMemsetAsync(b.cnt.p, 0, (size_t)nk * 4, s));
    hipLaunchKernelGGL(k_bc_bucket<false>, dim3(grid), dim3(kBfsBlock), 0, s, level, rp, n, maxlevel, b.sh, b.lg,
                       b.cnt.p, order);
    hipLaunchKernelGGL(k_bc_scan, dim3(1), dim3(kBfsBlock), 0, s, b.cnt.p, b.off.p, nk);
    hipLaunchKernelGGL(k_bc_bucket<true>, dim3(grid), dim3(kBfsBlock), 0, s, level, rp, n, maxlevel, b.sh, b.lg,
                       b.cnt.p, order);
    GX_TRY(check_launch("k_bc_bucket"));
    h_off.resize((size_t)nk + 1);
    GX_HIP_TRY(hipMemcpyAsync(h_off.data(), b.off.p, ((size_t)nk + 1) * 4, hipMemcpyDeviceToHost, s));
    GX_HIP_TRY(hipStreamSynchronize(s));
    if (h_off[nk] > (uint64_t)n) return fail(GX_PANIC, "gx_betweenness: bucket offsets exceed n");
    return GX_SUCCESS;
}

// The launches of level d's bucket, one per non-empty tier, probing level lv1.  A bucket of at
// least bits_rows rows probes the bitmap of level lv1, set from that level's bucket (of order_in:
// the same vertices in either order array) and cleared again; a smaller one reads level[x].
template <bool BACK>
void bc_level(const DevCSR &m, const int32_t *level, const int32_t *order, const std::vector<uint32_t> &h_off,
              int32_t d, int32_t lv1, BcWork &b, hipStream_t s) {
    const uint32_t *o = h_off.data() + 3 * (size_t)d;
    const uint32_t *p = b.h_off_in.data() + 3 * (size_t)lv1;
    const uint32_t probed = p[3] - p[0];
    const bool bits = o[3] - o[0] >= b.bits_rows && probed > 0;
    const unsigned long long *fb = b.bits.p;
    auto mark = [&](int set) {
        hipLaunchKernelGGL(k_bc_bits, dim3(grid_for(probed, kBfsBlock, 2048)), dim3(kBfsBlock), 0, s,
                           b.order_in.p + p[0], probed, b.bits.p, set);
    };
    if (bits) mark(1);
    if (const uint32_t c = o[1] - o[0]) {
        const dim3 grid(grid_for(c, kBfsBlock, 8192));
        if (bits)
            hipLaunchKernelGGL((k_bc_rows<BACK, true>), grid, dim3(kBfsBlock), 0, s, m.rp.p, m.ci.p, level, fb,
                               order + o[0], c, lv1, b.sigma.p, b.coef.p, b.cent.p);
        else
            hipLaunchKernelGGL((k_bc_rows<BACK, false>), grid, dim3(kBfsBlock), 0, s, m.rp.p, m.ci.p, level, fb,
                               order + o[0], c, lv1, b.sigma.p, b.coef.p, b.cent.p);
    }
    if (const uint32_t c = o[2] - o[1]) {
        const dim3 grid(grid_for((uint64_t)c * kWave, kBfsBlock, 8192));
        if (bits)
            hipLaunchKernelGGL((k_bc_wave<BACK, true>), grid, dim3(kBfsBlock), 0, s, m.rp.p, m.ci.p, level, fb,
                               order + o[1], c, lv1, b.sigma.p, b.coef.p, b.cent.p);
        else
            hipLaunchKernelGGL((k_bc_wave<BACK, false>), grid, dim3(kBfsBlock), 0, s, m.rp.p, m.ci.p, level, fb,
                               order + o[1], c, lv1, b.sigma.p, b.coef.p, b.cent.p);
    }
    if (const uint32_t c = o[3] - o[2]) {
        const dim3 grid(std::min(c, 4096u));
        if (bits)
            hipLaunchKernelGGL((k_bc_block<BACK, true>), grid, dim3(kBfsBlock), 0, s, m.rp.p, m.ci.p, level, fb,
                               order + o[2], c, lv1, b.sigma.p, b.coef.p, b.cent.p);
        else
            hipLaunchKernelGGL((k_bc_block<BACK, false>), grid, dim3(kBfsBlock), 0, s, m.rp.p, m.ci.p, level, fb,
                               order + o[2], c, lv1, b.sigma.p, b.coef.p, b.cent.p);
    }
    if (bits) mark(0);
}

// Brandes' two passes over w's finished levels from src: sigma (left in b.sigma for the caller's
// paths row) and the dependencies, added into b.cent.
int bc_source(gx_graph *g, uint64_t src, BfsWork &w, BcWork &b, hipStream_t s) {
    gx_ctx *ctx = g->ctx;
    const int64_t n = (int64_t)g->n;
    const DevCSR &in = g->directed ? g->AT : g->A;
    int32_t maxlevel = 0;
    {
        KTimer kt(ctx, "bc_bucket", s);
        GX_HIP_TRY(hipMemsetAsync(b.maxlevel.p, 0, 4, s));
        hipLaunchKernelGGL(k_bc_depth, dim3(grid_for(n, kBfsBlock, 1024)), dim3(kBfsBlock), 0, s, w.level.p, n,
                           b.maxlevel.p);
        GX_TRY(check_launch("k_bc_depth"));
        GX_HIP_TRY(hipMemcpyAsync(&maxlevel, b.maxlevel.p, 4, hipMemcpyDeviceToHost, s));
        GX_HIP_TRY(hipStreamSynchronize(s));
        if (maxlevel < 0 || maxlevel >= n) return fail(GX_PANIC, "gx_betweenness: level out of range");
        GX_TRY(bc_buckets(g, w.level.p, in.rp.p, maxlevel, b, b.order_in.p, b.h_off_in, s));
        if (g->directed) GX_TRY(bc_buckets(g, w.level.p, g->A.rp.p, maxlevel, b, b.order_out.p, b.h_off_out, s));
    }
    const int32_t *order_out = g->directed ? b.order_out.p : b.order_in.p;
    const std::vector<uint32_t> &h_off_out = g->directed ? b.h_off_out : b.h_off_in;
    GX_HIP_TRY(hipMemsetAsync(b.sigma.p, 0, (size_t)n * 8, s));
    hipLaunchKernelGGL(k_bc_seed, dim3(1), dim3(1), 0, s, b.sigma.p, b.coef.p, (int32_t)src);
    {
        KTimer kt(ctx, "bc_sigma", s);
        for (int32_t d = 1; d <= maxlevel; d++)
            bc_level<false>(in, w.level.p, b.order_in.p, b.h_off_in, d, d - 1, b, s);
    }
    GX_TRY(check_launch("k_bc_rows (sigma)"));
    {
        KTimer kt(ctx, "bc_delta", s);
        for (int32_t d = maxlevel - 1; d >= 1; d--)
            bc_level<true>(g->A, w.level.p, order_out, h_off_out, d, d + 1, b, s);
    }
    return check_launch("k_bc_rows (delta)");
}

}  // namespace
}  // namespace gx

using namespace gx;

extern "C" int gx_bfs(gx_graph *g, uint64_t src, int64_t *level_out) {
    if (!g || !level_out) return fail(GX_NULL_POINTER, "gx_bfs: null argument");
    if (src >= g->n) return fail(GX_INVALID_INDEX, "gx_bfs: source out of range");
    {
        gx_graph *h = nullptr;   // hub-first copy from the second call (gx_runtime.hip hub_for)
        GX_TRY(hub_for(g, ++g->hub_bfs_calls, &h, &src));
        if (h) return gx_bfs(h, src, level_out);
    }
    BfsWork w;
    const void *res = nullptr;
    GX_TRY(bfs_levels(g, src, w, [&](bool, bool &queued) -> int {
        queued = true;
        return remap_out(g, w.level.p, 4, g->ctx->stream, &res);
    }));
    GX_TRY(device_end(g->ctx));
    GX_TRY(download(g->ctx, level_out, res, g->n, Xfer::Levels));
    return GX_SUCCESS;
}

extern "C" int gx_bfs_parent(gx_graph *g, uint64_t src, int64_t *level_out, int64_t *parent_out) {
    if (!g || !parent_out) return fail(GX_NULL_POINTER, "gx_bfs_parent: null argument");
    if (src >= g->n) return fail(GX_INVALID_INDEX, "gx_bfs_parent: source out of range");
    {
        gx_graph *h = nullptr;   // a parent call counts as a BFS call: the copy from the second
        GX_TRY(hub_for(g, ++g->hub_bfs_calls, &h, &src));
        if (h) return gx_bfs_parent(h, src, level_out, parent_out);
    }
    GX_HIP_TRY(hipSetDevice(g->ctx->device));
    BfsWork w;
    DBuf<int32_t> parent;
    GX_TRY(parent.alloc(g->n));
    const void *res_level = nullptr, *res_parent = nullptr;
    // the parent pass reads finished levels and the loop's queue: never queued early
    GX_TRY(bfs_levels(g, src, w, [&](bool early, bool &queued) -> int {
        if (early) return GX_SUCCESS;
        queued = true;
        hipStream_t s = g->ctx->stream;
        GX_TRY(bfs_parents(g, w, parent.p, s));
        // on a copy the two results share remap_tmp: the levels its low 4-byte half, the parents its high
        if (level_out) GX_TRY(remap_out(g, w.level.p, 4, s, &res_level, 0));
        return remap_out(g, parent.p, 4, s, &res_parent, 1);
    }));
    GX_TRY(device_end(g->ctx));
    if (level_out) GX_TRY(download(g->ctx, level_out, res_level, g->n, Xfer::Levels));
    GX_TRY(download(g->ctx, parent_out, res_parent, g->n, Xfer::Sign32));
    return GX_SUCCESS;
}

extern "C" int gx_betweenness(gx_graph *g, const uint64_t *sources, uint64_t ns, double *centrality,
                              double *paths) {
    if (!g || !centrality || (ns > 0 && !sources)) return fail(GX_NULL_POINTER, "gx_betweenness: null argument");
    for (uint64_t k = 0; k < ns; k++)
        if (sources[k] >= g->n) return fail(GX_INVALID_INDEX, "gx_betweenness: source out of range");
    gx_ctx *ctx = g->ctx;
    GX_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const char *se = std::getenv("GX_BC_SHORT"), *le = std::getenv("GX_BC_LONG");
    BcWork b;
    b.sh = se ? std::max(0, std::atoi(se)) : kBcShort;
    b.lg = std::max(b.sh, le ? std::atoi(le) : kBcLong);
    // rows a bucket needs to probe a level bitmap: 0 always, -1 never
    if (const char *be = std::getenv("GX_BC_BITS")) b.bits_rows = (uint32_t)std::atoll(be);
    // the sigma pass reads in-edges whatever GX_BFS_TRANSPOSE says; built before the bracket
    if (g->directed) GX_TRY(ensure_transpose(g));
    GX_TRY(b.sigma.alloc(g->n));
    GX_TRY(b.coef.alloc(g->n));
    GX_TRY(b.bits.alloc(g->n / 64 + 1));
    GX_TRY(b.cent.alloc(g->n));
    GX_TRY(b.order_in.alloc(g->n));
    if (g->directed) GX_TRY(b.order_out.alloc(g->n));
    GX_TRY(b.maxlevel.alloc(1));
    GX_TRY(device_begin(ctx));
    GX_HIP_TRY(hipMemsetAsync(b.cent.p, 0, g->n * 8, s));
    GX_HIP_TRY(hipMemsetAsync(b.bits.p, 0, (g->n / 64 + 1) * 8, s));
    // g itself, never its hub-first copy: the copy permutes the rows, and with them the order
    // of every sum, between a graph's first and second call
    BfsWork w;
    for (uint64_t k = 0; k < ns; k++) {
        GX_TRY(bfs_levels(g, sources[k], w, [](bool, bool &queued) -> int {
            queued = true;
            return GX_SUCCESS;
        }, false));
        GX_TRY(bc_source(g, sources[k], w, b, s));
        if (paths) GX_TRY(download(ctx, paths + k * g->n, b.sigma.p, g->n, Xfer::Raw64));
    }
    GX_TRY(device_end(ctx));
    GX_TRY(download(ctx, centrality, b.cent.p, g->n, Xfer::Raw64));
    return GX_SUCCESS;
}

GX_MODULE_WARMER(bfs)

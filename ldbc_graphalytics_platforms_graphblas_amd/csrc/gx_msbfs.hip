// gx_msbfs.hip -- bit-parallel multi-source BFS (the role of LAGraph_MultiSourceBFS).
//
// Up to GX_MSBFS_BATCH = 64 traversals advance together: bit k of a 64-bit word per vertex stands
// for source k of the batch.  Three words per vertex: seen (reached so far), front (reached at the
// current level) and next (the push form's accumulator / the pull form's new frontier).  A level
// reads the adjacency once for all 64 sources; the per-edge work is one 8-byte gather and an OR.
//   pull   : every vertex v with need = ~seen[v] & live ORs front[u] over its in-row until the
//            accumulated word covers need; acc & need is v's part of the new frontier, written
//            with a plain store into next (then front and next swap).  A row belongs to one thread
//            (at most kMsShort entries), one wave (at most kMsLong) or one workgroup; the long
//            rows are listed once per call.  The commit is fused: no atomics on the vertex words.
//   push   : over a compact list of work items (frontier vertex, chunk of <= 256 out-edges); for
//            m = front[u] and every out-neighbour v one no-return atomicOr(&next[v], m & ~seen[v]),
//            issued only when that word is non-zero.  seen changes in the commit alone, so a stale
//            read only costs a redundant atomic.  The commit pass turns next into the new front.
// Every commit records level d + 1 for the new bits (source-major int32 rows, so the lanes of one
// bit store to consecutive addresses and a row downloads like gx_bfs's levels), counts the new
// bits per source (one ballot per bit present in the wave), and sums the new frontier's vertices
// and out-edges for the host, which reads them once per level to choose the next form.
// All sums are integer; a result is the same bit for bit on every run.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "gx_device.h"

namespace gx {
namespace {

using u64 = unsigned long long;

constexpr int kMsBatch = 64;             // GX_MSBFS_BATCH
constexpr int kMsBlock = 256;
constexpr int kMsWaves = kMsBlock / kWave;
constexpr int kMsChunk = 256;            // out-edges per push work item (4 per lane)
constexpr int kMsShort = 128;            // in-rows up to this length are one thread's
constexpr int kMsLong = 2048;            // ... up to this one wave's, longer ones a workgroup's
constexpr int64_t kMsTile = 4096;        // vertices per workgroup step of the tier listing
constexpr unsigned kMsGrid = 1024;       // cap of every grid = rows of the per-workgroup tallies
constexpr int kMsShards = 32;            // the frontier counters, one 128-byte line per shard
constexpr int kMsShardWords = 16;
// push while the frontier's out-edges <= nnz / alpha (GX_MSBFS_ALPHA).  SYN-g500-22: 64 5.37 ms,
// 256 4.42, 1 024 6.16; a 1 024 x 256 grid, 1 277 levels: 16 49.2, 64 30.2, 256 29.4, 1 024 29.0
// (profiles/msbfs_alpha_ab.txt)
constexpr u64 kMsAlpha = 256;

static_assert(kMsBatch == kWave, "lane k tallies bit k");
static_assert(kMsWaves == 4, "the LDS combines below take four waves");

__device__ __forceinline__ u64 wave_or(u64 x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x |= __shfl_xor(x, off, kWave);
    return x;
}

__device__ __forceinline__ u64 wave_add(u64 x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, kWave);
    return x;
}

// The new bits nw of the 64 vertices a wave holds (lane = vertex; 0 for a lane past n): for
// every bit k some lane has, the lanes that have it store level d1 to row k (consecutive
// addresses) and lane k adds their number to its tally.  Every lane of the wave must call it.
template <bool LEVELS>
__device__ __forceinline__ void record_lanes(u64 nw, int64_t v, int64_t n, int32_t d1, int32_t *lev, int lane,
                                             u64 &tally) {
    u64 any = wave_or(nw);
    // every lane holds the same word: keep it, and the loop, in scalar registers
    any = ((u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(any >> 32)) << 32) |
          (u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)any);
    while (any) {
        const int k = __builtin_ctzll(any);
        any &= any - 1;
        const bool has = (nw >> k) & 1ull;
        const u64 holders = __ballot(has);
        if (lane == k) tally += (u64)__popcll(holders);
        if (LEVELS && has) lev[(int64_t)k * n + v] = d1;
    }
}

// The same for one vertex whose new bits every lane knows: lane k is bit k.
template <bool LEVELS>
__device__ __forceinline__ void record_vertex(u64 nw, int64_t v, int64_t n, int32_t d1, int32_t *lev, int lane,
                                              u64 &tally) {
    if ((nw >> lane) & 1ull) {
        tally++;
        if (LEVELS) lev[(int64_t)lane * n + v] = d1;
    }
}

// End of a commit: the workgroup's per-bit tallies go to its own row of `part` (count, sum of
// levels, last level with a count: 3 x 64 words; launches are ordered on the stream and a row is
// one workgroup's, so plain read-modify-write), its found vertices and their out-edges to one
// shard of the frontier counters, one atomic each per workgroup.
__device__ __forceinline__ void block_finish(u64 tally, u64 found, u64 edges, int32_t d1, u64 *part, u64 *counters) {
    __shared__ u64 red[kMsWaves][kWave];
    __shared__ u64 fe[2][kMsWaves];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    found = wave_add(found);
    edges = wave_add(edges);
    red[w][lane] = tally;
    if (lane == 0) {
        fe[0][w] = found;
        fe[1][w] = edges;
    }
    __syncthreads();
    if (threadIdx.x < kWave) {
        const u64 c = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
        if (c) {
            u64 *p = part + (size_t)blockIdx.x * 3 * kWave;
            p[lane] += c;
            p[kWave + lane] += c * (u64)d1;
            p[2 * kWave + lane] = (u64)d1;
        }
    }
    if (threadIdx.x == 0) {
        const u64 f = (fe[0][0] + fe[0][1]) + (fe[0][2] + fe[0][3]);
        const u64 e = (fe[1][0] + fe[1][1]) + (fe[1][2] + fe[1][3]);
        u64 *c = counters + (size_t)(blockIdx.x % kMsShards) * kMsShardWords;
        if (f) atomicAdd(&c[0], f);
        if (e) atomicAdd(&c[1], e);
    }
}

// The batch's sources: bit k at sources[k] (atomic: a vertex may be listed twice), level 0.
__global__ void k_msbfs_seed(const uint64_t *__restrict__ src, int nb, const int64_t *__restrict__ rpo, u64 *seen,
                             u64 *front, int32_t *lev, int64_t n, u64 *counters) {
    const int k = threadIdx.x;
    if (k >= nb) return;
    const int64_t v = (int64_t)src[k];
    const u64 bit = 1ull << k;
    atomicOr(&seen[v], bit);
    atomicOr(&front[v], bit);
    if (lev) lev[(int64_t)k * n + v] = 0;
    atomicAdd(&counters[0], 1ull);
    atomicAdd(&counters[1], (u64)(rpo[v + 1] - rpo[v]));
}

// The vertices whose in-row is longer than short_len, once per call: the wave tier's from the
// front of `tiers` (n words), the workgroup tier's from its back; tcount = their numbers.  A
// tile's entries are gathered in LDS first: two global atomics per tile.
__global__ __launch_bounds__(kMsBlock) void k_msbfs_tiers(const int64_t *__restrict__ rpi, int64_t n, int short_len,
                                                          int long_len, int32_t *tiers, uint32_t *tcount) {
    __shared__ int32_t loc[kMsTile];
    __shared__ uint32_t c[2], base[2];
    for (int64_t t0 = (int64_t)blockIdx.x * kMsTile; t0 < n; t0 += (int64_t)gridDim.x * kMsTile) {
        const int64_t t1 = min(t0 + kMsTile, n);
        if (threadIdx.x < 2) c[threadIdx.x] = 0;
        __syncthreads();
        for (int64_t v = t0 + threadIdx.x; v < t1; v += kMsBlock) {
            const int64_t len = rpi[v + 1] - rpi[v];
            if (len > long_len) loc[kMsTile - 1 - atomicAdd(&c[1], 1u)] = (int32_t)v;
            else if (len > short_len) loc[atomicAdd(&c[0], 1u)] = (int32_t)v;
        }
        __syncthreads();
        if (threadIdx.x < 2 && c[threadIdx.x]) base[threadIdx.x] = atomicAdd(&tcount[threadIdx.x], c[threadIdx.x]);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < c[0]; i += kMsBlock) tiers[base[0] + i] = loc[i];
        for (uint32_t i = threadIdx.x; i < c[1]; i += kMsBlock) tiers[n - 1 - (base[1] + i)] = loc[kMsTile - 1 - i];
        __syncthreads();
    }
}

// pull, thread tier: one thread per vertex, four gathers in flight per step; writes next[v] for
// every v (0 for a long row: its tier's kernel, queued behind this one, overwrites it).
template <bool LEVELS>
__global__ __launch_bounds__(kMsBlock) void k_msbfs_pull(const int64_t *__restrict__ rpi,
                                                         const int32_t *__restrict__ cii,
                                                         const int64_t *__restrict__ rpo, u64 *seen,
                                                         const u64 *__restrict__ front, u64 *next, int64_t n, u64 live,
                                                         int32_t d1, int short_len, int32_t *lev, u64 *part,
                                                         u64 *counters) {
    const int lane = threadIdx.x & (kWave - 1);
    u64 tally = 0, found = 0, edges = 0;
    const int64_t stride = (int64_t)gridDim.x * kMsBlock;
    const int64_t nround = (n + stride - 1) / stride;   // uniform trip count: record_lanes shuffles
    for (int64_t r = 0; r < nround; r++) {
        const int64_t v = r * stride + (int64_t)blockIdx.x * kMsBlock + threadIdx.x;
        u64 nw = 0;
        if (v < n) {
            const u64 s = seen[v];
            const u64 need = ~s & live;
            if (need) {
                const int64_t b = rpi[v], e = rpi[v + 1];
                if (e - b <= short_len) {
                    const int64_t last = e - 1;
                    u64 acc = 0;
                    // stops once EVERY needed bit is found, not on the first one
                    for (int64_t k = b; k < e && (acc & need) != need; k += 4) {
                        const int32_t u0 = cii[k];
                        const int32_t u1 = cii[min(k + 1, last)];
                        const int32_t u2 = cii[min(k + 2, last)];
                        const int32_t u3 = cii[min(k + 3, last)];
                        acc |= (front[u0] | front[u1]) | (front[u2] | front[u3]);
                    }
                    nw = acc & need;
                    if (nw) {
                        seen[v] = s | nw;
                        found++;
                        edges += (u64)(rpo[v + 1] - rpo[v]);
                    }
                }
            }
            next[v] = nw;
        }
        record_lanes<LEVELS>(nw, v, n, d1, lev, lane, tally);
    }
    block_finish(tally, found, edges, d1, part, counters);
}

// pull, wave tier: one wave per listed vertex, 128 entries per step, OR-reduced across the lanes.
template <bool LEVELS>
__global__ __launch_bounds__(kMsBlock) void k_msbfs_pull_wave(const int64_t *__restrict__ rpi,
                                                              const int32_t *__restrict__ cii,
                                                              const int64_t *__restrict__ rpo,
                                                              const int32_t *__restrict__ list, uint32_t count,
                                                              u64 *seen, const u64 *__restrict__ front, u64 *next,
                                                              int64_t n, u64 live, int32_t d1, int32_t *lev, u64 *part,
                                                              u64 *counters) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = (blockIdx.x * kMsBlock + threadIdx.x) / kWave;
    const uint32_t nwaves = gridDim.x * kMsWaves;
    u64 tally = 0, found = 0, edges = 0;
    for (uint32_t i = wave; i < count; i += nwaves) {
        const int64_t v = list[i];
        const u64 s = seen[v];
        const u64 need = ~s & live;
        if (!need) continue;
        const int64_t b = rpi[v], e = rpi[v + 1];
        u64 acc = 0;
        for (int64_t kb = b; kb < e; kb += 2 * kWave) {
            const int64_t k0 = kb + lane, k1 = k0 + kWave;
            u64 x = 0;
            if (k0 < e) x = front[cii[k0]];
            if (k1 < e) x |= front[cii[k1]];
            acc |= wave_or(x);
            if ((acc & need) == need) break;
        }
        const u64 nw = acc & need;
        if (!nw) continue;
        if (lane == 0) {
            seen[v] = s | nw;
            next[v] = nw;
            found++;
            edges += (u64)(rpo[v + 1] - rpo[v]);
        }
        record_vertex<LEVELS>(nw, v, n, d1, lev, lane, tally);
    }
    block_finish(tally, found, edges, d1, part, counters);
}

// pull, workgroup tier: one workgroup per listed vertex, 1 024 entries per step; each wave's OR,
// then the four wave words through LDS.
template <bool LEVELS>
__global__ __launch_bounds__(kMsBlock) void k_msbfs_pull_block(const int64_t *__restrict__ rpi,
                                                               const int32_t *__restrict__ cii,
                                                               const int64_t *__restrict__ rpo,
                                                               const int32_t *__restrict__ list, uint32_t count,
                                                               u64 *seen, const u64 *__restrict__ front, u64 *next,
                                                               int64_t n, u64 live, int32_t d1, int32_t *lev, u64 *part,
                                                               u64 *counters) {
    __shared__ u64 wor[kMsWaves];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    u64 tally = 0, found = 0, edges = 0;
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        const int64_t v = list[i];
        const u64 s = seen[v];   // written by thread 0 alone, after the loop's last barrier
        const u64 need = ~s & live;
        if (!need) continue;     // the same for every thread
        const int64_t b = rpi[v], e = rpi[v + 1];
        u64 acc = 0;
        for (int64_t kb = b; kb < e; kb += 4 * kMsBlock) {
            u64 x = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int64_t k = kb + (int64_t)j * kMsBlock + threadIdx.x;
                if (k < e) x |= front[cii[k]];
            }
            x = wave_or(x);
            if (lane == 0) wor[w] = x;
            __syncthreads();
            acc |= (wor[0] | wor[1]) | (wor[2] | wor[3]);
            __syncthreads();
            if ((acc & need) == need) break;
        }
        const u64 nw = acc & need;
        if (!nw) continue;
        if (threadIdx.x == 0) {
            seen[v] = s | nw;
            next[v] = nw;
            found++;
            edges += (u64)(rpo[v + 1] - rpo[v]);
        }
        if (w == 0) record_vertex<LEVELS>(nw, v, n, d1, lev, lane, tally);
    }
    block_finish(tally, found, edges, d1, part, counters);
}

// push list: (vertex << 32 | chunk) for every chunk of kMsChunk out-edges of a frontier vertex;
// one wave-aggregated append per wave that holds frontier vertices (push runs on small frontiers).
__global__ __launch_bounds__(kMsBlock) void k_msbfs_list(const int64_t *__restrict__ rpo,
                                                         const u64 *__restrict__ front, int64_t n, uint64_t *queue,
                                                         uint32_t *qcount) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t stride = (int64_t)gridDim.x * kMsBlock;
    const int64_t nround = (n + stride - 1) / stride;
    for (int64_t r = 0; r < nround; r++) {
        const int64_t v = r * stride + (int64_t)blockIdx.x * kMsBlock + threadIdx.x;
        uint32_t k = 0;
        if (v < n && front[v] != 0) k = (uint32_t)((rpo[v + 1] - rpo[v] + kMsChunk - 1) / kMsChunk);
        uint32_t x = k;   // inclusive scan of the lanes' item counts
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const uint32_t y = __shfl_up(x, off, kWave);
            if (lane >= off) x += y;
        }
        const uint32_t total = __shfl(x, kWave - 1, kWave);
        if (total == 0) continue;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(qcount, total);
        base = __shfl(base, 0, kWave);
        const uint32_t excl = x - k;
        for (uint32_t j = 0; j < k; j++) queue[base + excl + j] = ((uint64_t)(uint32_t)v << 32) | j;
    }
}

// push: one wave per work item.  The atomic's result is unused, so it is the no-return form.
__global__ __launch_bounds__(kMsBlock) void k_msbfs_push(const int64_t *__restrict__ rpo,
                                                         const int32_t *__restrict__ cio,
                                                         const uint64_t *__restrict__ queue,
                                                         const uint32_t *__restrict__ qcount,
                                                         const u64 *__restrict__ seen, const u64 *__restrict__ front,
                                                         u64 *next) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = (blockIdx.x * kMsBlock + threadIdx.x) / kWave;
    const uint32_t nwaves = gridDim.x * kMsWaves;
    const uint32_t qsize = *qcount;
    for (uint32_t f = wave; f < qsize; f += nwaves) {
        const uint64_t item = queue[f];
        const int32_t u = (int32_t)(item >> 32);
        const u64 m = front[u];
        const int64_t b = rpo[u] + (int64_t)(uint32_t)item * kMsChunk;
        const int64_t end = min(rpo[u + 1], b + kMsChunk);
#pragma unroll
        for (int i = 0; i < kMsChunk / kWave; i++) {
            const int64_t k = b + lane + (int64_t)i * kWave;
            if (k < end) {
                const int32_t v = cio[k];
                const u64 t = m & ~seen[v];
                if (t) (void)__hip_atomic_fetch_or(&next[v], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// commit after a push level: new = next & ~seen; seen |= new; front = new; next = 0.
template <bool LEVELS>
__global__ __launch_bounds__(kMsBlock) void k_msbfs_commit(const int64_t *__restrict__ rpo, u64 *seen, u64 *front,
                                                           u64 *next, int64_t n, int32_t d1, int32_t *lev, u64 *part,
                                                           u64 *counters) {
    const int lane = threadIdx.x & (kWave - 1);
    u64 tally = 0, found = 0, edges = 0;
    const int64_t stride = (int64_t)gridDim.x * kMsBlock;
    const int64_t nround = (n + stride - 1) / stride;
    for (int64_t r = 0; r < nround; r++) {
        const int64_t v = r * stride + (int64_t)blockIdx.x * kMsBlock + threadIdx.x;
        u64 nw = 0;
        if (v < n) {
            const u64 x = next[v];
            if (x) {
                const u64 s = seen[v];
                nw = x & ~s;
                next[v] = 0;
                if (nw) {
                    seen[v] = s | nw;
                    found++;
                    edges += (u64)(rpo[v + 1] - rpo[v]);
                }
            }
            front[v] = nw;
        }
        record_lanes<LEVELS>(nw, v, n, d1, lev, lane, tally);
    }
    block_finish(tally, found, edges, d1, part, counters);
}

// statistics of source k (workgroup k): the tallies' rows summed; the source itself is level 0.
__global__ __launch_bounds__(kMsBlock) void k_msbfs_out(const u64 *__restrict__ part, unsigned rows, u64 *stats) {
    __shared__ u64 red[3][kMsWaves];
    const int k = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    u64 c = 0, sum = 0, mx = 0;
    for (unsigned b = threadIdx.x; b < rows; b += kMsBlock) {
        const u64 *p = part + (size_t)b * 3 * kWave;
        c += p[k];
        sum += p[kWave + k];
        mx = max(mx, p[2 * kWave + k]);
    }
    c = wave_add(c);
    sum = wave_add(sum);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (u64)__shfl_xor(mx, off, kWave));
    if (lane == 0) {
        red[0][w] = c;
        red[1][w] = sum;
        red[2][w] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        stats[3 * k] = 1 + (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        stats[3 * k + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        stats[3 * k + 2] = max(max(red[2][0], red[2][1]), max(red[2][2], red[2][3]));
    }
}

// What one call holds on the device; the knobs, read once.
struct MsWork {
    DBuf<u64> words;          // seen, front, next: n words each
    DBuf<int32_t> lev;        // [batch][n], -1 = unreached (only when levels are asked for)
    DBuf<int32_t> tiers;      // wave-tier vertices from the front, workgroup-tier ones from the back
    DBuf<uint32_t> tcount;    // their numbers, then the push list's length
    DBuf<uint64_t> queue;
    DBuf<u64> part, counters, stats;
    DBuf<uint64_t> src;
    uint32_t n_wave = 0, n_block = 0;
    u64 alpha = kMsAlpha;
    int dir = 0;              // 0 by the frontier's out-edges, 1 push everywhere, 2 pull everywhere
};

// One batch of nb <= 64 sources (already on the device in w.src): the levels into w.lev (when
// allocated) and the statistics into w.stats.  The caller brackets it.
template <bool LEVELS>
int msbfs_batch(gx_graph *g, MsWork &w, int nb) {
    gx_ctx *ctx = g->ctx;
    hipStream_t s = ctx->stream;
    const int64_t n = (int64_t)g->n;
    const DevCSR &in = g->directed ? g->AT : g->A;
    const u64 live = nb == kMsBatch ? ~0ull : (1ull << nb) - 1;
    u64 *seen = w.words.p, *front = seen + n, *next = front + n;
    int32_t *lev = LEVELS ? w.lev.p : nullptr;
    const unsigned vgrid = grid_for((uint64_t)n, kMsBlock, kMsGrid);
    GX_HIP_TRY(hipMemsetAsync(w.words.p, 0, (size_t)n * 3 * sizeof(u64), s));
    GX_HIP_TRY(hipMemsetAsync(w.part.p, 0, w.part.n * sizeof(u64), s));
    GX_HIP_TRY(hipMemsetAsync(w.counters.p, 0, w.counters.n * sizeof(u64), s));
    if (LEVELS) GX_HIP_TRY(hipMemsetAsync(lev, 0xff, (size_t)nb * n * sizeof(int32_t), s));
    hipLaunchKernelGGL(k_msbfs_seed, dim3(1), dim3(kMsBatch), 0, s, w.src.p, nb, g->A.rp.p, seen, front, lev, n,
                       w.counters.p);
    GX_TRY(check_launch("k_msbfs_seed"));
    // the frontier counters only grow; the host keeps the last totals (no clearing per level)
    u64 *h_cnt = static_cast<u64 *>(ctx->staging[0]);
    u64 tot_v = 0, tot_e = 0, fv = 0, fe = 0;
    auto read_counts = [&]() -> int {
        GX_HIP_TRY(hipMemcpyAsync(h_cnt, w.counters.p, w.counters.n * sizeof(u64), hipMemcpyDeviceToHost, s));
        GX_HIP_TRY(hipStreamSynchronize(s));
        u64 v = 0, e = 0;
        for (int i = 0; i < kMsShards; i++) {
            v += h_cnt[i * kMsShardWords];
            e += h_cnt[i * kMsShardWords + 1];
        }
        fv = v - tot_v;
        fe = e - tot_e;
        tot_v = v;
        tot_e = e;
        return GX_SUCCESS;
    };
    GX_TRY(read_counts());
    bool next_clean = true;   // next is all zero (what push accumulates into)
    for (int64_t d = 0; fv > 0; d++) {
        if (d > n) return fail(GX_PANIC, "gx_msbfs: level loop did not end");
        const int32_t d1 = (int32_t)(d + 1);
        const bool push = w.dir == 1 || (w.dir == 0 && fe <= g->nnz / w.alpha);
        if (push) {
            {
                KTimer kt(ctx, "msbfs_push", s);
                if (!next_clean) GX_HIP_TRY(hipMemsetAsync(next, 0, (size_t)n * sizeof(u64), s));
                next_clean = true;
                uint32_t *qcount = w.tcount.p + 2;
                GX_HIP_TRY(hipMemsetAsync(qcount, 0, sizeof(uint32_t), s));
                hipLaunchKernelGGL(k_msbfs_list, dim3(vgrid), dim3(kMsBlock), 0, s, g->A.rp.p, front, n, w.queue.p,
                                   qcount);
                const uint64_t items = fv + fe / kMsChunk;
                hipLaunchKernelGGL(k_msbfs_push, dim3(grid_for(items * kWave, kMsBlock, kMsGrid)), dim3(kMsBlock), 0, s,
                                   g->A.rp.p, g->A.ci.p, w.queue.p, qcount, seen, front, next);
                GX_TRY(check_launch("k_msbfs_push"));
            }
            KTimer kt(ctx, "msbfs_commit", s);
            hipLaunchKernelGGL(k_msbfs_commit<LEVELS>, dim3(vgrid), dim3(kMsBlock), 0, s, g->A.rp.p, seen, front, next,
                               n, d1, lev, w.part.p, w.counters.p);
            GX_TRY(check_launch("k_msbfs_commit"));
        } else {
            KTimer kt(ctx, "msbfs_pull", s);
            hipLaunchKernelGGL(k_msbfs_pull<LEVELS>, dim3(vgrid), dim3(kMsBlock), 0, s, in.rp.p, in.ci.p, g->A.rp.p,
                               seen, front, next, n, live, d1, kMsShort, lev, w.part.p, w.counters.p);
            if (w.n_wave)
                hipLaunchKernelGGL(k_msbfs_pull_wave<LEVELS>, dim3(grid_for((uint64_t)w.n_wave * kWave, kMsBlock, kMsGrid)),
                                   dim3(kMsBlock), 0, s, in.rp.p, in.ci.p, g->A.rp.p, w.tiers.p, w.n_wave, seen, front,
                                   next, n, live, d1, lev, w.part.p, w.counters.p);
            if (w.n_block)
                hipLaunchKernelGGL(k_msbfs_pull_block<LEVELS>, dim3(std::min(w.n_block, kMsGrid)), dim3(kMsBlock), 0, s,
                                   in.rp.p, in.ci.p, g->A.rp.p, w.tiers.p + (n - (int64_t)w.n_block), w.n_block, seen,
                                   front, next, n, live, d1, lev, w.part.p, w.counters.p);
            GX_TRY(check_launch("k_msbfs_pull"));
            std::swap(front, next);   // next now holds the last frontier
            next_clean = false;
        }
        GX_TRY(read_counts());
    }
    KTimer kt(ctx, "msbfs_out", s);
    hipLaunchKernelGGL(k_msbfs_out, dim3(nb), dim3(kMsBlock), 0, s, w.part.p, kMsGrid, w.stats.p);
    return check_launch("k_msbfs_out");
}

}  // namespace
}  // namespace gx

using namespace gx;

extern "C" int gx_msbfs(gx_graph *g, const uint64_t *sources, uint64_t ns, int64_t *level, uint64_t *stats) {
    if (!g || (ns > 0 && !sources) || (!level && !stats)) return fail(GX_NULL_POINTER, "gx_msbfs: null argument");
    for (uint64_t k = 0; k < ns; k++)
        if (sources[k] >= g->n) return fail(GX_INVALID_INDEX, "gx_msbfs: source out of range");
    if (ns == 0) return GX_SUCCESS;
    gx_ctx *ctx = g->ctx;
    GX_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int64_t n = (int64_t)g->n;
    MsWork w;
    if (const char *ae = std::getenv("GX_MSBFS_ALPHA")) w.alpha = (u64)std::max<long long>(1, std::atoll(ae));
    if (const char *de = std::getenv("GX_MSBFS_DIR"))
        w.dir = std::strcmp(de, "push") == 0 ? 1 : (std::strcmp(de, "pull") == 0 ? 2 : 0);
    // pull reads in-edges from the first level it runs; g itself, never the hub-first copy, and
    // none of g's BFS bookkeeping (bfs_calls, hub_bfs_calls, bfs_steps_hint) is touched
    if (g->directed) GX_TRY(ensure_transpose(g));
    const DevCSR &in = g->directed ? g->AT : g->A;
    const int nb_max = (int)std::min<uint64_t>(ns, kMsBatch);
    GX_TRY(w.words.alloc((size_t)n * 3));
    if (level) GX_TRY(w.lev.alloc((size_t)nb_max * n));
    GX_TRY(w.tiers.alloc(n));
    GX_TRY(w.tcount.alloc(3));
    GX_TRY(w.queue.alloc((size_t)n + g->nnz / kMsChunk + 64));   // sum over vertices of ceil(deg / kMsChunk)
    GX_TRY(w.part.alloc((size_t)kMsGrid * 3 * kWave));
    GX_TRY(w.counters.alloc((size_t)kMsShards * kMsShardWords));
    GX_TRY(w.stats.alloc(3 * kMsBatch));
    GX_TRY(w.src.alloc(kMsBatch));
    double total_ms = 0.0;
    for (uint64_t off = 0; off < ns; off += kMsBatch) {
        const int nb = (int)std::min<uint64_t>(ns - off, kMsBatch);
        GX_HIP_TRY(hipMemcpyAsync(w.src.p, sources + off, (size_t)nb * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        GX_TRY(device_begin(ctx));
        if (off == 0) {   // the long in-rows, listed once per call
            uint32_t h_t[2] = {0, 0};
            GX_HIP_TRY(hipMemsetAsync(w.tcount.p, 0, 3 * sizeof(uint32_t), s));
            hipLaunchKernelGGL(k_msbfs_tiers, dim3((unsigned)std::min<int64_t>((n + kMsTile - 1) / kMsTile, kMsGrid)),
                               dim3(kMsBlock), 0, s, in.rp.p, n, kMsShort, kMsLong, w.tiers.p, w.tcount.p);
            GX_TRY(check_launch("k_msbfs_tiers"));
            GX_HIP_TRY(hipMemcpyAsync(h_t, w.tcount.p, sizeof(h_t), hipMemcpyDeviceToHost, s));
            GX_HIP_TRY(hipStreamSynchronize(s));
            if ((uint64_t)h_t[0] + h_t[1] > (uint64_t)n) return fail(GX_PANIC, "gx_msbfs: tier lists exceed n");
            w.n_wave = h_t[0];
            w.n_block = h_t[1];
        }
        GX_TRY(level ? msbfs_batch<true>(g, w, nb) : msbfs_batch<false>(g, w, nb));
        GX_TRY(device_end(ctx));
        total_ms += ctx->last_device_ms;
        // the downloads stay outside the brackets, as in every other call
        if (level)
            for (int k = 0; k < nb; k++)
                GX_TRY(download(ctx, level + (off + k) * g->n, w.lev.p + (size_t)k * n, g->n, Xfer::Levels));
        if (stats) GX_TRY(download(ctx, stats + 3 * off, w.stats.p, 3 * (uint64_t)nb, Xfer::Raw64));
    }
    ctx->last_device_ms = total_ms;
    return GX_SUCCESS;
}

GX_MODULE_WARMER(msbfs)

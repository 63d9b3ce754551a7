// gx_core.hip -- k-core and core numbers (the roles of LAGraph_KCore and LAGraph_KCore_All).
//
// Peeling, with all state on the device.  The graph stays where it is; a vertex has a degree word
// and a core word:
//   prep    : once per graph (gx_graph::core): deg0[v] = row v's entries minus its diagonal ones.
//   state   : deg[v] (int32, starts as deg0), core[v] (uint32: kAlive, else the number the vertex
//             left with), two frontier lists of n words, one CoreState record.
//   seed    : k_core_seed sweeps the vertices: the alive ones with deg < k leave (core = k - 1) and
//             are compacted into the frontier, one atomic per wave; the same sweep reduces the
//             smallest degree of those that stay, so that gx_core_all jumps over empty levels
//             (k = that degree + 1).
//   expand  : k_core_expand, one synchronous round: for every frontier vertex u and every stored
//             off-diagonal (u, w) with w still alive, old = atomicSub(&deg[w], 1); the one thread
//             that sees old == k marks w as left and appends it to the next frontier.  A vertex that
//             left earlier, or leaves in this round, already has deg < k: it can never be seen at
//             k again, so it is appended exactly once whatever the order.  Whether a decrement of a
//             vertex that is leaving is skipped or not changes only a word nobody reads again.
//             A frontier row of at most GX_CORE_SHORT entries is one thread's, of at most
//             GX_CORE_LONG one wave's, a longer one the workgroup's, all in the one launch.
//   plan    : k_core_plan, thread 0 of one workgroup: takes the round just expanded into the
//             counters (rounds that removed a vertex, alive), swaps the frontiers, and when the
//             level is exhausted ends the call (gx_kcore) or moves k on and asks for a seed sweep
//             (gx_core_all).  A kernel queued past the end reads `done` and returns.
//   solo    : while the frontier holds at most GX_CORE_SOLO vertices the plan's workgroup runs
//             round after round by itself, on the same lists and words, ordered by __syncthreads()
//             alone, until the frontier is empty, outgrows the threshold or kCoreSoloRounds rounds
//             are done.  Every round it runs removes a vertex, and it is one round of the same
//             synchronous peel: the round count and every output are the same with it on or off.
//   driver  : steps of (plan, seed, expand) queued in batches of GX_CORE_BATCH with no host read
//             between them; the host reads the state record one batch late (gx_bfs.hip bfs_levels).
// No kernel waits for another workgroup; every device loop is bounded by a count known at launch.
// Integers only; a result is the same bit for bit on every run.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "gx_device.h"
#include "gx_rows.h"

namespace gx {
namespace {

using u64 = unsigned long long;

constexpr int kCoreBlock = kRowsBlock;   // walk_rows (gx_rows.h)
constexpr int kCoreWaves = kCoreBlock / kWave;
constexpr unsigned kCoreSweepGrid = 1024;   // cap of the vertex-sweeping grids (4 workgroups per CU)
constexpr unsigned kCoreExpandGrid = 512;   // cap of the expand grid: a workgroup that finds no
                                            // frontier chunk of its own returns at once
constexpr uint32_t kAlive = 0xffffffffu;    // never a core number: k - 1 <= 2^32 - 2
// A frontier row of at most kCoreShort entries is one thread's, at most kCoreLong one wave's, a longer
// one the workgroup's (GX_CORE_SHORT / GX_CORE_LONG; mirrored in algorithms.py).  SYN-g500-22,
// gx_core_all / gx_kcore at k = 481: 8:512 181.1 / 3.59 ms, 16:1 024 200.0 / 4.44, 32:2 048 198.9 / 4.51,
// 64:4 096 215.5 / 4.67 (profiles/kcore_knobs_ab.txt); smaller than 8:512 was not measured.
constexpr int kCoreShort = 8;
constexpr int kCoreLong = 512;
// the plan's workgroup runs the rounds whose frontier has at most this many vertices (GX_CORE_SOLO,
// 0 = never).  A 4 096-vertex path at k = 2 (2 048 rounds of two vertices): 7.65 ms with any value
// from 16 up, 23.2 ms at 0.  SYN-g500-22's gx_core_all: 202.3 ms at 0, 201.1 / 200.8 / 199.9 at 16 / 64 /
// 256, 259.0 at 1 024, 413.4 at 4 096: one workgroup on many long rows (same file).
constexpr int kCoreSolo = 256;
// steps queued between two host reads of the state (GX_CORE_BATCH).  gx_core_all is flat from 4 to 64
// (200.0-200.3 ms); gx_kcore at k = 481, which ends after 4 rounds and pays for the steps queued past
// the end, takes 4.33 / 4.37 / 4.45 / 4.59 / 4.88 ms at 4 / 8 / 16 / 32 / 64 (same file).
constexpr int kCoreBatch = 8;
// rounds one solo launch runs at most: bounds the launch.  Not measured.
constexpr int kCoreSoloRounds = 256;

static_assert(kCoreWaves == 4, "the LDS reductions below take four waves");

// The one record the kernels steer by and the host reads.
struct CoreState {
    uint32_t k;         // the level being pruned toward: vertices with deg < k leave
    uint32_t all;       // gx_core_all: move k on when a level is exhausted
    uint32_t done;
    uint32_t started;
    uint32_t seed;      // this step's sweep fills list[fi] (it is empty)
    uint32_t fi;        // the frontier to expand is list[fi], cnt[fi] long; the next one list[fi ^ 1]
    uint32_t cnt[2];
    uint32_t min_deg;   // the sweep's smallest degree among the vertices that stay
    uint32_t top;       // the largest core number given so far
    u64 alive;
    u64 rounds;         // rounds that removed at least one vertex
    u64 steps;          // plan launches that had work
};

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = min(x, (uint32_t)__shfl_xor((int)x, off, kWave));
    return x;
}

// prep: a diagonal entry counts toward no degree
struct DiagF {
    int32_t *deg0;
    __device__ __forceinline__ void visit(uint32_t u, uint32_t w, bool on) const {
        if (on && w == u) atomicSub(&deg0[u], 1);
    }
};

// one round's work on an entry (u, w)
struct ExpandF {
    uint32_t *core;
    int32_t *deg;
    uint32_t k;
    uint32_t *next, *ncnt;
    __device__ __forceinline__ void visit(uint32_t u, uint32_t w, bool on) const {
        bool app = false;
        if (on && w != u && core[w] == kAlive) {
            const int32_t old = atomicSub(&deg[w], 1);
            if ((uint32_t)old == k) {   // this decrement took w below k: nobody else sees k there
                core[w] = k - 1;
                app = true;
            }
        }
        wave_append(app, w, next, ncnt);
    }
};

__global__ __launch_bounds__(kCoreBlock) void k_core_len(const int64_t *__restrict__ rp, int64_t n,
                                                         int32_t *__restrict__ deg0) {
    for (int64_t v = (int64_t)blockIdx.x * kCoreBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kCoreBlock)
        deg0[v] = (int32_t)(rp[v + 1] - rp[v]);
}

__global__ __launch_bounds__(kCoreBlock) void k_core_diag(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                          uint32_t n, int short_len, int long_len, int32_t *deg0) {
    DiagF f{deg0};
    walk_rows(rp, ci, nullptr, n, short_len, long_len, blockIdx.x, gridDim.x, f);
}

// ---- a call's state ----

__global__ __launch_bounds__(kCoreBlock) void k_core_init(int64_t n, const int32_t *__restrict__ deg0,
                                                          int32_t *__restrict__ deg, uint32_t *__restrict__ core) {
    for (int64_t v = (int64_t)blockIdx.x * kCoreBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kCoreBlock) {
        deg[v] = deg0[v];
        core[v] = kAlive;
    }
}

// a frontier's count as the other waves' atomics left it (not a line this thread read earlier)
__device__ __forceinline__ uint32_t core_count(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// What thread 0 does between two rounds: takes the round just expanded (list[fi]) into the counters
// and decides what comes next.
__device__ void core_advance(CoreState *st) {
    if (st->done) return;
    if (!st->started) {
        st->started = 1;
        st->seed = 1;
        st->min_deg = 0xffffffffu;
        return;
    }
    st->steps++;
    const uint32_t removed = core_count(&st->cnt[st->fi]);
    if (removed) {
        st->rounds++;
        st->alive -= removed;
        st->top = st->k - 1;   // k only grows
    } else if (st->seed) {     // the sweep found nobody below k
        if (!st->all || st->min_deg == 0xffffffffu) {
            st->done = 1;
            st->seed = 0;
            return;
        }
        st->k = st->min_deg + 1;   // the levels up to the smallest alive degree are empty
        st->min_deg = 0xffffffffu;
        return;                    // seed stays set; list[fi] is empty
    }
    st->cnt[st->fi] = 0;
    st->fi ^= 1;
    st->seed = 0;
    if (core_count(&st->cnt[st->fi])) return;   // the next round of this level
    if (!st->all || st->alive == 0) {
        st->done = 1;
        return;
    }
    st->k++;   // every alive vertex has deg >= k here
    st->seed = 1;
    st->min_deg = 0xffffffffu;
}

// The step's plan, and the solo rounds (see the head of the file).  One workgroup.
__global__ __launch_bounds__(kCoreBlock) void k_core_plan(CoreState *st, const int64_t *__restrict__ rp,
                                                          const int32_t *__restrict__ ci, uint32_t *core, int32_t *deg,
                                                          uint32_t *list0, uint32_t *list1, uint32_t solo,
                                                          int short_len, int long_len) {
    __shared__ uint32_t go, s_fi, s_cnt, s_k;
    for (int r = 0; r <= kCoreSoloRounds; r++) {
        if (threadIdx.x == 0) {
            core_advance(st);
            const uint32_t c = core_count(&st->cnt[st->fi]);
            go = !st->done && !st->seed && c > 0 && c <= solo && r < kCoreSoloRounds;
            s_fi = st->fi;
            s_cnt = c;
            s_k = st->k;
        }
        __syncthreads();
        if (!go) return;
        const uint32_t fi = s_fi;
        ExpandF f{core, deg, s_k, fi ? list0 : list1, &st->cnt[fi ^ 1]};
        walk_rows(rp, ci, fi ? list1 : list0, s_cnt, short_len, long_len, 0, 1, f);
        __syncthreads();   // the round is complete before thread 0 reads its count
    }
}

// The alive vertices below k leave and become the frontier; the smallest degree of the others.
__global__ __launch_bounds__(kCoreBlock) void k_core_seed(CoreState *st, int64_t n, uint32_t *__restrict__ core,
                                                          const int32_t *__restrict__ deg, uint32_t *list0,
                                                          uint32_t *list1) {
    if (st->done || !st->seed) return;
    const uint32_t k = st->k, fi = st->fi;
    uint32_t *list = fi ? list1 : list0, *cnt = &st->cnt[fi];
    uint32_t mn = 0xffffffffu;
    for (int64_t v0 = (int64_t)blockIdx.x * kCoreBlock; v0 < n; v0 += (int64_t)gridDim.x * kCoreBlock) {
        const int64_t v = v0 + threadIdx.x;
        bool app = false;
        if (v < n && core[v] == kAlive) {
            const uint32_t d = (uint32_t)deg[v];
            if (d < k) {
                core[v] = k - 1;
                app = true;
            } else {
                mn = min(mn, d);
            }
        }
        wave_append(app, (uint32_t)v, list, cnt);
    }
    mn = wave_min_u32(mn);
    if ((threadIdx.x & (kWave - 1)) == 0 && mn < __hip_atomic_load(&st->min_deg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMin(&st->min_deg, mn);
}

__global__ __launch_bounds__(kCoreBlock) void k_core_expand(CoreState *st, const int64_t *__restrict__ rp,
                                                            const int32_t *__restrict__ ci, uint32_t *core, int32_t *deg,
                                                            uint32_t *list0, uint32_t *list1, int short_len,
                                                            int long_len) {
    if (st->done) return;
    const uint32_t fi = st->fi, count = st->cnt[fi];
    if ((u64)blockIdx.x * kCoreBlock >= count) return;
    ExpandF f{core, deg, st->k, fi ? list0 : list1, &st->cnt[fi ^ 1]};
    walk_rows(rp, ci, fi ? list1 : list0, count, short_len, long_len, blockIdx.x, gridDim.x, f);
}

// gx_kcore's result in place: deg[v] stays for an alive vertex and becomes -1 for the others; the
// sum of the alive degrees = 2 x the edges of the k-core.
__global__ __launch_bounds__(kCoreBlock) void k_core_finish(int64_t n, const uint32_t *__restrict__ core,
                                                            int32_t *__restrict__ deg, u64 *total) {
    u64 c = 0;
    for (int64_t v = (int64_t)blockIdx.x * kCoreBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kCoreBlock) {
        if (core[v] == kAlive) c += (u64)deg[v];
        else deg[v] = -1;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && c) atomicAdd(total, c);
}

// What a graph keeps between calls (gx_graph::core).
struct CoreCache {
    DBuf<int32_t> deg0, deg;
    DBuf<uint32_t> core, list0, list1;
    DBuf<CoreState> st;
    DBuf<u64> total;
    hipEvent_t ev = nullptr;   // the host's late read of the state
    ~CoreCache() {
        if (ev) (void)hipEventDestroy(ev);
    }
};

struct CoreKnobs {
    int short_len = kCoreShort, long_len = kCoreLong, solo = kCoreSolo, batch = kCoreBatch;
    bool verbose = false;
};

// The only place that reads a knob, once per call.
CoreKnobs core_knobs() {
    CoreKnobs k;
    if (const char *e = std::getenv("GX_CORE_SHORT")) k.short_len = std::max(1, std::atoi(e));
    if (const char *e = std::getenv("GX_CORE_LONG")) k.long_len = std::atoi(e);
    k.long_len = std::max(k.long_len, k.short_len);
    if (const char *e = std::getenv("GX_CORE_SOLO")) k.solo = std::max(0, std::atoi(e));
    if (const char *e = std::getenv("GX_CORE_BATCH")) k.batch = std::min(4096, std::max(1, std::atoi(e)));
    k.verbose = std::getenv("GX_CORE_VERBOSE") != nullptr;
    return k;
}

// One gx_kcore / gx_core_all call and its stages, in the order the entry points run them.
struct CoreCall {
    gx_graph *g;
    const char *fn;
    CoreKnobs kn;
    gx_ctx *ctx;
    hipStream_t s;
    int64_t n;
    CoreCache *C = nullptr;
    CoreState h{};   // the state as the host last read it

    CoreCall(gx_graph *g_, const char *fn_)
        : g(g_), fn(fn_), kn(core_knobs()), ctx(g_->ctx), s(g_->ctx->stream), n((int64_t)g_->n) {}

    unsigned sweep_grid() const { return grid_for((uint64_t)n, kCoreBlock, kCoreSweepGrid); }

    // Stage 1: the cache.  Built on the first call; nothing in it depends on a knob.
    int prep() {
        C = static_cast<CoreCache *>(g->core.get());
        if (C) return GX_SUCCESS;
        auto fresh = std::make_shared<CoreCache>();
        CoreCache &c = *fresh;
        GX_TRY(c.deg0.alloc(n));
        GX_TRY(c.deg.alloc(n));
        GX_TRY(c.core.alloc(n));
        GX_TRY(c.list0.alloc(n));
        GX_TRY(c.list1.alloc(n));
        GX_TRY(c.st.alloc(1));
        GX_TRY(c.total.alloc(1));
        GX_HIP_TRY(hipEventCreateWithFlags(&c.ev, hipEventDisableTiming));
        KTimer kt(ctx, "core_prep", s);
        hipLaunchKernelGGL(k_core_len, dim3(sweep_grid()), dim3(kCoreBlock), 0, s, g->A.rp.p, n, c.deg0.p);
        hipLaunchKernelGGL(k_core_diag, dim3(grid_for((uint64_t)n, kCoreBlock, 8192)), dim3(kCoreBlock), 0, s, g->A.rp.p,
                           g->A.ci.p, (uint32_t)n, kn.short_len, kn.long_len, c.deg0.p);
        GX_TRY(check_launch("k_core_diag"));
        g->core = fresh;
        C = fresh.get();
        return GX_SUCCESS;
    }

    // Stage 2: every vertex alive with its whole degree; pruning toward k (gx_core_all: from 1 up).
    int start(uint32_t k, bool all) {
        h = CoreState{};
        h.k = k;
        h.all = all;
        h.alive = (u64)n;
        GX_HIP_TRY(hipMemcpyAsync(C->st.p, &h, sizeof(h), hipMemcpyHostToDevice, s));
        KTimer kt(ctx, "core_init", s);
        hipLaunchKernelGGL(k_core_init, dim3(sweep_grid()), dim3(kCoreBlock), 0, s, n, C->deg0.p, C->deg.p, C->core.p);
        return check_launch("k_core_init");
    }

    // `steps` steps of plan (with its solo rounds), seed and expand; past the end they return at once.
    int enqueue(int steps) {
        const unsigned egrid = grid_for((uint64_t)n, kCoreBlock, kCoreExpandGrid);
        for (int i = 0; i < steps; i++) {
            {
                KTimer kt(ctx, "core_plan", s);
                hipLaunchKernelGGL(k_core_plan, dim3(1), dim3(kCoreBlock), 0, s, C->st.p, g->A.rp.p, g->A.ci.p, C->core.p,
                                   C->deg.p, C->list0.p, C->list1.p, (uint32_t)kn.solo, kn.short_len, kn.long_len);
            }
            {
                KTimer kt(ctx, "core_seed", s);
                hipLaunchKernelGGL(k_core_seed, dim3(sweep_grid()), dim3(kCoreBlock), 0, s, C->st.p, n, C->core.p, C->deg.p,
                                   C->list0.p, C->list1.p);
            }
            KTimer kt(ctx, "core_expand", s);
            hipLaunchKernelGGL(k_core_expand, dim3(egrid), dim3(kCoreBlock), 0, s, C->st.p, g->A.rp.p, g->A.ci.p, C->core.p,
                               C->deg.p, C->list0.p, C->list1.p, kn.short_len, kn.long_len);
        }
        return check_launch("k_core_expand");
    }

    // Stage 3: batches of steps until the state says done, read one batch late.
    int peel() {
        CoreState *hs = static_cast<CoreState *>(ctx->staging[0]);
        // every step but an empty sweep removes a vertex, and an empty sweep is followed by a full one
        const u64 limit = 2 * (u64)n + 4 + 2 * (u64)kn.batch;
        u64 queued = (u64)kn.batch;
        GX_TRY(enqueue(kn.batch));
        for (;;) {
            GX_HIP_TRY(hipMemcpyAsync(hs, C->st.p, sizeof(CoreState), hipMemcpyDeviceToHost, s));
            GX_HIP_TRY(hipEventRecord(C->ev, s));
            GX_TRY(enqueue(kn.batch));
            queued += (u64)kn.batch;
            GX_HIP_TRY(hipEventSynchronize(C->ev));
            h = *hs;
            if (kn.verbose)
                std::fprintf(stderr, "%s: k %u rounds %llu alive %llu steps %llu done %u\n", fn, h.k, h.rounds, h.alive,
                             h.steps, h.done);
            if (h.done) return GX_SUCCESS;
            if (queued > limit) return fail(GX_PANIC, std::string(fn) + ": the peel did not end");
        }
    }

    // Stage 4 (gx_kcore): -1 for the vertices that left, and the edges of what is left.
    int finish(uint64_t *edges) {
        u64 *ht = static_cast<u64 *>(ctx->staging[0]);
        GX_HIP_TRY(hipMemsetAsync(C->total.p, 0, sizeof(u64), s));
        {
            KTimer kt(ctx, "core_finish", s);
            hipLaunchKernelGGL(k_core_finish, dim3(sweep_grid()), dim3(kCoreBlock), 0, s, n, C->core.p, C->deg.p,
                               C->total.p);
            GX_TRY(check_launch("k_core_finish"));
        }
        GX_HIP_TRY(hipMemcpyAsync(ht, C->total.p, sizeof(u64), hipMemcpyDeviceToHost, s));
        GX_HIP_TRY(hipStreamSynchronize(s));
        *edges = (uint64_t)(ht[0] / 2);
        return GX_SUCCESS;
    }
};

// The checks both entry points share; GX_SUCCESS with *empty set: no vertex, nothing to compute.
int core_enter(gx_graph *g, const char *fn, bool *empty) {
    if (g->directed) return fail(GX_INVALID_VALUE, std::string(fn) + ": the graph is directed");
    *empty = g->n == 0;
    return GX_SUCCESS;
}

}  // namespace
}  // namespace gx

using namespace gx;

extern "C" int gx_kcore(gx_graph *g, uint32_t k, int64_t *degree, uint64_t *stats) {
    if (!g || (!degree && !stats)) return fail(GX_NULL_POINTER, "gx_kcore: null argument");
    bool empty = false;
    GX_TRY(core_enter(g, "gx_kcore", &empty));
    if (empty) {
        if (stats) stats[0] = stats[1] = stats[2] = 0;
        return GX_SUCCESS;
    }
    gx_ctx *ctx = g->ctx;
    GX_HIP_TRY(hipSetDevice(ctx->device));
    CoreCall c(g, "gx_kcore");
    GX_TRY(device_begin(ctx));
    GX_TRY(c.prep());
    GX_TRY(c.start(k, false));
    if (k > 0) GX_TRY(c.peel());   // k == 0 keeps every vertex
    uint64_t edges = 0;
    GX_TRY(c.finish(&edges));
    GX_TRY(device_end(ctx));
    if (degree) GX_TRY(download(ctx, degree, c.C->deg.p, (uint64_t)c.n, Xfer::Sign32));
    if (stats) {
        stats[0] = (uint64_t)c.h.alive;
        stats[1] = edges;
        stats[2] = (uint64_t)c.h.rounds;
    }
    return GX_SUCCESS;
}

extern "C" int gx_core_all(gx_graph *g, int64_t *core, uint64_t *kmax) {
    if (!g || (!core && !kmax)) return fail(GX_NULL_POINTER, "gx_core_all: null argument");
    bool empty = false;
    GX_TRY(core_enter(g, "gx_core_all", &empty));
    if (empty) {
        if (kmax) *kmax = 0;
        return GX_SUCCESS;
    }
    gx_ctx *ctx = g->ctx;
    GX_HIP_TRY(hipSetDevice(ctx->device));
    CoreCall c(g, "gx_core_all");
    GX_TRY(device_begin(ctx));
    GX_TRY(c.prep());
    // what leaves while pruning toward k was in the (k-1)-core and is in no larger one
    GX_TRY(c.start(1, true));
    GX_TRY(c.peel());
    GX_TRY(device_end(ctx));
    if (c.h.alive != 0) return fail(GX_PANIC, "gx_core_all: vertices left alive");
    if (core) GX_TRY(download(ctx, core, c.C->core.p, (uint64_t)c.n, Xfer::Sign32));
    if (kmax) *kmax = (uint64_t)c.h.top;
    return GX_SUCCESS;
}

GX_MODULE_WARMER(core)

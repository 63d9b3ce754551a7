// gx_scc.hip -- strongly connected components of a directed graph (the role of LAGraph_scc).
//
// Trim, one pivot, then colour propagation, with all state on the device.  A is the out-edge CSR, T
// the in-edge one (g->AT; A itself when the graph is undirected).  A vertex has one label word:
//   prep    : once per graph (gx_graph::scc): din0[v] / dout0[v] = the entries of v's row in T / in A
//             minus its diagonal ones.
//   state   : lab[v] (uint32: kAlive, else the final label = the smallest id of v's component),
//             din[v] / dout[v] (int32: v's alive in- and out-neighbours, diagonal entries not counted),
//             aux[v] (uint32: the pivot's reach bits, then the colour, then the component sizes), two
//             frontier lists and one list of the alive vertices (n words each), one SccState record.
//   stages  : SccState::stage says which one the next step runs; every stage is one synchronous round.
//     trim  : kZero (alive list rebuilt, degree words cleared; the call's first one, with every vertex
//             alive, copies din0 / dout0 and needs no count), kCount (every entry between two alive
//             vertices adds one to dout of its row and din of its column), kSeed (alive vertices with
//             din == 0 or dout == 0 take lab = v and form the frontier), kTrim (for a frontier vertex u:
//             atomicSub on din[w] over A's row and on dout[x] over T's row; the thread that sees a word
//             go from 1 to 0 claims the vertex and appends it).
//             Append once: a vertex is appended only by the thread whose atomicCAS takes lab[w] from
//             kAlive to w.  Its two words may both reach zero in one round, under two threads: both try
//             the claim, one wins.  A word reaches zero once, since it only falls and a claimed vertex
//             is skipped or, where a late decrement still lands, read by nobody again.
//     pivot : kPick (the alive vertex with the largest din x dout, the smallest id among equals, by one
//             64-bit atomicMax per wave; the product saturates at 2^32 - 1), kFwd / kBwd (level
//             traversals from it over A / T among alive vertices; atomicOr on the reach bits, the
//             thread that sets a bit appends), kMeet (wave-reduced atomicMin of the ids with both
//             bits), kLabel (they take that label).  Runs once, after the first trim.
//     colour: kCinit (alive list rebuilt, aux[v] = v), kCprop until a round changes nothing (aux[w] =
//             min(aux[w], aux[u]) over the entries between alive vertices; min only falls, so a value
//             written during the launch may be used by it and the fixed point is the same: the
//             smallest id that reaches w), kRoot (aux[r] == r: lab[r] = r, the frontier), kCbwd (over
//             T's rows: an alive x with aux[x] == lab[u] is claimed by atomicCAS on lab[x] and
//             appended; the classes are disjoint, so every root traverses at once).  Then trim again
//             on what is left, until nothing is alive.
//   plan    : k_scc_plan, thread 0 of one workgroup, takes the round just run into the counters and
//             chooses the next stage, and adds the wall clock since the last plan to the stage that ran
//             (GX_SCC_VERBOSE prints the sums).  A kernel queued past the end reads kDone and returns.
//   solo    : while the next stage's work (frontier, alive list or n) is at most GX_SCC_SOLO items the
//             plan's workgroup runs it itself, round after round, ordered by __syncthreads() alone, at
//             most kSccSoloRounds rounds a launch.  The rounds are the same rounds.
//   finish  : component sizes into aux (the pivot's component by one atomic per wave), then roots,
//             largest and singletons reduced per wave into the state record.
//   driver  : steps of (plan, step) queued in batches of GX_SCC_BATCH with no host read between them;
//             the host reads the state record one batch late (gx_core.hip, gx_bfs.hip bfs_levels).
// No kernel waits for another workgroup; every device loop is bounded by a count known at launch.
// Integers only, and every output is unique: the same bit for bit on every run and under every knob.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "gx_device.h"
#include "gx_rows.h"

namespace gx {
namespace {

using u64 = unsigned long long;

constexpr int kSccBlock = kRowsBlock;
// cap of the step grid (GX_SCC_GRID): a workgroup with no chunk of its own returns at once.  gx_scc on the
// SYN-cit stand-in / R-MAT 22 x 16, ms: 256 9.41 / 19.29, 512 9.16 / 18.84, 1 024 9.20 / 18.67, 2 048
// 9.35 / 18.65 (profiles/scc_time_mi355x.json).
constexpr unsigned kSccGrid = 512;
constexpr unsigned kSccSweepGrid = 1024;    // cap of the init / finish sweeps
constexpr uint32_t kAlive = 0xffffffffu;    // never a label: ids are below 2^31
// The row tiers (GX_SCC_SHORT / GX_SCC_LONG; mirrored in algorithms.py): gx_core.hip's pair.  Same graphs:
// 4:256 9.36 / 18.95, 8:512 9.23 / 18.84, 16:1 024 9.10 / 19.00, 32:2 048 9.20 / 18.92: flat (same file).
constexpr int kSccShort = 8;
constexpr int kSccLong = 512;
// the plan's workgroup runs the stages whose work is at most this many items (GX_SCC_SOLO, 0 = never).
// A 4 096-ring (8 190 levels): 72.57 ms at 0, 34.40 / 34.40 / 34.38 at 64 / 256 / 1 024; a 4 096-path (2 048 trim
// rounds): 19.93 at 0, 13.11 / 13.11 / 13.11; the two graphs above are flat, 9.25 / 18.87 at 0 and
// 9.20 / 18.86 at 256 (same file).
constexpr int kSccSolo = 256;
// steps queued between two host reads of the state (GX_SCC_BATCH).  Same graphs, 2 / 4 / 8 / 16 / 32:
// 9.18 / 18.93, 9.17 / 18.91, 9.11 / 18.86, 9.15 / 18.90, 9.25 / 19.02 (same file).
constexpr int kSccBatch = 8;
// rounds one solo launch runs at most: bounds the launch.  Not measured.
constexpr int kSccSoloRounds = 256;

enum Stage : uint32_t { kZero, kCount, kSeed, kTrim, kPick, kFwd, kBwd, kMeet, kLabel, kCinit, kCprop, kRoot, kCbwd, kDone };

// The one record the kernels steer by and the host reads.
struct SccState {
    uint32_t stage, started;
    uint32_t trim, pivot_left;   // phase 1 is on; phase 2 is on and has not run yet
    uint32_t whole;              // every vertex is alive: the degree words are din0 / dout0
    uint32_t fi;                 // the frontier is list[fi], cnt[fi] long; the next one list[fi ^ 1]
    uint32_t cnt[2];
    uint32_t acnt;               // the alive list's length
    uint32_t changed;            // kCprop lowered a colour
    uint32_t removed;            // kLabel's vertices
    uint32_t pmin, plabel;       // the pivot component's smallest id; its label once given (else kAlive)
    uint32_t pivot;
    u64 key;                     // kPick: (min(din x dout, 2^32 - 1) << 32) | ~id
    u64 alive;
    u64 trim_rounds, levels, colour_rounds, back_levels, outer, steps;
    u64 ncomp, largest, singles;   // finish
    u64 tick, ticks[kDone];        // the wall clock at the last plan; the ticks every stage took, gaps included
};

// What every stage works on.
struct SccArgs {
    const int64_t *rpA, *rpT;
    const int32_t *ciA, *ciT;
    uint32_t *lab, *aux;
    int32_t *din, *dout;
    const int32_t *din0, *dout0;
    uint32_t *list0, *list1, *alist;
    uint32_t n;
    int short_len, long_len;
};

// A word as the other waves' atomics left it.  An atomic is done in L2 and leaves this CU's L1 line as
// it was, so in the solo rounds, which no kernel boundary separates, a plain load of a word that an
// earlier round's atomic changed may still see the old value; every word that an atomic updates (lab,
// aux, din, dout, the counters) is read through this.
template <class T>
__device__ __forceinline__ T fresh(const T *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = min(x, (uint32_t)__shfl_xor((int)x, off, kWave));
    return x;
}

__device__ __forceinline__ u64 wave_max_u64(u64 x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = max(x, (u64)__shfl_xor(x, off, kWave));
    return x;
}

// ---- what a stage does with an entry (u, w) of a walked row ----

// kCount: an entry between two alive vertices; u is alive (the alive list is fresh)
struct CountF {
    const uint32_t *lab;
    int32_t *din, *dout;
    __device__ __forceinline__ void visit(uint32_t u, uint32_t w, bool on) const {
        const bool hit = on && w != u && fresh(&lab[w]) == kAlive;
        if (hit) atomicAdd(&din[w], 1);
        const u64 m = __ballot(hit);
        if (!m) return;
        const int leader = __ffsll(m) - 1;
        const uint32_t u0 = (uint32_t)__shfl((int)u, leader, kWave);
        if (__all(!hit || u == u0)) {   // one row across the wave: one atomic for its word
            if ((threadIdx.x & (kWave - 1)) == leader) atomicAdd(&dout[u0], (int32_t)__popcll(m));
        } else if (hit) {
            atomicAdd(&dout[u], 1);
        }
    }
};

// kTrim: the removed u takes one from `deg` of every alive neighbour w; see "append once" at the head
struct TrimF {
    uint32_t *lab;
    int32_t *deg;
    uint32_t *next, *ncnt;
    __device__ __forceinline__ void visit(uint32_t u, uint32_t w, bool on) const {
        bool app = false;
        if (on && w != u && fresh(&lab[w]) == kAlive && atomicSub(&deg[w], 1) == 1)
            app = atomicCAS(&lab[w], kAlive, w) == kAlive;
        wave_append(app, w, next, ncnt);
    }
};

// kFwd / kBwd: the thread that sets w's bit appends it
struct ReachF {
    const uint32_t *lab;
    uint32_t *aux;
    uint32_t bit;
    uint32_t *next, *ncnt;
    __device__ __forceinline__ void visit(uint32_t, uint32_t w, bool on) const {
        bool app = false;
        if (on && fresh(&lab[w]) == kAlive && !(fresh(&aux[w]) & bit)) app = !(atomicOr(&aux[w], bit) & bit);
        wave_append(app, w, next, ncnt);
    }
};

// kCprop: u's colour flows to w
struct ColourF {
    const uint32_t *lab;
    uint32_t *aux;
    uint32_t *changed;
    __device__ __forceinline__ void visit(uint32_t u, uint32_t w, bool on) const {
        if (!on || w == u || fresh(&lab[w]) != kAlive) return;
        const uint32_t c = fresh(&aux[u]);
        if (c < fresh(&aux[w]) && atomicMin(&aux[w], c) > c && fresh(changed) == 0)
            __hip_atomic_store(changed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// kCbwd: u carries its root's label; an alive in-neighbour of the same colour joins it
struct BackF {
    uint32_t *lab;
    const uint32_t *aux;
    uint32_t *next, *ncnt;
    __device__ __forceinline__ void visit(uint32_t u, uint32_t x, bool on) const {
        bool app = false;
        if (on && fresh(&lab[x]) == kAlive) {
            const uint32_t c = fresh(&lab[u]);
            if (fresh(&aux[x]) == c) app = atomicCAS(&lab[x], kAlive, c) == kAlive;
        }
        wave_append(app, x, next, ncnt);
    }
};

// What a stage reads of the state: taken once, by every workgroup the same.
struct Round {
    uint32_t stage, fi, cnt, acnt, pmin, whole;
};

__device__ __forceinline__ uint32_t work_of(const Round &r, uint32_t n) {
    switch (r.stage) {
        case kZero: case kCinit: return n;
        case kTrim: case kFwd: case kBwd: case kCbwd: return r.cnt;
        case kDone: return 0;
        default: return r.acnt;
    }
}

// One round of stage r.stage on the chunks first, first + stride, ...  Whole workgroups call it.
__device__ __forceinline__ void scc_round(const SccArgs &a, SccState *st, const Round &r, unsigned first,
                                          unsigned stride) {
    uint32_t *cur = r.fi ? a.list1 : a.list0, *next = r.fi ? a.list0 : a.list1;
    uint32_t *ccnt = &st->cnt[r.fi], *ncnt = &st->cnt[r.fi ^ 1];
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t work = work_of(r, a.n);
    switch (r.stage) {
        case kCount: {
            CountF f{a.lab, a.din, a.dout};
            walk_rows(a.rpA, a.ciA, a.alist, r.acnt, a.short_len, a.long_len, first, stride, f);
            return;
        }
        case kTrim: {
            TrimF fo{a.lab, a.din, next, ncnt}, fin{a.lab, a.dout, next, ncnt};
            walk_rows(a.rpA, a.ciA, cur, r.cnt, a.short_len, a.long_len, first, stride, fo);
            walk_rows(a.rpT, a.ciT, cur, r.cnt, a.short_len, a.long_len, first, stride, fin);
            return;
        }
        case kFwd: case kBwd: {
            const bool fwd = r.stage == kFwd;
            ReachF f{a.lab, a.aux, fwd ? 1u : 2u, next, ncnt};
            walk_rows(fwd ? a.rpA : a.rpT, fwd ? a.ciA : a.ciT, cur, r.cnt, a.short_len, a.long_len, first, stride, f);
            return;
        }
        case kCprop: {
            ColourF f{a.lab, a.aux, &st->changed};
            walk_rows(a.rpA, a.ciA, a.alist, r.acnt, a.short_len, a.long_len, first, stride, f);
            return;
        }
        case kCbwd: {
            BackF f{a.lab, a.aux, next, ncnt};
            walk_rows(a.rpT, a.ciT, cur, r.cnt, a.short_len, a.long_len, first, stride, f);
            return;
        }
        default: break;
    }
    // the vertex sweeps: item x of 0 .. work - 1 is vertex x (kZero, kCinit) or alist[x]
    u64 key = 0;
    uint32_t mn = kAlive, gone = 0;
    for (u64 base = (u64)first * kSccBlock; base < work; base += (u64)stride * kSccBlock) {
        const u64 x = base + threadIdx.x;
        const bool in = x < work;
        switch (r.stage) {
            case kZero: case kCinit: {
                const bool live = in && fresh(&a.lab[x]) == kAlive;
                if (live) {
                    if (r.stage == kCinit) {
                        a.aux[x] = (uint32_t)x;
                    } else {
                        a.din[x] = r.whole ? a.din0[x] : 0;
                        a.dout[x] = r.whole ? a.dout0[x] : 0;
                    }
                }
                wave_append(live, (uint32_t)x, a.alist, &st->acnt);
                break;
            }
            case kSeed: {
                const uint32_t v = in ? a.alist[x] : 0u;
                const bool app = in && (fresh(&a.din[v]) == 0 || fresh(&a.dout[v]) == 0);
                if (app) a.lab[v] = v;
                wave_append(app, v, cur, ccnt);
                break;
            }
            case kPick: {
                const uint32_t v = in ? a.alist[x] : 0u;
                if (in && fresh(&a.lab[v]) == kAlive) {
                    a.aux[v] = 0;
                    const u64 prod = (u64)(uint32_t)fresh(&a.din[v]) * (u64)(uint32_t)fresh(&a.dout[v]);
                    key = max(key, (min(prod, (u64)0xffffffffu) << 32) | (u64)(0xffffffffu - v));
                }
                break;
            }
            case kMeet: case kLabel: {
                const uint32_t v = in ? a.alist[x] : 0u;
                const bool both = in && fresh(&a.lab[v]) == kAlive && fresh(&a.aux[v]) == 3u;
                if (r.stage == kMeet) {
                    if (both) mn = min(mn, v);
                } else {
                    if (both) a.lab[v] = r.pmin;
                    gone += (uint32_t)__popcll(__ballot(both));
                }
                break;
            }
            case kRoot: {
                const uint32_t v = in ? a.alist[x] : 0u;
                const bool app = in && fresh(&a.aux[v]) == v;
                if (app) a.lab[v] = v;
                wave_append(app, v, cur, ccnt);
                break;
            }
            default: break;
        }
    }
    if (r.stage == kPick) {
        key = wave_max_u64(key);
        if (lane == 0 && key > fresh(&st->key)) atomicMax(&st->key, key);
    } else if (r.stage == kMeet) {
        mn = wave_min_u32(mn);
        if (lane == 0 && mn < fresh(&st->pmin)) atomicMin(&st->pmin, mn);
    } else if (r.stage == kLabel) {
        if (lane == 0 && gone) atomicAdd(&st->removed, gone);
    }
}

// ---- the plan ----

__device__ __forceinline__ void scc_end_or(SccState *st, uint32_t next) {
    if (st->alive == 0) {
        st->stage = kDone;
        return;
    }
    st->stage = next;
    if (next == kZero || next == kCinit) st->acnt = 0;
}

// the stage after a component was taken out: trim again, or straight to colours
__device__ __forceinline__ void scc_next_outer(SccState *st) { scc_end_or(st, st->trim ? kZero : kCinit); }

// the frontier list[fi] is spent: the next one becomes the frontier; its length
__device__ __forceinline__ uint32_t scc_swap(SccState *st) {
    st->cnt[st->fi] = 0;
    st->fi ^= 1;
    return fresh(&st->cnt[st->fi]);
}

__device__ __forceinline__ void scc_from_pivot(SccState *st, const SccArgs &a, uint32_t bit, uint32_t stage) {
    (st->fi ? a.list1 : a.list0)[0] = st->pivot;
    st->cnt[st->fi] = 1;
    atomicOr(&a.aux[st->pivot], bit);
    st->stage = stage;
}

// What thread 0 does between two rounds: takes the round just run into the counters and chooses
// the stage of the next one.
__device__ void scc_advance(SccState *st, const SccArgs &a) {
    if (st->stage == kDone) return;
    const u64 now = wall_clock64();
    if (st->started) st->ticks[st->stage] += now - st->tick;
    st->tick = now;
    if (!st->started) {
        st->started = 1;
        scc_end_or(st, (st->trim || st->pivot_left) ? kZero : kCinit);
        return;
    }
    st->steps++;
    switch (st->stage) {
        case kZero:
            if (!st->whole) {
                st->stage = kCount;
                return;
            }
            st->whole = 0;
            [[fallthrough]];
        case kCount:   // without trim the words are the pivot's alone
            st->stage = st->trim ? kSeed : kPick;
            return;
        case kSeed: case kTrim: {
            const uint32_t c = st->stage == kSeed ? fresh(&st->cnt[st->fi]) : scc_swap(st);
            if (c) {
                st->alive -= c;
                st->trim_rounds++;
                st->stage = kTrim;
                return;
            }
            scc_end_or(st, st->pivot_left ? kPick : kCinit);
            return;
        }
        case kPick:
            st->pivot_left = 0;
            st->pivot = 0xffffffffu - (uint32_t)fresh(&st->key);
            scc_from_pivot(st, a, 1u, kFwd);
            return;
        case kFwd: case kBwd:
            if (scc_swap(st)) {
                st->levels++;
                return;
            }
            if (st->stage == kFwd) {
                scc_from_pivot(st, a, 2u, kBwd);
                return;
            }
            st->pmin = kAlive;
            st->removed = 0;
            st->stage = kMeet;
            return;
        case kMeet:
            st->pmin = fresh(&st->pmin);
            st->stage = kLabel;
            return;
        case kLabel:
            st->alive -= fresh(&st->removed);
            st->plabel = st->pmin;
            scc_next_outer(st);
            return;
        case kCinit:
            st->acnt = fresh(&st->acnt);
            st->changed = 0;
            st->outer++;
            st->stage = kCprop;
            return;
        case kCprop:
            st->colour_rounds++;
            if (fresh(&st->changed)) st->changed = 0;
            else st->stage = kRoot;
            return;
        case kRoot:
            st->alive -= fresh(&st->cnt[st->fi]);   // every class has its root: at least one
            st->stage = kCbwd;
            return;
        case kCbwd: {
            const uint32_t c = scc_swap(st);
            if (c) {
                st->alive -= c;
                st->back_levels++;
                return;
            }
            scc_next_outer(st);
            return;
        }
        default: return;
    }
}

// The step's plan, and the solo rounds (see the head of the file).  One workgroup.
__global__ __launch_bounds__(kSccBlock) void k_scc_plan(SccState *st, SccArgs a, uint32_t solo) {
    __shared__ uint32_t go;
    __shared__ Round rd;
    for (int i = 0; i <= kSccSoloRounds; i++) {
        if (threadIdx.x == 0) {
            scc_advance(st, a);
            rd = Round{st->stage, st->fi, fresh(&st->cnt[st->fi]), fresh(&st->acnt), st->pmin, st->whole};
            go = st->stage != kDone && work_of(rd, a.n) <= solo && i < kSccSoloRounds;
            __threadfence();   // the pivot's list entry and reach bit
        }
        __syncthreads();
        if (!go) return;
        const Round r = rd;
        scc_round(a, st, r, 0, 1);
        __threadfence();
        __syncthreads();   // the round is complete before thread 0 reads what it counted
    }
}

__global__ __launch_bounds__(kSccBlock) void k_scc_step(SccState *st, SccArgs a) {
    const Round r{st->stage, st->fi, st->cnt[st->fi], st->acnt, st->pmin, st->whole};
    if (r.stage == kDone || (u64)blockIdx.x * kSccBlock >= work_of(r, a.n)) return;
    scc_round(a, st, r, blockIdx.x, gridDim.x);
}

// ---- prep: the degrees of the whole graph; a diagonal entry counts toward neither ----

struct DiagF {
    int32_t *din0, *dout0;
    __device__ __forceinline__ void visit(uint32_t u, uint32_t w, bool on) const {
        if (on && w == u) {
            atomicSub(&din0[u], 1);
            atomicSub(&dout0[u], 1);
        }
    }
};

__global__ __launch_bounds__(kSccBlock) void k_scc_len(const int64_t *__restrict__ rpA, const int64_t *__restrict__ rpT,
                                                        int64_t n, int32_t *__restrict__ din0,
                                                        int32_t *__restrict__ dout0) {
    for (int64_t v = (int64_t)blockIdx.x * kSccBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kSccBlock) {
        din0[v] = (int32_t)(rpT[v + 1] - rpT[v]);
        dout0[v] = (int32_t)(rpA[v + 1] - rpA[v]);
    }
}

__global__ __launch_bounds__(kSccBlock) void k_scc_diag(SccArgs a, int32_t *din0, int32_t *dout0) {
    DiagF f{din0, dout0};
    walk_rows(a.rpA, a.ciA, nullptr, a.n, a.short_len, a.long_len, blockIdx.x, gridDim.x, f);
}

// ---- a call's start and end ----

__global__ __launch_bounds__(kSccBlock) void k_scc_init(int64_t n, uint32_t *__restrict__ lab) {
    for (int64_t v = (int64_t)blockIdx.x * kSccBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kSccBlock)
        lab[v] = kAlive;
}

// size[l] = the vertices labelled l; the pivot's component, which may hold most of them, by one
// atomic per wave
__global__ __launch_bounds__(kSccBlock) void k_scc_sizes(int64_t n, const uint32_t *__restrict__ lab,
                                                         const SccState *st, uint32_t *size) {
    const uint32_t big = st->plabel;
    uint32_t nb = 0;
    for (int64_t v0 = (int64_t)blockIdx.x * kSccBlock; v0 < n; v0 += (int64_t)gridDim.x * kSccBlock) {
        const int64_t v = v0 + threadIdx.x;
        const uint32_t l = v < n ? lab[v] : kAlive;
        if (l != kAlive && l != big) atomicAdd(&size[l], 1u);
        nb += (uint32_t)__popcll(__ballot(l != kAlive && l == big));
    }
    if ((threadIdx.x & (kWave - 1)) == 0 && nb) atomicAdd(&size[big], nb);
}

__global__ __launch_bounds__(kSccBlock) void k_scc_stats(int64_t n, const uint32_t *__restrict__ lab,
                                                         const uint32_t *__restrict__ size, SccState *st) {
    u64 roots = 0, ones = 0, mx = 0;
    for (int64_t v = (int64_t)blockIdx.x * kSccBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kSccBlock) {
        if (lab[v] != (uint32_t)v) continue;
        const uint32_t sz = size[v];
        roots++;
        ones += sz == 1u;
        mx = max(mx, (u64)sz);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        roots += __shfl_xor(roots, off, kWave);
        ones += __shfl_xor(ones, off, kWave);
    }
    mx = wave_max_u64(mx);
    if ((threadIdx.x & (kWave - 1)) == 0 && roots) {
        atomicAdd(&st->ncomp, roots);
        if (ones) atomicAdd(&st->singles, ones);
        if (mx > fresh(&st->largest)) atomicMax(&st->largest, mx);
    }
}

// What a graph keeps between calls (gx_graph::scc).
struct SccCache {
    DBuf<uint32_t> lab, aux, list0, list1, alist;
    DBuf<int32_t> din, dout, din0, dout0;
    DBuf<SccState> st;
    hipEvent_t ev = nullptr;   // the host's late read of the state
    ~SccCache() {
        if (ev) (void)hipEventDestroy(ev);
    }
};

struct SccKnobs {
    bool trim = true, pivot = true, verbose = false;
    int short_len = kSccShort, long_len = kSccLong, solo = kSccSolo, batch = kSccBatch;
    unsigned grid = kSccGrid;
};

// The only place that reads a knob, once per call.
SccKnobs scc_knobs() {
    SccKnobs k;
    if (const char *e = std::getenv("GX_SCC_TRIM")) k.trim = std::atoi(e) != 0;
    if (const char *e = std::getenv("GX_SCC_PIVOT")) k.pivot = std::atoi(e) != 0;
    if (const char *e = std::getenv("GX_SCC_SHORT")) k.short_len = std::max(1, std::atoi(e));
    if (const char *e = std::getenv("GX_SCC_LONG")) k.long_len = std::atoi(e);
    k.long_len = std::max(k.long_len, k.short_len);
    if (const char *e = std::getenv("GX_SCC_SOLO")) k.solo = std::max(0, std::atoi(e));
    if (const char *e = std::getenv("GX_SCC_BATCH")) k.batch = std::min(4096, std::max(1, std::atoi(e)));
    if (const char *e = std::getenv("GX_SCC_GRID")) k.grid = (unsigned)std::min(65536, std::max(1, std::atoi(e)));
    k.verbose = std::getenv("GX_SCC_VERBOSE") != nullptr;
    return k;
}

// One gx_scc call and its stages, in the order the entry point runs them.
struct SccCall {
    gx_graph *g;
    SccKnobs kn;
    gx_ctx *ctx;
    hipStream_t s;
    int64_t n;
    SccCache *C = nullptr;
    SccArgs a{};
    SccState h{};   // the state as the host last read it

    explicit SccCall(gx_graph *g_) : g(g_), kn(scc_knobs()), ctx(g_->ctx), s(g_->ctx->stream), n((int64_t)g_->n) {}

    unsigned sweep_grid() const { return grid_for((uint64_t)n, kSccBlock, kSccSweepGrid); }

    // Stage 1: the cache.  Built on the first call; of its contents only din0 / dout0 outlive a call,
    // and they depend on no knob.
    int prep() {
        C = static_cast<SccCache *>(g->scc.get());
        const bool build = !C;
        if (build) {
            auto made = std::make_shared<SccCache>();
            SccCache &c = *made;
            GX_TRY(c.lab.alloc(n));
            GX_TRY(c.aux.alloc(n));
            GX_TRY(c.list0.alloc(n));
            GX_TRY(c.list1.alloc(n));
            GX_TRY(c.alist.alloc(n));
            GX_TRY(c.din.alloc(n));
            GX_TRY(c.dout.alloc(n));
            GX_TRY(c.din0.alloc(n));
            GX_TRY(c.dout0.alloc(n));
            GX_TRY(c.st.alloc(1));
            GX_HIP_TRY(hipEventCreateWithFlags(&c.ev, hipEventDisableTiming));
            g->scc = made;
            C = made.get();
        }
        const DevCSR &T = g->directed ? g->AT : g->A;   // an undirected graph is its own transpose
        a = SccArgs{g->A.rp.p, T.rp.p, g->A.ci.p, T.ci.p, C->lab.p, C->aux.p, C->din.p, C->dout.p,
                    C->din0.p, C->dout0.p, C->list0.p, C->list1.p, C->alist.p, (uint32_t)n, kn.short_len, kn.long_len};
        if (build) {
            KTimer kt(ctx, "scc_prep", s);
            hipLaunchKernelGGL(k_scc_len, dim3(sweep_grid()), dim3(kSccBlock), 0, s, a.rpA, a.rpT, n, C->din0.p, C->dout0.p);
            hipLaunchKernelGGL(k_scc_diag, dim3(grid_for((uint64_t)n, kSccBlock, 8192)), dim3(kSccBlock), 0, s, a,
                               C->din0.p, C->dout0.p);
            GX_TRY(check_launch("k_scc_diag"));
        }
        return GX_SUCCESS;
    }

    // Stage 2: every vertex alive.
    int start() {
        h = SccState{};
        h.trim = kn.trim;
        h.pivot_left = kn.pivot;
        h.plabel = kAlive;
        h.whole = 1;
        h.alive = (u64)n;
        GX_HIP_TRY(hipMemcpyAsync(C->st.p, &h, sizeof(h), hipMemcpyHostToDevice, s));
        KTimer kt(ctx, "scc_init", s);
        hipLaunchKernelGGL(k_scc_init, dim3(sweep_grid()), dim3(kSccBlock), 0, s, n, C->lab.p);
        return check_launch("k_scc_init");
    }

    // `steps` steps of plan (with its solo rounds) and step; past the end they return at once.
    int enqueue(int steps) {
        const unsigned grid = grid_for((uint64_t)n, kSccBlock, kn.grid);
        for (int i = 0; i < steps; i++) {
            {
                KTimer kt(ctx, "scc_plan", s);
                hipLaunchKernelGGL(k_scc_plan, dim3(1), dim3(kSccBlock), 0, s, C->st.p, a, (uint32_t)kn.solo);
            }
            KTimer kt(ctx, "scc_step", s);
            hipLaunchKernelGGL(k_scc_step, dim3(grid), dim3(kSccBlock), 0, s, C->st.p, a);
        }
        return check_launch("k_scc_step");
    }

    // GX_SCC_VERBOSE: where the call's time went, stage by stage, in microseconds.
    void print_ticks() const {
        static const char *names[kDone] = {"zero", "count", "seed", "trim", "pick", "fwd", "bwd", "meet", "label",
                                           "cinit", "cprop", "root", "cbwd"};
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device) != hipSuccess || khz <= 0) return;
        std::fprintf(stderr, "gx_scc: us");
        for (int i = 0; i < kDone; i++) std::fprintf(stderr, " %s %.1f", names[i], 1000.0 * (double)h.ticks[i] / khz);
        std::fprintf(stderr, "\n");
    }

    // Stage 3: batches of steps until the state says done, read one batch late.
    int run() {
        SccState *hs = static_cast<SccState *>(ctx->staging[0]);
        u64 last_steps = ~0ull;
        int stuck = 0;
        GX_TRY(enqueue(kn.batch));
        for (;;) {
            GX_HIP_TRY(hipMemcpyAsync(hs, C->st.p, sizeof(SccState), hipMemcpyDeviceToHost, s));
            GX_HIP_TRY(hipEventRecord(C->ev, s));
            GX_TRY(enqueue(kn.batch));
            GX_HIP_TRY(hipEventSynchronize(C->ev));
            h = *hs;
            if (kn.verbose)
                std::fprintf(stderr, "gx_scc: stage %u outer %llu trim %llu levels %llu colour %llu back %llu pivot %lld "
                             "alive %llu steps %llu done %u\n", h.stage, h.outer, h.trim_rounds, h.levels,
                             h.colour_rounds, h.back_levels, h.plabel == kAlive ? -1ll : (long long)h.pivot, h.alive,
                             h.steps, h.stage == kDone);
            if (h.stage == kDone) {
                if (kn.verbose) print_ticks();
                return GX_SUCCESS;
            }
            // every batch runs at least one step
            stuck = h.steps == last_steps ? stuck + 1 : 0;
            last_steps = h.steps;
            if (stuck > 2) return fail(GX_PANIC, "gx_scc: the steps did not advance");
        }
    }

    // Stage 4: the three statistics, on the device.
    int finish(uint64_t *stats) {
        SccState *hs = static_cast<SccState *>(ctx->staging[0]);
        GX_HIP_TRY(hipMemsetAsync(C->aux.p, 0, (size_t)n * sizeof(uint32_t), s));
        {
            KTimer kt(ctx, "scc_finish", s);
            hipLaunchKernelGGL(k_scc_sizes, dim3(sweep_grid()), dim3(kSccBlock), 0, s, n, C->lab.p, C->st.p, C->aux.p);
            hipLaunchKernelGGL(k_scc_stats, dim3(sweep_grid()), dim3(kSccBlock), 0, s, n, C->lab.p, C->aux.p, C->st.p);
            GX_TRY(check_launch("k_scc_stats"));
        }
        GX_HIP_TRY(hipMemcpyAsync(hs, C->st.p, sizeof(SccState), hipMemcpyDeviceToHost, s));
        GX_HIP_TRY(hipStreamSynchronize(s));
        h = *hs;
        stats[0] = (uint64_t)h.ncomp;
        stats[1] = (uint64_t)h.largest;
        stats[2] = (uint64_t)h.singles;
        return GX_SUCCESS;
    }
};

}  // namespace
}  // namespace gx

using namespace gx;

extern "C" int gx_scc(gx_graph *g, uint64_t *comp, uint64_t *stats) {
    if (!g || (!comp && !stats)) return fail(GX_NULL_POINTER, "gx_scc: null argument");
    if (g->n == 0) {
        if (stats) stats[0] = stats[1] = stats[2] = 0;
        return GX_SUCCESS;
    }
    gx_ctx *ctx = g->ctx;
    GX_HIP_TRY(hipSetDevice(ctx->device));
    if (g->directed) GX_TRY(ensure_transpose(g));   // kept with g; built before the bracket
    SccCall c(g);
    GX_TRY(device_begin(ctx));
    GX_TRY(c.prep());
    GX_TRY(c.start());
    GX_TRY(c.run());
    if (c.h.alive != 0) return fail(GX_PANIC, "gx_scc: vertices left alive");
    uint64_t st3[3] = {0, 0, 0};
    if (stats) GX_TRY(c.finish(st3));
    GX_TRY(device_end(ctx));
    if (comp) GX_TRY(download(ctx, comp, c.C->lab.p, (uint64_t)c.n, Xfer::Widen32));
    if (stats) std::copy(st3, st3 + 3, stats);
    return GX_SUCCESS;
}

GX_MODULE_WARMER(scc)

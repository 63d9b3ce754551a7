// gx_cdlp_tiers.hip -- one CDLP iteration: the tier kernels (by degree: tiny, small, light, mid,
// huge; the table in gx_cdlp.hip), the sparse kernels of an active iteration, the tier lists
// (cdlp_plan) and the launches (cdlp_iteration).  gx_cdlp and the partitioned API share it.
#include <algorithm>
#include <vector>

#include "gx_cdlp.h"

namespace gx {
namespace {

// Tiny vertices (deg <= kTiny, including isolated ones): one THREAD per vertex, labels in
// registers (all loads in flight), 64 vertices per wave instead of one (two thirds of the
// vertices of a power-law graph have degree <= 8, 84 % of SYN-7_5's <= 32).  The strict-
// majority vote first; else the labels are sorted in registers (a bitonic network, unrolled)
// and the longest run wins, the first one (smallest label) among equal runs.
__device__ __forceinline__ void sort_regs(uint32_t (&L)[kTiny]) {
#pragma unroll
    for (int k = 2; k <= kTiny; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1)
#pragma unroll
            for (int i = 0; i < kTiny; i++) {
                const int l = i ^ j;
                if (l > i) {
                    const uint32_t x = L[i], y = L[l];
                    const bool up = (i & k) == 0;
                    L[i] = up ? min(x, y) : max(x, y);
                    L[l] = up ? max(x, y) : min(x, y);
                }
            }
}

__global__ __launch_bounds__(kCdlpBlock) void k_cdlp_tiny(CdlpArgs a) {
    const bool kp = keep_on(a);
    if (tier_idle(a) && !kp) return;
    bool any = false;
    const bool all = all_active(a) || kp;
    for (int64_t v = a.v0 + (int64_t)blockIdx.x * kCdlpBlock + threadIdx.x; v < a.v1;
         v += (int64_t)gridDim.x * kCdlpBlock) {
        const int64_t ob = a.rpA[v], od = a.rpA[v + 1] - ob;
        int64_t ib = 0, id = 0;
        if (a.rpT) {
            ib = a.rpT[v];
            id = a.rpT[v + 1] - ib;
        }
        const int64_t d = od + id;
        if (d > kTiny) continue;
        const int32_t old = a.lab[v];
        int32_t best = old;
        if (d > 0 && active(a, all, v)) {
            uint32_t L[kTiny];
#pragma unroll
            for (int k = 0; k < kTiny; k++) L[k] = k < d ? (uint32_t)label_at(a, ob, od, ib, k) : kEmpty;
            Vote vt{kEmpty, 0u};
#pragma unroll
            for (int k = 0; k < kTiny; k++) vt = vote_add(vt, L[k], k < d);
            uint32_t nc = 0;
#pragma unroll
            for (int k = 0; k < kTiny; k++) nc += (k < d && L[k] == vt.c) ? 1u : 0u;
            uint32_t cnt = 0;   // the winner's count (the recount bound)
            if (a.first) {
                uint32_t mn = kEmpty;
#pragma unroll
                for (int k = 0; k < kTiny; k++) mn = min(mn, L[k]);   // padding is kEmpty
                best = (int32_t)mn;
            } else if (2 * (int64_t)nc > d) {
                best = (int32_t)vt.c;   // strict majority
                cnt = nc;
            } else {
                sort_regs(L);           // labels ascending, the padding last
                uint32_t bc = 0, bl = kEmpty, run = 0, prev = kEmpty;
#pragma unroll
                for (int k = 0; k < kTiny; k++) {
                    run = L[k] == prev ? run + 1u : 1u;
                    prev = L[k];
                    if (k < d && run > bc) {
                        bc = run;
                        bl = L[k];
                    }
                }
                best = (int32_t)bl;
                cnt = bc;
            }
            bound_set(a, v, cnt);
        }
        a.nxt[v] = best;
        any |= best != old;
    }
    if (__ballot(any) && (threadIdx.x & (kWave - 1)) == 0) raise_flag_sharded(a.changed, a.cshards);
}

// Small vertices (kTiny < deg <= 64), from a list: one wave per vertex, labels in registers,
// counts by shuffles; no LDS, so the kernel runs at full occupancy.
__global__ __launch_bounds__(kCdlpBlock) void k_cdlp_small(CdlpArgs a, const int32_t *__restrict__ sv,
                                                           int32_t nsmall) {
    if (tier_idle(a)) return;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t gw = ((int64_t)blockIdx.x * kCdlpBlock + threadIdx.x) / kWave;
    const int64_t nw = (int64_t)gridDim.x * (kCdlpBlock / kWave);
    bool any = false;
    const bool all = all_active(a);
    for (int64_t i = gw; i < nsmall; i += nw) {
        const int64_t v = sv[i];
        const VMeta m = vmeta_act(a, all, v);
        const int64_t ob = m.ob, od = m.od, ib = m.ib, id = m.id;
        const int64_t d = od + id;
        const int32_t old = a.lab[v];
        const uint32_t my = lane < d ? (uint32_t)label_at(a, ob, od, ib, lane) : kEmpty;
        const uint32_t cand = __shfl(wave_vote(Vote{my, lane < d ? 1u : 0u}).c, 0, kWave);
        int32_t best;
        uint32_t cnt = 0;   // the winner's count (the recount bound)
        const uint32_t ncand = (uint32_t)__popcll(__ballot(lane < d && my == cand));
        if (d == 0) {
            best = old;   // inactive (or isolated)
        } else if (a.first) {
            best = (int32_t)wave_min_u32(my);
        } else if (2 * (int64_t)ncand > d) {
            best = (int32_t)cand;   // strict majority
            cnt = ncand;
        } else {
            // one round per distinct label: the first remaining lane's label, its lanes by one
            // ballot (lane reads, no LDS; the d shuffles this replaces were ds_bpermute each)
            unsigned long long rem = __ballot(lane < d);
            uint32_t bc = 0, bl = kEmpty;
            while (rem) {
                const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)my, __ffsll((long long)rem) - 1);
                const unsigned long long eq = __ballot(my == l) & rem;
                const uint32_t c = (uint32_t)__popcll(eq);
                if (c > bc || (c == bc && l < bl)) {
                    bc = c;
                    bl = l;
                }
                rem &= ~eq;
            }
            best = (int32_t)bl;
            cnt = bc;
        }
        if (lane == 0) {
            a.nxt[v] = best;
            any |= best != old;
            if (d > 0) bound_set(a, v, cnt);
        }
    }
    if (any) raise_flag_sharded(a.changed, a.cshards);
}

// Light vertices (64 < deg <= kSlots/2), from a list: one wave per vertex, an LDS hash table of
// 2 deg slots per wave.  Two instances: kLightSlots for deg <= kLightSlots/2 (2 KiB per wave,
// so LDS does not cap occupancy) and kLdsHash for the rest.
template <int kSlots>
__global__ __launch_bounds__(kCdlpBlock) void k_cdlp_light(CdlpArgs a, const int32_t *__restrict__ lv,
                                                           int32_t nlight) {
    if (tier_idle(a)) return;
    __shared__ uint32_t keys[kCdlpBlock / kWave][kSlots];
    __shared__ uint32_t cnts[kCdlpBlock / kWave][kSlots];
    constexpr int R = kSlots / (2 * kWave);   // label rounds of the largest vertex of the tier
    const int lane = threadIdx.x & (kWave - 1);
    const int wv = threadIdx.x / kWave;
    uint32_t *K = keys[wv];
    uint32_t *C = cnts[wv];
    const int64_t nw = (int64_t)gridDim.x * (kCdlpBlock / kWave);
    int64_t i = ((int64_t)blockIdx.x * kCdlpBlock + threadIdx.x) / kWave;
    if (i >= nlight) return;
    bool any = false;
    const bool all = all_active(a);
    // software-pipelined over the wave's vertices like k_cdlp_mid: the next vertex's
    // dependent loads are issued one link at a time between this vertex's LDS phases
    int64_t v = lv[i];
    VMeta m = vmeta_act(a, all, v);
    uint32_t L[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int64_t k = (int64_t)r * kWave + lane;
        L[r] = k < (int64_t)m.od + m.id ? (uint32_t)a.lab[col_at(a, m, k)] : kEmpty;
    }
    for (;;) {
        const int64_t d = (int64_t)m.od + m.id;
        const int64_t inext = i + nw;
        const bool more = inext < nlight;
        const int64_t vn = more ? (int64_t)lv[inext] : v;      // next vertex, link 1
        const int32_t old = a.lab[v];
        // strict-majority fast path (a wave-uniform branch)
        Vote vt{kEmpty, 0u};
#pragma unroll
        for (int r = 0; r < R; r++) vt = vote_add(vt, L[r], (int64_t)r * kWave + lane < d);
        uint32_t cand = __shfl(wave_vote(vt).c, 0, kWave);
        int64_t nc = 0;
#pragma unroll
        for (int r = 0; r < R; r++)
            if ((int64_t)r * kWave < d) nc += __popcll(__ballot((int64_t)r * kWave + lane < d && L[r] == cand));
        if (a.first) {
            uint32_t mn = kEmpty;
#pragma unroll
            for (int r = 0; r < R; r++) mn = (int64_t)r * kWave + lane < d ? min(mn, L[r]) : mn;
            cand = wave_min_u32(mn);
        }
        const bool maj = 2 * nc > d || a.first || d == 0;   // d == 0: inactive, keeps its label
        int log2ts = 1;
        while ((1ll << log2ts) < 2 * d) log2ts++;
        const int ts = 1 << log2ts;
        if (!maj) {
            for (int s = lane; s < ts; s += kWave) {
                K[s] = kEmpty;
                C[s] = 0;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        const VMeta mn = vmeta_act(a, all, vn);                 // link 2
        const int64_t dn = more ? (int64_t)mn.od + mn.id : 0;
        if (!maj) {
#pragma unroll
            for (int r = 0; r < R; r++)
                if ((int64_t)r * kWave < d) lds_table_add_wave(K, C, L[r], (int64_t)r * kWave + lane < d, log2ts);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        int64_t cn[R];                                          // link 3
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int64_t k = (int64_t)r * kWave + lane;
            cn[r] = k < dn ? col_at(a, mn, k) : -1;
        }
        unsigned long long key = 0;
        if (!maj) {
            for (int s = lane; s < ts; s += kWave) {
                const uint32_t c = C[s];
                if (c) {
                    const unsigned long long kk = pack(c, K[s]);
                    key = kk > key ? kk : key;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++) L[r] = cn[r] >= 0 ? (uint32_t)a.lab[cn[r]] : kEmpty;   // link 4
        const unsigned long long wk = maj ? 0ull : wave_max_u64(key);
        const int32_t best = d == 0 ? old : maj ? (int32_t)cand : (int32_t)(kEmpty - (uint32_t)(wk & 0xffffffffu));
        // the winner's count (the recount bound; 0 for the first iteration's minimum)
        const uint32_t cnt = a.first ? 0u : maj ? (uint32_t)nc : (uint32_t)(wk >> 32);
        if (!maj) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        if (lane == 0) {
            a.nxt[v] = best;
            any |= best != old;
            if (d > 0) bound_set(a, v, cnt);
        }
        if (!more) break;
        i = inext;
        v = vn;
        m = mn;
    }
    if (any) raise_flag_sharded(a.changed, a.cshards);
}

// Huge vertices (deg > kMidMax): the label multiset is cut into kHugeChunk-label chunks; a
// 1024-thread workgroup histograms one chunk in a 64 KiB LDS table, then adds each distinct
// label once into the vertex's global table, so global atomics scale with distinct labels per
// chunk, not with the degree.  A global slot is one 64-bit word, (epoch << 58) | (count << 31) |
// label, claimed and counted by one CAS: a slot whose epoch is not this iteration's is empty, so
// the tables are never cleared (but once every kHugeEpochs iterations) and never scanned.  Every
// successful CAS knows the label's count so far; a label's last update carries its final count,
// so the maximum of (count << 32) | ~label over the updates is the vertex's winner.  Each
// workgroup folds its updates into one 64-bit atomicMax on the vertex's key.
constexpr int kHugeBlock = 1024;
constexpr int kHugeChunk = 4096;
constexpr int kHugeSlots = 2 * kHugeChunk;
constexpr int kHugeEpochs = 63;                   // epochs 1..63 in the top 6 bits; 0: never used
constexpr int64_t kHugeMaxDeg = (1ll << 27) - 1;  // the count field (bits 31..57)

__global__ __launch_bounds__(kHugeBlock) void k_cdlp_huge_insert(CdlpArgs a, const int32_t *__restrict__ hv,
                                                                 const int64_t *__restrict__ hoff,
                                                                 const int32_t *__restrict__ hlog2,
                                                                 const int32_t *__restrict__ cvert,
                                                                 const int64_t *__restrict__ cbeg,
                                                                 unsigned long long *gtab, uint32_t epoch,
                                                                 unsigned long long *vkey) {
    __shared__ uint32_t K[kHugeSlots];
    __shared__ uint32_t C[kHugeSlots];
    __shared__ unsigned long long red[kHugeBlock / kWave];
    constexpr int kLog2 = 13;   // log2(kHugeSlots)
    const int tid = threadIdx.x;
    const int32_t hi = cvert[blockIdx.x];
    const int64_t v = hv[hi];
    if (!active(a, all_active(a), v)) return;
    const int64_t ob = a.rpA[v], od = a.rpA[v + 1] - ob;
    int64_t ib = 0, id = 0;
    if (a.rpT) {
        ib = a.rpT[v];
        id = a.rpT[v + 1] - ib;
    }
    // the recount bound: a vertex whose label provably keeps a strict majority skips the
    // recount (every chunk of the vertex decides alike)
    if (bound_keeps(a, v, od + id)) return;
    const int64_t k0 = cbeg[blockIdx.x], k1 = min(k0 + kHugeChunk, od + id);
    for (int s = tid; s < kHugeSlots; s += kHugeBlock) {
        K[s] = kEmpty;
        C[s] = 0;
    }
    __syncthreads();
    constexpr int R = kHugeChunk / kHugeBlock;   // the chunk's gathers all in flight first
    uint32_t L[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int64_t k = k0 + (int64_t)r * kHugeBlock + tid;
        L[r] = k < k1 ? (uint32_t)label_at(a, ob, od, ib, k) : kEmpty;
    }
    if (a.first) {   // the chunk's smallest label, as a count-1 key (no tables)
        uint32_t mn = kEmpty;
#pragma unroll
        for (int r = 0; r < R; r++) mn = k0 + (int64_t)r * kHugeBlock + tid < k1 ? min(mn, L[r]) : mn;
        mn = wave_min_u32(mn);
        if ((tid & (kWave - 1)) == 0 && mn != kEmpty) atomicMax(&vkey[hi], pack(1u, mn));
        return;
    }
#pragma unroll
    for (int r = 0; r < R; r++)
        if (k0 + (int64_t)r * kHugeBlock < k1) lds_table_add_wave(K, C, L[r], k0 + (int64_t)r * kHugeBlock + tid < k1, kLog2);
    __syncthreads();
    const int log2ts = hlog2[hi];
    const int64_t ts = 1ll << log2ts;
    unsigned long long *GT = gtab + hoff[hi];
    const unsigned long long ep = (unsigned long long)epoch << 58;
    unsigned long long key = 0;
    for (int s = tid; s < kHugeSlots; s += kHugeBlock) {
        const uint32_t c = C[s];
        if (!c) continue;
        const uint32_t l = K[s];
        int64_t h = hash_slot(l, log2ts);
        unsigned long long old = GT[h];   // a stale copy only costs a failed CAS
        for (;;) {
            const bool live = (old & (63ull << 58)) == ep;
            if (live && (uint32_t)(old & 0x7fffffffu) != l) {   // another label's slot: probe on
                h = (h + 1) & (ts - 1);
                old = GT[h];
                continue;
            }
            const unsigned long long nw = live ? old + ((unsigned long long)c << 31)
                                               : ep | ((unsigned long long)c << 31) | (unsigned long long)l;
            const unsigned long long prev = atomicCAS(&GT[h], old, nw);
            if (prev == old) {
                const unsigned long long kk = pack((uint32_t)((nw >> 31) & kHugeMaxDeg), l);
                key = kk > key ? kk : key;
                break;
            }
            old = prev;
        }
    }
    key = wave_max_u64(key);
    if ((tid & (kWave - 1)) == 0) red[tid / kWave] = key;
    __syncthreads();
    if (tid == 0) {
        unsigned long long m = red[0];
        for (int w = 1; w < kHugeBlock / kWave; w++) m = red[w] > m ? red[w] : m;
        if (m) atomicMax(&vkey[hi], m);
    }
}

__global__ void k_cdlp_huge_final(CdlpArgs a, const int32_t *__restrict__ hv, int32_t nhuge,
                                  unsigned long long *vkey) {
    for (int32_t hi = blockIdx.x * blockDim.x + threadIdx.x; hi < nhuge; hi += gridDim.x * blockDim.x) {
        const int64_t v = hv[hi];
        // recomputed (a key), or inactive / kept by the majority bound (its label stays)
        const unsigned long long k = vkey[hi];
        const int32_t best = k ? (int32_t)(kEmpty - (uint32_t)(k & 0xffffffffu)) : a.lab[v];
        if (k) bound_set(a, v, a.first ? 0u : (uint32_t)(k >> 32));
        vkey[hi] = 0;   // clean for the next iteration
        a.nxt[v] = best;
        if (best != a.lab[v]) raise_flag_sharded(a.changed, a.cshards);
    }
}

// Medium vertices (kLdsHash/2 < deg <= kMidSlots/2): one workgroup per vertex with a
// kMidSlots-slot hash table in LDS; workgroups loop over the medium-vertex list so the table
// is reused without a relaunch.  Three sizes (kMid2 / kMid4 / kMid): 256 threads, 4K slots,
// 4 per CU; 512, 8K, 2 per CU; 1024, 16K, 1 per CU.
// Software-pipelined over the list: a vertex's labels sit at the end of a chain of dependent
// loads (list -> row pointers -> column ids -> labels, ~1 us each), so the next vertex's chain
// is issued one link at a time between the current vertex's LDS phases (clear, insert, scan):
// each load's wait lands after the LDS work that follows its issue.
template <int kMidBlock, int kMidSlots>
__global__ __launch_bounds__(kMidBlock) void k_cdlp_mid(CdlpArgs a, const int32_t *__restrict__ mv, int32_t nmid) {
    if (tier_idle(a)) return;
    __shared__ uint32_t K[kMidSlots];
    __shared__ uint32_t C[kMidSlots];
    __shared__ unsigned long long red[kMidBlock / kWave];
    __shared__ uint32_t cnt[kMidBlock / kWave];
    __shared__ uint32_t bcast[1];
    constexpr int R = kMidSlots / (2 * kMidBlock);
    const int tid = threadIdx.x;
    bool any = false;
    int32_t i = blockIdx.x;
    if (i >= nmid) return;
    const bool all = all_active(a);
    int64_t v = mv[i];
    VMeta m = vmeta_act(a, all, v);
    uint32_t L[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int64_t k = (int64_t)r * kMidBlock + tid;
        L[r] = k < (int64_t)m.od + m.id ? (uint32_t)a.lab[col_at(a, m, k)] : kEmpty;
    }
    for (;;) {
        const int64_t d = (int64_t)m.od + m.id;
        const int32_t inext = i + (int32_t)gridDim.x;
        const bool more = inext < nmid;
        // link 1 of the next vertex: its id
        const int64_t vn = more ? (int64_t)mv[inext] : v;
        // strict-majority fast path: the workgroup's candidate, then its exact count (the
        // first iteration of an undirected graph: the smallest label).  d, a.first and so the
        // branches are the same in every thread; an inactive vertex (d == 0) skips it all.
        uint32_t cand = kEmpty;
        bool maj = true;
        uint32_t ccount = 0;   // the candidate's count (the recount bound; 0 in the first iteration)
        if (d > 0 && a.first) {
            uint32_t mn = kEmpty;
#pragma unroll
            for (int r = 0; r < R; r++) mn = (int64_t)r * kMidBlock + tid < d ? min(mn, L[r]) : mn;
            mn = wave_min_u32(mn);
            if ((tid & (kWave - 1)) == 0) cnt[tid / kWave] = mn;
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kMidBlock / kWave; j++) cand = min(cand, cnt[j]);
        } else if (d > 0) {
            Vote vt{kEmpty, 0u};
#pragma unroll
            for (int r = 0; r < R; r++) vt = vote_add(vt, L[r], (int64_t)r * kMidBlock + tid < d);
            vt = wave_vote(vt);
            if ((tid & (kWave - 1)) == 0) red[tid / kWave] = ((unsigned long long)vt.c << 32) | vt.n;
            __syncthreads();
            if (tid == 0) {
                Vote w{(uint32_t)(red[0] >> 32), (uint32_t)red[0]};
                for (int j = 1; j < kMidBlock / kWave; j++) w = vote_merge(w, Vote{(uint32_t)(red[j] >> 32), (uint32_t)red[j]});
                bcast[0] = w.c;
            }
            __syncthreads();
            cand = bcast[0];
            uint32_t mc = 0;
#pragma unroll
            for (int r = 0; r < R; r++) mc += ((int64_t)r * kMidBlock + tid < d && L[r] == cand) ? 1u : 0u;
            mc = wave_sum_u32(mc);
            if ((tid & (kWave - 1)) == 0) cnt[tid / kWave] = mc;
            __syncthreads();
            uint32_t nc = 0;
#pragma unroll
            for (int j = 0; j < kMidBlock / kWave; j++) nc += cnt[j];
            maj = 2 * (int64_t)nc > d;
            ccount = nc;
        }
        int log2ts = 1;
        while ((1ll << log2ts) < 2 * d) log2ts++;
        const int ts = 1 << log2ts;
        if (!maj) {
            for (int s = tid; s < ts; s += kMidBlock) {
                K[s] = kEmpty;
                C[s] = 0;
            }
            __syncthreads();
        }
        // link 2: its row pointers
        const VMeta mn = vmeta_act(a, all, vn);
        const int64_t dn = more ? (int64_t)mn.od + mn.id : 0;
        if (!maj) {
#pragma unroll
            for (int r = 0; r < R; r++)
                if ((int64_t)r * kMidBlock < d) lds_table_add_wave(K, C, L[r], (int64_t)r * kMidBlock + tid < d, log2ts);
            __syncthreads();
        }
        // link 3: its column ids
        int64_t cn[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int64_t k = (int64_t)r * kMidBlock + tid;
            cn[r] = k < dn ? col_at(a, mn, k) : -1;
        }
        unsigned long long key = 0;
        if (!maj) {
            for (int s = tid; s < ts; s += kMidBlock) {
                const uint32_t c = C[s];
                if (c) {
                    const unsigned long long kk = pack(c, K[s]);
                    key = kk > key ? kk : key;
                }
            }
        }
        // link 4: its labels
#pragma unroll
        for (int r = 0; r < R; r++) L[r] = cn[r] >= 0 ? (uint32_t)a.lab[cn[r]] : kEmpty;
        if (maj) {
            if (tid == 0) {
                const int32_t best = d == 0 ? a.lab[v] : (int32_t)cand;
                a.nxt[v] = best;
                any |= best != a.lab[v];
                if (d > 0) bound_set(a, v, ccount);
            }
        } else {
            key = wave_max_u64(key);
            if ((tid & (kWave - 1)) == 0) red[tid / kWave] = key;
            __syncthreads();
            if (tid == 0) {
                unsigned long long mx = red[0];
                for (int w = 1; w < kMidBlock / kWave; w++) mx = red[w] > mx ? red[w] : mx;
                const int32_t best = (int32_t)(kEmpty - (uint32_t)(mx & 0xffffffffu));
                a.nxt[v] = best;
                any |= best != a.lab[v];
                bound_set(a, v, (uint32_t)(mx >> 32));
            }
        }
        if (d > 0) __syncthreads();   // red / cnt / bcast and the table are free for the next vertex
        if (!more) break;
        i = inext;
        v = vn;
        m = mn;
    }
    if (any) raise_flag_sharded(a.changed, a.cshards);
}

// Sparse iterations, active vertices of degree <= kSparseWaveMax: one wave each (the light
// tier's method: strict-majority vote, else a 2d-slot LDS hash table).  When *dense and the
// iteration has no tier kernels (a sparse-only iteration, fl != null), every vertex of the
// fallback list fl is recomputed instead.
// The role bodies take their block index and block count (bid, nblk) and their LDS (lds) as
// arguments, so k_cdlp_sparse_fused can run several roles in one launch.
constexpr int kSparseWaveSlots = 2 * kSparseWaveMax;
constexpr size_t kSparseWaveLds = (size_t)2 * (256 / kWave) * kSparseWaveSlots * sizeof(uint32_t);

__device__ __forceinline__ void sparse_wave_role(const CdlpArgs &a, const int32_t *__restrict__ wl, int64_t asub,
                                                 const unsigned int *wcount, const int32_t *__restrict__ fl,
                                                 int64_t fn, int64_t bid, int64_t nblk, uint32_t *lds) {
    const bool full = *a.dense != 0;
    if (full && !fl) return;
    constexpr int kSlots = kSparseWaveSlots;
    constexpr int R = kSparseWaveMax / kWave;
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t *K = lds + (threadIdx.x / kWave) * kSlots;
    uint32_t *C = lds + (256 / kWave) * kSlots + (threadIdx.x / kWave) * kSlots;
    const int64_t gw = (bid * 256 + threadIdx.x) / kWave;
    const int64_t nw = nblk * (256 / kWave);   // a multiple of kCdlpSubs
    const int j = (int)(gw % kCdlpSubs);
    const int32_t *src = full ? fl : wl + (int64_t)j * asub;
    const int64_t c = full ? fn : (int64_t)shard_count(wcount, j, asub);
    const int64_t step = full ? nw : nw / kCdlpSubs;
    bool any = false;
    for (int64_t i = full ? gw : gw / kCdlpSubs; i < c; i += step) {
        const int64_t v = src[i];
        const VMeta m = vmeta(a, v);
        const int64_t d = (int64_t)m.od + m.id;
        if (bound_keeps(a, v, d)) continue;   // its label provably stays (nxt already holds it)
        uint32_t L[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int64_t k = (int64_t)r * kWave + lane;
            L[r] = k < d ? (uint32_t)a.lab[col_at(a, m, k)] : kEmpty;
        }
        const int32_t old = a.lab[v];
        Vote vt{kEmpty, 0u};
#pragma unroll
        for (int r = 0; r < R; r++) vt = vote_add(vt, L[r], (int64_t)r * kWave + lane < d);
        const uint32_t cand = __shfl(wave_vote(vt).c, 0, kWave);
        int64_t nc = 0;
#pragma unroll
        for (int r = 0; r < R; r++)
            if ((int64_t)r * kWave < d) nc += __popcll(__ballot((int64_t)r * kWave + lane < d && L[r] == cand));
        int32_t best = old;
        uint32_t cnt = 0;   // the winner's count (the recount bound)
        if (d > 0 && 2 * nc > d) {
            best = (int32_t)cand;
            cnt = (uint32_t)nc;
        } else if (d > 0) {
            int log2ts = 1;
            while ((1ll << log2ts) < 2 * d) log2ts++;
            const int ts = 1 << log2ts;
            for (int t = lane; t < ts; t += kWave) {
                K[t] = kEmpty;
                C[t] = 0;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int r = 0; r < R; r++)
                if ((int64_t)r * kWave < d) lds_table_add_wave(K, C, L[r], (int64_t)r * kWave + lane < d, log2ts);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            unsigned long long key = 0;
            for (int t = lane; t < ts; t += kWave) {
                const uint32_t cc = C[t];
                if (cc) {
                    const unsigned long long kk = pack(cc, K[t]);
                    key = kk > key ? kk : key;
                }
            }
            const unsigned long long wk = wave_max_u64(key);
            best = (int32_t)(kEmpty - (uint32_t)(wk & 0xffffffffu));
            cnt = (uint32_t)(wk >> 32);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        if (lane == 0) {
            a.nxt[v] = best;
            any |= best != old;
            if (d > 0) bound_set(a, v, cnt);
        }
    }
    if (any) raise_flag_sharded(a.changed, a.cshards);
}


// Sparse iterations, active vertices of kSparseWaveMax < degree <= kMidMax: one workgroup each,
// kMaxDeg / kBlock labels per thread in registers, the strict-majority vote, else a kSlots-slot
// LDS table (the mid tier's method, without its pipelining).  Shapes: 256 threads / 4K slots
// (four or more workgroups per CU) for both lists; a vertex above 2048 without a majority (its
// 2d slots do not fit; none from SYN-7_5's fourth iteration on) is appended to `redo`, which
// the 1024-thread / 16K-slot instance then recomputes (rin: that list, *rcount entries).
// Fallback when *dense in a sparse-only iteration: every vertex of fl then fl2.
template <int kBlock, int kSlots>
constexpr size_t sparse_group_lds() {
    return (size_t)2 * kSlots * sizeof(uint32_t) + (kBlock / kWave) * (sizeof(unsigned long long) + sizeof(uint32_t)) +
           sizeof(uint32_t);
}

template <int kBlock, int kSlots, int kMaxDeg>
__device__ __forceinline__ void sparse_group_role(const CdlpArgs &a, const int32_t *__restrict__ gl, int64_t asub,
                                                  const unsigned int *gcount, const int32_t *__restrict__ fl,
                                                  int64_t fn, const int32_t *__restrict__ fl2, int64_t fn2,
                                                  int32_t *redo, unsigned int *rcount, const int32_t *__restrict__ rin,
                                                  int64_t bid, int64_t nblk, uint32_t *lds) {
    const bool full = !rin && *a.dense != 0;
    if (full && !fl && !fl2) return;
    uint32_t *K = lds;
    uint32_t *C = lds + kSlots;
    unsigned long long *red = reinterpret_cast<unsigned long long *>(lds + 2 * kSlots);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(red + kBlock / kWave);
    uint32_t *bcast = cnt + kBlock / kWave;
    constexpr int R = kMaxDeg / kBlock;
    constexpr int NW = kBlock / kWave;
    const int tid = threadIdx.x;
    const int j = (int)(bid % kCdlpSubs);   // the block count is a multiple of kCdlpSubs
    const int32_t *src = rin ? rin : full ? fl : gl + (int64_t)j * asub;
    const int64_t c = rin ? (int64_t)*rcount : full ? fn + fn2 : (int64_t)shard_count(gcount, j, asub);
    const int64_t step = rin || full ? nblk : nblk / kCdlpSubs;
    bool any = false;
    for (int64_t i = rin || full ? bid : bid / kCdlpSubs; i < c; i += step) {
        const int64_t v = full && i >= fn ? fl2[i - fn] : src[i];   // full: fn == 0 when fl is null
        const VMeta m = vmeta(a, v);
        const int64_t d = (int64_t)m.od + m.id;
        if (bound_keeps(a, v, d)) continue;   // uniform in the workgroup; nxt already holds the label
        uint32_t L[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int64_t k = (int64_t)r * kBlock + tid;
            L[r] = k < d ? (uint32_t)a.lab[col_at(a, m, k)] : kEmpty;
        }
        Vote vt{kEmpty, 0u};
#pragma unroll
        for (int r = 0; r < R; r++) vt = vote_add(vt, L[r], (int64_t)r * kBlock + tid < d);
        vt = wave_vote(vt);
        if ((tid & (kWave - 1)) == 0) red[tid / kWave] = ((unsigned long long)vt.c << 32) | vt.n;
        __syncthreads();
        if (tid == 0) {
            Vote w{(uint32_t)(red[0] >> 32), (uint32_t)red[0]};
            for (int q = 1; q < NW; q++) w = vote_merge(w, Vote{(uint32_t)(red[q] >> 32), (uint32_t)red[q]});
            bcast[0] = w.c;
        }
        __syncthreads();
        const uint32_t cand = bcast[0];
        uint32_t mc = 0;
#pragma unroll
        for (int r = 0; r < R; r++) mc += ((int64_t)r * kBlock + tid < d && L[r] == cand) ? 1u : 0u;
        mc = wave_sum_u32(mc);
        if ((tid & (kWave - 1)) == 0) cnt[tid / kWave] = mc;
        __syncthreads();
        uint32_t nc = 0;
#pragma unroll
        for (int q = 0; q < NW; q++) nc += cnt[q];
        int32_t best = (int32_t)cand;
        uint32_t wcount = nc;   // the winner's count (the recount bound)
        if (2 * (int64_t)nc <= d && 2 * d > kSlots) {
            // no majority and no room for the table: the 16K-slot instance recomputes it
            if (tid == 0) redo[atomicAdd(rcount, 1u)] = (int32_t)v;
            __syncthreads();   // red / cnt / bcast are free for the next vertex
            continue;
        }
        if (2 * (int64_t)nc <= d) {
            int log2ts = 1;
            while ((1ll << log2ts) < 2 * d) log2ts++;
            const int ts = 1 << log2ts;
            for (int t = tid; t < ts; t += kBlock) {
                K[t] = kEmpty;
                C[t] = 0;
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < R; r++)
                if ((int64_t)r * kBlock < d) lds_table_add_wave(K, C, L[r], (int64_t)r * kBlock + tid < d, log2ts);
            __syncthreads();
            unsigned long long key = 0;
            for (int t = tid; t < ts; t += kBlock) {
                const uint32_t cc = C[t];
                if (cc) {
                    const unsigned long long kk = pack(cc, K[t]);
                    key = kk > key ? kk : key;
                }
            }
            key = wave_max_u64(key);
            if ((tid & (kWave - 1)) == 0) red[tid / kWave] = key;   // red was last read before bcast
            __syncthreads();
            unsigned long long mx = red[0];
            for (int q = 1; q < NW; q++) mx = red[q] > mx ? red[q] : mx;
            best = (int32_t)(kEmpty - (uint32_t)(mx & 0xffffffffu));
            wcount = (uint32_t)(mx >> 32);
        }
        if (tid == 0) {
            const int32_t old = a.lab[v];
            a.nxt[v] = best;
            any |= best != old;
            if (d > 0) bound_set(a, v, wcount);
        }
        __syncthreads();   // red / cnt / bcast / the table are free for the next vertex
    }
    if (any) raise_flag_sharded(a.changed, a.cshards);
}

template <int kBlock, int kSlots, int kMaxDeg>
__global__ __launch_bounds__(kBlock) void k_cdlp_sparse_group(CdlpArgs a, const int32_t *__restrict__ gl,
                                                              int64_t asub, const unsigned int *gcount,
                                                              const int32_t *__restrict__ fl, int64_t fn,
                                                              const int32_t *__restrict__ fl2, int64_t fn2,
                                                              int32_t *redo, unsigned int *rcount,
                                                              const int32_t *__restrict__ rin) {
    __shared__ uint32_t lds[(sparse_group_lds<kBlock, kSlots>() + 3) / 4];
    sparse_group_role<kBlock, kSlots, kMaxDeg>(a, gl, asub, gcount, fl, fn, fl2, fn2, redo, rcount, rin, blockIdx.x,
                                               gridDim.x, lds);
}

// Two sparse roles of an iteration in one launch: blocks [0, 8S) recompute the wave list,
// [8S, 12S) the 2048-degree list (S = kCdlpSubs), each as its own kernel would; the
// 8192-degree list is k_cdlp_sparse_big's.  The roles are independent (they read `cur` and
// write disjoint vertices), and in a sparse iteration each is a short chain of dependent
// loads, so one launch overlaps them instead of running them in turn.  Block b of a launch
// plays block boff + b (always 0 now: the one-launch-per-range form is retired).
struct SparseFusedArgs {
    const int32_t *al;
    int64_t asub;
    const unsigned int *cnt;   // the three lists' counters (kCdlpSubs * kCntStride apart)
    const int32_t *fw, *fg2, *fg4, *fg;   // fallback lists (sparse-only iterations) or null
    int64_t nfw, nfg2, nfg4, nfg;
    int32_t *redo;
    unsigned int *rcount;
};

__global__ __launch_bounds__(256) void k_cdlp_sparse_fused(CdlpArgs a, SparseFusedArgs f, int boff) {
    constexpr size_t kLds = kSparseWaveLds > sparse_group_lds<kMid2Block, kMid2Slots>()
                                ? kSparseWaveLds
                                : sparse_group_lds<kMid2Block, kMid2Slots>();
    __shared__ uint32_t lds[(kLds + 3) / 4];
    const int64_t S = kCdlpSubs, shards = S * f.asub;
    const int64_t b = (int64_t)blockIdx.x + boff;
    if (b < 8 * S) {
        sparse_wave_role(a, f.al, f.asub, f.cnt, f.fw, f.nfw, b, 8 * S, lds);
    } else {
        sparse_group_role<kMid2Block, kMid2Slots, kMid2Max>(a, f.al + shards, f.asub, f.cnt + S * kCntStride, f.fg2,
                                                            f.nfg2, nullptr, 0, nullptr, nullptr, nullptr, b - 8 * S,
                                                            4 * S, lds);
    }
}

// The 8192-degree list on 512-thread workgroups, 16 labels per thread in registers: as a third
// role of k_cdlp_sparse_fused (256 threads, 32 labels each) it set the fused kernel's registers
// to 175 VGPRs, two workgroups per CU for every role.
constexpr int kSparseBigBlock = 512;
__global__ __launch_bounds__(kSparseBigBlock) void k_cdlp_sparse_big(CdlpArgs a, SparseFusedArgs f) {
    __shared__ uint32_t lds[(sparse_group_lds<kSparseBigBlock, kMid2Slots>() + 3) / 4];
    const int64_t S = kCdlpSubs, shards = S * f.asub;
    sparse_group_role<kSparseBigBlock, kMid2Slots, kMidMax>(a, f.al + 2 * shards, f.asub, f.cnt + 2 * S * kCntStride,
                                                            f.fg4, f.nfg4, f.fg, f.nfg, f.redo, f.rcount, nullptr,
                                                            blockIdx.x, gridDim.x, lds);
}

}  // namespace

// A host list on the device: allocated and copied when it is not empty.
template <typename T>
static int put_list(DBuf<T> &d, const std::vector<T> &v, hipStream_t s) {
    if (v.empty()) return GX_SUCCESS;
    GX_TRY(d.alloc(v.size()));
    GX_HIP_TRY(hipMemcpyAsync(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return GX_SUCCESS;
}

int cdlp_plan(const CdlpGraph &g, int64_t v0, int64_t v1, CdlpPlan &P, hipStream_t s) {
    std::vector<int32_t> hv, hl, mv, cvert, lv, mv2, sv, mv4, lvs, wall;
    std::vector<int64_t> hoff, cbeg;
    int64_t total = 0;
    for (int64_t v = v0; v < v1; v++) {
        int64_t d = g.h_rpA[v + 1] - g.h_rpA[v];
        if (g.directed) d += g.h_rpT[v + 1] - g.h_rpT[v];
        if (d <= kSparseWaveMax) wall.push_back((int32_t)v);
        if (d <= kTiny) continue;   // k_cdlp_tiny scans the range itself
        std::vector<int32_t> *tier = d <= kWave ? &sv : d <= kLightSlots / 2 ? &lvs : d <= kLdsHash / 2 ? &lv :
                                     d <= kMid2Max ? &mv2 : d <= kMid4Max ? &mv4 : d <= kMidMax ? &mv : &hv;
        if (tier == &hv) {
            if (d > kHugeMaxDeg) return fail(GX_INVALID_VALUE, "gx_cdlp: a vertex degree exceeds 2^27 - 1");
            int l2 = 1;
            while ((1ll << l2) < 2 * d) l2++;
            for (int64_t c = 0; c < d; c += kHugeChunk) {
                cvert.push_back((int32_t)hv.size());
                cbeg.push_back(c);
            }
            hl.push_back(l2);
            hoff.push_back(total);
            total += 1ll << l2;
        }
        tier->push_back((int32_t)v);
    }
    P.v0 = v0;
    P.v1 = v1;
    P.n_light = lv.size();
    P.n_light_s = lvs.size();
    P.n_small = sv.size();
    P.n_mid4 = mv4.size();
    P.n_mid2 = mv2.size();
    P.n_mid = mv.size();
    P.n_huge = hv.size();
    P.n_chunks = cvert.size();
    P.n_wall = wall.size();
    P.total = total;
    GX_TRY(put_list(P.d_mv4, mv4, s));
    GX_TRY(put_list(P.d_sv, sv, s));
    if (!hv.empty()) {
        GX_TRY(P.gtab.alloc(total));
        GX_TRY(P.vkey.alloc(hv.size()));
        GX_HIP_TRY(hipMemsetAsync(P.vkey.p, 0, hv.size() * 8, s));
        GX_HIP_TRY(hipMemsetAsync(P.gtab.p, 0, (size_t)total * 8, s));   // epoch 0: every slot empty
        P.epoch = 0;
    }
    GX_TRY(put_list(P.d_hv, hv, s));
    GX_TRY(put_list(P.d_hl, hl, s));
    GX_TRY(put_list(P.d_hoff, hoff, s));
    GX_TRY(put_list(P.d_cvert, cvert, s));
    GX_TRY(put_list(P.d_cbeg, cbeg, s));
    GX_TRY(put_list(P.d_mv, mv, s));
    GX_TRY(put_list(P.d_mv2, mv2, s));
    GX_TRY(put_list(P.d_lvs, lvs, s));
    GX_TRY(put_list(P.d_wall, wall, s));
    GX_TRY(put_list(P.d_lv, lv, s));
    GX_HIP_TRY(hipStreamSynchronize(s));   // host vectors go out of scope
    return GX_SUCCESS;
}

// One synchronous iteration for the plan's vertices: nxt[v] for v in [v0, v1) from cur
// (the full label array); *changed is set when a label moved (caller zeroes it).
// The tier kernels write disjoint vertices and only read `cur`; they run on one stream
// (overlapped on three they slow each other down: DESIGN.md).
int cdlp_iteration(const CdlpGraph &g, CdlpPlan &P, const int32_t *cur, int32_t *nxt, int *changed, hipStream_t s,
                   const CdlpStep &st) {
    gx_ctx *ctx = g.ctx;
    const SparseLists *sl = st.sl;
    CdlpArgs a{g.rpA,  g.ciA,  g.rpT,  g.ciT,    cur,      nxt,      g.n,      changed,
               P.v0,   P.v1,   st.act, st.stamp, st.dense, st.first && !g.directed ? 1 : 0,
               sl ? 1 : 0,     st.cshards};
    a.keep = st.keep;
    if (st.bd) {
        a.vlb = st.bd->vlb;
        a.vchg = st.bd->vchg;
        a.hvalid = st.bd->hvalid;
    }
    const bool tiers = !(sl && sl->only);   // sparse-only: the huge tier alone beside the sparse kernels
    const unsigned tiny_grid = grid_for((uint64_t)(P.v1 - P.v0), kCdlpBlock, 8192);
    if (sl) {
        // exit at once when *dense (the tier kernels below then recompute every vertex)
        KTimer kt(ctx, "cdlp_sparse", s);
        const unsigned int *cnt = sl->counts + kCdlpSubs * kCntStride;
        // a sparse-only iteration's fallback lists (nothing else recomputes these vertices)
        const bool o = sl->only;
        const SparseFusedArgs f{sl->al, sl->asub, cnt,
                                o ? P.d_wall.p : nullptr, o ? P.d_mv2.p : nullptr, o ? P.d_mv4.p : nullptr,
                                o ? P.d_mv.p : nullptr,
                                (int64_t)P.n_wall, (int64_t)P.n_mid2, (int64_t)P.n_mid4, (int64_t)P.n_mid,
                                sl->redo, sl->rcount};
        hipLaunchKernelGGL(k_cdlp_sparse_fused, dim3(12 * kCdlpSubs), dim3(256), 0, s, a, f, 0);
        GX_TRY(check_launch("k_cdlp_sparse_fused"));
        hipLaunchKernelGGL(k_cdlp_sparse_big, dim3(8 * kCdlpSubs), dim3(kSparseBigBlock), 0, s, a, f);
        GX_TRY(check_launch("k_cdlp_sparse_big"));
        hipLaunchKernelGGL((k_cdlp_sparse_group<kMidBlock, kMidSlots, kMidMax>), dim3(kCdlpSubs), dim3(kMidBlock), 0,
                           s, a, nullptr, (int64_t)0, nullptr, nullptr, (int64_t)0, nullptr, (int64_t)0, nullptr,
                           sl->rcount, sl->redo);
        GX_TRY(check_launch("k_cdlp_sparse_redo"));
        if (o && st.keep && P.v1 > P.v0) {   // the own-label check's tiny vertices (no tier kernels here)
            hipLaunchKernelGGL(k_cdlp_tiny, dim3(tiny_grid), dim3(kCdlpBlock), 0, s, a);
            GX_TRY(check_launch("k_cdlp_tiny"));
        }
    }
    // A list tier: kern over the cnt vertices of `list`; its timer is the label without the "k_".
    auto tier = [&](const char *label, auto kern, size_t grid, int block, const int32_t *list, size_t cnt) {
        if (!tiers || !cnt) return (int)GX_SUCCESS;
        KTimer kt(ctx, label + 2, s);
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(block), 0, s, a, list, (int32_t)cnt);
        return check_launch(label);
    };
    auto waves = [](size_t cnt) { return (size_t)grid_for((uint64_t)cnt * kWave, kCdlpBlock, 8192); };   // one per vertex
    const size_t cus = (size_t)std::max(1, ctx->num_cus);
    GX_TRY(tier("k_cdlp_mid2", k_cdlp_mid<kMid2Block, kMid2Slots>, std::min(P.n_mid2, cus * 4), kMid2Block, P.d_mv2.p,
                P.n_mid2));
    if (P.n_huge) {
        KTimer kt(ctx, "cdlp_heavy", s);
        uint32_t ep = P.epoch;
        if (!a.first) {   // a new epoch empties every table slot; past the last one, a real clear
            if (++ep > (uint32_t)kHugeEpochs) {
                GX_HIP_TRY(hipMemsetAsync(P.gtab.p, 0, (size_t)P.total * 8, s));
                ep = 1;
            }
            P.epoch = ep;
        }
        hipLaunchKernelGGL(k_cdlp_huge_insert, dim3((unsigned)P.n_chunks), dim3(kHugeBlock), 0, s, a, P.d_hv.p,
                           P.d_hoff.p, P.d_hl.p, P.d_cvert.p, P.d_cbeg.p, P.gtab.p, ep, P.vkey.p);
        GX_TRY(check_launch("k_cdlp_huge_insert"));
        hipLaunchKernelGGL(k_cdlp_huge_final, dim3(grid_for(P.n_huge, 64, 1024)), dim3(64), 0, s, a, P.d_hv.p,
                           (int32_t)P.n_huge, P.vkey.p);
        GX_TRY(check_launch("k_cdlp_huge_final"));
    }
    GX_TRY(tier("k_cdlp_light", k_cdlp_light<kLdsHash>, waves(P.n_light), kCdlpBlock, P.d_lv.p, P.n_light));
    GX_TRY(tier("k_cdlp_mid", k_cdlp_mid<kMidBlock, kMidSlots>, std::min(P.n_mid, cus), kMidBlock, P.d_mv.p, P.n_mid));
    GX_TRY(tier("k_cdlp_mid4", k_cdlp_mid<kMid4Block, kMid4Slots>, std::min(P.n_mid4, cus * 2), kMid4Block, P.d_mv4.p,
                P.n_mid4));
    GX_TRY(tier("k_cdlp_small", k_cdlp_small, waves(P.n_small), kCdlpBlock, P.d_sv.p, P.n_small));
    GX_TRY(tier("k_cdlp_light_s", k_cdlp_light<kLightSlots>, waves(P.n_light_s), kCdlpBlock, P.d_lvs.p, P.n_light_s));
    if (tiers && P.v1 > P.v0) {
        KTimer kt(ctx, "cdlp_tiny", s);
        hipLaunchKernelGGL(k_cdlp_tiny, dim3(tiny_grid), dim3(kCdlpBlock), 0, s, a);
        GX_TRY(check_launch("k_cdlp_tiny"));
    }
    return GX_SUCCESS;
}

}  // namespace gx

GX_MODULE_WARMER(cdlp_tiers)

// gx_lcc.hip -- local clustering coefficient via degree-oriented triangle enumeration.
//
// Replaces LA_LCC -> LAGraph_lcc(&d, A, symmetric = !directed) (lcc.cpp:61-71), which
// SuiteSparse runs as a masked SpGEMM (C<S> = S*S-type, PLUS_PAIR) plus reductions.
// With N(v) = in(v) U out(v) (the undirected closure S, built on the device) and
// k = |N(v)|:
//     LCC(v) = #{(u, w) in E : u, w in N(v)} / (k (k - 1)),   0 when k < 2.
// Each triangle {a, b, c} of S contributes to a the number of stored directions between b
// and c (1 or 2: the popcount of that S entry's flag byte), and likewise for b and c.
// Triangles are enumerated once each on the degree-ordered orientation O of S (edge v->u
// when (deg u, u) > (deg v, v)), whose out-degrees are at most sqrt(2|E|).
//   orientation : O and its transpose I = O^T (lcc_orient, gx_lcc_orient.hip);
//   triangles   : each triangle {v, u, x} (v -> u, v -> x, u -> x) is found at its middle
//                 vertex u: O(u) goes into an LDS hash table (flag popcount kept with each
//                 key) and the lists O(v), v in I(u), are walked by load-balanced waves and
//                 probed -- sum |O(v)| probes over oriented edges, 0.45x of probing O(u) per
//                 (v, u).  The three contributions are summed on chip (u in a register, v in
//                 an LDS slot per v, x in its hash slot) and leave as one 64-bit atomic per
//                 (work item, contribution target).
//   tiers       : work item (u, 64 in-neighbours) per wave for |O(u)| <= 512 (512- or
//                 1024-slot tables), (u, 256) per workgroup up to kBlockMax (LDS sized to the
//                 tier's largest |O(u)|), a merge-intersection fallback beyond (not reached
//                 on degree-oriented graphs below ~2^25 edges);
//   dense core  : optionally, the triangles among the highest-degree vertices as an int8 GEMM
//                 (lcc_dense_build / lcc_dense_count, gx_lcc_dense.hip).
// This file has the work items, the tiers and gx_lcc itself; gx_lcc_part.hip the partitioned
// entry points, which run the same stages on a range of middle vertices.
// Oriented entries are packed as (vertex << 2) | popcount(flag), so n < 2^29.
// Counts are exact integers, so the result is deterministic and equal to the oracle bit for
// bit (one fp64 division per vertex).
#include <algorithm>
#include <cstdlib>
#include <functional>
#include <memory>

#include "gx_lcc.h"

namespace gx {
namespace {

constexpr uint32_t kCntMask = (1u << 30) - 1;   // hash value: flag popcount << 30 | x count

__device__ __forceinline__ uint32_t hash_slot(int32_t x, uint32_t mask) {
    return ((uint32_t)x * 0x9E3779B1u) & mask;
}

__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- work items ----
// A triangle {v, u, x} with v -> u, v -> x, u -> x (ranks v < u < x) is found once, at its
// middle vertex u: O(u) goes into an LDS hash table and the lists O(v) of the in-neighbours
// v in I(u) are probed against it.  This costs sum over oriented edges (v, u) of |O(v)|,
// less than half of probing O(u) for every (v, u) (2.4 G -> 1.06 G probes on SYN-cit).
// Work item = (u, chunk of I(u)): kWaveGroup in-neighbours for the wave tier, kBlockGroup for
// the workgroup tier, so hubs with large in-lists spread over many waves.
constexpr int kWaveGroup = kWave;
constexpr int kBlockGroup = kLccBlock;
constexpr int kClassTile = 4096;

__global__ __launch_bounds__(kLccBlock) void k_lcc_items(const int64_t *__restrict__ orp,
                                                         const int64_t *__restrict__ irp, int64_t v0, int64_t v1,
                                                         int32_t wave_max, int32_t wave2_max, int32_t block_max,
                                                         uint64_t *items0, uint64_t *items1, uint64_t *items2,
                                                         int32_t *big_list, uint32_t *counts /* 4 tiers + max d */) {
    constexpr int kTiers = 4;
    __shared__ uint32_t tot[kTiers], base[kTiers], off[kTiers];
    uint64_t *items[3] = {items0, items1, items2};
    for (int64_t t0 = v0 + (int64_t)blockIdx.x * kClassTile; t0 < v1; t0 += (int64_t)gridDim.x * kClassTile) {
        const int64_t t1 = min(t0 + (int64_t)kClassTile, v1);
        if (threadIdx.x < kTiers) {
            tot[threadIdx.x] = 0;
            off[threadIdx.x] = 0;
        }
        __syncthreads();
        for (int pass = 0; pass < 2; pass++) {
            for (int64_t u = t0 + threadIdx.x; u < t1; u += kLccBlock) {
                const int64_t d = orp[u + 1] - orp[u], e = irp[u + 1] - irp[u];
                if (d == 0 || e == 0) continue;
                const int tier = d <= wave_max ? 0 : (d <= wave2_max ? 1 : (d <= block_max ? 2 : 3));
                const int64_t group = tier == 2 ? kBlockGroup : kWaveGroup;
                const uint32_t ni = tier == 3 ? 1u : (uint32_t)((e + group - 1) / group);
                if (pass == 0) {
                    atomicAdd(&tot[tier], ni);
                    if (tier == 2) atomicMax(&counts[4], (uint32_t)d);
                } else {
                    const uint32_t pos = base[tier] + atomicAdd(&off[tier], ni);
                    if (tier == 3) {
                        big_list[pos] = (int32_t)u;
                    } else {
                        for (uint32_t j = 0; j < ni; j++) items[tier][pos + j] = ((uint64_t)u << 32) | j;
                    }
                }
            }
            __syncthreads();
            if (pass == 0 && threadIdx.x < kTiers)
                base[threadIdx.x] = tot[threadIdx.x] ? atomicAdd(&counts[threadIdx.x], tot[threadIdx.x]) : 0u;
            __syncthreads();
        }
    }
}

// Build the hash table of O(u) (key x, value popcount(u,x) << 30) with `nthreads` threads.
__device__ __forceinline__ void table_build(const int64_t *__restrict__ orp, const uint32_t *__restrict__ ocode,
                                            int32_t u, int32_t *hkey, uint32_t *hval, uint32_t slots, int tid,
                                            int nthreads) {
    const int64_t b = orp[u], d = orp[u + 1] - b;
    const uint32_t hmask = slots - 1;
    for (int64_t i = tid; i < d; i += nthreads) {
        const uint32_t c = ocode[b + i];
        const int32_t x = (int32_t)(c >> 2);
        uint32_t h = hash_slot(x, hmask);
        while (atomicCAS(&hkey[h], -1, x) != -1) h = (h + 1) & hmask;   // keys of a row are distinct
        hval[h] = (c & 3u) << 30;
    }
}

// Per-wave LDS scratch of probe_in_group: the nonempty lists by rank, and the list starts
// falling in the current 64-entry window.
struct WaveScratch {
    uint64_t rank[kWave];   // (O(v) start - list offset) as 48-bit signed | popcount(v,u) << 48 | lane << 56
    uint8_t mark[kWave];
};

// Which list holds position E0 + lane of the concatenated lists, and where that entry is in
// ocode: lists starting inside the window mark their offset, one ballot turns the marks into a
// mask, and the list's rank is cb (lists started before the window) plus the marks at or below
// the lane.  Replaces a 6-step shuffle binary search (six dependent ds_bpermute per window).
__device__ __forceinline__ int64_t probe_locate(WaveScratch *ws, int32_t excl, int32_t vl, int lane, int32_t E0,
                                                int32_t total, int &cb, uint64_t &pk, bool &act) {
    if (vl > 0 && excl >= E0 && excl < E0 + kWave) ws->mark[excl - E0] = 1;
    wave_sync_lds();
    const unsigned long long M = __ballot(ws->mark[lane] != 0);
    ws->mark[lane] = 0;
    const int32_t e = E0 + lane;
    act = e < total;
    const unsigned long long upto = lane == kWave - 1 ? ~0ull : ((2ull << lane) - 1ull);
    const int r = cb + __popcll(M & upto) - 1;
    cb += __popcll(M);
    pk = act ? ws->rank[r] : 0ull;
    wave_sync_lds();
    return ((int64_t)(pk << 16) >> 16) + e;
}

// Probe the lists O(v) of the (up to 64) in-neighbours icode[ib .. ie) of u, one per lane,
// against the table of O(u).  Lanes walk the concatenated lists 64 entries at a time; the next
// window's entries are located and loaded before the current one is probed.  Returns u's
// contribution; v's go to vcnt[lane], x's into the table values.
__device__ __forceinline__ unsigned long long probe_in_group(const int64_t *__restrict__ orp,
                                                             const uint32_t *__restrict__ ocode,
                                                             const uint32_t *__restrict__ icode, int64_t ib,
                                                             int64_t ie, const int32_t *hkey, uint32_t *hval,
                                                             uint32_t hmask, uint32_t *vcnt, int lane,
                                                             WaveScratch *ws) {
    const int64_t i = ib + lane;
    const bool has = i < ie;
    const uint32_t ic = has ? icode[i] : 0u;
    const int32_t v = (int32_t)((ic >> 2) & kVMask);
    const uint32_t p_vu = ic & 3u;
    // a dense-core in-neighbour (dense bit): its triangles {v, u, x} lie wholly in the core
    // (u and x rank above v) and are counted by the core's MFMA pass (k_lcc_dense_mfma)
    const bool walk = has && !(ic & kDenseBit);
    const int64_t vb = walk ? orp[v] : 0;
    const int32_t vl = walk ? (int32_t)(orp[v + 1] - vb) : 0;
    int32_t incl = vl;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int32_t y = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += y;
    }
    const int32_t total = __shfl(incl, kWave - 1, kWave);
    const int32_t excl = incl - vl;
    const unsigned long long ne = __ballot(vl > 0);
    if (vl > 0)
        ws->rank[__popcll(ne & ((1ull << lane) - 1ull))] =
            ((uint64_t)(vb - excl) & 0xffffffffffffull) | ((uint64_t)p_vu << 48) | ((uint64_t)lane << 56);
    ws->mark[lane] = 0;
    unsigned long long tu = 0;
    if (total == 0) return tu;
    int cb = 0;
    uint64_t pk;
    bool act;
    int64_t k = probe_locate(ws, excl, vl, lane, 0, total, cb, pk, act);
    uint32_t c = act ? ocode[k] : 0u;
    for (int32_t e0 = 0; e0 < total; e0 += kWave) {
        const uint32_t cc = c;
        const uint64_t pc = pk;
        const bool ac = act;
        if (e0 + kWave < total) {
            k = probe_locate(ws, excl, vl, lane, e0 + kWave, total, cb, pk, act);
            c = act ? ocode[k] : 0u;
        }
        if (ac) {
            const int32_t x = (int32_t)(cc >> 2);
            uint32_t h = hash_slot(x, hmask);
            int32_t key;
            while ((key = hkey[h]) != x && key != -1) h = (h + 1) & hmask;
            if (key == x) {
                tu += cc & 3u;                                         // u: directions between v and x
                atomicAdd(&vcnt[pc >> 56], hval[h] >> 30);             // v: directions between u and x
                atomicAdd(&hval[h], (uint32_t)(pc >> 48) & 3u);        // x: directions between v and u
            }
        }
    }
    return tu;
}

// Slots of the hash table of a list of d entries: the power of two from 2 d up, at least 64.
__host__ __device__ __forceinline__ uint32_t table_slots(int64_t d) {
    uint32_t slots = 64;
    while (slots < 2 * (uint32_t)d) slots <<= 1;
    return slots;
}

// The workgroup tier's tables: sized for the tier's largest |O(u)|, which is at most kBlockMax.
inline uint32_t block_slots(uint32_t dmax) { return std::min<uint32_t>(kBlockSlots, table_slots(dmax)); }

template <int kWaveSlots>
__global__ __launch_bounds__(kLccBlock) void k_lcc_wave(const int64_t *__restrict__ orp,
                                                        const uint32_t *__restrict__ ocode,
                                                        const int64_t *__restrict__ irp,
                                                        const uint32_t *__restrict__ icode,
                                                        const uint64_t *__restrict__ items, uint32_t count,
                                                        unsigned long long *tc) {
    __shared__ int32_t s_key[kWavesPerBlock][kWaveSlots];
    __shared__ uint32_t s_val[kWavesPerBlock][kWaveSlots];
    __shared__ uint32_t s_vcnt[kWavesPerBlock][kWave];
    __shared__ WaveScratch s_ws[kWavesPerBlock];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    int32_t *hkey = s_key[wv];
    uint32_t *hval = s_val[wv];
    uint32_t *vcnt = s_vcnt[wv];
    const uint32_t nw = gridDim.x * kWavesPerBlock;
    for (uint32_t li = blockIdx.x * kWavesPerBlock + wv; li < count; li += nw) {
        const uint64_t item = items[li];
        const int32_t u = (int32_t)(item >> 32);
        const int64_t ib = irp[u] + (int64_t)(uint32_t)item * kWaveGroup, ie = min(irp[u + 1], ib + kWaveGroup);
        const uint32_t slots = table_slots(orp[u + 1] - orp[u]);
        for (uint32_t s = lane; s < slots; s += kWave) {
            hkey[s] = -1;
            hval[s] = 0;
        }
        vcnt[lane] = 0;
        wave_sync_lds();
        table_build(orp, ocode, u, hkey, hval, slots, lane, kWave);
        wave_sync_lds();
        unsigned long long tu =
            probe_in_group(orp, ocode, icode, ib, ie, hkey, hval, slots - 1, vcnt, lane, &s_ws[wv]);
        wave_sync_lds();
        const uint32_t c = vcnt[lane];
        if (c && ib + lane < ie) atomicAdd(&tc[(icode[ib + lane] >> 2) & kVMask], (unsigned long long)c);
        for (uint32_t s = lane; s < slots; s += kWave) {
            const uint32_t cx = hval[s] & kCntMask;
            if (cx) atomicAdd(&tc[hkey[s]], (unsigned long long)cx);
        }
        for (int off = 32; off > 0; off >>= 1) tu += __shfl_xor(tu, off, kWave);
        if (lane == 0 && tu) atomicAdd(&tc[u], tu);
        wave_sync_lds();
    }
}

__global__ __launch_bounds__(kLccBlock) void k_lcc_block(const int64_t *__restrict__ orp,
                                                         const uint32_t *__restrict__ ocode,
                                                         const int64_t *__restrict__ irp,
                                                         const uint32_t *__restrict__ icode,
                                                         const uint64_t *__restrict__ items, uint32_t count,
                                                         uint32_t max_slots, unsigned long long *tc) {
    extern __shared__ uint32_t dyn[];   // max_slots keys, then max_slots values
    int32_t *hkey = reinterpret_cast<int32_t *>(dyn);
    uint32_t *hval = dyn + max_slots;
    __shared__ uint32_t s_vcnt[kWavesPerBlock][kWave];
    __shared__ WaveScratch s_ws[kWavesPerBlock];
    __shared__ unsigned long long s_tu[kWavesPerBlock];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    uint32_t *vcnt = s_vcnt[wv];
    for (uint32_t li = blockIdx.x; li < count; li += gridDim.x) {
        const uint64_t item = items[li];
        const int32_t u = (int32_t)(item >> 32);
        const int64_t ib0 = irp[u] + (int64_t)(uint32_t)item * kBlockGroup, ie0 = min(irp[u + 1], ib0 + kBlockGroup);
        const uint32_t slots = table_slots(orp[u + 1] - orp[u]);
        for (uint32_t s = threadIdx.x; s < slots; s += kLccBlock) {
            hkey[s] = -1;
            hval[s] = 0;
        }
        vcnt[lane] = 0;
        __syncthreads();
        table_build(orp, ocode, u, hkey, hval, slots, threadIdx.x, kLccBlock);
        __syncthreads();
        const int64_t ib = ib0 + (int64_t)wv * kWave, ie = min(ie0, ib + kWave);
        unsigned long long tu = 0;
        if (ib < ie) tu = probe_in_group(orp, ocode, icode, ib, ie, hkey, hval, slots - 1, vcnt, lane, &s_ws[wv]);
        wave_sync_lds();
        const uint32_t c = vcnt[lane];
        if (c && ib + lane < ie) atomicAdd(&tc[(icode[ib + lane] >> 2) & kVMask], (unsigned long long)c);
        for (int off = 32; off > 0; off >>= 1) tu += __shfl_xor(tu, off, kWave);
        if (lane == 0) s_tu[wv] = tu;
        __syncthreads();
        for (uint32_t s = threadIdx.x; s < slots; s += kLccBlock) {
            const uint32_t cx = hval[s] & kCntMask;
            if (cx) atomicAdd(&tc[hkey[s]], (unsigned long long)cx);
        }
        if (threadIdx.x == 0) {
            unsigned long long t = 0;
            for (int w = 0; w < kWavesPerBlock; w++) t += s_tu[w];
            if (t) atomicAdd(&tc[u], t);
        }
        __syncthreads();
    }
}

// Fallback for |O(u)| > kBlockMax: thread per in-neighbour v of one u, merge intersection of
// the sorted lists O(v) and O(u).
__global__ __launch_bounds__(kLccBlock) void k_lcc_merge_in(const int64_t *__restrict__ orp,
                                                            const uint32_t *__restrict__ ocode,
                                                            const int64_t *__restrict__ irp,
                                                            const uint32_t *__restrict__ icode, int32_t u,
                                                            unsigned long long *tc) {
    const int64_t ub = orp[u], ue = orp[u + 1];
    for (int64_t t = irp[u] + (int64_t)blockIdx.x * kLccBlock + threadIdx.x; t < irp[u + 1];
         t += (int64_t)gridDim.x * kLccBlock) {
        const uint32_t ic = icode[t];
        if (ic & kDenseBit) continue;   // wholly in the dense core (k_lcc_dense_mfma)
        const int32_t v = (int32_t)((ic >> 2) & kVMask);
        const uint32_t p_vu = ic & 3u;
        int64_t i = orp[v], j = ub;
        const int64_t ie = orp[v + 1];
        unsigned long long tv = 0, tu = 0;
        while (i < ie && j < ue) {
            const uint32_t a = ocode[i], b = ocode[j];
            if ((a >> 2) < (b >> 2)) {
                i++;
            } else if ((a >> 2) > (b >> 2)) {
                j++;
            } else {
                tv += b & 3u;   // v: directions between u and x
                tu += a & 3u;   // u: directions between v and x
                atomicAdd(&tc[a >> 2], (unsigned long long)p_vu);
                i++;
                j++;
            }
        }
        if (tv) atomicAdd(&tc[v], tv);
        if (tu) atomicAdd(&tc[u], tu);
    }
}

__global__ void k_lcc_final(const int64_t *__restrict__ srp, const unsigned long long *__restrict__ tc,
                            int64_t n, double *__restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n;
         v += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = srp[v + 1] - srp[v];
        out[v] = k < 2 ? 0.0 : (double)tc[v] / ((double)k * (double)(k - 1));
    }
}

}  // namespace

// The only place that reads a knob (gx_lcc.h LccKnobs).
LccKnobs lcc_knobs() {
    const auto limit = [](const char *name, int32_t compiled) {
        const char *e = std::getenv(name);
        if (!e || !*e) return compiled;
        return (int32_t)std::min<long>(std::max<long>(std::atol(e), 1), compiled);
    };
    LccKnobs k;
    k.wave_max = limit("GX_LCC_WAVE_MAX", kWaveMax);
    k.wave2_max = std::max(k.wave_max, limit("GX_LCC_WAVE2_MAX", kWave2Max));
    k.block_max = std::max(k.wave2_max, limit("GX_LCC_BLOCK_MAX", kBlockMax));
    const char *ce = std::getenv("GX_LCC_CORE");
    k.core = ce ? std::atoi(ce) : 0;
    return k;
}

int lcc_items(const LccOrient &O, int64_t v0, int64_t v1, const LccKnobs &kn, LccItems &L, hipStream_t s) {
    const int64_t nv = v1 - v0;
    if (nv <= 0 || O.m == 0) return GX_SUCCESS;
    const uint64_t icap = (uint64_t)nv + (uint64_t)O.m / kWaveGroup + 64;
    DBuf<uint32_t> counts;
    GX_TRY(L.items0.alloc(icap));
    GX_TRY(L.items1.alloc(icap));
    GX_TRY(L.items2.alloc(icap));
    GX_TRY(L.big.alloc(nv));
    GX_TRY(counts.alloc(5));
    GX_HIP_TRY(hipMemsetAsync(counts.p, 0, 20, s));
    hipLaunchKernelGGL(k_lcc_items, dim3((unsigned)std::min<int64_t>((nv + kClassTile - 1) / kClassTile, 2048)),
                       dim3(kLccBlock), 0, s, O.orp.p, O.irp.p, v0, v1, kn.wave_max, kn.wave2_max, kn.block_max,
                       L.items0.p, L.items1.p, L.items2.p, L.big.p, counts.p);
    GX_TRY(check_launch("k_lcc_items"));
    GX_HIP_TRY(hipMemcpyAsync(L.hc, counts.p, 20, hipMemcpyDeviceToHost, s));
    GX_HIP_TRY(hipStreamSynchronize(s));
    if (L.hc[3]) {
        L.h_big.resize(L.hc[3]);
        GX_HIP_TRY(hipMemcpyAsync(L.h_big.data(), L.big.p, L.hc[3] * 4, hipMemcpyDeviceToHost, s));
        GX_HIP_TRY(hipStreamSynchronize(s));
    }
    return GX_SUCCESS;
}

int lcc_count_items(gx_graph *g, const LccOrient &O, const LccItems &L, unsigned long long *tc, hipStream_t s) {
    gx_ctx *ctx = g->ctx;
    if (O.m == 0) return GX_SUCCESS;
    const uint32_t *hc = L.hc;
    const int64_t *orp = O.orp.p, *irp = O.irp.p;
    const uint32_t *ocode = O.ocode.p, *icode = O.icode.p;
    const auto wave_grid = [](uint32_t items) { return dim3(grid_for((uint64_t)items * kWave, kLccBlock, 8192)); };
    const uint32_t slots = block_slots(hc[4]);
    // one nested timer per launched tier: their launch counts tell which tiers ran
    const struct {
        const char *timer;
        uint32_t items;
        std::function<int()> launch;
    } tiers[] = {
        {"lcc_wave", hc[0],
         [&] {
             hipLaunchKernelGGL(k_lcc_wave<512>, wave_grid(hc[0]), dim3(kLccBlock), 0, s, orp, ocode, irp, icode,
                                L.items0.p, hc[0], tc);
             return check_launch("k_lcc_wave<512>");
         }},
        {"lcc_wave2", hc[1],
         [&] {
             hipLaunchKernelGGL(k_lcc_wave<1024>, wave_grid(hc[1]), dim3(kLccBlock), 0, s, orp, ocode, irp, icode,
                                L.items1.p, hc[1], tc);
             return check_launch("k_lcc_wave<1024>");
         }},
        {"lcc_block", hc[2],
         [&] {
             hipLaunchKernelGGL(k_lcc_block, dim3(std::min<uint32_t>(hc[2], 4096)), dim3(kLccBlock),
                                (size_t)slots * 8, s, orp, ocode, irp, icode, L.items2.p, hc[2], slots, tc);
             return check_launch("k_lcc_block");
         }},
        {"lcc_merge", hc[3],
         [&] {
             for (int32_t u : L.h_big) {
                 hipLaunchKernelGGL(k_lcc_merge_in, dim3(64), dim3(kLccBlock), 0, s, orp, ocode, irp, icode, u, tc);
                 GX_TRY(check_launch("k_lcc_merge_in"));
             }
             return (int)GX_SUCCESS;
         }},
    };
    KTimer kt(ctx, "lcc_triangles", s);
    // more than 64 KiB of dynamic LDS is an opt-in, taken outside the tier's timer
    if (hc[2] && slots * 8 > 65536)
        GX_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_lcc_block),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)(slots * 8)));
    for (const auto &t : tiers) {
        if (!t.items) continue;
        KTimer kw(ctx, t.timer, s);
        GX_TRY(t.launch());
    }
    return GX_SUCCESS;
}

int lcc_finish(const int64_t *srp, const unsigned long long *tc, int64_t n, double *out, hipStream_t s) {
    if (n == 0) return GX_SUCCESS;
    hipLaunchKernelGGL(k_lcc_final, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, srp, tc, n, out);
    return check_launch("k_lcc_final");
}

namespace {

// One gx_lcc call and its stages, in the order the entry point runs them.
struct LccCall {
    gx_graph *g;
    LccKnobs kn;
    gx_ctx *ctx;
    hipStream_t s;
    int64_t n;
    LccCache *C = nullptr;

    explicit LccCall(gx_graph *g_) : g(g_), kn(lcc_knobs()), ctx(g_->ctx), s(g_->ctx->stream), n((int64_t)g_->n) {}

    // Stage 1: the closure, and the cache when the graph has none.  The knobs go into the cache
    // build and nowhere else, so a graph keeps the limits and the core it was first called with.
    int prep() {
        GX_TRY(ensure_closure(g));
        C = static_cast<LccCache *>(g->lcc.get());
        if (C) return GX_SUCCESS;
        auto fresh = std::make_shared<LccCache>();
        GX_TRY(lcc_orient(g, fresh->O, s));
        // the dense core (GX_LCC_CORE = its largest size, 0 none), before the items are cut:
        // its in-orientation entries carry the dense bit the hash kernels skip
        GX_TRY(lcc_dense_build(g, *fresh, kn.core, s));
        GX_TRY(lcc_items(fresh->O, 0, n, kn, fresh->L, s));
        GX_TRY(fresh->tc.alloc(n));
        GX_TRY(fresh->out.alloc(n));
        g->lcc = fresh;
        C = fresh.get();
        return GX_SUCCESS;
    }

    // Stage 2: the triangle counters, from the hash tiers and the dense core.
    int count() {
        GX_HIP_TRY(hipMemsetAsync(C->tc.p, 0, n * 8, s));
        GX_TRY(lcc_count_items(g, C->O, C->L, C->tc.p, s));
        return lcc_dense_count(g, *C, C->tc.p, s);
    }

    // Stage 3: the quotients.
    int finish() { return lcc_finish(g->S.rp.p, C->tc.p, n, C->out.p, s); }
};

}  // namespace
}  // namespace gx

using namespace gx;

extern "C" int gx_lcc(gx_graph *g, double *lcc) {
    if (!g || !lcc) return fail(GX_NULL_POINTER, "gx_lcc: null argument");
    GX_TRY(lcc_check_size(g->n, "gx_lcc"));
    gx_ctx *ctx = g->ctx;
    GX_HIP_TRY(hipSetDevice(ctx->device));
    if (g->n == 0) return GX_SUCCESS;
    LccCall c(g);
    GX_TRY(device_begin(ctx));
    GX_TRY(c.prep());
    GX_TRY(c.count());
    GX_TRY(c.finish());
    GX_TRY(device_end(ctx));
    GX_TRY(download(ctx, lcc, c.C->out.p, (uint64_t)c.n, Xfer::Raw64));
    return GX_SUCCESS;
}

GX_MODULE_WARMER(lcc)

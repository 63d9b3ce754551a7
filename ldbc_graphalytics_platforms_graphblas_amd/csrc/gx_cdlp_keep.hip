// gx_cdlp_keep.hip -- CDLP's own-label check of a dense active iteration: its kernels, the
// layouts it reads (keep_build, once per graph) and its launches (keep_check).
#include <algorithm>
#include <vector>

#include "gx_cdlp.h"

namespace gx {
namespace {

// ---- own-label check (dense active iterations) ----------------------------------------
// From the third iteration on, a vertex whose own label is held by more than half of its
// neighbours keeps it: that label is then the unique mode (SYN-7_5: every vertex of degree
// > 16 but 17 % passes at the third iteration, all but 0.05 % of the entries at the fourth).
// When an iteration's active set overflowed (*dense), one edge-parallel pass counts, per
// vertex of degree > kTiny, the neighbours holding its label; the vertices that fail go to
// the sparse iteration's activation lists (huge ones are stamped for their tier), tiny ones
// are recomputed by k_cdlp_tiny, and the iteration turns sparse (*dense = 0).  This replaces
// the tier kernels' pass over every vertex (~0.5 ms per dense iteration on SYN-7_5).
//
// Edge-parallel layout of a CSR (built once per graph): bit k of word s says that a
// non-empty row starts at entry 64 s + k, sne[s] is the position in ne (the non-empty rows,
// ascending) of the row that holds entry 64 s.  Lane k of a 64-entry slab then finds its row
// as ne[sne[s] + popcount(bits up to k) - bit 0], without a search.
__global__ __launch_bounds__(256) void k_keep_flags(const int64_t *__restrict__ rp, int64_t n, int64_t *flag) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256)
        flag[v] = rp[v + 1] > rp[v] ? 1 : 0;
}

// ne holds each row with its sign bit set when its degree (out + in) is at most kTiny: those
// are k_cdlp_tiny's, the check skips their entries.
__global__ __launch_bounds__(256) void k_keep_layout(const int64_t *__restrict__ rp, int64_t n,
                                                     const int64_t *__restrict__ nepos, const int64_t *__restrict__ rpA,
                                                     const int64_t *__restrict__ rpT, int32_t *ne,
                                                     unsigned long long *bits, int32_t *sne) {
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        const int64_t b = rp[v], e = rp[v + 1];
        if (e == b) continue;
        const int32_t p = (int32_t)nepos[v];
        ne[p] = cdlp_degree(rpA, rpT, v) > kTiny ? (int32_t)v : (int32_t)((uint32_t)v | 0x80000000u);
        atomicOr(&bits[b >> 6], 1ull << (b & 63));
        for (int64_t sl = (b + kWave - 1) / kWave; sl * kWave < e; sl++) sne[sl] = p;
    }
}

// Counts, for every row of degree > kTiny (out + in degree), the entries of this CSR whose
// label equals the row's own label, into kcnt.  A wave takes kKeepU consecutive 64-entry slabs
// with every load of the chunk issued before the first compare (the chain is bits / sne ->
// ne -> labels), and carries its last row's count across the slabs: one atomic per row and
// chunk.  The first launch of an iteration (A's entries) also records whether the check runs
// (*keep = *dense) and empties the activation lists.
struct alignas(64) KeepW8 {
    unsigned long long w[8];
};
struct alignas(32) KeepS8 {
    int32_t s[8];
};
constexpr int kKeepSlabs = 16;     // k_cdlp_keep_count's kKeepU: slabs per wave and chunk
constexpr int64_t kKeepPad = 32;   // the layout's slabs rounded up to this (a chunk or more)

template <int kKeepU>
__global__ __launch_bounds__(256) void k_cdlp_keep_count(const int32_t *__restrict__ ci, int64_t nnz,
                                                         const unsigned long long *__restrict__ bits,
                                                         const int32_t *__restrict__ sne, const int32_t *__restrict__ ne,
                                                         const int32_t *__restrict__ lab, uint32_t *kcnt,
                                                         const int *dense, int *keep, unsigned int *lcounts, int head) {
    const bool run = *dense != 0;
    if (head && blockIdx.x == 0) {
        if (threadIdx.x == 0) *keep = run ? 1 : 0;
        if (run)
            for (int i = threadIdx.x; i < 3 * kCdlpSubs; i += 256) lcounts[(int64_t)i * kCntStride] = 0u;
    }
    if (!run) return;
    const int lane = threadIdx.x & (kWave - 1);
    // wave-uniform in the compiler's view too: the slab words and row positions are scalar loads
    const int64_t gw = (int64_t)blockIdx.x * (256 / kWave) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t nw = (int64_t)gridDim.x * (256 / kWave);
    const int64_t nslabs = (nnz + kWave - 1) / kWave;
    const int64_t nchunks = (nslabs + kKeepU - 1) / kKeepU;
    const unsigned long long upto = lane == kWave - 1 ? ~0ull : (2ull << lane) - 1ull;
    for (int64_t ch = gw; ch < nchunks; ch += nw) {
        const int64_t sl0 = ch * kKeepU;
        // every load unconditional (clamped indices): predicated loads would each wait in turn.
        // The chunk's slab words and row positions are two wide scalar loads (the layout is
        // padded to whole chunks, zero words past the last slab).
        unsigned long long W[kKeepU];
        int32_t R[kKeepU], Cl[kKeepU], S[kKeepU];
#pragma unroll
        for (int h = 0; h < kKeepU / 8; h++) {
            const KeepW8 wb = *reinterpret_cast<const KeepW8 *>(bits + sl0 + 8 * h);
            const KeepS8 sb = *reinterpret_cast<const KeepS8 *>(sne + sl0 + 8 * h);
#pragma unroll
            for (int i = 0; i < 8; i++) {
                W[8 * h + i] = wb.w[i];
                S[8 * h + i] = sb.s[i];
            }
        }
#pragma unroll
        for (int u = 0; u < kKeepU; u++) Cl[u] = ci[min(sl0 * kWave + u * kWave + lane, nnz - 1)];
#pragma unroll
        for (int u = 0; u < kKeepU; u++) R[u] = ne[S[u] + __popcll(W[u] & upto) - (int)(W[u] & 1ull)];
        uint32_t M = 0, V = 0;   // bit u: lane's entry of slab u is checked / holds the row's own label
#pragma unroll
        for (int u = 0; u < kKeepU; u++) {
            const int32_t x = lab[Cl[u]], y = lab[R[u] & 0x7fffffff];
            const bool valid = (sl0 + u) * kWave + lane < nnz && R[u] >= 0;
            V |= valid ? 1u << u : 0u;
            M |= valid && x == y ? 1u << u : 0u;
        }
        int32_t crow = -1;
        uint32_t ccnt = 0;
#pragma unroll
        for (int u = 0; u < kKeepU; u++) {
            const bool valid = (V >> u) & 1u;
            const int seg = __popcll(W[u] & upto);
            unsigned long long rem = __ballot(valid);
            while (rem) {
                const int lead = __ffsll((long long)rem) - 1;
                const int sg = __builtin_amdgcn_readlane(seg, lead);
                const int32_t r = __builtin_amdgcn_readlane(R[u], lead);
                const bool in = valid && seg == sg;
                const unsigned long long grp = __ballot(in);
                const uint32_t c = (uint32_t)__popcll(__ballot(in && ((M >> u) & 1u)));
                if (r == crow) {
                    ccnt += c;
                } else {
                    if (ccnt && lane == 0) atomicAdd(&kcnt[crow], ccnt);
                    crow = r;
                    ccnt = c;
                }
                rem &= ~grp;
            }
        }
        if (ccnt && lane == 0) atomicAdd(&kcnt[crow], ccnt);
    }
}

// Column-sorted form of the count (the default where built; GX_CDLP_KEEP_SORTED=0: the slabs
// above).  The slab pass is bound by the texture units' line rate: rocprofv3 on SYN-7_5 shows
// TA busy 92 % of the launch for ~59 M L2 requests, one per label gather (its 64 lanes read 64
// different lines).  Here the entries of the rows the check reads are cut into blocks of at
// most kKeepBlock entries and a row span of at most kKeepRows rows, and each block's entries
// are sorted by column (built once per graph): a block's label gathers walk the label array in
// order, so a wave's lanes share lines (hub columns repeat many times per block).  Each entry
// keeps its column (4 B) and its row within the block (2 B); the rows' own labels and counts
// live in LDS, and one global atomic per (block, row) adds the count.
constexpr int64_t kKeepBlock = 65536;   // 32768 .. 1 Mi were measured: DESIGN.md
constexpr int kKeepRows = 1024;

// One wave per included row: the row's entries as (block << 32 | column) keys with the row's
// place in its block as the value (kpos: where the row's keys start; a row of kKeepBlock or
// more entries spans whole blocks of its own, from rblk).
__global__ __launch_bounds__(256) void k_keep_sorted_keys(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                          const int32_t *__restrict__ rows, const int64_t *__restrict__ kpos,
                                                          const int32_t *__restrict__ rblk,
                                                          const int32_t *__restrict__ brow0, int64_t nrows,
                                                          int64_t kKeepBlock, uint64_t *keys, uint16_t *vals) {
    const int lane = threadIdx.x & (kWave - 1);
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) / kWave; i < nrows;
         i += (int64_t)gridDim.x * (256 / kWave)) {
        const int64_t r = rows[i], b0 = rp[r], d = rp[r + 1] - b0;
        for (int64_t k = lane; k < d; k += kWave) {
            const int64_t b = d >= kKeepBlock ? rblk[i] + k / kKeepBlock : rblk[i];
            keys[kpos[i] + k] = ((uint64_t)b << 32) | (uint32_t)ci[b0 + k];
            vals[kpos[i] + k] = (uint16_t)(r - brow0[b]);
        }
    }
}

__global__ void k_keep_sorted_cols(const uint64_t *__restrict__ keys, int64_t m, int32_t *cols) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x)
        cols[i] = (int32_t)(uint32_t)keys[i];
}

__global__ __launch_bounds__(256) void k_cdlp_keep_sorted(const int64_t *__restrict__ bstart,
                                                          const int32_t *__restrict__ brow0, int64_t nb,
                                                          const int32_t *__restrict__ scol,
                                                          const uint16_t *__restrict__ srow,
                                                          const int32_t *__restrict__ lab, int64_t n, uint32_t *kcnt,
                                                          const int *dense, int *keep, unsigned int *lcounts, int head) {
    const bool run = *dense != 0;
    if (head && blockIdx.x == 0) {
        if (threadIdx.x == 0) *keep = run ? 1 : 0;
        if (run)
            for (int i = threadIdx.x; i < 3 * kCdlpSubs; i += 256) lcounts[(int64_t)i * kCntStride] = 0u;
    }
    if (!run) return;
    __shared__ int32_t own[kKeepRows];
    __shared__ uint32_t cnt[kKeepRows];
    const int tid = threadIdx.x;
    for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const int64_t r0 = brow0[b], e0 = bstart[b], e1 = bstart[b + 1];
        const int span = (int)min((int64_t)kKeepRows, n - r0);
        for (int i = tid; i < span; i += 256) {
            own[i] = lab[r0 + i];
            cnt[i] = 0u;
        }
        __syncthreads();
        // rounds of U entries per thread, software-pipelined: a round's label gathers are issued,
        // then the next round's columns and rows, then the compares wait for the gathers only
        constexpr int U = 8;
        int32_t c[U];
        uint32_t lr[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t k = min(e0 + tid + (int64_t)u * 256, e1 - 1);
            c[u] = scol[k];
            lr[u] = srow[k];
        }
        for (int64_t e = e0 + tid; e < e1; e += 256 * U) {
            int32_t x[U];
#pragma unroll
            for (int u = 0; u < U; u++) x[u] = lab[c[u]];
            int32_t cn[U];
            uint32_t ln[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int64_t k = min(e + (int64_t)(U + u) * 256, e1 - 1);
                cn[u] = scol[k];
                ln[u] = srow[k];
            }
#pragma unroll
            for (int u = 0; u < U; u++)
                if (e + (int64_t)u * 256 < e1 && x[u] == own[lr[u]]) atomicAdd(&cnt[lr[u]], 1u);
#pragma unroll
            for (int u = 0; u < U; u++) {
                c[u] = cn[u];
                lr[u] = ln[u];
            }
        }
        __syncthreads();
        for (int i = tid; i < span; i += 256)
            if (cnt[i]) atomicAdd(&kcnt[r0 + i], cnt[i]);
        __syncthreads();   // own / cnt are free for the next block
    }
}

// Per vertex of degree > kTiny: keep (2 count > degree) or recompute: onto the activation list
// of its degree (the sparse kernels' lists, shard = wave index mod kCdlpSubs), or, huge, the
// iteration's stamp for the huge tier (a kept huge vertex loses a stamp k_cdlp_mark gave it).
// kcnt is left zero.  A full list sets *kover.
__global__ __launch_bounds__(256) void k_cdlp_keep_apply(const int64_t *__restrict__ rpA, const int64_t *__restrict__ rpT,
                                                         int64_t v0, int64_t v1, uint32_t *kcnt, int32_t *act,
                                                         int32_t stamp, const int *keep, unsigned int *counts,
                                                         int32_t *al, int64_t asub, int *kover, int32_t *vlb,
                                                         int32_t *vchg) {
    if (*keep == 0) return;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t gw = ((int64_t)blockIdx.x * 256 + threadIdx.x) / kWave;
    const int64_t nw = (int64_t)gridDim.x * (256 / kWave);
    const int j = (int)(gw % kCdlpSubs);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t b = v0 + gw * kWave; b < v1; b += nw * kWave) {
        const int64_t v = b + lane;
        int L = -1;
        if (v < v1) {
            const int64_t d = cdlp_degree(rpA, rpT, v);
            if (d > kTiny) {
                const uint32_t c = kcnt[v];
                if (c) kcnt[v] = 0u;
                const bool kept = 2 * (int64_t)c > d;
                if (kept && vlb) {   // the recount bound: the own label's exact count
                    vlb[v] = (int32_t)c;
                    vchg[v] = 0;
                }
                if (d > kMidMax) {
                    if (!kept) act[v] = stamp;
                    else if (act[v] == stamp) act[v] = stamp - 1;

                } else if (!kept) {
                    L = d <= kSparseWaveMax ? 0 : d <= kSparseG2Max ? 1 : 2;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const unsigned long long m = __ballot(L == q);
            if (!m) continue;
            unsigned int base = 0;
            if (lane == 0) base = atomicAdd(&counts[((1 + q) * kCdlpSubs + j) * kCntStride], (unsigned int)__popcll(m));
            base = __shfl(base, 0, kWave);
            if (L == q) {
                const unsigned int idx = base + (unsigned int)__popcll(m & below);
                if (idx < (unsigned int)asub) al[((int64_t)q * kCdlpSubs + j) * asub + idx] = (int32_t)v;
                else *kover = 1;
            }
        }
    }
}

// The check's outcome: lists that fit make the iteration sparse; a full one leaves it dense
// (every tier kernel recomputes every vertex, as without the check).
__global__ void k_cdlp_keep_finish(int *dense, int *keep, int *kover) {
    if (*keep) {
        if (*kover) *keep = 0;
        else *dense = 0;
    }
    *kover = 0;
}

// The own-label check's layout of one CSR (k_keep_layout).
int keep_layout(const int64_t *rp, int64_t n, int64_t nnz, const int64_t *rpA, const int64_t *rpT, KeepCsr &K,
                hipStream_t s) {
    const int64_t nslabs = (nnz + kWave - 1) / kWave;
    const size_t padded = (size_t)((nslabs + kKeepPad - 1) / kKeepPad * kKeepPad + kKeepPad);
    GX_TRY(K.bits.alloc(padded));
    GX_TRY(K.sne.alloc(padded));
    GX_TRY(K.ne.alloc((size_t)std::max<int64_t>(n, 1)));
    GX_HIP_TRY(hipMemsetAsync(K.bits.p, 0, padded * 8, s));
    GX_HIP_TRY(hipMemsetAsync(K.sne.p, 0, padded * 4, s));
    GX_HIP_TRY(hipMemsetAsync(K.ne.p, 0, (size_t)std::max<int64_t>(n, 1) * 4, s));
    if (n == 0 || nnz == 0) return GX_SUCCESS;
    DBuf<int64_t> flag, pos;
    GX_TRY(flag.alloc(n));
    GX_TRY(pos.alloc(n));
    hipLaunchKernelGGL(k_keep_flags, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, rp, n, flag.p);
    GX_TRY(check_launch("k_keep_flags"));
    GX_TRY(scan_exclusive_i64(flag.p, pos.p, (size_t)n, s));
    hipLaunchKernelGGL(k_keep_layout, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, rp, n, pos.p, rpA, rpT, K.ne.p,
                       K.bits.p, K.sne.p);
    GX_TRY(check_launch("k_keep_layout"));
    GX_HIP_TRY(hipStreamSynchronize(s));   // flag / pos die at return
    return GX_SUCCESS;
}

// The column-sorted blocks of one CSR (host row pointers h_rp, device rp / ci): the rows of
// total degree > kTiny in order, cut greedily into blocks of <= kKeepBlock entries whose rows
// span <= kKeepRows positions (a row of kKeepBlock or more entries takes whole blocks of its own).
int keep_sorted_build(const CdlpGraph &G, const int64_t *h_rp, const int64_t *rp, const int32_t *ci,
                      KeepCsr &K, hipStream_t s) {
    std::vector<int32_t> rows, rblk, brow0;
    std::vector<int64_t> kpos, bsize;
    int64_t m = 0, cur_e = 0;
    bool open = false;
    for (int64_t v = 0; v < G.n; v++) {
        const int64_t dt = (G.h_rpA[v + 1] - G.h_rpA[v]) + (G.directed ? G.h_rpT[v + 1] - G.h_rpT[v] : 0);
        const int64_t d = h_rp[v + 1] - h_rp[v];
        if (dt <= kTiny || d == 0) continue;
        if (d >= kKeepBlock) {
            rows.push_back((int32_t)v);
            kpos.push_back(m);
            rblk.push_back((int32_t)brow0.size());
            for (int64_t k = 0; k < d; k += kKeepBlock) {
                brow0.push_back((int32_t)v);
                bsize.push_back(std::min(kKeepBlock, d - k));
            }
            m += d;
            open = false;
            continue;
        }
        if (!open || cur_e + d > kKeepBlock || v - brow0.back() >= kKeepRows) {
            brow0.push_back((int32_t)v);
            bsize.push_back(0);
            cur_e = 0;
            open = true;
        }
        rows.push_back((int32_t)v);
        kpos.push_back(m);
        rblk.push_back((int32_t)brow0.size() - 1);
        bsize.back() += d;
        cur_e += d;
        m += d;
    }
    K.nb = (int64_t)brow0.size();
    if (m == 0 || K.nb >= (1ll << 31)) {
        K.nb = 0;
        return GX_SUCCESS;
    }
    std::vector<int64_t> bstart(brow0.size() + 1, 0);
    for (size_t b = 0; b < bsize.size(); b++) bstart[b + 1] = bstart[b] + bsize[b];

    DBuf<int32_t> d_rows, d_rblk;
    DBuf<int64_t> d_kpos;
    DBuf<uint64_t> keys, keys2;
    DBuf<uint16_t> vals;
    GX_TRY(d_rows.alloc(rows.size()));
    GX_TRY(d_rblk.alloc(rblk.size()));
    GX_TRY(d_kpos.alloc(kpos.size()));
    GX_TRY(K.brow0.alloc(brow0.size()));
    GX_TRY(K.bstart.alloc(bstart.size()));
    GX_HIP_TRY(hipMemcpyAsync(d_rows.p, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, s));
    GX_HIP_TRY(hipMemcpyAsync(d_rblk.p, rblk.data(), rblk.size() * 4, hipMemcpyHostToDevice, s));
    GX_HIP_TRY(hipMemcpyAsync(d_kpos.p, kpos.data(), kpos.size() * 8, hipMemcpyHostToDevice, s));
    GX_HIP_TRY(hipMemcpyAsync(K.brow0.p, brow0.data(), brow0.size() * 4, hipMemcpyHostToDevice, s));
    GX_HIP_TRY(hipMemcpyAsync(K.bstart.p, bstart.data(), bstart.size() * 8, hipMemcpyHostToDevice, s));
    GX_TRY(keys.alloc((size_t)m));
    GX_TRY(keys2.alloc((size_t)m));
    GX_TRY(vals.alloc((size_t)m));
    GX_TRY(K.srow.alloc((size_t)m));
    hipLaunchKernelGGL(k_keep_sorted_keys, dim3(grid_for((uint64_t)rows.size() * kWave, 256, 16384)), dim3(256), 0, s,
                       rp, ci, d_rows.p, d_kpos.p, d_rblk.p, K.brow0.p, (int64_t)rows.size(), kKeepBlock, keys.p,
                       vals.p);
    GX_TRY(check_launch("k_keep_sorted_keys"));
    int end_bit = 32;
    while ((1ll << (end_bit - 32)) < K.nb) end_bit++;
    GX_TRY(sort_pairs_u64_u16(keys.p, keys2.p, vals.p, K.srow.p, (size_t)m, end_bit, s));
    keys.release();
    vals.release();
    GX_TRY(K.scol.alloc((size_t)m));
    hipLaunchKernelGGL(k_keep_sorted_cols, dim3(grid_for((uint64_t)m, 256, 8192)), dim3(256), 0, s, keys2.p, m, K.scol.p);
    GX_TRY(check_launch("k_keep_sorted_cols"));
    GX_HIP_TRY(hipStreamSynchronize(s));   // host vectors and the key buffers die at return
    return GX_SUCCESS;
}

}  // namespace

int keep_build(const CdlpGraph &G, bool relabel, CdlpKeep &K, hipStream_t s) {
    // the sorted blocks cost a device sort of the entries (~7 ms on SYN-7_5) and save ~0.1 ms
    // per call: built with the relabelled copy, i.e. once the graph serves a second CDLP run
    // The layout half of GX_CDLP_KEEP_SORTED is read here, when the layouts are built, and not
    // again: a later call can only choose between the layouts this one built (keep_check's `sorted`).
    if (relabel && G.h_rpA && (!G.directed || G.h_rpT) && env_on("GX_CDLP_KEEP_SORTED")) {
        GX_TRY(keep_sorted_build(G, G.h_rpA, G.rpA, G.ciA, K.A, s));
        if (G.directed) GX_TRY(keep_sorted_build(G, G.h_rpT, G.rpT, G.ciT, K.T, s));
        K.sorted = true;
    }
    GX_TRY(keep_layout(G.rpA, G.n, G.nnzA, G.rpA, G.rpT, K.A, s));
    if (G.directed) GX_TRY(keep_layout(G.rpT, G.n, G.nnzT, G.rpA, G.rpT, K.T, s));
    GX_TRY(K.kcnt.alloc((size_t)std::max<int64_t>(G.n, 1)));
    GX_HIP_TRY(hipMemsetAsync(K.kcnt.p, 0, (size_t)std::max<int64_t>(G.n, 1) * 4, s));
    GX_TRY(K.kflags.alloc(2));
    GX_HIP_TRY(hipMemsetAsync(K.kflags.p, 0, 2 * sizeof(int), s));
    K.nnzA = G.nnzA;
    K.nnzT = G.directed ? G.nnzT : 0;
    if (relabel && G.h_rpA && (!G.directed || G.h_rpT)) {
        auto deg = [&](int64_t i) {
            return (G.h_rpA[i + 1] - G.h_rpA[i]) + (G.directed ? G.h_rpT[i + 1] - G.h_rpT[i] : 0);
        };
        int64_t lo = 0, hi = G.n;   // the first position of degree <= kTiny (degrees non-increasing)
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (deg(mid) > kTiny) lo = mid + 1;
            else hi = mid;
        }
        K.nnzA = G.h_rpA[lo];
        if (G.directed) K.nnzT = G.h_rpT[lo];
    }
    K.built = true;
    return GX_SUCCESS;
}

int keep_check(const CdlpGraph &G, CdlpKeep &K, bool sorted, const int32_t *cur, int *dense, int32_t *act, int32_t it,
               unsigned int *lists, int32_t *al, int64_t asub, const CdlpBound *bd, hipStream_t s) {
    KTimer kk(G.ctx, "cdlp_keep", s);
    int *kf = K.kflags.p;
    // counts of the own label among each vertex's neighbours (the kernels exit unless *dense):
    // A's entries, whose launch is the head, then A''s
    for (int t = 0; t < (G.directed ? 2 : 1); t++) {
        const KeepCsr &L = t ? K.T : K.A;
        const int64_t nnz = t ? K.nnzT : K.nnzA, per = (int64_t)kWave * kKeepSlabs;   // one wave per kKeepSlabs slabs
        if (K.sorted && sorted) {
            const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(L.nb, 65536));
            hipLaunchKernelGGL(k_cdlp_keep_sorted, dim3(grid), dim3(256), 0, s, L.bstart.p, L.brow0.p, L.nb, L.scol.p,
                               L.srow.p, cur, G.n, K.kcnt.p, dense, kf, lists + kCdlpSubs * kCntStride, t == 0);
            GX_TRY(check_launch("k_cdlp_keep_sorted"));
        } else {
            const unsigned grid = grid_for((uint64_t)std::max<int64_t>(1, (nnz + per - 1) / per) * kWave, 256, 16384);
            hipLaunchKernelGGL(k_cdlp_keep_count<kKeepSlabs>, dim3(grid), dim3(256), 0, s, t ? G.ciT : G.ciA, nnz,
                               L.bits.p, L.sne.p, L.ne.p, cur, K.kcnt.p, dense, kf, lists + kCdlpSubs * kCntStride,
                               t == 0);
            GX_TRY(check_launch("k_cdlp_keep_count"));
        }
    }
    hipLaunchKernelGGL(k_cdlp_keep_apply, dim3(8 * kCdlpSubs), dim3(256), 0, s, G.rpA, G.rpT, (int64_t)0, G.n, K.kcnt.p,
                       act, it, kf, lists, al, asub, kf + 1, bd ? bd->vlb : nullptr, bd ? bd->vchg : nullptr);
    GX_TRY(check_launch("k_cdlp_keep_apply"));
    hipLaunchKernelGGL(k_cdlp_keep_finish, dim3(1), dim3(1), 0, s, dense, kf, kf + 1);
    GX_TRY(check_launch("k_cdlp_keep_finish"));
    return GX_SUCCESS;
}

}  // namespace gx

GX_MODULE_WARMER(cdlp_keep)

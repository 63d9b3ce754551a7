// gx_lcc_orient.hip -- LCC's degree-ordered orientation O of the closure S and its transpose I
// (lcc_orient; gx_lcc.hip has the algorithm).
//   orientation : stream compaction of S by 64-entry slabs (ballot masks + one scan);
//   transpose   : I = O^T by a radix sort of (x, v) keys on x only.
#include <cstring>   // rocprim's headers call memset

#include <rocprim/rocprim.hpp>

#include "gx_lcc.h"

namespace gx {
namespace {

__device__ __forceinline__ bool ranks_above(int64_t du, int32_t u, int64_t dv, int32_t v) {
    return du > dv || (du == dv && u > v);
}

// ---- orientation by slab compaction (one wave per 64-entry slab of S, lane = entry) ----
__global__ __launch_bounds__(kLccBlock) void k_orient_masks(const int64_t *__restrict__ rp,
                                                            const int32_t *__restrict__ ci,
                                                            const int64_t *__restrict__ srow, int64_t n, int64_t nnz,
                                                            int64_t nslabs, uint64_t *mask, int32_t *cnt) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t nw = (int64_t)gridDim.x * kWavesPerBlock;
    for (int64_t sl = ((int64_t)blockIdx.x * kLccBlock + threadIdx.x) / kWave; sl < nslabs; sl += nw) {
        const int64_t e0 = sl * kWave, e_last = min(e0 + kWave, nnz) - 1;
        const int64_t e = e0 + lane;
        const bool valid = e < nnz;
        const int64_t ee = valid ? e : e_last;
        const int64_t v = slab_row_of(rp, srow, n, sl, ee, lane);
        const int32_t u = ci[ee];
        const bool keep = valid && ranks_above(rp[u + 1] - rp[u], u, rp[v + 1] - rp[v], (int32_t)v);
        const uint64_t m = __ballot(keep);
        if (lane == 0) {
            mask[sl] = m;
            cnt[sl] = __popcll(m);
        }
    }
}

__device__ __forceinline__ int64_t kept_before(const uint64_t *mask, const int64_t *cpre, int64_t e) {
    const int64_t sl = e / kWave;
    const int b = (int)(e % kWave);
    return cpre[sl] + (b ? __popcll(mask[sl] & ((1ull << b) - 1)) : 0);
}

__global__ void k_orient_rows(const int64_t *__restrict__ rp, const uint64_t *__restrict__ mask,
                              const int64_t *__restrict__ cpre, int64_t n, int64_t *orp) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v <= n; v += (int64_t)gridDim.x * blockDim.x)
        orp[v] = kept_before(mask, cpre, rp[v]);
}

// Oriented entries are packed as (x << 2) | popcount(flag): one 4-byte load per probe.
__global__ __launch_bounds__(kLccBlock) void k_orient_scatter(const int32_t *__restrict__ ci,
                                                              const uint8_t *__restrict__ fl, int64_t nnz,
                                                              const uint64_t *__restrict__ mask,
                                                              const int64_t *__restrict__ cpre, uint32_t *ocode) {
    for (int64_t e = (int64_t)blockIdx.x * kLccBlock + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kLccBlock) {
        const int64_t sl = e / kWave;
        const int b = (int)(e % kWave);
        const uint64_t m = mask[sl];
        if ((m >> b) & 1ull) {
            const int64_t pos = cpre[sl] + (b ? __popcll(m & ((1ull << b) - 1)) : 0);
            ocode[pos] = ((uint32_t)ci[e] << 2) | (uint32_t)__popc(fl[e]);
        }
    }
}

// In-orientation I (transpose of O): keys (x << 32) | (v << 2 | p) for every v -> x.
__global__ void k_orient_tkeys(const int64_t *__restrict__ orp, const uint32_t *__restrict__ ocode, int64_t n,
                               uint64_t *keys) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x)
        for (int64_t k = orp[v]; k < orp[v + 1]; k++) {
            const uint32_t c = ocode[k];
            keys[k] = ((uint64_t)(c >> 2) << 32) | (((uint32_t)v << 2) | (c & 3u));
        }
}

__global__ void k_keys_to_in_csr(const uint64_t *__restrict__ keys, int64_t m, int64_t n, int64_t *irp,
                                 uint32_t *icode) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t <= n) {
        const uint64_t target = (uint64_t)t << 32;
        int64_t lo = 0, hi = m;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (keys[mid] < target) lo = mid + 1;
            else hi = mid;
        }
        irp[t] = lo;
    }
    for (int64_t k = t; k < m; k += (int64_t)gridDim.x * blockDim.x) icode[k] = (uint32_t)(keys[k] & 0xffffffffu);
}

}  // namespace

int lcc_orient(gx_graph *g, LccOrient &O, hipStream_t s) {
    gx_ctx *ctx = g->ctx;
    const int64_t n = (int64_t)g->n;
    const DevCSR &S = g->S;
    const int64_t nnz = (int64_t)S.h_rp[n];
    const int64_t nslabs = (nnz + kWave - 1) / kWave;
    DBuf<uint64_t> mask;
    DBuf<int32_t> cnt;
    DBuf<int64_t> cpre;
    GX_TRY(mask.alloc(nslabs + 1));
    GX_TRY(cnt.alloc(nslabs + 1));
    GX_TRY(cpre.alloc(nslabs + 1));
    GX_TRY(O.orp.alloc(n + 1));
    GX_TRY(O.irp.alloc(n + 1));
    DBuf<int64_t> srow;
    GX_TRY(srow.alloc(nslabs + 1));
    GX_HIP_TRY(hipMemsetAsync(cnt.p + nslabs, 0, sizeof(int32_t), s));
    GX_HIP_TRY(hipMemsetAsync(mask.p + nslabs, 0, sizeof(uint64_t), s));
    KTimer kt(ctx, "lcc_orient", s);
    GX_TRY(slab_rows(S.rp.p, n, nslabs, srow.p, s));
    if (nslabs)
        hipLaunchKernelGGL(k_orient_masks, dim3(grid_for((uint64_t)nslabs * kWave, kLccBlock, 16384)), dim3(kLccBlock),
                           0, s, S.rp.p, S.ci.p, srow.p, n, nnz, nslabs, mask.p, cnt.p);
    GX_TRY(check_launch("k_orient_masks"));
    size_t tmp_bytes = 0;
    GX_HIP_TRY(rocprim::exclusive_scan(nullptr, tmp_bytes, cnt.p, cpre.p, (int64_t)0, (size_t)(nslabs + 1),
                                       rocprim::plus<int64_t>(), s));
    DBuf<char> tmp;
    GX_TRY(tmp.alloc(tmp_bytes));
    GX_HIP_TRY(rocprim::exclusive_scan(tmp.p, tmp_bytes, cnt.p, cpre.p, (int64_t)0, (size_t)(nslabs + 1),
                                       rocprim::plus<int64_t>(), s));
    hipLaunchKernelGGL(k_orient_rows, dim3(grid_for(n + 1, 256, 16384)), dim3(256), 0, s, S.rp.p, mask.p, cpre.p, n,
                       O.orp.p);
    GX_TRY(check_launch("k_orient_rows"));
    GX_HIP_TRY(hipMemcpyAsync(&O.m, O.orp.p + n, 8, hipMemcpyDeviceToHost, s));
    GX_HIP_TRY(hipStreamSynchronize(s));
    GX_TRY(O.ocode.alloc(O.m, 16));
    GX_TRY(O.icode.alloc(O.m, 16));
    if (nnz)
        hipLaunchKernelGGL(k_orient_scatter, dim3(grid_for(nnz, kLccBlock, 16384)), dim3(kLccBlock), 0, s, S.ci.p,
                           S.flag.p, nnz, mask.p, cpre.p, O.ocode.p);
    GX_TRY(check_launch("k_orient_scatter"));
    // transpose: sort (x, v|p) keys by x only (bits 32 .. 32+log2 n), then row pointers
    DBuf<uint64_t> k0, k1;
    GX_TRY(k0.alloc(O.m + 1));
    GX_TRY(k1.alloc(O.m + 1));
    if (O.m) {
        hipLaunchKernelGGL(k_orient_tkeys, dim3(grid_for(n, 256, 16384)), dim3(256), 0, s, O.orp.p, O.ocode.p, n,
                           k0.p);
        GX_TRY(check_launch("k_orient_tkeys"));
        int hb = 1;
        while ((1ll << hb) <= n) hb++;
        size_t sbytes = 0;
        GX_HIP_TRY(rocprim::radix_sort_keys(nullptr, sbytes, k0.p, k1.p, (size_t)O.m, 32, 32 + hb, s));
        DBuf<char> stmp;
        GX_TRY(stmp.alloc(sbytes));
        GX_HIP_TRY(rocprim::radix_sort_keys(stmp.p, sbytes, k0.p, k1.p, (size_t)O.m, 32, 32 + hb, s));
        GX_HIP_TRY(hipStreamSynchronize(s));   // stmp is freed at scope end
    }
    hipLaunchKernelGGL(k_keys_to_in_csr, dim3(grid_for((uint64_t)n + 1, 256, 1u << 30)), dim3(256), 0, s, k1.p, O.m, n,
                       O.irp.p, O.icode.p);
    GX_TRY(check_launch("k_keys_to_in_csr"));
    GX_HIP_TRY(hipStreamSynchronize(s));   // the temporaries are freed on return
    return GX_SUCCESS;
}

}  // namespace gx

GX_MODULE_WARMER(lcc_orient)

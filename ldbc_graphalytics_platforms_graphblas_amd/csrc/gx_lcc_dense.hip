// gx_lcc_dense.hip -- LCC's dense core on the matrix cores (lcc_dense_build, lcc_dense_count;
// gx_lcc.hip has the algorithm).
//
// The vertices of closure degree > dcut (the top of the orientation order, so every triangle
// whose lowest-ranked vertex is in the core lies wholly in it) form a small, dense K x K block
// of S: on SYN-cit the 4 K highest-degree vertices hold 15.5 % of the hash kernels' probe work
// at 9 % density, the 8 K highest 34 % at 5 % (tools/dense_tiles.py).  Its
// triangles are counted as a masked dense product: with W[j][k] the number of stored directions
// between core vertices j and k (0, 1, 2) and B = (W > 0),
//     t(i) = 1/2 sum_j B[i][j] (W B)[j][i],
// each core triangle {i, j, k} adding w(j, k) at i, as the hash kernels do.  W B is an int8
// GEMM on v_mfma_i32_32x32x32_i8 (exact int32 sums), the mask and the row sums fused into its
// epilogue, 64 x 64 output tiles whose mask is empty skipped.  The hash kernels skip the
// in-neighbours v in the core (dense bit of the in-orientation entry), i.e. exactly the core's
// triangles.
#include "gx_lcc.h"

namespace gx {
namespace {

constexpr int kDenseWG = 128;   // output tile of a workgroup (4 waves of 64 x 64)

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
typedef int32_t i32x16 __attribute__((ext_vector_type(16)));

// closure degree and id of every vertex (a stable descending sort of the degrees follows)
__global__ void k_lcc_dense_degkeys(const int64_t *__restrict__ srp, int64_t n, uint32_t *__restrict__ deg,
                                    int32_t *__restrict__ ids) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        deg[v] = (uint32_t)(srp[v + 1] - srp[v]);
        ids[v] = (int32_t)v;
    }
}

// core index of the first K vertices of the degree-descending order (coreidx pre-filled -1)
__global__ void k_lcc_dense_place(const int32_t *__restrict__ sorted_ids, int32_t K, int32_t *__restrict__ coreidx,
                                  int32_t *__restrict__ corev) {
    for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < K; i += gridDim.x * blockDim.x) {
        const int32_t v = sorted_ids[i];
        coreidx[v] = i;
        corev[i] = v;
    }
}

// W and B rows of the core (one wave per core vertex), and the 64 x 64 tiles holding entries
__global__ __launch_bounds__(256) void k_lcc_dense_fill(const int64_t *__restrict__ srp,
                                                        const int32_t *__restrict__ sci,
                                                        const uint8_t *__restrict__ sflag,
                                                        const int32_t *__restrict__ coreidx,
                                                        const int32_t *__restrict__ corev, int32_t K, int32_t Kp,
                                                        int8_t *__restrict__ W, int8_t *__restrict__ B,
                                                        uint8_t *__restrict__ tmask) {
    const int lane = threadIdx.x & (kWave - 1);
    const int32_t nt = Kp / 64;
    for (int32_t i = (blockIdx.x * 256 + threadIdx.x) / kWave; i < K; i += gridDim.x * 256 / kWave) {
        const int32_t v = corev[i];
        for (int64_t e = srp[v] + lane; e < srp[v + 1]; e += kWave) {
            const int32_t c = coreidx[sci[e]];
            if (c < 0) continue;
            W[(int64_t)i * Kp + c] = (int8_t)__popc((uint32_t)sflag[e]);
            B[(int64_t)i * Kp + c] = 1;
            tmask[(i / 64) * nt + c / 64] = 1;
        }
    }
}

// the dense bit on every in-orientation entry whose source v is in the core
__global__ void k_lcc_dense_mark_in(uint32_t *__restrict__ icode, int64_t m, const int32_t *__restrict__ coreidx) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t ic = icode[k];
        if (coreidx[(ic >> 2) & kVMask] >= 0) icode[k] = ic | kDenseBit;
    }
}

// P = W B over 128 x 128 workgroup tiles, each wave 64 x 64 (2 x 2 MFMA tiles of 32 x 32, k
// steps of 32), then t(i) += sum_j B[j][i] P[j][i] over the tile's rows j.  W and B are
// symmetric, row-major Kp x Kp int8: the A operand (rows j) and the B operand (column i = row
// i of B) are both 16 contiguous bytes per lane (lane l: row l & 31, k = 16 (l >> 5) + 0..15).
// C/D: column lane & 31, row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
__global__ __launch_bounds__(256) void k_lcc_dense_mfma(const int8_t *__restrict__ W, const int8_t *__restrict__ B,
                                                        const uint8_t *__restrict__ tmask, int32_t Kp,
                                                        unsigned long long *__restrict__ tcore) {
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int32_t nwg = Kp / kDenseWG;
    const int32_t J0 = (int32_t)(blockIdx.x / nwg) * kDenseWG + (wv >> 1) * 64;
    const int32_t I0 = (int32_t)(blockIdx.x % nwg) * kDenseWG + (wv & 1) * 64;
    if (!tmask[(J0 / 64) * (Kp / 64) + I0 / 64]) return;   // B[j][i] = 0 over the tile: nothing to add
    const int r = lane & 31, h = lane >> 5;
    const int8_t *a0 = W + (int64_t)(J0 + r) * Kp + 16 * h, *a1 = a0 + (int64_t)32 * Kp;
    const int8_t *b0 = B + (int64_t)(I0 + r) * Kp + 16 * h, *b1 = b0 + (int64_t)32 * Kp;
    i32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int q = 0; q < 16; q++) acc[m][n][q] = 0;
    i32x4 fa0 = *reinterpret_cast<const i32x4 *>(a0), fa1 = *reinterpret_cast<const i32x4 *>(a1);
    i32x4 fb0 = *reinterpret_cast<const i32x4 *>(b0), fb1 = *reinterpret_cast<const i32x4 *>(b1);
    for (int32_t k = 32; k <= Kp; k += 32) {
        i32x4 na0, na1, nb0, nb1;
        if (k < Kp) {   // the next k step's fragments, in flight while this one multiplies
            na0 = *reinterpret_cast<const i32x4 *>(a0 + k);
            na1 = *reinterpret_cast<const i32x4 *>(a1 + k);
            nb0 = *reinterpret_cast<const i32x4 *>(b0 + k);
            nb1 = *reinterpret_cast<const i32x4 *>(b1 + k);
        }
        acc[0][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa0, fb0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa0, fb1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa1, fb0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa1, fb1, acc[1][1], 0, 0, 0);
        if (k < Kp) {
            fa0 = na0;
            fa1 = na1;
            fb0 = nb0;
            fb1 = nb1;
        }
    }
    // epilogue: lane's column i = I0 + 32 n + r; its rows j = J0 + 32 m + 8 g + 4 h + (0..3);
    // the mask B[j][i] = B[i][j] (symmetric): four contiguous bytes of row i per (m, g)
#pragma unroll
    for (int n = 0; n < 2; n++) {
        const int32_t i = I0 + 32 * n + r;
        const int8_t *brow = B + (int64_t)i * Kp;
        int64_t s = 0;
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const uint32_t mk = *reinterpret_cast<const uint32_t *>(brow + J0 + 32 * m + 8 * g + 4 * h);
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if ((mk >> (8 * q)) & 0xffu) s += acc[m][n][4 * g + q];
            }
        s += __shfl_xor(s, 32, kWave);
        if (h == 0 && s) atomicAdd(&tcore[i], (unsigned long long)s);
    }
}

// tc[corev[i]] += tcore[i] / 2 (each core pair (j, k) came in both orders)
__global__ void k_lcc_dense_final(const unsigned long long *__restrict__ tcore, const int32_t *__restrict__ corev,
                                  int32_t K, unsigned long long *__restrict__ tc) {
    for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < K; i += gridDim.x * blockDim.x)
        if (tcore[i]) atomicAdd(&tc[corev[i]], tcore[i] / 2);
}

}  // namespace

// The dense core of gx_lcc (k_lcc_dense_mfma): the vertices of closure degree above the
// (kmax + 1)-th largest degree, at most kmax of them; their W / B rows and tile mask, and the
// dense bit on the in-orientation entries.  Built once with the cached orientation.
int lcc_dense_build(gx_graph *g, LccCache &C, int32_t kmax, hipStream_t s) {
    const int64_t n = (int64_t)g->n;
    const DevCSR &S = g->S;
    if (kmax <= 0 || n <= kmax) return GX_SUCCESS;
    int32_t K = 0;
    {
        DBuf<uint32_t> d0, d1;
        DBuf<int32_t> i0, i1;
        GX_TRY(d0.alloc(n));
        GX_TRY(d1.alloc(n));
        GX_TRY(i0.alloc(n));
        GX_TRY(i1.alloc(n));
        hipLaunchKernelGGL(k_lcc_dense_degkeys, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, S.rp.p, n, d0.p, i0.p);
        GX_TRY(check_launch("k_lcc_dense_degkeys"));
        GX_TRY(sort_pairs_desc_u32_i32(d0.p, d1.p, i0.p, i1.p, (size_t)n, s));
        std::vector<uint32_t> top((size_t)kmax + 1);
        GX_HIP_TRY(hipMemcpyAsync(top.data(), d1.p, top.size() * 4, hipMemcpyDeviceToHost, s));
        GX_HIP_TRY(hipStreamSynchronize(s));
        const uint32_t dcut = top[(size_t)kmax];
        while (K < kmax && top[(size_t)K] > dcut) K++;   // every vertex of degree > dcut: upward closed
        if (K < kDenseWG) return GX_SUCCESS;
        C.K = K;
        C.Kp = (K + kDenseWG - 1) / kDenseWG * kDenseWG;
        GX_TRY(C.coreidx.alloc(n));
        GX_TRY(C.corev.alloc(K));
        GX_HIP_TRY(hipMemsetAsync(C.coreidx.p, 0xff, n * 4, s));
        hipLaunchKernelGGL(k_lcc_dense_place, dim3(grid_for(K, 256, 1024)), dim3(256), 0, s, i1.p, K, C.coreidx.p,
                           C.corev.p);
        GX_TRY(check_launch("k_lcc_dense_place"));
        GX_HIP_TRY(hipStreamSynchronize(s));   // the sort buffers are freed at the end of the block
    }
    const int64_t kp = C.Kp, nt = kp / 64;
    GX_TRY(C.W.alloc(kp * kp, 16));
    GX_TRY(C.B.alloc(kp * kp, 16));
    GX_TRY(C.tmask.alloc(nt * nt));
    GX_TRY(C.tcore.alloc(kp));
    GX_HIP_TRY(hipMemsetAsync(C.W.p, 0, kp * kp, s));
    GX_HIP_TRY(hipMemsetAsync(C.B.p, 0, kp * kp, s));
    GX_HIP_TRY(hipMemsetAsync(C.tmask.p, 0, nt * nt, s));
    hipLaunchKernelGGL(k_lcc_dense_fill, dim3(grid_for((uint64_t)K * kWave, 256, 8192)), dim3(256), 0, s, S.rp.p,
                       S.ci.p, S.flag.p, C.coreidx.p, C.corev.p, K, C.Kp, C.W.p, C.B.p, C.tmask.p);
    GX_TRY(check_launch("k_lcc_dense_fill"));
    if (C.O.m)
        hipLaunchKernelGGL(k_lcc_dense_mark_in, dim3(grid_for(C.O.m, 256, 16384)), dim3(256), 0, s, C.O.icode.p, C.O.m,
                           C.coreidx.p);
    GX_TRY(check_launch("k_lcc_dense_mark_in"));
    GX_HIP_TRY(hipStreamSynchronize(s));
    return GX_SUCCESS;
}

int lcc_dense_count(gx_graph *g, LccCache &C, unsigned long long *tc, hipStream_t s) {
    if (!C.K) return GX_SUCCESS;
    KTimer kt(g->ctx, "lcc_core", s);
    GX_HIP_TRY(hipMemsetAsync(C.tcore.p, 0, (size_t)C.Kp * 8, s));
    const int32_t nwg = C.Kp / kDenseWG;
    hipLaunchKernelGGL(k_lcc_dense_mfma, dim3((unsigned)nwg * nwg), dim3(256), 0, s, C.W.p, C.B.p, C.tmask.p, C.Kp,
                       C.tcore.p);
    GX_TRY(check_launch("k_lcc_dense_mfma"));
    hipLaunchKernelGGL(k_lcc_dense_final, dim3(grid_for(C.K, 256, 1024)), dim3(256), 0, s, C.tcore.p, C.corev.p, C.K,
                       tc);
    return check_launch("k_lcc_dense_final");
}

}  // namespace gx

GX_MODULE_WARMER(lcc_dense)

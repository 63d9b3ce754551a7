// gx_rows.h -- the row walk and the wave append that the frontier-peeling drivers share
// (gx_core.hip, gx_scc.hip): workgroups of kRowsBlock threads, wave64.
#pragma once

#include "gx_device.h"

namespace gx {

constexpr int kRowsBlock = 256;

// The lanes with `app` append w to list, one atomic per wave.  Every lane of the wave calls it.
__device__ __forceinline__ void wave_append(bool app, uint32_t w, uint32_t *__restrict__ list, uint32_t *cnt) {
    const unsigned long long m = __ballot(app);
    if (!m) return;
    const int lane = threadIdx.x & (kWave - 1), leader = __ffsll(m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(cnt, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader, kWave);
    if (app) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = w;
}

// Every stored entry (u, w) of the listed rows (list == nullptr: rows 0 .. count - 1), chunk by chunk
// of kRowsBlock rows, the chunks `first`, `first + stride`, ...: a row of at most short_len entries
// by its thread, of at most long_len by its wave, a longer one by the workgroup.  f.visit(u, w, on) is
// called by every lane of a wave together; `on` = the lane holds an entry.  Whole workgroups call it.
template <class F>
__device__ __forceinline__ void walk_rows(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                          const uint32_t *list, uint32_t count, int short_len, int long_len,
                                          unsigned first, unsigned stride, F &f) {
    __shared__ uint32_t big[kRowsBlock];
    __shared__ uint32_t nbig;
    const int lane = threadIdx.x & (kWave - 1);
    for (unsigned long long base = (unsigned long long)first * kRowsBlock; base < count;
         base += (unsigned long long)stride * kRowsBlock) {
        if (threadIdx.x == 0) nbig = 0;
        __syncthreads();
        const unsigned long long x = base + threadIdx.x;
        uint32_t u = 0;
        int64_t b = 0, e = 0;
        if (x < count) {
            u = list ? list[x] : (uint32_t)x;
            b = rp[u];
            e = rp[u + 1];
        }
        const int64_t len = e - b;
        const bool one = len <= short_len;            // an empty slot has len 0: nothing to do
        const bool wave = !one && len <= long_len;
        for (int64_t p = b; __any(one && p < e); p++) {
            const bool on = one && p < e;
            f.visit(u, on ? (uint32_t)ci[p] : 0u, on);
        }
        for (unsigned long long m = __ballot(wave); m; m &= m - 1) {
            const int l = __ffsll(m) - 1;
            const uint32_t u2 = (uint32_t)__shfl((int)u, l, kWave);
            const int64_t b2 = __shfl(b, l, kWave), e2 = __shfl(e, l, kWave);
            for (int64_t p = b2; p < e2; p += kWave) {
                const bool on = p + lane < e2;
                f.visit(u2, on ? (uint32_t)ci[p + lane] : 0u, on);
            }
        }
        if (!one && !wave) big[atomicAdd(&nbig, 1u)] = u;   // at most one per thread: <= kRowsBlock
        __syncthreads();
        const uint32_t nb = nbig;
        for (uint32_t i = 0; i < nb; i++) {
            const uint32_t u3 = big[i];
            const int64_t b3 = rp[u3], e3 = rp[u3 + 1];
            for (int64_t p = b3; p < e3; p += kRowsBlock) {
                const bool on = p + threadIdx.x < e3;
                f.visit(u3, on ? (uint32_t)ci[p + threadIdx.x] : 0u, on);
            }
        }
        __syncthreads();   // big and nbig are the next chunk's too
    }
}

}  // namespace gx

// gx_lcc_part.hip -- partitioned LCC (gx_lcc_part_*; gx_lcc.hip has the algorithm): the graph
// is replicated, ranks split the orientation sources; the caller sums the n counters of all
// ranks (one all-reduce) and finishes locally.
#include <memory>
#include <vector>

#include "gx_lcc.h"

namespace gx {
namespace {

// Work estimate of vertex u for balancing ranks: sum over v in I(u) of 1 + |O(v)|, plus
// |O(u)|.  One wave per vertex (hubs have long in-lists).
__global__ __launch_bounds__(kLccBlock) void k_lcc_work(const int64_t *__restrict__ orp,
                                                        const int64_t *__restrict__ irp,
                                                        const uint32_t *__restrict__ icode, int64_t n,
                                                        uint64_t *work) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t nw = (int64_t)gridDim.x * kWavesPerBlock;
    for (int64_t u = ((int64_t)blockIdx.x * kLccBlock + threadIdx.x) / kWave; u < n; u += nw) {
        uint64_t w = 0;
        for (int64_t k = irp[u] + lane; k < irp[u + 1]; k += kWave) {
            const int32_t v = (int32_t)((icode[k] >> 2) & kVMask);
            w += 1 + (uint64_t)(orp[v + 1] - orp[v]);
        }
        for (int off = 32; off > 0; off >>= 1) w += __shfl_xor(w, off, kWave);
        if (lane == 0) work[u] = w + 1 + (uint64_t)(orp[u + 1] - orp[u]);
    }
}

}  // namespace
}  // namespace gx

using namespace gx;

struct gx_lcc_part {
    gx_graph *g = nullptr;
    gx::LccOrient orient;
};

extern "C" int gx_lcc_part_create(gx_graph *g, gx_lcc_part **part) {
    if (!g || !part) return fail(GX_NULL_POINTER, "gx_lcc_part_create: null argument");
    GX_TRY(lcc_check_size(g->n, "gx_lcc_part_create"));
    GX_HIP_TRY(hipSetDevice(g->ctx->device));
    GX_TRY(ensure_closure(g));
    auto p = std::make_unique<gx_lcc_part>();
    p->g = g;
    if (g->n) GX_TRY(lcc_orient(g, p->orient, g->ctx->stream));
    *part = p.release();
    return GX_SUCCESS;
}

extern "C" int gx_lcc_part_ranges(gx_lcc_part *part, int nranks, uint64_t *ranges) {
    if (!part || !ranges) return fail(GX_NULL_POINTER, "gx_lcc_part_ranges: null argument");
    if (nranks < 1) return fail(GX_INVALID_VALUE, "gx_lcc_part_ranges: nranks < 1");
    gx_graph *g = part->g;
    const int64_t n = (int64_t)g->n;
    hipStream_t s = g->ctx->stream;
    std::vector<uint64_t> w(n);
    if (n) {
        DBuf<uint64_t> work;
        GX_TRY(work.alloc(n));
        hipLaunchKernelGGL(k_lcc_work, dim3(grid_for((uint64_t)n * kWave, kLccBlock, 8192)), dim3(kLccBlock), 0, s,
                           part->orient.orp.p, part->orient.irp.p, part->orient.icode.p, n, work.p);
        GX_TRY(check_launch("k_lcc_work"));
        GX_HIP_TRY(hipMemcpyAsync(w.data(), work.p, n * 8, hipMemcpyDeviceToHost, s));
        GX_HIP_TRY(hipStreamSynchronize(s));
    }
    uint64_t total = 0;
    for (uint64_t x : w) total += x;
    ranges[0] = 0;
    uint64_t acc = 0;
    int64_t v = 0;
    for (int k = 1; k < nranks; k++) {
        const uint64_t target = (uint64_t)((long double)total * k / nranks);
        while (v < n && acc + w[v] <= target) acc += w[v++];
        ranges[k] = (uint64_t)v;
    }
    ranges[nranks] = (uint64_t)n;
    return GX_SUCCESS;
}

// The items of [v0, v1) are cut at every call, under the knobs of that call.
extern "C" int gx_lcc_part_counts(gx_lcc_part *part, uint64_t v0, uint64_t v1, uint64_t *tc, void *stream) {
    if (!part || !tc) return fail(GX_NULL_POINTER, "gx_lcc_part_counts: null argument");
    gx_graph *g = part->g;
    if (v0 > v1 || v1 > g->n) return fail(GX_INVALID_INDEX, "gx_lcc_part_counts: bad vertex range");
    const LccKnobs kn = lcc_knobs();
    GX_HIP_TRY(hipSetDevice(g->ctx->device));
    hipStream_t s = (hipStream_t)stream;   // NULL = the null stream (torch's default)
    LccItems L;
    GX_TRY(lcc_items(part->orient, (int64_t)v0, (int64_t)v1, kn, L, s));
    GX_TRY(lcc_count_items(g, part->orient, L, (unsigned long long *)tc, s));
    GX_HIP_TRY(hipStreamSynchronize(s));   // item lists are freed on return
    return GX_SUCCESS;
}

extern "C" int gx_lcc_part_finish(gx_lcc_part *part, const uint64_t *tc, double *lcc, void *stream) {
    if (!part || !tc || !lcc) return fail(GX_NULL_POINTER, "gx_lcc_part_finish: null argument");
    gx_graph *g = part->g;
    GX_HIP_TRY(hipSetDevice(g->ctx->device));
    hipStream_t s = (hipStream_t)stream;   // NULL = the null stream (torch's default)
    return lcc_finish(g->S.rp.p, (const unsigned long long *)tc, (int64_t)g->n, lcc, s);
}

extern "C" int gx_lcc_part_free(gx_lcc_part *part) {
    delete part;
    return GX_SUCCESS;
}

GX_MODULE_WARMER(lcc_part)

// gx_pr_order.hip -- PageRank's hub-first order and the plans built from a resident graph.
//
// Hub-first: vertices by out-degree descending, ties by id.  The pull SpMV gathers x(u) once per
// out-edge of u, so this packs the most gathered entries of x into its first few MiB, which stay
// resident in each XCD's 4 MiB L2, and it puts every vertex without out-edges last (a rank's live
// prefix, its dangling rows one range).
//
// The plans: pr_single_plan (gx_pagerank: the whole graph as one rank; its adaptive variant
// materialises the relabelled CSR for k_pr_pull) and pr_multi_plan (gx_pagerank_multi: one
// device's rows of the interleaved or the block partition).  Both order the vertices on the
// device (HubOrder), hand the sorted plan the caller's pull matrix to read through order / perm,
// and end in pr_plan (gx_pr.hip).  The partitions built from host data are in gx_pr_part.hip.
#include <algorithm>
#include <memory>

#include "gx_pr.h"

using namespace gx;

namespace {

// keys[e] = (perm[row] << 32) | perm[col] for every entry: sorted, they give the relabelled
// CSR with every row sorted by new column id.  Edge-balanced.
__global__ void k_permute_keys(const int64_t *__restrict__ rp, const int32_t *__restrict__ ci, int64_t n,
                               int64_t nnz, const int32_t *__restrict__ perm, uint64_t *__restrict__ keys) {
    constexpr int kPer = 16;
    const int64_t e0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * kPer;
    if (e0 >= nnz) return;
    const int64_t e1 = min(e0 + kPer, nnz);
    int64_t r = row_of_edge(rp, n, e0);
    for (int64_t e = e0; e < e1; e++) {
        while (rp[r + 1] <= e) r++;
        keys[e] = ((uint64_t)(uint32_t)perm[r] << 32) | (uint32_t)perm[ci[e]];
    }
}

// (out-degree, vertex) pairs; a stable descending sort of the degrees gives the hub-first order
// (degree descending, ties by id)
__global__ void k_hub_keys(const int32_t *__restrict__ outdeg, int64_t n, uint32_t *__restrict__ deg,
                           int32_t *__restrict__ ids) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        deg[v] = (uint32_t)outdeg[v];
        ids[v] = (int32_t)v;
    }
}

// order[i] = v, perm[v] = i, the hub-first row's out-degree and pull length (plen[n] = 0, so an
// exclusive scan of n + 1 values gives the relabelled row pointers)
__global__ void k_hub_apply(const int32_t *__restrict__ sorted_ids, int64_t n, const int32_t *__restrict__ outdeg,
                            const int64_t *__restrict__ prp, int32_t *__restrict__ order, int32_t *__restrict__ perm,
                            int32_t *__restrict__ nout, int64_t *__restrict__ plen) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x) {
        if (i == n) {
            plen[n] = 0;
            continue;
        }
        const int32_t v = sorted_ids[i];
        order[i] = v;
        perm[v] = (int32_t)i;
        nout[i] = outdeg[v];
        plen[i] = prp[v + 1] - prp[v];
    }
}

// Runs of equal values in the sorted (non-increasing) degrees: (position << 32 | degree) of
// every run's first element, in any order; the count may pass `cap` (then nothing past it is
// written and the caller falls back to the full arrays).
__global__ void k_degree_runs(const uint32_t *__restrict__ sdeg, int64_t n, uint64_t *__restrict__ runs,
                              uint32_t *__restrict__ count, uint32_t cap) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (i > 0 && sdeg[i] == sdeg[i - 1]) continue;
        const uint32_t k = atomicAdd(count, 1u);
        if (k < cap) runs[k] = ((uint64_t)i << 32) | sdeg[i];
    }
}

// Device `d` of `ndev` (gx_pagerank_multi's interleaved partition): its local row j is hub-first
// position i = d + j ndev; the row's source vertex, out-degree and pull length (plen[rows] = 0
// for the exclusive scan).
__global__ void k_multi_pick(const int32_t *__restrict__ order, const int32_t *__restrict__ nout,
                             const int64_t *__restrict__ plen, int ndev, int d, int64_t rows,
                             int32_t *__restrict__ my_order, int32_t *__restrict__ my_out,
                             int64_t *__restrict__ my_plen) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j <= rows; j += (int64_t)gridDim.x * blockDim.x) {
        if (j == rows) {
            my_plen[rows] = 0;
            continue;
        }
        const int64_t i = (int64_t)d + j * ndev;
        my_order[j] = order[i];
        my_out[j] = nout[i];
        my_plen[j] = plen[i];
    }
}

// vertex -> its slot in the exchanged vector: owner (i mod ndev) * chunk + local row (i / ndev)
__global__ void k_multi_colmap(const int32_t *__restrict__ perm, int64_t n, int ndev, int64_t chunk,
                               int32_t *__restrict__ colmap) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = perm[v];
        colmap[v] = (int32_t)((i % ndev) * chunk + i / ndev);
    }
}

// Rows of device d's block partition: hub-first positions pos[j] (MultiBlocks).
__global__ void k_block_pick(const int32_t *__restrict__ order, const int32_t *__restrict__ nout,
                             const int64_t *__restrict__ plen, const int32_t *__restrict__ pos, int64_t rows,
                             int32_t *__restrict__ my_order, int32_t *__restrict__ my_out,
                             int64_t *__restrict__ my_plen) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j <= rows; j += (int64_t)gridDim.x * blockDim.x) {
        if (j == rows) {
            my_plen[rows] = 0;
            continue;
        }
        const int64_t i = pos[j];
        my_order[j] = order[i];
        my_out[j] = nout[i];
        my_plen[j] = plen[i];
    }
}

// vertex -> its exchange slot through its hub-first position (MultiBlocks::slot)
__global__ void k_block_colmap(const int32_t *__restrict__ perm, int64_t n, const int32_t *__restrict__ slot,
                               int32_t *__restrict__ colmap) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x)
        colmap[v] = slot[perm[v]];
}

// The hub-first order on the host (a stable counting sort), for the adaptive plan.
void hub_order(const std::vector<int32_t> &outdeg, std::vector<int32_t> &order, std::vector<int32_t> &perm) {
    const size_t n = outdeg.size();
    int32_t maxd = 0;
    for (int32_t d : outdeg) maxd = std::max(maxd, d);
    std::vector<int64_t> start((size_t)maxd + 2, 0);
    for (int32_t d : outdeg) start[(size_t)(maxd - d) + 1]++;
    for (size_t k = 1; k < start.size(); k++) start[k] += start[k - 1];
    order.assign(n, 0);
    perm.assign(n, 0);
    for (size_t v = 0; v < n; v++) {
        const int64_t pos = start[(size_t)(maxd - outdeg[v])]++;
        order[pos] = (int32_t)v;
        perm[v] = (int32_t)pos;
    }
}

// The hub-first order on the device as one stage: (out-degree, vertex) keys, a stable radix sort
// of the n pairs by degree descending, then per position its vertex, out-degree and pull length.
// It owns the sort's temporaries, which the stream still reads when run() returns: the caller
// keeps it alive up to its next stream synchronisation.
struct HubOrder {
    DBuf<uint32_t> d0, d1;   // the degrees as keys; d1: sorted, non-increasing
    DBuf<int32_t> i0, i1;    // the vertex ids beside them; i1: sorted, the order itself
    DBuf<int64_t> plen;      // pull length per position, plen[n] = 0 (an exclusive scan: row pointers)
    // order[i] = the vertex at position i, nout[i] its out-degree, perm[v] = v's position.
    // perm null: into i0, which is free once the ids are sorted.
    int run(gx_graph *g, const DevCSR &P, int32_t *order, int32_t *perm, int32_t *nout, hipStream_t s) {
        const uint64_t n = g->n;
        GX_TRY(d0.alloc(n));
        GX_TRY(d1.alloc(n));
        GX_TRY(i0.alloc(n));
        GX_TRY(i1.alloc(n));
        GX_TRY(plen.alloc(n + 1));
        const unsigned grid = grid_for(n + 1, 256, 8192);
        hipLaunchKernelGGL(k_hub_keys, dim3(grid), dim3(256), 0, s, g->outdeg.p, (int64_t)n, d0.p, i0.p);
        GX_TRY(check_launch("k_hub_keys"));
        GX_TRY(sort_pairs_desc_u32_i32(d0.p, d1.p, i0.p, i1.p, n, s));
        hipLaunchKernelGGL(k_hub_apply, dim3(grid), dim3(256), 0, s, i1.p, (int64_t)n, g->outdeg.p, P.rp.p, order,
                           perm ? perm : i0.p, nout, plen.p);
        return check_launch("k_hub_apply");
    }
};

// The CSR-Adaptive kernel's plan (GX_PR_KERNEL=adaptive): the hub-first relabelled pull CSR
// itself, built by a radix sort of (perm[row] << 32 | perm[col]) keys.
int pr_single_plan_adaptive(gx_graph *g, const PrKnobs &k, PrPart **out) {
    const uint64_t n = g->n;
    gx_ctx *ctx = g->ctx;
    hipStream_t s = ctx->stream;
    DevCSR &P = g->directed ? g->AT : g->A;
    PlanClock clk("single", s);
    GX_TRY(ensure_host_rp(ctx, g->A));
    std::vector<int32_t> h_outdeg(n), order, perm;
    for (uint64_t v = 0; v < n; v++) h_outdeg[v] = (int32_t)(g->A.h_rp[v + 1] - g->A.h_rp[v]);
    hub_order(h_outdeg, order, perm);
    clk.mark("outdeg + hub order (host)");
    std::vector<int64_t> nrp(n + 1, 0);
    std::vector<int32_t> nout(n);
    for (uint64_t i = 0; i < n; i++) {
        const int32_t v = order[i];
        nrp[i + 1] = nrp[i] + (P.h_rp[v + 1] - P.h_rp[v]);
        nout[i] = h_outdeg[v];
    }
    auto p = pr_new_part(ctx, n, 1, 0, pr_chunk(n), ~0ull, 0.85, false, k);
    GX_TRY(p->perm.alloc(n));
    GX_TRY(p->rp_own.alloc(n + 1));
    GX_TRY(p->ci_own.alloc(P.nnz, 16));
    GX_TRY(p->outdeg_own.alloc(n));
    GX_TRY(p->xa.alloc(p->chunk));
    GX_TRY(p->xb.alloc(p->chunk));
    GX_TRY(p->rank_out.alloc(n));
    GX_TRY(p->result.alloc(n));
    GX_HIP_TRY(hipMemsetAsync(p->xa.p, 0, p->chunk * sizeof(double), s));   // padding: the zero column
    GX_HIP_TRY(hipMemsetAsync(p->xb.p, 0, p->chunk * sizeof(double), s));
    GX_HIP_TRY(hipMemcpyAsync(p->perm.p, perm.data(), n * 4, hipMemcpyHostToDevice, s));
    GX_HIP_TRY(hipMemcpyAsync(p->rp_own.p, nrp.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
    GX_HIP_TRY(hipMemcpyAsync(p->outdeg_own.p, nout.data(), n * 4, hipMemcpyHostToDevice, s));
    clk.mark("row pointers + uploads");
    if (P.nnz) {
        DBuf<uint64_t> keys, scratch;
        GX_TRY(keys.alloc(P.nnz));
        GX_TRY(scratch.alloc(P.nnz));
        hipLaunchKernelGGL(k_permute_keys, dim3(grid_for((P.nnz + 15) / 16, 256, 1u << 30)), dim3(256), 0, s,
                           P.rp.p, P.ci.p, (int64_t)n, (int64_t)P.nnz, p->perm.p, keys.p);
        GX_TRY(check_launch("k_permute_keys"));
        GX_TRY(sort_keys_to_csr(keys, scratch, P.nnz, (int64_t)n, p->rp_own.p, p->ci_own.p, s));
        GX_HIP_TRY(hipStreamSynchronize(s));   // keys / scratch die here
    }
    clk.mark("relabel (keys + sort)");
    GX_TRY(pr_plan(p.get(), nrp, p->rp_own.p, p->ci_own.p, p->outdeg_own.p, nout));
    clk.mark("pr_plan");
    GX_HIP_TRY(hipStreamSynchronize(s));   // host vectors above die at return
    *out = p.release();
    return GX_SUCCESS;
}

}  // namespace

// gx_pagerank's plan: the hub-first order on the device (a radix sort of n keys), the
// relabelled row pointers by a scan, then the column-sorted blocks read straight from the
// caller's pull matrix through order / perm (pr_plan_sorted's one radix sort): no relabelled
// CSR is materialised.  The host sees only the row pointers and out-degrees it plans blocks
// from.  Replaces LAGraph_Cached_OutDegree / LAGraph_Cached_AT's share of processing time
// (pr.cpp:58-60).
int gx::pr_single_plan(gx_graph *g, const PrKnobs &k, PrPart **out) {
    if (k.adaptive) return pr_single_plan_adaptive(g, k, out);
    const uint64_t n = g->n;
    gx_ctx *ctx = g->ctx;
    hipStream_t s = ctx->stream;
    DevCSR &P = g->directed ? g->AT : g->A;
    PlanClock clk("single", s);
    GX_TRY(ensure_outdeg(g));
    auto p = pr_new_part(ctx, n, 1, 0, pr_chunk(n), ~0ull, 0.85, false, k);
    GX_TRY(p->perm.alloc(n));
    GX_TRY(p->order.alloc(n));
    GX_TRY(p->rp_own.alloc(n + 1));
    GX_TRY(p->outdeg_own.alloc(n));
    GX_TRY(p->xa.alloc(p->chunk));
    GX_TRY(p->xb.alloc(p->chunk));
    GX_HIP_TRY(hipMemsetAsync(p->xa.p, 0, p->chunk * sizeof(double), s));   // padding: the zero column
    GX_HIP_TRY(hipMemsetAsync(p->xb.p, 0, p->chunk * sizeof(double), s));
    GX_TRY(p->rank_out.alloc(n));
    GX_TRY(p->result.alloc(n));
    // An undirected graph pulls over A itself, so the hub-first rows' lengths are its degrees
    // sorted descending: the host gets them as runs of equal degrees (a few thousand pairs,
    // k_degree_runs over the device's sorted keys) instead of 12 n bytes of row pointers and
    // lengths (SYN-8_5: 6.6 ms of download).  A directed graph pulls over A' in out-degree order:
    // its row lengths come from the device.
    LengthRuns runs;
    bool have_runs = false;
    {
        HubOrder H;
        GX_TRY(H.run(g, P, p->order.p, p->perm.p, p->outdeg_own.p, s));
        GX_TRY(scan_exclusive_i64(H.plen.p, p->rp_own.p, n + 1, s));
        if (!g->directed) {
            constexpr uint32_t kRunCap = 1u << 20;
            DBuf<uint64_t> rb;
            DBuf<uint32_t> rc;
            GX_TRY(rb.alloc(kRunCap));
            GX_TRY(rc.alloc(1));
            GX_HIP_TRY(hipMemsetAsync(rc.p, 0, 4, s));
            hipLaunchKernelGGL(k_degree_runs, dim3(grid_for(n + 1, 256, 8192)), dim3(256), 0, s, H.d1.p, (int64_t)n,
                               rb.p, rc.p, kRunCap);
            GX_TRY(check_launch("k_degree_runs"));
            uint32_t nr = 0;
            GX_HIP_TRY(hipMemcpyAsync(&nr, rc.p, 4, hipMemcpyDeviceToHost, s));
            GX_HIP_TRY(hipStreamSynchronize(s));
            if (nr <= kRunCap) {
                std::vector<uint64_t> h(nr);
                if (nr) GX_HIP_TRY(hipMemcpy(h.data(), rb.p, (size_t)nr * 8, hipMemcpyDeviceToHost));
                std::sort(h.begin(), h.end());   // by position
                runs.n = n;
                int64_t acc = 0;
                for (size_t j = 0; j < h.size(); j++) {
                    const int64_t pos = (int64_t)(h[j] >> 32), val = (int64_t)(uint32_t)h[j];
                    if (j) acc += (pos - runs.pos.back()) * runs.val.back();
                    runs.pos.push_back(pos);
                    runs.val.push_back(val);
                    runs.base.push_back(acc);
                }
                runs.total = (int64_t)P.nnz;
                have_runs = true;
            }
        }
        GX_HIP_TRY(hipStreamSynchronize(s));   // the temporaries are freed at the end of the block
    }
    clk.mark("hub order + row pointers (device)");
    // not value-initialised: zeroing 12 n bytes on one thread cost more than the transfer
    std::unique_ptr<int64_t[]> nrp;
    std::unique_ptr<int32_t[]> nout;
    if (!have_runs) {
        // download() stages through the context's pinned buffers and events, which the column
        // upload of gx_pagerank_csr (g->job) is using on its own thread: let it finish first
        if (g->job) GX_TRY(g->job->join());
        nrp.reset(new int64_t[n + 1]);
        nout.reset(new int32_t[n]);
        GX_TRY(download(ctx, nrp.get(), p->rp_own.p, n + 1, Xfer::Raw64));
        GX_TRY(download(ctx, nout.get(), p->outdeg_own.p, n, Xfer::Raw32));
    } else {
        p->rows_desc = true;   // row lengths non-increasing: the LONG rows are a prefix
    }
    clk.mark("row pointers to the host");
    p->src_rp = P.rp.p;
    p->src_ci = P.ci.p;
    p->src_order = p->order.p;
    p->src_perm = p->perm.p;
    // the columns still arriving (gx_pagerank_csr; undirected: the pull matrix is A itself): the
    // plan's key pass takes them chunk by chunk as they land (pr_plan_sorted)
    p->job = g->directed ? nullptr : g->job.get();
    if (have_runs)
        GX_TRY(pr_plan(p.get(), HostView<int64_t>(&runs, true), p->rp_own.p, nullptr, p->outdeg_own.p,
                       HostView<int32_t>(&runs, false)));
    else
        GX_TRY(pr_plan(p.get(), HostView<int64_t>(nrp.get(), n + 1), p->rp_own.p, nullptr, p->outdeg_own.p,
                       HostView<int32_t>(nout.get(), n)));
    GX_HIP_TRY(hipStreamSynchronize(s));   // host vectors above die at return
    p->job = nullptr;
    clk.mark("pr_plan");
    *out = p.release();
    return GX_SUCCESS;
}

// gx_pagerank_multi's plan of device `d` of `ndev`, all on that device from its copy of the
// graph: the hub-first order (the same radix sort on every device, so every device derives
// the same partition), the device's rows (hub-first positions d, d + ndev, ..., or mb's blocks)
// as the sorted plan's source rows, and the column map into the exchange layout as its column
// renaming.  Replaces the host transpose / row picking / column remapping of round 3 (VERDICT
// r03 #2).
int gx::pr_multi_plan(gx_graph *g, int ndev, int d, uint64_t chunk, double damping, const MultiBlocks *mb,
                      const PrKnobs &k, PrPart **out) {
    const uint64_t n = g->n;
    gx_ctx *ctx = g->ctx;
    hipStream_t s = ctx->stream;
    DevCSR &P = g->directed ? g->AT : g->A;
    PlanClock clk("multi", s);
    GX_TRY(ensure_outdeg(g));
    const uint64_t rows = mb ? mb->pos[d].size() : n > (uint64_t)d ? (n - (uint64_t)d + ndev - 1) / ndev : 0;
    // force_huge: the whole graph's block cut (pr_plan_sorted `piece`); the live prefix comes below
    auto p = pr_new_part(ctx, n, ndev, d, chunk, ~0ull, damping, mb != nullptr, k);
    GX_TRY(p->order.alloc(std::max<uint64_t>(rows, 1)));
    GX_TRY(p->perm.alloc(n));   // the column map
    GX_TRY(p->rp_own.alloc(rows + 1));
    GX_TRY(p->outdeg_own.alloc(std::max<uint64_t>(rows, 1)));
    {
        HubOrder H;
        DBuf<int32_t> ord, nout;
        DBuf<int64_t> myplen;
        GX_TRY(ord.alloc(n));
        GX_TRY(nout.alloc(n));
        GX_TRY(myplen.alloc(rows + 1));
        GX_TRY(H.run(g, P, ord.p, nullptr, nout.p, s));
        const int32_t *full_perm = H.i0.p;
        if (mb) {
            DBuf<int32_t> pos, slot;
            GX_TRY(pos.alloc(std::max<uint64_t>(rows, 1)));
            GX_TRY(slot.alloc(n));
            if (rows) GX_HIP_TRY(hipMemcpy(pos.p, mb->pos[d].data(), rows * 4, hipMemcpyHostToDevice));
            GX_HIP_TRY(hipMemcpy(slot.p, mb->slot.data(), n * 4, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(k_block_pick, dim3(grid_for(rows + 1, 256, 8192)), dim3(256), 0, s, ord.p, nout.p,
                               H.plen.p, pos.p, (int64_t)rows, p->order.p, p->outdeg_own.p, myplen.p);
            GX_TRY(check_launch("k_block_pick"));
            hipLaunchKernelGGL(k_block_colmap, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, full_perm, (int64_t)n,
                               slot.p, p->perm.p);
            GX_TRY(check_launch("k_block_colmap"));
            GX_TRY(scan_exclusive_i64(myplen.p, p->rp_own.p, rows + 1, s));
            GX_HIP_TRY(hipStreamSynchronize(s));   // pos / slot die here
        } else {
            hipLaunchKernelGGL(k_multi_pick, dim3(grid_for(rows + 1, 256, 8192)), dim3(256), 0, s, ord.p, nout.p,
                               H.plen.p, ndev, d, (int64_t)rows, p->order.p, p->outdeg_own.p, myplen.p);
            GX_TRY(check_launch("k_multi_pick"));
            hipLaunchKernelGGL(k_multi_colmap, dim3(grid_for(n, 256, 8192)), dim3(256), 0, s, full_perm, (int64_t)n,
                               ndev, (int64_t)chunk, p->perm.p);
            GX_TRY(check_launch("k_multi_colmap"));
            GX_TRY(scan_exclusive_i64(myplen.p, p->rp_own.p, rows + 1, s));
        }
        GX_HIP_TRY(hipStreamSynchronize(s));   // the temporaries are freed at the end of the block
    }
    clk.mark("hub order + partition rows (device)");
    std::unique_ptr<int64_t[]> nrp(new int64_t[rows + 1]);
    std::unique_ptr<int32_t[]> nout(new int32_t[std::max<uint64_t>(rows, 1)]);
    GX_TRY(download(ctx, nrp.get(), p->rp_own.p, rows + 1, Xfer::Raw64));
    if (rows) GX_TRY(download(ctx, nout.get(), p->outdeg_own.p, rows, Xfer::Raw32));
    // the live prefix: rows with out-edges (hub-first, so a prefix of the device's rows)
    p->live = first_zero(HostView<int32_t>(nout.get(), rows));
    clk.mark("row pointers to the host");
    p->src_rp = P.rp.p;
    p->src_ci = P.ci.p;
    p->src_order = p->order.p;
    p->src_perm = p->perm.p;
    GX_TRY(pr_plan(p.get(), HostView<int64_t>(nrp.get(), rows + 1), p->rp_own.p, nullptr, p->outdeg_own.p,
                   HostView<int32_t>(nout.get(), rows)));
    GX_HIP_TRY(hipStreamSynchronize(s));   // host vectors above die at return
    clk.mark("pr_plan");
    *out = p.release();
    return GX_SUCCESS;
}

GX_MODULE_WARMER(pr_order)

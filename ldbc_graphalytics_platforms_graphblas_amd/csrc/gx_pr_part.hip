// gx_pr_part.hip -- PageRank partitions built from host data: the host-only partitions of
// gx_pagerank_multi (pr_multi_blocks, pr_multi_interleave), a rank's plan from its local rows
// (pr_part_build, pr_part_build_rows) and the row partition API gx_pr_part_*.  No kernel lives
// here: the plans end in pr_plan (gx_pr.hip), the plans of a resident graph are in
// gx_pr_order.hip.
#include <algorithm>
#include <memory>

#include "gx_pr.h"

using namespace gx;

// The block partition of gx_pagerank_multi (MultiBlocks), on the host from A: the hub-first
// order (as the devices' radix sort orders it), the pull rows' lengths in it (A's
// out-degrees; A''s rows, the in-degrees, when directed), the greedy cut of pr_plan_sorted's
// huge-graph blocks (kPlanBlockRows rows, kPlanBlockNnz entries; GX_PR_MULTI_BLOCK_ROWS /
// _NNZ shrink them for tests), then largest block first to the device with the least entries +
// rows.  A device's positions stay in hub-first order, so its rows without out-edges come last
// (the live prefix).  The devices' own sorts must agree with each other, not with this order:
// a position names whichever vertex a device's order puts there, and every device's plan and
// column map read the same (device) order.
int gx::pr_multi_blocks(const gx_csr *A, int directed, int ndev, const PrKnobs &k, MultiBlocks *out) {
    const uint64_t n = A->n;
    // hub-first order, its degrees, all on the host's threads (the serial counting sort and its
    // random re-reads of the degrees were ~350 ms of SYN-8_5's partition)
    std::vector<int32_t> &order = out->order, &perm = out->perm;
    order.resize(n);
    perm.resize(n);
    std::vector<int64_t> hdeg(n);   // out-degree of the vertex at each hub-first position
    PlanClock clk("multi_blocks", nullptr, true);
    host_hub_order_par(A->rowptr, n, order.data(), perm.data(), hdeg.data());
    clk.mark("hub order (host)");
    std::vector<int64_t> indeg_h;
    if (directed) {   // the pull rows are A''s: their lengths are the in-degrees
        std::vector<int64_t> indeg(n, 0);
        for (uint64_t e = 0; e < A->rowptr[n]; e++) indeg[A->colidx[e]]++;
        indeg_h.resize(n);
        for (uint64_t h = 0; h < n; h++) indeg_h[h] = indeg[order[h]];
    }
    const std::vector<int64_t> &len = directed ? indeg_h : hdeg;
    const int64_t R = k.block_rows, B = k.block_nnz;
    std::vector<int64_t> starts;
    for (uint64_t r = 0; r < n;) {
        starts.push_back((int64_t)r);
        uint64_t e = r;
        int64_t ent = 0;
        // at least one row; then rows while both caps hold
        do ent += len[e++];
        while (e < n && (int64_t)(e - r) < R && ent + len[e] <= B);
        r = e;
    }
    starts.push_back((int64_t)n);
    clk.mark("block cut");
    const size_t nb = starts.size() - 1;
    // work = entries + rows (the epilogue); live = rows with out-edges (the exchanged chunk)
    std::vector<int64_t> work(nb), blive(nb);
    for (size_t b = 0; b < nb; b++) {
        int64_t s = 0, l = 0;
        for (int64_t h = starts[b]; h < starts[b + 1]; h++) {
            s += len[h];
            l += hdeg[h] > 0;
        }
        work[b] = s + (starts[b + 1] - starts[b]);
        blive[b] = l;
    }
    // heaviest first: the upper half by work to the least loaded device (LPT), the lighter half
    // to the device with the fewest live rows among those it keeps within 1 % of the mean work
    // (pr_partition._deal_blocks): SYN-8_5 at 8 devices exchanges 0.672 n doubles, not 0.709 n
    std::vector<size_t> byb(nb);
    for (size_t b = 0; b < nb; b++) byb[b] = b;
    std::stable_sort(byb.begin(), byb.end(), [&](size_t x, size_t y) { return work[x] > work[y]; });
    double heavy = 0.0;
    if (nb) {
        std::vector<int64_t> w2(work);
        std::sort(w2.begin(), w2.end());
        heavy = nb % 2 ? (double)w2[nb / 2] : 0.5 * ((double)w2[nb / 2 - 1] + (double)w2[nb / 2]);
    }
    double total = 0.0;
    for (int64_t w : work) total += (double)w;
    const double target = total / ndev;
    std::vector<double> load(ndev, 0.0);
    std::vector<int64_t> lv(ndev, 0);
    std::vector<int> owner(nb, 0);
    for (size_t b : byb) {
        int d = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        if ((double)work[b] < heavy) {
            int best = -1;
            for (int j = 0; j < ndev; j++)
                if (load[j] + (double)work[b] <= target * 1.01 && (best < 0 || lv[j] < lv[best])) best = j;
            if (best >= 0) d = best;
        }
        owner[b] = d;
        load[d] += (double)work[b];
        lv[d] += blive[b];
    }
    clk.mark("work + deal");
    out->pos.assign(ndev, {});
    std::vector<uint64_t> npos(ndev, 0), lvd(ndev, 0);
    for (size_t b = 0; b < nb; b++) {
        npos[owner[b]] += (uint64_t)(starts[b + 1] - starts[b]);
        lvd[owner[b]] += (uint64_t)blive[b];
    }
    for (int d = 0; d < ndev; d++) out->pos[d].reserve(npos[d]);
    for (size_t b = 0; b < nb; b++)
        for (int64_t h = starts[b]; h < starts[b + 1]; h++) out->pos[owner[b]].push_back((int32_t)h);
    uint64_t live = 0;
    for (int d = 0; d < ndev; d++) live = std::max(live, lvd[d]);
    out->chunk = pr_chunk(live);
    if (!pr_chunk_fits(out->chunk, ndev)) return fail(GX_NOT_IMPLEMENTED, "gx_pagerank_multi: exchange too large");
    clk.mark("positions");
    out->slot.assign(n, 0);
    for (int d = 0; d < ndev; d++)
        for (size_t j = 0; j < out->pos[d].size(); j++)
            out->slot[out->pos[d][j]] = (int32_t)((uint64_t)d * out->chunk + j);
    clk.mark("slots");
    return GX_SUCCESS;
}

int gx::pr_multi_interleave(const gx_csr *A, int ndev, MultiBlocks *out) {
    const uint64_t n = A->n;
    const uint64_t nlive = host_count_live(A->rowptr, n);
    out->order.resize(n);
    out->perm.resize(n);
    std::vector<int64_t> hdeg(n);
    host_hub_order_par(A->rowptr, n, out->order.data(), out->perm.data(), hdeg.data());
    out->chunk = pr_chunk((nlive + ndev - 1) / ndev);   // rank 0 holds the most live rows
    if (!pr_chunk_fits(out->chunk, ndev)) return fail(GX_NOT_IMPLEMENTED, "gx_pagerank_multi: exchange too large");
    out->pos.assign(ndev, {});
    out->slot.assign(n, 0);
    for (uint64_t h = 0; h < n; h++) {
        const int d = (int)(h % (uint64_t)ndev);
        out->slot[h] = (int32_t)((uint64_t)d * out->chunk + out->pos[d].size());
        out->pos[d].push_back((int32_t)h);
    }
    return GX_SUCCESS;
}

int gx::pr_part_build(gx_ctx *ctx, uint64_t n_global, int nranks, int rank, uint64_t chunk, uint64_t live,
                      const std::vector<int64_t> &h_rp, const std::vector<int32_t> &ci,
                      const std::vector<int32_t> &h_outdeg, double damping, const PrKnobs &k, PrPart **out,
                      bool force_huge) {
    const uint64_t rows = h_rp.size() - 1, nnz = (uint64_t)h_rp[rows];
    auto p = pr_new_part(ctx, n_global, nranks, rank, chunk, live, damping, force_huge, k);
    GX_TRY(p->rp_own.alloc(rows + 1));
    GX_TRY(p->ci_own.alloc(nnz, 16));
    GX_TRY(p->outdeg_own.alloc(std::max<uint64_t>(rows, 1)));
    GX_HIP_TRY(hipMemcpy(p->rp_own.p, h_rp.data(), (rows + 1) * 8, hipMemcpyHostToDevice));
    if (nnz) GX_HIP_TRY(hipMemcpy(p->ci_own.p, ci.data(), nnz * 4, hipMemcpyHostToDevice));
    if (rows) GX_HIP_TRY(hipMemcpy(p->outdeg_own.p, h_outdeg.data(), rows * 4, hipMemcpyHostToDevice));
    p->src_rp = p->rp_own.p;
    p->src_ci = p->ci_own.p;
    GX_TRY(pr_plan(p.get(), h_rp, p->rp_own.p, p->ci_own.p, p->outdeg_own.p, h_outdeg));
    *out = p.release();
    return GX_SUCCESS;
}

int gx::pr_part_build_rows(gx_ctx *ctx, const gx_csr *A, int nranks, int rank, uint64_t chunk,
                           const std::vector<int32_t> &rows, const int32_t *colmap, double damping, bool force_huge,
                           const PrKnobs &k, PrPart **out) {
    const uint64_t nr = rows.size();
    std::vector<int64_t> h_rp(nr + 1);
    std::vector<int32_t> h_outdeg(nr);
    h_rp[0] = 0;
    uint64_t live = 0;
    for (uint64_t j = 0; j < nr; j++) {
        const int64_t len = (int64_t)(A->rowptr[rows[j] + 1] - A->rowptr[rows[j]]);
        h_rp[j + 1] = h_rp[j] + len;
        h_outdeg[j] = (int32_t)len;   // undirected: the pull row is the vertex's out-edge list
        live += len > 0;
    }
    const uint64_t nnz = (uint64_t)h_rp[nr];
    auto p = pr_new_part(ctx, A->n, nranks, rank, chunk, live, damping, force_huge, k);
    GX_TRY(p->rp_own.alloc(nr + 1));
    GX_TRY(p->ci_own.alloc(nnz, 16));
    GX_TRY(p->outdeg_own.alloc(std::max<uint64_t>(nr, 1)));
    bool bad = false;
    GX_TRY(upload_staged(ctx, p->rp_own.p, nr + 1, 8,
                         [&](uint64_t off, uint64_t cnt, void *buf) {
                             host_copy(buf, h_rp.data() + off, cnt * 8);
                             return true;
                         }, &bad));
    if (nr)
        GX_TRY(upload_staged(ctx, p->outdeg_own.p, nr, 4,
                             [&](uint64_t off, uint64_t cnt, void *buf) {
                                 host_copy(buf, h_outdeg.data() + off, cnt * 4);
                                 return true;
                             }, &bad));
    GX_TRY(upload_staged(ctx, p->ci_own.p, nnz, 4,
                         [&](uint64_t off, uint64_t cnt, void *buf) {
                             return host_pick_span(A->rowptr, A->colidx, rows.data(), h_rp.data(), nr, off, off + cnt,
                                                   A->n, static_cast<int32_t *>(buf));
                         }, &bad));
    if (bad) return fail(GX_INVALID_INDEX, "gx_pagerank_multi: column out of range");
    p->src_rp = p->rp_own.p;
    p->src_ci = p->ci_own.p;
    p->src_perm = colmap;
    GX_TRY(pr_plan(p.get(), HostView<int64_t>(h_rp), p->rp_own.p, p->ci_own.p, p->outdeg_own.p,
                   HostView<int32_t>(h_outdeg)));
    GX_HIP_TRY(hipStreamSynchronize(ctx->stream));
    *out = p.release();
    return GX_SUCCESS;
}

// ---------------------------------------------------------------- row partition API

extern "C" int gx_pr_part_create(gx_ctx *ctx, uint64_t n_global, int nranks, int rank,
                                 const uint64_t *row_ranges, const uint64_t *rowptr_local,
                                 const uint64_t *colidx_local, const uint64_t *outdeg_local,
                                 double damping, gx_pr_part **out) {
    return gx_pr_part_create_live(ctx, n_global, nranks, rank, row_ranges, nullptr, rowptr_local, colidx_local,
                                  outdeg_local, damping, out);
}

extern "C" int gx_pr_part_create_live(gx_ctx *ctx, uint64_t n_global, int nranks, int rank,
                                      const uint64_t *row_ranges, const uint64_t *live_rows,
                                      const uint64_t *rowptr_local, const uint64_t *colidx_local,
                                      const uint64_t *outdeg_local, double damping, gx_pr_part **out) {
    if (!ctx || !row_ranges || !rowptr_local || !outdeg_local || !out)
        return fail(GX_NULL_POINTER, "gx_pr_part_create: null argument");
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(GX_INVALID_VALUE, "bad rank/nranks");
    if (row_ranges[0] != 0 || row_ranges[nranks] != n_global)
        return fail(GX_INVALID_VALUE, "row_ranges must cover [0, n)");
    GX_HIP_TRY(hipSetDevice(ctx->device));
    // the exchanged prefix of every rank: its live rows (all of them without live_rows)
    std::vector<uint64_t> live(nranks);
    uint64_t maxlive = 0;
    for (int k = 0; k < nranks; k++) {
        if (row_ranges[k + 1] < row_ranges[k]) return fail(GX_INVALID_VALUE, "row_ranges not monotone");
        live[k] = row_ranges[k + 1] - row_ranges[k];
        if (live_rows) {
            if (live_rows[k] > live[k]) return fail(GX_INVALID_VALUE, "live_rows beyond the rank's rows");
            live[k] = live_rows[k];
        }
        maxlive = std::max(maxlive, live[k]);
    }
    const uint64_t chunk = pr_chunk(maxlive);
    if (!pr_chunk_fits(chunk, nranks)) return fail(GX_NOT_IMPLEMENTED, "partition too large");
    const uint64_t rows = row_ranges[rank + 1] - row_ranges[rank];
    const uint64_t nnz = rowptr_local[rows];
    if (nnz && !colidx_local) return fail(GX_NULL_POINTER, "null colidx");
    for (uint64_t i = live[rank]; i < rows; i++)
        if (outdeg_local[i] != 0) return fail(GX_INVALID_VALUE, "a row past live_rows has out-edges");
    std::vector<int64_t> h_rp(rows + 1);
    for (uint64_t i = 0; i <= rows; i++) h_rp[i] = (int64_t)rowptr_local[i];
    std::vector<int32_t> ci(nnz);
    const int bad = nnz ? host_chunk_columns(colidx_local, nnz, row_ranges, nranks, live.data(), chunk, n_global, ci.data())
                        : 0;
    if (bad & 1) return fail(GX_INVALID_INDEX, "column out of range");
    if (bad & 2) return fail(GX_INVALID_VALUE, "a column is past its owner's live rows (a vertex without out-edges)");
    std::vector<int32_t> h_outdeg(rows);
    for (uint64_t i = 0; i < rows; i++) h_outdeg[i] = (int32_t)outdeg_local[i];
    PrPart *p = nullptr;
    GX_TRY(pr_part_build(ctx, n_global, nranks, rank, chunk, live[rank], h_rp, ci, h_outdeg, damping, pr_knobs(), &p));
    *out = reinterpret_cast<gx_pr_part *>(p);
    return GX_SUCCESS;
}

extern "C" int gx_pr_part_chunk(gx_pr_part *part, uint64_t *chunk) {
    if (!part || !chunk) return fail(GX_NULL_POINTER, "null argument");
    *chunk = reinterpret_cast<PrPart *>(part)->chunk;
    return GX_SUCCESS;
}

extern "C" int gx_pr_part_init(gx_pr_part *part, double *x_local, void *stream) {
    if (!part || !x_local) return fail(GX_NULL_POINTER, "null argument");
    PrPart *p = reinterpret_cast<PrPart *>(part);
    GX_HIP_TRY(hipSetDevice(p->ctx->device));
    return pr_init(p, x_local, stream ? (hipStream_t)stream : p->ctx->stream);
}

extern "C" int gx_pr_part_step(gx_pr_part *part, const double *x_full, double *x_local,
                               double *rank_out, void *stream) {
    if (!part || !x_full || !x_local) return fail(GX_NULL_POINTER, "null argument");
    PrPart *p = reinterpret_cast<PrPart *>(part);
    GX_HIP_TRY(hipSetDevice(p->ctx->device));
    return pr_step(p, x_full, x_local, rank_out, stream ? (hipStream_t)stream : p->ctx->stream);
}

extern "C" int gx_pr_part_free(gx_pr_part *part) {
    if (!part) return GX_SUCCESS;
    PrPart *p = reinterpret_cast<PrPart *>(part);
    (void)hipSetDevice(p->ctx->device);
    (void)hipDeviceSynchronize();
    delete p;
    return GX_SUCCESS;
}

// gx_pr.hip -- PageRank (Graphalytics definition) as one fused pull-SpMV per iteration: the
// iteration (pr_plan, pr_step, the closed-form first iteration) and the single-GPU entry points
// gx_pagerank / gx_pagerank_csr.  The hub-first order and the plans of a resident graph are in
// gx_pr_order.hip, the partitions built from host data and the gx_pr_part_* API in
// gx_pr_part.hip, the default kernel and its plan in gx_pr_sorted.hip / gx_pr_plan.hip.
//
// Replaces LA_PR -> LAGraph_Cached_OutDegree + LAGraph_Cached_AT + LAGr_PageRankGX
// (pr.cpp:47-66), whose hot loop is one GrB_mxv PLUS_SECOND over A' per iteration.
//
// Per iteration, for every vertex v of the rank's rows:
//     teleport = (1-d)/n + d/n * sum_k dangling_k           (k over ranks, fixed order)
//     r(v)     = teleport + sum_{u in in(v)} x(u)
//     x'(v)    = outdeg(v) > 0 ? r(v) / (outdeg(v)/d) : r(v)
// where x(u) = r(u)/(outdeg(u)/d) is what the previous iteration stored, and a dangling
// vertex stores r itself (it has no out-edges, so nobody gathers its slot).  That is the
// GX arithmetic of the oracle (oracle/gx_oracle.c orc_pagerank) with the division by the
// out-degree fused into the producer of x instead of a separate GrB_eWiseMult pass.
//
// HBM traffic per iteration (algorithmic): 4 B per stored entry (int32 column index),
// 8 B row pointer + 4 B out-degree + 8 B x write per row, the x gathers (L2 / MALL
// resident for the graphs we run), and 8 B per row for the scores in the last iteration.
//
// The kernel of an iteration is the plan's (PrPart::kernel, chosen by whoever lays the matrix
// out): k_pr_pull_units over column-sorted blocks (gx_pr_sorted.hip) by default, or k_pr_pull
// here under GX_PR_KERNEL=adaptive, the fallback whose sums run in row order and are bitwise
// the same in every run (about 3x slower).
//
// k_pr_pull is CSR-Adaptive (Greathouse & Daga): rows are packed into workgroups of at
// most kStreamNnz entries; a workgroup streams its contiguous column-index range with
// 16-B loads, gathers x into LDS, then reduces each row with a power-of-two lane group.
// Rows longer than kStreamNnz get whole workgroups (split into kSegNnz segments, combined
// by the last-arriving segment through an agent-scope release/acquire ticket), and are
// dispatched first so they overlap the stream blocks.
#include <algorithm>
#include <string>

#include "gx_pr.h"

namespace gx {
namespace {

struct PullArgs {
    const RowBlock *blocks;
    const int64_t *rp;
    const int32_t *ci;
    const int32_t *outdeg;
    const double *x_in;
    double *x_out;
    int64_t block_offset;
    double *rank_out;
    int64_t chunk;
    int nranks;
    int zero_slot;
    double teleport0, damping_over_n, damping;
    const int32_t *long_first;
    const int32_t *long_nseg;
    double *long_part;
    uint32_t *long_ticket;
    double *xd;
    int64_t live;
};

__device__ __forceinline__ void pr_epilogue(const PullArgs &a, int32_t row, double s,
                                            double teleport) {
    const double r = teleport + s;
    if (a.rank_out) a.rank_out[row] = r;
    const int32_t deg = a.outdeg[row];
    store_x(a.x_out, a.xd, a.live, row, deg > 0 ? r / ((double)deg / a.damping) : r);
}

template <int NB, bool STRIDE1>
__global__ __launch_bounds__(kPullBlock) void k_pr_pull(PullArgs a) {
    __shared__ __attribute__((aligned(16))) double vals[NB + 4];
    __shared__ int32_t rofs[kStreamRows + 1];
    __shared__ double wred[kPullBlock / kWave];

    const RowBlock b = a.blocks[a.block_offset + blockIdx.x];
    const int tid = threadIdx.x;

    double dsum = 0.0;
    for (int k = 0; k < a.nranks; k++) dsum += a.x_in[(int64_t)k * a.chunk + a.chunk - 1];
    const double teleport = a.teleport0 + a.damping_over_n * dsum;
    if (a.zero_slot && blockIdx.x == 0 && tid == 0) a.x_out[a.chunk - 1] = 0.0;

    if (b.split < 0) {
        // ---------------- STREAM: short rows staged through LDS ----------------
        const int64_t z0 = b.nz_begin, z1 = b.nz_end;
        const int32_t r0 = b.row_begin;
        const int nrows = b.row_end - b.row_begin;
        // LDS is indexed from the 16-B aligned `base`, so every lane stores its four values
        // as two aligned 16-B words; the reduction only reads [rofs[r], rofs[r+1]).
        const int64_t base = z0 & ~(int64_t)3;
        for (int i = tid; i <= nrows; i += kPullBlock) rofs[i] = (int32_t)(a.rp[r0 + i] - base);
        const int nq = (int)((z1 - base + 3) >> 2);
        const int4 *ci4 = reinterpret_cast<const int4 *>(a.ci) + (base >> 2);
        // lane group per row, fixed for the block; the epilogue's out-degree is fetched early
        int L = kWave;
        while (L > 1 && L * nrows > kPullBlock) L >>= 1;
        const int row = tid / L, lane = tid & (L - 1);
        const bool writer = row < nrows && lane == 0;
        const int32_t deg = writer ? a.outdeg[r0 + row] : 0;
        if (STRIDE1) {
            // Lane-consecutive entries: gather instruction j of a wave covers 64 consecutive
            // entries, so with every row sorted by (hub-first) column id neighbouring lanes
            // often hit the same x cache line -- one L1 miss serves several gathers.  The
            // L1-miss count is what bounds this kernel (~70 misses in flight per CU).
            constexpr int NE = (NB + 3 + kPullBlock - 1) / kPullBlock;
            const int64_t last = z1 > base ? z1 - 1 : base;   // clamp: index loads stay valid
            int32_t c[NE];
#pragma unroll
            for (int j = 0; j < NE; j++)
                c[j] = __builtin_nontemporal_load(a.ci + min(base + tid + (int64_t)j * kPullBlock, last));
            double v[NE];
#pragma unroll
            for (int j = 0; j < NE; j++) v[j] = a.x_in[c[j]];
#pragma unroll
            for (int j = 0; j < NE; j++) {
                const int e = tid + j * kPullBlock;
                if (base + e < z1) vals[e] = v[j];
            }
        } else {
        constexpr int NQ = (NB / 4 + kPullBlock) / kPullBlock;
        // Column indices: 16 B per lane, non-temporal (read once; keep L2 for x).  Every
        // index read here is a valid x offset (neighbouring rows' entries, or the zeroed
        // slack past the end), so all gathers below are issued unconditionally.
        int4 c[NQ];
#pragma unroll
        for (int j = 0; j < NQ; j++) {
            const int q = tid + j * kPullBlock;
            c[j] = q < nq ? load_nt(ci4 + q) : make_int4(0, 0, 0, 0);
        }
        double v[NQ][4];
#pragma unroll
        for (int j = 0; j < NQ; j++) {
            v[j][0] = a.x_in[c[j].x];
            v[j][1] = a.x_in[c[j].y];
            v[j][2] = a.x_in[c[j].z];
            v[j][3] = a.x_in[c[j].w];
        }
#pragma unroll
        for (int j = 0; j < NQ; j++) {
            const int q = tid + j * kPullBlock;
            if (q < nq) {
                double2 *d = reinterpret_cast<double2 *>(&vals[4 * q]);
                d[0] = make_double2(v[j][0], v[j][1]);
                d[1] = make_double2(v[j][2], v[j][3]);
            }
        }
        }
        __syncthreads();
        double s = 0.0;
        if (row < nrows) {
            const int kb = rofs[row], ke = rofs[row + 1];
            for (int k = kb + lane; k < ke; k += L) s += vals[k];
        }
        for (int off = L >> 1; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
        if (writer) {
            const double r = teleport + s;
            if (a.rank_out) a.rank_out[r0 + row] = r;
            store_x(a.x_out, a.xd, a.live, r0 + row, deg > 0 ? r / ((double)deg / a.damping) : r);
        }
        return;
    }

    // ---------------- LONG: one segment of one long row ----------------
    const int64_t zb = b.nz_begin, ze = b.nz_end;
    double s0 = 0.0, s1 = 0.0;
    if (STRIDE1) {
        // lane-consecutive entries, 8 loads in flight per lane, clamped (always valid)
        constexpr int U = 8;
        for (int64_t k0 = zb + tid; k0 < ze; k0 += (int64_t)U * kPullBlock) {
            int32_t c[U];
#pragma unroll
            for (int u = 0; u < U; u++)
                c[u] = __builtin_nontemporal_load(a.ci + min(k0 + (int64_t)u * kPullBlock, ze - 1));
            double g[U];
#pragma unroll
            for (int u = 0; u < U; u++) g[u] = a.x_in[c[u]];
#pragma unroll
            for (int u = 0; u < U; u++)
                if (k0 + (int64_t)u * kPullBlock < ze) ((u & 1) ? s1 : s0) += g[u];
        }
    }
    const int64_t base = zb & ~(int64_t)3;
    const int64_t nq = STRIDE1 ? 0 : (ze - base + 3) >> 2;
    const int4 *ci4 = reinterpret_cast<const int4 *>(a.ci) + (base >> 2);
    for (int64_t q = tid; q < nq; q += 2 * kPullBlock) {
        const int64_t q1 = q + kPullBlock;
        const int4 c0 = load_nt(ci4 + q);
        const int4 c1 = q1 < nq ? load_nt(ci4 + q1) : make_int4(0, 0, 0, 0);
        const int64_t e0 = base + 4 * q, e1 = base + 4 * q1;
        const int a0[4] = {c0.x, c0.y, c0.z, c0.w};
        const int a1[4] = {c1.x, c1.y, c1.z, c1.w};
        double g0[4], g1[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {   // unconditional gathers, masked adds
            g0[k] = a.x_in[a0[k]];
            g1[k] = a.x_in[a1[k]];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!(e0 + k >= zb && e0 + k < ze)) g0[k] = 0.0;
            if (!(e1 + k >= zb && e1 + k < ze)) g1[k] = 0.0;
        }
        s0 += (g0[0] + g0[1]) + (g0[2] + g0[3]);
        s1 += (g1[0] + g1[1]) + (g1[2] + g1[3]);
    }
    double s = wave_sum(s0 + s1);
    if ((tid & (kWave - 1)) == 0) wred[tid / kWave] = s;
    __syncthreads();
    if (tid != 0) return;
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < kPullBlock / kWave; w++) tot += wred[w];
    const int32_t sp = b.split;
    const int32_t nseg = a.long_nseg[sp];
    if (nseg == 1) {
        pr_epilogue(a, b.row_begin, tot, teleport);
        return;
    }
    const int32_t first = a.long_first[sp];
    // publish the partial (agent scope), then take a ticket; the last arriver combines
    __hip_atomic_store(&a.long_part[first + b.seg], tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t t = __hip_atomic_fetch_add(&a.long_ticket[sp], 1u, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
    if (t != (uint32_t)(nseg - 1)) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    double all = 0.0;
    for (int j = 0; j < nseg; j++)
        all += __hip_atomic_load(&a.long_part[first + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.long_ticket[sp], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    pr_epilogue(a, b.row_begin, all, teleport);
}

// Sum of the scores of this rank's dangling vertices into the chunk's last slot.
// dlist == nullptr: the dangling rows are the contiguous range [d0, d0 + nd) (hub-first
// order puts every out-degree-0 vertex last), read coalesced.  Workgroup partials are
// combined by the last arriver's whole workgroup in a fixed order (deterministic).
__global__ __launch_bounds__(256) void k_pr_dangling(const int32_t *__restrict__ dlist, int64_t d0,
                                                     int64_t nd, int64_t per, double *x, int64_t slot,
                                                     double *part, uint32_t *ticket, const double *xd,
                                                     int64_t live) {
    __shared__ double wred[256 / kWave];
    __shared__ int last;
    const int tid = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * per, b1 = min(b0 + per, nd);
    double s = 0.0;
    if (dlist) {
        for (int64_t i = b0 + tid; i < b1; i += 256) {
            const int64_t r = dlist[i];
            s += r < live ? x[r] : xd[r - live];
        }
    } else {
        for (int64_t i = b0 + tid; i < b1; i += 256) {
            const int64_t r = d0 + i;
            s += r < live ? x[r] : xd[r - live];
        }
    }
    s = wave_sum(s);
    if ((tid & (kWave - 1)) == 0) wred[tid / kWave] = s;
    __syncthreads();
    const uint32_t G = gridDim.x;
    if (tid == 0) {
        const double tot = (wred[0] + wred[1]) + (wred[2] + wred[3]);
        if (G == 1) {
            x[slot] = tot;
            last = 0;
        } else {
            __hip_atomic_store(&part[blockIdx.x], tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == G - 1;
        }
    }
    __syncthreads();
    if (!last) return;
    // the last arriver sums the partials with the whole workgroup (a serial loop of agent-
    // scope loads by one thread took ~20 us); thread t always takes partials t, t+256, ...
    // and the tree below is fixed, so the sum is the same in every run
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    double a = 0.0;
    for (uint32_t j = tid; j < G; j += 256) a += __hip_atomic_load(&part[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a = wave_sum(a);
    __syncthreads();
    if ((tid & (kWave - 1)) == 0) wred[tid / kWave] = a;
    __syncthreads();
    if (tid == 0) {
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x[slot] = (wred[0] + wred[1]) + (wred[2] + wred[3]);
    }
}

// x = PR_0 / (outdeg / d) (dangling rows: PR_0 itself), and the chunk's dangling slot = the
// sum of its dangling rows' PR_0 = nd / n, known at plan time (no k_pr_dangling launch per run).
__global__ void k_pr_init(const int32_t *__restrict__ outdeg, int64_t rows, double inv_n,
                          double damping, double *x, int64_t slot, double dangling0, double *xd, int64_t live) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t deg = outdeg[i];
        store_x(x, xd, live, i, deg > 0 ? inv_n / ((double)deg / damping) : inv_n);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) x[slot] = dangling0;
}

// k_pr_init and the first iteration in one pass (PrPart::S): x0(u) = d / (n outdeg(u)) is the
// graph's up to a scalar, so r1 = t1 + d/n S with t1 = (1-d)/n + d/n nd/n (nd: the dangling rows
// of all ranks) and S = A (1/outdeg), and x1 = r1 / (outdeg / d) (dangling rows: r1 itself).
// 20 B per row (out-degree, S, x; 8 more when the scores are asked for, a run of one iteration).
// The chunk's dangling slot = the sum of r1 over this rank's nd_local dangling rows.  The padding
// slots (the kernels' zero column among them) are not written.
__global__ void k_pr_first(const int32_t *__restrict__ outdeg, const double *__restrict__ S, int64_t rows, double t1,
                           double damping_over_n, double damping, double nd_local, double *x, int64_t slot,
                           double *rank_out, double *xd, int64_t live) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t deg = outdeg[i];
        const double r = t1 + damping_over_n * S[i];
        if (rank_out) rank_out[i] = r;
        store_x(x, xd, live, i, deg > 0 ? r / ((double)deg / damping) : r);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) x[slot] = nd_local * t1 + damping_over_n * S[rows];
}

// k_pr_pull's work list: the short rows packed into STREAM blocks of at most kStreamNnz entries
// and kStreamRows rows, every longer row cut into LONG segments of kSegNnz entries, those first.
int plan_adaptive_blocks(PrPart *p, HostView<int64_t> h_rp) {
    const int64_t rows = (int64_t)p->rows;
    const int64_t NB = kStreamNnz;
    std::vector<RowBlock> longb, streamb;
    std::vector<int32_t> lfirst, lnseg;
    int32_t nsegs = 0;
    std::vector<std::pair<int64_t, int32_t>> longrows;   // (length, row)
    int64_t r = 0;
    while (r < rows) {
        const int64_t len = h_rp[r + 1] - h_rp[r];
        if (len > NB) {
            longrows.push_back({len, (int32_t)r});
            r++;
            continue;
        }
        const int64_t start = r;
        int64_t nz = 0;
        while (r < rows && r - start < kStreamRows) {
            const int64_t l = h_rp[r + 1] - h_rp[r];
            if (l > NB || nz + l > NB) break;
            nz += l;
            r++;
        }
        streamb.push_back({h_rp[start], h_rp[r], (int32_t)start, (int32_t)r, -1, 0});
    }
    // longest rows first: they are the tail of the launch otherwise
    std::stable_sort(longrows.begin(), longrows.end(),
                     [](const auto &x, const auto &y) { return x.first > y.first; });
    for (const auto &lr : longrows) {
        const int32_t row = lr.second;
        const int64_t len = lr.first;
        const int32_t nseg = (int32_t)((len + kSegNnz - 1) / kSegNnz);
        const int32_t sp = (int32_t)lfirst.size();
        lfirst.push_back(nsegs);
        lnseg.push_back(nseg);
        for (int32_t s = 0; s < nseg; s++) {
            const int64_t zb = h_rp[row] + (int64_t)s * kSegNnz;
            const int64_t ze = std::min(zb + kSegNnz, h_rp[row + 1]);
            longb.push_back({zb, ze, row, row + 1, sp, s});
        }
        nsegs += nseg;
    }
    std::vector<RowBlock> all;
    all.reserve(longb.size() + streamb.size());
    all.insert(all.end(), longb.begin(), longb.end());
    all.insert(all.end(), streamb.begin(), streamb.end());
    p->nblocks = (uint32_t)all.size();
    p->nlong_blocks = (uint32_t)longb.size();
    p->nlong = (uint32_t)lfirst.size();
    p->nsegs = (uint32_t)nsegs;
    GX_TRY(p->blocks.alloc(std::max<size_t>(all.size(), 1)));
    GX_TRY(p->long_first.alloc(std::max<size_t>(lfirst.size(), 1)));
    GX_TRY(p->long_nseg.alloc(std::max<size_t>(lnseg.size(), 1)));
    GX_TRY(p->long_part.alloc(std::max<size_t>(nsegs, 1)));
    GX_TRY(p->long_ticket.alloc(std::max<size_t>(lfirst.size(), 1)));
    if (!all.empty())
        GX_HIP_TRY(hipMemcpy(p->blocks.p, all.data(), all.size() * sizeof(RowBlock), hipMemcpyHostToDevice));
    if (!lfirst.empty()) {
        GX_HIP_TRY(hipMemcpy(p->long_first.p, lfirst.data(), lfirst.size() * 4, hipMemcpyHostToDevice));
        GX_HIP_TRY(hipMemcpy(p->long_nseg.p, lnseg.data(), lnseg.size() * 4, hipMemcpyHostToDevice));
    }
    GX_HIP_TRY(hipMemset(p->long_ticket.p, 0, p->long_ticket.n * 4));
    return GX_SUCCESS;
}

// The dangling rows: one contiguous range (hub-first orders put them last), or a list.
int plan_dangling(PrPart *p, HostView<int32_t> h_outdeg) {
    const int64_t rows = (int64_t)p->rows;
    int64_t dfirst = 0, dlast = -1;
    std::vector<int32_t> dl;
    if (p->src_order) {
        // gx_pagerank's hub-first rows: out-degrees non-increasing, the dangling rows a suffix
        dfirst = (int64_t)first_zero(h_outdeg);
        dlast = rows - 1;
        p->nd = (uint64_t)(rows - dfirst);
    } else {
        for (int64_t i = 0; i < rows; i++)
            if (h_outdeg[i] == 0) dl.push_back((int32_t)i);
        if (!dl.empty()) {
            dfirst = dl.front();
            dlast = dl.back();
        }
        p->nd = dl.size();
    }
    p->d_range = p->nd > 0 && (uint64_t)(dlast - dfirst + 1) == p->nd;
    p->d0 = p->nd > 0 ? dfirst : 0;
    if (!p->d_range) {
        GX_TRY(p->dlist.alloc(std::max<size_t>(dl.size(), 1)));
        if (!dl.empty())
            GX_HIP_TRY(hipMemcpy(p->dlist.p, dl.data(), dl.size() * 4, hipMemcpyHostToDevice));
    }
    p->dgrid = (uint32_t)std::min<uint64_t>(512, std::max<uint64_t>(1, (p->nd + 2047) / 2048));
    GX_TRY(p->dpart.alloc(p->dgrid));
    GX_TRY(p->dticket.alloc(1));
    GX_HIP_TRY(hipMemset(p->dticket.p, 0, 4));
    return GX_SUCCESS;
}

}  // namespace

int pr_plan(PrPart *p, HostView<int64_t> h_rp, const int64_t *d_rp, const int32_t *d_ci,
            const int32_t *d_outdeg, HostView<int32_t> h_outdeg) {
    p->rows = (uint64_t)h_rp.size() - 1;
    if (p->live > p->rows) p->live = p->rows;   // no live prefix given: all rows
    if (p->live < p->rows) GX_TRY(p->xd.alloc(p->rows - p->live));
    p->rp = d_rp;
    p->ci = d_ci;
    p->outdeg = d_outdeg;
    if (p->kernel == 1 && !d_ci)
        return fail(GX_NOT_IMPLEMENTED, "pr_plan: the adaptive kernel needs a plan that holds its own columns");
    PlanClock clk("pr_plan", p->ctx->stream);
    if (p->kernel == 1) {
        GX_TRY(plan_adaptive_blocks(p, h_rp));
        clk.mark("adaptive blocks");
    }
    GX_TRY(plan_dangling(p, h_outdeg));
    clk.mark("dangling rows");
    if (p->kernel == 2) {
        GX_TRY(pr_plan_sorted(p, h_rp, h_outdeg));
        clk.mark("sorted blocks");
    }
    return GX_SUCCESS;
}

int pr_dangling(PrPart *p, double *x_local, hipStream_t s) {
    if (p->nd == 0) return GX_SUCCESS;
    const int64_t per = (int64_t)((p->nd + p->dgrid - 1) / p->dgrid);
    hipLaunchKernelGGL(k_pr_dangling, dim3(p->dgrid), dim3(256), 0, s, p->d_range ? nullptr : p->dlist.p,
                       (int64_t)p->d0, (int64_t)p->nd, per,
                       x_local, (int64_t)p->chunk - 1, p->dpart.p, p->dticket.p, p->xd.p, (int64_t)p->live);
    return check_launch("k_pr_dangling");
}

int pr_init(PrPart *p, double *x_local, hipStream_t s) {
    const double inv_n = 1.0 / (double)p->n_global;
    hipLaunchKernelGGL(k_pr_init, dim3(grid_for(p->rows, 256, 8192)), dim3(256), 0, s, p->outdeg,
                       (int64_t)p->rows, inv_n, p->damping, x_local, (int64_t)p->chunk - 1,
                       (double)p->nd / (double)p->n_global, p->xd.p, (int64_t)p->live);
    return check_launch("k_pr_init");
}

// S, on the first run that wants it.  A failed allocation turns the closed form off for this
// plan: its runs go on as without S, and the launch checks must not see the allocation's error.
bool pr_first_alloc(PrPart *p) {
    if (!p->first_on) return false;
    if (p->S.p) return true;
    if (p->S.alloc(p->rows + 1) != GX_SUCCESS) {
        (void)hipGetLastError();
        p->first_on = false;
        return false;
    }
    return true;
}

// S mode's input: x = 1 / outdeg (k_pr_init with n = 1, d = 1), dangling slot 0.  The dangling
// rows hold 1.0, which nobody gathers.
int pr_first_init(PrPart *p, double *x_local, hipStream_t s) {
    p->first_ready = false;
    hipLaunchKernelGGL(k_pr_init, dim3(grid_for(p->rows, 256, 8192)), dim3(256), 0, s, p->outdeg,
                       (int64_t)p->rows, 1.0, 1.0, x_local, (int64_t)p->chunk - 1, 0.0, p->xd.p, (int64_t)p->live);
    return check_launch("k_pr_init");
}

// S mode's iteration: teleport 0 and damping 1 make the scores the plain sums S, written as the
// launch's scores (so every item runs, the closed-form isolated blocks too: S = 0), and the
// launch's dangling sum is S over the dangling rows, since a dangling row's x is its score.
int pr_first_step(PrPart *p, const double *x_full, double *x_local, hipStream_t s) {
    const PrScalars ov = {0.0, 0.0, 1.0};
    GX_TRY(pr_step(p, x_full, x_local, p->S.p, s, &ov));
    GX_HIP_TRY(hipMemcpyAsync(p->S.p + p->rows, x_local + p->chunk - 1, sizeof(double), hipMemcpyDeviceToDevice, s));
    p->first_ready = true;
    return GX_SUCCESS;
}

int pr_first_build(PrPart *p, double *x_in, double *x_out, hipStream_t s) {
    GX_TRY(pr_first_init(p, x_in, s));
    return pr_first_step(p, x_in, x_out, s);
}

int pr_first(PrPart *p, uint64_t nd_total, double *x_local, double *rank_out, hipStream_t s) {
    const double dn = (double)p->n_global;
    const double t1 = (1.0 - p->damping) / dn + p->damping / dn * ((double)nd_total / dn);
    {
        KTimer kt(p->ctx, "pr_first", s);
        hipLaunchKernelGGL(k_pr_first, dim3(grid_for(p->rows, 256, 8192)), dim3(256), 0, s, p->outdeg, p->S.p,
                           (int64_t)p->rows, t1, p->damping / dn, p->damping, (double)p->nd, x_local,
                           (int64_t)p->chunk - 1, rank_out, p->xd.p, (int64_t)p->live);
    }
    return check_launch("k_pr_first");
}

int pr_step(PrPart *p, const double *x_full, double *x_local, double *rank_out, hipStream_t s, const PrScalars *ov) {
    if (p->kernel == 2) return pr_step_sorted(p, x_full, x_local, rank_out, s, ov);
    const double dn = (double)p->n_global;
    PullArgs a;
    a.blocks = p->blocks.p;
    a.rp = p->rp;
    a.ci = p->ci;
    a.outdeg = p->outdeg;
    a.x_in = x_full;
    a.x_out = x_local;
    a.rank_out = rank_out;
    a.chunk = (int64_t)p->chunk;
    a.nranks = p->nranks;
    a.zero_slot = p->nd == 0 ? 1 : 0;
    a.teleport0 = (1.0 - p->damping) / dn;
    a.damping_over_n = p->damping / dn;
    a.damping = p->damping;
    if (ov) {   // pr_first_build's S mode
        a.teleport0 = ov->teleport0;
        a.damping_over_n = ov->damping_over_n;
        a.damping = ov->damping;
    }
    a.long_first = p->long_first.p;
    a.long_nseg = p->long_nseg.p;
    a.long_part = p->long_part.p;
    a.long_ticket = p->long_ticket.p;
    a.xd = p->xd.p;
    a.live = (int64_t)p->live;
    a.block_offset = 0;
    if (p->nblocks) {
        KTimer kt(p->ctx, "pr_pull", s);
        hipLaunchKernelGGL((k_pr_pull<kStreamNnz, true>), dim3(p->nblocks), dim3(kPullBlock), 0, s, a);
    }
    GX_TRY(check_launch("k_pr_pull"));
    return pr_dangling(p, x_local, s);
}

}  // namespace gx

using namespace gx;

namespace {

// out[v] = in[perm[v]]: back from the hub-first order to the caller's vertex order.
__global__ void k_gather_perm(const double *__restrict__ in, const int32_t *__restrict__ perm, int64_t n,
                              double *__restrict__ out) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n;
         v += (int64_t)gridDim.x * blockDim.x)
        out[v] = in[perm[v]];
}

}  // namespace

using PrClock = std::chrono::steady_clock;

// gx_pagerank, stage 1: columns still arriving (gx_pagerank_csr): only the sorted single plan
// consumes them as they land; every other path waits for all of them
static int pr_settle_upload(gx_graph *g, const PrKnobs &k) {
    if (g->job && (g->directed || g->pr || k.adaptive)) {
        GX_TRY(g->job->join());
        g->job.reset();
    }
    if (g->directed) GX_TRY(ensure_transpose(g));
    return GX_SUCCESS;
}

// Stage 2: the graph's plan, on its first call, built beside the upload when one is running.
static int pr_plan_beside_upload(gx_graph *g, const PrKnobs &k) {
    if (g->pr) return GX_SUCCESS;
    // the plan's temporaries are freed once the upload is over (g_deferred_frees)
    std::vector<void *> deferred;
    // the upload thread narrows with half the host threads: the plan's host loops take the
    // other half (all of them on top of the upload's ran some fused calls 115 ms, not 88)
    const int saved_threads = host_threads();
    if (g->job) {
        g_deferred_frees = &deferred;
        host_set_threads(std::max(1, saved_threads - std::max(1, saved_threads / 2)));
    }
    const int rc = pr_single_plan(g, k, &g->pr);
    g_deferred_frees = nullptr;
    host_set_threads(saved_threads);
    if (g->job) {   // the plan has taken every chunk (or stopped early): the upload is over
        const int jrc = g->job->join();
        g->job.reset();
        for (void *q : deferred) (void)hipFree(q);
        if (rc == GX_SUCCESS && jrc != GX_SUCCESS) return jrc;
    }
    return rc;
}

// Stage 3: the iterations, the last one writing the scores (hub-first order) to p->rank_out.
static int pr_iterate(PrPart *p, int iters, hipStream_t s) {
    double *cur = p->xa.p, *nxt = p->xb.p;
    // iteration 1 in closed form from the plan's S, which the plan's first run builds with the
    // SpMV launch that iteration would have been (GX_PR_FIRST=0, or no memory for S: as before)
    int it0 = 0;
    if (iters >= 1 && pr_first_alloc(p)) {
        if (!p->first_ready) GX_TRY(pr_first_build(p, cur, nxt, s));
        GX_TRY(pr_first(p, p->nd, cur, iters == 1 ? p->rank_out.p : nullptr, s));
        it0 = 1;
    } else {
        GX_TRY(pr_init(p, cur, s));
    }
    for (int it = it0; it < iters; it++) {
        GX_TRY(pr_step(p, cur, nxt, it == iters - 1 ? p->rank_out.p : nullptr, s));
        std::swap(cur, nxt);
    }
    return GX_SUCCESS;
}

// Stage 4: the scores back in the caller's vertex order, and GX_PLAN_TIMES' line of the call.
static int pr_hand_back(gx_graph *g, int iters, double *rank, const PrKnobs &k, PrClock::time_point t_entry,
                        PrClock::time_point t_plan) {
    const uint64_t n = g->n;
    gx_ctx *ctx = g->ctx;
    PrPart *p = g->pr;
    const auto t0 = PrClock::now();
    auto ms = [&](PrClock::time_point a, PrClock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    PrClock::time_point t1 = t0;
    if (iters > 0) {
        hipLaunchKernelGGL(k_gather_perm, dim3(grid_for(n, 256, 8192)), dim3(256), 0, ctx->stream, p->rank_out.p,
                           p->perm.p, (int64_t)n, p->result.p);
        GX_TRY(check_launch("k_gather_perm"));
        host_prefault(rank, n * sizeof(double));
        t1 = PrClock::now();
    }
    GX_TRY(device_end(ctx));
    const auto t2 = PrClock::now();
    if (iters == 0) {
        for (uint64_t v = 0; v < n; v++) rank[v] = 1.0 / (double)n;
        return GX_SUCCESS;
    }
    GX_TRY(download(ctx, rank, p->result.p, n, Xfer::Raw64));
    if (k.plan_times)
        std::fprintf(stderr, "[pagerank] plan %.2f ms, launches %.2f ms, prefault %.2f ms, device wait %.2f ms, "
                     "result copy %.2f ms (device %.2f ms)\n", ms(t_entry, t_plan), ms(t_plan, t0), ms(t0, t1),
                     ms(t1, t2), ms(t2, PrClock::now()), ctx->last_device_ms);
    return GX_SUCCESS;
}

// The four stages in order, under the knobs of the entry call: gx_pagerank_csr has read them
// for its own choice (fused or not) and passes them on, so that a call reads them once.
static int pr_run(gx_graph *g, double damping, int iters, double *rank, const PrKnobs &k) {
    if (g->n == 0) return GX_SUCCESS;
    const auto t_entry = PrClock::now();
    gx_ctx *ctx = g->ctx;
    GX_HIP_TRY(hipSetDevice(ctx->device));
    GX_TRY(device_begin(ctx));
    GX_TRY(pr_settle_upload(g, k));
    GX_TRY(pr_plan_beside_upload(g, k));
    const auto t_plan = PrClock::now();
    g->pr->damping = damping;
    GX_TRY(pr_iterate(g->pr, iters, ctx->stream));
    return pr_hand_back(g, iters, rank, k, t_entry, t_plan);
}

extern "C" int gx_pagerank(gx_graph *g, double damping, int iters, double *rank) {
    if (!g || !rank) return fail(GX_NULL_POINTER, "gx_pagerank: null argument");
    if (iters < 0) return fail(GX_INVALID_VALUE, "gx_pagerank: negative iteration count");
    return pr_run(g, damping, iters, rank, pr_knobs());
}

// The executable's PageRank (bin/exe/pr: pr.cpp:77-79 brackets LAGraph_New .. LAGr_PageRankGX
// between its markers): upload + plan + iterations in one call.  For an undirected graph the
// columns are uploaded by a host thread chunk by chunk while the plan builds the hub-first order
// from the row pointers and then takes each chunk as it lands (graph_create_async,
// pr_plan_sorted's source-side key pass), and the weights, which PageRank never reads, are not
// uploaded at all.  Directed graphs (the plan needs A' whole) and GX_PR_FUSED=0 take
// gx_graph_create + gx_pagerank.
extern "C" int gx_pagerank_csr(gx_ctx *ctx, const gx_csr *A, int directed, double damping, int iters, double *rank,
                               gx_graph **keep) {
    if (!ctx || !A || !rank) return fail(GX_NULL_POINTER, "gx_pagerank_csr: null argument");
    if (iters < 0) return fail(GX_INVALID_VALUE, "gx_pagerank_csr: negative iteration count");
    if (keep) *keep = nullptr;
    const PrKnobs k = pr_knobs();
    const bool fused = !directed && k.fused;
    gx_graph *g = nullptr;
    PlanClock clk("pagerank_csr", ctx->stream);
    if (fused) GX_TRY(graph_create_async(ctx, A, directed, &g));
    else GX_TRY(gx_graph_create(ctx, A, directed, &g));
    clk.mark("graph (columns on their way)");
    const int rc = pr_run(g, damping, iters, rank, k);
    clk.mark("gx_pagerank");
    if (rc != GX_SUCCESS) {
        const std::string msg = gx_last_error();
        (void)gx_graph_free(g);   // joins an upload the call left running (an early error)
        return fail(rc, msg);
    }
    // the graph and its plan (gigabytes of device memory) are the caller's to free, outside the
    // processing time if it likes (bin/exe/pr frees after its end marker, as before)
    if (keep) *keep = g;
    else return gx_graph_free(g);
    return GX_SUCCESS;
}

GX_MODULE_WARMER(pr)

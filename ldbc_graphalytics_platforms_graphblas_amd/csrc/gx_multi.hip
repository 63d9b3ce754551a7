// gx_multi.hip -- the one-process multi-device drivers (bin/exe/* with GX_NGPUS): gx_pagerank_multi,
// gx_sssp_multi, gx_lcc_multi, gx_bfs_multi, gx_wcc_multi, gx_cdlp_multi.  Each is the single-device
// algorithm's partitioned steps on every device, exchanged by the clique of gx_comm.h, which also
// has the per-device owners and loops they share.  The partitioned steps themselves are in
// gx_pr_part.hip, gx_sssp_split.hip, gx_lcc_part.hip (with gx_lcc.h's size check) and gx_part.hip.
#include "gx_comm.h"
#include "gx_lcc.h"

namespace gx {

MultiKnobs multi_knobs(int ndev, bool directed, uint64_t nnz, int num_cus) {
    MultiKnobs k;
    // GX_PR_MULTI_PIECES (1..8; default 2 for several devices, 1 for one: at N = 1 there is no
    // exchange to hide)
    k.pieces = ndev > 1 ? 2 : 1;
    if (const char *e = std::getenv("GX_PR_MULTI_PIECES")) k.pieces = std::atoi(e);
    k.pieces = std::max(1, std::min(k.pieces, Clique::kMaxPieces));
    // A huge graph (more than 2 Mi entries per CU, the single-GPU plan's huge-graph cut) is
    // split by blocks instead (pr_multi_blocks; pr_partition.block_relabel): every virtual
    // rank's blocks are the single-GPU plan's own, so its gathers share x lines as the whole
    // graph's do (1/8 pieces of SYN-8_5: 140 us per SpMV against 208 interleaved).
    // GX_PR_MULTI_PARTITION=blocks / interleave overrides.
    k.by_blocks = ndev * k.pieces > 1 && (double)nnz / (double)std::max(1, num_cus) > (double)(2 << 20);
    if (const char *e = std::getenv("GX_PR_MULTI_PARTITION")) k.by_blocks = std::strcmp(e, "blocks") == 0;
    // Partitioned upload (round 6; GX_PR_MULTI_UPLOAD=rows, the default for
    // undirected graphs, whose pull rows are A's own): the host deals the hub-first order once,
    // and every virtual rank's rows leave the 64-bit input once, for that rank's device only,
    // picked straight into the staging buffers (pr_part_build_rows); the plan's key pass renames
    // the columns into the exchange layout through a device column map.  "whole" (and every
    // directed graph, whose pull rows are A''s) uploads A to every device and plans there
    // (pr_multi_plan).
    k.by_rows = !directed;
    if (const char *e = std::getenv("GX_PR_MULTI_UPLOAD")) k.by_rows = k.by_rows && std::strcmp(e, "whole") != 0;
    k.pr = pr_knobs();
    k.by_rows = k.by_rows && !k.pr.adaptive;   // the adaptive plan is built from a resident graph
    const char *ex = std::getenv("GX_EXCHANGE");
    k.force_dense = ex && std::strcmp(ex, "dense") == 0;
    k.force_sparse = ex && std::strcmp(ex, "sparse") == 0;
    k.plan_times = k.pr.plan_times != 0;
    return k;
}

namespace {

// One gx_pagerank_multi call and its stages, in the order the entry point runs them.
// Pieces (round 6): every device's rows are cut into P pieces, each its
// own plan and launch.  Piece p of every device runs, then its chunks are all-gathered on
// the comm streams while piece p + 1 runs on the compute streams, so only the last piece's
// exchange is exposed (1/P of it) instead of all of it.  Piece p of device d is virtual rank
// p * ndev + d of V = ndev * P ranges: x's slab p (ndev chunks) is what piece p's all-gather
// fills, the layout PrDist uses across processes.
struct MultiRun {
    gx_ctx *const *ctxs;
    const int ndev;
    const gx_csr *A;
    const int directed;
    const double damping;
    const int iters;
    double *rank;
    const MultiKnobs k;
    const int P = k.pieces, V = ndev * k.pieces;
    PlanClock clk{"multi_call", ctxs[0]->stream};
    // partition (host)
    uint64_t chunk = 0;
    MultiBlocks mb;
    std::vector<int32_t> colmap;   // by_rows: vertex -> exchange slot
    // devices: per device its graph (not by_rows) or column map (by_rows) and its full vectors,
    // double-buffered; per piece (piece(d, p)) a plan, its local chunk and its scores
    struct Piece {
        PrPart *part = nullptr;
        DBuf<double> xl, ro;
        uint64_t rows = 0;
        std::vector<int32_t> vrows;   // by_rows: the vertex of each local row (the scores' scatter)
        uint64_t picked = 0;          // by_rows: input columns read
    };
    MultiGraphs G{ndev};   // freed after the destructor's body, so after the pieces planned from them
    std::vector<DBuf<int32_t>> cmap = std::vector<DBuf<int32_t>>(ndev);
    // the vector an iteration reads and the one it writes
    std::vector<DBuf<double>> xr = std::vector<DBuf<double>>(ndev), xw = std::vector<DBuf<double>>(ndev);
    std::vector<Piece> pieces = std::vector<Piece>((size_t)V);
    std::shared_ptr<Clique> clique;

    ~MultiRun() {
        for (int d = 0; d < ndev; d++) {
            (void)hipSetDevice(ctxs[d]->device);
            (void)hipStreamSynchronize(ctxs[d]->stream);
        }
        for (int d = 0; d < ndev; d++) {
            (void)hipSetDevice(ctxs[d]->device);
            for (int p = 0; p < P; p++) {
                delete piece(d, p).part;
                piece(d, p).xl.release();
                piece(d, p).ro.release();
            }
            xr[d].release();
            xw[d].release();
            cmap[d].release();
        }
    }

    Piece &piece(int d, int p) { return pieces[(size_t)d * P + p]; }

    // interleaved hub-first partition (pr_partition.interleaved_relabel): hub-first position i
    // goes to virtual rank i % V as its local row i / V.  The vertices with out-edges come first
    // in that order, so virtual rank 0 holds the most live rows, ceil(nlive / V): the chunk every
    // rank exchanges (+ the zero padding slot and the dangling slot).  The pull matrix of a
    // directed graph is A', whose rows with out-edges in the PageRank sense are still A's rows
    // with out-edges: liveness is A's out-degree either way.  Or the block partition
    // (multi_knobs), whose chunk is its own.
    int partition() {
        const uint64_t n = A->n;
        const uint64_t nlive = host_count_live(A->rowptr, n);
        chunk = pr_chunk((nlive + V - 1) / V);
        if (k.by_rows) {
            if (A->rowptr[0] != 0 || A->rowptr[n] != A->nnz || !host_monotone(A->rowptr, n))
                return fail(GX_INVALID_VALUE, "gx_pagerank_multi: inconsistent row pointers");
        }
        if (k.by_blocks) {
            GX_TRY(pr_multi_blocks(A, directed, V, k.pr, &mb));
            chunk = mb.chunk;
        } else if (k.by_rows) {
            GX_TRY(pr_multi_interleave(A, V, &mb));
            if (mb.chunk != chunk) return fail(GX_PANIC, "gx_pagerank_multi: interleaved chunk mismatch");
        }
        if (!pr_chunk_fits(chunk, V)) return fail(GX_NOT_IMPLEMENTED, "gx_pagerank_multi: exchange too large");
        if (k.by_rows) {
            colmap.resize(n);
            host_compose(mb.slot.data(), mb.perm.data(), n, colmap.data());
        }
        clk.mark("partition (host)");
        return GX_SUCCESS;
    }

    // per device, on the device: upload A, A' if directed (LAGraph_Cached_AT, pr.cpp:60), the
    // hub-first order and each piece's plan (pr_multi_plan), the exchange buffers; or (by_rows)
    // each piece's own rows, picked on the host, and its plan
    int upload_and_plan() {
        const uint64_t n = A->n;
        GX_TRY(per_device(ctxs, ndev, [&](int d) -> int {
            if (!k.by_rows) {
                GX_TRY(gx_graph_create(ctxs[d], A, directed, &G.g[d]));
                if (directed) GX_TRY(ensure_transpose(G.g[d]));
            } else {
                // the column map, once per device (the pieces' key passes rename through it)
                GX_TRY(cmap[d].alloc(n));
                bool bad = false;
                GX_TRY(upload_staged(ctxs[d], cmap[d].p, n, 4,
                                     [&](uint64_t off, uint64_t cnt, void *buf) {
                                         host_copy(buf, colmap.data() + off, cnt * 4);
                                         return true;
                                     }, &bad));
            }
            hipStream_t s = ctxs[d]->stream;
            for (int p = 0; p < P; p++) {
                Piece &pc = piece(d, p);
                const int vr = p * ndev + d;
                if (k.by_rows) {
                    const std::vector<int32_t> &pos = mb.pos[vr];
                    pc.vrows.resize(pos.size());
                    for (size_t j = 0; j < pos.size(); j++) pc.vrows[j] = mb.order[pos[j]];
                    for (int32_t v : pc.vrows) pc.picked += A->rowptr[v + 1] - A->rowptr[v];
                    GX_TRY(pr_part_build_rows(ctxs[d], A, V, vr, chunk, pc.vrows, cmap[d].p, damping, k.by_blocks, k.pr,
                                              &pc.part));
                } else {
                    GX_TRY(pr_multi_plan(G.g[d], V, vr, chunk, damping, k.by_blocks ? &mb : nullptr, k.pr, &pc.part));
                }
                pc.rows = pc.part->rows;
                GX_TRY(pc.xl.alloc(chunk));
                GX_TRY(pc.ro.alloc(std::max<uint64_t>(pc.rows, 1)));
                GX_HIP_TRY(hipMemsetAsync(pc.xl.p, 0, chunk * sizeof(double), s));
            }
            const size_t full = chunk * (size_t)V;
            GX_TRY(xr[d].alloc(full));
            GX_TRY(xw[d].alloc(full));
            GX_HIP_TRY(hipMemsetAsync(xr[d].p, 0, full * sizeof(double), s));
            GX_HIP_TRY(hipMemsetAsync(xw[d].p, 0, full * sizeof(double), s));
            return GX_SUCCESS;
        }));
        clk.mark("devices: upload + plans");
        if (k.by_rows && k.plan_times) {
            uint64_t tot = 0;
            for (const Piece &pc : pieces) tot += pc.picked;
            std::fprintf(stderr, "[multi] partitioned upload: %llu of %llu input columns read (%.3fx), %d devices x %d pieces\n",
                         (unsigned long long)tot, (unsigned long long)A->nnz, A->nnz ? (double)tot / (double)A->nnz : 0.0,
                         ndev, P);
        }
        return GX_SUCCESS;
    }

    // piece p's chunks into slab p of every device's dst, on the compute streams (init) or,
    // after each device's piece-p SpMV, on the comm streams
    int gather(int p, std::vector<DBuf<double>> &dst, bool on_comm) {
        Clique &C = *clique;
        std::vector<void *> send(ndev), recv(ndev);
        for (int d = 0; d < ndev; d++) {
            send[d] = piece(d, p).xl.p;
            recv[d] = dst[d].p + (size_t)p * chunk * (size_t)ndev;
        }
        if (on_comm)
            GX_TRY(in_turn(ctxs, ndev, [&](int d) -> int {
                hipEvent_t ev = C.ev_piece[(size_t)d * Clique::kMaxPieces + p];
                GX_HIP_TRY(hipEventRecord(ev, C.st[d]));
                GX_HIP_TRY(hipStreamWaitEvent(C.cs[d], ev, 0));
                return GX_SUCCESS;
            }));
        return C.all_gather(send.data(), recv.data(), chunk * sizeof(double), (on_comm ? C.cs : C.st).data());
    }

    // the compute streams wait for every exchange issued on the comm streams
    int join() {
        Clique &C = *clique;
        return in_turn(ctxs, ndev, [&](int d) -> int {
            GX_HIP_TRY(hipEventRecord(C.ev_comm[d], C.cs[d]));
            GX_HIP_TRY(hipStreamWaitEvent(C.st[d], C.ev_comm[d], 0));
            return GX_SUCCESS;
        });
    }

    int iterate() {
        GX_TRY(get_clique(ctxs, ndev, &clique));
        GX_TRY(in_turn(ctxs, ndev, [&](int d) -> int {
            for (int p = 0; p < P; p++) GX_TRY(pr_init(piece(d, p).part, piece(d, p).xl.p, ctxs[d]->stream));
            return GX_SUCCESS;
        }));
        for (int p = 0; p < P; p++) GX_TRY(gather(p, xr, false));
        for (int it = 0; it < iters; it++) {
            const bool last = it == iters - 1;
            for (int p = 0; p < P; p++) {
                GX_TRY(in_turn(ctxs, ndev, [&](int d) {
                    Piece &pc = piece(d, p);
                    return pr_step(pc.part, xr[d].p, pc.xl.p, last ? pc.ro.p : nullptr, ctxs[d]->stream);
                }));
                if (!last) GX_TRY(gather(p, xw, true));
            }
            if (last) break;
            GX_TRY(join());
            std::swap(xr, xw);
        }
        clk.mark("iterations");
        return GX_SUCCESS;
    }

    // scores back in A's vertex order: piece k's local row j is vertex order_k[j]
    int scores() {
        GX_TRY(in_turn(ctxs, ndev, [&](int d) -> int {
            std::vector<std::vector<double>> buf(P);
            std::vector<std::vector<int32_t>> who(P);
            for (int p = 0; p < P; p++) {
                Piece &pc = piece(d, p);
                buf[p].resize(pc.rows);
                who[p].resize(pc.rows);
                if (pc.rows) {
                    GX_HIP_TRY(hipMemcpyAsync(buf[p].data(), pc.ro.p, pc.rows * sizeof(double), hipMemcpyDeviceToHost,
                                              ctxs[d]->stream));
                    if (k.by_rows)
                        std::copy(pc.vrows.begin(), pc.vrows.end(), who[p].begin());
                    else
                        GX_HIP_TRY(hipMemcpyAsync(who[p].data(), pc.part->order.p, pc.rows * sizeof(int32_t),
                                                  hipMemcpyDeviceToHost, ctxs[d]->stream));
                }
            }
            GX_HIP_TRY(hipStreamSynchronize(ctxs[d]->stream));
            for (int p = 0; p < P; p++)
                for (uint64_t j = 0; j < buf[p].size(); j++) rank[who[p][j]] = buf[p][j];
            return GX_SUCCESS;
        }));
        clk.mark("scores");
        return GX_SUCCESS;
    }
};

// The vertex ranges of the devices: contiguous, ~nnz / ndev stored entries each
// (pr_partition.partition_rows).
std::vector<uint64_t> entry_ranges(const gx_csr *A, int ndev) {
    const uint64_t n = A->n, nnz = A->nnz;
    std::vector<uint64_t> ranges(ndev + 1, 0);
    for (int k = 1; k < ndev; k++) {
        const uint64_t target = nnz / ndev * k + nnz % ndev * k / ndev;
        const uint64_t r = (uint64_t)(std::lower_bound(A->rowptr, A->rowptr + n + 1, target) - A->rowptr);
        ranges[k] = std::min(std::max(r, ranges[k - 1]), n);
    }
    ranges[ndev] = n;
    return ranges;
}

int upload_replicas(gx_ctx *const *ctxs, int ndev, const gx_csr *A, int directed, MultiGraphs &G) {
    return per_device(ctxs, ndev, [&](int d) -> int { return gx_graph_create(ctxs[d], A, directed, &G.g[d]); });
}

// What one round of a BFS / WCC / CDLP driver exchanges (WordExchange::run): device d's entries
// [span[d].first, span[d].second) of arr[d] that differ from old[d] (old null: from 0) are applied
// to every device's dst[d] with `op` (gx_part_apply), or dense() runs instead.
struct WordRound {
    void *const *arr = nullptr, *const *old = nullptr, *const *dst = nullptr;
    std::vector<std::pair<uint64_t, uint64_t>> span;
    int elem = 4, op = 0;
    uint64_t dense_bytes = 0;      // what dense() moves per device
    std::function<int()> dense;    // empty: no dense form, the words always
};

// Per-device buffers of the word exchange; `cap` words per device (any step changes at most n
// entries), the gathered words grown on demand.
struct WordExchange {
    gx_ctx *const *ctxs;
    const int ndev;
    const MultiKnobs k;
    HostWords<int64_t> hc;   // the all-gathered counts (device 0's copy)
    PerDev<uint64_t> words{ctxs, ndev}, gathered{ctxs, ndev};
    PerDev<int64_t> count{ctxs, ndev}, counts{ctxs, ndev};
    std::vector<uint64_t> gcap = std::vector<uint64_t>(ndev, 0);
    uint64_t rounds = 0, word_rounds = 0, word_bytes = 0, dense_bytes = 0;

    int init(uint64_t cap) {
        GX_TRY(in_turn(ctxs, ndev, [&](int d) -> int {
            GX_TRY(words.alloc_on(d, cap));
            GX_TRY(count.alloc_on(d, 1));
            return counts.alloc_on(d, ndev);
        }));
        return host_words(ctxs[0], ndev, &hc);
    }
    // The round's changes as words, or r.dense() instead when 8 max-count ndev bytes exceed
    // r.dense_bytes (GX_EXCHANGE = sparse / dense forces one).  *total = changes over all devices
    // (0: none anywhere).
    int run(Clique &C, const WordRound &r, uint64_t *total) {
        rounds++;
        GX_TRY(in_turn(ctxs, ndev, [&](int d) {
            return gx_part_changes(r.arr[d], r.old ? r.old[d] : nullptr, r.span[d].first, r.span[d].second, r.elem,
                                   words[d], count[d], ctxs[d]->stream);
        }));
        GX_TRY(C.gather_counts(count.all(), counts.all(), sizeof(int64_t), hc.get()));
        uint64_t m = 0, tot = 0;
        for (int d = 0; d < ndev; d++) {
            m = std::max<uint64_t>(m, (uint64_t)hc[d]);
            tot += (uint64_t)hc[d];
        }
        *total = tot;
        if (m == 0) return GX_SUCCESS;
        if (r.dense && (k.force_dense || (!k.force_sparse && 8 * m * (uint64_t)ndev > r.dense_bytes))) {
            dense_bytes += r.dense_bytes;
            return r.dense();
        }
        word_rounds++;
        word_bytes += 8 * m * (uint64_t)ndev;
        GX_TRY(in_turn(ctxs, ndev, [&](int d) -> int {
            if (gcap[d] >= m * (uint64_t)ndev) return GX_SUCCESS;
            GX_HIP_TRY(hipStreamSynchronize(ctxs[d]->stream));   // the old buffer may still be read
            gcap[d] = std::max<uint64_t>(m * (uint64_t)ndev, 2 * gcap[d]);
            return gathered.alloc_on(d, gcap[d]);
        }));
        GX_TRY(C.all_gather(words.all(), gathered.all(), m * sizeof(uint64_t), C.st.data()));
        return in_turn(ctxs, ndev, [&](int d) {
            return gx_part_apply(gathered[d], counts[d], ndev, m, r.dst[d], r.elem, r.op, ctxs[d]->stream);
        });
    }
    void report(const char *who) const {
        if (k.plan_times)
            std::fprintf(stderr, "[%s] %llu rounds, %llu as words (%.1f MB), dense %.1f MB per device\n", who,
                         (unsigned long long)rounds, (unsigned long long)word_rounds, word_bytes / 1e6 / ndev,
                         dense_bytes / 1e6);
    }
};

}  // namespace
}  // namespace gx

using namespace gx;

extern "C" int gx_pagerank_multi(gx_ctx *const *ctxs, int ndev, const gx_csr *A, int directed, double damping,
                                 int iters, double *rank) {
    GX_TRY(check_multi(ctxs, ndev, A, "gx_pagerank_multi"));
    if (!rank) return fail(GX_NULL_POINTER, "gx_pagerank_multi: null argument");
    if (iters < 0) return fail(GX_INVALID_VALUE, "gx_pagerank_multi: negative iteration count");
    const uint64_t n = A->n;
    const MultiKnobs k = multi_knobs(ndev, directed != 0, A->rowptr[n], ctxs[0]->num_cus);
    if (n == 0) return GX_SUCCESS;
    if (iters == 0) {
        for (uint64_t v = 0; v < n; v++) rank[v] = 1.0 / (double)n;
        return GX_SUCCESS;
    }
    if (n >= (1ull << 31) - 64) return fail(GX_NOT_IMPLEMENTED, "gx_pagerank_multi: n >= 2^31");
    // one device, one piece: no exchange at all, so the single-GPU call itself (upload
    // overlapped with the plan, 24-bit columns: 77 ms on SYN-8_5 where this path's upload and
    // separate plan took 149)
    if (ndev == 1 && k.pieces == 1) return gx_pagerank_csr(ctxs[0], A, directed, damping, iters, rank, nullptr);
    MultiRun M{ctxs, ndev, A, directed, damping, iters, rank, k};
    GX_TRY(M.partition());
    GX_TRY(M.upload_and_plan());
    GX_TRY(M.iterate());
    return M.scores();
}

// Multi-device SSSP in one process (bin/exe/sssp with GX_NGPUS; config 4's other half): the
// 1-D split of gx_sssp_split on every device, the rounds exchanged by the clique.
// Device d owns the targets [ranges[d], ranges[d+1]) (contiguous, ~nnz / ndev stored entries
// each); per round: every device relaxes into its owned vertices, the 2-word counts
// {pairs, done} are all-gathered and read by the host (the only host read of a round), then
// max-count pairs of every device are all-gathered and applied everywhere.  The decisions
// come from replicated state, so every device stops at the same round; a disagreement is an
// error, not a silent stop.
extern "C" int gx_sssp_multi(gx_ctx *const *ctxs, int ndev, const gx_csr *A, int directed, uint64_t src,
                             double *dist) {
    GX_TRY(check_multi(ctxs, ndev, A, "gx_sssp_multi"));
    if (!dist) return fail(GX_NULL_POINTER, "gx_sssp_multi: null argument");
    if (!A->vals) return fail(GX_INVALID_VALUE, "gx_sssp_multi: graph has no edge weights");
    const uint64_t n = A->n;
    if (src >= n) return fail(GX_INVALID_INDEX, "gx_sssp_multi: source out of range");
    const std::vector<uint64_t> ranges = entry_ranges(A, ndev);
    uint64_t maxown = 1;
    for (int d = 0; d < ndev; d++) maxown = std::max(maxown, ranges[d + 1] - ranges[d]);
    MultiGraphs G(ndev);
    HostWords<uint64_t> hc;
    PerDev<uint64_t> pairs(ctxs, ndev), count(ctxs, ndev), counts(ctxs, ndev), all(ctxs, ndev);
    PerDevHandle<gx_sssp_split, gx_sssp_split_free> sp(ctxs, ndev);
    GX_TRY(per_device(ctxs, ndev, [&](int d) -> int {
        GX_TRY(gx_graph_create(ctxs[d], A, directed, &G.g[d]));
        GX_TRY(gx_sssp_split_create(G.g[d], ranges[d], ranges[d + 1], &sp[d]));
        GX_TRY(pairs.alloc_on(d, 2 * maxown));
        GX_TRY(count.alloc_on(d, 2));
        GX_TRY(counts.alloc_on(d, 2 * (uint64_t)ndev));
        return all.alloc_on(d, 2 * maxown * (uint64_t)ndev);
    }));
    std::shared_ptr<Clique> clique;
    GX_TRY(get_clique(ctxs, ndev, &clique));
    Clique &C = *clique;
    GX_TRY(host_words(ctxs[0], 2 * (size_t)ndev, &hc));
    GX_TRY(in_turn(ctxs, ndev, [&](int d) { return gx_sssp_split_start(sp[d], src, ctxs[d]->stream); }));
    for (uint64_t round = 0;; round++) {
        if (round > 4 * (n + 16)) return fail(GX_DEVICE_ERROR, "gx_sssp_multi: no fixed point");
        GX_TRY(in_turn(ctxs, ndev, [&](int d) {
            return gx_sssp_split_relax(sp[d], pairs[d], count[d], ctxs[d]->stream);
        }));
        GX_TRY(C.gather_counts(count.all(), counts.all(), 2 * sizeof(uint64_t), hc.get()));
        int ndone = 0;
        uint64_t m = 0;
        for (int d = 0; d < ndev; d++) {
            ndone += hc[2 * d + 1] != 0;
            m = std::max(m, hc[2 * d]);
        }
        if (ndone == ndev) break;
        if (ndone) {
            // a device that stopped alone stopped on an error (a full settled list):
            // report that cause rather than the disagreement it led to
            for (int d = 0; d < ndev; d++)
                if (hc[2 * d + 1]) {
                    GX_HIP_TRY(hipSetDevice(ctxs[d]->device));
                    GX_TRY(sssp_split_check(sp[d], ctxs[d]->stream));
                }
            return fail(GX_DEVICE_ERROR, "gx_sssp_multi: devices disagree on termination");
        }
        if (m > maxown) return fail(GX_DEVICE_ERROR, "gx_sssp_multi: pair count beyond the owned range");
        if (m) GX_TRY(C.all_gather(pairs.all(), all.all(), 2 * m * sizeof(uint64_t), C.st.data()));
        GX_TRY(in_turn(ctxs, ndev, [&](int d) {
            return gx_sssp_split_apply(sp[d], m ? all[d] : pairs[d], counts[d], ndev, m, ctxs[d]->stream);
        }));
    }
    // the distance vector is replicated: device 0's, in A's vertex order
    GX_HIP_TRY(hipSetDevice(ctxs[0]->device));
    DBuf<double> out;
    GX_TRY(out.alloc(std::max<uint64_t>(n, 1)));
    GX_TRY(gx_sssp_split_distances(sp[0], out.p, ctxs[0]->stream));
    GX_HIP_TRY(hipStreamSynchronize(ctxs[0]->stream));
    GX_TRY(download(ctxs[0], dist, out.p, n, Xfer::Raw64));
    return GX_SUCCESS;
}

// Multi-device LCC in one process (bin/exe/lcc with GX_NGPUS; BASELINE config 5, "LCC on
// cit-Patents, 1 -> 8 GPUs"): A is replicated, every device builds the degree orientation
// (gx_lcc_part_create) and counts the triangles whose middle vertex lies in its range of
// orientation sources, the ranges balanced by the probe work sum |O(v)| over in-neighbours
// (gx_lcc_part_ranges); the n triangle counters of all devices are summed onto device 0 by one
// reduction, which divides by the closure degree there (gx_lcc_part_finish).  The counters are
// integers, so the result is bit-identical to gx_lcc whatever the split.  Replaces LA_LCC
// (lcc.cpp:61-71) when it runs on several GPUs.
extern "C" int gx_lcc_multi(gx_ctx *const *ctxs, int ndev, const gx_csr *A, int directed, double *lcc) {
    GX_TRY(check_multi(ctxs, ndev, A, "gx_lcc_multi"));
    if (!lcc) return fail(GX_NULL_POINTER, "gx_lcc_multi: null argument");
    const uint64_t n = A->n;
    if (n == 0) return GX_SUCCESS;
    GX_TRY(lcc_check_size(n, "gx_lcc_multi"));
    MultiGraphs G(ndev);
    PerDev<uint64_t> tc(ctxs, ndev);
    PerDevHandle<gx_lcc_part, gx_lcc_part_free> part(ctxs, ndev);
    GX_TRY(per_device(ctxs, ndev, [&](int d) -> int {
        GX_TRY(gx_graph_create(ctxs[d], A, directed, &G.g[d]));
        GX_TRY(gx_lcc_part_create(G.g[d], &part[d]));
        return tc.alloc_on(d, n);
    }));
    std::vector<uint64_t> ranges(ndev + 1);
    GX_HIP_TRY(hipSetDevice(ctxs[0]->device));
    GX_TRY(gx_lcc_part_ranges(part[0], ndev, ranges.data()));
    GX_TRY(per_device(ctxs, ndev, [&](int d) -> int {
        GX_HIP_TRY(hipMemsetAsync(tc[d], 0, n * sizeof(uint64_t), ctxs[d]->stream));
        return gx_lcc_part_counts(part[d], ranges[d], ranges[d + 1], tc[d], ctxs[d]->stream);
    }));
    {
        std::shared_ptr<Clique> clique;
        GX_TRY(get_clique(ctxs, ndev, &clique));
        GX_TRY(clique->reduce_sum_u64(tc.all(), n));
    }
    GX_HIP_TRY(hipSetDevice(ctxs[0]->device));
    DBuf<double> out;
    GX_TRY(out.alloc(n));
    GX_TRY(gx_lcc_part_finish(part[0], tc[0], out.p, ctxs[0]->stream));
    GX_HIP_TRY(hipStreamSynchronize(ctxs[0]->stream));
    GX_TRY(download(ctxs[0], lcc, out.p, n, Xfer::Raw64));
    return GX_SUCCESS;
}

// ---- BFS / WCC / CDLP on several devices in one process (round 6) ----
// bin/exe/{bfs,wcc,cdlp} with GX_NGPUS: the graph replicated on every device, device d owning
// the vertex range [ranges[d], ranges[d+1]) (~nnz / ndev stored entries each), the rounds of
// distributed.py (the torch.distributed driver) restated over the in-process clique: every
// device runs its step on its own range, then only what the step changed travels as
// (v << 32 | value) words (gx_part_changes: the counts all-gathered and read by the host, the
// first max-count words of every device all-gathered, gx_part_apply on every device), or the
// dense form when the words would outweigh it.  Every device starts a round with the same
// state, so every device takes the same decisions; results are device 0's copy.

extern "C" int gx_bfs_multi(gx_ctx *const *ctxs, int ndev, const gx_csr *A, int directed, uint64_t src,
                            int64_t *level) {
    GX_TRY(check_multi(ctxs, ndev, A, "gx_bfs_multi"));
    if (!level) return fail(GX_NULL_POINTER, "gx_bfs_multi: null argument");
    const MultiKnobs k = multi_knobs(ndev, directed != 0, A->nnz, ctxs[0]->num_cus);
    const uint64_t n = A->n;
    if (src >= n) return fail(GX_INVALID_INDEX, "gx_bfs_multi: source out of range");
    const std::vector<uint64_t> ranges = entry_ranges(A, ndev);
    MultiGraphs G(ndev);
    GX_TRY(upload_replicas(ctxs, ndev, A, directed, G));
    std::shared_ptr<Clique> clique;
    GX_TRY(get_clique(ctxs, ndev, &clique));
    Clique &C = *clique;
    const uint64_t nw = (n + 31) / 32;
    PerDev<int64_t> lv(ctxs, ndev), cnt(ctxs, ndev);
    PerDev<uint8_t> nxt(ctxs, ndev);
    PerDev<uint32_t> bits(ctxs, ndev), gbits(ctxs, ndev);
    GX_TRY(lv.alloc(n));
    GX_TRY(cnt.alloc(1));
    GX_TRY(nxt.alloc((n + 15) / 16 * 16));   // 16-B multiple (gx_part_pack_bits)
    GX_TRY(bits.alloc(nw));
    GX_TRY(gbits.alloc(nw * (uint64_t)ndev));
    WordExchange X{ctxs, ndev, k};
    GX_TRY(X.init(n));
    GX_TRY(in_turn(ctxs, ndev, [&](int d) { return gx_bfs_part_init(G.g[d], src, lv[d], ctxs[d]->stream); }));
    // the discoveries (next's non-zero bytes) into every device's next
    WordRound r;
    r.arr = r.dst = nxt.all();
    r.span.assign(ndev, {0, n});
    r.elem = 1;
    // dense form: every device's bitmap all-gathered and OR-ed (ndev n / 8 bytes < 2 n below 16)
    r.dense_bytes = (uint64_t)ndev * nw * 4;
    r.dense = [&]() -> int {
        GX_TRY(in_turn(ctxs, ndev, [&](int d) { return gx_part_pack_bits(nxt[d], n, bits[d], ctxs[d]->stream); }));
        GX_TRY(C.all_gather(bits.all(), gbits.all(), nw * sizeof(uint32_t), C.st.data()));
        return in_turn(ctxs, ndev, [&](int d) { return gx_part_or_bits(gbits[d], ndev, n, nxt[d], ctxs[d]->stream); });
    };
    int64_t hcount = 0;
    for (int64_t cur = 0;; cur++) {
        if ((uint64_t)cur > n + 1) return fail(GX_DEVICE_ERROR, "gx_bfs_multi: no fixed point");
        GX_TRY(in_turn(ctxs, ndev, [&](int d) -> int {
            GX_HIP_TRY(hipMemsetAsync(nxt[d], 0, n, ctxs[d]->stream));
            return gx_bfs_part_expand(G.g[d], ranges[d], ranges[d + 1], lv[d], cur, nxt[d], ctxs[d]->stream);
        }));
        uint64_t tot = 0;
        GX_TRY(X.run(C, r, &tot));
        GX_TRY(in_turn(ctxs, ndev, [&](int d) -> int {
            GX_HIP_TRY(hipMemsetAsync(cnt[d], 0, sizeof(int64_t), ctxs[d]->stream));   // commit adds to it
            return gx_bfs_part_commit(G.g[d], nxt[d], lv[d], cur, reinterpret_cast<uint64_t *>(cnt[d]), ctxs[d]->stream);
        }));
        GX_HIP_TRY(hipSetDevice(ctxs[0]->device));
        GX_HIP_TRY(hipMemcpyAsync(&hcount, cnt[0], sizeof(int64_t), hipMemcpyDeviceToHost, ctxs[0]->stream));
        GX_HIP_TRY(hipStreamSynchronize(ctxs[0]->stream));
        if (hcount == 0) break;   // identical on every device (same inputs)
    }
    X.report("bfs_multi");
    GX_HIP_TRY(hipSetDevice(ctxs[0]->device));
    return download(ctxs[0], level, lv[0], n, Xfer::Raw64);
}

extern "C" int gx_wcc_multi(gx_ctx *const *ctxs, int ndev, const gx_csr *A, int directed, uint64_t *comp) {
    GX_TRY(check_multi(ctxs, ndev, A, "gx_wcc_multi"));
    if (!comp) return fail(GX_NULL_POINTER, "gx_wcc_multi: null argument");
    const MultiKnobs k = multi_knobs(ndev, directed != 0, A->nnz, ctxs[0]->num_cus);
    const uint64_t n = A->n;
    if (n == 0) return GX_SUCCESS;
    const std::vector<uint64_t> ranges = entry_ranges(A, ndev);
    MultiGraphs G(ndev);
    GX_TRY(upload_replicas(ctxs, ndev, A, directed, G));
    std::shared_ptr<Clique> clique;
    GX_TRY(get_clique(ctxs, ndev, &clique));
    Clique &C = *clique;
    PerDev<int32_t> par(ctxs, ndev), prev(ctxs, ndev);
    PerDev<int> chg(ctxs, ndev);
    GX_TRY(par.alloc(n));
    GX_TRY(prev.alloc(n));
    GX_TRY(chg.alloc(1));
    WordExchange X{ctxs, ndev, k};
    GX_TRY(X.init(n));
    GX_TRY(in_turn(ctxs, ndev, [&](int d) { return gx_wcc_part_init(G.g[d], par[d], ctxs[d]->stream); }));
    // the changed parents always travel as words (applied with MIN): the dense form of the
    // torch driver is an all-reduce MIN, which the words bound from above anyway
    WordRound r;
    r.arr = r.dst = par.all();
    r.old = prev.all();
    r.span.assign(ndev, {0, n});
    r.op = 1;
    for (uint64_t round = 0;; round++) {
        if (round > n + 1) return fail(GX_DEVICE_ERROR, "gx_wcc_multi: no fixed point");
        GX_TRY(in_turn(ctxs, ndev, [&](int d) -> int {
            GX_HIP_TRY(hipMemcpyAsync(prev[d], par[d], n * 4, hipMemcpyDeviceToDevice, ctxs[d]->stream));
            GX_HIP_TRY(hipMemsetAsync(chg[d], 0, sizeof(int), ctxs[d]->stream));
            return gx_wcc_part_hook(G.g[d], ranges[d], ranges[d + 1], par[d], chg[d], ctxs[d]->stream);
        }));
        uint64_t tot = 0;
        GX_TRY(X.run(C, r, &tot));
        if (tot == 0) break;   // a round in which no device changed anything: the fixed point
        GX_TRY(in_turn(ctxs, ndev, [&](int d) { return gx_wcc_part_compress(G.g[d], par[d], ctxs[d]->stream); }));
    }
    X.report("wcc_multi");
    GX_HIP_TRY(hipSetDevice(ctxs[0]->device));
    return download(ctxs[0], comp, par[0], n, Xfer::Widen32);
}

extern "C" int gx_cdlp_multi(gx_ctx *const *ctxs, int ndev, const gx_csr *A, int directed, int iters,
                             uint64_t *labels) {
    GX_TRY(check_multi(ctxs, ndev, A, "gx_cdlp_multi"));
    if (!labels) return fail(GX_NULL_POINTER, "gx_cdlp_multi: null argument");
    if (iters < 0) return fail(GX_INVALID_VALUE, "gx_cdlp_multi: negative iteration count");
    const MultiKnobs k = multi_knobs(ndev, directed != 0, A->nnz, ctxs[0]->num_cus);
    const uint64_t n = A->n;
    if (n == 0) return GX_SUCCESS;
    const std::vector<uint64_t> ranges = entry_ranges(A, ndev);
    uint64_t chunk = 1;
    for (int d = 0; d < ndev; d++) chunk = std::max(chunk, ranges[d + 1] - ranges[d]);
    MultiGraphs G(ndev);
    GX_TRY(upload_replicas(ctxs, ndev, A, directed, G));
    std::shared_ptr<Clique> clique;
    GX_TRY(get_clique(ctxs, ndev, &clique));
    Clique &C = *clique;
    PerDev<int32_t> lab(ctxs, ndev), nxt(ctxs, ndev), send(ctxs, ndev), gath(ctxs, ndev);
    PerDev<int> chg(ctxs, ndev);
    GX_TRY(lab.alloc(n));
    GX_TRY(nxt.alloc(n));
    GX_TRY(send.alloc(chunk));
    GX_TRY(gath.alloc(chunk * (uint64_t)ndev));
    GX_TRY(chg.alloc(1));
    PerDevHandle<gx_cdlp_part, gx_cdlp_part_free> part(ctxs, ndev);
    WordExchange X{ctxs, ndev, k};
    GX_TRY(X.init(n));
    GX_TRY(in_turn(ctxs, ndev, [&](int d) -> int {
        GX_TRY(gx_cdlp_part_create(G.g[d], ranges[d], ranges[d + 1], &part[d]));
        return gx_cdlp_part_init(part[d], lab[d], ctxs[d]->stream);
    }));
    // the owned labels that changed, set into every device's labels; the owned slices
    // all-gathered when that is smaller
    WordRound r;
    r.arr = nxt.all();
    r.old = r.dst = lab.all();
    for (int d = 0; d < ndev; d++) r.span.push_back({ranges[d], ranges[d + 1]});
    // dense form: the owned slices all-gathered (padded to the largest range) into every labels
    r.dense_bytes = 4 * n;
    r.dense = [&]() -> int {
        GX_TRY(in_turn(ctxs, ndev, [&](int d) -> int {
            const uint64_t own = ranges[d + 1] - ranges[d];
            if (own)
                GX_HIP_TRY(hipMemcpyAsync(send[d], nxt[d] + ranges[d], own * 4, hipMemcpyDeviceToDevice, ctxs[d]->stream));
            return GX_SUCCESS;
        }));
        GX_TRY(C.all_gather(send.all(), gath.all(), chunk * 4, C.st.data()));
        return in_turn(ctxs, ndev, [&](int d) -> int {
            for (int e = 0; e < ndev; e++) {
                const uint64_t own = ranges[e + 1] - ranges[e];
                if (own)
                    GX_HIP_TRY(hipMemcpyAsync(lab[d] + ranges[e], gath[d] + (uint64_t)e * chunk, own * 4,
                                              hipMemcpyDeviceToDevice, ctxs[d]->stream));
            }
            return GX_SUCCESS;
        });
    };
    for (int it = 0; it < iters; it++) {
        GX_TRY(in_turn(ctxs, ndev, [&](int d) -> int {
            GX_HIP_TRY(hipMemsetAsync(chg[d], 0, sizeof(int), ctxs[d]->stream));
            return gx_cdlp_part_step(part[d], lab[d], nxt[d], chg[d], ctxs[d]->stream);
        }));
        uint64_t tot = 0;
        GX_TRY(X.run(C, r, &tot));
        if (tot == 0) break;   // fixed point (LAGraph_cdlp.c:328-332)
    }
    X.report("cdlp_multi");
    GX_HIP_TRY(hipSetDevice(ctxs[0]->device));
    return download(ctxs[0], labels, lab[0], n, Xfer::Widen32);
}

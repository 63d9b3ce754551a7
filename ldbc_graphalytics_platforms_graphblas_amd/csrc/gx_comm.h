// gx_comm.h -- what the multi-device files share.  gx_comm.hip: the RCCL loader, gx_comm_* and the
// in-process clique with its cache; gx_pr_dist.hip: the cross-process PageRank runner (gx_pr_dist_*);
// gx_multi.hip: the one-process drivers (gx_*_multi).
#pragma once

#include <rccl/rccl.h>

#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "gx_pr.h"

struct gx_comm {
    gx_ctx *ctx = nullptr;
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
};

namespace gx {

// RCCL, opened lazily with dlopen: torch's copy when the process already has one (same soname,
// librccl.so.1), else ROCm's.  libgx itself has no link dependency on it, so the single-GPU
// executables never load RCCL.
struct Rccl {
    ncclResult_t (*get_unique_id)(ncclUniqueId *) = nullptr;
    ncclResult_t (*comm_init_rank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    ncclResult_t (*all_gather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t,
                               hipStream_t) = nullptr;
    ncclResult_t (*comm_init_all)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*reduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t,
                           hipStream_t) = nullptr;
    ncclResult_t (*group_start)() = nullptr;
    ncclResult_t (*group_end)() = nullptr;
    const char *(*error_string)(ncclResult_t) = nullptr;
    std::string error;
    bool ok = false;
};
const Rccl &rccl();
int rccl_fail(const char *what, ncclResult_t e);

#define GX_NCCL_TRY(what, expr)                                  \
    do {                                                         \
        ncclResult_t _r = (expr);                                \
        if (_r != ncclSuccess) return ::gx::rccl_fail(what, _r); \
    } while (0)

// ---- knobs, read once per call at the top of each entry point (the tests flip them between calls
// of one process) and nowhere else ----
struct MultiKnobs {
    int pieces;          // gx_pagerank_multi's pieces per device, 1..Clique::kMaxPieces
    bool by_blocks;      // ... its block partition instead of the interleaved one
    bool by_rows;        // ... its partitioned upload
    bool force_dense, force_sparse;   // GX_EXCHANGE = dense / sparse (WordExchange::run); anything else: by size
    bool plan_times;     // GX_PLAN_TIMES not 0 (pr.plan_times): the [multi] upload line and WordExchange::report on stderr
    PrKnobs pr;          // gx_pagerank_multi: the PageRank driver's own knobs (pr_knobs), passed to its plans
};
MultiKnobs multi_knobs(int ndev, bool directed, uint64_t nnz, int num_cus);

struct P2pKnobs {
    uint32_t polls = 1u << 22;   // GX_P2P_POLLS: polls before a k_p2p_wait gives up
    uint32_t put_blocks = 32;    // GX_P2P_BLOCKS: k_p2p_put's workgroups per peer (at least 1)
};
inline P2pKnobs p2p_knobs() {
    P2pKnobs k;
    if (const char *pl = std::getenv("GX_P2P_POLLS")) k.polls = (uint32_t)std::strtoul(pl, nullptr, 10);
    if (const char *pb = std::getenv("GX_P2P_BLOCKS")) k.put_blocks = std::max(1u, (uint32_t)std::strtoul(pb, nullptr, 10));
    return k;
}

// ---- the in-process clique ----
// The exchange among the ndev contexts of a one-process multi-device call (gx_*_multi).
// Contexts on distinct devices form an in-process RCCL clique (ncclCommInitAll; xGMI between
// MI355X GPUs), every collective issued for all devices inside one group.  Two or more
// contexts that all sit on ONE device are virtual devices (bin/exe/* with GX_NGPUS=N and
// GX_MULTI_SIM=1): the same call, partition and kernels per virtual device, with each
// collective restated as device-to-device copies with its semantics -- every context's
// stream waits for every sender before the copies, and for every receiver after them, so a
// send buffer is never rewritten while a peer still reads it.  That runs the N > 1 code of
// gx_pagerank_multi / gx_sssp_multi / gx_lcc_multi on a one-GPU box.
// One context alone keeps a size-1 RCCL clique, so the RCCL path stays exercised there too.
// The collectives take one pointer per device, in device order.
struct Clique {
    static constexpr int kMaxPieces = 8;   // gx_pagerank_multi's pieces per device (events below)
    int ndev = 0;
    std::vector<gx_ctx *> ctx;
    std::vector<ncclComm_t> comm;
    bool local = false;
    std::vector<hipEvent_t> ev_in, ev_out;
    // per device: its compute stream (the context's), a comm stream (the pieces' exchanges overlap
    // the next piece's SpMV on the compute stream), an event per piece (its SpMV done) and one
    // for the iteration's exchanges (made here, by gx_multi_prepare, outside the processing time:
    // creating a stream cost 10-30 ms inside a call)
    std::vector<hipStream_t> st, cs;
    std::vector<hipEvent_t> ev_piece, ev_comm;

    ~Clique();
    int init(gx_ctx *const *ctxs, int n);

    // local mode: every stream of s[0 .. ndev) waits for what every such stream has enqueued so far
    // (ev_in before an exchange's copies, ev_out after them)
    int fence(const std::vector<hipEvent_t> &ev, const hipStream_t *s);
    // recv[d][e * bytes, (e + 1) * bytes) = send[e][0, bytes) for every pair (ncclAllGather), on the
    // streams s[d]: st, or cs for gx_pagerank_multi's pieces
    int all_gather(const void *const *send, void *const *recv, size_t bytes, const hipStream_t *s);
    // all_gather of `bytes` count bytes per device on the compute streams, then device 0's gathered
    // copy to `host` (pinned, ndev * bytes) with its stream synchronised: a round's only host read
    int gather_counts(const void *const *count, void *const *counts, size_t bytes, void *host);
    // buf[0][i] = sum over d of buf[d][i], i < count (ncclReduce, root 0, in place there); the
    // other devices' buffers are left as they were in local mode, undefined under RCCL
    int reduce_sum_u64(void *const *buf, size_t count);
};
// The clique of a context list, cached until one of its contexts is freed (forget_cliques).
int get_clique(gx_ctx *const *ctxs, int n, std::shared_ptr<Clique> *out);

// Contexts must be all on distinct devices (an RCCL clique) or all on one device (virtual
// devices exchanging by copies); RCCL is required for the former and for one context.
int check_ctxs(gx_ctx *const *ctxs, int ndev, const char *who);
int check_multi(gx_ctx *const *ctxs, int ndev, const gx_csr *A, const char *who);

// Run fn(d) for every device on a host thread of its own (its device current, an equal share
// of the host's OpenMP threads), so the devices' uploads and plans overlap; one device runs
// inline.  Virtual devices (every context on one device) run one after the other on the
// calling thread, each drained before the next: they share the device's grow-only sort and
// plan scratch (gx_runtime.hip), which one host thread at a time may use.  The first
// failure's code and message come back on the calling thread.
int per_device(gx_ctx *const *ctxs, int ndev, const std::function<int(int)> &fn);

// The sequential sibling: fn(d) for every device in turn on the calling thread, that device
// current, nothing drained in between; stops at the first error.  What a round enqueues.
template <class F>
int in_turn(gx_ctx *const *ctxs, int ndev, F fn) {
    for (int d = 0; d < ndev; d++) {
        GX_HIP_TRY(hipSetDevice(ctxs[d]->device));
        GX_TRY(fn(d));
    }
    return GX_SUCCESS;
}

// ---- per-device state of a driver ----
// Owners release on their devices with the context's stream drained first.  A driver declares them
// so that they are released in this order on every exit: the per-device handles (splits, parts),
// the device buffers, the pinned host words, and last the graphs (MultiGraphs) the handles were
// made from -- that is, MultiGraphs first, then HostWords, PerDev, PerDevHandle.

// The graphs of a multi-device call: A on every device (gx_graph_create validates it there),
// freed with their contexts' streams drained.
struct MultiGraphs {
    std::vector<gx_graph *> g;
    explicit MultiGraphs(int ndev) : g(ndev, nullptr) {}
    ~MultiGraphs() {
        for (gx_graph *x : g) (void)gx_graph_free(x);
    }
};

// Pinned host words (the host's copy of a round's gathered counts).
struct HostFree {
    void operator()(void *p) const { (void)hipHostFree(p); }
};
template <class T>
using HostWords = std::unique_ptr<T[], HostFree>;
template <class T>
int host_words(gx_ctx *ctx, size_t count, HostWords<T> *out) {
    T *p = nullptr;
    GX_HIP_TRY(hipSetDevice(ctx->device));
    GX_HIP_TRY(hipHostMalloc((void **)&p, count * sizeof(T), hipHostMallocDefault));
    out->reset(p);
    return GX_SUCCESS;
}

// fn(d) for every device, that device current and its stream drained: how the owners release.
template <class F>
void each_drained(gx_ctx *const *ctxs, size_t ndev, F fn) {
    for (size_t d = 0; d < ndev; d++) {
        (void)hipSetDevice(ctxs[d]->device);
        (void)hipStreamSynchronize(ctxs[d]->stream);
        fn(d);
    }
}

// A per-device array of at least one element: the same size on every device.
template <class T>
struct PerDev {
    gx_ctx *const *ctxs;
    std::vector<DBuf<T>> b;
    std::vector<void *> raw;   // b[d].p, as the clique's collectives take them
    PerDev(gx_ctx *const *c, int ndev) : ctxs(c), b(ndev), raw(ndev, nullptr) {}
    ~PerDev() {
        each_drained(ctxs, b.size(), [&](size_t d) { b[d].release(); });
    }
    // the buffers of every device from the calling thread, or one device's (from per_device, that
    // device current)
    int alloc(uint64_t n) {
        return in_turn(ctxs, (int)b.size(), [&](int d) { return alloc_on(d, n); });
    }
    int alloc_on(int d, uint64_t n) {
        GX_TRY(b[d].alloc(std::max<uint64_t>(n, 1)));
        raw[d] = b[d].p;
        return GX_SUCCESS;
    }
    T *operator[](int d) const { return b[d].p; }
    void *const *all() const { return raw.data(); }
};

// A per-device opaque handle with its free function (gx_sssp_split, gx_lcc_part, gx_cdlp_part).
template <class H, int (*Free)(H *)>
struct PerDevHandle {
    gx_ctx *const *ctxs;
    std::vector<H *> h;
    PerDevHandle(gx_ctx *const *c, int ndev) : ctxs(c), h(ndev, nullptr) {}
    PerDevHandle(const PerDevHandle &) = delete;
    ~PerDevHandle() {
        each_drained(ctxs, h.size(), [&](size_t d) { (void)Free(h[d]); });
    }
    H *&operator[](int d) { return h[d]; }
};

}  // namespace gx

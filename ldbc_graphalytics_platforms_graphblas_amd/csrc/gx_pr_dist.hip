// gx_pr_dist.hip -- the device-driven partitioned PageRank loop across processes (gx_pr_dist_*).
//
// the pull matrix is 1-D row partitioned over the GPUs (one process per GPU)
// and the rank vector is all-gathered over xGMI every iteration.  The reference has no
// distributed path; this replaces the per-iteration GrB_mxv of LAGr_PageRankGX
// (pr.cpp:61) when it runs on several GPUs.
//
// gx_pr_part_step is one iteration of one rank (or piece); driving the iterations from
// Python costs one ctypes call plus one torch.distributed collective per piece and
// iteration (~60 us of host time each, measured), more than the per-rank SpMV at 8 GPUs.
// gx_pr_dist runs a whole PageRank from here instead: every kernel and every
// ncclAllGather is enqueued by one C call, and with `use_graph` the whole run (init, all
// iterations, all gathers) is captured once into a hipGraph and replayed, so the host
// cost per run is one graph launch.
//
// Pipelining (pr_partition.local_pieces): a rank owns `npieces` virtual ranks
// p * nranks + rank.  Piece p's chunks of all ranks form one contiguous slab of the
// exchanged vector, so each piece is gathered by its own ncclAllGather on the comm
// stream while the compute stream runs the next piece's SpMV:
//
//   compute: step(0) step(1) ... step(P-1) |wait comm| step(0) ...
//   comm   :        gather(0) gather(1) ... gather(P-1)|
//
// The vector is double-buffered (x_read / x_write) so a gather never overwrites values
// that a later piece of the same iteration still reads.
#include "gx_comm.h"

namespace gx {
namespace {

// ---- one-shot peer-to-peer exchange (gx_pr_dist_create_p2p) ----
// Every rank writes its chunk straight into every peer's exchanged vector (IPC-mapped over
// xGMI: one write per peer, all 7 links at once) instead of RCCL's ring, then raises an
// arrival flag in the peer's flag array.  Tokens grow monotonically across runs (a device
// run counter, so a replayed hipGraph raises new ones): token = run * kTok + step, step 0 =
// the initial exchange, it + 1 = iteration it's.  Memory model (LLVM AMDGPU, gfx942/950):
// the writer's data stores, a system-scope release, the flag store (system scope); the reader
// polls with system-scope loads and ends with a system-scope acquire, and the SpMV that
// reads x follows in stream order.  A wait gives up after `polls` polls (a dead or diverged
// peer), sets the error word and exits, so no wave spins forever.
constexpr uint64_t kTok = 1ull << 24;

__global__ void k_p2p_begin(uint64_t *seq) {
    if (threadIdx.x == 0) seq[0] += 1;
}

// chunk doubles of src into dst[q] + off for every rank q (blockIdx.y; chunk, off: multiples
// of 2), then flag[q][slot] = this run's token for `step`, raised by the workgroup that takes
// the last ticket (after every workgroup's system-scope release).  A few workgroups per peer:
// one xGMI link is ~50 GB/s, and the puts run beside the next piece's SpMV.
__global__ __launch_bounds__(256) void k_p2p_put(const double *__restrict__ src, uint64_t chunk,
                                                 double *const *__restrict__ dst, uint64_t off,
                                                 uint64_t *const *__restrict__ flags, uint64_t slot,
                                                 const uint64_t *seq, uint64_t step, uint32_t *ticket) {
    double2 *d = reinterpret_cast<double2 *>(dst[blockIdx.y] + off);
    const double2 *s = reinterpret_cast<const double2 *>(src);
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < chunk / 2; i += (uint64_t)gridDim.x * 256) d[i] = s[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // system scope: the stores reach the peers first
    __syncthreads();
    if (threadIdx.x != 0) return;
    const uint32_t all = gridDim.x * gridDim.y;
    if (__hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_SYSTEM) != all - 1) return;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    const uint64_t tok = seq[0] * kTok + step;
    for (uint32_t q = 0; q < gridDim.y; q++) __hip_atomic_store(flags[q] + slot, tok, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// flag[q][slot] = this run's token for `step`, for every rank q < world
__global__ void k_p2p_signal(uint64_t *const *__restrict__ flags, int world, uint64_t slot, const uint64_t *seq,
                             uint64_t step) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    const int q = threadIdx.x;
    if (q < world) __hip_atomic_store(flags[q] + slot, seq[0] * kTok + step, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// one wave: until flags[0 .. count) all hold at least (run - prev) * kTok + step
__global__ __launch_bounds__(64) void k_p2p_wait(const uint64_t *flags, int count, const uint64_t *seq, uint64_t step,
                                                 uint64_t prev, uint64_t *err, uint32_t polls) {
    const uint64_t target = (seq[0] - prev) * kTok + step;
    // after a timeout the run's results are void: later waits of the run do not poll again
    if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    for (uint32_t it = 0;; it++) {
        bool ok = true;
        for (int i = threadIdx.x; i < count; i += 64)
            ok = ok && __hip_atomic_load(flags + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) >= target;
        if (__all(ok)) break;
        if (it >= polls) {
            if (threadIdx.x == 0) __hip_atomic_store(err, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
        }
        __builtin_amdgcn_s_sleep(8);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");   // system scope
}

}  // namespace
}  // namespace gx

using namespace gx;

namespace {

struct PrDist {
    gx_ctx *ctx = nullptr;
    gx_comm *comm = nullptr;           // null: one rank (pieces exchanged by D2D copies)
    std::vector<PrPart *> pieces;
    int world = 1, rank = 0;           // real ranks
    uint64_t chunk = 0;
    DBuf<double> xa, xb;               // gathered vector, double-buffered
    std::vector<std::unique_ptr<DBuf<double>>> xl;   // per piece: its local chunk
    std::vector<std::unique_ptr<DBuf<double>>> ro;   // per piece: scores of its rows
    hipStream_t cs = nullptr;          // comm stream
    std::vector<hipEvent_t> ev_piece;
    hipEvent_t ev_comm = nullptr;
    hipGraphExec_t gexec = nullptr;
    hipGraph_t graph = nullptr;
    int g_iters = -1;
    bool g_first = false;              // the captured run starts with pr_first (ensure_first)
    hipStream_t g_stream = nullptr;
    hipStream_t last_stream = nullptr;
    // one-shot peer-to-peer exchange (gx_pr_dist_create_p2p): flags[p * world + q] = the last
    // token rank q raised here for piece p, flags[np * world + q] = q's end of its last run
    bool p2p = false, attached = false;
    DBuf<uint64_t> flags, seq;            // seq[0]: runs started; seq[1]: a wait timed out
    DBuf<double *> pxa, pxb;              // per rank: its xa / xb (ours for this rank)
    DBuf<uint64_t *> pfl;                 // per rank: its flags
    std::vector<void *> opened;           // the peers' IPC mappings
    DBuf<uint32_t> tickets;               // per piece: k_p2p_put's workgroup tickets
    P2pKnobs k;

    ~PrDist() {
        (void)hipSetDevice(ctx->device);
        (void)hipDeviceSynchronize();
        for (void *q : opened) (void)hipIpcCloseMemHandle(q);
        if (gexec) (void)hipGraphExecDestroy(gexec);
        if (graph) (void)hipGraphDestroy(graph);
        for (hipEvent_t e : ev_piece) (void)hipEventDestroy(e);
        if (ev_comm) (void)hipEventDestroy(ev_comm);
        if (cs) (void)hipStreamDestroy(cs);
    }

    size_t span() const { return chunk * (size_t)world; }   // one piece's slab

    int np() const { return (int)pieces.size(); }

    // exchange piece p's local chunk into slab p of `x` (after what s has enqueued so far);
    // `step` names the exchange for the peer-to-peer flags
    int gather(int p, double *x, hipStream_t s, uint64_t step) {
        double *dst = x + (size_t)p * span();
        if (p2p) {
            GX_HIP_TRY(hipEventRecord(ev_piece[p], s));
            GX_HIP_TRY(hipStreamWaitEvent(cs, ev_piece[p], 0));
            const unsigned blocks = (unsigned)std::min<uint64_t>(k.put_blocks, (chunk / 2 + 255) / 256);
            hipLaunchKernelGGL(k_p2p_put, dim3(std::max(blocks, 1u), world), dim3(256), 0, cs, xl[p]->p, chunk,
                               x == xa.p ? pxa.p : pxb.p, (uint64_t)p * span() + (uint64_t)rank * chunk, pfl.p,
                               (uint64_t)p * world + rank, seq.p, step, tickets.p + p);
            return check_launch("k_p2p_put");
        }
        if (!comm) {
            GX_HIP_TRY(hipMemcpyAsync(dst, xl[p]->p, chunk * sizeof(double), hipMemcpyDeviceToDevice, s));
            return GX_SUCCESS;
        }
        GX_HIP_TRY(hipEventRecord(ev_piece[p], s));
        GX_HIP_TRY(hipStreamWaitEvent(cs, ev_piece[p], 0));
        GX_NCCL_TRY("ncclAllGather", rccl().all_gather(xl[p]->p, dst, chunk, ncclFloat64, comm->comm, cs));
        return GX_SUCCESS;
    }

    // compute stream waits for every gather issued so far (peer-to-peer: and for every
    // rank's chunks of exchange `step` to have arrived here)
    int join(hipStream_t s, uint64_t step) {
        if (!comm && !p2p) return GX_SUCCESS;
        GX_HIP_TRY(hipEventRecord(ev_comm, cs));
        GX_HIP_TRY(hipStreamWaitEvent(s, ev_comm, 0));
        if (p2p) {
            hipLaunchKernelGGL(k_p2p_wait, dim3(1), dim3(64), 0, s, flags.p, np() * world, seq.p, step, (uint64_t)0,
                               seq.p + 1, k.polls);
            GX_TRY(check_launch("k_p2p_wait"));
        }
        return GX_SUCCESS;
    }

    // The first iteration in closed form (PrPart::S) for a runner that exchanges by device copies:
    // every piece's S, built once by one iteration in S mode over the same buffers and exchange as
    // a run's first.  Never under capture: run() calls this first.  False: a piece has the closed
    // form off (GX_PR_FIRST=0, or no memory for its S) and the runs start with pr_init as before.
    int ensure_first(hipStream_t s, bool *ok) {
        *ok = false;
        if (comm || p2p) return GX_SUCCESS;
        const int np = (int)pieces.size();
        bool ready = true;
        for (int p = 0; p < np; p++) {
            if (!pr_first_alloc(pieces[p])) return GX_SUCCESS;
            ready = ready && pieces[p]->first_ready;
        }
        *ok = true;
        if (ready) return GX_SUCCESS;
        if (np == 1) return pr_first_build(pieces[0], xa.p, xb.p, s);
        for (int p = 0; p < np; p++) GX_TRY(pr_first_init(pieces[p], xl[p]->p, s));
        for (int p = 0; p < np; p++) GX_TRY(gather(p, xa.p, s, 0));
        for (int p = 0; p < np; p++) GX_TRY(pr_first_step(pieces[p], xa.p, xl[p]->p, s));
        return GX_SUCCESS;
    }

    int enqueue(int iters, hipStream_t s, bool first) {
        const int np = (int)pieces.size();
        const bool swap_only = !comm && !p2p && np == 1;   // one rank, one piece: no exchange at all
        double *xr = xa.p, *xw = xb.p;
        if (p2p) {
            // a new run; its first exchange overwrites the peers' xa, so every peer must have
            // finished reading it in the previous run (their end-of-run tokens)
            hipLaunchKernelGGL(k_p2p_begin, dim3(1), dim3(64), 0, s, seq.p);
            GX_TRY(check_launch("k_p2p_begin"));
            hipLaunchKernelGGL(k_p2p_wait, dim3(1), dim3(64), 0, s, flags.p + (size_t)np * world, world, seq.p,
                               (uint64_t)0, (uint64_t)1, seq.p + 1, k.polls);
            GX_TRY(check_launch("k_p2p_wait"));
        }
        if (first) {
            // pr_init and iteration 1 as one streaming kernel per piece (device copies only: no join)
            uint64_t nd_total = 0;
            for (int p = 0; p < np; p++) nd_total += pieces[p]->nd;
            const bool only = iters == 1;
            for (int p = 0; p < np; p++)
                GX_TRY(pr_first(pieces[p], nd_total, swap_only ? xr : xl[p]->p, only ? ro[p]->p : nullptr, s));
            if (!swap_only && !only)
                for (int p = 0; p < np; p++) GX_TRY(gather(p, xr, s, 1));
        } else {
            for (int p = 0; p < np; p++) GX_TRY(pr_init(pieces[p], swap_only ? xr : xl[p]->p, s));
            if (!swap_only) {
                for (int p = 0; p < np; p++) GX_TRY(gather(p, xr, s, 0));
                GX_TRY(join(s, 0));
            }
        }
        for (int it = first ? 1 : 0; it < iters; it++) {
            const bool last = it == iters - 1;
            for (int p = 0; p < np; p++) {
                double *out = swap_only ? xw : xl[p]->p;
                GX_TRY(pr_step(pieces[p], xr, out, last ? ro[p]->p : nullptr, s));
                if (!last && !swap_only) GX_TRY(gather(p, xw, s, (uint64_t)it + 1));
            }
            if (last) break;
            if (!swap_only) GX_TRY(join(s, (uint64_t)it + 1));
            std::swap(xr, xw);
        }
        if (p2p) {   // this rank is done reading its vectors: the end-of-run token to every rank
            hipLaunchKernelGGL(k_p2p_signal, dim3(1), dim3(64), 0, s, pfl.p, world, (uint64_t)np * world + rank, seq.p,
                               (uint64_t)0);
            GX_TRY(check_launch("k_p2p_signal"));
        }
        return GX_SUCCESS;
    }

    int run(int iters, bool use_graph, hipStream_t s) {
        last_stream = s;
        // before any capture: the captured graph holds k_pr_first and iters - 1 iterations
        bool first = false;
        GX_TRY(ensure_first(s, &first));
        // kernel timing brackets launches with events, which a replayed graph would not
        // refresh: timed runs go through direct launches
        if (!use_graph || ctx->timing) return enqueue(iters, s, first);
        if (!gexec || g_iters != iters || g_stream != s || g_first != first) {
            if (gexec) (void)hipGraphExecDestroy(gexec);
            if (graph) (void)hipGraphDestroy(graph);
            gexec = nullptr;
            graph = nullptr;
            GX_HIP_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            const int rc = enqueue(iters, s, first);
            hipGraph_t g = nullptr;
            const hipError_t e = hipStreamEndCapture(s, &g);
            if (rc != GX_SUCCESS) {
                if (g) (void)hipGraphDestroy(g);
                return rc;
            }
            if (e != hipSuccess) return fail(GX_DEVICE_ERROR, std::string("PageRank capture: ") + hipGetErrorString(e));
            graph = g;
            GX_HIP_TRY(hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0));
            g_iters = iters;
            g_stream = s;
            g_first = first;
        }
        GX_HIP_TRY(hipGraphLaunch(gexec, s));
        return GX_SUCCESS;
    }
};

}  // namespace

struct gx_pr_dist {
    PrDist d;
};

namespace {

int dist_create(gx_comm *comm, int world, int rank, bool p2p, gx_pr_part *const *parts, int npieces, gx_pr_dist **out) {
    const P2pKnobs knobs = p2p_knobs();
    // its own HIP calls fail as "gx_pr_dist_create: <hip error>"
    auto hip = [](hipError_t e) {
        return e == hipSuccess ? (int)GX_SUCCESS : fail(GX_DEVICE_ERROR, std::string("gx_pr_dist_create: ") + hipGetErrorString(e));
    };
    if (!parts || !out || npieces < 1) return fail(GX_NULL_POINTER, "gx_pr_dist_create: null argument");
    PrPart *p0 = reinterpret_cast<PrPart *>(parts[0]);
    if (!p0) return fail(GX_NULL_POINTER, "gx_pr_dist_create: null piece");
    if (comm && comm->ctx != p0->ctx) return fail(GX_INVALID_VALUE, "gx_pr_dist_create: comm and pieces on different contexts");
    for (int p = 0; p < npieces; p++) {
        PrPart *q = reinterpret_cast<PrPart *>(parts[p]);
        if (!q) return fail(GX_NULL_POINTER, "gx_pr_dist_create: null piece");
        if (q->ctx != p0->ctx || q->chunk != p0->chunk || q->n_global != p0->n_global)
            return fail(GX_INVALID_VALUE, "gx_pr_dist_create: pieces of different partitions");
        if (q->nranks != world * npieces || q->rank != p * world + rank)
            return fail(GX_INVALID_VALUE, "gx_pr_dist_create: piece p must be virtual rank p * nranks + rank "
                                          "of a partition into nranks * npieces ranges");
    }
    gx_ctx *ctx = p0->ctx;
    GX_HIP_TRY(hipSetDevice(ctx->device));
    auto h = std::make_unique<gx_pr_dist>();   // ~PrDist on every failure below
    PrDist &d = h->d;
    d.ctx = ctx;
    d.comm = comm;
    d.world = world;
    d.rank = rank;
    d.chunk = p0->chunk;
    d.k = knobs;
    for (int p = 0; p < npieces; p++) d.pieces.push_back(reinterpret_cast<PrPart *>(parts[p]));
    const size_t full = d.chunk * (size_t)world * (size_t)npieces;
    GX_TRY(d.xa.alloc(full));
    GX_TRY(d.xb.alloc(full));
    for (int p = 0; p < npieces; p++) {
        d.xl.emplace_back(new DBuf<double>());
        d.ro.emplace_back(new DBuf<double>());
    }
    for (int p = 0; p < npieces; p++) {
        GX_TRY(d.xl[p]->alloc(d.chunk));
        GX_TRY(d.ro[p]->alloc(std::max<uint64_t>(d.pieces[p]->rows, 1)));
        // the padding slots (the kernel's zero column among them) stay 0.0 through the exchange
        if (hipMemset(d.xl[p]->p, 0, d.chunk * sizeof(double)) != hipSuccess) return fail(GX_DEVICE_ERROR, "hipMemset");
    }
    GX_TRY(hip(hipMemset(d.xa.p, 0, full * sizeof(double))));
    GX_TRY(hip(hipMemset(d.xb.p, 0, full * sizeof(double))));
    if (p2p) {
        d.p2p = true;
        const size_t nf = (size_t)(npieces + 1) * world;
        GX_TRY(d.flags.alloc(nf));
        GX_TRY(d.seq.alloc(2));
        GX_TRY(d.pxa.alloc(world));
        GX_TRY(d.pxb.alloc(world));
        GX_TRY(d.pfl.alloc(world));
        GX_TRY(d.tickets.alloc(npieces));
        GX_TRY(hip(hipMemset(d.tickets.p, 0, npieces * sizeof(uint32_t))));
        GX_TRY(hip(hipMemset(d.flags.p, 0, nf * sizeof(uint64_t))));
        GX_TRY(hip(hipMemset(d.seq.p, 0, 2 * sizeof(uint64_t))));
    }
    if (comm || p2p) {
        GX_TRY(hip(hipStreamCreateWithFlags(&d.cs, hipStreamNonBlocking)));
        d.ev_piece.assign(npieces, nullptr);
        for (int p = 0; p < npieces; p++) GX_TRY(hip(hipEventCreateWithFlags(&d.ev_piece[p], hipEventDisableTiming)));
        GX_TRY(hip(hipEventCreateWithFlags(&d.ev_comm, hipEventDisableTiming)));
    }
    *out = h.release();
    return GX_SUCCESS;
}

}  // namespace

extern "C" int gx_pr_dist_create(gx_comm *comm, gx_pr_part *const *parts, int npieces, gx_pr_dist **out) {
    return dist_create(comm, comm ? comm->nranks : 1, comm ? comm->rank : 0, false, parts, npieces, out);
}

// IPC handles of this rank: xa, xb, flags (hipIpcMemHandle_t each)
extern "C" int gx_pr_dist_create_p2p(int nranks, int rank, gx_pr_part *const *parts, int npieces, uint8_t *handle,
                                     gx_pr_dist **out) {
    if (!handle || !out) return fail(GX_NULL_POINTER, "gx_pr_dist_create_p2p: null argument");
    if (nranks < 1 || rank < 0 || rank >= nranks || nranks > 64)
        return fail(GX_INVALID_VALUE, "gx_pr_dist_create_p2p: bad rank/nranks (at most 64 ranks)");
    static_assert(3 * sizeof(hipIpcMemHandle_t) <= GX_P2P_HANDLE_BYTES, "handle bytes");
    gx_pr_dist *h = nullptr;
    GX_TRY(dist_create(nullptr, nranks, rank, true, parts, npieces, &h));
    PrDist &d = h->d;
    std::memset(handle, 0, GX_P2P_HANDLE_BYTES);
    hipIpcMemHandle_t m[3];
    void *bufs[3] = {d.xa.p, d.xb.p, d.flags.p};
    for (int k = 0; k < 3; k++) {
        const hipError_t e = hipIpcGetMemHandle(&m[k], bufs[k]);
        if (e != hipSuccess) {
            delete h;
            return fail(GX_DEVICE_ERROR, std::string("hipIpcGetMemHandle: ") + hipGetErrorString(e));
        }
        std::memcpy(handle + k * sizeof(hipIpcMemHandle_t), &m[k], sizeof(hipIpcMemHandle_t));
    }
    *out = h;
    return GX_SUCCESS;
}

// handles: nranks * GX_P2P_HANDLE_BYTES in rank order (this rank's own entry is not opened)
extern "C" int gx_pr_dist_p2p_attach(gx_pr_dist *h, const uint8_t *handles) {
    if (!h) return fail(GX_NULL_POINTER, "gx_pr_dist_p2p_attach: null argument");
    PrDist &d = h->d;
    if (!d.p2p) return fail(GX_INVALID_OBJECT, "gx_pr_dist_p2p_attach: not a peer-to-peer runner");
    if (d.attached) return fail(GX_INVALID_OBJECT, "gx_pr_dist_p2p_attach: already attached");
    if (!handles && d.world > 1) return fail(GX_NULL_POINTER, "gx_pr_dist_p2p_attach: null handles");
    GX_HIP_TRY(hipSetDevice(d.ctx->device));
    std::vector<double *> a(d.world), b(d.world);
    std::vector<uint64_t *> f(d.world);
    for (int q = 0; q < d.world; q++) {
        if (q == d.rank) {
            a[q] = d.xa.p;
            b[q] = d.xb.p;
            f[q] = d.flags.p;
            continue;
        }
        void *ptr[3] = {nullptr, nullptr, nullptr};
        for (int k = 0; k < 3; k++) {
            hipIpcMemHandle_t m;
            std::memcpy(&m, handles + (size_t)q * GX_P2P_HANDLE_BYTES + k * sizeof(hipIpcMemHandle_t), sizeof(m));
            const hipError_t e = hipIpcOpenMemHandle(&ptr[k], m, hipIpcMemLazyEnablePeerAccess);
            if (e != hipSuccess)
                return fail(GX_DEVICE_ERROR, "hipIpcOpenMemHandle (rank " + std::to_string(q) + "): " + hipGetErrorString(e));
            d.opened.push_back(ptr[k]);
        }
        a[q] = static_cast<double *>(ptr[0]);
        b[q] = static_cast<double *>(ptr[1]);
        f[q] = static_cast<uint64_t *>(ptr[2]);
    }
    GX_HIP_TRY(hipMemcpy(d.pxa.p, a.data(), d.world * sizeof(double *), hipMemcpyHostToDevice));
    GX_HIP_TRY(hipMemcpy(d.pxb.p, b.data(), d.world * sizeof(double *), hipMemcpyHostToDevice));
    GX_HIP_TRY(hipMemcpy(d.pfl.p, f.data(), d.world * sizeof(uint64_t *), hipMemcpyHostToDevice));
    d.attached = true;
    return GX_SUCCESS;
}

extern "C" int gx_pr_dist_run(gx_pr_dist *h, int iters, int use_graph, void *stream) {
    if (!h) return fail(GX_NULL_POINTER, "gx_pr_dist_run: null argument");
    if (iters < 1) return fail(GX_INVALID_VALUE, "gx_pr_dist_run: iters must be >= 1");
    PrDist &d = h->d;
    if (d.p2p && !d.attached) return fail(GX_INVALID_OBJECT, "gx_pr_dist_run: peer-to-peer runner not attached");
    // a token is run * kTok + step with step <= iters: a longer run would raise tokens that
    // satisfy the next run's waits early
    if (d.p2p && (uint64_t)iters >= kTok - 1) return fail(GX_INVALID_VALUE, "gx_pr_dist_run: at most 2^24 - 2 iterations with the peer-to-peer exchange");
    GX_HIP_TRY(hipSetDevice(d.ctx->device));
    return d.run(iters, use_graph != 0, stream ? (hipStream_t)stream : d.ctx->stream);
}

extern "C" int gx_pr_dist_scores(gx_pr_dist *h, int piece, double *scores) {
    if (!h || !scores) return fail(GX_NULL_POINTER, "gx_pr_dist_scores: null argument");
    PrDist &d = h->d;
    if (piece < 0 || piece >= (int)d.pieces.size()) return fail(GX_INVALID_INDEX, "gx_pr_dist_scores: bad piece");
    GX_HIP_TRY(hipSetDevice(d.ctx->device));
    if (d.last_stream) GX_HIP_TRY(hipStreamSynchronize(d.last_stream));
    if (d.p2p) {
        uint64_t err = 0;
        GX_HIP_TRY(hipMemcpy(&err, d.seq.p + 1, sizeof(err), hipMemcpyDeviceToHost));
        if (err) return fail(GX_DEVICE_ERROR, "gx_pr_dist_scores: a peer-to-peer wait timed out (a peer stopped or diverged)");
    }
    const uint64_t rows = d.pieces[piece]->rows;
    if (rows) GX_HIP_TRY(hipMemcpy(scores, d.ro[piece]->p, rows * sizeof(double), hipMemcpyDeviceToHost));
    return GX_SUCCESS;
}

extern "C" int gx_pr_dist_free(gx_pr_dist *h) {
    if (!h) return GX_SUCCESS;
    (void)hipSetDevice(h->d.ctx->device);
    (void)hipDeviceSynchronize();
    delete h;
    return GX_SUCCESS;
}

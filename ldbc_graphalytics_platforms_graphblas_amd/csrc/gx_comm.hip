// gx_comm.hip -- the RCCL loader and communicator (gx_comm_*), and the in-process clique of the
// one-process multi-device calls with its cache (gx_multi_prepare).  gx_comm.h says who uses them.
#include <dlfcn.h>

#include <algorithm>
#include <mutex>
#include <thread>

#include "gx_comm.h"

namespace gx {

const Rccl &rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);   // torch's, if loaded
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) {
            const char *e = dlerror();
            r.error = std::string("cannot load librccl.so.1: ") + (e ? e : "?");
            return;
        }
        r.get_unique_id = reinterpret_cast<decltype(r.get_unique_id)>(dlsym(h, "ncclGetUniqueId"));
        r.comm_init_rank = reinterpret_cast<decltype(r.comm_init_rank)>(dlsym(h, "ncclCommInitRank"));
        r.comm_destroy = reinterpret_cast<decltype(r.comm_destroy)>(dlsym(h, "ncclCommDestroy"));
        r.all_gather = reinterpret_cast<decltype(r.all_gather)>(dlsym(h, "ncclAllGather"));
        r.error_string = reinterpret_cast<decltype(r.error_string)>(dlsym(h, "ncclGetErrorString"));
        r.comm_init_all = reinterpret_cast<decltype(r.comm_init_all)>(dlsym(h, "ncclCommInitAll"));
        r.group_start = reinterpret_cast<decltype(r.group_start)>(dlsym(h, "ncclGroupStart"));
        r.reduce = reinterpret_cast<decltype(r.reduce)>(dlsym(h, "ncclReduce"));
        r.group_end = reinterpret_cast<decltype(r.group_end)>(dlsym(h, "ncclGroupEnd"));
        r.ok = r.get_unique_id && r.comm_init_rank && r.comm_destroy && r.all_gather && r.error_string &&
               r.comm_init_all && r.group_start && r.group_end && r.reduce;
        if (!r.ok) r.error = "librccl.so.1 lacks an expected entry point";
    });
    return r;
}

int rccl_fail(const char *what, ncclResult_t e) {
    return fail(GX_DEVICE_ERROR, std::string(what) + ": " + rccl().error_string(e));
}

}  // namespace gx

using namespace gx;

extern "C" int gx_comm_unique_id(uint8_t *id) {
    if (!id) return fail(GX_NULL_POINTER, "gx_comm_unique_id: null argument");
    const Rccl &r = rccl();
    if (!r.ok) return fail(GX_NOT_IMPLEMENTED, r.error);
    ncclUniqueId u;
    GX_NCCL_TRY("ncclGetUniqueId", r.get_unique_id(&u));
    std::memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
    return GX_SUCCESS;
}

extern "C" int gx_comm_create(gx_ctx *ctx, int nranks, int rank, const uint8_t *id, gx_comm **out) {
    if (!ctx || !id || !out) return fail(GX_NULL_POINTER, "gx_comm_create: null argument");
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(GX_INVALID_VALUE, "gx_comm_create: bad rank/nranks");
    const Rccl &r = rccl();
    if (!r.ok) return fail(GX_NOT_IMPLEMENTED, r.error);
    GX_HIP_TRY(hipSetDevice(ctx->device));
    ncclUniqueId u;
    std::memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
    ncclComm_t c = nullptr;
    GX_NCCL_TRY("ncclCommInitRank", r.comm_init_rank(&c, nranks, u, rank));
    auto *cm = new gx_comm();
    cm->ctx = ctx;
    cm->comm = c;
    cm->nranks = nranks;
    cm->rank = rank;
    *out = cm;
    return GX_SUCCESS;
}

extern "C" int gx_comm_free(gx_comm *comm) {
    if (!comm) return GX_SUCCESS;
    (void)hipSetDevice(comm->ctx->device);
    (void)hipDeviceSynchronize();
    if (comm->comm) (void)rccl().comm_destroy(comm->comm);
    delete comm;
    return GX_SUCCESS;
}

// ---------------------------------------------------------------- one process, N GPUs

namespace {

// Adds src into dst (n words): the local reduction of Clique::reduce_sum_u64.
__global__ __launch_bounds__(256) void k_add_u64(uint64_t *__restrict__ dst, const uint64_t *__restrict__ src, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) dst[i] += src[i];
}

}  // namespace

namespace gx {

static bool one_device(gx_ctx *const *ctxs, int ndev) {
    for (int d = 1; d < ndev; d++)
        if (ctxs[d]->device != ctxs[0]->device) return false;
    return true;
}

Clique::~Clique() {
    for (int d = 0; d < ndev; d++) {
        (void)hipSetDevice(ctx[d]->device);
        (void)hipStreamSynchronize(ctx[d]->stream);
        if (d < (int)cs.size() && cs[d]) (void)hipStreamSynchronize(cs[d]);
    }
    for (ncclComm_t c : comm)
        if (c) (void)rccl().comm_destroy(c);
    for (hipEvent_t e : ev_in) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_out) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_piece)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_comm)
        if (e) (void)hipEventDestroy(e);
    for (int d = 0; d < (int)cs.size(); d++)
        if (cs[d]) {
            (void)hipSetDevice(ctx[d]->device);
            (void)hipStreamDestroy(cs[d]);
        }
}

int Clique::init(gx_ctx *const *ctxs, int n) {
    ndev = n;
    ctx.assign(ctxs, ctxs + n);
    local = n > 1 && one_device(ctxs, n);
    st.resize(n);
    for (int d = 0; d < n; d++) st[d] = ctxs[d]->stream;
    cs.assign(n, nullptr);
    ev_comm.assign(n, nullptr);
    ev_piece.assign((size_t)n * kMaxPieces, nullptr);
    for (int d = 0; d < n; d++) {
        GX_HIP_TRY(hipSetDevice(ctxs[d]->device));
        GX_HIP_TRY(hipStreamCreateWithFlags(&cs[d], hipStreamNonBlocking));
        GX_HIP_TRY(hipEventCreateWithFlags(&ev_comm[d], hipEventDisableTiming));
        for (int p = 0; p < kMaxPieces; p++)
            GX_HIP_TRY(hipEventCreateWithFlags(&ev_piece[(size_t)d * kMaxPieces + p], hipEventDisableTiming));
    }
    if (!local) {
        std::vector<int> devs(n);
        for (int d = 0; d < n; d++) devs[d] = ctxs[d]->device;
        comm.assign(n, nullptr);
        GX_NCCL_TRY("ncclCommInitAll", rccl().comm_init_all(comm.data(), n, devs.data()));
        return GX_SUCCESS;
    }
    GX_HIP_TRY(hipSetDevice(ctxs[0]->device));
    ev_in.assign(n, nullptr);
    ev_out.assign(n, nullptr);
    for (int d = 0; d < n; d++) {
        GX_HIP_TRY(hipEventCreateWithFlags(&ev_in[d], hipEventDisableTiming));
        GX_HIP_TRY(hipEventCreateWithFlags(&ev_out[d], hipEventDisableTiming));
    }
    return GX_SUCCESS;
}

int Clique::fence(const std::vector<hipEvent_t> &ev, const hipStream_t *s) {
    for (int e = 0; e < ndev; e++) GX_HIP_TRY(hipEventRecord(ev[e], s[e]));
    for (int d = 0; d < ndev; d++)
        for (int e = 0; e < ndev; e++)
            if (e != d) GX_HIP_TRY(hipStreamWaitEvent(s[d], ev[e], 0));
    return GX_SUCCESS;
}

// One RCCL call per device inside one group; the group is closed on the error path too.
template <class F>
static int grouped(const Clique &C, const char *what, F call) {
    const Rccl &r = rccl();
    GX_NCCL_TRY("ncclGroupStart", r.group_start());
    for (int d = 0; d < C.ndev; d++) {
        const ncclResult_t e = call(r, d);
        if (e != ncclSuccess) {
            (void)r.group_end();
            return rccl_fail(what, e);
        }
    }
    GX_NCCL_TRY("ncclGroupEnd", r.group_end());
    return GX_SUCCESS;
}

int Clique::all_gather(const void *const *send, void *const *recv, size_t bytes, const hipStream_t *s) {
    if (local) {
        GX_HIP_TRY(hipSetDevice(ctx[0]->device));
        GX_TRY(fence(ev_in, s));
        for (int d = 0; d < ndev; d++)
            for (int e = 0; e < ndev; e++)
                GX_HIP_TRY(hipMemcpyAsync(static_cast<char *>(recv[d]) + (size_t)e * bytes, send[e], bytes,
                                          hipMemcpyDeviceToDevice, s[d]));
        return fence(ev_out, s);
    }
    return grouped(*this, "ncclAllGather", [&](const Rccl &r, int d) {
        return r.all_gather(send[d], recv[d], bytes, ncclUint8, comm[d], s[d]);
    });
}

int Clique::gather_counts(const void *const *count, void *const *counts, size_t bytes, void *host) {
    GX_TRY(all_gather(count, counts, bytes, st.data()));
    GX_HIP_TRY(hipSetDevice(ctx[0]->device));
    GX_HIP_TRY(hipMemcpyAsync(host, counts[0], (size_t)ndev * bytes, hipMemcpyDeviceToHost, st[0]));
    GX_HIP_TRY(hipStreamSynchronize(st[0]));
    return GX_SUCCESS;
}

int Clique::reduce_sum_u64(void *const *buf, size_t count) {
    if (local) {
        GX_HIP_TRY(hipSetDevice(ctx[0]->device));
        GX_TRY(fence(ev_in, st.data()));
        for (int e = 1; e < ndev && count; e++) {
            hipLaunchKernelGGL(k_add_u64, dim3(grid_for(count, 256, 8192)), dim3(256), 0, st[0],
                               static_cast<uint64_t *>(buf[0]), static_cast<const uint64_t *>(buf[e]), (uint64_t)count);
            GX_TRY(check_launch("k_add_u64"));
        }
        return fence(ev_out, st.data());
    }
    return grouped(*this, "ncclReduce", [&](const Rccl &r, int d) {
        return r.reduce(buf[d], buf[d], count, ncclUint64, ncclSum, 0, comm[d], st[d]);
    });
}

// The cliques of gx_*_multi, one per context list, kept until one of its contexts is freed
// (forget_cliques from gx_free): ncclCommInitAll took ~0.5 s of every call.  gx_multi_prepare
// makes one ahead of the caller's timed region, as gx_init does for a context.
struct CliqueCache {
    std::mutex mu;
    std::vector<std::pair<std::vector<gx_ctx *>, std::shared_ptr<Clique>>> list;
};
// never destroyed: an exit-time destructor would tear down communicators after the HIP runtime
static CliqueCache &cliques() {
    static CliqueCache *c = new CliqueCache;
    return *c;
}

int get_clique(gx_ctx *const *ctxs, int n, std::shared_ptr<Clique> *out) {
    CliqueCache &cc = cliques();
    std::lock_guard<std::mutex> lk(cc.mu);
    const std::vector<gx_ctx *> key(ctxs, ctxs + n);
    for (auto &e : cc.list)
        if (e.first == key) {
            *out = e.second;
            return GX_SUCCESS;
        }
    auto c = std::make_shared<Clique>();
    GX_TRY(c->init(ctxs, n));
    cc.list.push_back({key, c});
    *out = c;
    return GX_SUCCESS;
}

void forget_cliques(gx_ctx *ctx) {
    std::vector<std::shared_ptr<Clique>> drop;  // destroyed outside the lock
    CliqueCache &cc = cliques();
    {
        std::lock_guard<std::mutex> lk(cc.mu);
        for (size_t i = 0; i < cc.list.size();) {
            auto &k = cc.list[i].first;
            if (std::find(k.begin(), k.end(), ctx) != k.end()) {
                drop.push_back(std::move(cc.list[i].second));
                cc.list.erase(cc.list.begin() + i);
            } else {
                i++;
            }
        }
    }
}

int per_device(gx_ctx *const *ctxs, int ndev, const std::function<int(int)> &fn) {
    if (ndev == 1 || one_device(ctxs, ndev)) {
        for (int d = 0; d < ndev; d++) {
            GX_HIP_TRY(hipSetDevice(ctxs[d]->device));
            const int rc = fn(d);
            if (rc != GX_SUCCESS)
                return ndev == 1 ? rc : fail(rc, "virtual device " + std::to_string(d) + ": " + gx_last_error());
            GX_HIP_TRY(hipStreamSynchronize(ctxs[d]->stream));
        }
        return GX_SUCCESS;
    }
    std::vector<int> rc(ndev, GX_SUCCESS);
    std::vector<std::string> msg(ndev);
    std::vector<std::thread> th;
    const int share = std::max(1, host_threads() / ndev);
    for (int d = 0; d < ndev; d++)
        th.emplace_back([&, d] {
            host_set_threads(share);
            const hipError_t e = hipSetDevice(ctxs[d]->device);
            rc[d] = e == hipSuccess ? fn(d) : fail(GX_DEVICE_ERROR, hipGetErrorString(e));
            if (rc[d] != GX_SUCCESS) msg[d] = gx_last_error();
        });
    for (auto &t : th) t.join();
    for (int d = 0; d < ndev; d++)
        if (rc[d] != GX_SUCCESS) return fail(rc[d], "device " + std::to_string(ctxs[d]->device) + ": " + msg[d]);
    return GX_SUCCESS;
}

int check_multi(gx_ctx *const *ctxs, int ndev, const gx_csr *A, const char *who) {
    if (!ctxs || !A || (A->nnz && !A->colidx) || !A->rowptr) return fail(GX_NULL_POINTER, std::string(who) + ": null argument");
    return check_ctxs(ctxs, ndev, who);
}

int check_ctxs(gx_ctx *const *ctxs, int ndev, const char *who) {
    if (!ctxs) return fail(GX_NULL_POINTER, std::string(who) + ": null argument");
    if (ndev < 1) return fail(GX_INVALID_VALUE, std::string(who) + ": ndev < 1");
    for (int d = 0; d < ndev; d++)
        if (!ctxs[d]) return fail(GX_NULL_POINTER, std::string(who) + ": null context");
    for (int d = 0; d < ndev; d++)
        for (int e = 0; e < d; e++)
            if (ctxs[d] == ctxs[e]) return fail(GX_INVALID_VALUE, std::string(who) + ": a context passed twice");
    if (ndev > 1 && one_device(ctxs, ndev)) return GX_SUCCESS;
    for (int d = 0; d < ndev; d++)
        for (int e = 0; e < d; e++)
            if (ctxs[d]->device == ctxs[e]->device)
                return fail(GX_INVALID_VALUE, std::string(who) + ": contexts must be on distinct devices, or all on one");
    const Rccl &r = rccl();
    if (!r.ok) return fail(GX_NOT_IMPLEMENTED, r.error);
    return GX_SUCCESS;
}

}  // namespace gx

extern "C" int gx_multi_prepare(gx_ctx *const *ctxs, int ndev) {
    GX_TRY(check_ctxs(ctxs, ndev, "gx_multi_prepare"));
    std::shared_ptr<Clique> clique;
    return get_clique(ctxs, ndev, &clique);
}

// ngp_host_comm.h — the one collective: librccl opened at run time (RcclApi, load_rccl), ngp_comm,
// ngp_comm_unique_id / _create / _destroy, ngp_shard, ngp_weights_unpad_normalize and
// ngp_weights_allgather_normalize.
// Included from ngp_api.hip behind that file's own code (HIPCHK; ngp_ctx: mu, device, stream, alloc /
// release, drop_cache, ws_drop; DevCall; <dlfcn.h>) and behind ngp_host_mixture.h
// (weights_normalize_strided).
#pragma once

// ---------------------------------------------------------------------------------------
// The one collective of the path (north_star: RCCL over xGMI only for the particle-weight
// normalisation / resample reduction), for hosts that bring no collective library of their own
// (the Julia shim; the Python mirror uses torch.distributed, whose "nccl" backend is this same
// RCCL).  librccl is opened at run time: the library has no link-time dependency on it and the
// entry points answer NGP_ERR_UNAVAILABLE when it is not installed.
// ---------------------------------------------------------------------------------------
namespace {
struct RcclUid { char internal[128]; };   // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128)
struct RcclApi {
    void *handle = nullptr;
    int (*GetUniqueId)(RcclUid *) = nullptr;
    int (*CommInitRank)(void **, int, RcclUid, int) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    bool ok = false;
};
RcclApi load_rccl() {
    RcclApi r;
    // The RCCL that belongs to the HIP runtime THIS library is bound to, by path: a host process may
    // hold a second ROCm stack (PyTorch wheels bundle libamdhip64 / libhsa-runtime64 / librccl; when
    // torch is imported after libngp both stacks are mapped), and a bare dlopen("librccl.so.1")
    // then returns the copy already loaded — tied to the other, uninitialised runtime
    // ("no ROCm-capable device", scripts/rccl_probe.py).  The directory of the libamdhip64 that
    // resolved our own HIP calls decides.
    std::vector<std::string> names;
    Dl_info di{};
    if (dladdr((void *)&hipGetDeviceCount, &di) && di.dli_fname) {
        std::string dir(di.dli_fname);
        const size_t slash = dir.rfind('/');
        if (slash != std::string::npos) {
            dir.resize(slash + 1);
            names.push_back(dir + "librccl.so.1");
            names.push_back(dir + "librccl.so");
        }
    }
    for (const char *nm : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) names.push_back(nm);
    for (const std::string &name : names) {
        r.handle = dlopen(name.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (r.handle) break;
    }
    if (!r.handle) return r;
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(r.handle, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(r.handle, "ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.handle, "ncclCommDestroy");
    r.AllGather = (decltype(r.AllGather))dlsym(r.handle, "ncclAllGather");
    r.ok = r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.AllGather;
    return r;
}
const RcclApi &rccl() {
    static const RcclApi api = load_rccl();
    return api;
}
constexpr int RCCL_FLOAT64 = 8;   // ncclFloat64 (rccl.h)
}  // namespace

struct ngp_comm {
    ngp_ctx *ctx = nullptr;
    void *comm = nullptr;
    int rank = 0, world = 1;
    // send / receive buffers of the all-gather, grow-only: after the first call of a shape no
    // rank allocates inside a collective (an allocation that fails on ONE rank would leave its
    // peers waiting in the all-gather)
    void *d_send = nullptr, *d_recv = nullptr;
    size_t cap = 0;   // doubles per rank
};

extern "C" ngp_status ngp_comm_unique_id(void *id128) {
    if (!id128) return NGP_ERR_ARG;
    if (!rccl().ok) return NGP_ERR_UNAVAILABLE;
    RcclUid uid{};
    if (rccl().GetUniqueId(&uid) != 0) return NGP_ERR_UNAVAILABLE;
    std::memcpy(id128, uid.internal, sizeof(uid.internal));
    return NGP_OK;
}

extern "C" ngp_status ngp_comm_create(ngp_ctx *c, const void *id128, int32_t rank, int32_t world,
                                      ngp_comm **out) {
    if (!c || !id128 || !out || world <= 0 || rank < 0 || rank >= world) return NGP_ERR_ARG;
    *out = nullptr;
    if (!rccl().ok) return NGP_ERR_UNAVAILABLE;
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(hipSetDevice(c->device));
    RcclUid uid{};
    std::memcpy(uid.internal, id128, sizeof(uid.internal));
    ngp_comm *m = new (std::nothrow) ngp_comm();
    if (!m) return NGP_ERR_TOO_LARGE;
    m->ctx = c;
    m->rank = rank;
    m->world = world;
    // RCCL allocates its own device buffers, and after a large job most of the device can sit in
    // the caching allocators of this process: they are given back BEFORE the one attempt.  (The
    // initialisation is a collective — a rank that retried it alone after a failure would pair
    // with nobody, its peers having returned from the first attempt or still waiting inside it.)
    c->drop_cache();
    c->ws_drop();
    ngp_ctx::drop_other_caches(c);
    if (rccl().CommInitRank(&m->comm, world, uid, rank) != 0) {
        (void)hipGetLastError();
        delete m;
        return NGP_ERR_UNAVAILABLE;
    }
    *out = m;
    return NGP_OK;
}

extern "C" void ngp_comm_destroy(ngp_comm *m) {
    if (!m) return;
    if (m->comm && rccl().ok) {
        (void)hipSetDevice(m->ctx->device);
        (void)rccl().CommDestroy(m->comm);
    }
    {
        std::lock_guard<std::mutex> lk(m->ctx->mu);
        m->ctx->release(m->d_send);
        m->ctx->release(m->d_recv);
    }
    delete m;
}

extern "C" ngp_status ngp_shard(int32_t P_total, int32_t world, int32_t rank, int32_t *first,
                                int32_t *rows) {
    if (P_total < 0 || world <= 0 || rank < 0 || rank >= world) return NGP_ERR_ARG;
    const int base = P_total / world, rem = P_total % world;
    if (first) *first = rank * base + std::min(rank, rem);
    if (rows) *rows = base + (rank < rem ? 1 : 0);
    return NGP_OK;
}

// The host half of the exchange: `padded` holds what an all-gather of equally sized, zero-padded
// shards delivers — world blocks of pmax x D doubles, pmax = the largest shard (rank 0's), block r =
// rank r's rows then padding — and comes out as the P_total x D normalised weights.  Exported so that
// a host with a collective of its own (MPI.jl, Julia's Distributed, torch.distributed) pads,
// gathers with that, and normalises exactly as ngp_weights_allgather_normalize does.
extern "C" ngp_status ngp_weights_unpad_normalize(int32_t P_total, int32_t world, int32_t D,
                                                  const double *padded, double *w_all, double *ess,
                                                  double *log_norm) {
    if (!padded || P_total <= 0 || D <= 0 || world <= 0 || P_total < world) return NGP_ERR_ARG;
    auto rows_of = [&](int r) { int32_t v = 0; (void)ngp_shard(P_total, world, r, nullptr, &v); return (size_t)v; };
    auto first_of = [&](int r) { int32_t v = 0; (void)ngp_shard(P_total, world, r, &v, nullptr); return (size_t)v; };
    const size_t cnt = rows_of(0) * (size_t)D;
    std::vector<double> lw((size_t)P_total * D), wn((size_t)P_total * D);
    for (int r = 0; r < world; ++r)
        std::memcpy(lw.data() + first_of(r) * D, padded + (size_t)r * cnt, 8 * rows_of(r) * D);
    for (int sidx = 0; sidx < D; ++sidx)
        weights_normalize_strided(P_total, lw.data() + sidx, D, wn.data() + sidx, D,
                                  ess ? ess + sidx : nullptr, log_norm ? log_norm + sidx : nullptr);
    if (w_all) std::memcpy(w_all, wn.data(), 8 * wn.size());
    return NGP_OK;
}

extern "C" ngp_status ngp_weights_allgather_normalize(ngp_comm *m, int32_t P_total, int32_t D,
                                                      const double *logw_local, double *w_local,
                                                      double *w_all, double *ess,
                                                      double *log_norm) {
    if (!m || !logw_local || P_total <= 0 || D <= 0 || P_total < m->world) return NGP_ERR_ARG;
    // block partition of the particles over the ranks, remainder to the low ranks (ngp_shard: the
    // partition nowcastautogp_amd.distributed.shard and the Julia shim use)
    auto rows_of = [&](int r) { int32_t v = 0; (void)ngp_shard(P_total, m->world, r, nullptr, &v); return (int)v; };
    auto first_of = [&](int r) { int32_t v = 0; (void)ngp_shard(P_total, m->world, r, &v, nullptr); return (int)v; };
    const int mine = rows_of(m->rank), pmax = rows_of(0);
    ngp_ctx *c = m->ctx;
    std::vector<double> h_all;
    DevCall call(c);   // for the lock, the device and the copies: the buffers are the communicator's
    if (call.status()) return call.status();
    hipStream_t s = c->stream;
    // ragged shards: every rank sends pmax rows (its own, then padding).  The buffers stay with the
    // communicator; every rank sees the same (P_total, D), so they grow on all ranks in the same
    // call — and a rank that cannot grow them has left the collective for good: any non-zero
    // return of this function is FATAL for the communicator (its peers may be inside the
    // all-gather), destroy it and start over.
    const size_t cnt = (size_t)pmax * D;
    if (cnt > m->cap) {
        void *a = nullptr, *b = nullptr;
        ngp_status st;
        if ((st = c->alloc(&a, 8 * cnt)) || (st = c->alloc(&b, 8 * cnt * (size_t)m->world))) {
            c->release(a);
            return st;
        }
        c->release(m->d_send);
        c->release(m->d_recv);
        m->d_send = a;
        m->d_recv = b;
        m->cap = cnt;
    }
    void *d_send = m->d_send, *d_recv = m->d_recv;
    h_all.resize(cnt * (size_t)m->world);
    int rc = 0;
    call.run([&] { return hipMemsetAsync(d_send, 0, 8 * cnt, s); })
        .up(d_send, logw_local, 8 * (size_t)mine * D)
        .run([&] { rc = rccl().AllGather(d_send, d_recv, cnt, RCCL_FLOAT64, m->comm, s); });
    if (rc == 0) call.down(h_all.data(), d_recv, 8 * h_all.size());
    const ngp_status gathered = call.sync();
    if (rc != 0) return NGP_ERR_UNAVAILABLE;
    if (gathered) return gathered;
    // compact the padded shards to [P_total x D], then the columns as ngp_weights_normalize_cols
    std::vector<double> wn((size_t)P_total * D);
    const ngp_status st = ngp_weights_unpad_normalize(P_total, m->world, D, h_all.data(), wn.data(), ess, log_norm);
    if (st) return st;
    if (w_all) std::memcpy(w_all, wn.data(), 8 * wn.size());
    if (w_local)
        std::memcpy(w_local, wn.data() + (size_t)first_of(m->rank) * D, 8 * (size_t)mine * D);
    return NGP_OK;
}

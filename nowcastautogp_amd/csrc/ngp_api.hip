// ngp_api.hip — host side of libngp: contexts, staged jobs, launch schedule, C-ABI (include/ngp.h).
//
// One translation unit, as ngp_kernels.hip is on the device side.  The subsystems that nothing else
// in the host layer depends on are one ngp_host_*.h each, included at the END of this file in
// dependency order; the headers are not self-contained, and each says at its top what it holds and
// what stands before it.  In the order of the text:
//   this file            hip_status / HIPCHK, the page-locked pool and PinVec, ScopedEvent;
//                        check_program, compile_program; ngp_ctx and its registry, WsPlan, EventTimer,
//                        DevCall, dev_spec; the context's life cycle and switches; staged value jobs
//                        (FillLists, ngp_job, factor_chunk, stage_general, refinement, ngp_job_*, the
//                        *_stage calls, *_direct, ngp_nowcast_batch); the resident factor with its
//                        long-horizon and component queries, ngp_kernel_components / _terms,
//                        ngp_cov_batch
//   ngp_host_grad.h      gradient jobs: GradLeaf, LeafRun and its working blocks, the pair run, the
//                        HMC trajectory, ngp_grad_job and its entry points, logml_grad_direct — on
//                        the context, DevCall and the value jobs' sweep (factor_chunk, FillLists)
//   ngp_host_mixture.h   the forecast mixture: weight normalisation, MixInput, sampler, summaries,
//                        mapped CRPS, trajectory targets, ensemble and path scores — on the context
//                        and DevCall alone: no job, factor or gradient code
//   ngp_host_combine.h   flat combining, and the entry points that are requests (ngp_logml_batch,
//                        ngp_predict_batch, ngp_logml_grad_batch, ngp_grad_job_run,
//                        ngp_mixture_sample) — behind the value, gradient and mixture one-shot paths
//                        it merges
//   ngp_host_comm.h      the RCCL communicator, ngp_shard, all-gather and normalise — behind the
//                        mixture's weight normalisation
//   ngp_host_bench.h     microbenchmarks and MFMA layout self-tests — last, nothing needs it
//
// Host code of a new entry point goes with the subsystem whose state it runs on; a new subsystem gets
// a header of its own, a line in this table and an include where its prerequisites allow.  A section
// of this file that becomes a header moves as whole consecutive runs, no body edited.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "ngp_internal.h"

using namespace ngp;

// the only place a HIP error becomes a status: the positive HIP code
static ngp_status hip_status(hipError_t e) {
    return e == hipSuccess ? NGP_OK : (ngp_status)(e > 0 ? e : 999);
}
#define HIPCHK(expr)                                    \
    do {                                                \
        hipError_t e__ = (expr);                        \
        if (e__ != hipSuccess) return hip_status(e__);  \
    } while (0)

// ---- page-locked host memory for everything that crosses the bus ---------------------------
// A copy to or from pageable memory is not asynchronous: the runtime waits for the stream, moves
// the bytes through a bounce buffer of its own and only then returns (kernel trace of a 24-particle
// call at n = 208: the result copy started 25 us after the last kernel had ended).  The staging
// vectors of the jobs therefore live in page-locked memory, from a process-wide pool: blocks are
// kept by size class when a vector lets go of them, because hipHostMalloc costs a hundred
// microseconds and a fit stages ten thousand jobs.  When page-locking fails (no device, limits)
// the block is ordinary memory and everything still works, only slower.
namespace {
class PinnedPool {
    std::mutex mu;
    std::multimap<size_t, void *> free_;          // size class -> block
    std::map<void *, std::pair<size_t, bool>> live_;   // block -> (class, page-locked)
    size_t cached_ = 0;
    static constexpr size_t MAX_CACHED = (size_t)256 << 20, MAX_PINNED_BLOCK = (size_t)8 << 20;
    static size_t size_class(size_t n) {
        size_t c = 4096;
        while (c < n) c <<= 1;
        return c;
    }
public:
    void *take(size_t n) {
        const size_t c = size_class(n);
        {
            std::lock_guard<std::mutex> lk(mu);
            auto it = free_.find(c);
            if (it != free_.end()) {
                void *p = it->second;
                free_.erase(it);
                cached_ -= c;
                return p;
            }
        }
        // (page-locking is for the latency of small jobs; a large job's staging copy is a one-off whose
        // time is its bytes, and locking hundreds of megabytes costs more than it saves)
        void *p = nullptr;
        bool pinned = c <= MAX_PINNED_BLOCK &&
                      hipHostMalloc(&p, c, hipHostMallocPortable | hipHostMallocMapped) == hipSuccess && p;
        if (!pinned) {
            (void)hipGetLastError();
            p = std::malloc(c);
            if (!p) throw std::bad_alloc();
        }
        std::lock_guard<std::mutex> lk(mu);
        live_[p] = {c, pinned};
        return p;
    }
    bool is_pinned(const void *p) {
        std::lock_guard<std::mutex> lk(mu);
        auto it = live_.find(const_cast<void *>(p));
        return it != live_.end() && it->second.second;
    }
    void give(void *p) {
        std::lock_guard<std::mutex> lk(mu);
        auto it = live_.find(p);
        if (it == live_.end()) return;
        const size_t c = it->second.first;
        // (small blocks are always kept: were the cache ever full of large ones, every 24-item call
        // would page-lock and unlock its staging buffers again — 450 us per call, seen once)
        if (c <= MAX_PINNED_BLOCK && (c <= ((size_t)256 << 10) || cached_ + c <= MAX_CACHED)) {
            free_.emplace(c, p);
            cached_ += c;
            return;
        }
        const bool pinned = it->second.second;
        live_.erase(it);
        if (pinned) (void)hipHostFree(p);
        else std::free(p);
    }
    ~PinnedPool() {   // process exit: the runtime may already be gone — ordinary blocks only
        for (auto &kv : free_) {
            auto it = live_.find(kv.second);
            if (it != live_.end() && !it->second.second) std::free(kv.second);
        }
    }
};
inline PinnedPool &pinned_pool() {
    static PinnedPool *pool = new PinnedPool();   // never destroyed: vectors of static lifetime may outlive main
    return *pool;
}
template <class T> struct PinnedAlloc {
    typedef T value_type;
    PinnedAlloc() = default;
    template <class U> PinnedAlloc(const PinnedAlloc<U> &) {}
    T *allocate(size_t n) { return static_cast<T *>(pinned_pool().take(n * sizeof(T))); }
    void deallocate(T *p, size_t) { pinned_pool().give(p); }
    template <class U> bool operator==(const PinnedAlloc<U> &) const { return true; }
    template <class U> bool operator!=(const PinnedAlloc<U> &) const { return false; }
};
template <class T> using PinVec = std::vector<T, PinnedAlloc<T>>;
}  // namespace

namespace {
struct ScopedEvent {   // a timing event of a microbenchmark
    hipEvent_t e = nullptr;
    ScopedEvent() { (void)hipEventCreate(&e); }
    ~ScopedEvent() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};
}  // namespace

namespace {

// ---------------------------------------------------------------------------------------
// program validation + flattening for the device
// ---------------------------------------------------------------------------------------
ngp_status check_program(const ngp_kernel *k) {
    if (!k || !k->ops || k->n_ops <= 0) return NGP_ERR_PROGRAM;
    if (k->n_ops > NGP_MAX_OPS) return NGP_ERR_TOO_LARGE;
    int depth = 0, np = 0;
    for (int i = 0; i < k->n_ops; ++i) {
        const int op = k->ops[i];
        if (op < 1 || op > 8) return NGP_ERR_PROGRAM;
        np += k_nparams[op];
        if (op >= NGP_OP_PLUS) {
            if (depth < 2) return NGP_ERR_PROGRAM;
            depth -= 1;
        } else {
            depth += 1;
            if (depth > NGP_MAX_STACK) return NGP_ERR_TOO_LARGE;
        }
    }
    if (depth != 1) return NGP_ERR_PROGRAM;
    if (np != k->n_params) return NGP_ERR_PROGRAM;
    if (np > NGP_MAX_PARAMS) return NGP_ERR_TOO_LARGE;
    if (np > 0 && !k->params) return NGP_ERR_PROGRAM;
    return NGP_OK;
}

struct TNode {
    int op, left, right, pfirst, need;
};

// Re-emit the postfix program so the deeper subtree of every operator is evaluated first
// (Sethi-Ullman): the device keeps its evaluation stack in DEV_STACK registers.  Plus/Times
// commute bit-exactly in IEEE arithmetic; ChangePoint gets a swapped-operand opcode.
// perm[device param index] = caller's param index.
ngp_status compile_program(const ngp_kernel *k, DevProgram *out, std::vector<int> *perm,
                           int *n_stat = nullptr, int *n_cp = nullptr, int *n_tab = nullptr) {
    ngp_status st = check_program(k);
    if (st) return st;
    std::vector<TNode> nodes;
    std::vector<int> stack;
    int pi = 0;
    for (int i = 0; i < k->n_ops; ++i) {
        const int op = k->ops[i];
        TNode nd{op, -1, -1, pi, 1};
        if (op >= NGP_OP_PLUS) {
            nd.right = stack.back(); stack.pop_back();
            nd.left = stack.back(); stack.pop_back();
            const int a = nodes[nd.left].need, b = nodes[nd.right].need;
            nd.need = (a == b) ? a + 1 : std::max(a, b);
        }
        pi += k_nparams[op];
        nodes.push_back(nd);
        stack.push_back((int)nodes.size() - 1);
    }
    if (nodes[stack.back()].need > DEV_STACK) return NGP_ERR_TOO_LARGE;
    std::memset(out, 0, sizeof(DevProgram));
    out->n_ops = k->n_ops;
    out->n_params = k->n_params;
    out->noise = k->noise;
    int no = 0, np = 0, nstat = 0, ncp = 0;
    if (perm) perm->clear();
    // iterative post-order with child reordering
    struct Frame { int node, stage; };
    std::vector<int> dev_index(nodes.size(), -1), dev_first(nodes.size(), -1);
    std::vector<Frame> fs{{stack.back(), 0}};
    while (!fs.empty()) {
        Frame &f = fs.back();
        const TNode &nd = nodes[f.node];
        if (dev_first[(size_t)f.node] < 0) dev_first[(size_t)f.node] = no;   // first op of its subtree
        const bool swap = nd.op >= NGP_OP_PLUS && nodes[nd.right].need > nodes[nd.left].need;
        if (nd.op < NGP_OP_PLUS || f.stage == 2) {
            int op = nd.op;
            if (op == NGP_OP_CHANGEPOINT && swap) op = OP_CP_SWAPPED;
            if (nd.op >= NGP_OP_SQEXP && nd.op <= NGP_OP_PERIODIC) out->slot[no] = (uint8_t)nstat++;
            if (nd.op == NGP_OP_CHANGEPOINT) out->slot[no] = (uint8_t)ncp++;
            if (nd.op >= NGP_OP_PLUS)
                out->first[no] = (uint8_t)dev_index[(size_t)(swap ? nd.right : nd.left)];
            out->poff[no] = (uint8_t)np;
            dev_index[(size_t)f.node] = no;
            out->ops[no++] = (uint8_t)op;
            for (int q = 0; q < k_nparams[nd.op]; ++q) {
                out->params[np++] = k->params[nd.pfirst + q];
                if (perm) perm->push_back(nd.pfirst + q);
            }
            fs.pop_back();
        } else if (f.stage == 0) {
            f.stage = 1;
            fs.push_back({swap ? nd.right : nd.left, 0});
        } else {
            f.stage = 2;
            fs.push_back({swap ? nd.left : nd.right, 0});
        }
    }
    if (n_stat) *n_stat = nstat;
    if (n_cp) *n_cp = ncp;
    // ---- reduced program: maximal stationary subtrees become table leaves ----
    std::vector<char> stat(nodes.size(), 0);
    for (size_t i = 0; i < nodes.size(); ++i) {   // postfix input order: children come first
        const TNode &nd = nodes[i];
        if (nd.op == NGP_OP_PLUS || nd.op == NGP_OP_TIMES)
            stat[i] = stat[(size_t)nd.left] && stat[(size_t)nd.right];
        else
            stat[i] = nd.op != NGP_OP_LINEAR && nd.op != NGP_OP_CHANGEPOINT;
    }
    int nr = 0, ntab = 0;
    struct RFrame { int node, stage; };
    auto new_table = [&](int node) {
        out->tb_first[ntab] = (uint8_t)dev_first[(size_t)node];
        out->tb_last[ntab] = (uint8_t)dev_index[(size_t)node];
        return ntab++;
    };
    std::vector<RFrame> rs{{stack.back(), 0}};
    while (!rs.empty()) {
        RFrame &f = rs.back();
        const TNode &nd = nodes[(size_t)f.node];
        const int di = dev_index[(size_t)f.node];
        if (stat[(size_t)f.node]) {
            out->rops[nr] = (uint8_t)OP_TABLE;
            out->rslot[nr] = (uint8_t)new_table(f.node);
            ++nr;
            rs.pop_back();
        } else if (nd.op < NGP_OP_PLUS) {   // Linear
            out->rops[nr] = (uint8_t)nd.op;
            out->rpoff[nr] = out->poff[di];
            ++nr;
            rs.pop_back();
        } else {
            const bool swap = nodes[(size_t)nd.right].need > nodes[(size_t)nd.left].need;
            const int second = swap ? nd.left : nd.right;
            const bool leaf2 = stat[(size_t)second] || nodes[(size_t)second].op == NGP_OP_LINEAR;
            if (f.stage == 0) {
                f.stage = 1;
                rs.push_back({swap ? nd.right : nd.left, 0});
            } else if (f.stage == 1 && !leaf2) {
                f.stage = 2;
                rs.push_back({second, 0});
            } else {
                int code = out->ops[di];            // Plus / Times / ChangePoint or its swapped form
                if (leaf2) {                        // the second operand rides along (never pushed)
                    if (stat[(size_t)second]) {
                        code |= RLEAF_TABLE << 4;
                        out->rleaf[nr] = (uint8_t)new_table(second);
                    } else {
                        code |= RLEAF_LINEAR << 4;
                        out->rleaf[nr] = out->poff[dev_index[(size_t)second]];
                    }
                }
                out->rops[nr] = (uint8_t)code;
                out->rslot[nr] = out->slot[di];
                out->rpoff[nr] = out->poff[di];
                ++nr;
                rs.pop_back();
            }
        }
    }
    out->n_rops = nr;
    out->n_tab = ntab;
    out->rchain = 1;
    for (int i = 1; i < nr; ++i)
        if ((out->rops[i] >> 4) == 0) out->rchain = 0;
    if (n_tab) *n_tab = ntab;
    return NGP_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------
struct ngp_comb_req;   // one caller's request while it waits to be combined (ngp_combine below)

struct ngp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;          // diag-ahead tiles run beside the main schedule
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // extra lanes: small chunks of long series are swept as several sub-chunks side by side
    // (factor_chunk); made on first use
    static constexpr int MAX_LANES = 2;
    hipStream_t lane_main[MAX_LANES] = {}, lane_side[MAX_LANES] = {};
    hipEvent_t lane_fork[MAX_LANES] = {}, lane_join[MAX_LANES] = {}, lane_done[MAX_LANES] = {};
    hipEvent_t ev_lane_go = nullptr;
    int lanes_made = 1;   // lane 0 is (stream, side, ev_fork, ev_join)
    bool make_lanes(int n) {
        if (!ev_lane_go && hipEventCreateWithFlags(&ev_lane_go, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            ev_lane_go = nullptr;
            return false;
        }
        for (; lanes_made < n; ++lanes_made) {
            const int i = lanes_made;
            if (hipStreamCreateWithFlags(&lane_main[i], hipStreamNonBlocking) != hipSuccess ||
                hipStreamCreateWithFlags(&lane_side[i], hipStreamNonBlocking) != hipSuccess ||
                hipEventCreateWithFlags(&lane_fork[i], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&lane_join[i], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&lane_done[i], hipEventDisableTiming) != hipSuccess) {
                (void)hipGetLastError();
                return false;
            }
        }
        return true;
    }
    ngp_spec spec{};
    std::mutex mu;
    // Flat combining of concurrent callers ("combining" section below): one-shot calls that arrive
    // while the device is busy wait in `pending`; the thread that finds nobody serving takes ALL of
    // them and runs every group of compatible requests as ONE launch sequence.  qmu guards these
    // fields only and is never held across a device call; mu stays the execution lock.
    std::mutex qmu;
    std::vector<ngp_comb_req *> pending;
    bool combining = false, combine_on = true, combine_linger = true;
    int64_t comb_stats[6] = {};   // requests | launch sequences | largest group | requests that shared one |
                                  // requests served from ONE factorisation per particle | (reserved)
    // company seen lately: the number of requests the last server took (decays when a wait for
    // it was in vain) and the condition a would-be server waits on for at most COMB_LINGER_US
    size_t comb_expect = 1;
    std::condition_variable comb_arrival;
    bool profiling = false;
    bool toeplitz = true;   // ngp_set_structured_storage
    bool invariant = false; // ngp_set_batch_invariant (JobGeom::invariant of the jobs staged after)
    bool short_series = true;   // ngp_set_short_series_path: n0 <= 256 factorised in one launch
    ngp_profile prof{};
    size_t mem_cap = 0;  // bytes the factor storage of one job may take
    // caching allocator: repeated jobs of the same shape (the SMC/MCMC loop, the steps of a
    // staged batch) reuse blocks.  A context that cannot allocate first gives its own cache back
    // to the device, then the caches of the process's other contexts (registry below).
    std::multimap<size_t, void *> free_blocks;
    std::map<void *, size_t> live;
    size_t cached_bytes = 0;

    void drop_cache() {
        for (auto &kv : free_blocks) (void)hipFree(kv.second);
        free_blocks.clear();
        cached_bytes = 0;
    }
    // Workspace: ONE grow-only block for the working storage of a call (factor slabs, K^-1, tables —
    // everything a run takes at its start and gives back at its end; calls on a context are
    // serialised and end synchronised, so the next call may overwrite it).  Jobs of different
    // shapes alternate in the reference's flow — gradient calls (115 + 57 GB blocks at 12,800 items)
    // and a predictive call (221 GB) in forecast_with_nowcasts' refinement modes — and with
    // per-shape blocks every switch freed and re-allocated most of the device: 7.7 of the 8.5 s the
    // predictive call of the lockstep HMC leg took (scripts/hmc_leg_cprofile.py).  Things that
    // outlive a call (job arenas, resident factors) stay with alloc / release.
    void *ws_base = nullptr;
    size_t ws_cap = 0, ws_used = 0;
    void ws_drop() {
        if (ws_base) (void)hipFree(ws_base);
        ws_base = nullptr;
        ws_cap = ws_used = 0;
    }
    static size_t ws_round(size_t bytes) { return (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255; }
    // room for `total` bytes of bump allocations (sum of ws_round of the pieces); the previous
    // call's contents are dead
    ngp_status ws_reserve(size_t total) {
        ws_used = 0;
        if (total <= ws_cap) return NGP_OK;
        ws_drop();
        hipError_t e = hipMalloc(&ws_base, total);
        for (int attempt = 0; e != hipSuccess && attempt < 2; ++attempt) {
            (void)hipGetLastError();   // handled here: must not surface as the job's last error
            if (attempt == 0) drop_cache();
            else drop_other_caches(this);
            e = hipMalloc(&ws_base, total);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            ws_base = nullptr;
            return NGP_ERR_TOO_LARGE;
        }
        ws_cap = total;
        return NGP_OK;
    }
    void *ws_take(size_t bytes) {   // inside the reservation: cannot fail
        bytes = ws_round(bytes);
        if (ws_used + bytes > ws_cap) return nullptr;
        void *p = (char *)ws_base + ws_used;
        ws_used += bytes;
        return p;
    }
    static void drop_other_caches(ngp_ctx *self);
    ngp_status alloc(void **p, size_t bytes) {
        bytes = (bytes + 255) / 256 * 256;
        if (bytes == 0) bytes = 256;
        auto it = free_blocks.lower_bound(bytes);
        if (it != free_blocks.end() && it->first <= bytes * 2) {
            *p = it->second;
            live[*p] = it->first;
            cached_bytes -= it->first;
            free_blocks.erase(it);
            return NGP_OK;
        }
        hipError_t e = hipMalloc(p, bytes);
        for (int attempt = 0; e != hipSuccess && attempt < 2; ++attempt) {
            (void)hipGetLastError();   // handled here: must not surface as the job's last error
            if (attempt == 0) drop_cache();
            else drop_other_caches(this);
            e = hipMalloc(p, bytes);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            *p = nullptr;
            return NGP_ERR_TOO_LARGE;
        }
        live[*p] = bytes;
        return NGP_OK;
    }
    void release(void *p) {
        if (!p) return;
        auto it = live.find(p);
        if (it == live.end()) return;
        free_blocks.emplace(it->second, p);
        cached_bytes += it->second;
        live.erase(it);
    }
    // split-k fat steps of small chunks (ngp_col_kernels.h): grow-only, owned by the context
    double *splitk_part = nullptr;
    int splitk_items = 0;
    ngp_status splitk_reserve(int items) {
        if (items <= splitk_items) return NGP_OK;
        void *a = nullptr;
        if (alloc(&a, sizeof(double) * (size_t)items * SPLITK_SLOTS * 4 * 64 * 64))
            return NGP_ERR_TOO_LARGE;
        release(splitk_part);
        splitk_part = (double *)a;
        splitk_items = items;
        return NGP_OK;
    }
    // bytes a job's factor storage may take: 3/4 of what the device has free now plus what this
    // context's cache would give back (the figure of ngp_ctx_create goes stale as soon as another
    // context or a resident factor allocates)
    void refresh_mem_cap() {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess)
            mem_cap = (size_t)(0.75 * (double)(fr + cached_bytes + ws_cap));
    }
};

// every live context of the process (alloc falls back on the others' caches)
static std::mutex g_ctx_registry_mu;
static std::vector<ngp_ctx *> g_ctx_registry;
void ngp_ctx::drop_other_caches(ngp_ctx *self) {
    std::lock_guard<std::mutex> lk(g_ctx_registry_mu);
    for (ngp_ctx *o : g_ctx_registry) {
        if (o == self || o->device != self->device) continue;
        if (o->mu.try_lock()) {   // a context in the middle of a call keeps its cache
            o->drop_cache();
            o->ws_drop();
            o->mu.unlock();
        }
    }
}

// The working storage of a run is laid out twice through the same sequence of requests: once to
// add the sizes up (the workspace is then reserved in one piece), once to take the pieces.
struct WsPlan {
    ngp_ctx *c;
    bool measuring;
    size_t total = 0;
    ngp_status operator()(void **q, size_t bytes) {
        if (measuring) {
            total += ngp_ctx::ws_round(bytes);
            *q = nullptr;
            return NGP_OK;
        }
        *q = c->ws_take(bytes);
        return *q ? NGP_OK : NGP_ERR_TOO_LARGE;
    }
};

struct EventTimer {  // HIP events on the launch stream, resolved after the job's final sync
    struct Rec { int cls; hipEvent_t a, b; double flops, bytes; };
    std::vector<Rec> recs;
    bool on;
    hipStream_t s;
    EventTimer(bool on_, hipStream_t s_) : on(on_), s(s_) {}
    ~EventTimer() {   // an error path left before resolve()
        for (auto &r : recs) {
            (void)hipEventDestroy(r.a);
            (void)hipEventDestroy(r.b);
        }
    }
    // `on_stream`: the stream f launches on when it is not the timer's own (diag-ahead tiles)
    template <class F> void run(int cls, double flops, double bytes, F &&f,
                                hipStream_t on_stream = nullptr) {
        if (!on) { f(); return; }
        hipStream_t es = on_stream ? on_stream : s;
        Rec r{cls, nullptr, nullptr, flops, bytes};
        (void)hipEventCreate(&r.a);
        (void)hipEventCreate(&r.b);
        (void)hipEventRecord(r.a, es);
        f();
        (void)hipEventRecord(r.b, es);
        recs.push_back(r);
    }
    template <class F> void run(const Cost &c, F &&f, hipStream_t on_stream = nullptr) {
        run(c.cls, c.flops, c.bytes, std::forward<F>(f), on_stream);
    }
    void resolve(ngp_profile &p) {
        for (auto &r : recs) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
                p.ms[r.cls] += ms;
                p.launches[r.cls] += 1;
                p.flops[r.cls] += r.flops;
                p.bytes[r.cls] += r.bytes;
            }
            (void)hipEventDestroy(r.a);
            (void)hipEventDestroy(r.b);
        }
        recs.clear();
    }
};

// A call or a staged run on a context: the execution lock, the device, the timers of its launches,
// the blocks it takes from the context's allocator and the first error of its copies, memsets and
// launches.  After an error every further step is skipped, so a run is written straight down and asks
// once, at sync(), how it went.  Whatever it has queued may read and write host memory of its frame,
// of its job and of the caller, and blocks that go back to the cache when it ends: sync() waits for
// every stream the run used also after an error, asks the runtime for its last error once and books
// the timers into the profile; a scope that is left with work queued is synchronised by the
// destructor before its blocks are released.  Host memory that a queued copy targets is declared
// before the scope (or lives in the job).
class DevCall {
    static constexpr int MAX_BLOCKS = 32;   // the trajectory targets take 27; nothing here touches the heap
    ngp_ctx *c;
    std::unique_lock<std::mutex> lk;
    void *blocks[MAX_BLOCKS];
    int n_blocks = 0;
    ngp_status st = NGP_OK;
    bool queued = false, lane1 = false;
    EventTimer tm1;   // launches on lane 1 (second_lane)
    DevCall &copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
        return run([&] { return hipMemcpyAsync(dst, src, bytes, kind, s ? s : c->stream); });
    }
public:
    EventTimer tm;    // launches on the context's stream
    explicit DevCall(ngp_ctx *ctx) : c(ctx), lk(ctx->mu), tm1(false, nullptr), tm(ctx->profiling, ctx->stream) {
        st = hip_status(hipSetDevice(c->device));
    }
    // an inner scope of a call in flight (the rounds of a loop): same lock, blocks of its own
    explicit DevCall(DevCall &outer) : c(outer.c), st(outer.st), tm1(false, nullptr), tm(false, outer.c->stream) {}
    DevCall(const DevCall &) = delete;
    ~DevCall() {   // the lock is held here: unlocked() is the only place that drops it
        (void)sync();
        for (int i = 0; i < n_blocks; ++i) c->release(blocks[i]);
    }
    ngp_status status() const { return st; }
    DevCall &fail(ngp_status s) {   // an error of the host's own (no room): the steps after it are skipped
        if (!st) st = s;
        return *this;
    }
    template <class T> DevCall &take(T **p, size_t count) {
        void *q = nullptr;
        if (!st && n_blocks == MAX_BLOCKS) st = NGP_ERR_TOO_LARGE;
        if (!st && !(st = c->alloc(&q, sizeof(T) * count))) blocks[n_blocks++] = q;
        *p = static_cast<T *>(q);
        return *this;
    }
    // a block that outlives the call (a job's arena, a resident factor): *p is set when there is one, and
    // whoever owns *p releases it (`owned`: the list a job releases)
    template <class T> DevCall &keep(T **p, size_t count, std::vector<void *> *owned = nullptr) {
        void *q = nullptr;
        if (st || (st = c->alloc(&q, sizeof(T) * count))) return *this;
        if (owned) owned->push_back(q);
        *p = static_cast<T *>(q);
        return *this;
    }
    // host work that takes the context's lock itself (a staged job's run and fetch), on this thread:
    // the lock is dropped around it, the blocks stay held; skipped after an error, its status is kept
    template <class F> DevCall &unlocked(F &&work) {
        if (st) return *this;
        lk.unlock();
        st = work();
        lk.lock();
        return *this;
    }
    // s: the lane's stream when it is not the context's
    DevCall &up(void *dev, const void *host, size_t bytes, hipStream_t s = nullptr) {
        return copy(dev, host, bytes, hipMemcpyHostToDevice, s);
    }
    DevCall &down(void *host, const void *dev, size_t bytes, hipStream_t s = nullptr) {
        return copy(host, dev, bytes, hipMemcpyDeviceToHost, s);
    }
    DevCall &move(void *dst, const void *src, size_t bytes) { return copy(dst, src, bytes, hipMemcpyDeviceToDevice, nullptr); }
    DevCall &zero(void *dev, size_t bytes, hipStream_t s = nullptr) {
        return run([&] { return hipMemsetAsync(dev, 0, bytes, s ? s : c->stream); });
    }
    // launches: void, or the hipError_t of what they asked of the runtime
    template <class F> DevCall &run(F &&launches) {
        if (st) return *this;
        queued = true;
        if constexpr (std::is_void<decltype(launches())>::value) launches();
        else st = hip_status(launches());
        return *this;
    }
    // launches booked by a timer of this scope: t.run(a...) (EventTimer::run)
    template <class... A> DevCall &timed(EventTimer &t, A &&...a) {
        return run([&] { t.run(std::forward<A>(a)...); });
    }
    // a run on two lanes (grad_pair_run): the timer of lane 1, which sync() then waits for as well
    EventTimer &second_lane() {
        lane1 = true;
        tm1.on = tm.on;
        tm1.s = c->lane_main[1];
        return tm1;
    }
    // work an earlier call left on the stream (a kept staging copy) is this scope's to wait for
    DevCall &pending() { queued = true; return *this; }
    // what this scope queued stays with a job that outlives it, which waits for it before it lets go
    // of what the work reads and writes (a small job's staging copy: ngp_job_destroy, grad_leaf_destroy)
    void handed_over() { queued = false; }
    // a host round trip inside a run: waits for every stream used, does not end the scope
    ngp_status wait() {
        if (queued) {
            hipError_t e = hipStreamSynchronize(c->stream);
            if (lane1) {
                const hipError_t e1 = hipStreamSynchronize(c->lane_main[1]);
                if (e == hipSuccess) e = e1;
            }
            if (e == hipSuccess) e = hipGetLastError();
            if (!st) st = hip_status(e);
            queued = false;
        }
        return st;
    }
    ngp_status sync() {
        (void)wait();
        tm.resolve(c->prof);
        tm1.resolve(c->prof);
        return st;
    }
};

static DevSpec dev_spec(const ngp_spec &s) {
    return DevSpec{s.se_form, s.periodic_form, s.cp_form, s.precision, s.jitter, s.mixed_tau};
}

extern "C" void ngp_default_spec(ngp_spec *s) {
    if (!s) return;
    s->se_form = 0;
    s->periodic_form = 0;
    s->cp_form = 0;
    s->precision = NGP_PREC_F64;
    s->jitter = 1e-5;
    s->mixed_tau = 1e-6;
    s->refine_tol = 1e-9;
    s->refine_max = 3;
    s->reserved = 0;
}

extern "C" const char *ngp_version(void) { return "libngp 0.1.0 (gfx950)"; }

extern "C" const char *ngp_strerror(ngp_status st) {
    switch (st) {
    case NGP_OK: return "ok";
    case NGP_ERR_ARG: return "bad argument (null pointer or negative size)";
    case NGP_ERR_PROGRAM: return "malformed kernel program";
    case NGP_ERR_TOO_LARGE: return "problem exceeds a library limit or device memory";
    case NGP_ERR_NO_DEVICE: return "no usable HIP device";
    case NGP_ERR_STATE: return "job used out of order / entry point unavailable";
    case NGP_ERR_UNAVAILABLE: return "optional component (librccl) is not available";
    default: break;
    }
    if (st > 0) return hipGetErrorString((hipError_t)st);
    return "unknown error";
}

extern "C" ngp_status ngp_kernel_check(const ngp_kernel *k) {
    DevProgram tmp;
    return compile_program(k, &tmp, nullptr);
}

extern "C" ngp_status ngp_ctx_create(int32_t device, ngp_ctx **out) {
    if (!out) return NGP_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return NGP_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return NGP_ERR_ARG;
    HIPCHK(hipSetDevice(device));
    ngp_ctx *c = new (std::nothrow) ngp_ctx();
    if (!c) return NGP_ERR_TOO_LARGE;
    c->device = device;
    ngp_default_spec(&c->spec);
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return hip_status(e);
    }
    if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
        delete c;
        return NGP_ERR_NO_DEVICE;
    }
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) c->mem_cap = (size_t)(0.75 * (double)fr);
    else c->mem_cap = (size_t)8 << 30;
    {
        std::lock_guard<std::mutex> lk(g_ctx_registry_mu);
        g_ctx_registry.push_back(c);
    }
    *out = c;
    return NGP_OK;
}

extern "C" void ngp_ctx_destroy(ngp_ctx *c) {
    if (!c) return;
    {
        std::lock_guard<std::mutex> lk(g_ctx_registry_mu);
        g_ctx_registry.erase(std::remove(g_ctx_registry.begin(), g_ctx_registry.end(), c),
                             g_ctx_registry.end());
    }
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto &kv : c->free_blocks) (void)hipFree(kv.second);
    for (auto &kv : c->live) (void)hipFree(kv.first);
    c->ws_drop();
    (void)hipStreamDestroy(c->stream);
    if (c->side) { (void)hipStreamSynchronize(c->side); (void)hipStreamDestroy(c->side); }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    for (int i = 1; i < ngp_ctx::MAX_LANES; ++i) {
        if (c->lane_main[i]) { (void)hipStreamSynchronize(c->lane_main[i]); (void)hipStreamDestroy(c->lane_main[i]); }
        if (c->lane_side[i]) { (void)hipStreamSynchronize(c->lane_side[i]); (void)hipStreamDestroy(c->lane_side[i]); }
        for (hipEvent_t e : {c->lane_fork[i], c->lane_join[i], c->lane_done[i]})
            if (e) (void)hipEventDestroy(e);
    }
    if (c->ev_lane_go) (void)hipEventDestroy(c->ev_lane_go);
    delete c;
}

extern "C" ngp_status ngp_set_spec(ngp_ctx *c, const ngp_spec *s) {
    if (!c || !s) return NGP_ERR_ARG;
    if (s->se_form < 0 || s->se_form > 1 || s->periodic_form < 0 || s->periodic_form > 1 ||
        s->cp_form < 0 || s->cp_form > 1 || !(s->jitter >= 0.0))
        return NGP_ERR_ARG;
    if (s->precision != NGP_PREC_F64 && s->precision != NGP_PREC_MIXED) return NGP_ERR_ARG;
    if (s->precision == NGP_PREC_MIXED &&
        (!(s->mixed_tau >= 0.0) || !(s->refine_tol > 0.0) || s->refine_max < 0 || s->refine_max > 16))
        return NGP_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    c->spec = *s;
    return NGP_OK;
}
extern "C" ngp_status ngp_get_spec(const ngp_ctx *c, ngp_spec *s) {
    if (!c || !s) return NGP_ERR_ARG;
    std::lock_guard<std::mutex> lk(const_cast<ngp_ctx *>(c)->mu);
    *s = c->spec;
    return NGP_OK;
}

extern "C" ngp_status ngp_set_structured_storage(ngp_ctx *c, int32_t on) {
    if (!c) return NGP_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    c->toeplitz = on != 0;
    return NGP_OK;
}
extern "C" ngp_status ngp_set_batch_invariant(ngp_ctx *c, int32_t on) {
    if (!c) return NGP_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    c->invariant = on != 0;
    return NGP_OK;
}
extern "C" ngp_status ngp_set_short_series_path(ngp_ctx *c, int32_t on) {
    if (!c) return NGP_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    c->short_series = on != 0;
    return NGP_OK;
}
extern "C" ngp_status ngp_profile_enable(ngp_ctx *c, int32_t on) {
    if (!c) return NGP_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    c->profiling = on != 0;
    return NGP_OK;
}
extern "C" ngp_status ngp_profile_reset(ngp_ctx *c) {
    if (!c) return NGP_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    std::memset(&c->prof, 0, sizeof(c->prof));
    return NGP_OK;
}
extern "C" ngp_status ngp_profile_get(ngp_ctx *c, ngp_profile *out) {
    if (!c || !out) return NGP_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    *out = c->prof;
    return NGP_OK;
}

// ---------------------------------------------------------------------------------------
// jobs
// ---------------------------------------------------------------------------------------
// The fill-list section of a staging arena.  A lattice job's items by the shape of their reduced
// program — one table for the whole tree (fill_single_kernel; in a Toeplitz job the structured
// items, prog_structure) / chain programs (fill_chain_kernel) / the rest (the general fill) — as
// ascending job-wide indices, and where the three lists sit in the arena.  launch_fill reads a
// chunk's share of each list (share_of).
struct FillLists {
    std::vector<int32_t> single, chain, other;
    size_t o_single = 0, o_chain = 0, o_other = 0;   // byte offsets in the arena

    void sort_items(const DevProgram *hp, int n) {
        for (int i = 0; i < n; ++i)
            (prog_single_table(&hp[i]) ? single : hp[i].rchain ? chain : other).push_back(i);
    }
    // take(bytes) -> offset: the arena's own allocator, so the section sits where it always did
    template <class Take>
    void layout(Take &&take) {
        o_single = take(4 * single.size());
        o_chain = take(4 * chain.size());
        o_other = take(4 * other.size());
    }
    void copy_to(unsigned char *h) const {
        auto put = [&](const std::vector<int32_t> &v, size_t o) {
            if (!v.empty()) std::memcpy(h + o, v.data(), 4 * v.size());
        };
        put(single, o_single);
        put(chain, o_chain);
        put(other, o_other);
    }
    // the share of chunk [b0, b0 + bc) in each list; io: the arena on the device
    void share_of(const unsigned char *io, int b0, int bc, ChunkPtrs *p) const {
        auto share = [&](const std::vector<int32_t> &v, size_t o, const int32_t **ptr, int32_t *cnt) {
            const auto lo = std::lower_bound(v.begin(), v.end(), b0);
            const auto hi = std::lower_bound(v.begin(), v.end(), b0 + bc);
            *ptr = (const int32_t *)(io + o) + (lo - v.begin());
            *cnt = (int32_t)(hi - lo);
        };
        share(single, o_single, &p->fill_single, &p->n_fill_single);
        share(chain, o_chain, &p->fill_chain, &p->n_fill_chain);
        share(other, o_other, &p->fill_other, &p->n_fill_other);
        p->fill_base = b0;
    }
};

struct ngp_job {
    ngp_ctx *ctx = nullptr;
    JobGeom g{};
    int n = 0;          // base training points (n0 + tail)
    bool ran = false;
    // device buffers
    DevProgram *progs = nullptr;
    double *t0 = nullptr, *taux = nullptr, *y0 = nullptr, *ya = nullptr;
    double *logdet = nullptr, *G = nullptr, *work = nullptr, *zbuf = nullptr;
    int32_t *info = nullptr, *qpts = nullptr;
    double *logml_base = nullptr, *logml_full = nullptr, *mu = nullptr, *sigma = nullptr;
    int64_t work_stride = 0;
    std::vector<void *> owned;
    // the staging copy of the inputs (kept while small: stage_general), the result region of the
    // arena ([info | logml_base | logml_full | mu | sigma], offsets from info) and whether logdet /
    // info still hold the zeros they were staged with
    PinVec<unsigned char> h_in, h_out;
    size_t out_off[5] = {}, out_bytes = 0;
    bool zeroed = false, copy_in_flight = false;
    bool out_fetched = false;   // h_out holds the result region of the last run
    // the spec the job was staged under: a later ngp_set_spec does not reach a staged job
    ngp_spec spec{};
    // lattice jobs with a main block: the items by their fill kernel; fill_io: the arena once the
    // lists are on the device (null: every item goes through the general fill)
    FillLists fill;
    const unsigned char *fill_io = nullptr;
    // NGP_PREC_MIXED: per item, filled by ngp_job_run
    std::vector<int32_t> refine_steps;
    std::vector<double> refine_delta, frac32;
    // The one place the outcome of a run reaches the job, after the run's scope has synchronised
    // (nothing is in flight any more).  A failed run leaves the job as staged-and-never-run with logdet
    // / info dirty: the next run is an ordinary re-run (it clears them), a fetch is refused.
    // fetched: the run brought the result region to h_out behind its last kernel
    void run_ended(ngp_status st, bool fetched) {
        copy_in_flight = zeroed = false;
        ran = st == NGP_OK;
        out_fetched = ran && fetched;
    }
};

namespace {

// The left-looking factorisation of one chunk (every item's block columns in lock step): which step
// runs in which form is ngp_plan.h's (col_step, small_job, two_lane, splitk_eligible, ahead_early),
// what it is booked as ngp_cost.h's.
struct Lane {
    hipStream_t main, side;
    hipEvent_t fork, join;
    ngp_ctx *ctx;
};
inline Lane lane_of(ngp_ctx *c) { return Lane{c->stream, c->side, c->ev_fork, c->ev_join, c}; }
inline Lane lane_of(ngp_ctx *c, int i) {
    return i == 0 ? lane_of(c) : Lane{c->lane_main[i], c->lane_side[i], c->lane_fork[i], c->lane_join[i], c};
}

// The column kernels address an item's factor storage through a buffer descriptor with 32-bit
// byte offsets: it must stay below 2 GiB (n <= 16,256 for value jobs, 11,520 for gradient jobs).
inline bool item_too_large(int64_t item_stride) { return item_stride * 8 > (int64_t)0x7fffffff; }

void factor_chunk_lanes(const Lane &ln, const JobGeom &g, const ChunkPtrs &p0, int bc, EventTimer &tm,
                        size_t dinv_step, const DevSpec *sp, int32_t *order_buf, unsigned *order_prev);

// dinv_step != 0: block column jj writes / reads its M at p.dinv + jj * dinv_step (cached factor:
// every M_j is kept); 0: one buffer reused by every step.
// sp != null and p0.L32 set: mixed-precision job (fat steps on chol_col_glds_kernel<MIXED>, class 9).
// order_buf / order_prev ([bc] each, mixed jobs): the ranking of MIXED_REORDER.
void factor_chunk(const Lane &ln, const JobGeom &g, const ChunkPtrs &p_in, int bc, EventTimer &tm,
                  size_t dinv_step = 0, const DevSpec *sp = nullptr, int32_t *order_buf = nullptr,
                  unsigned *order_prev = nullptr, bool half = false) {
    ChunkPtrs p0 = p_in;
    const bool mixed = sp != nullptr && p0.L32 != nullptr;
    hipStream_t s = ln.main;
    // Short series: the whole sweep of an item in one launch (ngp_small_kernels.h).  Resident factors
    // and the Toeplitz gradient path keep every M_j (dinv_step) and stay on the column sweep.
    SmallPlan spl;
    if (!mixed && dinv_step == 0 && small_job(g, bc, &spl)) {
        tm.run(cost_small(g, spl, bc), [&] { launch_chol_small(g, p0, bc, spl, s); });
        return;
    }
    // room for the split-k fat steps; the buffer stays with the context
    if (splitk_eligible(g, bc, mixed, half) && ln.ctx->splitk_reserve(bc) == NGP_OK)
        p0.splitk_part = ln.ctx->splitk_part;
    if (two_lane(g, bc, mixed, half) && ln.main == ln.ctx->stream && ln.ctx->make_lanes(ngp_ctx::MAX_LANES))
        return factor_chunk_lanes(ln, g, p0, bc, tm, dinv_step, sp, order_buf, order_prev);
    const double lazy_frac = lazy_fraction(g, p0.n_fill_single, bc, mixed);
    for (int jj = 0; jj < g.nb0; ++jj) {
        const ColStepPlan st = col_step(g, jj);
        ChunkPtrs p = p0;
        p.dinv = p0.dinv + (size_t)jj * dinv_step;
        if (st.join) (void)hipStreamWaitEvent(s, ln.join, 0);   // chol_diag(jj) is the tile's only consumer
        auto launch_ahead = [&] {
            (void)hipEventRecord(ln.fork, s);
            (void)hipStreamWaitEvent(ln.side, ln.fork, 0);
            tm.run(cost_ahead(bc, jj), [&] { launch_diag_ahead(g, p0, bc, jj, ln.side); }, ln.side);
            (void)hipEventRecord(ln.join, ln.side);
        };
        if (st.ahead && ahead_early(bc)) launch_ahead();
        tm.run(cost_diag(bc, jj, st.k0_diag), [&] { launch_chol_diag(g, p, bc, jj, st.k0_diag, s); });
        tm.run(cost_col(g, bc, jj, st.mode, st.k0_col, mixed, lazy_frac),
               [&] { launch_chol_col(g, p, bc, jj, st.mode, st.k0_col, s, sp); });
        if (mixed && st.mode == COL_FAT && order_buf && jj >= 8 && jj % MIXED_REORDER == 8) {
            // p0.order stays null (dispatch order) unless the ranking was really launched:
            // order_buf comes from the caching allocator uninitialised
            if (launch_mixed_order(p0, order_prev, order_buf, bc, s)) p0.order = order_buf;
        }
        if (st.ahead && !ahead_early(bc)) launch_ahead();
    }
}

// Small chunks of long series (the 64-particle calls of a fit) are swept as two half-chunks side
// by side, each on its own pair of streams (lanes).  A launch of such a chunk rarely fills the chip or
// fills it one and a fraction times (64 items at n = 2048: 576 workgroups on 512 slots at
// column 14 — two rounds for the price of 1.1), and chol_diag / the thin step leave it almost
// empty: the other half's fat step runs in those gaps.  Every item's arithmetic is what it
// would be in a chunk of its half's size.
void factor_chunk_lanes(const Lane &ln, const JobGeom &g, const ChunkPtrs &p0, int bc, EventTimer &tm,
                        size_t dinv_step, const DevSpec *sp, int32_t *order_buf, unsigned *order_prev) {
    ngp_ctx *c = ln.ctx;
    const int nl = ngp_ctx::MAX_LANES;
    (void)hipEventRecord(c->ev_lane_go, ln.main);
    std::vector<EventTimer> tms;
    tms.reserve((size_t)nl);
    int h0 = 0;
    for (int i = 0; i < nl; ++i) {
        const int h1 = (int)((long)bc * (i + 1) / nl);
        ChunkPtrs pi = p0;
        pi.L += (size_t)h0 * g.item_stride;
        pi.dinv += (size_t)h0 * NB * NB;
        pi.progs += h0;
        pi.logdet += h0;
        pi.info += h0;
        if (pi.tab) pi.tab += (size_t)h0 * g.maxstat * g.R;   // read by the column kernels (toep)
        pi.n_fill_single = (int32_t)((long)p0.n_fill_single * (h1 - h0) / bc);   // byte accounting only
        if (pi.splitk_part) pi.splitk_part += (size_t)h0 * SPLITK_SLOTS * 4 * 64 * 64;
        if (i == 0) {
            factor_chunk(ln, g, pi, h1 - h0, tm, dinv_step, sp, order_buf, order_prev, true);
        } else {
            const Lane li = lane_of(c, i);
            tms.emplace_back(tm.on, li.main);
            (void)hipStreamWaitEvent(li.main, c->ev_lane_go, 0);
            factor_chunk(li, g, pi, h1 - h0, tms.back(), dinv_step, sp, order_buf, order_prev, true);
            (void)hipEventRecord(c->lane_done[i], li.main);
        }
        h0 = h1;
    }
    for (int i = 1; i < nl; ++i) (void)hipStreamWaitEvent(ln.main, c->lane_done[i], 0);
    for (auto &t : tms) {
        tm.recs.insert(tm.recs.end(), t.recs.begin(), t.recs.end());
        t.recs.clear();
    }
}

// The one copy that carries a staged job's inputs up (bytes of h_in to io); a failure is
// NGP_ERR_STATE.  A small staging buffer stays with the job — no wait here: the run is queued right
// behind the copy, and the job's destroy waits for it if no run did; a large one is given back once
// the copy has left it.
ngp_status stage_up(DevCall &call, hipStream_t s, void *io, PinVec<unsigned char> &h_in, size_t bytes) {
    call.run([&] {
        if (hipMemcpyAsync(io, h_in.data(), bytes, hipMemcpyHostToDevice, s) != hipSuccess) call.fail(NGP_ERR_STATE);
    });
    if (call.status()) return call.status();
    if (bytes <= STAGE_KEEP_BYTES) {
        call.handed_over();
        return NGP_OK;
    }
    if (call.wait()) return NGP_ERR_STATE;
    PinVec<unsigned char>().swap(h_in);
    return NGP_OK;
}

// Stage a job in its general form: P kernels; base data (t[n], y [P or 1][n]); d appended
// times; D scenarios y_add [(P or 1)][D][d]; m forecast times.
// yrows (combined calls, ngp_combine below): item b's observations are yrows[b][0..n) — the rows of
// several callers' arrays, never copied into one matrix on the host; y / ldy are then not read.
ngp_status stage_general(ngp_ctx *c, int P, const ngp_kernel *kernels, int n, const double *t,
                         const double *y, int64_t ldy, int d, const double *t_add, int D,
                         const double *y_add, int64_t ld_yadd_item, int m, const double *t_new,
                         int noise_on_new, ngp_job **out, const double *const *yrows = nullptr) {
    if (!c || !out || !kernels || P <= 0 || n < 0 || d < 0 || m < 0 || D <= 0) return NGP_ERR_ARG;
    if (n + d <= 0) return NGP_ERR_ARG;
    if ((n > 0 && (!t || (!y && !yrows))) || (d > 0 && (!t_add || !y_add)) || (m > 0 && !t_new))
        return NGP_ERR_ARG;
    *out = nullptr;
    auto yrow = [&](int b) { return yrows ? yrows[b] : y + (int64_t)b * ldy; };
    std::vector<DevProgram> hp((size_t)P);
    int maxstat = 0, maxcp = 0;
    for (int i = 0; i < P; ++i) {
        int ns = 0, nc = 0, nt = 0;
        ngp_status st = compile_program(&kernels[i], &hp[(size_t)i], nullptr, &ns, &nc, &nt);
        if (st) return st;
        maxstat = std::max(maxstat, nt);   // value job: one table per maximal stationary subtree
        maxcp = std::max(maxcp, nc);
    }
    JobGeom g{};
    g.B = P;
    g.n0 = (n / NB) * NB;
    g.nb0 = g.n0 / NB;
    g.tail = n - g.n0;
    g.da = g.tail + d;
    g.d = d;
    g.m = m;
    g.naux = g.da + m + 1;
    if (g.naux > NGP_MAX_AUX) return NGP_ERR_TOO_LARGE;
    g.naux_pad = (g.naux + NB - 1) / NB * NB;
    g.D = D;
    g.noise_on_new = noise_on_new ? 1 : 0;
    g.y_shared = (ldy == 0 && !yrows) ? 1 : 0;
    g.ld = g.n0;
    g.item_stride = (int64_t)(g.n0 + g.naux_pad) * g.n0;
    if (item_too_large(g.item_stride)) return NGP_ERR_TOO_LARGE;
    g.npts = g.n0 + g.da + m;
    g.n_real = g.n0;
    g.aux_identity = 0;
    g.maxstat = std::max(maxstat, 1);
    g.maxcp = std::max(maxcp, 1);
    std::vector<int32_t> h_q;
    int32_t toep_stride = 0;
    if (g.n0 > 0) {
        std::vector<double> allt((size_t)g.npts);
        for (int i = 0; i < n; ++i) allt[(size_t)i] = t[i];
        for (int a = 0; a < d; ++a) allt[(size_t)(n + a)] = t_add[a];
        for (int i = 0; i < m; ++i) allt[(size_t)(n + d + i)] = t_new[i];
        double hh = 0.0;
        int R = 0;
        if (detect_lattice(allt, &hh, &h_q, &R)) {
            g.lattice = 1;
            g.h = hh;
            g.R = R;
            // the main block at a constant lattice stride (a regular series — every one the
            // reference's tests and vignettes fit): K of a stationary tree is Toeplitz there and
            // its off-diagonal tiles are never stored (JobGeom::toep).  fp64 value jobs with at
            // least one tile below the diagonal; mixed precision keeps every tile (its shadow
            // copies and tile maxima come from the stored rows).
            if (g.nb0 >= 2) {
                const long st0 = (long)h_q[1] - (long)h_q[0];
                bool reg = st0 != 0;
                for (int i = 2; i < g.n0 && reg; ++i)
                    reg = (long)h_q[(size_t)i] - (long)h_q[(size_t)i - 1] == st0;
                if (reg) toep_stride = (int32_t)std::labs(st0);
            }
        }
    }

    // (the job before the scope: on a failure the scope ends, synchronised, before the job is destroyed)
    std::unique_ptr<ngp_job, void (*)(ngp_job *)> job(new (std::nothrow) ngp_job(), ngp_job_destroy);
    ngp_job *j = job.get();
    if (!j) return NGP_ERR_TOO_LARGE;
    j->ctx = c;
    DevCall call(c);
    g.invariant = c->invariant ? 1 : 0;
    g.short_series = c->short_series ? 1 : 0;
    if (stores_structured(g, P, c->toeplitz, c->spec.precision)) g.toep = toep_stride;
    j->g = g;
    j->n = n;
    j->spec = c->spec;
    const int ny = g.y_shared ? 1 : P;
    if (g.lattice && g.n0 > 0) j->fill.sort_items(hp.data(), P);
    // ONE device arena for everything that crosses the bus, inputs first, outputs last:
    //   [programs | t0 | taux | y0 | ya | lattice indices | fill lists | logdet | info |
    //    logml_base | logml_full | mu | sigma]
    // The inputs go up in ONE copy (logdet and info arrive as the zeros the first run expects) and
    // a small job's results come back in one (ngp_job_fetch): the 24- and 64-particle calls of a
    // fit on a short series are chains of dependent launches a few microseconds long, and every
    // separate copy or memset was one more link (ten copies and two memsets before).
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += al(std::max<size_t>(bytes, 8)); return o; };
    const size_t n_t0 = (size_t)std::max(g.n0, 1), n_taux = (size_t)std::max(g.da + m, 1),
                 n_y0 = (size_t)std::max(ny * g.n0, 1),
                 n_ya = (size_t)std::max((int64_t)ny * D * g.da, (int64_t)1);
    const size_t o_progs = take(sizeof(DevProgram) * (size_t)P), o_t0 = take(8 * n_t0),
                 o_taux = take(8 * n_taux), o_y0 = take(8 * n_y0), o_ya = take(8 * n_ya),
                 o_q = take(g.lattice ? 4 * (size_t)g.npts : 0);
    j->fill.layout(take);
    const size_t o_logdet = take(8 * (size_t)P), o_info = take(4 * (size_t)P);
    const size_t in_bytes = off;
    const size_t o_lb = take(8 * (size_t)P), o_lf = take(8 * (size_t)P * D),
                 o_mu = take(m > 0 ? 8 * (size_t)P * D * m : 0),
                 o_sigma = take(m > 0 ? 8 * (size_t)P * m * m : 0);
    j->h_in.assign(in_bytes, 0);
    {
        unsigned char *h = j->h_in.data();
        std::memcpy(h + o_progs, hp.data(), sizeof(DevProgram) * (size_t)P);
        if (g.n0 > 0) std::memcpy(h + o_t0, t, 8 * (size_t)g.n0);
        double *h_taux = (double *)(h + o_taux), *h_y0 = (double *)(h + o_y0),
               *h_ya = (double *)(h + o_ya);
        for (int a = 0; a < g.tail; ++a) h_taux[a] = t[g.n0 + a];
        for (int a = 0; a < d; ++a) h_taux[g.tail + a] = t_add[a];
        for (int i = 0; i < m; ++i) h_taux[g.da + i] = t_new[i];
        for (int b = 0; b < ny; ++b)
            if (g.n0 > 0) std::memcpy(h_y0 + (size_t)b * g.n0, yrow(b), 8 * (size_t)g.n0);
        for (int b = 0; b < ny; ++b)
            for (int sc = 0; sc < D; ++sc) {
                double *dst = h_ya + ((size_t)b * D + sc) * g.da;
                for (int a = 0; a < g.tail; ++a) dst[a] = yrow(b)[g.n0 + a];
                for (int a = 0; a < d; ++a)
                    dst[g.tail + a] = y_add[(int64_t)b * ld_yadd_item + (int64_t)sc * d + a];
            }
        if (g.lattice) std::memcpy(h + o_q, h_q.data(), 4 * (size_t)g.npts);
        j->fill.copy_to(h);
    }
    unsigned char *io = nullptr;
    j->work_stride = (int64_t)g.da * g.da + (int64_t)m * g.da + g.da + 8;
    call.keep(&io, off, &j->owned)
        .keep(&j->G, (size_t)P * g.naux * g.naux, &j->owned)
        .keep(&j->work, (size_t)P * j->work_stride, &j->owned)
        .keep(&j->zbuf, (size_t)std::max((int64_t)P * D * g.da, (int64_t)1), &j->owned);
    if (call.status()) return call.status();   // nothing is queued yet
    j->progs = (DevProgram *)(io + o_progs);
    j->t0 = (double *)(io + o_t0);
    j->taux = (double *)(io + o_taux);
    j->y0 = (double *)(io + o_y0);
    j->ya = (double *)(io + o_ya);
    if (g.lattice) j->qpts = (int32_t *)(io + o_q);
    if (g.lattice && g.n0 > 0) j->fill_io = io;
    j->logdet = (double *)(io + o_logdet);
    j->info = (int32_t *)(io + o_info);
    j->logml_base = (double *)(io + o_lb);
    j->logml_full = (double *)(io + o_lf);
    if (m > 0) {
        j->mu = (double *)(io + o_mu);
        j->sigma = (double *)(io + o_sigma);
    }
    j->out_off[0] = 0;                     // offsets inside the result region, which starts at info
    j->out_off[1] = o_lb - o_info;
    j->out_off[2] = o_lf - o_info;
    j->out_off[3] = o_mu - o_info;
    j->out_off[4] = o_sigma - o_info;
    j->out_bytes = off - o_info;
    const ngp_status st = stage_up(call, c->stream, io, j->h_in, in_bytes);
    if (st) return st;
    j->zeroed = true;
    j->copy_in_flight = !j->h_in.empty();
    *out = job.release();
    return NGP_OK;
}

}  // namespace

namespace {

// what the epilogue reads and writes, from a staged job (tab / sig / qpts: the caller's, when resident)
EpiPtrs epi_ptrs_of(const ngp_job &j) {
    EpiPtrs e{};
    e.progs = j.progs;
    e.taux = j.taux;
    e.G = j.G;
    e.ya = j.ya;
    e.logdet = j.logdet;
    e.info = j.info;
    e.work = j.work;
    e.zbuf = j.zbuf;
    e.logml_base = j.logml_base;
    e.logml_full = j.logml_full;
    e.mu = j.mu;
    e.sigma = j.sigma;
    e.work_stride = j.work_stride;
    return e;
}

// One attempt at a run's working storage: `layout` is walked twice through the same sequence of
// requests (WsPlan), once to add the sizes up and reserve the workspace in one piece, once to take
// the pieces.  NGP_ERR_TOO_LARGE: the caller cuts its chunk (each by its own policy) and tries again.
template <class Layout> ngp_status ws_layout(ngp_ctx *c, Layout &&layout) {
    WsPlan measure{c, true}, take{c, false};
    (void)layout(measure);
    ngp_status st = c->ws_reserve(measure.total);
    if (!st) st = layout(take);
    return st;
}

// Device buffers of the Gram refinement of one chunk (NGP_PREC_MIXED).
struct RefineBufs {
    double *X = nullptr, *A = nullptr, *R = nullptr;   // [Bc][naux_pad][n0]
    double *S = nullptr, *T = nullptr;                 // [Bc][naux^2]
    double *U = nullptr;                               // [Bc][naux]
    double *delta = nullptr;                           // [Bc][2]
    int32_t *items = nullptr;                          // [Bc] items a later step still works on
};

// What the refinement of a chunk keeps on the host.  Queued copies read and write these: the owner
// declares them before the run's scope.
struct RefineHost {
    std::vector<double> dprev, dboth;
    std::vector<int32_t> active, still;
};

// G <- X K^-1 X' refined against the fp64 covariance (see kapply_kernel).  On entry the aux rows
// of the slab hold W = X L^-T and p.dinv every block inverse M_j ([nb0][mstep]).  steps / delta
// (host, [bc]) receive the per-item step count and last correction; the items that did not reach
// `tol` within `max_steps` go to not_refined.  Every step reads its corrections back: one wait() of
// the run's scope each, and nothing of it is in flight when this returns.
void refine_chunk(DevCall &call, hipStream_t s, const JobGeom &g, const ChunkPtrs &p, const RefineBufs &rb,
                  double *Gchunk, int bc, size_t mstep, const ngp_spec &spec, const DevSpec &sp,
                  RefineHost &h, int32_t *steps, double *delta_out, std::vector<int> *not_refined) {
    EventTimer &tm = call.tm;
    const double naux = (double)g.naux, n0 = (double)g.n0;
    ChunkPtrs pf = p;          // the sweeps are fp64: no shadow rows, no tile maxima
    pf.L32 = nullptr;
    pf.tmax = nullptr;
    pf.mixcnt = nullptr;
    pf.auxX = nullptr;
    int na = bc;               // items still being refined (pf.items: their indices; null = all)
    auto backward = [&](int accumulate) {
        for (int cc = g.nb0 - 1; cc >= 0; --cc)
            call.timed(tm, 10, na * naux * 2.0 * NB * (double)(cc + 1) * NB,
                       na * 8.0 * ((double)NB * NB * (cc + 1) + 2.0 * naux * NB * (cc + 1)), [&] {
                           launch_aux_back(g, pf, p.dinv, mstep, rb.A, accumulate, na, cc, s);
                       });
    };
    backward(0);               // A_0 = W L^-1
    h.dprev.assign((size_t)bc, 1.0);
    h.dboth.assign(2 * (size_t)bc, 0.0);
    h.active.resize((size_t)bc);
    for (int i = 0; i < bc; ++i) { steps[i] = 0; delta_out[i] = 0.0; h.active[(size_t)i] = i; }
    for (int it = 1;; ++it) {
        call.timed(tm, 10, na * 2.0 * naux * n0 * n0, na * 8.0 * 3.0 * naux * n0,
                   [&] { launch_kapply(g, pf, rb.A, rb.X, rb.R, na, sp, s); });
        call.timed(tm, 10, na * 4.0 * naux * naux * n0, na * 8.0 * 3.0 * naux * n0, [&] {
            launch_refine_gram(g, rb.A, rb.X, rb.R, rb.S, rb.T, rb.U, Gchunk, rb.delta, na, pf.items, s);
        });
        if (call.down(h.dboth.data(), rb.delta, sizeof(double) * 2 * (size_t)bc).wait()) break;
        h.still.clear();
        for (int i : h.active) {
            const double d = h.dboth[2 * (size_t)i];
            // What is left after this step's correction d is about d * rho, rho the contraction
            // of the iteration: measured as d / d_previous from the second step on, and from the
            // residual itself (max_a |R_a| / |X_a|) at the first, whichever is larger.
            double rho = h.dboth[2 * (size_t)i + 1];
            if (it > 1) rho = std::max(rho, d / h.dprev[(size_t)i]);
            const double est = d * std::min(rho, 1.0);
            steps[i] = it;
            delta_out[i] = d;
            h.dprev[(size_t)i] = d;
            if (!(est <= spec.refine_tol)) h.still.push_back(i);   // NaN stays
        }
        h.active.swap(h.still);
        if (h.active.empty() || it >= spec.refine_max) break;
        // the next step only touches the items that are not there yet (h.active is not written again
        // before the next wait)
        na = (int)h.active.size();
        call.up(rb.items, h.active.data(), 4 * (size_t)na);
        pf.items = rb.items;
        // A += (R L^-T) L^-1: R into the aux rows, forward sweep (the resident-factor kernels),
        // backward sweep accumulating into A
        for (int i : h.active)
            call.move(p.L + (size_t)i * g.item_stride + (size_t)g.n0 * g.ld, rb.R + (size_t)i * g.naux_pad * g.n0,
                      (size_t)g.naux_pad * g.n0 * 8);
        for (int jj = 0; jj < g.nb0; ++jj) {
            ChunkPtrs pj = pf;
            pj.dinv = p.dinv + (size_t)jj * mstep;
            call.timed(tm, 10, na * naux * (double)NB * NB, na * 8.0 * 3.0 * naux * NB,
                       [&] { launch_chol_col(g, pj, na, jj, COL_AUX, jj * NB, s); });
            call.timed(tm, 10, na * naux * 2.0 * NB * (double)(g.n0 - (jj + 1) * NB),
                       na * 8.0 * (g.n0 - (jj + 1) * NB) * (2.0 * naux + NB),
                       [&] { launch_aux_update(g, pj, na, jj, s); });
        }
        backward(1);
    }
    if (!call.status()) not_refined->assign(h.active.begin(), h.active.end());
}

// what a chunk's kernels read of a staged job, from item b0 on; the factor storage and the tables are
// the caller's (the workspace of a run, a resident factor)
ChunkPtrs chunk_ptrs_of(const ngp_job &j, int b0, double *L, double *dinv, double *tab, double *sig) {
    ChunkPtrs p{};
    p.L = L;
    p.dinv = dinv;
    p.progs = j.progs + b0;
    p.t0 = j.t0;
    p.taux = j.taux;
    p.y0 = j.y0 + (j.g.y_shared ? 0 : (int64_t)b0 * j.g.n0);
    p.logdet = j.logdet + b0;
    p.info = j.info + b0;
    p.tab = tab;
    p.sig = sig;
    p.qpts = j.qpts;
    return p;
}

}  // namespace

extern "C" ngp_status ngp_job_run(ngp_job *j) {
    if (!j) return NGP_ERR_ARG;
    ngp_ctx *c = j->ctx;
    // host memory that queued copies of the run write (mixed jobs): before the scope, which ends synchronised
    std::vector<unsigned> hc;
    std::vector<int32_t> hi;
    RefineHost rh;
    DevCall call(c);
    EventTimer &tm = call.tm;
    const JobGeom &g = j->g;
    hipStream_t s = c->stream;
    const DevSpec sp = dev_spec(j->spec);
    // a re-run: the first one finds the zeros the staging copy brought.  (Short jobs: chol_small_kernel
    // writes both outright; whatever the chunk size turns out to be, it is at most the batch.)
    if (!j->zeroed && !(g.n0 > 0 && small_job(g, g.B) && j->spec.precision != NGP_PREC_MIXED))
        call.zero(j->logdet, sizeof(double) * (size_t)g.B).zero(j->info, sizeof(int32_t) * (size_t)g.B);
    const bool mixed = mixed_eligible(g, j->spec.precision);
    const bool refine = mixed && j->spec.refine_max > 0;
    j->refine_steps.assign((size_t)g.B, 0);
    j->refine_delta.assign((size_t)g.B, 0.0);
    j->frac32.assign((size_t)g.B, 0.0);
    // the run's working storage comes from the context's workspace (ngp_ctx::ws_reserve): nothing
    // to give back, the next call overwrites it
    void *Lbuf = nullptr, *dinv = nullptr, *tab = nullptr, *sig = nullptr;
    void *L32 = nullptr, *tmx = nullptr, *cnt = nullptr, *order_buf = nullptr, *order_prev = nullptr;
    RefineBufs rb;
    bool single_chunk = false;
    if (g.n0 > 0) {
        const size_t tab_bytes = g.lattice ? sizeof(double) * (size_t)g.maxstat * g.R : 0;
        const size_t sig_bytes = g.lattice ? sizeof(double) * (size_t)g.maxcp * g.npts : 0;
        const size_t l_bytes = (size_t)g.item_stride * sizeof(double);
        const size_t nbt = (size_t)g.nb0 + (size_t)g.naux_pad / NB;
        const size_t aux_bytes = sizeof(double) * (size_t)g.naux_pad * g.n0;
        size_t item_bytes = l_bytes + tab_bytes + sig_bytes + sizeof(double) * NB * NB;
        if (mixed)
            item_bytes += l_bytes / 2 + 4 * nbt * g.nb0 + aux_bytes + 16 +
                          (refine ? sizeof(double) * NB * NB * (size_t)g.nb0 + 2 * aux_bytes +
                                        16 * (size_t)g.naux * g.naux + 8 * (size_t)g.naux + 20
                                  : 0);
        // as few chunks as the memory allows, of equal size (a short last chunk runs every launch
        // of the sweep again for a fraction of the items)
        // (several kernels index the items of a chunk with blockIdx.y: at most 65,535 of them)
        if ((size_t)g.B * item_bytes > c->mem_cap) c->refresh_mem_cap();   // large job: today's figure
        const size_t bc_max = std::min<size_t>(
            std::min<size_t>((size_t)g.B, MAX_CHUNK_ITEMS), std::max<size_t>(1, c->mem_cap / item_bytes));
        size_t nchunks = ((size_t)g.B + bc_max - 1) / bc_max;
        int Bc = 0;
        size_t mstep = 0;
        ngp_status st = NGP_OK;
        // the estimate above leaves the allocator's rounding and other live handles out: when an
        // allocation fails the job is cut into more chunks instead of being refused
        auto take_all = [&](WsPlan &dalloc) -> ngp_status {
            ngp_status st = dalloc(&Lbuf, l_bytes * (size_t)Bc);
            if (!st) st = dalloc(&dinv, sizeof(double) * (size_t)Bc * NB * NB * (refine ? g.nb0 : 1));
            if (!st && g.lattice) st = dalloc(&tab, tab_bytes * (size_t)Bc);
            if (!st && g.lattice) st = dalloc(&sig, sig_bytes * (size_t)Bc);
            if (!st && mixed) {
                st = dalloc(&L32, (l_bytes / 2) * (size_t)Bc);
                if (!st) st = dalloc(&tmx, 4 * nbt * g.nb0 * (size_t)Bc);
                if (!st) st = dalloc(&cnt, 8 * (size_t)Bc);
                if (!st) st = dalloc(&order_buf, 4 * (size_t)Bc);
                if (!st) st = dalloc(&order_prev, 4 * (size_t)Bc);
                if (!st) st = dalloc((void **)&rb.X, aux_bytes * (size_t)Bc);
            }
            if (!st && refine) {
                st = dalloc((void **)&rb.A, aux_bytes * (size_t)Bc);
                if (!st) st = dalloc((void **)&rb.R, aux_bytes * (size_t)Bc);
                if (!st) st = dalloc((void **)&rb.S, 8 * (size_t)g.naux * g.naux * Bc);
                if (!st) st = dalloc((void **)&rb.T, 8 * (size_t)g.naux * g.naux * Bc);
                if (!st) st = dalloc((void **)&rb.U, 8 * (size_t)g.naux * Bc);
                if (!st) st = dalloc((void **)&rb.delta, 16 * (size_t)Bc);
                if (!st) st = dalloc((void **)&rb.items, 4 * (size_t)Bc);
            }
            return st;
        };
        for (;; nchunks *= 2) {
            Bc = (int)(((size_t)g.B + nchunks - 1) / nchunks);
            // refinement sweeps need every block inverse M_j, not only the current one
            mstep = refine ? (size_t)Bc * NB * NB : 0;
            st = ws_layout(c, take_all);
            if (st != NGP_ERR_TOO_LARGE || Bc <= 1) break;
        }
        single_chunk = Bc >= g.B;
        call.fail(st);
        const Lane ln = lane_of(c);
        std::vector<int> bad;
        for (int b0 = 0; b0 < g.B && !call.status(); b0 += Bc) {
            const int bc = std::min(Bc, g.B - b0);
            ChunkPtrs p = chunk_ptrs_of(*j, b0, (double *)Lbuf, (double *)dinv, (double *)tab, (double *)sig);
            if (j->fill_io) j->fill.share_of(j->fill_io, b0, bc, &p);
            if (mixed) {
                p.L32 = (float *)L32;
                p.tmax = (float *)tmx;
                p.mixcnt = (unsigned *)cnt;
                p.auxX = rb.X;
                call.zero(cnt, 8 * (size_t)bc);
            }
            if (g.lattice) call.timed(tm, 4, 0.0, 0.0, [&] { launch_tables(g, p, bc, sp, s); });
            call.timed(tm, cost_fill(g, bc, p.n_fill_single), [&] { launch_fill(g, p, bc, sp, s); });
            if (mixed) call.zero(order_prev, 4 * (size_t)bc);
            double *Gchunk = j->G + (int64_t)b0 * g.naux * g.naux;
            // short jobs: the one launch of the factorisation leaves G too
            const bool gram_inside = !mixed && mstep == 0 && small_job(g, bc);
            if (gram_inside) p.G = Gchunk;
            call.run([&] {
                factor_chunk(ln, g, p, bc, tm, mstep, mixed ? &sp : nullptr, (int32_t *)order_buf,
                             (unsigned *)order_prev);
            });
            if (!gram_inside)
                call.timed(tm, cost_gram(g, bc), [&] { launch_gram(g, (const double *)Lbuf, Gchunk, bc, s); });
            if (!mixed) continue;
            hc.assign(2 * (size_t)bc, 0u);
            call.down(hc.data(), cnt, 8 * (size_t)bc);
            bad.clear();
            if (refine)
                refine_chunk(call, s, g, p, rb, Gchunk, bc, mstep, j->spec, sp, rh, j->refine_steps.data() + b0,
                             j->refine_delta.data() + b0, &bad);
            if (call.wait()) break;
            for (int i = 0; i < bc; ++i) {
                const double a = hc[2 * (size_t)i], b = hc[2 * (size_t)i + 1];
                j->frac32[(size_t)(b0 + i)] = (a + b) > 0.0 ? a / (a + b) : 0.0;
            }
            if (!bad.empty()) {   // keep a pivot failure if the factorisation reported one
                hi.assign((size_t)bc, 0);
                if (call.down(hi.data(), p.info, 4 * (size_t)bc).wait()) break;
                for (int i : bad)
                    if (hi[(size_t)i] == 0) hi[(size_t)i] = NGP_INFO_NOT_REFINED;
                (void)call.up(p.info, hi.data(), 4 * (size_t)bc).wait();   // hi is the next chunk's too
            }
        }
    }
    EpiPtrs e = epi_ptrs_of(*j);
    // (batch-invariant jobs evaluate the small Schur blocks directly, whatever the number of chunks)
    if (g.lattice && single_chunk && !g.invariant) {   // the tables of the only chunk are still in place
        e.tab = (const double *)tab;
        e.sig = (const double *)sig;
        e.qpts = j->qpts;
    }
    call.timed(tm, 3, 0.0, 0.0, [&] { launch_epilogue(g, e, sp, s); });
    // small results travel behind the last kernel, in the same queue: a fetch after the run's
    // synchronisation would be a second host round trip (25 us of a 24-item call: the copy started
    // that long after the epilogue had ended)
    const bool packed = j->out_bytes <= FETCH_PACKED_BYTES;
    if (packed) {
        j->h_out.resize(j->out_bytes);
        call.down(j->h_out.data(), j->info, j->out_bytes);
    }
    const ngp_status st = call.sync();
    j->run_ended(st, packed);
    return st;
}

extern "C" ngp_status ngp_job_mixed_stats(ngp_job *j, int32_t *refine_steps, double *refine_delta,
                                          double *frac_f32) {
    if (!j) return NGP_ERR_ARG;
    if (!j->ran) return NGP_ERR_STATE;
    for (int i = 0; i < j->g.B; ++i) {
        if (refine_steps) refine_steps[i] = j->refine_steps[(size_t)i];
        if (refine_delta) refine_delta[i] = j->refine_delta[(size_t)i];
        if (frac_f32) frac_f32[i] = j->frac32[(size_t)i];
    }
    return NGP_OK;
}

// (j->ran: a run has synchronised since the job was staged, so no staging copy is in flight)
extern "C" ngp_status ngp_job_fetch(ngp_job *j, double *logml_base, double *logml_full, double *mu,
                                    double *sigma, int32_t *info) {
    if (!j) return NGP_ERR_ARG;
    if (!j->ran) return NGP_ERR_STATE;
    const JobGeom &g = j->g;
    const size_t B = (size_t)g.B;
    const bool packed = j->out_bytes <= FETCH_PACKED_BYTES;   // small results: one copy of the whole region
    DevCall call(j->ctx);
    if (packed) {
        if (!j->out_fetched) {   // (normally ngp_job_run has brought it already)
            j->h_out.resize(j->out_bytes);
            call.down(j->h_out.data(), j->info, j->out_bytes);
        }
    } else {
        if (logml_base) call.down(logml_base, j->logml_base, 8 * B);
        if (logml_full) call.down(logml_full, j->logml_full, 8 * B * g.D);
        if (mu && g.m > 0) call.down(mu, j->mu, 8 * B * g.D * g.m);
        if (sigma && g.m > 0) call.down(sigma, j->sigma, 8 * B * g.m * g.m);
        if (info) call.down(info, j->info, 4 * B);
    }
    const ngp_status st = call.sync();
    if (st || !packed) return st;
    const unsigned char *h = j->h_out.data();
    if (info) std::memcpy(info, h + j->out_off[0], 4 * B);
    if (logml_base) std::memcpy(logml_base, h + j->out_off[1], 8 * B);
    if (logml_full) std::memcpy(logml_full, h + j->out_off[2], 8 * B * g.D);
    if (mu && g.m > 0) std::memcpy(mu, h + j->out_off[3], 8 * B * g.D * g.m);
    if (sigma && g.m > 0) std::memcpy(sigma, h + j->out_off[4], 8 * B * g.m * g.m);
    return NGP_OK;
}

extern "C" void ngp_job_destroy(ngp_job *j) {
    if (!j) return;
    {
        DevCall call(j->ctx);
        // staged but never run: the staging copy may still be reading j->h_in
        if (j->copy_in_flight) call.pending();
        (void)call.sync();
        for (void *p : j->owned) j->ctx->release(p);
    }
    delete j;
}

// ---------------------------------------------------------------------------------------
// staged + one-shot entry points
// ---------------------------------------------------------------------------------------
extern "C" ngp_status ngp_logml_stage(ngp_ctx *c, int32_t B, const ngp_kernel *k, int32_t n,
                                      const double *t, const double *y, int64_t ldy,
                                      ngp_job **job) {
    if (n <= 0) return NGP_ERR_ARG;
    static const double dummy = 0.0;
    return stage_general(c, B, k, n, t, y, ldy, 0, &dummy, 1, &dummy, 0, 0, nullptr, 0, job);
}

extern "C" ngp_status ngp_predict_stage(ngp_ctx *c, int32_t B, const ngp_kernel *k, int32_t n,
                                        const double *t, const double *y, int64_t ldy, int32_t m,
                                        const double *t_new, int32_t noise_on_new, ngp_job **job) {
    if (n <= 0 || m <= 0) return NGP_ERR_ARG;
    static const double dummy = 0.0;
    return stage_general(c, B, k, n, t, y, ldy, 0, &dummy, 1, &dummy, 0, m, t_new, noise_on_new,
                         job);
}

extern "C" ngp_status ngp_nowcast_stage(ngp_ctx *c, int32_t P, const ngp_kernel *k, int32_t n,
                                        const double *t, const double *y, int32_t d,
                                        const double *t_add, int32_t D, const double *y_add,
                                        int32_t m, const double *t_new, int32_t noise_on_new,
                                        ngp_job **job) {
    if (n <= 0 || d < 0 || D <= 0) return NGP_ERR_ARG;
    static const double dummy = 0.0;
    if (d == 0) { t_add = &dummy; y_add = &dummy; }
    return stage_general(c, P, k, n, t, y, 0, d, t_add, D, y_add, 0, m, t_new, noise_on_new, job);
}

static ngp_status run_fetch_destroy(ngp_job *job, double *lb, double *lf, double *mu,
                                    double *sigma, int32_t *info) {
    ngp_status st = ngp_job_run(job);
    if (!st) st = ngp_job_fetch(job, lb, lf, mu, sigma, info);
    ngp_job_destroy(job);
    return st;
}

static ngp_status logml_direct(ngp_ctx *c, int32_t B, const ngp_kernel *k, int32_t n,
                               const double *t, const double *y, int64_t ldy, double *logml,
                               int32_t *info) {
    ngp_job *job = nullptr;
    ngp_status st = ngp_logml_stage(c, B, k, n, t, y, ldy, &job);
    if (st) return st;
    return run_fetch_destroy(job, nullptr, logml, nullptr, nullptr, info);
}

static ngp_status predict_direct(ngp_ctx *c, int32_t B, const ngp_kernel *k, int32_t n,
                                 const double *t, const double *y, int64_t ldy, int32_t m,
                                 const double *t_new, int32_t noise_on_new, double *mu,
                                 double *sigma, double *logml, int32_t *info) {
    ngp_job *job = nullptr;
    ngp_status st = ngp_predict_stage(c, B, k, n, t, y, ldy, m, t_new, noise_on_new, &job);
    if (st) return st;
    return run_fetch_destroy(job, nullptr, logml, mu, sigma, info);
}

// (ngp_logml_batch, ngp_predict_batch, ngp_logml_grad_batch and ngp_mixture_sample are defined in
// the "combining" section further down: they enter through combine_submit)

extern "C" ngp_status ngp_nowcast_batch(ngp_ctx *c, int32_t P, const ngp_kernel *k, int32_t n,
                                        const double *t, const double *y, int32_t d,
                                        const double *t_add, int32_t D, const double *y_add,
                                        int32_t m, const double *t_new, int32_t noise_on_new,
                                        double *logml_base, double *logml_full, double *mu,
                                        double *sigma, int32_t *info) {
    ngp_job *job = nullptr;
    ngp_status st = ngp_nowcast_stage(c, P, k, n, t, y, d, t_add, D, y_add, m, t_new, noise_on_new,
                                      &job);
    if (st) return st;
    return run_fetch_destroy(job, logml_base, logml_full, mu, sigma, info);
}

// ---------------------------------------------------------------------------------------
// cached factor
// ---------------------------------------------------------------------------------------
struct ngp_factor {
    ngp_ctx *ctx = nullptr;
    int P = 0, n = 0;
    int64_t ldy = 0;
    std::vector<std::vector<int32_t>> ops;
    std::vector<std::vector<double>> params;
    std::vector<ngp_kernel> kernels;      // point into ops / params
    std::vector<double> t, y;             // y: [P or 1][n] packed
    int n0 = 0, nb0 = 0;
    int64_t item_stride = 0;              // (n0 + NGP_MAX_AUX) x n0 doubles
    double *L = nullptr;                  // [P][item_stride]
    double *dinv = nullptr;               // [nb0][P][64 x 64]
    double *logdet = nullptr;             // [P] sum log diag L of the main block
    int32_t *info = nullptr;              // [P]
    std::vector<double> logml0;
    std::vector<int32_t> info0;
    ngp_spec spec{};                      // the spec the factor was created under (always fp64)
};

namespace {

// run the job of a cached-factor query: only the aux rows are filled and swept
// comp (ngp_factor_components): the job's forecast rows are component rows — filled a second time
// under their own programs, and read by the component epilogue (comp_work: its [B][stride] buffer)
ngp_status factor_run(ngp_factor *f, ngp_job *j, bool create, const CompPtrs *comp = nullptr,
                      double *comp_work = nullptr, int64_t comp_work_stride = 0) {
    ngp_ctx *c = f->ctx;
    DevCall call(c);
    EventTimer &tm = call.tm;
    JobGeom &g = j->g;
    g.item_stride = f->item_stride;
    hipStream_t s = c->stream;
    j->spec = f->spec;
    const DevSpec sp = dev_spec(f->spec);
    const int P = f->P;
    const size_t ld_bytes = sizeof(double) * (size_t)P, info_bytes = sizeof(int32_t) * (size_t)P;
    double *tab = nullptr, *sig = nullptr;
    if (g.n0 > 0) {
        if (g.lattice) call.take(&tab, (size_t)g.maxstat * g.R * P).take(&sig, (size_t)g.maxcp * g.npts * P);
        const ChunkPtrs p = chunk_ptrs_of(*j, 0, f->L, f->dinv, tab, sig);
        const size_t mstep = (size_t)P * NB * NB;
        if (g.lattice) call.timed(tm, 4, 0.0, 0.0, [&] { launch_tables(g, p, P, sp, s); });
        if (create) {
            call.zero(j->logdet, ld_bytes).zero(j->info, info_bytes);
            call.timed(tm, cost_fill(g, P, 0), [&] { launch_fill(g, p, P, sp, s); });
            call.run([&] { factor_chunk(lane_of(c), g, p, P, tm, mstep); });
            call.move(f->logdet, j->logdet, ld_bytes).move(f->info, j->info, info_bytes);
        } else {
            call.move(j->logdet, f->logdet, ld_bytes).move(j->info, f->info, info_bytes);
            call.timed(tm, cost_fill_aux(g, P), [&] { launch_fill(g, p, P, sp, s, /*aux_only=*/true); });
            if (comp)
                call.timed(tm, 4, 0.0, 8.0 * P * (double)g.m * g.n0, [&] { launch_component_fill(g, p, *comp, P, sp, s); });
            // right-looking sweep of the aux rows through the resident factor
            for (int jj = 0; jj < g.nb0; ++jj) {
                ChunkPtrs pj = p;
                pj.dinv = f->dinv + (size_t)jj * mstep;
                call.timed(tm, cost_aux_solve(g, P), [&] { launch_chol_col(g, pj, P, jj, COL_AUX, jj * NB, s); });
                call.timed(tm, cost_aux_update(g, P, jj), [&] { launch_aux_update(g, pj, P, jj, s); });
            }
        }
        call.timed(tm, cost_gram(g, P), [&] { launch_gram(g, f->L, j->G, P, s); });
    } else {
        call.zero(j->logdet, ld_bytes).zero(j->info, info_bytes);
    }
    EpiPtrs e = epi_ptrs_of(*j);
    if (g.lattice && g.n0 > 0) {
        e.tab = tab;
        e.sig = sig;
        e.qpts = j->qpts;
    }
    if (comp) {
        e.work = comp_work;
        e.work_stride = comp_work_stride;
        call.timed(tm, 3, 0.0, 0.0, [&] { launch_component_epilogue(g, e, *comp, sp, s); });
    } else {
        call.timed(tm, 3, 0.0, 0.0, [&] { launch_epilogue(g, e, sp, s); });
    }
    const ngp_status st = call.sync();
    j->run_ended(st, false);
    return st;
}

}  // namespace

extern "C" ngp_status ngp_factor_create(ngp_ctx *c, int32_t P, const ngp_kernel *kernels,
                                        int32_t n, const double *t, const double *y, int64_t ldy,
                                        ngp_factor **out) {
    if (!c || !out || !kernels || !t || !y || P <= 0 || n <= 0) return NGP_ERR_ARG;
    *out = nullptr;
    if ((size_t)P > MAX_CHUNK_ITEMS) return NGP_ERR_TOO_LARGE;   // a resident factor is one chunk
    for (int i = 0; i < P; ++i) {
        ngp_status st = check_program(&kernels[i]);
        if (st) return st;
    }
    ngp_factor *f = new (std::nothrow) ngp_factor();
    if (!f) return NGP_ERR_TOO_LARGE;
    f->ctx = c;
    f->P = P;
    f->n = n;
    (void)ngp_get_spec(c, &f->spec);
    f->spec.precision = NGP_PREC_F64;     // a resident factor is queried many times: keep it exact
    f->ldy = ldy ? n : 0;
    f->ops.resize((size_t)P);
    f->params.resize((size_t)P);
    f->kernels.resize((size_t)P);
    for (int i = 0; i < P; ++i) {
        f->ops[(size_t)i].assign(kernels[i].ops, kernels[i].ops + kernels[i].n_ops);
        f->params[(size_t)i].assign(kernels[i].params, kernels[i].params + kernels[i].n_params);
        f->kernels[(size_t)i] = kernels[i];
        f->kernels[(size_t)i].ops = f->ops[(size_t)i].data();
        f->kernels[(size_t)i].params = f->params[(size_t)i].data();
    }
    f->t.assign(t, t + n);
    const int ny = ldy ? P : 1;
    f->y.resize((size_t)ny * n);
    for (int b = 0; b < ny; ++b)
        for (int i = 0; i < n; ++i) f->y[(size_t)b * n + i] = y[(int64_t)b * ldy + i];
    f->n0 = (n / NB) * NB;
    f->nb0 = f->n0 / NB;
    f->item_stride = (int64_t)(f->n0 + NGP_MAX_AUX) * f->n0;
    if (item_too_large(f->item_stride)) {
        delete f;
        return NGP_ERR_TOO_LARGE;
    }
    ngp_status st = NGP_OK;
    {
        DevCall call(c);
        if (call.status()) st = NGP_ERR_NO_DEVICE;
        if (f->n0 > 0) call.keep(&f->L, (size_t)f->item_stride * P).keep(&f->dinv, (size_t)f->nb0 * P * NB * NB);
        if (!st) st = call.keep(&f->logdet, (size_t)P).keep(&f->info, (size_t)P).status();
    }
    ngp_job *job = nullptr;
    static const double dummy = 0.0;
    if (!st)
        st = stage_general(c, P, f->kernels.data(), n, f->t.data(), f->y.data(), f->ldy, 0, &dummy,
                           1, &dummy, 0, 0, nullptr, 0, &job);
    if (!st) st = factor_run(f, job, /*create=*/true);
    f->logml0.resize((size_t)P);
    f->info0.resize((size_t)P);
    if (!st) st = ngp_job_fetch(job, nullptr, f->logml0.data(), nullptr, nullptr, f->info0.data());
    ngp_job_destroy(job);
    if (st) {
        ngp_factor_destroy(f);
        return st;
    }
    *out = f;
    return NGP_OK;
}

extern "C" ngp_status ngp_factor_logml(const ngp_factor *f, double *logml, int32_t *info) {
    if (!f) return NGP_ERR_ARG;
    for (int i = 0; i < f->P; ++i) {
        if (logml) logml[i] = f->logml0[(size_t)i];
        if (info) info[i] = f->info0[(size_t)i];
    }
    return NGP_OK;
}

extern "C" ngp_status ngp_factor_nowcast(ngp_factor *f, int32_t d, const double *t_add, int32_t D,
                                         const double *y_add, int32_t m, const double *t_new,
                                         int32_t noise_on_new, double *logml_base,
                                         double *logml_full, double *mu, double *sigma,
                                         int32_t *info) {
    if (!f || d < 0 || D <= 0 || m < 0) return NGP_ERR_ARG;
    static const double dummy = 0.0;
    if (d == 0) { t_add = &dummy; y_add = &dummy; }
    ngp_job *job = nullptr;
    ngp_status st = stage_general(f->ctx, f->P, f->kernels.data(), f->n, f->t.data(), f->y.data(),
                                  f->ldy, d, t_add, D, y_add, 0, m, t_new, noise_on_new, &job);
    if (st) return st;
    st = factor_run(f, job, /*create=*/false);
    if (!st) st = ngp_job_fetch(job, logml_base, logml_full, mu, sigma, info);
    ngp_job_destroy(job);
    return st;
}

// ---- long horizons (DESIGN.md sections 4.25, 4.27 - 4.29) -----------------------------------
// The dates are the panel of a triangular solve against the resident L (ngp_long_kernels.h), not
// aux rows: m is bounded by NGP_MAX_LONG_HORIZON and the device's memory, not by NGP_MAX_AUX.  The
// particles are worked through in chunks sized to what the device holds.
//
// The four entry points share the checks (long_check), the geometry and inputs (long_stage), one
// list of the query's device blocks (LongStage::blocks: bytes per item, takes and uploads are read
// off it) and the run on the device (LongRun: sizing, takes, chunks, a chunk's launches in their one
// order).  An entry point reads: checks, geometry, blocks, per chunk its own steps and downloads.
struct LongBlock {
    void **p;               // null: counted, not taken
    bool per_item;          // `bytes` for every item of a chunk, or for the call
    size_t bytes, spare;    // spare: taken behind the last item, not counted
    const void *host;       // copied up once the blocks are taken
};

struct LongStage {
    LongGeom g{};
    LongPtrs p{};
    std::vector<unsigned char> h_in;   // what travels up: programs | t0 | tp | y0 | yc
    size_t o_t0 = 0, o_tp = 0, o_y0 = 0, o_yc = 0;
    unsigned char *d_in = nullptr;
    size_t cw = 0;                     // the row of S: y' and the conditioning points
    std::vector<LongBlock> blocks;     // in the order they are taken (and given back)
    template <class T> LongStage &per_call(T **q, size_t count, const void *host = nullptr) {
        blocks.push_back({reinterpret_cast<void **>(q), false, sizeof(T) * count, 0, host});
        return *this;
    }
    template <class T> LongStage &per_item(T **q, size_t count, size_t spare = 0) {
        blocks.push_back({reinterpret_cast<void **>(q), true, sizeof(T) * count, sizeof(T) * spare, nullptr});
        return *this;
    }
    // the panel, the small blocks, the dates' diagonal (where the layout has one) and the u_s (an
    // empty z still has an address)
    LongStage &work_blocks(bool has_dg = true) {
        if (g.n0 > 0) per_item(&p.W, (size_t)g.qpad * g.n0);
        per_item(&p.S, (size_t)g.q1 * cw);
        if (has_dg) per_item(&p.dg, (size_t)g.q1);
        return per_item(&p.z, (size_t)g.D * g.c, 1);
    }
    size_t bytes(bool per_item) const {
        size_t n = 0;
        for (const LongBlock &b : blocks) n += b.per_item == per_item ? b.bytes : 0;
        return n;
    }
};

static ngp_status long_check(const ngp_factor *f, int32_t d, const double *t_add, int32_t D,
                             const double *y_add, int32_t m, const double *t_new) {
    if (!f || !t_new || m < 1 || d < 0) return NGP_ERR_ARG;
    if (d > 0 && (D < 1 || !t_add || !y_add)) return NGP_ERR_ARG;
    if (m > NGP_MAX_LONG_HORIZON) return NGP_ERR_TOO_LARGE;
    if ((int64_t)(f->n - f->n0) + d + 1 > NGP_MAX_AUX) return NGP_ERR_TOO_LARGE;
    return NGP_OK;
}

// A query long_check has passed: its geometry and its inputs, the first of its blocks.
// groups = 0: the panel is y', the conditioning rows and the m dates, padded to LONG_TILE as a
// whole; groups = C: the head and each of C groups of date rows are padded on their own (4.28).
// sig_ld: the row stride LongPtrs::sigma is formed with (0: it is not); want_sigma: the kernels
// form a sigma, LongPtrs' or the entry point's own.
static ngp_status long_stage(const ngp_factor *f, int32_t d, const double *t_add, int32_t D,
                             const double *y_add, int32_t m, const double *t_new, int32_t noise_on_new,
                             int32_t groups, int64_t sig_ld, bool want_sigma, LongStage &st) {
    if (d == 0) D = 1;
    const int P = f->P, n = f->n, n0 = f->n0, tail = n - n0, cc = tail + d;
    std::vector<DevProgram> hp((size_t)P);
    for (int i = 0; i < P; ++i)
        if (ngp_status e = compile_program(&f->kernels[(size_t)i], &hp[(size_t)i], nullptr)) return e;
    auto padded = [](int32_t rows) { return (rows + LONG_TILE - 1) / LONG_TILE * LONG_TILE; };
    LongGeom &g = st.g;
    g.n0 = n0, g.nb0 = f->nb0, g.c = cc, g.m = m, g.D = D;
    g.q1 = groups ? padded(1 + cc) + groups * padded(m) : 1 + cc + m;   // 65,534 groups of 4,096 fit
    g.qpad = padded(g.q1);
    g.noise_on_new = noise_on_new ? 1 : 0, g.y_shared = f->ldy ? 0 : 1, g.want_sigma = want_sigma ? 1 : 0;
    g.ld = n0, g.L_stride = f->item_stride, g.dinv_step = (int64_t)P * NB * NB;
    g.sig_ld = sig_ld, g.sig_stride = sig_ld * sig_ld;
    const int ny = g.y_shared ? 1 : P;
    st.o_t0 = sizeof(DevProgram) * (size_t)P, st.o_tp = st.o_t0 + 8 * (size_t)n0;
    st.o_y0 = st.o_tp + 8 * (size_t)(cc + m), st.o_yc = st.o_y0 + 8 * (size_t)ny * n0;
    std::vector<unsigned char> &h_in = st.h_in;
    h_in.resize(st.o_yc + 8 * (size_t)ny * D * cc);
    std::memcpy(h_in.data(), hp.data(), st.o_t0);
    auto at = [&](size_t o) { return reinterpret_cast<double *>(h_in.data() + o); };
    double *h_t0 = at(st.o_t0), *h_tp = at(st.o_tp), *h_y0 = at(st.o_y0), *h_yc = at(st.o_yc);
    std::copy(f->t.begin(), f->t.begin() + n0, h_t0);
    std::copy(f->t.begin() + n0, f->t.end(), h_tp);
    for (int a = 0; a < d; ++a) h_tp[tail + a] = t_add[a];
    std::copy(t_new, t_new + m, h_tp + cc);
    for (int b = 0; b < ny; ++b) {
        const double *yb = f->y.data() + (size_t)b * n;
        std::copy(yb, yb + n0, h_y0 + (size_t)b * n0);
        for (int s = 0; s < D; ++s) {
            double *dst = h_yc + ((size_t)b * D + s) * cc;
            std::copy(yb + n0, yb + n, dst);
            for (int a = 0; a < d; ++a) dst[tail + a] = y_add[(size_t)s * d + a];
        }
    }
    st.cw = (size_t)cc + 1;
    st.per_call(&st.d_in, h_in.size(), h_in.data());
    return NGP_OK;
}

// the context's cap, refreshed when a call of `whole` bytes would not fit the remembered one
static size_t long_cap(ngp_ctx *c, size_t whole) {
    if (whole > c->mem_cap) c->refresh_mem_cap();
    return c->mem_cap;
}

// the slots of a chunk's launches an entry point may fill itself (LongRun::launch)
enum { LONG_OWN_FILL, LONG_OWN_SMALL, LONG_OWN_AFTER_SOLVE, LONG_OWN_PRODUCTS, LONG_OWN_FINISH };
static bool long_plain(int) { return false; }

// A long query on the device: the call's scope, the chunk size, the takes and uploads (open), the
// chunks with their pointers (next), a chunk's launches (launch) and its pivot reports (info_down).
struct LongRun {
    ngp_factor *f;
    LongStage &st;
    DevCall call;
    const DevSpec sp;
    hipStream_t s;
    size_t Pc = 0;
    LongRun(ngp_factor *f_, LongStage &st_)
        : f(f_), st(st_), call(f_->ctx), sp(dev_spec(f_->spec)), s(f_->ctx->stream) {}
    // reserved: bytes beside the declared blocks.  A call whose single item does not fit is refused.
    ngp_status open(size_t reserved = 0) {
        if (call.status()) return call.status();
        const size_t P = (size_t)f->P, fixed = st.bytes(false) + reserved, item = st.bytes(true);
        const size_t cap = long_cap(f->ctx, fixed + P * item);
        if (fixed + item > cap) return NGP_ERR_TOO_LARGE;
        Pc = std::min<size_t>(std::min<size_t>(P, MAX_CHUNK_ITEMS), std::max<size_t>(1, (cap - fixed) / item));
        for (const LongBlock &b : st.blocks)
            if (b.p) call.take(reinterpret_cast<unsigned char **>(b.p), (b.per_item ? Pc : 1) * b.bytes + b.spare);
        for (const LongBlock &b : st.blocks)
            if (b.host) call.up(*b.p, b.host, b.bytes);
        return NGP_OK;
    }
    // the items of the chunk at b0 (0: no more, or the call has failed), its inputs and its part of
    // the resident factor bound
    size_t next(size_t b0) {
        if (b0 >= (size_t)f->P || call.status()) return 0;
        const size_t bc = std::min(Pc, (size_t)f->P - b0);
        LongGeom &g = st.g;
        LongPtrs &p = st.p;
        unsigned char *d_in = st.d_in;
        g.B = (int32_t)bc;
        p.progs = reinterpret_cast<const DevProgram *>(d_in) + b0;
        p.L = f->L ? f->L + b0 * (size_t)f->item_stride : nullptr;
        p.dinv = f->dinv ? f->dinv + b0 * (size_t)(NB * NB) : nullptr;
        p.finfo = g.n0 > 0 ? f->info + b0 : nullptr;   // without a main block create leaves it unwritten
        p.t0 = reinterpret_cast<const double *>(d_in + st.o_t0);
        p.tp = reinterpret_cast<const double *>(d_in + st.o_tp);
        p.y0 = reinterpret_cast<const double *>(d_in + st.o_y0) + (g.y_shared ? 0 : b0 * (size_t)g.n0);
        p.yc = reinterpret_cast<const double *>(d_in + st.o_yc) + (g.y_shared ? 0 : b0 * (size_t)g.D * g.c);
        return bc;
    }
    double small_bytes() const {   // what the plain query's small blocks write
        return 8.0 * st.g.B * ((double)st.g.q1 * (double)st.cw + (st.g.want_sigma ? (double)st.g.m * st.g.m : 0.0));
    }
    // The bound chunk's launches: panel, small blocks, solve, [a step behind the solve, where `after`
    // has a class], products, conditioning block and what is read off it.  own(slot): the entry point
    // launches that slot itself and says so; the plain query's kernels otherwise.
    template <class Own> void launch(Own own, double small_b, Cost after = Cost{-1, 0.0, 0.0}) {
        const LongGeom &g = st.g;
        const LongPtrs &p = st.p;
        EventTimer &tm = call.tm;
        const double dB = (double)g.B, dq = (double)g.q1, dn = (double)g.n0;
        call.timed(tm, 4, 0.0, 8.0 * dB * g.qpad * dn, [&] { if (!own(LONG_OWN_FILL)) launch_long(LONG_FILL, g, p, sp, s); });
        call.timed(tm, 4, 0.0, small_b, [&] { if (!own(LONG_OWN_SMALL)) launch_long(LONG_SMALL, g, p, sp, s); });
        // n0^2 q flops per item; L once per workgroup tile, the panel once in and once out, and —
        // left-looking — block column j of the solved panel read back by every later step
        const double wg_tiles = (double)((g.qpad + LONG_WG_TILE - 1) / LONG_WG_TILE);
        call.timed(tm, 6, dB * dn * dn * dq,
                   8.0 * dB * (wg_tiles * dn * dn / 2 + 2.0 * g.qpad * dn + g.qpad * dn * (g.nb0 - 1) / 2.0),
                   [&] { launch_long(LONG_SOLVE, g, p, sp, s); });
        if (after.cls >= 0) call.timed(tm, after, [&] { own(LONG_OWN_AFTER_SOLVE); });
        call.timed(tm, 2, 0.0, 0.0, [&] { if (!own(LONG_OWN_PRODUCTS)) launch_long(LONG_GRAM, g, p, sp, s); });
        call.timed(tm, 3, 0.0, 0.0, [&] {
            launch_long(LONG_COND, g, p, sp, s);
            if (own(LONG_OWN_FINISH)) return;
            launch_long(LONG_APPLY, g, p, sp, s);
            launch_long(LONG_SIGMA, g, p, sp, s);
        });
    }
    void info_down(int32_t *info, size_t b0) { if (info) call.down(info + b0, st.p.info, 4 * (size_t)st.g.B); }
};

extern "C" ngp_status ngp_factor_predict_long(ngp_factor *f, int32_t d, const double *t_add,
                                              int32_t D, const double *y_add, int32_t m,
                                              const double *t_new, int32_t noise_on_new, double *mu,
                                              double *var, double *sigma, int32_t *info) {
    if (!mu || !var) return NGP_ERR_ARG;
    if (ngp_status e = long_check(f, d, t_add, D, y_add, m, t_new)) return e;
    LongStage st;
    if (ngp_status e = long_stage(f, d, t_add, D, y_add, m, t_new, noise_on_new, 0, sigma ? m : 0, sigma, st)) return e;
    LongPtrs &p = st.p;
    const size_t um = (size_t)m, n_mu = (size_t)st.g.D * um, mm = sigma ? um * um : 0;
    st.work_blocks().per_item(&p.mu, n_mu).per_item(&p.var, um).per_item(&p.info, 1);
    if (sigma) st.per_item(&p.sigma, mm);
    LongRun run(f, st);
    if (ngp_status e = run.open()) return e;
    for (size_t b0 = 0, bc; (bc = run.next(b0)); b0 += bc) {
        run.launch(long_plain, run.small_bytes());
        run.call.down(mu + b0 * n_mu, p.mu, 8 * bc * n_mu).down(var + b0 * um, p.var, 8 * bc * um);
        if (sigma) run.call.down(sigma + b0 * mm, p.sigma, 8 * bc * mm);
        run.info_down(info, b0);
    }
    return run.call.sync();
}

// ---- paths of a long horizon (DESIGN.md sections 4.27, 4.30) --------------------------------
// sigma of the long query stays on the device, [mpad x mpad] per particle with a unit diagonal in
// the padding: factorised in place 64 columns at a time, then X = mu + L Z for the paths that
// picked the particle, their normals staged once per path.  Particles go through in chunks sized
// to the memory, and a chunk's paths in slices of the rows the staged normals have room for.
//
// The two forms — ngp_factor_sample_long (S mixtures over the same P items) and
// ngp_factor_sample_long_indep (S mixtures of P' items of their own) — differ in their checks, in
// the blocks of the pick and in two launches, the pick and the normals; everything behind the picks
// is long_sample_run.
struct LongSampleDev {     // the sampler's device blocks beside the long query's
    double *w = nullptr, *out = nullptr, *Z = nullptr, *dinv = nullptr, *logdet = nullptr;
    int32_t *comp = nullptr, *item = nullptr, *order = nullptr, *cinfo = nullptr;
    uint32_t *cnt = nullptr, *off = nullptr;
    uint64_t *seeds = nullptr;
};

static LongSampleGeom long_sample_geom(size_t P, int S, int draws, int m, int mu_rows, int mu_own) {
    LongSampleGeom sg{};
    sg.P = (int32_t)P, sg.S = S, sg.draws = draws, sg.m = m;
    sg.mpad = (m + NB - 1) / NB * NB, sg.nb = sg.mpad / NB;
    sg.mu_rows = mu_rows, sg.mu_own = mu_own;
    sg.N = (int64_t)S * draws, sg.stride = (int64_t)sg.mpad * sg.mpad;
    return sg;
}

// A staged long query (d_in first) with the sampler's blocks declared in `dv`: the room of the
// staged normals, the takes, the picks with the count round trip, the offsets and the grouping, the
// runs of active items, the chunk loop with the slices of Z, the downloads.
//   key        the block the paths are counted and grouped by: the item every path picked
//   pick_cost  of the launch `pick(stream)` makes, the count behind it included
//   normals    (first sorted position, rows, stream): Z of that slice
//   weighted   (item): whether its own mixture gives it weight
template <class Pick, class Normals, class Weighted>
static ngp_status long_sample_run(ngp_factor *f, LongStage &st, const LongSampleGeom &sg, LongSampleDev &dv,
                                  int32_t *LongSampleDev::*key, Cost pick_cost, Pick pick, Normals normals,
                                  Weighted weighted, double *out, int32_t *comp, double *mu, double *var,
                                  int32_t *info, int32_t *chol_info) {
    const LongPtrs &p = st.p;
    const int m = sg.m, mpad = sg.mpad;
    const size_t P = (size_t)f->P, N = (size_t)sg.N, um = (size_t)m, n_mu = (size_t)sg.mu_rows * um;
    LongRun run(f, st);
    DevCall &call = run.call;
    if (call.status()) return call.status();
    // the staged normals: a quarter of the room, at least Z_MIN_ROWS paths, never the last item's share
    const size_t row_bytes = 8 * (size_t)mpad, fixed = st.bytes(false), item_bytes = st.bytes(true);
    constexpr size_t Z_MIN_ROWS = LS_WG_PATHS, Z_MAX_ROWS = (size_t)1 << 22;   // the latter bounds gridDim.y
    const size_t z_least = row_bytes * (std::min(N, Z_MIN_ROWS) + NB);
    const size_t cap = long_cap(f->ctx, fixed + P * item_bytes + row_bytes * (N + NB));
    if (fixed + item_bytes + z_least > cap) return NGP_ERR_TOO_LARGE;
    const size_t room = cap - fixed;
    const size_t z_bytes = std::min(room - item_bytes, std::max(z_least, room / 4));
    const size_t zcap = std::min(std::min(N, Z_MAX_ROWS), z_bytes / row_bytes - NB);
    if (ngp_status e = run.open(row_bytes * (zcap + NB))) return e;
    call.take(&dv.Z, (size_t)mpad * (zcap + NB));
    hipStream_t s = run.s;
    EventTimer &tm = call.tm;
    // the picks and how many paths each item got: one round trip, the offsets are the host's
    std::vector<uint32_t> cnt(P, 0u), off(P + 1, 0u);
    std::vector<int32_t> hinfo(P, 0), hcinfo(P, 0);
    call.timed(tm, pick_cost, [&] {
        pick(s);
        launch_ls_count(sg, dv.*key, dv.cnt, s);
    });
    call.down(cnt.data(), dv.cnt, 4 * P);
    if (comp) call.down(comp, dv.comp, 4 * N);
    if (call.wait()) return call.sync();
    for (size_t k = 0; k < P; ++k) off[k + 1] = off[k] + (uint32_t)std::min<size_t>(cnt[k], N - off[k]);
    call.up(dv.off, off.data(), 4 * (P + 1));
    call.timed(tm, 4, 0.0, 4.0 * (double)N * (double)P + 4.0 * (double)N,
               [&] { launch_ls_group(sg, dv.*key, dv.off, dv.order, s); });
    // an item is factorised when a mixture gives it weight (or, rows that do not sum to 1, the
    // fallback of the pick fell on it)
    std::vector<char> active(P, 0);
    for (size_t k = 0; k < P; ++k) active[k] = off[k + 1] > off[k] || weighted(k);
    for (size_t b0 = 0, bc; (bc = run.next(b0)); b0 += bc) {
        run.launch(long_plain, run.small_bytes());
        if (mu) call.down(mu + b0 * n_mu, p.mu, 8 * bc * n_mu);
        if (var) call.down(var + b0 * um, p.var, 8 * bc * um);
        run.info_down(hinfo.data(), b0);
        // the chunk's sigma padded and factorised, then its paths drawn
        call.zero(dv.cinfo, 4 * bc).zero(dv.logdet, 8 * bc);
        call.timed(tm, 4, 0.0, 8.0 * (double)bc * (double)(mpad - m) * (double)(m + mpad),
                   [&] { launch_ls_pad(sg, p.sigma, (int)bc, s); });
        LongSamplePtrs q{};
        q.info = p.info, q.mu = p.mu, q.order = dv.order, q.Z = dv.Z, q.out = dv.out;
        // the factorisation, one launch sequence per run of active items
        for (size_t r0 = 0; r0 < bc;) {
            if (!active[b0 + r0]) { ++r0; continue; }
            size_t r1 = r0;
            while (r1 < bc && active[b0 + r1]) ++r1;
            const int B = (int)(r1 - r0);
            q.sigma = p.sigma + r0 * (size_t)sg.stride;
            q.dinv = dv.dinv + r0 * (size_t)(NB * NB);
            q.logdet = dv.logdet + r0;
            q.cinfo = dv.cinfo + r0;
            for (int j = 0; j < sg.nb; ++j) {
                call.timed(tm, cost_diag(B, j, 0), [&] { launch_ls_diag(sg, q, B, j, s); });
                if (j + 1 < sg.nb) call.timed(tm, cost_ls_panel(sg, B, j), [&] { launch_ls_panel(sg, q, B, j, s); });
            }
            r0 = r1;
        }
        q.sigma = p.sigma, q.dinv = dv.dinv, q.logdet = dv.logdet, q.cinfo = dv.cinfo;
        q.off = dv.off + b0;
        // the chunk's paths, a slice of sorted positions at a time
        for (size_t z0 = off[b0]; z0 < off[b0 + bc] && !call.status(); z0 += zcap) {
            const size_t zr = std::min(zcap, (size_t)off[b0 + bc] - z0);
            size_t most = 0, waves = 0, wgs = 0;
            for (size_t k = b0; k < b0 + bc; ++k) {
                const size_t lo = std::max<size_t>(off[k], z0), hi = std::min<size_t>(off[k + 1], z0 + zr);
                const size_t have = hi > lo ? hi - lo : 0;
                most = std::max(most, have);
                waves += (have + NB - 1) / NB;
                wgs += (have + LS_WG_PATHS - 1) / LS_WG_PATHS;
            }
            call.timed(tm, cost_ls_normals(sg, (double)zr), [&] { normals((int64_t)z0, (int64_t)zr, s); });
            call.timed(tm, cost_ls_draw(sg, (double)zr, (double)waves, (double)wgs), [&] {
                launch_ls_draw(sg, q, (int)bc, (int64_t)z0, (int64_t)zr, (int)((most + LS_WG_PATHS - 1) / LS_WG_PATHS), s);
            });
        }
        call.down(hcinfo.data() + b0, dv.cinfo, 4 * bc);
    }
    call.down(out, dv.out, 8 * N * um);
    const ngp_status e = call.sync();
    if (e) return e;
    for (size_t k = 0; k < P; ++k) {
        if (info) info[k] = hinfo[k];
        // a failed long query leaves NaN in sigma: its factorisation reports nothing of its own
        if (chol_info) chol_info[k] = hinfo[k] > 0 ? 0 : hcinfo[k];
    }
    return NGP_OK;
}

extern "C" ngp_status ngp_factor_sample_long(ngp_factor *f, int32_t d, const double *t_add, int32_t D,
                                             const double *y_add, int32_t m, const double *t_new,
                                             int32_t noise_on_new, const double *w, int32_t draws,
                                             uint64_t seed, double *out, int32_t *comp, double *mu,
                                             double *var, int32_t *info, int32_t *chol_info) {
    if (!w || !out || draws < 1) return NGP_ERR_ARG;
    if (ngp_status e = long_check(f, d, t_add, D, y_add, m, t_new)) return e;
    const int mpad = (m + NB - 1) / NB * NB;
    LongStage st;
    if (ngp_status e = long_stage(f, d, t_add, D, y_add, m, t_new, noise_on_new, 0, mpad, true, st)) return e;
    const int S = st.g.D;                          // 1 without appended points
    if ((int64_t)S * draws > INT32_MAX) return NGP_ERR_TOO_LARGE;
    const size_t P = (size_t)f->P, N = (size_t)S * draws, um = (size_t)m, n_mu = (size_t)S * um;
    const LongSampleGeom sg = long_sample_geom(P, S, draws, m, S, 1);
    // weights, picks, grouping, every path (and the four bytes by which the chunk's size has always
    // overcounted them); per item also sigma, block inverse, an unread log determinant, pivot report
    LongSampleDev dv;
    st.work_blocks().per_item(&st.p.mu, n_mu).per_item(&st.p.var, um).per_item(&st.p.info, 1);
    st.per_item(&st.p.sigma, (size_t)sg.stride).per_call(&dv.w, (size_t)S * P, w).per_call(&dv.comp, N);
    st.per_call(&dv.order, N).per_call(&dv.cnt, P).per_call((uint32_t **)nullptr, 1).per_call(&dv.off, P + 1);
    st.per_call(&dv.out, N * um).per_item(&dv.dinv, (size_t)(NB * NB)).per_item(&dv.logdet, 1).per_item(&dv.cinfo, 1);
    return long_sample_run(
        f, st, sg, dv, &LongSampleDev::comp, Cost{4, 0.0, 8.0 * (double)N + 4.0 * (double)N * (double)P},
        [&](hipStream_t s) { launch_ls_pick(sg, dv.w, seed, dv.comp, s); },
        [&](int64_t z0, int64_t zr, hipStream_t s) { launch_ls_normals(sg, seed, dv.order, z0, zr, dv.Z, s); },
        [&](size_t k) {
            for (int sc = 0; sc < S; ++sc)
                if (w[(size_t)sc * P + k] > 0.0) return true;
            return false;
        },
        out, comp, mu, var, info, chol_info);
}

// The independent form: the factor's items are S mixtures of P' = P / S
// components, mixture-major, without appended points; mixture s is keyed by seeds[s].
extern "C" ngp_status ngp_factor_sample_long_indep(ngp_factor *f, int32_t S, int32_t m, const double *t_new,
                                                   int32_t noise_on_new, const double *w, int32_t draws,
                                                   const uint64_t *seeds, double *out, int32_t *comp,
                                                   double *mu, double *var, int32_t *info,
                                                   int32_t *chol_info) {
    if (!w || !seeds || !out || draws < 1 || S < 1) return NGP_ERR_ARG;
    if (ngp_status e = long_check(f, 0, nullptr, 1, nullptr, m, t_new)) return e;
    if (f->P % S != 0) return NGP_ERR_ARG;
    if ((int64_t)S * draws > INT32_MAX) return NGP_ERR_TOO_LARGE;
    const int mpad = (m + NB - 1) / NB * NB;
    LongStage st;
    if (ngp_status e = long_stage(f, 0, nullptr, 1, nullptr, m, t_new, noise_on_new, 0, mpad, true, st)) return e;
    const size_t P = (size_t)f->P, N = (size_t)S * draws, um = (size_t)m;
    const int Pm = (int)(P / (size_t)S);
    const LongSampleGeom sg = long_sample_geom(P, S, draws, m, 1, 0);
    // as the shared form, with one weight per item, the mixtures' seeds and the picked item beside
    // the component the caller gets
    LongSampleDev dv;
    st.work_blocks().per_item(&st.p.mu, um).per_item(&st.p.var, um).per_item(&st.p.info, 1);
    st.per_item(&st.p.sigma, (size_t)sg.stride).per_call(&dv.w, P, w).per_call(&dv.seeds, (size_t)S, seeds);
    st.per_call(&dv.comp, N).per_call(&dv.item, N).per_call(&dv.order, N).per_call(&dv.cnt, P).per_call(&dv.off, P + 1);
    st.per_call(&dv.out, N * um).per_item(&dv.dinv, (size_t)(NB * NB)).per_item(&dv.logdet, 1).per_item(&dv.cinfo, 1);
    return long_sample_run(
        f, st, sg, dv, &LongSampleDev::item, cost_lsi_pick(sg, Pm),
        [&](hipStream_t s) { launch_lsi_pick(sg, Pm, dv.w, dv.seeds, dv.item, dv.comp, s); },
        [&](int64_t z0, int64_t zr, hipStream_t s) { launch_lsi_normals(sg, dv.seeds, dv.order, z0, zr, dv.Z, s); },
        [&](size_t k) { return w[k] > 0.0; }, out, comp, mu, var, info, chol_info);
}

// ---- additive decomposition ---------------------------------------
// The components of a tree: its maximal non-Plus subtrees reached from the root through Plus nodes
// only, left to right.  In postfix order a subtree is a contiguous slice of ops and of params.
extern "C" ngp_status ngp_kernel_components(const ngp_kernel *k, int32_t *count, int32_t *op_first,
                                            int32_t *op_len, int32_t *par_first, int32_t *par_len) {
    if (!k || !count) return NGP_ERR_ARG;
    ngp_status st = check_program(k);
    if (st) return st;
    struct Sub { int left, right, op0, par0, par1; };   // children, first op, params [par0, par1)
    std::vector<Sub> nodes;
    std::vector<int> stack;
    int pi = 0;
    for (int i = 0; i < k->n_ops; ++i) {
        const int op = k->ops[i];
        Sub nd{-1, -1, i, pi, 0};
        if (op >= NGP_OP_PLUS) {
            nd.right = stack.back(); stack.pop_back();
            nd.left = stack.back(); stack.pop_back();
            nd.op0 = nodes[(size_t)nd.left].op0;
            nd.par0 = nodes[(size_t)nd.left].par0;
        }
        pi += k_nparams[op];
        nd.par1 = pi;
        nodes.push_back(nd);
        stack.push_back(i);
    }
    int nc = 0;
    std::vector<int> todo{stack.back()};
    while (!todo.empty()) {
        const int i = todo.back();
        todo.pop_back();
        const Sub &nd = nodes[(size_t)i];
        if (k->ops[i] == NGP_OP_PLUS) {
            todo.push_back(nd.right);   // the left summand comes out first
            todo.push_back(nd.left);
            continue;
        }
        if (op_first) op_first[nc] = nd.op0;
        if (op_len) op_len[nc] = i - nd.op0 + 1;
        if (par_first) par_first[nc] = nd.par0;
        if (par_len) par_len[nc] = nd.par1 - nd.par0;
        ++nc;
    }
    *count = nc;
    return NGP_OK;
}

// ---- sum-of-products terms of a tree ------------------------------
// terms(leaf) = {leaf}; terms(Plus(l, r)) = terms(l) then terms(r); with NGP_SPLIT_CHANGEPOINT
// terms(CP(l, r)) = {CP(x, Constant(0))} then {CP(Constant(0), y)}; with NGP_SPLIT_TIMES
// terms(Times(l, r)) = {Times(x, y)}, x outer.  A node that is not split is one term, verbatim.
// The device blend of a ChangePoint is g1 a g2 + (1 - g1) b (1 - g2) (cp_blend, ngp_tree_kernels.h)
// under both cp_form values — the form only picks the sigmoid — so it is linear in its operand
// values and the terms sum to the tree; an operand that is Constant(0) contributes an exact zero.
extern "C" ngp_status ngp_kernel_terms(const ngp_kernel *k, int32_t split, int32_t max_terms,
                                       int32_t *count, int32_t *op_first, int32_t *op_len,
                                       int32_t *par_first, int32_t *par_len, int32_t *ops_out,
                                       int32_t ops_cap, double *params_out, int32_t par_cap) {
    if (!k || !count || split < 0 || split > (NGP_SPLIT_CHANGEPOINT | NGP_SPLIT_TIMES) ||
        max_terms < 0 || ops_cap < 0 || par_cap < 0)
        return NGP_ERR_ARG;
    *count = 0;
    // the structure alone: a tree longer than NGP_MAX_OPS may still have terms that fit
    if (!k->ops || k->n_ops <= 0) return NGP_ERR_PROGRAM;
    constexpr int MAX_IN = 64 * NGP_MAX_OPS;      // bounds the recursion below
    if (k->n_ops > MAX_IN) return NGP_ERR_TOO_LARGE;
    // cnt: the number of terms below the node; lo / lp: the longest term's ops / parameters;
    // to / tp: the ops / parameters of all its terms together (all saturating)
    struct Sub { int op, left, right, op0, par0, own; int64_t cnt, lo, lp, to, tp; };
    constexpr int64_t SAT = (int64_t)1 << 40;
    auto sat = [&](int64_t v) { return std::min(SAT, v); };
    auto mul = [&](int64_t a, int64_t b) { return a >= SAT || b >= SAT || a * b >= SAT ? SAT : a * b; };
    std::vector<Sub> nodes;
    std::vector<int> stack;
    int pi = 0;
    auto splits = [&](int op) {
        return op == NGP_OP_PLUS || (op == NGP_OP_CHANGEPOINT && (split & NGP_SPLIT_CHANGEPOINT)) ||
               (op == NGP_OP_TIMES && (split & NGP_SPLIT_TIMES));
    };
    for (int i = 0; i < k->n_ops; ++i) {
        const int op = k->ops[i];
        if (op < 1 || op > 8) return NGP_ERR_PROGRAM;
        Sub nd{op, -1, -1, i, pi, pi, 1, 0, 0, 0, 0};
        if (op >= NGP_OP_PLUS) {
            if (stack.size() < 2) return NGP_ERR_PROGRAM;
            nd.right = stack.back(); stack.pop_back();
            nd.left = stack.back(); stack.pop_back();
            nd.op0 = nodes[(size_t)nd.left].op0;
            nd.par0 = nodes[(size_t)nd.left].par0;
            // the count of a node reached through split nodes only (its operands then are, too)
            const Sub &l = nodes[(size_t)nd.left], &r = nodes[(size_t)nd.right];
            const int64_t a = l.cnt, b = r.cnt;
            if (op == NGP_OP_PLUS) {
                nd.cnt = sat(a + b);
                nd.lo = std::max(l.lo, r.lo); nd.lp = std::max(l.lp, r.lp);
                nd.to = sat(l.to + r.to); nd.tp = sat(l.tp + r.tp);
            } else if (op == NGP_OP_CHANGEPOINT && splits(op)) {     // + Constant(0) and the node
                nd.cnt = sat(a + b);
                nd.lo = std::max(l.lo, r.lo) + 2; nd.lp = std::max(l.lp, r.lp) + 3;
                nd.to = sat(l.to + r.to + mul(2, nd.cnt)); nd.tp = sat(l.tp + r.tp + mul(3, nd.cnt));
            } else if (splits(op)) {                                 // Times: x y and the node
                nd.cnt = mul(a, b);
                nd.lo = l.lo + r.lo + 1; nd.lp = l.lp + r.lp;
                nd.to = sat(mul(l.to, b) + mul(r.to, a) + nd.cnt);
                nd.tp = sat(mul(l.tp, b) + mul(r.tp, a));
            }
        }
        pi += k_nparams[op];
        if (op < NGP_OP_PLUS || !splits(op)) {                       // one term, verbatim
            nd.lo = nd.to = i - nd.op0 + 1;
            nd.lp = nd.tp = pi - nd.par0;
        }
        nodes.push_back(nd);
        stack.push_back(i);
    }
    if (stack.size() != 1 || pi != k->n_params || (pi > 0 && !k->params)) return NGP_ERR_PROGRAM;
    const int root = stack.back();
    const int64_t total = nodes[(size_t)root].cnt;
    *count = (int32_t)std::min<int64_t>(total, INT32_MAX);
    if (total > max_terms) return NGP_ERR_TOO_LARGE;
    const bool want = op_first || op_len || par_first || par_len || ops_out || params_out;
    const Sub &rt = nodes[(size_t)root];
    // a term that is no valid program, or more than the buffers hold: known before a term is
    // built, so what is built below is bounded by the caller's own buffers
    if (rt.lo > NGP_MAX_OPS || rt.lp > NGP_MAX_PARAMS) return NGP_ERR_TOO_LARGE;
    if (!want) return NGP_OK;                     // the count alone: no term is built
    if (!ops_out || !params_out || rt.to > ops_cap || rt.tp > par_cap) return NGP_ERR_TOO_LARGE;
    struct Term { std::vector<int32_t> ops; std::vector<double> par; };
    auto terms = [&](auto &&self, int i) -> std::vector<Term> {
        const Sub &nd = nodes[(size_t)i];
        std::vector<Term> out;
        const double *th = k->params + nd.own;    // the node's own parameters
        if (nd.op < NGP_OP_PLUS || !splits(nd.op)) {
            Term t;
            t.ops.assign(k->ops + nd.op0, k->ops + i + 1);
            t.par.assign(k->params + nd.par0, k->params + nd.own + k_nparams[nd.op]);
            out.push_back(std::move(t));
            return out;
        }
        std::vector<Term> L = self(self, nd.left), R = self(self, nd.right);
        if (nd.op == NGP_OP_PLUS) {
            out = std::move(L);
            for (Term &t : R) out.push_back(std::move(t));
        } else if (nd.op == NGP_OP_CHANGEPOINT) {
            for (Term &x : L) {                   // the window before the change point
                x.ops.push_back(NGP_OP_CONSTANT); x.ops.push_back(NGP_OP_CHANGEPOINT);
                x.par.push_back(0.0); x.par.push_back(th[0]); x.par.push_back(th[1]);
                out.push_back(std::move(x));
            }
            for (Term &y : R) {                   // the window after it
                Term t;
                t.ops.push_back(NGP_OP_CONSTANT);
                t.ops.insert(t.ops.end(), y.ops.begin(), y.ops.end());
                t.ops.push_back(NGP_OP_CHANGEPOINT);
                t.par.push_back(0.0);
                t.par.insert(t.par.end(), y.par.begin(), y.par.end());
                t.par.push_back(th[0]); t.par.push_back(th[1]);
                out.push_back(std::move(t));
            }
        } else {
            for (const Term &x : L)
                for (const Term &y : R) {
                    Term t = x;
                    t.ops.insert(t.ops.end(), y.ops.begin(), y.ops.end());
                    t.ops.push_back(NGP_OP_TIMES);
                    t.par.insert(t.par.end(), y.par.begin(), y.par.end());
                    out.push_back(std::move(t));
                }
        }
        return out;
    };
    const std::vector<Term> all = terms(terms, root);
    bool fits = true;
    int64_t no = 0, np = 0;
    for (size_t c = 0; c < all.size(); ++c) {
        const Term &t = all[c];
        const ngp_kernel tk{(int32_t)t.ops.size(), (int32_t)t.par.size(), t.ops.data(), t.par.data(), k->noise};
        if (ngp_kernel_check(&tk) != NGP_OK) fits = false;
        if (!ops_out || !params_out || no + (int64_t)t.ops.size() > ops_cap ||
            np + (int64_t)t.par.size() > par_cap)
            fits = false;
        if (fits) {
            std::copy(t.ops.begin(), t.ops.end(), ops_out + no);
            std::copy(t.par.begin(), t.par.end(), params_out + np);
            if (op_first) op_first[c] = (int32_t)no;
            if (op_len) op_len[c] = (int32_t)t.ops.size();
            if (par_first) par_first[c] = (int32_t)np;
            if (par_len) par_len[c] = (int32_t)t.par.size();
        }
        no += (int64_t)t.ops.size();
        np += (int64_t)t.par.size();
    }
    return fits ? NGP_OK : NGP_ERR_TOO_LARGE;
}

namespace {

// ngp_factor_components (d = 0, D = 1, no logml) and ngp_factor_components_nowcast: one body
ngp_status components_query(ngp_factor *f, int32_t d, const double *t_add, int32_t D,
                            const double *y_add, const int32_t *comp_count, const ngp_kernel *comps,
                            int32_t m, const double *t_new, double *logml_full, double *mu,
                            double *sigma, double *var, int32_t *info) {
    const int P = f->P;
    std::vector<int32_t> first((size_t)P + 1, 0);
    std::vector<int64_t> sig_off((size_t)P, 0);
    int cmax = 0;
    int64_t sig_total = 0;
    for (int b = 0; b < P; ++b) {
        const int cb = comp_count[b];
        if (cb < 1) return NGP_ERR_ARG;
        if ((int64_t)(f->n % NB) + d + 1 + (int64_t)cb * m > NGP_MAX_AUX) return NGP_ERR_TOO_LARGE;
        first[(size_t)b + 1] = first[(size_t)b] + cb;
        sig_off[(size_t)b] = sig_total;
        sig_total += (int64_t)cb * m * cb * m;
        cmax = std::max(cmax, cb);
    }
    const size_t ncomp = (size_t)first[(size_t)P];
    std::vector<DevProgram> hp(ncomp);
    for (size_t i = 0; i < ncomp; ++i) {
        ngp_status st = compile_program(&comps[i], &hp[i], nullptr);
        if (st) return st;
    }
    // the query's geometry: cmax groups of the m dates (an item with fewer components leaves its
    // last groups zero); no noise on the new points
    std::vector<double> t_rep((size_t)cmax * m);
    for (int c = 0; c < cmax; ++c) std::copy(t_new, t_new + m, t_rep.begin() + (size_t)c * m);
    ngp_ctx *c = f->ctx;
    static const double dummy = 0.0;
    if (d == 0) { t_add = &dummy; y_add = &dummy; }
    ngp_job *job = nullptr;
    ngp_status st = stage_general(c, P, f->kernels.data(), f->n, f->t.data(), f->y.data(), f->ldy, d,
                                  t_add, D, y_add, 0, cmax * m, t_rep.data(), 0, &job);
    if (st) return st;
    const size_t n_out = ncomp * (size_t)m, n_mu = n_out * (size_t)D;
    // V and the prior's diagonal, then room for L_A and its three vectors when LDS does not hold them
    const int64_t work_stride = (int64_t)cmax * m * (job->g.da + 1) + comp_epi_small(job->g.da);
    const size_t o_first = sizeof(DevProgram) * ncomp, o_sig = (o_first + 4 * first.size() + 7) & ~(size_t)7,
                 in_bytes = o_sig + 8 * sig_off.size();
    std::vector<unsigned char> h_in(in_bytes);
    std::memcpy(h_in.data(), hp.data(), o_first);
    std::memcpy(h_in.data() + o_first, first.data(), 4 * first.size());
    std::memcpy(h_in.data() + o_sig, sig_off.data(), 8 * sig_off.size());
    {
        // the call keeps its blocks while the job runs and is fetched under the lock those take
        // themselves (same thread, same device)
        DevCall call(c);
        unsigned char *d_in = nullptr;
        double *d_mu = nullptr, *d_sigma = nullptr, *d_var = nullptr, *d_work = nullptr;
        call.take(&d_in, in_bytes).take(&d_mu, n_mu);
        if (sigma) call.take(&d_sigma, (size_t)sig_total);
        if (var) call.take(&d_var, n_out);
        call.take(&d_work, (size_t)P * (size_t)work_stride).up(d_in, h_in.data(), in_bytes);
        call.unlocked([&] {
            CompPtrs cp{};
            cp.progs = (const DevProgram *)d_in;
            cp.first = (const int32_t *)(d_in + o_first);
            cp.sig_off = (const int64_t *)(d_in + o_sig);
            cp.mu = d_mu;
            cp.sigma = d_sigma;
            cp.var = d_var;
            cp.m = m;
            cp.cmax = cmax;
            const ngp_status ran = factor_run(f, job, /*create=*/false, &cp, d_work, work_stride);
            return ran ? ran : ngp_job_fetch(job, nullptr, logml_full, nullptr, nullptr, info);
        });
        call.down(mu, d_mu, 8 * n_mu);
        if (sigma) call.down(sigma, d_sigma, 8 * (size_t)sig_total);
        if (var) call.down(var, d_var, 8 * n_out);
        st = call.sync();   // also when the job failed: the staging copy reads h_in
    }
    ngp_job_destroy(job);
    return st;
}

}  // namespace

extern "C" ngp_status ngp_factor_components(ngp_factor *f, const int32_t *comp_count,
                                            const ngp_kernel *comps, int32_t m, const double *t_new,
                                            double *mu, double *sigma, double *var, int32_t *info) {
    if (!f || !comp_count || !comps || !t_new || !mu || m < 1) return NGP_ERR_ARG;
    return components_query(f, 0, nullptr, 1, nullptr, comp_count, comps, m, t_new, nullptr, mu, sigma,
                            var, info);
}

extern "C" ngp_status ngp_factor_components_nowcast(ngp_factor *f, int32_t d, const double *t_add,
                                                    int32_t D, const double *y_add,
                                                    const int32_t *comp_count, const ngp_kernel *comps,
                                                    int32_t m, const double *t_new, double *logml_full,
                                                    double *mu, double *sigma, double *var,
                                                    int32_t *info) {
    if (!f || !comp_count || !comps || !t_new || !mu || m < 1) return NGP_ERR_ARG;
    if (d < 0 || D < 1 || (d > 0 && (!t_add || !y_add))) return NGP_ERR_ARG;
    return components_query(f, d, t_add, D, y_add, comp_count, comps, m, t_new, logml_full, mu, sigma,
                            var, info);
}

// ---- the decomposition over a long horizon ---------------------------
// The long query (LongStage, LongRun) with its own panel layout: cmax groups of date rows, each
// padded to LONG_TILE, and every panel row has a row of S (ngp_long_component_kernels.h).  Fill,
// small blocks, products and what follows the conditioning block are its own kernels.
extern "C" ngp_status ngp_factor_components_long(ngp_factor *f, int32_t d, const double *t_add,
                                                 int32_t D, const double *y_add,
                                                 const int32_t *comp_count, const ngp_kernel *comps,
                                                 int32_t m, const double *t_new, double *mu,
                                                 double *cross, double *sigma, int32_t *info) {
    if (!comp_count || !comps || !mu || !cross) return NGP_ERR_ARG;
    if (ngp_status e = long_check(f, d, t_add, D, y_add, m, t_new)) return e;
    const size_t P = (size_t)f->P;
    std::vector<int32_t> first(P + 1, 0);
    std::vector<int64_t> cr_off(P + 1, 0), sig_off(P + 1, 0);
    int64_t cmax = 0;
    for (size_t b = 0; b < P; ++b) {
        const int64_t cb = comp_count[b];
        if (cb < 1) return NGP_ERR_ARG;
        if (cb > 65534 || (sigma && cb * m > NGP_MAX_LONG_HORIZON)) return NGP_ERR_TOO_LARGE;
        if (first[b] + cb > INT32_MAX) return NGP_ERR_TOO_LARGE;
        first[b + 1] = (int32_t)(first[b] + cb);
        cr_off[b + 1] = cr_off[b] + cb * cb;
        sig_off[b + 1] = sig_off[b] + cb * m * cb * m;
        cmax = std::max(cmax, cb);
    }
    const size_t ncomp = (size_t)first[P];
    std::vector<DevProgram> hp(ncomp);
    for (size_t i = 0; i < ncomp; ++i)
        if (ngp_status e = compile_program(&comps[i], &hp[i], nullptr)) return e;
    LongStage st;
    if (ngp_status e = long_stage(f, d, t_add, D, y_add, m, t_new, 0, (int32_t)cmax, 0, sigma, st)) return e;
    const LongGeom &g = st.g;
    LongCompGeom cg{};
    cg.m = m;
    cg.mpad = (m + LONG_TILE - 1) / LONG_TILE * LONG_TILE;
    cg.cmax = (int32_t)cmax;
    cg.hpad = g.q1 - cg.cmax * cg.mpad;
    const size_t S = (size_t)g.D, um = (size_t)m, uc = (size_t)cmax;
    const size_t n_cr = uc * uc * um, n_sig = sigma ? n_cr * um : 0;
    const size_t o_first = sizeof(DevProgram) * ncomp, o_cr = (o_first + 4 * first.size() + 7) & ~(size_t)7,
                 o_sig = o_cr + 8 * cr_off.size(), cin_bytes = o_sig + 8 * sig_off.size();
    std::vector<unsigned char> h_cin(cin_bytes);
    std::memcpy(h_cin.data(), hp.data(), o_first);
    std::memcpy(h_cin.data() + o_first, first.data(), 4 * first.size());
    std::memcpy(h_cin.data() + o_cr, cr_off.data(), 8 * cr_off.size());
    std::memcpy(h_cin.data() + o_sig, sig_off.data(), 8 * sig_off.size());
    const LongPtrs &p = st.p;
    LongCompPtrs cp{};
    unsigned char *d_cin = nullptr;
    st.per_call(&d_cin, cin_bytes, h_cin.data()).work_blocks(false).per_item(&st.p.info, 1);
    st.per_item(&cp.mu, uc * S * um).per_item(&cp.cross, n_cr);
    if (sigma) st.per_item(&cp.sigma, n_sig);
    LongRun run(f, st);
    if (ngp_status e = run.open()) return e;
    const DevSpec &sp = run.sp;
    hipStream_t s = run.s;
    auto own = [&](int slot) {   // every slot but the one behind the solve, which it has not
        if (slot == LONG_OWN_FILL) launch_long_comp(LCOMP_FILL, g, p, cg, cp, sp, s);
        if (slot == LONG_OWN_SMALL) launch_long_comp(LCOMP_SMALL, g, p, cg, cp, sp, s);
        if (slot == LONG_OWN_PRODUCTS) launch_long_comp(LCOMP_GRAM, g, p, cg, cp, sp, s);
        if (slot == LONG_OWN_FINISH) {
            launch_long_comp(LCOMP_APPLY, g, p, cg, cp, sp, s);
            launch_long_comp(LCOMP_CROSS, g, p, cg, cp, sp, s);
            launch_long_comp(LCOMP_SIGMA, g, p, cg, cp, sp, s);
        }
        return true;
    };
    for (size_t b0 = 0, bc; (bc = run.next(b0)); b0 += bc) {
        const size_t b1 = b0 + bc;
        cp.progs = reinterpret_cast<const DevProgram *>(d_cin) + first[b0];
        cp.first = reinterpret_cast<const int32_t *>(d_cin + o_first) + b0;
        cp.cr_off = reinterpret_cast<const int64_t *>(d_cin + o_cr) + b0;
        cp.sig_off = reinterpret_cast<const int64_t *>(d_cin + o_sig) + b0;
        // the chunk's components, elements of cross and of sigma
        const size_t nc = (size_t)(first[b1] - first[b0]), ncr = (size_t)(cr_off[b1] - cr_off[b0]) * um,
                     nsg = sigma ? (size_t)(sig_off[b1] - sig_off[b0]) : 0;
        run.launch(own, 8.0 * ((double)bc * cg.hpad * (double)st.cw + (double)nc * um * (double)st.cw + (double)ncr + (double)nsg / 2));
        run.call.down(mu + (size_t)first[b0] * S * um, cp.mu, 8 * nc * S * um);
        run.call.down(cross + (size_t)cr_off[b0] * um, cp.cross, 8 * ncr);
        if (sigma) run.call.down(sigma + sig_off[b0], cp.sigma, 8 * nsg);
        run.info_down(info, b0);
    }
    return run.call.sync();
}

// ---- hindcasts at many forecast origins ------------------------------
// The long query without appended points, unchanged up to the conditioning block; the dates' means
// and variances are read off the solved panel at every prefix the call asks for, the main block's
// right behind the solve (ngp_long_origin_kernels.h).
extern "C" ngp_status ngp_factor_predict_origins(ngp_factor *f, int32_t R, const int32_t *cut,
                                                 int32_t m, const double *t_new,
                                                 int32_t noise_on_new, double *mu, double *var,
                                                 double *logml, int32_t *info) {
    if (!f || !cut || !t_new || !mu || !var || R < 1 || m < 1) return NGP_ERR_ARG;
    if (R > NGP_MAX_ORIGINS) return NGP_ERR_TOO_LARGE;
    for (int32_t r = 0; r < R; ++r)
        if (cut[r] < 1 || cut[r] > f->n || (r > 0 && cut[r] <= cut[r - 1])) return NGP_ERR_ARG;
    if (ngp_status e = long_check(f, 0, nullptr, 1, nullptr, m, t_new)) return e;
    LongStage st;
    if (ngp_status e = long_stage(f, 0, nullptr, 1, nullptr, m, t_new, noise_on_new, 0, 0, false, st)) return e;
    const LongGeom &g = st.g;
    const LongPtrs &p = st.p;
    LongOriginGeom og{};
    og.R = R;
    og.R0 = (int32_t)(std::upper_bound(cut, cut + R, g.n0) - cut);
    LongOriginPtrs op{};
    int32_t *d_cut = nullptr;
    const size_t uR = (size_t)R, n_out = uR * (size_t)m;
    st.per_call(&d_cut, uR, cut).work_blocks().per_item(&st.p.info, 1);
    st.per_item(&op.mu, n_out).per_item(&op.var, n_out);
    st.per_item(logml ? &op.logml : (double **)nullptr, uR);   // counted also when nobody asks for it
    LongRun run(f, st);
    if (ngp_status e = run.open()) return e;
    op.cut = d_cut;
    auto own = [&](int slot) {
        if (slot == LONG_OWN_AFTER_SOLVE) launch_long_origin(LORG_MAIN, g, p, og, op, run.sp, run.s);
        if (slot == LONG_OWN_FINISH) {
            launch_long_origin(LORG_TAIL, g, p, og, op, run.sp, run.s);
            launch_long_origin(LORG_LOGML, g, p, og, op, run.sp, run.s);
        }
        return slot == LONG_OWN_AFTER_SOLVE || slot == LONG_OWN_FINISH;
    };
    for (size_t b0 = 0, bc; (bc = run.next(b0)); b0 += bc) {
        // behind the solve: one read of the solved date rows, two stores per origin and date
        run.launch(own, run.small_bytes(),
                   Cost{3, 2.0 * (double)bc * (double)m * (double)g.n0,
                        8.0 * (double)bc * ((double)g.qpad * (double)g.n0 + 2.0 * og.R0 * (double)m)});
        run.call.down(mu + b0 * n_out, op.mu, 8 * bc * n_out).down(var + b0 * n_out, op.var, 8 * bc * n_out);
        if (logml) run.call.down(logml + b0 * uR, op.logml, 8 * bc * uR);
        run.info_down(info, b0);
    }
    return run.call.sync();
}

extern "C" void ngp_factor_destroy(ngp_factor *f) {
    if (!f) return;
    {
        std::lock_guard<std::mutex> lk(f->ctx->mu);
        f->ctx->release(f->L);
        f->ctx->release(f->dinv);
        f->ctx->release(f->logdet);
        f->ctx->release(f->info);
    }
    delete f;
}

extern "C" ngp_status ngp_cov_batch(ngp_ctx *c, int32_t B, const ngp_kernel *kernels, int32_t n1,
                                    const double *t1, int32_t n2, const double *t2,
                                    int32_t add_diag, double *out) {
    if (!c || !kernels || !t1 || !t2 || !out || B <= 0 || n1 <= 0 || n2 <= 0) return NGP_ERR_ARG;
    std::vector<DevProgram> hp((size_t)B);
    for (int i = 0; i < B; ++i) {
        ngp_status st = compile_program(&kernels[i], &hp[(size_t)i], nullptr);
        if (st) return st;
    }
    DevCall call(c);
    DevProgram *dp = nullptr;
    double *d1 = nullptr, *d2 = nullptr, *dout = nullptr;
    const size_t nout = (size_t)B * n1 * n2;
    call.take(&dp, (size_t)B).take(&d1, (size_t)n1).take(&d2, (size_t)n2).take(&dout, nout);
    hipStream_t s = c->stream;
    call.up(dp, hp.data(), sizeof(DevProgram) * (size_t)B)
        .up(d1, t1, sizeof(double) * (size_t)n1)
        .up(d2, t2, sizeof(double) * (size_t)n2)
        .timed(call.tm, 4, 0.0, 8.0 * (double)nout, [&] {
            for (int b0 = 0; b0 < B; b0 += (int)MAX_CHUNK_ITEMS)   // items are blockIdx.y
                launch_cov(dp + b0, std::min(B - b0, (int)MAX_CHUNK_ITEMS), d1, n1, d2, n2, add_diag,
                           dout + (size_t)b0 * n1 * n2, dev_spec(c->spec), s);
        })
        .down(out, dout, sizeof(double) * nout);
    return call.sync();
}

#include "ngp_host_grad.h"
#include "ngp_host_mixture.h"
#include "ngp_host_combine.h"
#include "ngp_host_comm.h"
#include "ngp_host_bench.h"

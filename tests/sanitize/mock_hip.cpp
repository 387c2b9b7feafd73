// A stand-in for the HIP runtime, for SANITIZER builds of the host layer only
// (tests/test_host_sanitizers.py): ngp_api.hip and the launchers of ngp_kernels.hip are compiled
// host-only (hipcc --cuda-host-only) with -fsanitize=thread or address,undefined and linked against
// this file instead of libamdhip64.  "Device" memory is zeroed host memory, copies are memcpy,
// streams and events are inert handles, kernel launches do nothing.  What runs for real is every
// line of host code behind the C-ABI: the context mutex, the caching allocator, job / factor
// lifetimes, the staging code, the error paths — entered from several threads at once.
// Nothing here is part of the product; libngp.so never links it.
//
// Launch trace (off by default; tests/sanitize/route_trace.cpp switches it on, single-threaded): one
// line per kernel launch — interned mangled name, grid, block, dynamic LDS bytes, stream ordinal,
// a checksum of the JobGeom / ColStep arguments and the values of the int / long arguments behind
// a leading JobGeom — and one per event record / wait, memset and asynchronous copy.  Streams and
// events are numbered in creation order; pointers are never written, so the trace is the same on
// every run.  Identical consecutive lines are written once with a repeat count.  In digest mode the
// lines are not printed but counted and hashed (FNV-1a, 64 bit), and the launches are tallied by
// kernel (with the grid of its first launch); the driver prints both per call.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

extern "C" {
typedef int hipError_t;
typedef struct ihipStream_t *hipStream_t;
typedef struct ihipEvent_t *hipEvent_t;
struct dim3_ { uint32_t x, y, z; };

static std::mutex g_mu;
static std::unordered_map<void *, size_t> g_live;      // allocation -> bytes
static std::atomic<long> g_launches{0}, g_bad_free{0}, g_oob{0}, g_sync_us{0};

// ---- trace ------------------------------------------------------------------------------------
// The registration hook runs from static constructors of the library's objects, possibly before this
// file's own: the tables are made on first use.
struct Trace {
    bool on = false, digest = false;
    uint64_t hash = 14695981039346656037ull;
    long lines = 0;
    struct Tally { int id; long n; dim3_ first; };
    std::vector<Tally> tally;            // kernels launched since the last digest, in order of appearance
    std::vector<std::string> by_id;      // interned names
    std::string summary;
    std::unordered_map<const void *, std::string> names;   // host stub -> mangled device name
    std::unordered_map<std::string, int> ids;
    std::unordered_map<const void *, int> streams, events;
    int n_streams = 0, n_events = 0;
    std::vector<int> launch_streams;     // stream ordinals that saw a launch since mock_hip_launch_streams()
    std::string last;
    long repeat = 0;
};
static Trace &tr() { static Trace t; return t; }
static void trace_flush() {
    Trace &t = tr();
    if (!t.repeat) return;
    std::string out = t.last;
    if (t.repeat > 1) out += " x" + std::to_string(t.repeat);
    out += "\n";
    t.repeat = 0;
    if (!t.digest) { std::fputs(out.c_str(), stdout); return; }
    for (unsigned char ch : out) t.hash = (t.hash ^ ch) * 1099511628211ull;
    ++t.lines;
}
static void trace_line(const char *buf) {
    Trace &t = tr();
    if (t.repeat && t.last == buf) { ++t.repeat; return; }
    trace_flush();
    t.last = buf;
    t.repeat = 1;
}
static int ordinal(const std::unordered_map<const void *, int> &m, const void *p) {
    auto it = m.find(p);
    return it == m.end() ? -1 : it->second;   // -1: the null stream / an event made for timing
}
static uint32_t fnv(uint32_t h, const void *p, size_t n) {
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char *)p)[i]) * 16777619u;
    return h;
}
// The arguments of a kernel whose first parameter is ngp::JobGeom, read off its mangled name: the
// geometry (128 bytes, no pointers: sizeof is asserted in plan_check.cpp), the four counts behind the
// pointers of a ChunkPtrs (offset asserted there too) and a ColStep (seven ints, a gap, two doubles)
// go into a checksum, int / long values are appended as they are; pointers and
// other structs are passed over.  Anything this little reader does not know ends the walk.
// "NS_<len><name>E" (a type of namespace ngp): its name, and q behind it; false: something else
static bool nested_name(const char *&q, std::string *ty) {
    if (std::strncmp(q, "NS_", 3) != 0) return false;
    char *e = nullptr;
    const long n = std::strtol(q + 3, &e, 10);
    if (n <= 0 || std::strlen(e) < (size_t)n + 1 || e[n] != 'E') return false;
    ty->assign(e, (size_t)n);
    q = e + n + 1;
    return true;
}
static void trace_args(const std::string &name, void **args, char *out, size_t cap) {
    out[0] = 0;
    const size_t at = name.find("NS_7JobGeomE");
    if (at == std::string::npos || at < 2 || name[at - 1] != (name[at - 2] == 'E' ? 'v' : 'E')) return;
    const char *q = name.c_str() + at;
    uint32_t h = 2166136261u;
    size_t len = 0;
    std::string ty;
    for (int a = 0; *q; ++a) {
        if (*q == 'P') {                                   // pointer (to const) to a builtin or a struct
            ++q;
            if (*q == 'K') ++q;
            if (*q == 'N') { if (!nested_name(q, &ty)) break; }
            else if (*q == 'S') { const char *e = std::strchr(q, '_'); if (!e) break; q = e + 1; }
            else ++q;
        } else if (*q == 'N') {
            if (!nested_name(q, &ty)) break;
            if (ty == "JobGeom") h = fnv(h, args[a], 128);
            if (ty == "ChunkPtrs") h = fnv(h, (const char *)args[a] + 168, 16);   // n_fill_chain .. fill_base
            if (ty == "ColStep") { h = fnv(h, args[a], 28); h = fnv(h, (const char *)args[a] + 32, 16); }
        } else if (*q == 'i' || *q == 'l') {
            const long v = *q == 'i' ? (long)*(const int *)args[a] : *(const long *)args[a];
            len += (size_t)std::snprintf(out + len, cap - len, " %ld", v);
            ++q;
        } else break;
    }
    std::snprintf(out + len, cap - len, " #%08x", h);
}

static bool inside(const void *p, size_t n) {
    // host pointers (stack / heap of the caller) are not tracked: only check "device" ones
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto &kv : g_live) {
        const char *b = (const char *)kv.first;
        if ((const char *)p >= b && (const char *)p < b + kv.second)
            return (const char *)p + n <= b + kv.second;
    }
    return true;
}

hipError_t hipGetDeviceCount(int *n) { *n = 1; return 0; }
hipError_t hipGetDevice(int *d) { *d = 0; return 0; }
hipError_t hipFuncSetAttribute(const void *, int, int) { return 0; }
hipError_t hipSetDevice(int) { return 0; }
static std::atomic<size_t> g_device_bytes{(size_t)2 << 30};
hipError_t hipMemGetInfo(size_t *fr, size_t *tot) { *fr = *tot = g_device_bytes.load(); return 0; }
static std::atomic<size_t> g_alloc_limit{0};   // 0: none; else one allocation above it fails
hipError_t hipMalloc(void **p, size_t n) {
    if (g_alloc_limit.load() && n > g_alloc_limit.load()) return 2;
    void *q = calloc(n ? n : 1, 1);
    if (!q) return 2;
    std::lock_guard<std::mutex> lk(g_mu);
    g_live[q] = n;
    *p = q;
    return 0;
}
// page-locked host memory: plain host memory here (the staging vectors of the jobs, ngp_api.hip
// PinnedPool — reachable from its process-lifetime pool, so not a leak)
hipError_t hipHostMalloc(void **p, size_t n, unsigned) {
    *p = malloc(n ? n : 1);
    return *p ? 0 : 2;
}
hipError_t hipHostFree(void *p) { free(p); return 0; }
hipError_t hipFree(void *p) {
    if (!p) return 0;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (!g_live.erase(p)) { ++g_bad_free; return 1; }
    }
    free(p);
    return 0;
}
hipError_t hipMemcpy(void *d, const void *s, size_t n, int) {
    if (!inside(d, n) || !inside(s, n)) { ++g_oob; return 1; }
    memcpy(d, s, n);
    return 0;
}
// mock_hip_fail_copy_after, mock_hip_syncs; g_syncs_at_fail: the count when the ordered copy failed
static std::atomic<long> g_copy_fail_in{0}, g_syncs{0}, g_syncs_at_fail{0};
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int k, hipStream_t st) {
    if (g_copy_fail_in.load() > 0 && g_copy_fail_in.fetch_sub(1) == 1) {   // copies nothing
        g_syncs_at_fail.store(g_syncs.load());
        return 1;
    }
    if (tr().on) {
        char buf[96];
        std::snprintf(buf, sizeof buf, "C k%d %zu s%d", k, n, ordinal(tr().streams, st));
        trace_line(buf);
    }
    return hipMemcpy(d, s, n, k);
}
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t st) {
    if (tr().on) {
        char buf[96];
        std::snprintf(buf, sizeof buf, "M %zu s%d", n, ordinal(tr().streams, st));
        trace_line(buf);
    }
    if (!inside(d, n)) { ++g_oob; return 1; }
    memset(d, v, n);
    return 0;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) {
    *s = (hipStream_t)malloc(8);
    if (tr().on) tr().streams[*s] = tr().n_streams++;
    return 0;
}
hipError_t hipStreamDestroy(hipStream_t s) {
    if (tr().on) tr().streams.erase(s);
    free(s);
    return 0;
}
// a "busy device": every synchronisation takes mock_hip_set_sync_delay_us microseconds, so that
// concurrent callers pile up behind the one that holds the context (combine_stress.cpp)
hipError_t hipStreamSynchronize(hipStream_t) {
    ++g_syncs;
    const long us = g_sync_us.load();
    if (us > 0) std::this_thread::sleep_for(std::chrono::microseconds(us));
    return 0;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
    if (tr().on) {
        char buf[64];
        std::snprintf(buf, sizeof buf, "W e%d s%d", ordinal(tr().events, e), ordinal(tr().streams, s));
        trace_line(buf);
    }
    return 0;
}
// events made for timing (EventTimer: a pair per launch, made and destroyed at once) stay unnumbered
static std::atomic<long> g_timing_events{0};
hipError_t hipEventCreate(hipEvent_t *e) { *e = (hipEvent_t)malloc(8); ++g_timing_events; return 0; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) {
    *e = (hipEvent_t)malloc(8);
    if (tr().on) tr().events[*e] = tr().n_events++;
    return 0;
}
hipError_t hipEventDestroy(hipEvent_t e) {
    if (tr().on) tr().events.erase(e);
    free(e);
    return 0;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    if (tr().on) {
        char buf[64];
        std::snprintf(buf, sizeof buf, "R e%d s%d", ordinal(tr().events, e), ordinal(tr().streams, s));
        trace_line(buf);
    }
    return 0;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.001f; return 0; }
hipError_t hipGetLastError(void) { return 0; }
const char *hipGetErrorString(hipError_t) { return "mock HIP runtime"; }
hipError_t hipLaunchKernel(const void *fn, dim3_ g, dim3_ b, void **args, size_t shm, hipStream_t s) {
    ++g_launches;
    Trace &t = tr();
    if (t.on) {
        auto nm = t.names.find(fn);
        const std::string name = nm == t.names.end() ? "?" : nm->second;
        auto id = t.ids.find(name);
        char buf[256], extra[128];
        if (id == t.ids.end()) {
            id = t.ids.emplace(name, (int)t.ids.size()).first;
            std::snprintf(buf, sizeof buf, "K%d = ", id->second);
            trace_line((buf + name).c_str());
        }
        if (t.digest) {
            if ((int)t.by_id.size() <= id->second) t.by_id.resize((size_t)id->second + 1);
            t.by_id[(size_t)id->second] = name;
            auto it = t.tally.begin();
            while (it != t.tally.end() && it->id != id->second) ++it;
            if (it == t.tally.end()) t.tally.push_back({id->second, 1, g});
            else ++it->n;
        }
        const int so = ordinal(t.streams, s);
        if (std::find(t.launch_streams.begin(), t.launch_streams.end(), so) == t.launch_streams.end())
            t.launch_streams.push_back(so);
        trace_args(name, args, extra, sizeof extra);
        std::snprintf(buf, sizeof buf, "L K%d %u,%u,%u %u %zu s%d%s", id->second, g.x, g.y, g.z, b.x,
                      shm, ordinal(t.streams, s), extra);
        trace_line(buf);
    }
    return 0;
}

// kernel<<<...>>> lowering
struct CallCfg { dim3_ g, b; size_t shm; hipStream_t s; };
static thread_local CallCfg t_cfg;
hipError_t __hipPushCallConfiguration(dim3_ g, dim3_ b, size_t shm, hipStream_t s) { t_cfg = {g, b, shm, s}; return 0; }
hipError_t __hipPopCallConfiguration(dim3_ *g, dim3_ *b, size_t *shm, hipStream_t *s) {
    *g = t_cfg.g; *b = t_cfg.b; *shm = t_cfg.shm; *s = t_cfg.s;
    return 0;
}
void **__hipRegisterFatBinary(const void *) { static void *h; return &h; }
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host_fn, char *, const char *device_name, unsigned, void *,
                           void *, void *, void *, int *) {
    tr().names[host_fn] = device_name;
}
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}

// for the driver
long mock_hip_launches(void) { return g_launches.load(); }
void mock_hip_set_sync_delay_us(long us) { g_sync_us.store(us); }
long mock_hip_live_allocations(void) { std::lock_guard<std::mutex> lk(g_mu); return (long)g_live.size(); }
long mock_hip_errors(void) { return g_bad_free.load() + g_oob.load(); }
// the trace: switch it on before the first context is created (streams are numbered as they are made);
// flush before the driver prints a line of its own
// 0: off, 1: print every line, 2: digest
void mock_hip_trace(int on) { trace_flush(); tr().on = on != 0; tr().digest = on == 2; }
// digest mode: lines and their hash since the last call, and the kernels launched: "name[grid of the
// first launch] x count, ..." (name: the function and its template arguments as mangled)
const char *mock_hip_trace_digest(long *lines, unsigned long long *hash) {
    trace_flush();
    Trace &t = tr();
    t.summary.clear();
    for (const auto &k : t.tally) {
        const std::string &m = t.by_id[(size_t)k.id];
        char *e = nullptr;
        const long len = m.compare(0, 7, "_ZN3ngp") == 0 ? std::strtol(m.c_str() + 7, &e, 10) : 0;
        std::string nm = len > 0 ? std::string(e, (size_t)len) : m;
        if (len > 0 && e[len] == 'I') {           // template arguments, up to the "EEv" that ends them
            const char *end = std::strstr(e + len, "EEv");
            if (end) nm.append((const char *)e + len, end);
        }
        for (const char *cut : {"NS_7NoProbeE", "_kernel"})   // (said by every column kernel / every kernel)
            for (size_t at; (at = nm.find(cut)) != std::string::npos;) nm.erase(at, std::strlen(cut));
        char buf[64];
        std::snprintf(buf, sizeof buf, "[%u,%u,%u] x%ld", k.first.x, k.first.y, k.first.z, k.n);
        t.summary += (t.summary.empty() ? "" : ", ") + nm + buf;
    }
    t.tally.clear();
    *lines = tr().lines;
    *hash = tr().hash;
    tr().lines = 0;
    tr().hash = 14695981039346656037ull;
    return t.summary.c_str();
}
void mock_hip_trace_flush(void) { trace_flush(); }
// allocations above `bytes` fail (0: no limit) — the reserve loops of the library cut their chunks
void mock_hip_set_alloc_limit(size_t bytes) { g_alloc_limit.store(bytes); }
// the n-th hipMemcpyAsync from now on returns 1 and copies nothing (0: switched off); returns how
// many copies the previous order still had to wait for (0: it has failed its copy, or there was none)
long mock_hip_fail_copy_after(long n) { return g_copy_fail_in.exchange(n > 0 ? n : 0); }
// hipStreamSynchronize calls so far
long mock_hip_syncs(void) { return g_syncs.load(); }
// the same count at the moment the copy ordered by mock_hip_fail_copy_after failed
long mock_hip_syncs_at_failed_copy(void) { return g_syncs_at_fail.load(); }
// events made for timing so far (EventTimer: two per timed launch record)
long mock_hip_timing_events(void) { return g_timing_events.load(); }
// how many different streams saw a kernel launch since the last call of this function (trace on)
long mock_hip_launch_streams(void) {
    const long n = (long)tr().launch_streams.size();
    tr().launch_streams.clear();
    return n;
}
// what hipMemGetInfo reports (2 GiB unless set; memory is only touched where the host layer copies)
void mock_hip_set_device_bytes(size_t bytes) { g_device_bytes.store(bytes); }
}

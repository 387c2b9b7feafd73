// The launch sequences of the library, written down: a fixed table of calls goes through the C-ABI
// against the mock HIP runtime with its trace on (mock_hip.cpp), single-threaded and with combining
// off, and everything the host layer asks of the runtime is printed — kernel (mangled name, so the
// template arguments show), grid, block, LDS bytes, stream, the geometry and step arguments, events,
// memsets, copies — and after every group of calls the profile's flops, bytes and launches.
// By default a call's records are printed as their number, a hash and the kernels launched (name,
// grid of the first launch, count: a job cut into chunks shows as several tables_kernel launches of
// the chunk's size); `route_trace --full` prints every record, for a diff of two builds.
// tests/test_route_trace.py compares the output byte for byte with tests/golden/route_trace_v1.txt:
// a change of any host-side route rule (which kernel, which shape, which stream, in which order) or
// of a roofline formula shows as a diff.  The table puts at least one job on each side of every
// rule in csrc/ngp_plan.h; the geometries are those of tests/test_value_routes_gpu.py and
// tests/test_routes_gpu.py.
// `route_trace --grammar FILE` runs the grammar zoo instead (below, before main).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <initializer_list>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/ngp.h"

extern "C" void mock_hip_trace(int on);
extern "C" void mock_hip_trace_flush(void);
extern "C" const char *mock_hip_trace_digest(long *lines, unsigned long long *hash);
extern "C" void mock_hip_set_alloc_limit(size_t bytes);
extern "C" void mock_hip_set_device_bytes(size_t bytes);
extern "C" long mock_hip_errors(void);

static int fails = 0;
static bool full = false;
static ngp_ctx *ctx = nullptr;

static void say(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
#include <cstdarg>
static void say(const char *fmt, ...) {
    mock_hip_trace_flush();
    va_list ap;
    va_start(ap, fmt);
    std::vprintf(fmt, ap);
    va_end(ap);
    std::printf("\n");
}
// the end of a call of the table: in digest mode, what the runtime was asked since the last one
static void done() {
    if (full) return;
    long n = 0;
    unsigned long long h = 0;
    const char *kernels = mock_hip_trace_digest(&n, &h);
    say("   %ld records #%016llx: %s", n, h, kernels);
}
#define OK(call) do { const ngp_status st_ = (call); if (st_ != NGP_OK) { ++fails; say("FAIL %s -> %d", #call, (int)st_); } } while (0)

// ---- trees: left folds of leaves (tests/value_cases.py tree()) ------------------------------------
enum { STAT = 0, CHAIN = 1, OTHER = 2 };   // whole tree stationary | Linear first, leaves folded on | a sum of two products
struct Ens {
    std::vector<std::vector<int32_t>> ops;
    std::vector<std::vector<double>> par;
    std::vector<ngp_kernel> ks;
    Ens(int B, std::initializer_list<int> sizes, std::initializer_list<int> kinds) {
        std::vector<int> sz(sizes), kd(kinds);
        ops.resize((size_t)B);
        par.resize((size_t)B);
        ks.resize((size_t)B);
        for (int i = 0; i < B; ++i) {
            const int n_ops = sz[(size_t)i % sz.size()], kind = kd[(size_t)i % kd.size()];
            const int leaves = (n_ops + 1) / 2;
            auto &o = ops[(size_t)i];
            auto &p = par[(size_t)i];
            auto leaf = [&](int k, bool linear) {
                if (linear) { o.push_back(NGP_OP_LINEAR); p.insert(p.end(), {0.5, 0.1, 0.5}); }
                else if (k % 3 == 2 && leaves <= 16) { o.push_back(NGP_OP_PERIODIC); p.insert(p.end(), {1.1 + 0.01 * k, 0.2, 0.4}); }
                else { o.push_back(NGP_OP_SQEXP); p.insert(p.end(), {0.1 + 0.01 * k, 0.5}); }
            };
            int k = 1;
            leaf(0, kind != STAT);
            if (kind == OTHER && leaves >= 4) {   // (LIN x SE) + (LIN x leaf): neither operand of the sum is a leaf
                leaf(1, false);
                o.push_back(NGP_OP_TIMES);
                leaf(2, true);
                leaf(3, false);
                o.push_back(NGP_OP_TIMES);
                o.push_back(NGP_OP_PLUS);
                k = 4;
            }
            for (; k < leaves; ++k) {
                leaf(k, false);
                o.push_back(k % 4 == 1 ? NGP_OP_TIMES : NGP_OP_PLUS);
            }
            ks[(size_t)i] = ngp_kernel{(int32_t)o.size(), (int32_t)p.size(), o.data(), p.data(), 0.02 + 0.001 * (i % 7)};
        }
    }
};

struct Series {
    std::vector<double> t, y, t_add, y_add, t_new;
    Series(int n, bool lattice, int d, int D, int m) {
        // dates on a lattice of step 1 / 4096 (exact in binary), or pushed off it by up to 0.3 of a step
        // (golden-ratio fractions: on no common lattice)
        auto at = [&](int i) {
            const double x = i * 0.6180339887498949;
            return (i + (lattice ? 0.0 : 0.3 * (x - (double)(long)x))) / 4096.0;
        };
        t.resize((size_t)n);
        y.resize((size_t)n);
        for (int i = 0; i < n; ++i) { t[(size_t)i] = at(i); y[(size_t)i] = ((i * 37) % 11) / 11.0 - 0.5; }
        for (int a = 0; a < d; ++a) t_add.push_back(at(n + a));
        for (int i = 0; i < D * d; ++i) y_add.push_back(0.1 * (i % 5));
        for (int i = 0; i < m; ++i) t_new.push_back(at(n + d + i));
        if (t_add.empty()) t_add.push_back(0.0);
        if (y_add.empty()) y_add.push_back(0.0);
        if (t_new.empty()) t_new.push_back(0.0);
    }
};

static std::vector<double> out_a, out_b, out_c, out_d;
static std::vector<int32_t> out_i;
static void room(size_t n) {
    if (out_a.size() < n) { out_a.resize(n); out_b.resize(n); out_c.resize(n); out_d.resize(n); out_i.resize(n); }
}

static void value(int n, int B, bool lattice, std::initializer_list<int> kinds, int m = 4, int d = 2, int D = 3,
                  int n_ops = 0) {
    say("== nowcast n=%d B=%d lattice=%d m=%d d=%d D=%d", n, B, (int)lattice, m, d, D);
    Ens e = n_ops ? Ens(B, {n_ops}, kinds) : Ens(B, {1, 3, 5, 7, 9}, kinds);
    Series s(n, lattice, d, D, m);
    room((size_t)B * (size_t)std::max(D * std::max(m, 1), m * m) + 16);
    OK(ngp_nowcast_batch(ctx, B, e.ks.data(), n, s.t.data(), s.y.data(), d, s.t_add.data(), D, s.y_add.data(),
                         m, s.t_new.data(), 1, out_a.data(), out_b.data(), out_c.data(), out_d.data(), out_i.data()));
    done();
}
static void logml(int n, int B, bool lattice) {
    say("== logml n=%d B=%d lattice=%d", n, B, (int)lattice);
    Ens e(B, {1, 3, 5, 7, 9}, {STAT, CHAIN, OTHER});
    Series s(n, lattice, 0, 1, 0);
    room((size_t)B + 16);
    OK(ngp_logml_batch(ctx, B, e.ks.data(), n, s.t.data(), s.y.data(), 0, out_a.data(), out_i.data()));
    done();
}
static void resident(int n, int P) {
    say("== factor n=%d P=%d", n, P);
    Ens e(P, {1, 3, 5}, {STAT, CHAIN, OTHER});
    Series s(n, true, 2, 3, 4);
    room((size_t)P * 16 + 16);
    ngp_factor *f = nullptr;
    OK(ngp_factor_create(ctx, P, e.ks.data(), n, s.t.data(), s.y.data(), 0, &f));
    done();
    if (!f) return;
    say("-- nowcast");
    OK(ngp_factor_nowcast(f, 2, s.t_add.data(), 3, s.y_add.data(), 4, s.t_new.data(), 1, out_a.data(),
                          out_b.data(), out_c.data(), out_d.data(), out_i.data()));
    ngp_factor_destroy(f);
    done();
}
static void grad(int n, int B, bool lattice, std::initializer_list<int> sizes, std::initializer_list<int> kinds,
                 bool rerun = false) {
    std::vector<int> sz(sizes), kd(kinds);
    say("== grad n=%d B=%d lattice=%d sizes=%d.. kinds=%d..(%d) rerun=%d", n, B, (int)lattice, sz[0], kd[0],
        (int)kd.size(), (int)rerun);
    Ens e(B, sizes, kinds);
    Series s(n, lattice, 0, 1, 0);
    room((size_t)B * (NGP_MAX_PARAMS + 1) + 16);
    if (!rerun) {
        OK(ngp_logml_grad_batch(ctx, B, e.ks.data(), n, s.t.data(), s.y.data(), 0, out_a.data(), out_b.data(),
                                out_i.data()));
        done();
        return;
    }
    ngp_grad_job *j = nullptr;
    OK(ngp_grad_stage(ctx, B, e.ks.data(), n, s.t.data(), s.y.data(), 0, &j));
    if (!j) return;
    OK(ngp_grad_job_run(j, out_a.data(), out_b.data(), out_i.data()));
    std::vector<double> flat, nz;
    for (int k = 0; k < B; ++k) {
        for (double v : e.par[(size_t)k]) flat.push_back(v * 1.01);
        nz.push_back(e.ks[(size_t)k].noise * 0.9);
    }
    done();
    say("-- new parameters");
    OK(ngp_grad_job_set_params(j, flat.data(), nz.data()));
    OK(ngp_grad_job_run(j, out_a.data(), out_b.data(), out_i.data()));
    int32_t how[5] = {};
    OK(ngp_grad_job_info(j, how));
    say("-- leaves: general %d (chunk %d), toeplitz %d (chunk %d), side by side %d", how[0], how[1], how[2],
        how[3], how[4]);
    ngp_grad_job_destroy(j);
    done();
}

static void profile(const char *group) {
    ngp_profile p;
    OK(ngp_profile_get(ctx, &p));
    say("## profile after %s", group);
    for (int c = 0; c < NGP_NUM_KERNEL_CLASSES; ++c)
        if (p.launches[c]) say("P %d %lld %.17g %.17g", c, (long long)p.launches[c], p.flops[c], p.bytes[c]);
    OK(ngp_profile_reset(ctx));
}

// A new context: its memory budget is what the mock device reports NOW, and its workspace is empty
// (a context refreshes its budget only when a job exceeds it, and a workspace grown by an earlier job
// never meets the allocator again).
static void fresh_context(size_t device_bytes = (size_t)2 << 30) {
    if (ctx) ngp_ctx_destroy(ctx);
    ctx = nullptr;
    mock_hip_set_device_bytes(device_bytes);
    if (ngp_ctx_create(0, &ctx) != NGP_OK) { say("FAIL no context"); std::exit(2); }
    OK(ngp_set_combining(ctx, 0));
    OK(ngp_profile_enable(ctx, 1));
}

static void precision(int prec, int refine_max) {
    ngp_spec sp;
    ngp_default_spec(&sp);
    sp.precision = prec;
    sp.refine_max = refine_max;
    OK(ngp_set_spec(ctx, &sp));
}

// ---- route_trace --grammar FILE: the grammar zoo (tests/grammar_cases.py writes the file: one item per
// line, "name | operators | parameters | noise") through the batches of tests/test_grammar_gpu.py whose
// contraction instantiation the kernel-class profile cannot show.  tests/test_route_trace.py compares
// the output with tests/golden/route_trace_grammar_v1.txt.
struct Zoo {
    std::vector<std::string> names;
    std::vector<std::vector<int32_t>> ops;
    std::vector<std::vector<double>> par;
    std::vector<double> noise;
    explicit Zoo(const char *path) {
        std::ifstream in(path);
        std::string line;
        while (std::getline(in, line)) {
            if (line.empty()) continue;
            std::vector<std::string> f;
            size_t a = 0;
            for (size_t b; (b = line.find('|', a)) != std::string::npos; a = b + 1) f.push_back(line.substr(a, b - a));
            f.push_back(line.substr(a));
            if (f.size() != 4) { say("FAIL zoo line: %s", line.c_str()); std::exit(2); }
            std::istringstream nm(f[0]), so(f[1]), sp(f[2]);
            std::string name;
            nm >> name;
            names.push_back(name);
            ops.emplace_back();
            par.emplace_back();
            for (int v; so >> v;) ops.back().push_back(v);
            for (double v; sp >> v;) par.back().push_back(v);
            noise.push_back(std::stod(f[3]));
        }
    }
    // the items idx as kernels (the vectors above outlive them)
    std::vector<ngp_kernel> kernels(const std::vector<int> &idx) const {
        std::vector<ngp_kernel> ks;
        for (int i : idx)
            ks.push_back(ngp_kernel{(int32_t)ops[(size_t)i].size(), (int32_t)par[(size_t)i].size(), ops[(size_t)i].data(),
                                    par[(size_t)i].data(), noise[(size_t)i]});
        return ks;
    }
    bool toeplitz_eligible(int i) const {
        for (int32_t o : ops[(size_t)i]) if (o == NGP_OP_LINEAR || o == NGP_OP_CHANGEPOINT) return false;
        return ops[(size_t)i].size() <= 31;
    }
};

static void zoo_grad(const Zoo &z, const char *row, const std::vector<int> &idx, int n) {
    int maxops = 0;
    for (int i : idx) maxops = std::max(maxops, (int)z.ops[(size_t)i].size());
    say("== %s n=%d B=%d largest tree %d operators", row, n, (int)idx.size(), maxops);
    std::vector<ngp_kernel> ks = z.kernels(idx);
    Series s(n, true, 0, 1, 0);
    room(idx.size() * (NGP_MAX_PARAMS + 1) + 16);
    ngp_grad_job *j = nullptr;
    OK(ngp_grad_stage(ctx, (int32_t)ks.size(), ks.data(), n, s.t.data(), s.y.data(), 0, &j));
    if (!j) return;
    OK(ngp_grad_job_run(j, out_a.data(), out_b.data(), out_i.data()));
    int32_t how[5] = {};
    OK(ngp_grad_job_info(j, how));
    say("-- leaves: general %d, toeplitz %d", how[0], how[2]);
    ngp_grad_job_destroy(j);
    done();
}

static int grammar(const char *path) {
    Zoo z(path);
    const int B = (int)z.names.size();
    say("grammar zoo: %d items", B);
    std::vector<int> by_size((size_t)B);
    for (int i = 0; i < B; ++i) by_size[(size_t)i] = i;
    std::stable_sort(by_size.begin(), by_size.end(),
                     [&](int a, int b) { return z.ops[(size_t)a].size() < z.ops[(size_t)b].size(); });
    auto prefixes = [&](const std::vector<int> &idx) {
        std::vector<std::vector<int>> out;
        for (size_t cap : {1, 3, 7, 15, 31, 63}) {
            std::vector<int> p;
            for (int i : idx) if (z.ops[(size_t)i].size() <= cap) p.push_back(i);
            if (!p.empty() && (out.empty() || p.size() > out.back().size())) out.push_back(p);
        }
        return out;
    };
    for (const auto &p : prefixes(by_size)) zoo_grad(z, "G-sized", p, 130);
    OK(ngp_set_batch_invariant(ctx, 1));
    zoo_grad(z, "G-own", by_size, 130);
    OK(ngp_set_batch_invariant(ctx, 0));
    std::vector<int> toep;
    int stat17 = -1;
    for (int i : by_size) {
        if (z.toeplitz_eligible(i)) toep.push_back(i);
        if (z.names[(size_t)i] == "stat17") stat17 = i;
    }
    for (const auto &p : prefixes(toep)) zoo_grad(z, "G-toep", p, 321);
    toep.push_back(stat17);
    zoo_grad(z, "G-toep with the 17-leaf tree", toep, 321);
    {
        say("== V-lists n=321 B=%d", B);
        std::vector<ngp_kernel> ks = z.kernels(by_size);
        const int d = 2, D = 2, m = 5;
        Series s(321, true, d, D, m);
        room((size_t)B * (size_t)(D * m + m * m) + 16);
        OK(ngp_nowcast_batch(ctx, B, ks.data(), 321, s.t.data(), s.y.data(), d, s.t_add.data(), D, s.y_add.data(),
                             m, s.t_new.data(), 1, out_a.data(), out_b.data(), out_c.data(), out_d.data(), out_i.data()));
        done();
    }
    ngp_ctx_destroy(ctx);
    if (mock_hip_errors()) { ++fails; say("FAIL the mock runtime saw a bad free or an out-of-bounds copy"); }
    say("route_trace --grammar: %d failures", fails);
    return fails ? 1 : 0;
}

int main(int argc, char **argv) {
    full = argc > 1 && std::string(argv[1]) == "--full";
    mock_hip_trace(full ? 1 : 2);
    fresh_context();
    if (argc > 2 && std::string(argv[1]) == "--grammar") return grammar(argv[2]);
    const std::initializer_list<int> MIX = {STAT, CHAIN, OTHER};

    // ---- value jobs: short series (one launch | column sweep), the three fill kernels -------------
    for (int B : {1, 24, 4096, 4097}) value(130, B, true, MIX);
    for (int B : {1, 24, 4096, 4097}) value(200, B, true, MIX);
    for (int n : {256, 319, 320}) value(n, 24, true, MIX);
    value(256, 24, true, MIX, 60);      // two sweeps of the one-launch kernel
    value(256, 24, true, MIX, 180);     // three
    value(130, 24, false, MIX);
    value(200, 24, false, MIX);
    logml(330, 2, true);
    logml(130, 24, true);
    profile("short value jobs");

    // ---- value jobs on the column sweep --------------------------------------------------------------
    for (int n : {448, 1024}) { value(n, 24, true, MIX); value(n, 24, false, MIX); }
    for (int n : {377, 378, 441, 442}) value(n, 24, true, MIX);   // naux = 64 | 65, 128 | 129 at nb0 = 5
    value(448, 512, true, MIX);          // nb0 = 7 | 8: split-k
    value(512, 512, true, MIX);          // 512 | 513 items: diagonal form, diag-ahead order, split-k
    value(512, 513, true, MIX);
    value(576, 64, true, MIX);           // nb0 = 9: the pairs start at column 1
    value(448, 8, true, MIX);            // few items: the late fat steps of nb0 = 8 are cut along k, nb0 = 7 not
    value(512, 8, true, MIX);
    value(1024, 55, true, MIX);          // 384 / 55 = 6 pieces at column 14 (one tile pair, 56 chunks)
    profile("column sweep");
    value(1536, 63, true, MIX);          // two lanes: 63 | 64 items, 23 | 24 block columns
    value(1536, 64, true, MIX);
    value(1472, 64, true, MIX);
    value(1536, 64, false, MIX);
    value(2048, 8, true, MIX);
    value(2049, 8, true, MIX);
    value(2112, 8, true, MIX);           // 33 block columns
    profile("long series");

    // ---- fill launches by size: 1024 | 2048 workgroups, four tiles per workgroup from 65,536 on --
    for (int B : {29, 30, 58, 59}) value(448, B, true, {OTHER}, 4, 2, 3, 7);       // 35 tiles per item
    profile("fill sizes");
    fresh_context((size_t)8 << 30);
    for (int B : {1489, 1490}) value(512, B, true, {CHAIN});           // 44 tiles x 1,490 = 65,560
    for (int B : {32767, 32768}) value(100, B, true, {CHAIN});         // 2 tiles: 65,536 exactly
    profile("fill sizes, large launches");

    // ---- chunks (a device of 2 GiB: 1.5 GiB for a job's factor storage) -----------------------------
    fresh_context();
    value(448, 1000, true, MIX);         // 1.8 GB: two equal chunks of 500
    value(130, 4097, true, MIX);         // (fits: one chunk beyond the one-launch path)
    profile("chunks by the memory budget");
    fresh_context();
    mock_hip_set_alloc_limit((size_t)64 << 20);
    value(448, 100, true, MIX);          // 190 MB in one chunk: the allocation fails, twice the chunks until it fits
    mock_hip_set_alloc_limit(0);
    profile("chunks by a failed allocation");
    fresh_context();

    // ---- switches ------------------------------------------------------------------------------------
    OK(ngp_set_short_series_path(ctx, 0));
    for (int n : {130, 200, 256}) value(n, 24, true, MIX);
    OK(ngp_set_short_series_path(ctx, 1));
    OK(ngp_set_batch_invariant(ctx, 1));
    value(130, 4097, true, MIX);
    value(200, 24, true, MIX);
    value(512, 512, true, MIX);
    value(1536, 64, true, MIX);
    OK(ngp_set_batch_invariant(ctx, 0));
    OK(ngp_set_structured_storage(ctx, 0));
    value(448, 24, true, MIX);
    value(1536, 64, true, MIX);
    OK(ngp_set_structured_storage(ctx, 1));
    profile("switches");

    // ---- mixed precision -------------------------------------------------------------------------------
    for (int rm : {3, 0}) {
        precision(NGP_PREC_MIXED, rm);
        for (int n : {100, 130, 1536}) value(n, 8, true, MIX);
    }
    precision(NGP_PREC_F64, 3);
    profile("mixed precision");

    // ---- resident factors ----------------------------------------------------------------------------
    resident(130, 24);
    resident(330, 24);
    resident(1024, 8);
    profile("resident factors");

    // ---- gradient jobs, general leaf (trees with a Linear leaf) --------------------------------------
    for (int n : {21, 208, 448}) for (int B : {512, 513}) grad(n, B, true, {3, 5}, {CHAIN});
    for (int B : {36, 37, 73, 74}) grad(448, B, true, {3, 5}, {CHAIN});   // 28 tiles: 1024 | 2048 workgroups
    grad(512, 24, true, {3, 7}, {CHAIN, OTHER});                          // nb0 = 7 | 8: the K^-1 form
    grad(512, 512, true, {3, 7}, {CHAIN, OTHER});
    grad(2049, 4, true, {3, 7}, {CHAIN, OTHER});
    grad(208, 24, false, {3, 5}, {CHAIN});
    grad(448, 24, false, {3, 5}, {CHAIN});
    grad(208, 4097, true, {3}, {CHAIN});                                   // beyond the one-launch path
    for (int B : {1024, 1025, 2048, 2049}) grad(50, B, true, {3}, {CHAIN});   // one tile: the steps themselves
    for (int B : {4096, 4097}) grad(50, B, true, {1, 3, 7}, {CHAIN});      // by size from 4,097 workgroups on
    profile("gradient, general leaf");
    fresh_context((size_t)24 << 30);
    for (int B : {2340, 2341}) grad(448, B, true, {3}, {CHAIN});           // 28 x 2,341 = 65,548
    profile("gradient, large launches");
    fresh_context();
    // trees of 1 .. 32 leaves in one batch: buckets, two streams up to 512 items
    for (int B : {24, 512, 513}) grad(448, B, true, {1, 3, 7, 15, 31, 63}, {CHAIN});
    grad(448, 148, true, {1, 3, 7, 15, 31}, {CHAIN});                      // 28 x 147 > 4096: by size, no large trees
    grad(448, 146, true, {1, 3, 7, 15, 31}, {CHAIN});
    grad(208, 24, true, {3, 5}, {CHAIN}, true);
    grad(448, 24, true, {3, 5}, {CHAIN}, true);
    profile("gradient, buckets and re-runs");
    // chunks of both leaves: by the memory budget (3 GB and 4 GB on the 2 GiB device), then halved by
    // the reserve loop when the allocation fails
    fresh_context();
    grad(448, 600, true, {3, 5}, {CHAIN}, true);
    grad(448, 2000, true, {3, 5}, {STAT}, true);
    profile("gradient, chunks by the memory budget");
    fresh_context();
    mock_hip_set_alloc_limit((size_t)64 << 20);
    grad(448, 64, true, {3, 5}, {CHAIN}, true);
    mock_hip_set_alloc_limit(0);
    profile("gradient, chunks by a failed allocation");
    fresh_context();

    // ---- gradient jobs: stationary trees on a regular series (Toeplitz leaf), alone and mixed ------
    for (int n : {208, 448, 1024}) grad(n, 24, true, {1, 3, 7, 15, 31}, {STAT});
    grad(208, 4097, true, {3}, {STAT});
    for (int B : {128, 129, 512, 513}) grad(1024, B, true, {1, 3, 7, 15, 31}, {STAT});   // 4 x 129 > 512: by size
    for (int B : {170, 171}) grad(600, B, true, {1, 3, 7}, {STAT});        // 3 x 171 = 513
    for (int B : {127, 128, 255, 256}) for (int n : {1023, 1024}) grad(n, B, true, {3, 5}, {STAT, CHAIN}, true);
    OK(ngp_set_batch_invariant(ctx, 1));
    grad(448, 24, true, {3, 5}, {STAT, CHAIN}, true);
    grad(448, 37, true, {3, 5}, {CHAIN});
    grad(208, 24, true, {1, 3, 7}, {CHAIN});
    OK(ngp_set_batch_invariant(ctx, 0));
    OK(ngp_set_structured_storage(ctx, 0));
    grad(448, 24, true, {3, 5}, {STAT});
    OK(ngp_set_structured_storage(ctx, 1));
    OK(ngp_set_short_series_path(ctx, 0));
    grad(208, 24, true, {3, 5}, {STAT, CHAIN});
    OK(ngp_set_short_series_path(ctx, 1));
    profile("gradient, Toeplitz leaf and mixed batches");

    ngp_ctx_destroy(ctx);
    if (mock_hip_errors()) { ++fails; say("FAIL the mock runtime saw a bad free or an out-of-bounds copy"); }
    say("route_trace: %d failures", fails);
    return fails ? 1 : 0;
}

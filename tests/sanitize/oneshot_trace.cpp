// The launch sequences of the one-shot device calls, written down: the table of oneshot_calls.h goes
// through the C-ABI against the mock HIP runtime with its trace on (mock_hip.cpp), single-threaded
// and with combining off, as route_trace.cpp does for the staged jobs.  After each call the number of
// records (kernel launches with grid, block, LDS bytes, stream and integer arguments; event records;
// memsets; copies with kind, bytes and stream), their hash and the kernels launched are printed;
// `oneshot_trace --full` prints every record, for a diff of two builds.
// tests/test_oneshot_trace.py compares the output byte for byte with
// tests/golden/oneshot_trace_v2.txt: a one-shot call that issues another copy or launch, or the same
// ones in another order, shows as a diff.  The mock's copies happen at once and its launches write
// nothing, so ngp_mixture_crps_mapped plans its rounds from a zeroed scan record.  A section of
// invalid calls follows the table (below).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "oneshot_calls.h"

extern "C" void mock_hip_trace(int on);
extern "C" void mock_hip_trace_flush(void);
extern "C" const char *mock_hip_trace_digest(long *lines, unsigned long long *hash);
extern "C" long mock_hip_errors(void);
extern "C" long mock_hip_live_allocations(void);

static int fails = 0;
static bool full = false;

static void say(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void say(const char *fmt, ...) {
    mock_hip_trace_flush();
    va_list ap;
    va_start(ap, fmt);
    std::vprintf(fmt, ap);
    va_end(ap);
    std::printf("\n");
}
static void done() {
    if (full) return;
    long n = 0;
    unsigned long long h = 0;
    const char *kernels = mock_hip_trace_digest(&n, &h);
    say("   %ld records #%016llx: %s", n, h, kernels);
}
#define OK(call) do { const ngp_status st_ = (call); if (st_ != NGP_OK) { ++fails; say("FAIL %s -> %d", #call, (int)st_); } } while (0)

// ---- invalid calls of the three families that take a forecast mixture ----------------------------
// The arguments of the Paths fixture with one of them (or two) spoilt; every call must return before
// anything touches a device.  One line per call, `family form, fault: status`: which status a
// fault gets, and which of two wins, is part of what the host code around these calls may not change.
struct Spoilt {
    oneshot::Paths pa;
    int32_t P = pa.P, S = pa.S, m = pa.m, draws = pa.draws, fair = 1, scale = NGP_SCORE_NATURAL;
    bool null_w = false, null_seeds = false;
    ngp_inv_transform inv = pa.inv;
    ngp_path_target tg[oneshot::Paths::T];
    double probs[oneshot::Paths::Q], shift = 0.0;
    std::vector<double> y = std::vector<double>(NGP_MAX_AUX + 1, 1.25);
    int32_t win[4] = {2, 2, 0, pa.m - 1};
    Spoilt() {
        for (int i = 0; i < pa.T; ++i) tg[i] = pa.tg[i];
        for (int i = 0; i < pa.Q; ++i) probs[i] = pa.probs[i];
    }
    const double *w() { return null_w ? nullptr : pa.w.data(); }
    const double *sigma(bool indep) { return indep ? pa.sigma_indep.data() : pa.sigma.data(); }
    const uint64_t *seeds() { return null_seeds ? nullptr : pa.seeds; }
    ngp_status sample(ngp_ctx *c, bool indep) {
        if (indep)
            return ngp_mixture_sample_indep(c, P, S, m, w(), pa.mu.data(), sigma(true), draws, seeds(),
                                            pa.out.data(), nullptr, nullptr);
        return ngp_mixture_sample(c, P, S, m, w(), pa.mu.data(), sigma(false), draws, 11u, pa.out.data(),
                                  nullptr, nullptr);
    }
    ngp_status targets(ngp_ctx *c, bool indep) {
        if (indep)
            return ngp_mixture_path_targets_indep(c, P, S, m, w(), pa.mu.data(), sigma(true), draws, seeds(),
                                                  &inv, pa.T, tg, pa.Q, probs, pa.q.data(), pa.mean.data(),
                                                  pa.count.data(), pa.hist.data(), nullptr, pa.info.data());
        return ngp_mixture_path_targets(c, P, S, m, w(), pa.mu.data(), sigma(false), draws, 11u, &inv, pa.T, tg,
                                        pa.Q, probs, pa.q.data(), pa.mean.data(), pa.count.data(),
                                        pa.hist.data(), nullptr, pa.info.data());
    }
    ngp_status scores(ngp_ctx *c, bool indep) {
        return ngp_mixture_path_scores(c, P, S, m, w(), pa.mu.data(), sigma(indep), indep ? 1 : 0, draws, seeds(),
                                       &inv, y.data(), scale, shift, fair, 2, win, pa.es, pa.term_obs,
                                       pa.term_pair, pa.winfo, nullptr);
    }
};

enum { F_SAMPLE = 1, F_TARGETS = 2, F_SCORES = 4, F_SHARED_TOO = 8, F_ALL = 15 };

static void invalid(ngp_ctx *ctx, const char *fault, int which, const std::function<void(Spoilt &)> &spoil) {
    for (int indep = (which & F_SHARED_TOO) ? 0 : 1; indep < 2; ++indep) {
        const char *form = indep ? "indep" : "shared";
        if (which & F_SAMPLE) { Spoilt s; spoil(s); say("sample %s, %s: %d", form, fault, (int)s.sample(ctx, indep)); }
        if (which & F_TARGETS) { Spoilt s; spoil(s); say("path_targets %s, %s: %d", form, fault, (int)s.targets(ctx, indep)); }
        if (which & F_SCORES) { Spoilt s; spoil(s); say("path_scores %s, %s: %d", form, fault, (int)s.scores(ctx, indep)); }
    }
}

static void invalid_calls(ngp_ctx *ctx) {
    const double inf = 1.0 / 0.0;
    const int paths = F_TARGETS | F_SCORES | F_SHARED_TOO;
    say("-- invalid calls");
    invalid(ctx, "null w", F_ALL, [](Spoilt &s) { s.null_w = true; });
    invalid(ctx, "draws = 0", F_ALL, [](Spoilt &s) { s.draws = 0; });
    invalid(ctx, "m = NGP_MAX_AUX + 1", F_ALL, [](Spoilt &s) { s.m = NGP_MAX_AUX + 1; });
    // (the shared form of the scores reads seeds[0]: null seeds are refused there as well)
    invalid(ctx, "null seeds", F_SAMPLE | F_TARGETS, [](Spoilt &s) { s.null_seeds = true; });
    invalid(ctx, "null seeds", F_SCORES | F_SHARED_TOO, [](Spoilt &s) { s.null_seeds = true; });
    invalid(ctx, "inv of unknown kind", paths, [](Spoilt &s) { s.inv.kind = NGP_INV_BOXCOX + 1; });
    invalid(ctx, "Box-Cox with cap = 0", paths, [](Spoilt &s) { s.inv.cap = 0.0; });
    invalid(ctx, "a level of 1.0", F_TARGETS | F_SHARED_TOO, [](Spoilt &s) { s.probs[1] = 1.0; });
    invalid(ctx, "a window with j1 = m", paths, [](Spoilt &s) { s.tg[0].j1 = s.m; s.win[3] = s.m; });
    invalid(ctx, "fair = 1 with one path", F_SCORES | F_SHARED_TOO, [](Spoilt &s) { s.S = 1; s.draws = 1; });
    invalid(ctx, "a non-finite y", F_SCORES | F_SHARED_TOO, [=](Spoilt &s) { s.y[3] = inf; });
    invalid(ctx, "log scale with y + shift = 0", F_SCORES | F_SHARED_TOO,
            [](Spoilt &s) { s.scale = NGP_SCORE_LOG; s.shift = 0.5; s.y[1] = -0.5; });
    // two faults: which status wins
    invalid(ctx, "m = NGP_MAX_AUX + 1 and null w", F_ALL, [](Spoilt &s) { s.m = NGP_MAX_AUX + 1; s.null_w = true; });
    invalid(ctx, "m = NGP_MAX_AUX + 1 and draws = 0", F_ALL, [](Spoilt &s) { s.m = NGP_MAX_AUX + 1; s.draws = 0; });
    invalid(ctx, "m = NGP_MAX_AUX + 1 and Box-Cox with cap = 0", paths,
            [](Spoilt &s) { s.m = NGP_MAX_AUX + 1; s.inv.cap = 0.0; });
    invalid(ctx, "m = NGP_MAX_AUX + 1 and a level of 1.0", F_TARGETS | F_SHARED_TOO,
            [](Spoilt &s) { s.m = NGP_MAX_AUX + 1; s.probs[1] = 1.0; });
    invalid(ctx, "m = NGP_MAX_AUX + 1 and a window with j1 = m", paths,
            [](Spoilt &s) { s.m = NGP_MAX_AUX + 1; s.tg[0].j1 = s.m; s.win[3] = s.m; });
    invalid(ctx, "m = NGP_MAX_AUX + 1 and a non-finite y", F_SCORES | F_SHARED_TOO,
            [=](Spoilt &s) { s.m = NGP_MAX_AUX + 1; s.y[3] = inf; });
    invalid(ctx, "m = NGP_MAX_AUX + 1 and fair = 1 with one path", F_SCORES | F_SHARED_TOO,
            [](Spoilt &s) { s.m = NGP_MAX_AUX + 1; s.S = 1; s.draws = 1; });
    // S P beyond 32 bits (the sampler alone does not bound it; its w would not exist: not called)
    invalid(ctx, "S P = 2^32", paths, [](Spoilt &s) { s.S = 65536; s.P = 65536; s.draws = 1; });
    invalid(ctx, "S P = 2^32 and a non-finite y", F_SCORES | F_SHARED_TOO,
            [=](Spoilt &s) { s.S = 65536; s.P = 65536; s.draws = 1; s.y[3] = inf; });
    invalid(ctx, "S P = 2^32 and a level of 1.0", F_TARGETS | F_SHARED_TOO,
            [](Spoilt &s) { s.S = 65536; s.P = 65536; s.draws = 1; s.probs[1] = 1.0; });
    done();   // no record: none of them reached the runtime
}

int main(int argc, char **argv) {
    full = argc > 1 && std::string(argv[1]) == "--full";
    mock_hip_trace(full ? 1 : 2);
    ngp_ctx *ctx = nullptr;
    if (ngp_ctx_create(0, &ctx) != NGP_OK) { say("FAIL no context"); return 2; }
    OK(ngp_set_combining(ctx, 0));
    OK(ngp_profile_enable(ctx, 1));
    for (const oneshot::Entry &e : oneshot::table()) {
        if (e.setup) {
            say("-- setup of %s", e.name.c_str());
            OK(e.setup(ctx));
            done();
        }
        // twice: the second call draws its blocks from what the first one gave back
        for (int rep = 0; rep < 2; ++rep) {
            say("== %s", e.name.c_str());
            OK(e.call(ctx));
            done();
        }
        if (e.teardown) e.teardown();
    }
    invalid_calls(ctx);
    ngp_ctx_destroy(ctx);
    if (mock_hip_errors()) { ++fails; say("FAIL the mock runtime saw a bad free or an out-of-bounds copy"); }
    if (mock_hip_live_allocations()) { ++fails; say("FAIL device allocations left after the context was destroyed"); }
    say("oneshot_trace: %d failures", fails);
    return fails ? 1 : 0;
}

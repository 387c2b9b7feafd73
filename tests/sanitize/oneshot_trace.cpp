// The launch sequences of the one-shot device calls, written down: the table of oneshot_calls.h goes
// through the C-ABI against the mock HIP runtime with its trace on (mock_hip.cpp), single-threaded
// and with combining off, as route_trace.cpp does for the staged jobs.  After each call the number of
// records (kernel launches with grid, block, LDS bytes, stream and integer arguments; event records;
// memsets; copies with kind, bytes and stream), their hash and the kernels launched are printed;
// `oneshot_trace --full` prints every record, for a diff of two builds.
// tests/test_oneshot_trace.py compares the output byte for byte with
// tests/golden/oneshot_trace_v3.txt: a one-shot call that issues another copy or launch, or the same
// ones in another order, shows as a diff.  The mock's copies happen at once and its launches write
// nothing, so ngp_mixture_crps_mapped plans its rounds from a zeroed scan record.  Behind the table
// come the long-horizon family on two more factors (long_table), two sections of invalid calls and
// the long-horizon family on devices so small that the particles go through in chunks (below).
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

// ---- invalid calls of the long-horizon family ----------------------------------------------------
// The arguments of the Long fixture (n = 191) with one of them or two spoilt, in the same form.
struct SpoiltLong {
    oneshot::Long &l;
    ngp_factor *f;
    int32_t d = l.d, D = l.D, m = l.m, draws = l.draws, R = l.R;
    std::vector<double> t_far = std::vector<double>(NGP_MAX_LONG_HORIZON + 1, 1.0);
    std::vector<double> t_add = std::vector<double>(NGP_MAX_AUX, 0.8), y_add = std::vector<double>(3 * NGP_MAX_AUX, 0.1);
    std::vector<int32_t> counts = std::vector<int32_t>(l.counts, l.counts + l.P);
    std::vector<int32_t> cut = std::vector<int32_t>(NGP_MAX_ORIGINS + 1);
    std::vector<ngp_kernel> comps = std::vector<ngp_kernel>(l.comps, l.comps + l.NC);
    bool null_t_new = false, null_t_add = false, null_y_add = false, null_mu = false, null_second = false,
         null_w = false, null_counts = false, null_comps = false, null_cut = false, with_sigma = false;
    explicit SpoiltLong(oneshot::Long &l_) : l(l_), f(l_.f) {
        for (size_t r = 0; r < cut.size(); ++r) cut[r] = r < l.cut.size() ? l.cut[r] : 0;
    }
    const double *tn() { return null_t_new ? nullptr : m > l.m ? t_far.data() : l.t_new.data(); }
    const double *ta() { return null_t_add ? nullptr : t_add.data(); }
    const double *ya() { return null_y_add ? nullptr : y_add.data(); }
    double *mu() { return null_mu ? nullptr : l.mu; }
    // the second required output: var, out, cross, var
    ngp_status predict_long() {
        return ngp_factor_predict_long(f, d, ta(), D, ya(), m, tn(), 1, mu(), null_second ? nullptr : l.var,
                                       with_sigma ? l.sigma : nullptr, l.info);
    }
    ngp_status sample_long() {
        return ngp_factor_sample_long(f, d, ta(), D, ya(), m, tn(), 1, null_w ? nullptr : l.w2, draws, 17u,
                                      null_second ? nullptr : l.out, l.comp, mu(), l.var, l.info, l.cinfo);
    }
    ngp_status components_long() {
        return ngp_factor_components_long(f, d, ta(), D, ya(), null_counts ? nullptr : counts.data(),
                                          null_comps ? nullptr : comps.data(), m, tn(), mu(),
                                          null_second ? nullptr : l.cross, with_sigma ? l.sigma : nullptr, l.info);
    }
    ngp_status predict_origins() {
        return ngp_factor_predict_origins(f, R, null_cut ? nullptr : cut.data(), m, tn(), 1, mu(),
                                          null_second ? nullptr : l.var, l.logml, l.info);
    }
};

enum { L_PREDICT = 1, L_SAMPLE = 2, L_COMPONENTS = 4, L_ORIGINS = 8, L_APPENDING = 7, L_ALL = 15 };

static void invalid_long(oneshot::Long &l, const char *fault, int which, const std::function<void(SpoiltLong &)> &spoil) {
    if (which & L_PREDICT) { SpoiltLong s(l); spoil(s); say("predict_long, %s: %d", fault, (int)s.predict_long()); }
    if (which & L_SAMPLE) { SpoiltLong s(l); spoil(s); say("sample_long, %s: %d", fault, (int)s.sample_long()); }
    if (which & L_COMPONENTS) { SpoiltLong s(l); spoil(s); say("components_long, %s: %d", fault, (int)s.components_long()); }
    if (which & L_ORIGINS) { SpoiltLong s(l); spoil(s); say("predict_origins, %s: %d", fault, (int)s.predict_origins()); }
}

static void invalid_long_calls(ngp_ctx *ctx) {
    static oneshot::Long l(191, 6);
    static int32_t plus_alone[1] = {6};
    const int over = NGP_MAX_LONG_HORIZON + 1, d_over = NGP_MAX_AUX - 191 % 64;   // tail + d + 1 = 193
    say("-- setup of the invalid calls of the long-horizon family");
    OK(l.create(ctx));
    done();
    say("-- invalid calls of the long-horizon family");
    invalid_long(l, "none", L_ALL, [](SpoiltLong &) {});
    done();
    invalid_long(l, "null factor", L_ALL, [](SpoiltLong &s) { s.f = nullptr; });
    invalid_long(l, "null t_new", L_ALL, [](SpoiltLong &s) { s.null_t_new = true; });
    invalid_long(l, "m = 0", L_ALL, [](SpoiltLong &s) { s.m = 0; });
    invalid_long(l, "m = NGP_MAX_LONG_HORIZON + 1", L_ALL, [=](SpoiltLong &s) { s.m = over; });
    invalid_long(l, "null mu", L_PREDICT | L_COMPONENTS | L_ORIGINS, [](SpoiltLong &s) { s.null_mu = true; });
    invalid_long(l, "null var / out / cross / var", L_ALL, [](SpoiltLong &s) { s.null_second = true; });
    invalid_long(l, "d = -1", L_APPENDING, [](SpoiltLong &s) { s.d = -1; });
    invalid_long(l, "d = 2 with D = 0", L_APPENDING, [](SpoiltLong &s) { s.D = 0; });
    invalid_long(l, "d = 2 with null t_add", L_APPENDING, [](SpoiltLong &s) { s.null_t_add = true; });
    invalid_long(l, "d = 2 with null y_add", L_APPENDING, [](SpoiltLong &s) { s.null_y_add = true; });
    invalid_long(l, "tail + d + 1 = NGP_MAX_AUX + 1", L_APPENDING, [=](SpoiltLong &s) { s.d = d_over; });
    invalid_long(l, "null w", L_SAMPLE, [](SpoiltLong &s) { s.null_w = true; });
    invalid_long(l, "draws = 0", L_SAMPLE, [](SpoiltLong &s) { s.draws = 0; });
    invalid_long(l, "D draws = 2^31", L_SAMPLE, [](SpoiltLong &s) { s.D = 2; s.draws = 1 << 30; });
    invalid_long(l, "null counts", L_COMPONENTS, [](SpoiltLong &s) { s.null_counts = true; });
    invalid_long(l, "null components", L_COMPONENTS, [](SpoiltLong &s) { s.null_comps = true; });
    invalid_long(l, "a count of 0", L_COMPONENTS, [](SpoiltLong &s) { s.counts[1] = 0; });
    invalid_long(l, "a count of 65535", L_COMPONENTS, [](SpoiltLong &s) { s.counts[2] = 65535; });
    invalid_long(l, "sigma with 3 m over NGP_MAX_LONG_HORIZON", L_COMPONENTS,
                 [](SpoiltLong &s) { s.with_sigma = true; s.m = NGP_MAX_LONG_HORIZON / 3 + 1; });
    invalid_long(l, "a malformed component", L_COMPONENTS, [](SpoiltLong &s) { s.comps[4] = {1, 0, plus_alone, s.l.par0, 0.0}; });
    invalid_long(l, "null cut", L_ORIGINS, [](SpoiltLong &s) { s.null_cut = true; });
    invalid_long(l, "R = 0", L_ORIGINS, [](SpoiltLong &s) { s.R = 0; });
    invalid_long(l, "R = NGP_MAX_ORIGINS + 1", L_ORIGINS, [](SpoiltLong &s) { s.R = NGP_MAX_ORIGINS + 1; });
    invalid_long(l, "a cut of 0", L_ORIGINS, [](SpoiltLong &s) { s.cut[0] = 0; });
    invalid_long(l, "a cut of n + 1", L_ORIGINS, [](SpoiltLong &s) { s.cut[s.R - 1] = 192; });
    invalid_long(l, "equal cuts", L_ORIGINS, [](SpoiltLong &s) { s.cut[2] = s.cut[1]; });
    // two faults: which status wins
    invalid_long(l, "m = NGP_MAX_LONG_HORIZON + 1 and null mu", L_PREDICT | L_COMPONENTS | L_ORIGINS,
                 [=](SpoiltLong &s) { s.m = over; s.null_mu = true; });
    invalid_long(l, "m = NGP_MAX_LONG_HORIZON + 1 and null var / out / cross / var", L_ALL,
                 [=](SpoiltLong &s) { s.m = over; s.null_second = true; });
    invalid_long(l, "m = NGP_MAX_LONG_HORIZON + 1 and null t_new", L_ALL, [=](SpoiltLong &s) { s.m = over; s.null_t_new = true; });
    invalid_long(l, "m = NGP_MAX_LONG_HORIZON + 1 and d = -1", L_APPENDING, [=](SpoiltLong &s) { s.m = over; s.d = -1; });
    invalid_long(l, "m = NGP_MAX_LONG_HORIZON + 1 and tail + d + 1 = NGP_MAX_AUX + 1", L_APPENDING,
                 [=](SpoiltLong &s) { s.m = over; s.d = d_over; });
    invalid_long(l, "draws = 0 and d = -1", L_SAMPLE, [](SpoiltLong &s) { s.draws = 0; s.d = -1; });
    invalid_long(l, "draws = 0 and tail + d + 1 = NGP_MAX_AUX + 1", L_SAMPLE, [=](SpoiltLong &s) { s.draws = 0; s.d = d_over; });
    invalid_long(l, "draws = 0 and m = NGP_MAX_LONG_HORIZON + 1", L_SAMPLE, [=](SpoiltLong &s) { s.draws = 0; s.m = over; });
    invalid_long(l, "D draws = 2^31 and m = NGP_MAX_LONG_HORIZON + 1", L_SAMPLE,
                 [=](SpoiltLong &s) { s.D = 2; s.draws = 1 << 30; s.m = over; });
    invalid_long(l, "D draws = 2^31 and d = 2 with null y_add", L_SAMPLE,
                 [](SpoiltLong &s) { s.D = 2; s.draws = 1 << 30; s.null_y_add = true; });
    invalid_long(l, "a count of 0 and m = NGP_MAX_LONG_HORIZON + 1", L_COMPONENTS, [=](SpoiltLong &s) { s.counts[1] = 0; s.m = over; });
    invalid_long(l, "a count of 0 and null counts", L_COMPONENTS, [](SpoiltLong &s) { s.counts[1] = 0; s.null_counts = true; });
    invalid_long(l, "a count of 0 and d = -1", L_COMPONENTS, [](SpoiltLong &s) { s.counts[1] = 0; s.d = -1; });
    invalid_long(l, "a count of 0 behind a count of 65535", L_COMPONENTS, [](SpoiltLong &s) { s.counts[0] = 65535; s.counts[1] = 0; });
    invalid_long(l, "a count of 0 and a malformed component", L_COMPONENTS,
                 [](SpoiltLong &s) { s.counts[2] = 0; s.comps[0] = {1, 0, plus_alone, s.l.par0, 0.0}; });
    invalid_long(l, "R = NGP_MAX_ORIGINS + 1 and a cut of 0", L_ORIGINS, [](SpoiltLong &s) { s.R = NGP_MAX_ORIGINS + 1; s.cut[0] = 0; });
    invalid_long(l, "R = NGP_MAX_ORIGINS + 1 and null var", L_ORIGINS, [](SpoiltLong &s) { s.R = NGP_MAX_ORIGINS + 1; s.null_second = true; });
    invalid_long(l, "m = NGP_MAX_LONG_HORIZON + 1 and a cut of 0", L_ORIGINS, [=](SpoiltLong &s) { s.m = over; s.cut[0] = 0; });
    invalid_long(l, "m = NGP_MAX_LONG_HORIZON + 1 and R = NGP_MAX_ORIGINS + 1", L_ORIGINS,
                 [=](SpoiltLong &s) { s.m = over; s.R = NGP_MAX_ORIGINS + 1; });
    done();   // no record: none of them reached the runtime
    l.destroy();
}

// ---- chunks -----------------------------------------------------------------------------------
// A device so small that the three particles of the n = 191 factor go through in two or three chunks:
// the grids and the copies' sizes in the trace show each chunk's size.  The first of a call's two runs
// also checks where the downloads land on the host (Long::cover): every element of the outputs the
// call writes is 0 afterwards, every element around them still holds the sentinel.
// The mock's count kernel writes nothing, so the chunked sampler sees zero counts and draws no path:
// its padding and factorisation per chunk are pinned here, its draw loop is not, and `out` is covered
// by the one final copy only.
extern "C" void mock_hip_set_device_bytes(size_t bytes);

static void chunked_calls() {
    using oneshot::Long;
    static Long l(191, 300);
    const size_t um = (size_t)l.m, P = Long::P, D = Long::D;
    struct Case {
        const char *name;
        size_t device_bytes;
        std::function<ngp_status()> call;
        std::vector<Long::Span> written;
    };
    const Case cases[] = {
        {"ngp_factor_predict_long d=0 sigma", (size_t)4 << 20, [] { return l.predict_long(false, true); },
         {{l.mu, P * um}, {l.var, P * um}, {l.sigma, P * um * um}, {l.info, P}}},
        {"ngp_factor_predict_long d=2 D=3", (size_t)2 << 20, [] { return l.predict_long(true, false); },
         {{l.mu, P * D * um}, {l.var, P * um}, {l.info, P}}},
        {"ngp_factor_sample_long d=2 D=3", (size_t)4 << 20, [] { return l.sample_long(true); },
         {{l.out, D * l.draws * um}, {l.comp, D * (size_t)l.draws}, {l.mu, P * D * um}, {l.var, P * um}, {l.info, P}, {l.cinfo, P}}},
        {"ngp_factor_components_long d=2 D=3 sigma", (size_t)24 << 20, [] { return l.components_long(true, true); },
         {{l.mu, Long::NC * D * um}, {l.cross, Long::NC2 * um}, {l.sigma, Long::NC2 * um * um}, {l.info, P}}},
        {"ngp_factor_components_long d=0", (size_t)4 << 20, [] { return l.components_long(false, false); },
         {{l.mu, (size_t)Long::NC * um}, {l.cross, Long::NC2 * um}, {l.info, P}}},
        {"ngp_factor_predict_origins logml", (size_t)1 << 20, [] { return l.predict_origins(true); },
         {{l.mu, P * l.R * um}, {l.var, P * l.R * um}, {l.logml, P * (size_t)l.R}, {l.info, P}}},
    };
    for (const Case &c : cases) {
        mock_hip_set_device_bytes(c.device_bytes);
        ngp_ctx *ctx = nullptr;
        if (ngp_ctx_create(0, &ctx) != NGP_OK) { ++fails; say("FAIL no context"); return; }
        OK(ngp_set_combining(ctx, 0));
        OK(ngp_profile_enable(ctx, 1));
        say("-- setup of chunked %s on %zu KiB", c.name, c.device_bytes >> 10);
        OK(l.create(ctx));
        done();
        for (int rep = 0; rep < 2; ++rep) {
            say("== chunked %s", c.name);
            ngp_status st = NGP_OK;
            const long bad = rep ? (st = c.call(), 0) : l.cover(c.call, c.written, &st);
            OK(st);
            if (bad) { ++fails; say("FAIL %ld output elements not written or guard elements overwritten", bad); }
            done();
        }
        l.destroy();
        ngp_ctx_destroy(ctx);
    }
    mock_hip_set_device_bytes((size_t)2 << 30);
}

int main(int argc, char **argv) {
    full = argc > 1 && std::string(argv[1]) == "--full";
    mock_hip_trace(full ? 1 : 2);
    ngp_ctx *ctx = nullptr;
    if (ngp_ctx_create(0, &ctx) != NGP_OK) { say("FAIL no context"); return 2; }
    OK(ngp_set_combining(ctx, 0));
    OK(ngp_profile_enable(ctx, 1));
    std::vector<oneshot::Entry> calls = oneshot::table();
    for (const oneshot::Entry &e : oneshot::long_table()) calls.push_back(e);
    for (const oneshot::Entry &e : calls) {
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
    invalid_long_calls(ctx);
    ngp_ctx_destroy(ctx);
    chunked_calls();
    if (mock_hip_errors()) { ++fails; say("FAIL the mock runtime saw a bad free or an out-of-bounds copy"); }
    if (mock_hip_live_allocations()) { ++fails; say("FAIL device allocations left after the context was destroyed"); }
    say("oneshot_trace: %d failures", fails);
    return fails ? 1 : 0;
}

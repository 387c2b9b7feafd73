// The trajectory targets (ngp_mixture_path_targets / _indep) against the mock HIP runtime (see
// mock_hip.cpp): three threads on one context call both entry points with good and bad arguments,
// every status checked.  Built with -fsanitize=address,undefined by
// tests/test_path_targets_sanitizers.py; exit code 0 and a silent sanitizer are the test.  (The
// mock's kernels do nothing: values are not looked at, except where the HOST writes them — the NaN
// of q for the kinds that have no quantiles; device blocks are reused between calls, so what the
// absent kernels would have written is whatever an earlier call left.)
#include <atomic>
#include <cmath>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../include/ngp.h"

extern "C" long mock_hip_launches(void);
extern "C" long mock_hip_live_allocations(void);
extern "C" long mock_hip_errors(void);

static std::atomic<int> fails{0};
#define CHECK(c, what) do { if (!(c)) { ++fails; std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, what); } } while (0)

struct Call {
    int P, S, m, draws, T, Q;
    std::vector<double> w, mu, sigma, sigma_indep, mu_indep, probs, q, mean, values;
    std::vector<uint64_t> seeds;
    std::vector<ngp_path_target> tg;
    std::vector<int64_t> count, hist;
    std::vector<int32_t> info;
    ngp_inv_transform inv;
    Call(int id) : P(3 + id), S(2 + id), m(5 + 30 * id), draws(40 + id), T(5 + id), Q(7 + id) {
        w.assign((size_t)S * P, 1.0 / P);
        mu.assign((size_t)P * S * m, 0.5);
        mu_indep = mu;
        sigma.assign((size_t)P * m * m, 0.0);
        for (int k = 0; k < P; ++k)
            for (int j = 0; j < m; ++j) sigma[((size_t)k * m + j) * m + j] = 0.04;
        sigma_indep.assign((size_t)S * P * m * m, 0.0);
        for (size_t k = 0; k < (size_t)S * P; ++k)
            for (int j = 0; j < m; ++j) sigma_indep[(k * m + j) * m + j] = 0.04;
        seeds.assign(S, 7u);
        for (int t = 0; t < T; ++t) tg.push_back(ngp_path_target{t % 5, t % m, m - 1, 1.5});
        for (int i = 0; i < Q; ++i) probs.push_back((i + 1.0) / (Q + 1.0));
        probs[Q - 1] = probs[0];                    // a repeated level
        q.assign((size_t)T * Q, -1.0);
        mean.assign(T, -1.0);
        count.assign(T, -1);
        hist.assign((size_t)T * m, -1);
        values.assign((size_t)T * S * draws, -1.0);
        info.assign((size_t)S * P, -1);
        inv = ngp_inv_transform{NGP_INV_BOXCOX, -0.3, 0.25, 1.0e4};
    }
    ngp_status shared(ngp_ctx *c, double *vals) {
        return ngp_mixture_path_targets(c, P, S, m, w.data(), mu.data(), sigma.data(), draws, 11u, &inv, T,
                                        tg.data(), Q, probs.data(), q.data(), mean.data(), count.data(),
                                        hist.data(), vals, info.data());
    }
    ngp_status indep(ngp_ctx *c, const uint64_t *sd) {
        return ngp_mixture_path_targets_indep(c, P, S, m, w.data(), mu_indep.data(), sigma_indep.data(),
                                              draws, sd, &inv, T, tg.data(), Q, probs.data(), q.data(),
                                              mean.data(), count.data(), hist.data(), nullptr, nullptr);
    }
};

static void worker(ngp_ctx *ctx, int id, int rounds) {
    Call a(id);
    for (int r = 0; r < rounds; ++r) {
        CHECK(a.shared(ctx, a.values.data()) == NGP_OK, "path_targets");
        CHECK(a.shared(ctx, nullptr) == NGP_OK, "path_targets without values");
        CHECK(a.indep(ctx, a.seeds.data()) == NGP_OK, "path_targets_indep");
        for (int t = 0; t < a.T; ++t)
            if (a.tg[t].kind > NGP_TARGET_DIFF) CHECK(std::isnan(a.q[(size_t)t * a.Q + a.Q - 1]), "quantiles of a kind that has none");
        // malformed calls: refused, nothing left behind
        CHECK(a.shared(nullptr, nullptr) == NGP_ERR_ARG, "null context accepted");
        CHECK(a.indep(ctx, nullptr) == NGP_ERR_ARG, "null seeds accepted");
#define REFUSED(change, status, what) do { Call x(id); change; CHECK(x.shared(ctx, nullptr) == status, what); } while (0)
        REFUSED(x.T = 0, NGP_ERR_ARG, "T = 0 accepted");
        REFUSED(x.Q = 0, NGP_ERR_ARG, "Q = 0 accepted");
        REFUSED(x.draws = 0, NGP_ERR_ARG, "draws = 0 accepted");
        REFUSED(x.m = 0, NGP_ERR_ARG, "m = 0 accepted");
        REFUSED(x.tg[1].j1 = x.m, NGP_ERR_ARG, "window beyond m accepted");
        REFUSED(x.tg[1].j0 = -1, NGP_ERR_ARG, "negative window start accepted");
        REFUSED((x.tg[2].j0 = 3, x.tg[2].j1 = 2), NGP_ERR_ARG, "j0 > j1 accepted");
        REFUSED(x.tg[0].kind = 5, NGP_ERR_ARG, "unknown target kind accepted");
        REFUSED(x.tg[0].kind = -1, NGP_ERR_ARG, "negative target kind accepted");
        REFUSED(x.tg[4].thr = NAN, NGP_ERR_ARG, "non-finite thr accepted");
        REFUSED(x.probs[2] = (r & 1) ? 1.0 : 0.0, NGP_ERR_ARG, "level outside (0, 1) accepted");
        REFUSED(x.probs[0] = NAN, NGP_ERR_ARG, "NaN level accepted");
        REFUSED(x.inv.kind = 4, NGP_ERR_ARG, "unknown transformation accepted");
        REFUSED(x.inv.lam = INFINITY, NGP_ERR_ARG, "non-finite lam accepted");
        REFUSED(x.inv.offset = NAN, NGP_ERR_ARG, "non-finite offset accepted");
        REFUSED(x.inv.cap = (r & 1) ? 0.0 : -2.0, NGP_ERR_ARG, "Box-Cox cap <= 0 accepted");
        REFUSED((x.inv.kind = NGP_INV_EXP, x.inv.cap = INFINITY), NGP_ERR_ARG, "non-finite cap accepted");
        REFUSED(x.draws = INT32_MAX, NGP_ERR_TOO_LARGE, "N beyond 2^31 - 1 accepted");
        {
            Call x(id);     // limits: 65 targets, 65 levels, more dates than NGP_MAX_AUX
            x.tg.assign(65, x.tg[0]);
            x.q.assign((size_t)65 * x.Q, 0.0);
            x.T = 65;
            CHECK(x.shared(ctx, nullptr) == NGP_ERR_TOO_LARGE, "T = 65 accepted");
            Call y(id);
            y.probs.assign(65, 0.5);
            y.Q = 65;
            CHECK(y.shared(ctx, nullptr) == NGP_ERR_TOO_LARGE, "Q = 65 accepted");
            Call z(id);
            z.m = NGP_MAX_AUX + 1;          // refused before any array is read
            CHECK(z.shared(ctx, nullptr) == NGP_ERR_TOO_LARGE, "m beyond NGP_MAX_AUX accepted");
        }
        {
            Call x(id);     // null arrays
            CHECK(ngp_mixture_path_targets(ctx, x.P, x.S, x.m, x.w.data(), x.mu.data(), x.sigma.data(), x.draws, 1u,
                                           nullptr, x.T, x.tg.data(), x.Q, x.probs.data(), x.q.data(), x.mean.data(),
                                           x.count.data(), x.hist.data(), nullptr, nullptr) == NGP_ERR_ARG, "null inv accepted");
            CHECK(ngp_mixture_path_targets(ctx, x.P, x.S, x.m, x.w.data(), x.mu.data(), x.sigma.data(), x.draws, 1u,
                                           &x.inv, x.T, nullptr, x.Q, x.probs.data(), x.q.data(), x.mean.data(),
                                           x.count.data(), x.hist.data(), nullptr, nullptr) == NGP_ERR_ARG, "null targets accepted");
            CHECK(ngp_mixture_path_targets(ctx, x.P, x.S, x.m, x.w.data(), nullptr, x.sigma.data(), x.draws, 1u,
                                           &x.inv, x.T, x.tg.data(), x.Q, x.probs.data(), x.q.data(), x.mean.data(),
                                           x.count.data(), x.hist.data(), nullptr, nullptr) == NGP_ERR_ARG, "null means accepted");
            CHECK(ngp_mixture_path_targets(ctx, x.P, x.S, x.m, x.w.data(), x.mu.data(), x.sigma.data(), x.draws, 1u,
                                           &x.inv, x.T, x.tg.data(), x.Q, x.probs.data(), x.q.data(), x.mean.data(),
                                           nullptr, x.hist.data(), nullptr, nullptr) == NGP_ERR_ARG, "null count accepted");
        }
    }
}

int main() {
    ngp_ctx *ctx = nullptr;
    if (ngp_ctx_create(0, &ctx) != NGP_OK) return 2;
    const int T = 3, rounds = 4;
    std::vector<std::thread> th;
    for (int i = 0; i < T; ++i) th.emplace_back(worker, ctx, i, rounds);
    for (auto &t : th) t.join();
    ngp_ctx_destroy(ctx);
    CHECK(mock_hip_errors() == 0, "bad free / out-of-bounds copy seen by the mock runtime");
    CHECK(mock_hip_live_allocations() == 0, "device allocations left after the context was destroyed");
    std::printf("path_targets_stress: %ld kernel launches issued, %d failures\n", mock_hip_launches(), fails.load());
    return fails.load() ? 1 : 0;
}

// The path scores (ngp_ensemble_scores / ngp_mixture_path_scores) against the mock HIP runtime (see
// mock_hip.cpp): three threads on one context call both entry points with good and bad arguments,
// every status checked — validation, limits, staging of shapes around the tile and slice edges,
// and the blocks given back on every error return.  Built with -fsanitize=address,undefined by
// tests/test_ensemble_scores_sanitizers.py; exit code 0 and a silent sanitizer are the test.  (The
// mock's kernels do nothing: the totals read back are whatever zeroed or reused device memory
// holds, so values are looked at only where the HOST decides them — a one-path V-statistic's pair
// divisor, NULL outputs left alone.)
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

struct Ens {
    int N, m, W, scale, fair;
    double shift;
    std::vector<double> x, y, es, to, tp;
    std::vector<int32_t> win, info;
    Ens(int N_, int m_) : N(N_), m(m_), scale(NGP_SCORE_LOG), fair(N_ > 1), shift(0.5) {
        x.assign((size_t)N * m, 2.0);
        y.assign(m, 1.5);
        for (int j = 0; j < m; ++j) { win.push_back(j); win.push_back(j); }
        win.push_back(0); win.push_back(m - 1);
        win.push_back(m / 2); win.push_back(m - 1);
        W = (int)win.size() / 2;
        es.assign(W, -1.0); to.assign(W, -1.0); tp.assign(W, -1.0);
        info.assign(W, -7);
    }
    ngp_status run(ngp_ctx *c, bool all_outputs = true) {
        return ngp_ensemble_scores(c, N, m, x.data(), y.data(), scale, shift, fair, W, win.data(), es.data(),
                                   all_outputs ? to.data() : nullptr, all_outputs ? tp.data() : nullptr,
                                   all_outputs ? info.data() : nullptr);
    }
};

struct Mix {
    int P, S, m, draws, indep, W, scale, fair;
    double shift;
    std::vector<double> w, mu, sigma, y, es, to, tp;
    std::vector<uint64_t> seeds;
    std::vector<int32_t> win, info, cinfo;
    ngp_inv_transform inv;
    Mix(int id, int indep_) : P(2 + id), S(2 + id), m(4 + 40 * id), draws(50 + 40 * id), indep(indep_),
                              scale(NGP_SCORE_NATURAL), fair(1), shift(0.0) {
        const size_t mats = indep ? (size_t)S * P : (size_t)P;
        w.assign((size_t)S * P, 1.0 / P);
        mu.assign((size_t)S * P * m, 0.5);
        sigma.assign(mats * m * m, 0.0);
        for (size_t k = 0; k < mats; ++k)
            for (int j = 0; j < m; ++j) sigma[(k * m + j) * m + j] = 0.04;
        seeds.assign(S, 7u);
        y.assign(m, 1.0);
        win = {0, 0, 0, m - 1, 1, m - 2, 0, m - 1};
        W = 4;
        es.assign(W, -1.0); to.assign(W, -1.0); tp.assign(W, -1.0);
        info.assign(W, -7);
        cinfo.assign(mats, -7);
        inv = ngp_inv_transform{NGP_INV_BOXCOX, 0.3, 0.25, 1.0e4};
    }
    ngp_status run(ngp_ctx *c, bool all_outputs = true) {
        return ngp_mixture_path_scores(c, P, S, m, w.data(), mu.data(), sigma.data(), indep, draws, seeds.data(),
                                       &inv, y.data(), scale, shift, fair, W, win.data(), es.data(),
                                       all_outputs ? to.data() : nullptr, all_outputs ? tp.data() : nullptr,
                                       all_outputs ? info.data() : nullptr, all_outputs ? cinfo.data() : nullptr);
    }
};

static void worker(ngp_ctx *ctx, int id, int rounds) {
    const int shapes[][2] = {{1, 1}, {2, 3}, {127, 1}, {128, 3}, {129, 33}, {257, 3}, {300, 70}};
    for (int r = 0; r < rounds; ++r) {
        for (const auto &sh : shapes) {
            Ens e(sh[0] + id, sh[1] + id);
            CHECK(e.run(ctx) == NGP_OK, "ensemble_scores");
            for (int w = 0; w < e.W; ++w) CHECK(e.info[w] == 0 || e.info[w] == NGP_INFO_NOT_FINITE, "info not written");
            CHECK(e.run(ctx, false) == NGP_OK, "ensemble_scores without the optional outputs");
        }
        {
            Ens e(40 + id, 2100);               // a window beyond 2,048 dates: the two-level distance
            e.win = {0, 2099, 5, 9, 0, 2047};
            e.W = 3;
            CHECK(e.run(ctx) == NGP_OK, "ensemble_scores with a long window");
        }
        for (int indep = 0; indep < 2; ++indep) {
            Mix a(id, indep);
            CHECK(a.run(ctx) == NGP_OK, "mixture_path_scores");
            CHECK(a.cinfo[0] != -7, "chol_info not written");
            CHECK(a.run(ctx, false) == NGP_OK, "mixture_path_scores without the optional outputs");
        }
        // malformed calls: refused, nothing left behind
        CHECK(Ens(5, 3).run(nullptr) == NGP_ERR_ARG, "null context accepted");
        CHECK(Mix(id, 0).run(nullptr) == NGP_ERR_ARG, "null context accepted");
#define REFUSED(T, init, change, status, what) do { T x init; change; CHECK(x.run(ctx) == status, what); } while (0)
        REFUSED(Ens, (5, 3), x.N = 0, NGP_ERR_ARG, "N = 0 accepted");
        REFUSED(Ens, (5, 3), x.m = 0, NGP_ERR_ARG, "m = 0 accepted");
        REFUSED(Ens, (5, 3), x.W = 0, NGP_ERR_ARG, "W = 0 accepted");
        REFUSED(Ens, (5, 3), (x.N = 1, x.fair = 1), NGP_ERR_ARG, "fair with one path accepted");
        REFUSED(Ens, (5, 3), x.fair = 2, NGP_ERR_ARG, "fair = 2 accepted");
        REFUSED(Ens, (5, 3), x.scale = 2, NGP_ERR_ARG, "unknown scale accepted");
        REFUSED(Ens, (5, 3), x.shift = -1.0, NGP_ERR_ARG, "negative shift accepted");
        REFUSED(Ens, (5, 3), x.shift = NAN, NGP_ERR_ARG, "NaN shift accepted");
        REFUSED(Ens, (5, 3), x.win[1] = 3, NGP_ERR_ARG, "window beyond m accepted");
        REFUSED(Ens, (5, 3), x.win[0] = -1, NGP_ERR_ARG, "negative window start accepted");
        REFUSED(Ens, (5, 3), (x.win[6] = 2, x.win[7] = 1), NGP_ERR_ARG, "j0 > j1 accepted");
        REFUSED(Ens, (5, 3), x.y[1] = INFINITY, NGP_ERR_ARG, "non-finite y accepted");
        REFUSED(Ens, (5, 3), x.y[2] = -0.5, NGP_ERR_ARG, "y + shift <= 0 accepted on the log scale");
        // limits: refused before any array is read (the arrays are far smaller than the counts say)
        REFUSED(Ens, (5, 3), x.N = (1 << 20) + 1, NGP_ERR_TOO_LARGE, "N beyond 2^20 accepted");
        REFUSED(Ens, (5, 3), x.W = 4097, NGP_ERR_TOO_LARGE, "W beyond 4,096 accepted");
        REFUSED(Ens, (5, 3), x.m = 65536, NGP_ERR_TOO_LARGE, "m beyond 65,535 accepted");
        REFUSED(Mix, (id, 0), x.m = NGP_MAX_AUX + 1, NGP_ERR_TOO_LARGE, "m beyond NGP_MAX_AUX accepted");
        REFUSED(Mix, (id, 0), x.draws = (1 << 20), NGP_ERR_TOO_LARGE, "S draws beyond 2^20 accepted");
        REFUSED(Mix, (id, 1), x.P = 0, NGP_ERR_ARG, "P = 0 accepted");
        REFUSED(Mix, (id, 1), x.S = 0, NGP_ERR_ARG, "S = 0 accepted");
        REFUSED(Mix, (id, 1), x.draws = 0, NGP_ERR_ARG, "draws = 0 accepted");
        REFUSED(Mix, (id, 1), x.indep = 2, NGP_ERR_ARG, "indep = 2 accepted");
        REFUSED(Mix, (id, 0), x.inv.kind = 4, NGP_ERR_ARG, "unknown transformation accepted");
        REFUSED(Mix, (id, 0), x.inv.lam = INFINITY, NGP_ERR_ARG, "non-finite lam accepted");
        REFUSED(Mix, (id, 0), x.inv.cap = (r & 1) ? 0.0 : -2.0, NGP_ERR_ARG, "Box-Cox cap <= 0 accepted");
        REFUSED(Mix, (id, 0), x.win[3] = x.m, NGP_ERR_ARG, "window beyond m accepted");
        REFUSED(Mix, (id, 0), x.y[0] = NAN, NGP_ERR_ARG, "NaN y accepted");
        {
            Mix x(id, 0);     // null arrays
            CHECK(ngp_mixture_path_scores(ctx, x.P, x.S, x.m, x.w.data(), x.mu.data(), x.sigma.data(), 0, x.draws,
                                          nullptr, &x.inv, x.y.data(), 0, 0.0, 1, x.W, x.win.data(), x.es.data(),
                                          nullptr, nullptr, nullptr, nullptr) == NGP_ERR_ARG, "null seeds accepted");
            CHECK(ngp_mixture_path_scores(ctx, x.P, x.S, x.m, x.w.data(), x.mu.data(), x.sigma.data(), 0, x.draws,
                                          x.seeds.data(), nullptr, x.y.data(), 0, 0.0, 1, x.W, x.win.data(),
                                          x.es.data(), nullptr, nullptr, nullptr, nullptr) == NGP_ERR_ARG, "null inv accepted");
            CHECK(ngp_mixture_path_scores(ctx, x.P, x.S, x.m, x.w.data(), nullptr, x.sigma.data(), 0, x.draws,
                                          x.seeds.data(), &x.inv, x.y.data(), 0, 0.0, 1, x.W, x.win.data(),
                                          x.es.data(), nullptr, nullptr, nullptr, nullptr) == NGP_ERR_ARG, "null means accepted");
            Ens e(5, 3);
            CHECK(ngp_ensemble_scores(ctx, e.N, e.m, nullptr, e.y.data(), 0, 0.0, 1, e.W, e.win.data(), e.es.data(),
                                      nullptr, nullptr, nullptr) == NGP_ERR_ARG, "null paths accepted");
            CHECK(ngp_ensemble_scores(ctx, e.N, e.m, e.x.data(), e.y.data(), 0, 0.0, 1, e.W, e.win.data(), nullptr,
                                      nullptr, nullptr, nullptr) == NGP_ERR_ARG, "null es accepted");
            CHECK(ngp_ensemble_scores(ctx, e.N, e.m, e.x.data(), e.y.data(), 0, 0.0, 1, e.W, nullptr, e.es.data(),
                                      nullptr, nullptr, nullptr) == NGP_ERR_ARG, "null windows accepted");
        }
    }
}

int main() {
    ngp_ctx *ctx = nullptr;
    if (ngp_ctx_create(0, &ctx) != NGP_OK) return 2;
    const int T = 3, rounds = 3;
    std::vector<std::thread> th;
    for (int i = 0; i < T; ++i) th.emplace_back(worker, ctx, i, rounds);
    for (auto &t : th) t.join();
    ngp_ctx_destroy(ctx);
    CHECK(mock_hip_errors() == 0, "bad free / out-of-bounds copy seen by the mock runtime");
    CHECK(mock_hip_live_allocations() == 0, "device allocations left after the context was destroyed");
    std::printf("ensemble_scores_stress: %ld kernel launches issued, %d failures\n", mock_hip_launches(), fails.load());
    return fails.load() ? 1 : 0;
}

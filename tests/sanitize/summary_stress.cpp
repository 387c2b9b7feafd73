// The mixture summaries (ngp_mixture_cdf / _quantiles / _crps) against the mock HIP runtime (see
// mock_hip.cpp): four threads on one context call the three entry points with good and bad
// arguments, every status checked.  Built with -fsanitize=thread and with
// -fsanitize=address,undefined by tests/test_mixture_sanitizers.py; exit code 0 and a silent
// sanitizer are the test.  (The mock's kernels do nothing: values are not looked at, except where
// the HOST writes them — info and the NaN of a bad date.)
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

static void worker(ngp_ctx *ctx, int id, int rounds) {
    const int C = 300 + 77 * id, m = 3 + id, Q = 23, K = 5;   // more than one tile of components
    std::vector<double> w(C), mu((size_t)C * m), var((size_t)C * m), probs(Q), x((size_t)m * K), y(m);
    std::vector<double> q((size_t)m * Q), cdf((size_t)m * K), crps(m);
    std::vector<int32_t> info(m);
    for (int c = 0; c < C; ++c) {
        w[c] = (c % 7 == 3) ? 0.0 : 1.0;
        for (int j = 0; j < m; ++j) {
            mu[(size_t)c * m + j] = 0.3 + 0.01 * ((c * 31 + j * 7) % 53);
            var[(size_t)c * m + j] = 0.01 + 0.001 * ((c + j) % 11);
        }
    }
    double sum = 0.0;
    for (double v : w) sum += v;
    for (double &v : w) v /= sum;
    for (int k = 0; k < Q; ++k) probs[k] = (k + 1.0) / (Q + 1.0);
    for (size_t i = 0; i < x.size(); ++i) x[i] = 0.1 * (double)(i % 9);
    for (int j = 0; j < m; ++j) y[j] = 0.4;
    for (int r = 0; r < rounds; ++r) {
        CHECK(ngp_mixture_cdf(ctx, C, m, w.data(), mu.data(), var.data(), K, x.data(), cdf.data(),
                              info.data()) == NGP_OK, "mixture_cdf");
        CHECK(ngp_mixture_quantiles(ctx, C, m, w.data(), mu.data(), var.data(), Q, probs.data(), q.data(),
                                    info.data()) == NGP_OK, "mixture_quantiles");
        CHECK(ngp_mixture_crps(ctx, C, m, w.data(), mu.data(), var.data(), y.data(), crps.data(),
                               info.data()) == NGP_OK, "mixture_crps");
        for (int j = 0; j < m; ++j) CHECK(info[j] == 0, "clean date flagged");
        // a bad value in one date: reported there and nowhere else, its outputs NaN; the same
        // value under weight zero is ignored (component 3 has weight zero)
        const int bad_c = 4, bad_j = m - 1;
        const double keep = var[(size_t)bad_c * m + bad_j], keep0 = mu[(size_t)3 * m + 0];
        var[(size_t)bad_c * m + bad_j] = (r & 1) ? -1.0 : 0.0;
        mu[(size_t)3 * m + 0] = NAN;
        CHECK(ngp_mixture_crps(ctx, C, m, w.data(), mu.data(), var.data(), y.data(), crps.data(),
                               info.data()) == NGP_OK, "mixture_crps (bad date)");
        for (int j = 0; j < m; ++j) CHECK(info[j] == (j == bad_j ? bad_c + 1 : 0), "info of a bad date");
        CHECK(std::isnan(crps[bad_j]) && !std::isnan(crps[0]), "NaN exactly on the bad date");
        CHECK(ngp_mixture_quantiles(ctx, C, m, w.data(), mu.data(), var.data(), Q, probs.data(), q.data(),
                                    info.data()) == NGP_OK, "mixture_quantiles (bad date)");
        CHECK(info[bad_j] == bad_c + 1 && std::isnan(q[(size_t)bad_j * Q + Q - 1]), "quantiles of a bad date");
        var[(size_t)bad_c * m + bad_j] = keep;
        mu[(size_t)3 * m + 0] = keep0;
        // malformed calls: refused, nothing left behind
        CHECK(ngp_mixture_cdf(nullptr, C, m, w.data(), mu.data(), var.data(), K, x.data(), cdf.data(),
                              info.data()) == NGP_ERR_ARG, "null context accepted");
        CHECK(ngp_mixture_cdf(ctx, C, m, w.data(), mu.data(), var.data(), 0, x.data(), cdf.data(),
                              info.data()) == NGP_ERR_ARG, "K = 0 accepted");
        CHECK(ngp_mixture_cdf(ctx, 0, m, w.data(), mu.data(), var.data(), K, x.data(), cdf.data(),
                              info.data()) == NGP_ERR_ARG, "C = 0 accepted");
        CHECK(ngp_mixture_crps(ctx, C, -1, w.data(), mu.data(), var.data(), y.data(), crps.data(),
                               info.data()) == NGP_ERR_ARG, "m < 0 accepted");
        CHECK(ngp_mixture_crps(ctx, C, m, w.data(), nullptr, var.data(), y.data(), crps.data(),
                               info.data()) == NGP_ERR_ARG, "null means accepted");
        const double p_keep = probs[2];
        probs[2] = (r & 1) ? 1.0 : 0.0;
        CHECK(ngp_mixture_quantiles(ctx, C, m, w.data(), mu.data(), var.data(), Q, probs.data(), q.data(),
                                    info.data()) == NGP_ERR_ARG, "level outside (0, 1) accepted");
        probs[2] = p_keep;
        const double w_keep = w[0];
        w[0] = (r & 1) ? -0.5 : NAN;
        CHECK(ngp_mixture_cdf(ctx, C, m, w.data(), mu.data(), var.data(), K, x.data(), cdf.data(),
                              info.data()) == NGP_ERR_ARG, "bad weight accepted");
        w[0] = w_keep;
        std::vector<double> zero(C, 0.0);
        CHECK(ngp_mixture_crps(ctx, C, m, zero.data(), mu.data(), var.data(), y.data(), crps.data(),
                               info.data()) == NGP_ERR_ARG, "all-zero weights accepted");
        CHECK(ngp_mixture_cdf(ctx, 70000, m, w.data(), mu.data(), var.data(), K, x.data(), cdf.data(),
                              info.data()) == NGP_ERR_TOO_LARGE, "C beyond the limit accepted");
        double rate = 0.0;
        CHECK(ngp_microbench_mixture_pairs(ctx, 16, &rate) == NGP_OK, "microbench_mixture_pairs");
        CHECK(ngp_microbench_mixture_pairs(ctx, 0, &rate) == NGP_ERR_ARG, "iters = 0 accepted");
    }
}

int main() {
    ngp_ctx *ctx = nullptr;
    if (ngp_ctx_create(0, &ctx) != NGP_OK) return 2;
    const int T = 4, rounds = 6;
    std::vector<std::thread> th;
    for (int i = 0; i < T; ++i) th.emplace_back(worker, ctx, i, rounds);
    for (auto &t : th) t.join();
    ngp_ctx_destroy(ctx);
    CHECK(mock_hip_errors() == 0, "bad free / out-of-bounds copy seen by the mock runtime");
    CHECK(mock_hip_live_allocations() == 0, "device allocations left after the context was destroyed");
    std::printf("summary_stress: %ld kernel launches issued, %d failures\n", mock_hip_launches(), fails.load());
    return fails.load() ? 1 : 0;
}

// The host code of ngp_factor_predict_origins (argument checks, limits, the cuts' way to the device,
// chunking of the particles by what the device holds, the context's lock) against the mock HIP
// runtime (see mock_hip.cpp): good and bad arguments, every limit at exactly the bound and one over,
// a device so small that the particles go through in several chunks, and two threads querying ONE
// factor.  Built with -fsanitize=thread and with -fsanitize=address,undefined by
// tests/test_predict_origins_sanitizers.py; exit code 0 and a silent sanitizer are the test.  (The
// mock's kernels do nothing: values are not looked at.  (n mod 64) + 1 never exceeds NGP_MAX_AUX, so
// that refusal has no case.)
#include <atomic>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <thread>
#include <vector>

#include "../../include/ngp.h"

extern "C" long mock_hip_launches(void);
extern "C" long mock_hip_live_allocations(void);
extern "C" long mock_hip_errors(void);
extern "C" void mock_hip_set_device_bytes(size_t bytes);

static std::atomic<int> fails{0};
#define CHECK(c, what) do { if (!(c)) { ++fails; std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, what); } } while (0)

// Plus(Plus(Linear, Periodic), SqExp) | Times(Plus(Linear, Periodic), SqExp) |
// Plus(ChangePoint(Plus(SqExp, Constant), Periodic), GammaExp)
struct Ensemble {
    int32_t ops0[5] = {2, 5, 6, 3, 6}, ops1[5] = {2, 5, 6, 3, 7}, ops2[7] = {3, 1, 6, 5, 8, 4, 6};
    double par0[8] = {0.2, 0.1, 0.5, 0.9, 0.3, 0.7, 0.21, 0.4};
    double par1[8] = {0.1, 0.3, 0.8, 1.1, 0.21, 0.4, 0.3, 0.6};
    double par2[11] = {0.2, 0.5, 0.25, 1.0, 0.3, 0.3, 0.5, 0.1, 0.3, 1.5, 0.2};
    ngp_kernel ks[3];
    Ensemble() {
        ks[0] = {5, 8, ops0, par0, 0.05};
        ks[1] = {5, 8, ops1, par1, 0.02};
        ks[2] = {7, 11, ops2, par2, 0.1};
    }
};
constexpr int P = 3;

struct Series {
    std::vector<double> t, y;
    explicit Series(int n) : t(n), y(n) {
        for (int i = 0; i < n; ++i) { t[i] = (double)i / 200; y[i] = std::sin(9.0 * t[i]); }
    }
};

static std::vector<double> after(double t0, int first, int count) {
    std::vector<double> v(count);
    for (int i = 0; i < count; ++i) v[i] = t0 + (double)(first + i) / 200;
    return v;
}

static ngp_factor *make_factor(ngp_ctx *ctx, const Ensemble &e, const Series &s) {
    ngp_factor *f = nullptr;
    CHECK(ngp_factor_create(ctx, 3, e.ks, (int)s.t.size(), s.t.data(), s.y.data(), 0, &f) == NGP_OK && f,
          "factor_create");
    return f;
}

struct Out {
    std::vector<double> mu, var, logml;
    std::vector<int32_t> info;
    Out(int R, int m) : mu((size_t)P * R * m), var((size_t)P * R * m), logml((size_t)P * R), info(P) {}
};

static void arguments_and_limits(ngp_ctx *ctx) {
    Ensemble e;
    const int n = 191, m = 40;                     // tail 63, a main block of 128
    Series s(n);
    ngp_factor *f = make_factor(ctx, e, s);
    if (!f) return;
    const std::vector<double> t_new = after(s.t[n - 1], -8, m);
    const int32_t cuts[8] = {1, 2, 64, 127, 128, 129, 190, 191};
    Out o(8, m);
    const double *tn = t_new.data();
    double *mu = o.mu.data(), *var = o.var.data(), *lm = o.logml.data();
    int32_t *info = o.info.data();
    auto call = ngp_factor_predict_origins;
    CHECK(call(f, 8, cuts, m, tn, 1, mu, var, lm, info) == NGP_OK, "origins either side of every boundary");
    CHECK(call(f, 8, cuts, m, tn, 0, mu, var, nullptr, nullptr) == NGP_OK, "logml and info may be null");
    CHECK(call(f, 5, cuts, m, tn, 1, mu, var, lm, info) == NGP_OK, "origins in the main block alone");
    CHECK(call(f, 3, cuts + 5, m, tn, 1, mu, var, lm, info) == NGP_OK, "origins in the tail alone");
    CHECK(call(nullptr, 8, cuts, m, tn, 1, mu, var, lm, info) == NGP_ERR_ARG, "null factor accepted");
    CHECK(call(f, 8, nullptr, m, tn, 1, mu, var, lm, info) == NGP_ERR_ARG, "null cuts accepted");
    CHECK(call(f, 8, cuts, m, nullptr, 1, mu, var, lm, info) == NGP_ERR_ARG, "null dates accepted");
    CHECK(call(f, 8, cuts, m, tn, 1, nullptr, var, lm, info) == NGP_ERR_ARG, "null means accepted");
    CHECK(call(f, 8, cuts, m, tn, 1, mu, nullptr, lm, info) == NGP_ERR_ARG, "null variances accepted");
    CHECK(call(f, 0, cuts, m, tn, 1, mu, var, lm, info) == NGP_ERR_ARG, "R = 0 accepted");
    CHECK(call(f, -1, cuts, m, tn, 1, mu, var, lm, info) == NGP_ERR_ARG, "R < 0 accepted");
    CHECK(call(f, 8, cuts, 0, tn, 1, mu, var, lm, info) == NGP_ERR_ARG, "m = 0 accepted");
    // a cut at n and one over, at 1 and one under, equal and descending cuts
    const int32_t last[1] = {n}, over[1] = {n + 1}, zero[1] = {0}, eq[3] = {5, 70, 70}, desc[3] = {5, 70, 69};
    CHECK(call(f, 1, last, m, tn, 1, mu, var, lm, info) == NGP_OK, "cut = n refused");
    CHECK(call(f, 1, over, m, tn, 1, mu, var, lm, info) == NGP_ERR_ARG, "cut = n + 1 accepted");
    CHECK(call(f, 1, zero, m, tn, 1, mu, var, lm, info) == NGP_ERR_ARG, "cut = 0 accepted");
    CHECK(call(f, 3, eq, m, tn, 1, mu, var, lm, info) == NGP_ERR_ARG, "equal cuts accepted");
    CHECK(call(f, 3, desc, m, tn, 1, mu, var, lm, info) == NGP_ERR_ARG, "descending cuts accepted");
    // the horizon at the bound and one over
    const int m_max = NGP_MAX_LONG_HORIZON;
    const std::vector<double> t_far = after(s.t[n - 1], 1, m_max + 1);
    {
        Out far(2, m_max + 1);
        CHECK(call(f, 2, cuts + 3, m_max, t_far.data(), 1, far.mu.data(), far.var.data(), lm, info) == NGP_OK, "the longest horizon refused");
        CHECK(call(f, 2, cuts + 3, m_max + 1, t_far.data(), 1, far.mu.data(), far.var.data(), lm, info) == NGP_ERR_TOO_LARGE, "one date over the limit accepted");
    }
    ngp_factor_destroy(f);
    // the origins at the bound and one over: every count of a series of 1,100 but the last 76 / 75
    {
        const int nl = 1100, r_max = NGP_MAX_ORIGINS;
        Series sl(nl);
        ngp_factor *g = make_factor(ctx, e, sl);
        if (g) {
            std::vector<int32_t> all(r_max + 1);
            std::iota(all.begin(), all.end(), 1);
            Out big(r_max + 1, 3);
            CHECK(call(g, r_max, all.data(), 3, t_far.data(), 1, big.mu.data(), big.var.data(), big.logml.data(), info) == NGP_OK, "the most origins refused");
            CHECK(call(g, r_max + 1, all.data(), 3, t_far.data(), 1, big.mu.data(), big.var.data(), big.logml.data(), info) == NGP_ERR_TOO_LARGE, "one origin over the limit accepted");
            ngp_factor_destroy(g);
        }
    }
    // no main block at all (n < 64), and a series that is all main block
    for (int ns : {20, 128}) {
        Series ss(ns);
        ngp_factor *g = make_factor(ctx, e, ss);
        if (g) {
            const int32_t c3[3] = {1, ns / 2, ns};
            const std::vector<double> t3 = after(ss.t[ns - 1], -5, 300);
            Out o3(3, 300);
            CHECK(call(g, 3, c3, 300, t3.data(), 1, o3.mu.data(), o3.var.data(), o3.logml.data(), info) == NGP_OK, "a series without a main block or without a tail");
            ngp_factor_destroy(g);
        }
    }
}

// a device that holds one or two particles' working storage: the particles go through in chunks
static void chunking() {
    mock_hip_set_device_bytes((size_t)8 << 20);
    ngp_ctx *ctx = nullptr;
    if (ngp_ctx_create(0, &ctx) != NGP_OK) { ++fails; return; }
    Ensemble e;
    const int n = 191, m = 1000, R = 50;
    Series s(n);
    ngp_factor *f = make_factor(ctx, e, s);
    if (f) {
        const std::vector<double> t_new = after(s.t[n - 1], 1, m);
        std::vector<int32_t> cuts(R);
        std::iota(cuts.begin(), cuts.end(), 60);
        Out o(R, m);
        const long before = mock_hip_launches();
        CHECK(ngp_factor_predict_origins(f, R, cuts.data(), m, t_new.data(), 1, o.mu.data(), o.var.data(),
                                         o.logml.data(), o.info.data()) == NGP_OK,
              "a large P refused on a small device");
        // eight per chunk: fill, small blocks, solve, origins of the main block, products,
        // conditioning block, origins of the tail, evidence
        const long launches = mock_hip_launches() - before;
        CHECK(launches % 8 == 0 && launches > 8, "the particles did not go through in chunks");
        ngp_factor_destroy(f);
    }
    ngp_ctx_destroy(ctx);
    mock_hip_set_device_bytes((size_t)2 << 30);
}

static void query_loop(ngp_factor *f, double t_last, int id, int rounds) {
    const int m = 100 + 17 * id, R = 5 + id;
    const std::vector<double> t_new = after(t_last, -3, m);
    std::vector<int32_t> cuts(R);
    for (int r = 0; r < R; ++r) cuts[r] = 20 + 25 * r + id;
    Out o(R, m);
    for (int r = 0; r < rounds; ++r) {
        CHECK(ngp_factor_predict_origins(f, R, cuts.data(), m, t_new.data(), r & 1, o.mu.data(), o.var.data(),
                                         (r + id) & 1 ? o.logml.data() : nullptr, o.info.data()) == NGP_OK,
              "concurrent query");
        std::vector<double> mu((size_t)P * m), var((size_t)P * m);
        CHECK(ngp_factor_predict_long(f, 0, nullptr, 1, nullptr, m, t_new.data(), 0, mu.data(), var.data(),
                                      nullptr, o.info.data()) == NGP_OK, "the long query beside it");
    }
}

int main() {
    ngp_ctx *ctx = nullptr;
    if (ngp_ctx_create(0, &ctx) != NGP_OK) return 2;
    arguments_and_limits(ctx);
    {   // two threads, one factor
        Ensemble e;
        Series s(150);
        ngp_factor *f = make_factor(ctx, e, s);
        if (f) {
            std::thread a(query_loop, f, s.t[149], 0, 6), b(query_loop, f, s.t[149], 1, 6);
            a.join();
            b.join();
            ngp_factor_destroy(f);
        }
    }
    ngp_ctx_destroy(ctx);
    chunking();
    CHECK(mock_hip_errors() == 0, "bad free / out-of-bounds copy seen by the mock runtime");
    CHECK(mock_hip_live_allocations() == 0, "device allocations left after the context was destroyed");
    std::printf("predict_origins_stress: %ld kernel launches issued, %d failures\n", mock_hip_launches(), fails.load());
    return fails.load() ? 1 : 0;
}

// The host code of ngp_factor_predict_long (argument checks, limits, staging of the panel's inputs,
// chunking of the particles by what the device holds, the context's lock) against the mock HIP
// runtime (see mock_hip.cpp): good and bad arguments, the limits at exactly the bound and one over,
// a device so small that the particles go through in several chunks, and two threads querying ONE
// factor.  Built with -fsanitize=thread and with -fsanitize=address,undefined by
// tests/test_predict_long_sanitizers.py; exit code 0 and a silent sanitizer are the test.  (The
// mock's kernels do nothing: values are not looked at.)
#include <atomic>
#include <cmath>
#include <cstdio>
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

static ngp_factor *make_factor(ngp_ctx *ctx, const Ensemble &e, const Series &s, bool per_item_y) {
    const int n = (int)s.t.size();
    std::vector<double> Y;
    if (per_item_y)
        for (int p = 0; p < 3; ++p) for (int i = 0; i < n; ++i) Y.push_back((p + 1) * s.y[i]);
    ngp_factor *f = nullptr;
    CHECK(ngp_factor_create(ctx, 3, e.ks, n, s.t.data(), per_item_y ? Y.data() : s.y.data(),
                            per_item_y ? n : 0, &f) == NGP_OK && f, "factor_create");
    return f;
}

static void arguments_and_limits(ngp_ctx *ctx) {
    Ensemble e;
    const int P = 3, n = 191, m = 40;             // tail 63, one main block row of 128
    Series s(n);
    ngp_factor *f = make_factor(ctx, e, s, false);
    if (!f) return;
    const std::vector<double> t_new = after(s.t[n - 1], 4, m), t_add = after(s.t[n - 1], 1, 3);
    const std::vector<double> y_add = {0.1, 0.2, 0.3, -0.1, -0.2, -0.3};   // D = 2, d = 3
    std::vector<double> mu(P * 2 * m), var(P * m), sg((size_t)P * m * m);
    std::vector<int32_t> info(P);
    auto call = [&](ngp_factor *ff, int d, const double *ta, int D, const double *ya, int mm,
                    const double *tn, double *pmu, double *pvar, double *psg, int32_t *pinfo) {
        return ngp_factor_predict_long(ff, d, ta, D, ya, mm, tn, 1, pmu, pvar, psg, pinfo);
    };
    CHECK(call(f, 3, t_add.data(), 2, y_add.data(), m, t_new.data(), mu.data(), var.data(), sg.data(), info.data()) == NGP_OK, "nowcast form");
    CHECK(call(f, 0, nullptr, 0, nullptr, m, t_new.data(), mu.data(), var.data(), sg.data(), info.data()) == NGP_OK, "d = 0 ignores D, t_add, y_add");
    CHECK(call(f, 0, nullptr, 1, nullptr, m, t_new.data(), mu.data(), var.data(), nullptr, nullptr) == NGP_OK, "sigma and info may be null");
    CHECK(call(nullptr, 0, nullptr, 1, nullptr, m, t_new.data(), mu.data(), var.data(), sg.data(), info.data()) == NGP_ERR_ARG, "null factor accepted");
    CHECK(call(f, 0, nullptr, 1, nullptr, m, nullptr, mu.data(), var.data(), sg.data(), info.data()) == NGP_ERR_ARG, "null dates accepted");
    CHECK(call(f, 0, nullptr, 1, nullptr, m, t_new.data(), nullptr, var.data(), sg.data(), info.data()) == NGP_ERR_ARG, "null means accepted");
    CHECK(call(f, 0, nullptr, 1, nullptr, m, t_new.data(), mu.data(), nullptr, sg.data(), info.data()) == NGP_ERR_ARG, "null variances accepted");
    CHECK(call(f, 0, nullptr, 1, nullptr, 0, t_new.data(), mu.data(), var.data(), sg.data(), info.data()) == NGP_ERR_ARG, "m = 0 accepted");
    CHECK(call(f, -1, t_add.data(), 2, y_add.data(), m, t_new.data(), mu.data(), var.data(), sg.data(), info.data()) == NGP_ERR_ARG, "d < 0 accepted");
    CHECK(call(f, 3, t_add.data(), 0, y_add.data(), m, t_new.data(), mu.data(), var.data(), sg.data(), info.data()) == NGP_ERR_ARG, "D = 0 with d > 0 accepted");
    CHECK(call(f, 3, nullptr, 2, y_add.data(), m, t_new.data(), mu.data(), var.data(), sg.data(), info.data()) == NGP_ERR_ARG, "null t_add with d > 0 accepted");
    CHECK(call(f, 3, t_add.data(), 2, nullptr, m, t_new.data(), mu.data(), var.data(), sg.data(), info.data()) == NGP_ERR_ARG, "null y_add with d > 0 accepted");
    // the horizon at the bound and one over (means and variances alone: no m x m array)
    const int m_max = NGP_MAX_LONG_HORIZON;
    const std::vector<double> t_far = after(s.t[n - 1], 1, m_max + 1);
    std::vector<double> mul((size_t)P * (m_max + 1)), varl((size_t)P * (m_max + 1));
    CHECK(call(f, 0, nullptr, 1, nullptr, m_max, t_far.data(), mul.data(), varl.data(), nullptr, info.data()) == NGP_OK, "the longest horizon refused");
    CHECK(call(f, 0, nullptr, 1, nullptr, m_max + 1, t_far.data(), mul.data(), varl.data(), nullptr, info.data()) == NGP_ERR_TOO_LARGE, "one date over the limit accepted");
    // the conditioning block at the bound and one over: tail + d + 1 = 192 / 193
    const int d_fit = NGP_MAX_AUX - n % 64 - 1, d_over = d_fit + 1;
    const std::vector<double> ta_l = after(s.t[n - 1], 1, d_over), ya_l(d_over, 0.25);
    const std::vector<double> tn_l = after(s.t[n - 1], d_over + 1, m);
    CHECK(call(f, d_fit, ta_l.data(), 1, ya_l.data(), m, tn_l.data(), mu.data(), var.data(), sg.data(), info.data()) == NGP_OK, "the largest conditioning block refused");
    CHECK(call(f, d_over, ta_l.data(), 1, ya_l.data(), m, tn_l.data(), mu.data(), var.data(), sg.data(), info.data()) == NGP_ERR_TOO_LARGE, "one appended point over the limit accepted");
    ngp_factor_destroy(f);
    // no main block at all (n < 64), per-item y rows
    Series s20(20);
    ngp_factor *g = make_factor(ctx, e, s20, true);
    if (g) {
        const std::vector<double> tn = after(s20.t[19], 1, 300);
        std::vector<double> mu3((size_t)P * 300), var3((size_t)P * 300), sg3((size_t)P * 300 * 300);
        CHECK(call(g, 0, nullptr, 1, nullptr, 300, tn.data(), mu3.data(), var3.data(), sg3.data(), info.data()) == NGP_OK, "a series without a main block");
        ngp_factor_destroy(g);
    }
}

// a device that holds one or two particles' working storage: the particles go through in chunks
static void chunking() {
    mock_hip_set_device_bytes((size_t)4 << 20);
    ngp_ctx *ctx = nullptr;
    if (ngp_ctx_create(0, &ctx) != NGP_OK) { ++fails; return; }
    Ensemble e;
    const int P = 3, n = 191, m = 300;
    Series s(n);
    ngp_factor *f = make_factor(ctx, e, s, false);
    if (f) {
        const std::vector<double> t_new = after(s.t[n - 1], 1, m);
        std::vector<double> mu((size_t)P * m), var((size_t)P * m), sg((size_t)P * m * m);
        std::vector<int32_t> info(P);
        const long before = mock_hip_launches();
        CHECK(ngp_factor_predict_long(f, 0, nullptr, 1, nullptr, m, t_new.data(), 1, mu.data(), var.data(),
                                      sg.data(), info.data()) == NGP_OK, "a large P refused on a small device");
        const long launches = mock_hip_launches() - before;   // seven per chunk: fill, small, solve, products, three of algebra
        CHECK(launches % 7 == 0 && launches > 7, "the particles did not go through in chunks");
        ngp_factor_destroy(f);
    }
    ngp_ctx_destroy(ctx);
    mock_hip_set_device_bytes((size_t)2 << 30);
}

static void query_loop(ngp_factor *f, double t_last, int id, int rounds) {
    const int P = 3, m = 200 + 17 * id, d = 2;
    const std::vector<double> t_add = after(t_last, 1, d), t_new = after(t_last, d + 1, m);
    const std::vector<double> y_add = {0.1, -0.1, 0.3, 0.2};
    std::vector<double> mu((size_t)P * 2 * m), var((size_t)P * m), sg((size_t)P * m * m);
    std::vector<int32_t> info(P);
    for (int r = 0; r < rounds; ++r) {
        CHECK(ngp_factor_predict_long(f, d, t_add.data(), 2, y_add.data(), m, t_new.data(), r & 1, mu.data(),
                                      var.data(), (r + id) & 1 ? sg.data() : nullptr, info.data()) == NGP_OK,
              "concurrent query");
        std::vector<double> lb(P), lf(P * 2);
        CHECK(ngp_factor_nowcast(f, d, t_add.data(), 2, y_add.data(), 0, nullptr, 1, lb.data(), lf.data(), nullptr,
                                 nullptr, info.data()) == NGP_OK, "the weight update beside it");
    }
}

int main() {
    ngp_ctx *ctx = nullptr;
    if (ngp_ctx_create(0, &ctx) != NGP_OK) return 2;
    arguments_and_limits(ctx);
    {   // two threads, one factor
        Ensemble e;
        Series s(150);
        ngp_factor *f = make_factor(ctx, e, s, false);
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
    std::printf("predict_long_stress: %ld kernel launches issued, %d failures\n", mock_hip_launches(), fails.load());
    return fails.load() ? 1 : 0;
}

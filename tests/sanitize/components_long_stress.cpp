// The host code of ngp_factor_components_long (argument checks, limits, the ragged offsets of the
// outputs, chunking of the particles by what the device holds, the context's lock) against the mock
// HIP runtime (see mock_hip.cpp): good and bad arguments, every limit at exactly the bound and one
// over, a device so small that the particles go through in several chunks, and two threads querying
// ONE factor.  Built with -fsanitize=thread and with -fsanitize=address,undefined by
// tests/test_components_long_sanitizers.py; exit code 0 and a silent sanitizer are the test.  (The
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
// Plus(ChangePoint(Plus(SqExp, Constant), Periodic), GammaExp); the components of a call are
// C_p = 3, 1, 2 programs taken from these arrays (the library does not check that they sum to k)
struct Ensemble {
    int32_t ops0[5] = {2, 5, 6, 3, 6}, ops1[5] = {2, 5, 6, 3, 7}, ops2[7] = {3, 1, 6, 5, 8, 4, 6};
    double par0[8] = {0.2, 0.1, 0.5, 0.9, 0.3, 0.7, 0.21, 0.4};
    double par1[8] = {0.1, 0.3, 0.8, 1.1, 0.21, 0.4, 0.3, 0.6};
    double par2[11] = {0.2, 0.5, 0.25, 1.0, 0.3, 0.3, 0.5, 0.1, 0.3, 1.5, 0.2};
    int32_t lin[1] = {2}, per[1] = {5}, se[1] = {3}, bad_op[1] = {6};
    ngp_kernel ks[3], comps[6];
    int32_t counts[3] = {3, 1, 2};
    Ensemble() {
        ks[0] = {5, 8, ops0, par0, 0.05};
        ks[1] = {5, 8, ops1, par1, 0.02};
        ks[2] = {7, 11, ops2, par2, 0.1};
        comps[0] = {1, 3, lin, par0, 0.0};
        comps[1] = {1, 3, per, par0 + 3, 0.0};
        comps[2] = {1, 2, se, par0 + 6, 0.0};
        comps[3] = ks[1];
        comps[4] = {5, 8, ops2, par2, 0.0};        // ChangePoint(Plus(SqExp, Constant), Periodic)
        comps[5] = {1, 3, ops2 + 5, par2 + 8, 0.0};      // GammaExp
    }
};
constexpr int P = 3, NC = 6, NC2 = 9 + 1 + 4;      // sum C_p, sum C_p^2

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
    std::vector<double> mu, cross, sigma;
    std::vector<int32_t> info;
    Out(int S, int m, bool with_sigma)
        : mu((size_t)NC * S * m), cross((size_t)NC2 * m), sigma(with_sigma ? (size_t)NC2 * m * m : 0), info(P) {}
    double *sg() { return sigma.empty() ? nullptr : sigma.data(); }
};

static void arguments_and_limits(ngp_ctx *ctx) {
    Ensemble e;
    const int n = 191, m = 40;                     // tail 63, one main block row of 128
    Series s(n);
    ngp_factor *f = make_factor(ctx, e, s);
    if (!f) return;
    const std::vector<double> t_new = after(s.t[n - 1], 4, m), t_add = after(s.t[n - 1], 1, 3);
    const std::vector<double> y_add = {0.1, 0.2, 0.3, -0.1, -0.2, -0.3};   // D = 2, d = 3
    Out o(2, m, true);
    auto call = [&](ngp_factor *ff, int d, const double *ta, int D, const double *ya, const int32_t *cnt,
                    const ngp_kernel *ks, int mm, const double *tn, double *pmu, double *pcr, double *psg,
                    int32_t *pinfo) {
        return ngp_factor_components_long(ff, d, ta, D, ya, cnt, ks, mm, tn, pmu, pcr, psg, pinfo);
    };
    const double *ta = t_add.data(), *ya = y_add.data(), *tn = t_new.data();
    double *mu = o.mu.data(), *cr = o.cross.data(), *sg = o.sg();
    int32_t *info = o.info.data();
    CHECK(call(f, 3, ta, 2, ya, e.counts, e.comps, m, tn, mu, cr, sg, info) == NGP_OK, "nowcast form");
    CHECK(call(f, 0, nullptr, 0, nullptr, e.counts, e.comps, m, tn, mu, cr, sg, info) == NGP_OK, "d = 0 ignores D, t_add, y_add");
    CHECK(call(f, 0, nullptr, 1, nullptr, e.counts, e.comps, m, tn, mu, cr, nullptr, nullptr) == NGP_OK, "sigma and info may be null");
    CHECK(call(nullptr, 0, nullptr, 1, nullptr, e.counts, e.comps, m, tn, mu, cr, sg, info) == NGP_ERR_ARG, "null factor accepted");
    CHECK(call(f, 0, nullptr, 1, nullptr, nullptr, e.comps, m, tn, mu, cr, sg, info) == NGP_ERR_ARG, "null counts accepted");
    CHECK(call(f, 0, nullptr, 1, nullptr, e.counts, nullptr, m, tn, mu, cr, sg, info) == NGP_ERR_ARG, "null components accepted");
    CHECK(call(f, 0, nullptr, 1, nullptr, e.counts, e.comps, m, nullptr, mu, cr, sg, info) == NGP_ERR_ARG, "null dates accepted");
    CHECK(call(f, 0, nullptr, 1, nullptr, e.counts, e.comps, m, tn, nullptr, cr, sg, info) == NGP_ERR_ARG, "null means accepted");
    CHECK(call(f, 0, nullptr, 1, nullptr, e.counts, e.comps, m, tn, mu, nullptr, sg, info) == NGP_ERR_ARG, "null cross accepted");
    CHECK(call(f, 0, nullptr, 1, nullptr, e.counts, e.comps, 0, tn, mu, cr, sg, info) == NGP_ERR_ARG, "m = 0 accepted");
    CHECK(call(f, -1, ta, 2, ya, e.counts, e.comps, m, tn, mu, cr, sg, info) == NGP_ERR_ARG, "d < 0 accepted");
    CHECK(call(f, 3, ta, 0, ya, e.counts, e.comps, m, tn, mu, cr, sg, info) == NGP_ERR_ARG, "D = 0 with d > 0 accepted");
    CHECK(call(f, 3, nullptr, 2, ya, e.counts, e.comps, m, tn, mu, cr, sg, info) == NGP_ERR_ARG, "null t_add with d > 0 accepted");
    CHECK(call(f, 3, ta, 2, nullptr, e.counts, e.comps, m, tn, mu, cr, sg, info) == NGP_ERR_ARG, "null y_add with d > 0 accepted");
    const int32_t zero[3] = {3, 0, 2};
    CHECK(call(f, 0, nullptr, 1, nullptr, zero, e.comps, m, tn, mu, cr, sg, info) == NGP_ERR_ARG, "C_p = 0 accepted");
    {
        Ensemble b;
        b.comps[4] = {1, 0, b.bad_op, b.par0, 0.0};     // a Plus without operands
        CHECK(call(f, 0, nullptr, 1, nullptr, b.counts, b.comps, m, tn, mu, cr, sg, info) == NGP_ERR_PROGRAM, "a malformed component accepted");
    }
    // the horizon at the bound and one over, cross alone: nothing (C m)^2 is formed
    const int m_max = NGP_MAX_LONG_HORIZON;
    const std::vector<double> t_far = after(s.t[n - 1], 1, m_max + 1);
    {
        Out far(1, m_max + 1, false);
        CHECK(call(f, 0, nullptr, 1, nullptr, e.counts, e.comps, m_max, t_far.data(), far.mu.data(), far.cross.data(), nullptr, info) == NGP_OK, "the longest horizon refused");
        CHECK(call(f, 0, nullptr, 1, nullptr, e.counts, e.comps, m_max + 1, t_far.data(), far.mu.data(), far.cross.data(), nullptr, info) == NGP_ERR_TOO_LARGE, "one date over the limit accepted");
    }
    // sigma: max C_p m at the bound (the same six programs cut 4 | 1 | 1: 4 x 1,024 = 4,096) and over it
    // (4 x 1,025; 3 x 1,366 = 4,098).  A refused call writes nothing: `one` stands for sigma there.
    {
        const int32_t four[3] = {4, 1, 1};
        const int m4 = 1024, ms = 1366;
        double one = 0.0;
        std::vector<double> mu4((size_t)6 * ms), cr4((size_t)18 * ms), sg4((size_t)18 * m4 * m4);
        CHECK(call(f, 0, nullptr, 1, nullptr, four, e.comps, m4, t_far.data(), mu4.data(), cr4.data(), sg4.data(), info) == NGP_OK, "sigma with C m = 4,096 refused");
        CHECK(call(f, 0, nullptr, 1, nullptr, four, e.comps, m4 + 1, t_far.data(), mu4.data(), cr4.data(), &one, info) == NGP_ERR_TOO_LARGE, "sigma with C m = 4,100 accepted");
        CHECK(call(f, 0, nullptr, 1, nullptr, e.counts, e.comps, ms, t_far.data(), mu4.data(), cr4.data(), &one, info) == NGP_ERR_TOO_LARGE, "sigma with C m = 4,098 accepted");
        CHECK(call(f, 0, nullptr, 1, nullptr, e.counts, e.comps, ms, t_far.data(), mu4.data(), cr4.data(), nullptr, info) == NGP_OK, "the cap of sigma applied without sigma");
    }
    // the conditioning block at the bound and one over: tail + d + 1 = 192 / 193
    const int d_fit = NGP_MAX_AUX - n % 64 - 1, d_over = d_fit + 1;
    const std::vector<double> ta_l = after(s.t[n - 1], 1, d_over), ya_l(d_over, 0.25);
    const std::vector<double> tn_l = after(s.t[n - 1], d_over + 1, m);
    CHECK(call(f, d_fit, ta_l.data(), 1, ya_l.data(), e.counts, e.comps, m, tn_l.data(), mu, cr, sg, info) == NGP_OK, "the largest conditioning block refused");
    CHECK(call(f, d_over, ta_l.data(), 1, ya_l.data(), e.counts, e.comps, m, tn_l.data(), mu, cr, sg, info) == NGP_ERR_TOO_LARGE, "one appended point over the limit accepted");
    ngp_factor_destroy(f);
    // no main block at all (n < 64)
    Series s20(20);
    ngp_factor *g = make_factor(ctx, e, s20);
    if (g) {
        const std::vector<double> t3 = after(s20.t[19], 1, 300);
        Out o3(1, 300, true);
        CHECK(call(g, 0, nullptr, 1, nullptr, e.counts, e.comps, 300, t3.data(), o3.mu.data(), o3.cross.data(), o3.sg(), info) == NGP_OK, "a series without a main block");
        ngp_factor_destroy(g);
    }
}

// a device that holds one or two particles' working storage: the particles go through in chunks
static void chunking() {
    mock_hip_set_device_bytes((size_t)8 << 20);
    ngp_ctx *ctx = nullptr;
    if (ngp_ctx_create(0, &ctx) != NGP_OK) { ++fails; return; }
    Ensemble e;
    const int n = 191, m = 130;
    Series s(n);
    ngp_factor *f = make_factor(ctx, e, s);
    if (f) {
        const std::vector<double> t_new = after(s.t[n - 1], 1, m);
        Out o(1, m, true);
        const long before = mock_hip_launches();
        CHECK(ngp_factor_components_long(f, 0, nullptr, 1, nullptr, e.counts, e.comps, m, t_new.data(), o.mu.data(),
                                         o.cross.data(), o.sg(), o.info.data()) == NGP_OK,
              "a large P refused on a small device");
        // eight per chunk: fill, small blocks, solve, products, conditioning block, means, cross, sigma
        const long launches = mock_hip_launches() - before;
        CHECK(launches % 8 == 0 && launches > 8, "the particles did not go through in chunks");
        ngp_factor_destroy(f);
    }
    ngp_ctx_destroy(ctx);
    mock_hip_set_device_bytes((size_t)2 << 30);
}

static void query_loop(ngp_factor *f, double t_last, int id, int rounds) {
    Ensemble e;
    const int m = 100 + 17 * id, d = 2;
    const std::vector<double> t_add = after(t_last, 1, d), t_new = after(t_last, d + 1, m);
    const std::vector<double> y_add = {0.1, -0.1, 0.3, 0.2};
    Out o(2, m, true);
    for (int r = 0; r < rounds; ++r) {
        CHECK(ngp_factor_components_long(f, d, t_add.data(), 2, y_add.data(), e.counts, e.comps, m, t_new.data(),
                                         o.mu.data(), o.cross.data(), (r + id) & 1 ? o.sg() : nullptr,
                                         o.info.data()) == NGP_OK, "concurrent query");
        std::vector<double> mu((size_t)P * 2 * m), var((size_t)P * m);
        CHECK(ngp_factor_predict_long(f, d, t_add.data(), 2, y_add.data(), m, t_new.data(), 0, mu.data(), var.data(),
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
    std::printf("components_long_stress: %ld kernel launches issued, %d failures\n", mock_hip_launches(), fails.load());
    return fails.load() ? 1 : 0;
}

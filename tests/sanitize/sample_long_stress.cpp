// The host code of ngp_factor_sample_long (argument checks, limits, the staging it shares with
// ngp_factor_predict_long, the round trip for the path counts, chunking of the particles and of
// the staged normals by what the device holds, the runs of particles that carry weight, the
// context's lock) against the mock HIP runtime (see mock_hip.cpp): good and bad arguments, the
// limits at exactly the bound and one over, a device so small that the particles go through in
// several chunks, and two threads drawing from ONE factor.  Built with -fsanitize=thread and with
// -fsanitize=address,undefined by tests/test_sample_long_sanitizers.py; exit code 0 and a silent
// sanitizer are the test.  (The mock's kernels do nothing: values are not looked at, and every
// count of paths comes back zero, so the host must cope with counts that do not add up.)
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

static ngp_factor *make_factor(ngp_ctx *ctx, const Ensemble &e, const Series &s) {
    ngp_factor *f = nullptr;
    CHECK(ngp_factor_create(ctx, 3, e.ks, (int)s.t.size(), s.t.data(), s.y.data(), 0, &f) == NGP_OK && f, "factor_create");
    return f;
}

static void arguments_and_limits(ngp_ctx *ctx) {
    Ensemble e;
    const int P = 3, n = 191, m = 200, draws = 5;
    Series s(n);
    ngp_factor *f = make_factor(ctx, e, s);
    if (!f) return;
    const std::vector<double> t_new = after(s.t[n - 1], 4, m), t_add = after(s.t[n - 1], 1, 3);
    const std::vector<double> y_add = {0.1, 0.2, 0.3, -0.1, -0.2, -0.3};   // D = 2, d = 3
    const std::vector<double> w2 = {0.5, 0.0, 0.5, 0.25, 0.0, 0.75}, w1 = {0.2, 0.3, 0.5};
    std::vector<double> out((size_t)2 * draws * m), mu((size_t)P * 2 * m), var((size_t)P * m);
    std::vector<int32_t> comp(2 * draws), info(P), cinfo(P);
    auto call = [&](ngp_factor *ff, int d, const double *ta, int D, const double *ya, int mm, const double *tn,
                    const double *w, int dr, double *po) {
        return ngp_factor_sample_long(ff, d, ta, D, ya, mm, tn, 1, w, dr, 99u, po, comp.data(), mu.data(),
                                      var.data(), info.data(), cinfo.data());
    };
    CHECK(call(f, 3, t_add.data(), 2, y_add.data(), m, t_new.data(), w2.data(), draws, out.data()) == NGP_OK, "nowcast form");
    CHECK(call(f, 0, nullptr, 0, nullptr, m, t_new.data(), w1.data(), draws, out.data()) == NGP_OK, "d = 0 ignores D, t_add, y_add");
    CHECK(ngp_factor_sample_long(f, 0, nullptr, 1, nullptr, m, t_new.data(), 0, w1.data(), draws, 1u, out.data(), nullptr,
                                 nullptr, nullptr, nullptr, nullptr) == NGP_OK, "the optional outputs may be null");
    CHECK(call(f, 0, nullptr, 1, nullptr, 63, t_new.data(), w1.data(), 1, out.data()) == NGP_OK, "under one block, one draw");
    CHECK(call(nullptr, 0, nullptr, 1, nullptr, m, t_new.data(), w1.data(), draws, out.data()) == NGP_ERR_ARG, "null factor accepted");
    CHECK(call(f, 0, nullptr, 1, nullptr, m, nullptr, w1.data(), draws, out.data()) == NGP_ERR_ARG, "null dates accepted");
    CHECK(call(f, 0, nullptr, 1, nullptr, m, t_new.data(), nullptr, draws, out.data()) == NGP_ERR_ARG, "null weights accepted");
    CHECK(call(f, 0, nullptr, 1, nullptr, m, t_new.data(), w1.data(), draws, nullptr) == NGP_ERR_ARG, "null out accepted");
    CHECK(call(f, 0, nullptr, 1, nullptr, 0, t_new.data(), w1.data(), draws, out.data()) == NGP_ERR_ARG, "m = 0 accepted");
    CHECK(call(f, 0, nullptr, 1, nullptr, m, t_new.data(), w1.data(), 0, out.data()) == NGP_ERR_ARG, "draws = 0 accepted");
    CHECK(call(f, -1, t_add.data(), 2, y_add.data(), m, t_new.data(), w2.data(), draws, out.data()) == NGP_ERR_ARG, "d < 0 accepted");
    CHECK(call(f, 3, t_add.data(), 0, y_add.data(), m, t_new.data(), w2.data(), draws, out.data()) == NGP_ERR_ARG, "D = 0 with d > 0 accepted");
    CHECK(call(f, 3, nullptr, 2, y_add.data(), m, t_new.data(), w2.data(), draws, out.data()) == NGP_ERR_ARG, "null t_add with d > 0 accepted");
    CHECK(call(f, 3, t_add.data(), 2, nullptr, m, t_new.data(), w2.data(), draws, out.data()) == NGP_ERR_ARG, "null y_add with d > 0 accepted");
    // the horizon at the bound and one over
    const int m_max = NGP_MAX_LONG_HORIZON;
    const std::vector<double> t_far = after(s.t[n - 1], 1, m_max + 1);
    std::vector<double> outl((size_t)m_max + 1);
    CHECK(ngp_factor_sample_long(f, 0, nullptr, 1, nullptr, m_max, t_far.data(), 1, w1.data(), 1, 3u, outl.data(), nullptr,
                                 nullptr, nullptr, nullptr, nullptr) == NGP_OK, "the longest horizon refused");
    CHECK(ngp_factor_sample_long(f, 0, nullptr, 1, nullptr, m_max + 1, t_far.data(), 1, w1.data(), 1, 3u, outl.data(), nullptr,
                                 nullptr, nullptr, nullptr, nullptr) == NGP_ERR_TOO_LARGE, "one date over the limit accepted");
    // the conditioning block at the bound and one over: tail + d + 1 = 192 / 193
    const int d_fit = NGP_MAX_AUX - n % 64 - 1, d_over = d_fit + 1;
    const std::vector<double> ta_l = after(s.t[n - 1], 1, d_over), ya_l(d_over, 0.25);
    const std::vector<double> tn_l = after(s.t[n - 1], d_over + 1, m);
    CHECK(call(f, d_fit, ta_l.data(), 1, ya_l.data(), m, tn_l.data(), w1.data(), draws, out.data()) == NGP_OK, "the largest conditioning block refused");
    CHECK(call(f, d_over, ta_l.data(), 1, ya_l.data(), m, tn_l.data(), w1.data(), draws, out.data()) == NGP_ERR_TOO_LARGE, "one appended point over the limit accepted");
    // more paths than an int32 counts: refused before anything is allocated
    CHECK(call(f, 3, t_add.data(), 2, y_add.data(), m, t_new.data(), w2.data(), INT32_MAX / 2 + 1, out.data()) == NGP_ERR_TOO_LARGE, "S draws > INT32_MAX accepted");
    ngp_factor_destroy(f);
}

// a device that holds one or two particles' working storage: the particles go through in chunks,
// and one that does not hold a single particle beside the paths refuses
static void chunking() {
    mock_hip_set_device_bytes((size_t)4 << 20);
    ngp_ctx *ctx = nullptr;
    if (ngp_ctx_create(0, &ctx) != NGP_OK) { ++fails; return; }
    Ensemble e;
    const int n = 191, m = 300, draws = 4;
    Series s(n);
    ngp_factor *f = make_factor(ctx, e, s);
    if (f) {
        const std::vector<double> t_new = after(s.t[n - 1], 1, m);
        const std::vector<double> w_all = {0.2, 0.3, 0.5}, w_one = {1.0, 0.0, 0.0};
        std::vector<double> out((size_t)draws * m);
        std::vector<int32_t> cinfo(3);
        long before = mock_hip_launches();
        CHECK(ngp_factor_sample_long(f, 0, nullptr, 1, nullptr, m, t_new.data(), 1, w_all.data(), draws, 5u, out.data(),
                                     nullptr, nullptr, nullptr, nullptr, cinfo.data()) == NGP_OK, "a large P refused on a small device");
        const long all = mock_hip_launches() - before;
        // one chunk would be 3 (pick, count, group) + 7 (the long query) + 1 (padding) + 2 nb - 1 launches
        const int nb = (m + 63) / 64;
        CHECK(all > 3 + 7 + 1 + 2 * nb - 1, "the particles did not go through in chunks");
        before = mock_hip_launches();
        CHECK(ngp_factor_sample_long(f, 0, nullptr, 1, nullptr, m, t_new.data(), 1, w_one.data(), draws, 5u, out.data(),
                                     nullptr, nullptr, nullptr, nullptr, cinfo.data()) == NGP_OK, "particles without weight");
        // the chunks behind the first hold no particle with weight: no factorisation is launched for them
        CHECK(mock_hip_launches() - before < all, "particles without weight were factorised");
        ngp_factor_destroy(f);
    }
    ngp_ctx_destroy(ctx);
    mock_hip_set_device_bytes((size_t)1 << 20);
    if (ngp_ctx_create(0, &ctx) != NGP_OK) { ++fails; return; }
    Series s64(64);
    f = make_factor(ctx, e, s64);
    if (f) {
        const std::vector<double> t_new = after(s64.t[63], 1, 1024), w = {0.2, 0.3, 0.5};
        std::vector<double> out((size_t)1024);
        CHECK(ngp_factor_sample_long(f, 0, nullptr, 1, nullptr, 1024, t_new.data(), 1, w.data(), 1, 5u, out.data(), nullptr,
                                     nullptr, nullptr, nullptr, nullptr) == NGP_ERR_TOO_LARGE, "a particle the device cannot hold accepted");
        ngp_factor_destroy(f);
    }
    ngp_ctx_destroy(ctx);
    mock_hip_set_device_bytes((size_t)2 << 30);
}

static void draw_loop(ngp_factor *f, double t_last, int id, int rounds) {
    const int P = 3, m = 200 + 17 * id, d = 2, draws = 3 + id;
    const std::vector<double> t_add = after(t_last, 1, d), t_new = after(t_last, d + 1, m);
    const std::vector<double> y_add = {0.1, -0.1, 0.3, 0.2};
    const std::vector<double> w = {0.5, 0.25, 0.25, 0.0, 0.5, 0.5};
    std::vector<double> out((size_t)2 * draws * m), mu((size_t)P * 2 * m), var((size_t)P * m);
    std::vector<int32_t> info(P), cinfo(P), comp(2 * draws);
    for (int r = 0; r < rounds; ++r) {
        CHECK(ngp_factor_sample_long(f, d, t_add.data(), 2, y_add.data(), m, t_new.data(), r & 1, w.data(), draws,
                                     (uint64_t)(r + id), out.data(), comp.data(), (r + id) & 1 ? mu.data() : nullptr,
                                     var.data(), info.data(), cinfo.data()) == NGP_OK, "concurrent draw");
        CHECK(ngp_factor_predict_long(f, d, t_add.data(), 2, y_add.data(), m, t_new.data(), 1, mu.data(), var.data(),
                                      nullptr, info.data()) == NGP_OK, "the long query beside it");
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
            std::thread a(draw_loop, f, s.t[149], 0, 6), b(draw_loop, f, s.t[149], 1, 6);
            a.join();
            b.join();
            ngp_factor_destroy(f);
        }
    }
    ngp_ctx_destroy(ctx);
    chunking();
    CHECK(mock_hip_errors() == 0, "bad free / out-of-bounds copy seen by the mock runtime");
    CHECK(mock_hip_live_allocations() == 0, "device allocations left after the context was destroyed");
    std::printf("sample_long_stress: %ld kernel launches issued, %d failures\n", mock_hip_launches(), fails.load());
    return fails.load() ? 1 : 0;
}

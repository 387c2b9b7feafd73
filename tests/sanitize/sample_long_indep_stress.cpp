// The host code of ngp_factor_sample_long_indep (its own checks and blocks, and the body it shares
// with ngp_factor_sample_long: the count round trip, chunking of the items and of the staged
// normals by what the device holds, the runs of items that carry weight, the context's lock)
// against the mock HIP runtime (see mock_hip.cpp): good and bad arguments, the limits at exactly
// the bound and one over, a device so small that the items go through in several chunks, and two
// threads drawing from ONE factor, one of them in the shared form.  Built with -fsanitize=thread
// and with -fsanitize=address,undefined by tests/test_sample_long_indep_sanitizers.py; exit code 0
// and a silent sanitizer are the test.  (The mock's kernels do nothing: values are not looked at,
// and every count of paths comes back zero, so the host must cope with counts that do not add up.)
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

// six items: three mixtures of two (or two of three), every mixture with a data row of its own
struct Ensemble {
    int32_t ops0[5] = {2, 5, 6, 3, 6}, ops1[5] = {2, 5, 6, 3, 7}, ops2[7] = {3, 1, 6, 5, 8, 4, 6};
    double par0[8] = {0.2, 0.1, 0.5, 0.9, 0.3, 0.7, 0.21, 0.4};
    double par1[8] = {0.1, 0.3, 0.8, 1.1, 0.21, 0.4, 0.3, 0.6};
    double par2[11] = {0.2, 0.5, 0.25, 1.0, 0.3, 0.3, 0.5, 0.1, 0.3, 1.5, 0.2};
    ngp_kernel ks[6];
    Ensemble() {
        ks[0] = {5, 8, ops0, par0, 0.05};
        ks[1] = {5, 8, ops1, par1, 0.02};
        ks[2] = {7, 11, ops2, par2, 0.1};
        ks[3] = ks[1];
        ks[4] = ks[2];
        ks[5] = ks[0];
    }
};

struct Series {
    int n;
    std::vector<double> t, y;   // y [6][n]
    explicit Series(int n_) : n(n_), t(n_), y((size_t)6 * n_) {
        for (int i = 0; i < n; ++i) t[i] = (double)i / 200;
        for (int b = 0; b < 6; ++b)
            for (int i = 0; i < n; ++i) y[(size_t)b * n + i] = std::sin(9.0 * t[i]) + 0.05 * (b / 2);
    }
};

static std::vector<double> after(double t0, int first, int count) {
    std::vector<double> v(count);
    for (int i = 0; i < count; ++i) v[i] = t0 + (double)(first + i) / 200;
    return v;
}

static ngp_factor *make_factor(ngp_ctx *ctx, const Ensemble &e, const Series &s, int P = 6) {
    ngp_factor *f = nullptr;
    CHECK(ngp_factor_create(ctx, P, e.ks, s.n, s.t.data(), s.y.data(), s.n, &f) == NGP_OK && f, "factor_create");
    return f;
}

static void arguments_and_limits(ngp_ctx *ctx) {
    Ensemble e;
    const int P = 6, n = 191, m = 200, draws = 5;
    Series s(n);
    ngp_factor *f = make_factor(ctx, e, s);
    if (!f) return;
    const std::vector<double> t_new = after(s.t[n - 1], 1, m);
    const std::vector<double> w = {0.5, 0.5, 1.0, 0.0, 0.25, 0.75};
    const std::vector<uint64_t> seeds = {11u, 12u, 13u, 14u, 15u, 16u};
    std::vector<double> out((size_t)P * draws * m), mu((size_t)P * m), var((size_t)P * m);
    std::vector<int32_t> comp(P * draws), info(P), cinfo(P);
    auto call = [&](ngp_factor *ff, int S, int mm, const double *tn, const double *ww, int dr, const uint64_t *sd,
                    double *po) {
        return ngp_factor_sample_long_indep(ff, S, mm, tn, 1, ww, dr, sd, po, comp.data(), mu.data(), var.data(),
                                            info.data(), cinfo.data());
    };
    CHECK(call(f, 3, m, t_new.data(), w.data(), draws, seeds.data(), out.data()) == NGP_OK, "three mixtures of two");
    CHECK(call(f, 2, m, t_new.data(), w.data(), draws, seeds.data(), out.data()) == NGP_OK, "two mixtures of three");
    CHECK(call(f, 6, m, t_new.data(), w.data(), draws, seeds.data(), out.data()) == NGP_OK, "six mixtures of one");
    CHECK(call(f, 1, m, t_new.data(), w.data(), draws, seeds.data(), out.data()) == NGP_OK, "one mixture of six");
    CHECK(ngp_factor_sample_long_indep(f, 3, m, t_new.data(), 0, w.data(), draws, seeds.data(), out.data(), nullptr, nullptr,
                                       nullptr, nullptr, nullptr) == NGP_OK, "the optional outputs may be null");
    CHECK(call(f, 3, 63, t_new.data(), w.data(), 1, seeds.data(), out.data()) == NGP_OK, "under one block, one draw");
    CHECK(call(nullptr, 3, m, t_new.data(), w.data(), draws, seeds.data(), out.data()) == NGP_ERR_ARG, "null factor accepted");
    CHECK(call(f, 3, m, nullptr, w.data(), draws, seeds.data(), out.data()) == NGP_ERR_ARG, "null dates accepted");
    CHECK(call(f, 3, m, t_new.data(), nullptr, draws, seeds.data(), out.data()) == NGP_ERR_ARG, "null weights accepted");
    CHECK(call(f, 3, m, t_new.data(), w.data(), draws, nullptr, out.data()) == NGP_ERR_ARG, "null seeds accepted");
    CHECK(call(f, 3, m, t_new.data(), w.data(), draws, seeds.data(), nullptr) == NGP_ERR_ARG, "null out accepted");
    CHECK(call(f, 3, 0, t_new.data(), w.data(), draws, seeds.data(), out.data()) == NGP_ERR_ARG, "m = 0 accepted");
    CHECK(call(f, 3, m, t_new.data(), w.data(), 0, seeds.data(), out.data()) == NGP_ERR_ARG, "draws = 0 accepted");
    CHECK(call(f, 0, m, t_new.data(), w.data(), draws, seeds.data(), out.data()) == NGP_ERR_ARG, "S = 0 accepted");
    CHECK(call(f, 4, m, t_new.data(), w.data(), draws, seeds.data(), out.data()) == NGP_ERR_ARG, "six items as four mixtures accepted");
    CHECK(call(f, 7, m, t_new.data(), w.data(), draws, seeds.data(), out.data()) == NGP_ERR_ARG, "more mixtures than items accepted");
    // the horizon at the bound and one over
    const int m_max = NGP_MAX_LONG_HORIZON;
    const std::vector<double> t_far = after(s.t[n - 1], 1, m_max + 1);
    std::vector<double> outl((size_t)3 * (m_max + 1));
    CHECK(ngp_factor_sample_long_indep(f, 3, m_max, t_far.data(), 1, w.data(), 1, seeds.data(), outl.data(), nullptr, nullptr,
                                       nullptr, nullptr, nullptr) == NGP_OK, "the longest horizon refused");
    CHECK(ngp_factor_sample_long_indep(f, 3, m_max + 1, t_far.data(), 1, w.data(), 1, seeds.data(), outl.data(), nullptr,
                                       nullptr, nullptr, nullptr, nullptr) == NGP_ERR_TOO_LARGE, "one date over the limit accepted");
    // more paths than an int32 counts: refused before anything is allocated
    CHECK(call(f, 3, m, t_new.data(), w.data(), INT32_MAX / 3 + 1, seeds.data(), out.data()) == NGP_ERR_TOO_LARGE, "S draws > INT32_MAX accepted");
    ngp_factor_destroy(f);
}

// a device that holds one or two items' working storage: the items go through in chunks, and one
// that does not hold a single item beside the paths refuses
static void chunking() {
    mock_hip_set_device_bytes((size_t)6 << 20);
    ngp_ctx *ctx = nullptr;
    if (ngp_ctx_create(0, &ctx) != NGP_OK) { ++fails; return; }
    Ensemble e;
    const int n = 191, m = 300, draws = 4;
    Series s(n);
    ngp_factor *f = make_factor(ctx, e, s);
    if (f) {
        const std::vector<double> t_new = after(s.t[n - 1], 1, m);
        const std::vector<double> w_all = {0.5, 0.5, 0.5, 0.5, 0.5, 0.5}, w_one = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const std::vector<uint64_t> seeds = {5u, 6u, 7u};
        std::vector<double> out((size_t)3 * draws * m);
        std::vector<int32_t> cinfo(6);
        long before = mock_hip_launches();
        CHECK(ngp_factor_sample_long_indep(f, 3, m, t_new.data(), 1, w_all.data(), draws, seeds.data(), out.data(), nullptr,
                                           nullptr, nullptr, nullptr, cinfo.data()) == NGP_OK, "a large P refused on a small device");
        const long all = mock_hip_launches() - before;
        // one chunk would be 3 (pick, count, group) + 7 (the long query) + 1 (padding) + 2 nb - 1 launches
        const int nb = (m + 63) / 64;
        CHECK(all > 3 + 7 + 1 + 2 * nb - 1, "the items did not go through in chunks");
        before = mock_hip_launches();
        CHECK(ngp_factor_sample_long_indep(f, 3, m, t_new.data(), 1, w_one.data(), draws, seeds.data(), out.data(), nullptr,
                                           nullptr, nullptr, nullptr, cinfo.data()) == NGP_OK, "items without weight");
        // the chunks behind the first hold no item with weight: no factorisation is launched for them
        CHECK(mock_hip_launches() - before < all, "items without weight were factorised");
        ngp_factor_destroy(f);
    }
    ngp_ctx_destroy(ctx);
    mock_hip_set_device_bytes((size_t)1 << 20);
    if (ngp_ctx_create(0, &ctx) != NGP_OK) { ++fails; return; }
    Series s64(64);
    f = make_factor(ctx, e, s64, 2);
    if (f) {
        const std::vector<double> t_new = after(s64.t[63], 1, 1024), w = {0.5, 0.5};
        const std::vector<uint64_t> seeds = {5u, 6u};
        std::vector<double> out((size_t)2 * 1024);
        CHECK(ngp_factor_sample_long_indep(f, 2, 1024, t_new.data(), 1, w.data(), 1, seeds.data(), out.data(), nullptr, nullptr,
                                           nullptr, nullptr, nullptr) == NGP_ERR_TOO_LARGE, "an item the device cannot hold accepted");
        ngp_factor_destroy(f);
    }
    ngp_ctx_destroy(ctx);
    mock_hip_set_device_bytes((size_t)2 << 30);
}

static void draw_loop(ngp_factor *f, double t_last, int id, int rounds) {
    const int P = 6, m = 200 + 17 * id, draws = 3 + id;
    const std::vector<double> t_new = after(t_last, 1, m);
    const std::vector<double> w = {0.5, 0.5, 1.0, 0.0, 0.25, 0.75};
    const std::vector<uint64_t> seeds = {21u, 22u, 23u};
    std::vector<double> out((size_t)3 * draws * m), mu((size_t)P * m), var((size_t)P * m);
    std::vector<int32_t> info(P), cinfo(P), comp(3 * draws);
    for (int r = 0; r < rounds; ++r) {
        if (id == 0)
            CHECK(ngp_factor_sample_long_indep(f, 3, m, t_new.data(), r & 1, w.data(), draws, seeds.data(), out.data(),
                                               comp.data(), r & 1 ? mu.data() : nullptr, var.data(), info.data(),
                                               cinfo.data()) == NGP_OK, "concurrent draw, independent form");
        else   // the shared form beside it: S = 1 over the same six items
            CHECK(ngp_factor_sample_long(f, 0, nullptr, 1, nullptr, m, t_new.data(), r & 1, w.data(), draws, (uint64_t)r,
                                         out.data(), comp.data(), mu.data(), var.data(), info.data(),
                                         cinfo.data()) == NGP_OK, "concurrent draw, shared form");
        CHECK(ngp_factor_predict_long(f, 0, nullptr, 1, nullptr, m, t_new.data(), 1, mu.data(), var.data(), nullptr,
                                      info.data()) == NGP_OK, "the long query beside it");
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
    std::printf("sample_long_indep_stress: %ld kernel launches issued, %d failures\n", mock_hip_launches(), fails.load());
    return fails.load() ? 1 : 0;
}

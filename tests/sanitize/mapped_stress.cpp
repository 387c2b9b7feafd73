// ngp_mixture_crps_mapped against the mock HIP runtime (see mock_hip.cpp): four threads on one
// context call it with good and bad arguments, every status checked; and the panel planner of
// ngp_mixmap_plan.h on hostile records.  Built with -fsanitize=thread and with
// -fsanitize=address,undefined by tests/test_mixture_mapped_sanitizers.py; exit code 0 and a
// silent sanitizer are the test.  (The mock's kernels do nothing: a date's record is whatever the
// reused block held, so the planner sees arbitrary numbers — what is looked at is what the HOST
// writes: the statuses, the component index of a bad date and its NaN.)
#include <atomic>
#include <cmath>
#include <cstdio>
#include <limits>
#include <thread>
#include <vector>

#include "../../include/ngp.h"
#include "../../nowcastautogp_amd/csrc/ngp_mixmap_plan.h"

extern "C" long mock_hip_launches(void);
extern "C" long mock_hip_live_allocations(void);
extern "C" long mock_hip_errors(void);

static std::atomic<int> fails{0};
#define CHECK(c, what) do { if (!(c)) { ++fails; std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, what); } } while (0)

static void planner() {
    using namespace ngp;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const double vals[] = {0.0, -1.0, 1.0, 1e-300, 1e300, inf, -inf, nan, 3.5};
    for (double alo : vals) for (double x0 : vals) for (double ahi : vals) for (double sd : vals) {
        double rec[MIXMAP_REC] = {0};
        rec[MIXMAP_REC_ALO] = alo; rec[MIXMAP_REC_X0] = x0; rec[MIXMAP_REC_AHI] = ahi;
        rec[MIXMAP_REC_SDMIN] = sd;
        MixMapPlan p = mixmap_plan(7, rec);
        CHECK(p.date == 7 && p.npanels >= 0 && p.npanels <= MIXMAP_MAX_PANELS && p.n0 >= 0 &&
              p.n0 <= p.npanels, "plan outside its bounds");
        while (mixmap_refine(&p)) CHECK(p.npanels <= MIXMAP_MAX_PANELS, "refined beyond the cap");
    }
    double rec[MIXMAP_REC] = {0};
    rec[MIXMAP_REC_ALO] = 0.0; rec[MIXMAP_REC_X0] = 3.0; rec[MIXMAP_REC_AHI] = 10.0;
    rec[MIXMAP_REC_SDMIN] = 0.5;
    MixMapPlan p = mixmap_plan(0, rec);
    CHECK(p.n0 == 6 && p.npanels == 20 && p.h0 == 0.5 && p.h1 == 0.5 && p.a1 == 3.0, "a plain plan");
    rec[MIXMAP_REC_SDMIN] = 1e-5;                          // a million panels wanted
    p = mixmap_plan(0, rec);
    CHECK(p.npanels <= MIXMAP_MAX_PANELS && p.npanels > MIXMAP_MAX_PANELS - 2 && p.n0 >= 1, "a capped plan");
    CHECK(!mixmap_refine(&p), "a capped plan refined");
}

static void worker(ngp_ctx *ctx, int id, int rounds) {
    const int C = 300 + 77 * id, m = 3 + id;
    std::vector<double> w(C), mu((size_t)C * m), var((size_t)C * m), y(m, 5.0);
    std::vector<double> crps(m), mean(m), err(m);
    std::vector<int32_t> info(m);
    for (int c = 0; c < C; ++c) {
        w[c] = (c % 7 == 3) ? 0.0 : 1.0;
        for (int j = 0; j < m; ++j) {
            mu[(size_t)c * m + j] = 3.0 + 0.01 * ((c * 31 + j * 7) % 53);
            var[(size_t)c * m + j] = 0.01 + 0.001 * ((c + j) % 11);
        }
    }
    double sum = 0.0;
    for (double v : w) sum += v;
    for (double &v : w) v /= sum;
    ngp_inv_transform inv = {NGP_INV_BOXCOX, 0.3, 0.5, 1e6};
    for (int r = 0; r < rounds; ++r) {
        const int scale = r & 1;
        CHECK(ngp_mixture_crps_mapped(ctx, C, m, w.data(), mu.data(), var.data(), &inv, scale, 1.0,
                                      y.data(), 0.0, crps.data(), mean.data(), err.data(),
                                      info.data()) == NGP_OK, "crps_mapped");
        for (int j = 0; j < m; ++j) CHECK(info[j] <= 0 && info[j] >= NGP_INFO_NOT_CONVERGED, "clean date");
        CHECK(ngp_mixture_crps_mapped(ctx, C, m, w.data(), mu.data(), var.data(), &inv, scale, 1.0,
                                      y.data(), 1e-12, crps.data(), nullptr, nullptr,
                                      info.data()) == NGP_OK, "crps_mapped without mean and err");
        const int bad_c = 4, bad_j = m - 1;
        const double keep = var[(size_t)bad_c * m + bad_j], keep0 = mu[(size_t)3 * m + 0];
        var[(size_t)bad_c * m + bad_j] = (r & 1) ? -1.0 : 0.0;
        mu[(size_t)3 * m + 0] = NAN;                       // weight zero: ignored
        CHECK(ngp_mixture_crps_mapped(ctx, C, m, w.data(), mu.data(), var.data(), &inv, scale, 1.0,
                                      y.data(), 0.0, crps.data(), mean.data(), err.data(),
                                      info.data()) == NGP_OK, "crps_mapped (bad date)");
        for (int j = 0; j < m; ++j) CHECK(j == bad_j ? info[j] == bad_c + 1 : info[j] <= 0, "info of a bad date");
        CHECK(std::isnan(crps[bad_j]) && std::isnan(mean[bad_j]) && std::isnan(err[bad_j]),
              "NaN on the bad date");
        var[(size_t)bad_c * m + bad_j] = keep;
        mu[(size_t)3 * m + 0] = keep0;
#define BAD(what, ...) CHECK(ngp_mixture_crps_mapped(__VA_ARGS__) == NGP_ERR_ARG, what)
        BAD("null context", nullptr, C, m, w.data(), mu.data(), var.data(), &inv, 0, 0.0, y.data(), 0.0,
            crps.data(), nullptr, nullptr, info.data());
        BAD("null inv", ctx, C, m, w.data(), mu.data(), var.data(), nullptr, 0, 0.0, y.data(), 0.0,
            crps.data(), nullptr, nullptr, info.data());
        BAD("unknown scale", ctx, C, m, w.data(), mu.data(), var.data(), &inv, 2, 0.0, y.data(), 0.0,
            crps.data(), nullptr, nullptr, info.data());
        BAD("negative shift", ctx, C, m, w.data(), mu.data(), var.data(), &inv, 1, -1.0, y.data(), 0.0,
            crps.data(), nullptr, nullptr, info.data());
        BAD("NaN tol", ctx, C, m, w.data(), mu.data(), var.data(), &inv, 1, 1.0, y.data(), NAN,
            crps.data(), nullptr, nullptr, info.data());
        BAD("m = 0", ctx, C, 0, w.data(), mu.data(), var.data(), &inv, 1, 1.0, y.data(), 0.0,
            crps.data(), nullptr, nullptr, info.data());
        ngp_inv_transform bad = inv;
        bad.kind = 9;
        BAD("unknown kind", ctx, C, m, w.data(), mu.data(), var.data(), &bad, 0, 0.0, y.data(), 0.0,
            crps.data(), nullptr, nullptr, info.data());
        const double y_keep = y[0];
        y[0] = (r & 1) ? NAN : -2.0;                       // log(-2 + 1) is undefined
        BAD("bad y", ctx, C, m, w.data(), mu.data(), var.data(), &inv, 1, 1.0, y.data(), 0.0,
            crps.data(), nullptr, nullptr, info.data());
        y[0] = y_keep;
        CHECK(ngp_mixture_crps_mapped(ctx, 70000, m, w.data(), mu.data(), var.data(), &inv, 0, 0.0,
                                      y.data(), 0.0, crps.data(), nullptr, nullptr,
                                      info.data()) == NGP_ERR_TOO_LARGE, "C beyond the limit accepted");
    }
}

int main() {
    planner();
    ngp_ctx *ctx = nullptr;
    if (ngp_ctx_create(0, &ctx) != NGP_OK) return 2;
    const int T = 4, rounds = 6;
    std::vector<std::thread> th;
    for (int i = 0; i < T; ++i) th.emplace_back(worker, ctx, i, rounds);
    for (auto &t : th) t.join();
    ngp_ctx_destroy(ctx);
    CHECK(mock_hip_errors() == 0, "bad free / out-of-bounds copy seen by the mock runtime");
    CHECK(mock_hip_live_allocations() == 0, "device allocations left after the context was destroyed");
    std::printf("mapped_stress: %ld kernel launches issued, %d failures\n", mock_hip_launches(), fails.load());
    return fails.load() ? 1 : 0;
}

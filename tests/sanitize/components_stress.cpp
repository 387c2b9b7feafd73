// The host code of the additive decomposition (ngp_kernel_components, ngp_factor_components: the
// argument checks, the staging of the component programs, allocation, the context's lock) against
// the mock HIP runtime (see mock_hip.cpp): four threads share one context, each with a resident
// factor of its own, good and bad arguments, every status checked.  Built with -fsanitize=thread
// and with -fsanitize=address,undefined by tests/test_components_sanitizers.py; exit code 0 and a
// silent sanitizer are the test.  (The mock's kernels do nothing: values are not looked at.)
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

static void slicing(const Ensemble &e) {
    int32_t cnt = 0, of[NGP_MAX_OPS / 2 + 1], ol[NGP_MAX_OPS / 2 + 1], pf[NGP_MAX_OPS / 2 + 1],
            pl[NGP_MAX_OPS / 2 + 1];
    const int want[3] = {3, 1, 2};
    for (int k = 0; k < 3; ++k) {
        CHECK(ngp_kernel_components(&e.ks[k], &cnt, of, ol, pf, pl) == NGP_OK && cnt == want[k], "slicing");
        int ops = 0, par = 0, nops = 0;
        for (int i = 0; i < cnt; ++i) {   // contiguous slices, in order, that leave only the Plus nodes out
            CHECK(of[i] >= ops && pf[i] == par, "slices out of order");
            ops = of[i] + ol[i];
            nops += ol[i];
            par += pl[i];
            const ngp_kernel c{ol[i], pl[i], e.ks[k].ops + of[i], e.ks[k].params + pf[i], 0.0};
            CHECK(ngp_kernel_check(&c) == NGP_OK, "a component is not a valid program");
        }
        CHECK(par == e.ks[k].n_params && nops + (cnt - 1) == e.ks[k].n_ops, "slices do not cover the tree");
    }
    CHECK(ngp_kernel_components(&e.ks[2], &cnt, nullptr, nullptr, nullptr, nullptr) == NGP_OK && cnt == 2,
          "count alone");
    CHECK(ngp_kernel_components(nullptr, &cnt, of, ol, pf, pl) == NGP_ERR_ARG, "null kernel accepted");
    CHECK(ngp_kernel_components(&e.ks[0], nullptr, of, ol, pf, pl) == NGP_ERR_ARG, "null count accepted");
    ngp_kernel bad = e.ks[0];
    bad.n_ops = 4;
    CHECK(ngp_kernel_components(&bad, &cnt, of, ol, pf, pl) == NGP_ERR_PROGRAM, "malformed program accepted");
}

static void worker(ngp_ctx *ctx, int id, int rounds) {
    Ensemble e;
    slicing(e);
    const int P = 3, n = 40 + 45 * id, m = 3 + id;   // n = 40: no main block; 85, 130, 175: tails 21, 2, 47
    std::vector<double> t(n), y(n), t_new(m);
    for (int i = 0; i < n; ++i) { t[i] = (double)i / (n - 1); y[i] = std::sin(9.0 * t[i]); }
    for (int i = 0; i < m; ++i) t_new[i] = 1.0 + (double)(i + 1) / (n - 1);
    // the component programs, particle-major: slices of the particles' own arrays
    std::vector<ngp_kernel> comps;
    int32_t counts[3];
    for (int k = 0; k < P; ++k) {
        int32_t cnt = 0, of[33], ol[33], pf[33], pl[33];
        CHECK(ngp_kernel_components(&e.ks[k], &cnt, of, ol, pf, pl) == NGP_OK, "slicing");
        counts[k] = cnt;
        for (int i = 0; i < cnt; ++i)
            comps.push_back(ngp_kernel{ol[i], pl[i], e.ks[k].ops + of[i], e.ks[k].params + pf[i], 99.0});
    }
    const size_t tot = comps.size();
    size_t nsig = 0;
    for (int k = 0; k < P; ++k) nsig += (size_t)counts[k] * m * counts[k] * m;
    std::vector<double> mu(tot * m), var(tot * m), sg(nsig);
    std::vector<int32_t> info(P);
    for (int r = 0; r < rounds; ++r) {
        CHECK(ngp_set_structured_storage(ctx, (r + id) & 1) == NGP_OK, "set_structured_storage");
        CHECK(ngp_profile_enable(ctx, r & 1) == NGP_OK, "profile_enable");
        ngp_factor *f = nullptr;
        CHECK(ngp_factor_create(ctx, P, e.ks, n, t.data(), y.data(), 0, &f) == NGP_OK && f, "factor_create");
        if (!f) continue;
        CHECK(ngp_factor_components(f, counts, comps.data(), m, t_new.data(), mu.data(), sg.data(),
                                    var.data(), info.data()) == NGP_OK, "factor_components");
        CHECK(ngp_factor_components(f, counts, comps.data(), m, t_new.data(), mu.data(), nullptr,
                                    var.data(), nullptr) == NGP_OK, "factor_components (var alone)");
        CHECK(ngp_factor_components(f, counts, comps.data(), m, t_new.data(), mu.data(), nullptr,
                                    nullptr, info.data()) == NGP_OK, "factor_components (mu alone)");
        // malformed calls: refused, nothing left behind
        CHECK(ngp_factor_components(nullptr, counts, comps.data(), m, t_new.data(), mu.data(), sg.data(),
                                    var.data(), info.data()) == NGP_ERR_ARG, "null factor accepted");
        CHECK(ngp_factor_components(f, nullptr, comps.data(), m, t_new.data(), mu.data(), sg.data(),
                                    var.data(), info.data()) == NGP_ERR_ARG, "null counts accepted");
        CHECK(ngp_factor_components(f, counts, nullptr, m, t_new.data(), mu.data(), sg.data(),
                                    var.data(), info.data()) == NGP_ERR_ARG, "null components accepted");
        CHECK(ngp_factor_components(f, counts, comps.data(), m, nullptr, mu.data(), sg.data(),
                                    var.data(), info.data()) == NGP_ERR_ARG, "null dates accepted");
        CHECK(ngp_factor_components(f, counts, comps.data(), m, t_new.data(), nullptr, sg.data(),
                                    var.data(), info.data()) == NGP_ERR_ARG, "null means accepted");
        CHECK(ngp_factor_components(f, counts, comps.data(), 0, t_new.data(), mu.data(), sg.data(),
                                    var.data(), info.data()) == NGP_ERR_ARG, "m = 0 accepted");
        int32_t zero[3] = {counts[0], 0, counts[2]};
        CHECK(ngp_factor_components(f, zero, comps.data(), m, t_new.data(), mu.data(), sg.data(),
                                    var.data(), info.data()) == NGP_ERR_ARG, "C_p = 0 accepted");
        std::vector<ngp_kernel> broken = comps;
        broken[tot - 1].n_params -= 1;
        CHECK(ngp_factor_components(f, counts, broken.data(), m, t_new.data(), mu.data(), sg.data(),
                                    var.data(), info.data()) == NGP_ERR_PROGRAM, "malformed component accepted");
        // the aux limit, exactly and one row over: (n mod 64) + 1 + C m <= NGP_MAX_AUX with C = 3
        const int room = NGP_MAX_AUX - n % 64 - 1, m_fit = room / 3, m_over = m_fit + 1;
        std::vector<double> tl(m_over), mul(tot * m_over);
        for (int i = 0; i < m_over; ++i) tl[i] = 1.0 + (double)(i + 1) / (n - 1);
        CHECK(ngp_factor_components(f, counts, comps.data(), m_fit, tl.data(), mul.data(), nullptr, nullptr,
                                    info.data()) == NGP_OK, "the largest horizon refused");
        CHECK(ngp_factor_components(f, counts, comps.data(), m_over, tl.data(), mul.data(), nullptr, nullptr,
                                    info.data()) == NGP_ERR_TOO_LARGE, "one row over the limit accepted");
        ngp_factor_destroy(f);
    }
}

int main() {
    ngp_ctx *ctx = nullptr;
    if (ngp_ctx_create(0, &ctx) != NGP_OK) return 2;
    const int T = 4, rounds = 5;
    std::vector<std::thread> th;
    for (int i = 0; i < T; ++i) th.emplace_back(worker, ctx, i, rounds);
    for (auto &t : th) t.join();
    ngp_ctx_destroy(ctx);
    CHECK(mock_hip_errors() == 0, "bad free / out-of-bounds copy seen by the mock runtime");
    CHECK(mock_hip_live_allocations() == 0, "device allocations left after the context was destroyed");
    std::printf("components_stress: %ld kernel launches issued, %d failures\n", mock_hip_launches(), fails.load());
    return fails.load() ? 1 : 0;
}

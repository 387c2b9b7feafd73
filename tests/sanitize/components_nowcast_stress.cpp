// The host code of the sum-of-products terms and of the decomposition conditioned on nowcasts
// (ngp_kernel_terms, ngp_factor_components_nowcast: the argument checks, the staging of the appended
// points, the scenarios and the component programs, allocation, the context's lock) against the
// mock HIP runtime (see mock_hip.cpp): four threads share one context, each with a resident factor
// of its own, good and bad arguments, every status checked.  Built with -fsanitize=thread and with
// -fsanitize=address,undefined by tests/test_component_terms_cpu.py; exit code 0 and a silent
// sanitizer are the test.  (The mock's kernels do nothing: values are not looked at.)
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

// ChangePoint(Plus(Linear, Periodic), SqExp) | Times(Plus(Linear, Periodic), Plus(SqExp, Constant)) |
// Plus(ChangePoint(Plus(SqExp, Constant), Periodic), GammaExp)
struct Ensemble {
    int32_t ops0[5] = {2, 5, 6, 3, 8}, ops1[7] = {2, 5, 6, 3, 1, 6, 7}, ops2[7] = {3, 1, 6, 5, 8, 4, 6};
    double par0[10] = {0.2, 0.1, 0.5, 0.9, 0.3, 0.7, 0.21, 0.4, 0.5, 0.1};
    double par1[9] = {0.1, 0.3, 0.8, 1.1, 0.21, 0.4, 0.3, 0.6, 0.25};
    double par2[11] = {0.2, 0.5, 0.25, 1.0, 0.3, 0.3, 0.5, 0.1, 0.3, 1.5, 0.2};
    ngp_kernel ks[3];
    Ensemble() {
        ks[0] = {5, 10, ops0, par0, 0.05};
        ks[1] = {7, 9, ops1, par1, 0.02};
        ks[2] = {7, 11, ops2, par2, 0.1};
    }
};

struct Terms {   // the terms of one tree, in buffers of their own
    int32_t cnt = 0, of[16], ol[16], pf[16], pl[16], ops[16 * 8];
    double par[16 * 12];
};

static void splitting(const Ensemble &e) {
    const int split = NGP_SPLIT_CHANGEPOINT | NGP_SPLIT_TIMES;
    const int want_full[3] = {3, 4, 4}, want_plus[3] = {1, 1, 2};
    Terms t;
    for (int k = 0; k < 3; ++k) {
        CHECK(ngp_kernel_terms(&e.ks[k], split, 16, &t.cnt, t.of, t.ol, t.pf, t.pl, t.ops, 16 * 8, t.par,
                               16 * 12) == NGP_OK && t.cnt == want_full[k], "terms");
        int ops = 0, par = 0;
        for (int i = 0; i < t.cnt; ++i) {   // back to back, each a valid program no longer than the tree
            CHECK(t.of[i] == ops && t.pf[i] == par, "terms not back to back");
            ops += t.ol[i];
            par += t.pl[i];
            CHECK(t.ol[i] <= e.ks[k].n_ops && t.pl[i] <= e.ks[k].n_params, "a term longer than its tree");
            const ngp_kernel c{t.ol[i], t.pl[i], t.ops + t.of[i], t.par + t.pf[i], 0.0};
            CHECK(ngp_kernel_check(&c) == NGP_OK, "a term is not a valid program");
        }
        int32_t cnt = -1;
        CHECK(ngp_kernel_terms(&e.ks[k], 0, 16, &cnt, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                               0) == NGP_OK && cnt == want_plus[k], "count alone");
        // exactly enough room, and one short in either buffer
        CHECK(ngp_kernel_terms(&e.ks[k], split, t.cnt, &cnt, t.of, t.ol, t.pf, t.pl, t.ops, ops, t.par, par) ==
                  NGP_OK, "exact buffers refused");
        CHECK(ngp_kernel_terms(&e.ks[k], split, t.cnt, &cnt, t.of, t.ol, t.pf, t.pl, t.ops, ops - 1, t.par,
                               par) == NGP_ERR_TOO_LARGE && cnt == want_full[k], "ops short by one accepted");
        CHECK(ngp_kernel_terms(&e.ks[k], split, t.cnt, &cnt, t.of, t.ol, t.pf, t.pl, t.ops, ops, t.par,
                               par - 1) == NGP_ERR_TOO_LARGE && cnt == want_full[k], "params short by one accepted");
        CHECK(ngp_kernel_terms(&e.ks[k], split, t.cnt - 1, &cnt, t.of, t.ol, t.pf, t.pl, t.ops, ops, t.par,
                               par) == NGP_ERR_TOO_LARGE && cnt == want_full[k], "max_terms exceeded accepted");
    }
    int32_t cnt = 0;
    CHECK(ngp_kernel_terms(nullptr, 0, 16, &cnt, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0) ==
              NGP_ERR_ARG, "null kernel accepted");
    CHECK(ngp_kernel_terms(&e.ks[0], 0, 16, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                           0) == NGP_ERR_ARG, "null count accepted");
    CHECK(ngp_kernel_terms(&e.ks[0], 4, 16, &cnt, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0) ==
              NGP_ERR_ARG, "unknown split flag accepted");
    ngp_kernel bad = e.ks[0];
    bad.n_ops = 4;
    CHECK(ngp_kernel_terms(&bad, 0, 16, &cnt, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0) ==
              NGP_ERR_PROGRAM, "malformed program accepted");
}

static void worker(ngp_ctx *ctx, int id, int rounds) {
    Ensemble e;
    splitting(e);
    // n = 40: no main block; 85, 130, 175: tails 21, 2, 47.  d = 2, 9, 16, 23 and D = 1, 3, 5, 7;
    // the last worker eliminates 47 + 23 = 70 rows, and every worker once more with da > 76 (the
    // working set then lives in the per-item buffer)
    const int P = 3, n = 40 + 45 * id, m = 3 + id, d = 2 + 7 * id, D = 1 + 2 * id;
    std::vector<double> t(n), y(n), t_new(m), t_add(64), y_add((size_t)D * 64);
    for (int i = 0; i < n; ++i) { t[i] = (double)i / (n - 1); y[i] = std::sin(9.0 * t[i]); }
    for (int i = 0; i < 64; ++i) t_add[i] = 1.0 + (double)(i + 1) / (n - 1);
    for (size_t i = 0; i < y_add.size(); ++i) y_add[i] = std::cos(0.3 * (double)i);
    for (int i = 0; i < m; ++i) t_new[i] = 2.0 + (double)(i + 1) / (n - 1);
    // the term programs, particle-major
    std::vector<Terms> terms(P);
    std::vector<ngp_kernel> comps;
    int32_t counts[3];
    for (int k = 0; k < P; ++k) {
        Terms &tk = terms[k];
        CHECK(ngp_kernel_terms(&e.ks[k], NGP_SPLIT_CHANGEPOINT | NGP_SPLIT_TIMES, 16, &tk.cnt, tk.of, tk.ol, tk.pf,
                               tk.pl, tk.ops, 16 * 8, tk.par, 16 * 12) == NGP_OK, "terms");
        counts[k] = tk.cnt;
        for (int i = 0; i < tk.cnt; ++i)
            comps.push_back(ngp_kernel{tk.ol[i], tk.pl[i], tk.ops + tk.of[i], tk.par + tk.pf[i], 99.0});
    }
    const size_t tot = comps.size();
    size_t nsig = 0;
    for (int k = 0; k < P; ++k) nsig += (size_t)counts[k] * m * counts[k] * m;
    std::vector<double> mu(tot * D * m), var(tot * m), sg(nsig), lf((size_t)P * D);
    std::vector<int32_t> info(P);
    for (int r = 0; r < rounds; ++r) {
        CHECK(ngp_set_structured_storage(ctx, (r + id) & 1) == NGP_OK, "set_structured_storage");
        CHECK(ngp_profile_enable(ctx, r & 1) == NGP_OK, "profile_enable");
        ngp_factor *f = nullptr;
        CHECK(ngp_factor_create(ctx, P, e.ks, n, t.data(), y.data(), 0, &f) == NGP_OK && f, "factor_create");
        if (!f) continue;
        auto call = [&](ngp_factor *f_, int d_, const double *ta, int D_, const double *ya, const int32_t *cc,
                        const ngp_kernel *cs, int m_, const double *tn, double *mu_) {
            return ngp_factor_components_nowcast(f_, d_, ta, D_, ya, cc, cs, m_, tn, lf.data(), mu_, sg.data(),
                                                 var.data(), info.data());
        };
        CHECK(call(f, d, t_add.data(), D, y_add.data(), counts, comps.data(), m, t_new.data(), mu.data()) == NGP_OK,
              "factor_components_nowcast");
        CHECK(ngp_factor_components_nowcast(f, d, t_add.data(), D, y_add.data(), counts, comps.data(), m,
                                            t_new.data(), nullptr, mu.data(), nullptr, var.data(), nullptr) ==
                  NGP_OK, "factor_components_nowcast (mu and var alone)");
        CHECK(ngp_factor_components_nowcast(f, d, t_add.data(), D, y_add.data(), counts, comps.data(), m,
                                            t_new.data(), lf.data(), mu.data(), nullptr, nullptr, info.data()) ==
                  NGP_OK, "factor_components_nowcast (mu alone)");
        CHECK(call(f, 0, nullptr, 1, nullptr, counts, comps.data(), m, t_new.data(), mu.data()) == NGP_OK,
              "no appended points refused");
        // more rows to eliminate than the epilogue keeps in LDS: tail + d > 76
        const int d_big = 77 - n % 64 > 0 ? 77 - n % 64 : 1;
        if (n % 64 + d_big + 1 + 4 * m <= NGP_MAX_AUX && d_big <= 64)
            CHECK(call(f, d_big, t_add.data(), 1, y_add.data(), counts, comps.data(), m, t_new.data(), mu.data()) ==
                      NGP_OK, "a long appended block refused");
        // malformed calls: refused, nothing left behind
        CHECK(call(nullptr, d, t_add.data(), D, y_add.data(), counts, comps.data(), m, t_new.data(), mu.data()) ==
                  NGP_ERR_ARG, "null factor accepted");
        CHECK(call(f, -1, t_add.data(), D, y_add.data(), counts, comps.data(), m, t_new.data(), mu.data()) ==
                  NGP_ERR_ARG, "d < 0 accepted");
        CHECK(call(f, d, t_add.data(), 0, y_add.data(), counts, comps.data(), m, t_new.data(), mu.data()) ==
                  NGP_ERR_ARG, "D = 0 accepted");
        CHECK(call(f, d, nullptr, D, y_add.data(), counts, comps.data(), m, t_new.data(), mu.data()) ==
                  NGP_ERR_ARG, "null appended dates accepted");
        CHECK(call(f, d, t_add.data(), D, nullptr, counts, comps.data(), m, t_new.data(), mu.data()) ==
                  NGP_ERR_ARG, "null scenarios accepted");
        CHECK(call(f, d, t_add.data(), D, y_add.data(), nullptr, comps.data(), m, t_new.data(), mu.data()) ==
                  NGP_ERR_ARG, "null counts accepted");
        CHECK(call(f, d, t_add.data(), D, y_add.data(), counts, nullptr, m, t_new.data(), mu.data()) ==
                  NGP_ERR_ARG, "null components accepted");
        CHECK(call(f, d, t_add.data(), D, y_add.data(), counts, comps.data(), m, nullptr, mu.data()) ==
                  NGP_ERR_ARG, "null dates accepted");
        CHECK(call(f, d, t_add.data(), D, y_add.data(), counts, comps.data(), m, t_new.data(), nullptr) ==
                  NGP_ERR_ARG, "null means accepted");
        CHECK(call(f, d, t_add.data(), D, y_add.data(), counts, comps.data(), 0, t_new.data(), mu.data()) ==
                  NGP_ERR_ARG, "m = 0 accepted");
        int32_t zero[3] = {counts[0], 0, counts[2]};
        CHECK(call(f, d, t_add.data(), D, y_add.data(), zero, comps.data(), m, t_new.data(), mu.data()) ==
                  NGP_ERR_ARG, "C_p = 0 accepted");
        std::vector<ngp_kernel> broken = comps;
        broken[tot - 1].n_params -= 1;
        CHECK(call(f, d, t_add.data(), D, y_add.data(), counts, broken.data(), m, t_new.data(), mu.data()) ==
                  NGP_ERR_PROGRAM, "malformed component accepted");
        // the aux limit, exactly and one row over: (n mod 64) + d + 1 + C m <= NGP_MAX_AUX with C = 4
        const int room = NGP_MAX_AUX - n % 64 - d - 1, m_fit = room / 4, m_over = m_fit + 1;
        std::vector<double> tl(m_over), mul(tot * D * m_over);
        for (int i = 0; i < m_over; ++i) tl[i] = 2.0 + (double)(i + 1) / (n - 1);
        CHECK(ngp_factor_components_nowcast(f, d, t_add.data(), D, y_add.data(), counts, comps.data(), m_fit,
                                            tl.data(), lf.data(), mul.data(), nullptr, nullptr, info.data()) ==
                  NGP_OK, "the largest horizon refused");
        CHECK(ngp_factor_components_nowcast(f, d, t_add.data(), D, y_add.data(), counts, comps.data(), m_over,
                                            tl.data(), lf.data(), mul.data(), nullptr, nullptr, info.data()) ==
                  NGP_ERR_TOO_LARGE, "one row over the limit accepted");
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
    std::printf("components_nowcast_stress: %ld kernel launches issued, %d failures\n", mock_hip_launches(),
                fails.load());
    return fails.load() ? 1 : 0;
}

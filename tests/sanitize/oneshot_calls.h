// The one-shot device calls of the C-ABI at small fixed shapes: the table that oneshot_trace.cpp
// records and oneshot_faults.cpp breaks.  A one-shot call takes the context, allocates a few device
// blocks, copies up, launches, copies down, synchronises and gives the blocks back, all inside one
// call.  The component and long-horizon queries need a resident factor: `setup` makes it and
// `teardown` destroys it, outside of what is recorded or broken.
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/ngp.h"

namespace oneshot {

struct Entry {
    std::string name;
    std::function<ngp_status(ngp_ctx *)> call;
    std::function<ngp_status(ngp_ctx *)> setup;   // may be empty
    std::function<void()> teardown;               // may be empty
    // the call's first copies that are those of the job it stages: that code reports a failed copy
    // as NGP_ERR_STATE, every other copy of a one-shot call as the HIP code
    long job_copies = 0;
};

// ---- ngp_cov_batch: B = 3 mixed trees, n1 = 5, n2 = 4 -------------------------------------------
struct Cov {
    int32_t ops0[1] = {NGP_OP_SQEXP}, ops1[3] = {NGP_OP_LINEAR, NGP_OP_SQEXP, NGP_OP_TIMES},
            ops2[5] = {NGP_OP_SQEXP, NGP_OP_PERIODIC, NGP_OP_PLUS, NGP_OP_LINEAR, NGP_OP_TIMES};
    double par0[2] = {0.3, 0.8}, par1[5] = {0.5, 0.1, 0.5, 0.2, 0.7},
           par2[8] = {0.4, 0.6, 0.25, 0.2, 0.4, 0.5, 0.1, 0.5};
    ngp_kernel ks[3];
    double t1[5] = {0.0, 0.125, 0.25, 0.5, 0.75}, t2[4] = {0.0625, 0.25, 0.875, 1.0}, out[3 * 5 * 4];
    Cov() {
        ks[0] = {1, 2, ops0, par0, 0.05};
        ks[1] = {3, 5, ops1, par1, 0.02};
        ks[2] = {5, 8, ops2, par2, 0.1};
    }
};

// ---- the sampler and the trajectory targets: P = 3, S = 2, m = 5, draws = 8 ---------------------
struct Paths {
    static constexpr int P = 3, S = 2, m = 5, draws = 8, T = 3, Q = 3;
    std::vector<double> w, mu, sigma, sigma_indep, out, q, mean, values;
    std::vector<int32_t> comp, info;
    std::vector<int64_t> count, hist;
    uint64_t seeds[S] = {7u, 9u};
    // one target that has quantiles, the first date of the maximum, an exceedance
    ngp_path_target tg[T] = {{NGP_TARGET_SUM, 0, m - 1, 0.0}, {NGP_TARGET_ARGMAX, 1, 3, 0.0},
                             {NGP_TARGET_EXCEED, 0, 2, 1.5}};
    double probs[Q] = {0.45, 0.5, 0.9};   // N = 16 paths: ranks 8, 8, 15
    ngp_inv_transform inv = {NGP_INV_BOXCOX, -0.3, 0.25, 1.0e4};
    Paths() {
        w.assign((size_t)S * P, 1.0 / P);
        mu.assign((size_t)P * S * m, 0.5);
        auto diag = [&](std::vector<double> &sg, size_t mats) {
            sg.assign(mats * m * m, 0.0);
            for (size_t k = 0; k < mats; ++k)
                for (int j = 0; j < m; ++j) sg[(k * m + j) * m + j] = 0.04 + 0.01 * (double)k;
        };
        diag(sigma, P);
        diag(sigma_indep, (size_t)S * P);
        out.assign((size_t)S * draws * m, 0.0);
        comp.assign((size_t)S * draws, 0);
        info.assign((size_t)S * P, 0);
        q.assign((size_t)T * Q, 0.0);
        mean.assign(T, 0.0);
        count.assign(T, 0);
        hist.assign((size_t)T * m, 0);
        values.assign((size_t)T * S * draws, 0.0);
    }
    ngp_status sample(ngp_ctx *c, bool extras) {
        return ngp_mixture_sample(c, P, S, m, w.data(), mu.data(), sigma.data(), draws, 11u, out.data(),
                                  extras ? comp.data() : nullptr, extras ? info.data() : nullptr);
    }
    ngp_status sample_indep(ngp_ctx *c, bool extras) {
        return ngp_mixture_sample_indep(c, P, S, m, w.data(), mu.data(), sigma_indep.data(), draws, seeds,
                                        out.data(), extras ? comp.data() : nullptr,
                                        extras ? info.data() : nullptr);
    }
    ngp_status targets(ngp_ctx *c, bool with_values) {
        return ngp_mixture_path_targets(c, P, S, m, w.data(), mu.data(), sigma.data(), draws, 11u, &inv, T, tg,
                                        Q, probs, q.data(), mean.data(), count.data(), hist.data(),
                                        with_values ? values.data() : nullptr, info.data());
    }
    ngp_status targets_indep(ngp_ctx *c, bool with_values) {
        return ngp_mixture_path_targets_indep(c, P, S, m, w.data(), mu.data(), sigma_indep.data(), draws,
                                              seeds, &inv, T, tg, Q, probs, q.data(), mean.data(),
                                              count.data(), hist.data(),
                                              with_values ? values.data() : nullptr, info.data());
    }
    // the paths scored on the natural scale, the fair estimator: one date, all dates
    double y[m] = {0.75, 1.0, 1.25, 1.5, 1.75}, es[2], term_obs[2], term_pair[2];
    int32_t win[4] = {2, 2, 0, m - 1}, winfo[2];
    ngp_status scores(ngp_ctx *c, bool indep, bool with_chol_info) {
        return ngp_mixture_path_scores(c, P, S, m, w.data(), mu.data(), indep ? sigma_indep.data() : sigma.data(),
                                       indep ? 1 : 0, draws, seeds, &inv, y, NGP_SCORE_NATURAL, 0.0, 1, 2, win,
                                       es, term_obs, term_pair, winfo, with_chol_info ? info.data() : nullptr);
    }
};

// ---- the scores of paths the caller hands in: N = 16, m = 5, W = 2 (one date, all dates) --------
struct Ens {
    static constexpr int N = 16, m = 5, W = 2;
    double x[N * m], y[m] = {0.75, 1.0, 1.25, 1.5, 1.75}, es[W], term_obs[W], term_pair[W];
    int32_t win[2 * W] = {2, 2, 0, m - 1}, info[W];
    Ens() {
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < m; ++j) x[i * m + j] = 0.5 + 0.125 * ((i * 7 + j * 3) % 11);
    }
    ngp_status scores(ngp_ctx *c, bool log_scale) {
        return ngp_ensemble_scores(c, N, m, x, y, log_scale ? NGP_SCORE_LOG : NGP_SCORE_NATURAL,
                                   log_scale ? 0.5 : 0.0, log_scale ? 1 : 0, W, win, es, term_obs, term_pair, info);
    }
};

// ---- the summaries: C = 5 with one zero weight, m = 7, K = Q = 3, one date with a bad component --
struct Mix {
    static constexpr int C = 5, m = 7, K = 3;
    double w[C] = {0.3, 0.0, 0.2, 0.4, 0.1}, mu[C * m], var[C * m], x[m * K], probs[K] = {0.1, 0.5, 0.9},
           y[m], res[m * K], mean[m], err[m];
    int32_t info[m];
    ngp_inv_transform ident = {NGP_INV_IDENTITY, 0.0, 0.0, 0.0}, boxcox = {NGP_INV_BOXCOX, 0.5, 0.25, 1.0e4};
    Mix() {
        for (int c = 0; c < C; ++c)
            for (int j = 0; j < m; ++j) {
                mu[c * m + j] = 1.0 + 0.25 * c + 0.125 * j;
                var[c * m + j] = 0.04 + 0.01 * ((c + j) % 3);
            }
        var[2 * m + 4] = -1.0;             // component 2 (positive weight) is bad on date 4
        for (int j = 0; j < m; ++j) {
            y[j] = 1.5 + 0.125 * j;
            for (int k = 0; k < K; ++k) x[j * K + k] = 1.0 + 0.5 * k + 0.125 * j;
        }
    }
    ngp_status cdf(ngp_ctx *c) { return ngp_mixture_cdf(c, C, m, w, mu, var, K, x, res, info); }
    ngp_status quantiles(ngp_ctx *c) { return ngp_mixture_quantiles(c, C, m, w, mu, var, K, probs, res, info); }
    ngp_status crps(ngp_ctx *c) { return ngp_mixture_crps(c, C, m, w, mu, var, y, res, info); }
    ngp_status mapped(ngp_ctx *c, bool log_scale) {
        return ngp_mixture_crps_mapped(c, C, m, w, mu, var, log_scale ? &boxcox : &ident,
                                       log_scale ? NGP_SCORE_LOG : NGP_SCORE_NATURAL, log_scale ? 0.5 : 0.0, y,
                                       0.0, res, mean, err, info);
    }
};

// ---- the component queries: a resident factor of P = 2, n = 70; d = 0 and d = 2 -----------------
struct Comp {
    static constexpr int P = 2, n = 70, m = 3, d = 2, D = 2;
    int32_t ops0[3] = {NGP_OP_SQEXP, NGP_OP_PERIODIC, NGP_OP_PLUS}, ops1[3] = {NGP_OP_LINEAR, NGP_OP_SQEXP, NGP_OP_TIMES};
    double par0[5] = {0.3, 0.8, 0.4, 0.25, 0.5}, par1[5] = {0.5, 0.1, 0.5, 0.2, 0.7};
    ngp_kernel ks[P], comps[3];
    int32_t counts[P] = {2, 1};
    double t[n], y[n], t_add[d], y_add[D * d], t_new[m];
    // 3 components in all; sigma: 2 m x 2 m and m x m
    double mu[3 * D * m], sigma[(2 * m) * (2 * m) + m * m], var[3 * m], lf[P * D];
    int32_t info[P];
    ngp_factor *f = nullptr;
    Comp() {
        ks[0] = {3, 5, ops0, par0, 0.05};
        ks[1] = {3, 5, ops1, par1, 0.02};
        comps[0] = {1, 2, ops0, par0, 0.0};           // SqExp | Periodic of the first tree
        comps[1] = {1, 3, ops0 + 1, par0 + 2, 0.0};
        comps[2] = ks[1];                             // the second tree is one component
        for (int i = 0; i < n; ++i) { t[i] = i / 128.0; y[i] = ((i * 37) % 11) / 11.0 - 0.5; }
        for (int i = 0; i < d; ++i) t_add[i] = (n + i) / 128.0;
        for (int i = 0; i < D * d; ++i) y_add[i] = 0.1 * (i % 3);
        for (int i = 0; i < m; ++i) t_new[i] = (n + d + i) / 128.0;
    }
    ngp_status create(ngp_ctx *c) { return ngp_factor_create(c, P, ks, n, t, y, 0, &f); }
    void destroy() { ngp_factor_destroy(f); f = nullptr; }
    ngp_status query(bool nowcast) {
        if (!nowcast) return ngp_factor_components(f, counts, comps, m, t_new, mu, sigma, var, info);
        return ngp_factor_components_nowcast(f, d, t_add, D, y_add, counts, comps, m, t_new, lf, mu, sigma, var,
                                             info);
    }
    // the long-horizon query of the same factor: m = 6 dates
    static constexpr int mL = 6;
    double t_long[mL], mu_long[P * D * mL], var_long[P * mL], sigma_long[P * mL * mL];
    ngp_status predict_long(bool appended, bool with_sigma) {
        for (int i = 0; i < mL; ++i) t_long[i] = (n + d + i) / 128.0;
        return ngp_factor_predict_long(f, appended ? d : 0, t_add, D, y_add, mL, t_long, 0, mu_long, var_long,
                                       with_sigma ? sigma_long : nullptr, info);
    }
    // its paths (4 draws; the second particle without weight when nothing is appended), its
    // decomposition (counts 2 | 1) and its hindcasts either side of the main block's end
    static constexpr int drawsL = 4, RL = 5;
    double wL0[P] = {1.0, 0.0}, wL2[D * P] = {0.5, 0.5, 0.25, 0.75}, out_long[D * drawsL * mL];
    double cmu_long[3 * D * mL], cross_long[5 * mL], csigma_long[5 * mL * mL];
    double omu_long[P * RL * mL], ovar_long[P * RL * mL], logml_long[P * RL];
    int32_t cutL[RL] = {1, 63, 64, 65, n}, comp_long[D * drawsL], cinfo_long[P];
    void dates() { for (int i = 0; i < mL; ++i) t_long[i] = (n + d + i) / 128.0; }
    ngp_status sample_long(bool appended) {
        dates();
        return ngp_factor_sample_long(f, appended ? d : 0, t_add, D, y_add, mL, t_long, 1, appended ? wL2 : wL0,
                                      drawsL, 17u, out_long, comp_long, mu_long, var_long, info, cinfo_long);
    }
    ngp_status components_long(bool appended, bool with_sigma) {
        dates();
        return ngp_factor_components_long(f, appended ? d : 0, t_add, D, y_add, counts, comps, mL, t_long, cmu_long,
                                          cross_long, with_sigma ? csigma_long : nullptr, info);
    }
    ngp_status predict_origins(bool with_logml) {
        dates();
        return ngp_factor_predict_origins(f, RL, cutL, mL, t_long, 0, omu_long, ovar_long,
                                          with_logml ? logml_long : nullptr, info);
    }
};

// ---- the long-horizon family: a resident factor of P = 3 with a main block and a tail (n = 191:
// 128 + 63) or without a main block (n = 20); d = 0, and d = 2 with D = 3 --------------------------
struct Long {
    static constexpr int P = 3, d = 2, D = 3, NC = 6, NC2 = 1 + 9 + 4;   // sum C_p, sum C_p^2
    // Plus(Plus(Linear, Periodic), SqExp) | Times(Plus(Linear, Periodic), SqExp) |
    // Plus(ChangePoint(Plus(SqExp, Constant), Periodic), GammaExp)
    int32_t ops0[5] = {2, 5, 6, 3, 6}, ops1[5] = {2, 5, 6, 3, 7}, ops2[7] = {3, 1, 6, 5, 8, 4, 6};
    double par0[8] = {0.2, 0.1, 0.5, 0.9, 0.3, 0.7, 0.21, 0.4};
    double par1[8] = {0.1, 0.3, 0.8, 1.1, 0.21, 0.4, 0.3, 0.6};
    double par2[11] = {0.2, 0.5, 0.25, 1.0, 0.3, 0.3, 0.5, 0.1, 0.3, 1.5, 0.2};
    int32_t lin[1] = {2}, per[1] = {5}, se[1] = {3};
    ngp_kernel ks[P], comps[NC];
    int32_t counts[P] = {1, 3, 2};
    int n, m, draws, R;
    std::vector<double> t, y, t_add, y_add, t_new;
    std::vector<int32_t> cut;
    // d = 0: the middle particle has no weight; d = 2: the last one has none in any scenario
    double w0[P] = {0.5, 0.0, 0.5}, w2[D * P] = {0.5, 0.5, 0.0, 1.0, 0.0, 0.0, 0.25, 0.75, 0.0};
    // every output of a call lies in `host` between two guard bands (cover(), below)
    static constexpr size_t GUARD = 32;
    std::vector<double> host;
    std::vector<int32_t> ihost;
    double *mu = nullptr, *var = nullptr, *sigma = nullptr, *out = nullptr, *cross = nullptr, *logml = nullptr;
    int32_t *info = nullptr, *cinfo = nullptr, *comp = nullptr;
    ngp_factor *f = nullptr;
    Long(int n_, int m_, int draws_ = 4) : n(n_), m(m_), draws(draws_), t(n_), y(n_), t_add(d), y_add(D * d), t_new(m_) {
        ks[0] = {5, 8, ops0, par0, 0.05};
        ks[1] = {5, 8, ops1, par1, 0.02};
        ks[2] = {7, 11, ops2, par2, 0.1};
        comps[0] = ks[0];
        comps[1] = {1, 3, lin, par1, 0.0};
        comps[2] = {1, 3, per, par1 + 3, 0.0};
        comps[3] = {1, 2, se, par1 + 6, 0.0};
        comps[4] = {5, 8, ops2, par2, 0.0};          // ChangePoint(Plus(SqExp, Constant), Periodic)
        comps[5] = {1, 3, ops2 + 5, par2 + 8, 0.0};  // GammaExp
        for (int i = 0; i < n; ++i) { t[i] = i / 256.0; y[i] = ((i * 37) % 11) / 11.0 - 0.5; }
        for (int i = 0; i < d; ++i) t_add[i] = (n + i) / 256.0;
        for (int i = 0; i < D * d; ++i) y_add[i] = 0.1 * (i % 3);
        for (int i = 0; i < m; ++i) t_new[i] = (n + d + i) / 256.0;
        // origins either side of the main block's end (and of its first block row)
        for (int c : {1, 64, 127, 128, 129, 191}) if (c <= n) cut.push_back(c);
        if (cut.back() != n) cut.push_back(n);
        R = (int)cut.size();
        const size_t um = (size_t)m, nd[6] = {(size_t)std::max(NC * D, P * R) * um, (size_t)P * R * um, (size_t)NC2 * um * um,
                                              (size_t)D * draws * um, (size_t)NC2 * um, (size_t)P * R};
        size_t at = GUARD;
        double **pd[6] = {&mu, &var, &sigma, &out, &cross, &logml};
        for (size_t k : nd) at += k + GUARD;
        host.assign(at, 0.0);
        at = GUARD;
        for (int k = 0; k < 6; ++k) { *pd[k] = host.data() + at; at += nd[k] + GUARD; }
        ihost.assign(4 * GUARD + 2 * P + (size_t)D * draws, 0);
        info = ihost.data() + GUARD;
        cinfo = info + P + GUARD;
        comp = cinfo + P + GUARD;
    }
    ngp_status create(ngp_ctx *c) { return ngp_factor_create(c, P, ks, n, t.data(), y.data(), 0, &f); }
    void destroy() { ngp_factor_destroy(f); f = nullptr; }
    ngp_status predict_long(bool appended, bool with_sigma) {
        return ngp_factor_predict_long(f, appended ? d : 0, t_add.data(), D, y_add.data(), m, t_new.data(), 1, mu,
                                       var, with_sigma ? sigma : nullptr, info);
    }
    ngp_status sample_long(bool appended, bool extras = true) {
        return ngp_factor_sample_long(f, appended ? d : 0, t_add.data(), D, y_add.data(), m, t_new.data(), 1,
                                      appended ? w2 : w0, draws, 17u, out, extras ? comp : nullptr,
                                      extras ? mu : nullptr, extras ? var : nullptr, extras ? info : nullptr,
                                      extras ? cinfo : nullptr);
    }
    ngp_status components_long(bool appended, bool with_sigma) {
        return ngp_factor_components_long(f, appended ? d : 0, t_add.data(), D, y_add.data(), counts, comps, m,
                                          t_new.data(), mu, cross, with_sigma ? sigma : nullptr, info);
    }
    ngp_status predict_origins(bool with_logml) {
        return ngp_factor_predict_origins(f, R, cut.data(), m, t_new.data(), 1, mu, var, with_logml ? logml : nullptr,
                                          info);
    }
    // The downloads of a call land at host offsets that depend on the chunk; the trace does not show
    // them.  cover(call, ...) fills everything with a sentinel, runs the call and counts the elements of
    // the named outputs (pointer, length) that are not 0 afterwards — the mock's device memory is zeroed
    // and its copies are memcpy — plus the elements outside them that lost the sentinel.
    struct Span { const void *p; size_t n; };
    long cover(const std::function<ngp_status()> &call, const std::vector<Span> &written, ngp_status *st) {
        const double ds = 7.5;
        const int32_t is = 0x5a5a5a5a;
        std::vector<char> dw(host.size(), 0), iw(ihost.size(), 0);
        for (const Span &s : written) {
            const double *pdbl = static_cast<const double *>(s.p);
            const int32_t *pint = static_cast<const int32_t *>(s.p);
            if (pdbl >= host.data() && pdbl < host.data() + host.size())
                std::fill_n(dw.begin() + (pdbl - host.data()), s.n, 1);
            else
                std::fill_n(iw.begin() + (pint - ihost.data()), s.n, 1);
        }
        std::fill(host.begin(), host.end(), ds);
        std::fill(ihost.begin(), ihost.end(), is);
        *st = call();
        long bad = 0;
        for (size_t i = 0; i < host.size(); ++i) bad += dw[i] ? host[i] != 0.0 : host[i] != ds;
        for (size_t i = 0; i < ihost.size(); ++i) bad += iw[i] ? ihost[i] != 0 : ihost[i] != is;
        return bad;
    }
};

struct Probes {
    double A[64], B[64], D[512], r[4];
    float Af[64], Bf[64], Df[1024];
    Probes() {
        for (int i = 0; i < 64; ++i) { A[i] = 1.0 + i; B[i] = 0.5 - i; Af[i] = (float)A[i]; Bf[i] = (float)B[i]; }
    }
};

inline std::vector<Entry> table() {
    static Cov cov;
    static Paths pa;
    static Mix mx;
    static Comp cq;
    static Ens en;
    static Probes pr;
    auto make = [](ngp_ctx *c) { return cq.create(c); };
    auto drop = [] { cq.destroy(); };
    return {
        {"ngp_cov_batch", [](ngp_ctx *c) { return ngp_cov_batch(c, 3, cov.ks, 5, cov.t1, 4, cov.t2, 1, cov.out); }},
        {"ngp_mixture_sample comp info", [](ngp_ctx *c) { return pa.sample(c, true); }},
        {"ngp_mixture_sample", [](ngp_ctx *c) { return pa.sample(c, false); }},
        {"ngp_mixture_sample_indep comp info", [](ngp_ctx *c) { return pa.sample_indep(c, true); }},
        {"ngp_mixture_sample_indep", [](ngp_ctx *c) { return pa.sample_indep(c, false); }},
        {"ngp_mixture_cdf", [](ngp_ctx *c) { return mx.cdf(c); }},
        {"ngp_mixture_quantiles", [](ngp_ctx *c) { return mx.quantiles(c); }},
        {"ngp_mixture_crps", [](ngp_ctx *c) { return mx.crps(c); }},
        {"ngp_mixture_crps_mapped natural identity", [](ngp_ctx *c) { return mx.mapped(c, false); }},
        {"ngp_mixture_crps_mapped log boxcox", [](ngp_ctx *c) { return mx.mapped(c, true); }},
        {"ngp_mixture_path_targets values", [](ngp_ctx *c) { return pa.targets(c, true); }},
        {"ngp_mixture_path_targets", [](ngp_ctx *c) { return pa.targets(c, false); }},
        {"ngp_mixture_path_targets_indep values", [](ngp_ctx *c) { return pa.targets_indep(c, true); }},
        {"ngp_mixture_path_targets_indep", [](ngp_ctx *c) { return pa.targets_indep(c, false); }},
        {"ngp_factor_components", [](ngp_ctx *) { return cq.query(false); }, make, drop, 1},
        {"ngp_factor_components_nowcast", [](ngp_ctx *) { return cq.query(true); }, make, drop, 1},
        {"ngp_selftest_mfma_layout", [](ngp_ctx *c) { return ngp_selftest_mfma_layout(c, pr.A, pr.B, pr.D); }},
        {"ngp_selftest_mfma_f32_layout", [](ngp_ctx *c) { return ngp_selftest_mfma_f32_layout(c, pr.Af, pr.Bf, pr.Df); }},
        {"ngp_microbench_mfma_f64", [](ngp_ctx *c) { return ngp_microbench_mfma_f64(c, 1, pr.r); }},
        {"ngp_microbench_mfma_f64_detail", [](ngp_ctx *c) { return ngp_microbench_mfma_f64_detail(c, 1, 1, pr.r); }},
        {"ngp_microbench_mixture_pairs", [](ngp_ctx *c) { return ngp_microbench_mixture_pairs(c, 1, pr.r); }},
        {"ngp_microbench_hbm", [](ngp_ctx *c) { return ngp_microbench_hbm(c, 4096, pr.r, pr.r + 1); }},
        {"ngp_ensemble_scores natural", [](ngp_ctx *c) { return en.scores(c, false); }},
        {"ngp_ensemble_scores log shift", [](ngp_ctx *c) { return en.scores(c, true); }},
        {"ngp_mixture_path_scores chol_info", [](ngp_ctx *c) { return pa.scores(c, false, true); }},
        {"ngp_mixture_path_scores", [](ngp_ctx *c) { return pa.scores(c, false, false); }},
        {"ngp_mixture_path_scores indep chol_info", [](ngp_ctx *c) { return pa.scores(c, true, true); }},
        {"ngp_mixture_path_scores indep", [](ngp_ctx *c) { return pa.scores(c, true, false); }},
        {"ngp_factor_predict_long d=0 sigma", [](ngp_ctx *) { return cq.predict_long(false, true); }, make, drop},
        {"ngp_factor_predict_long d=0", [](ngp_ctx *) { return cq.predict_long(false, false); }, make, drop},
        {"ngp_factor_predict_long d=2 sigma", [](ngp_ctx *) { return cq.predict_long(true, true); }, make, drop},
        {"ngp_factor_predict_long d=2", [](ngp_ctx *) { return cq.predict_long(true, false); }, make, drop},
        {"ngp_factor_sample_long d=0", [](ngp_ctx *) { return cq.sample_long(false); }, make, drop},
        {"ngp_factor_sample_long d=2", [](ngp_ctx *) { return cq.sample_long(true); }, make, drop},
        {"ngp_factor_components_long d=0", [](ngp_ctx *) { return cq.components_long(false, false); }, make, drop},
        {"ngp_factor_components_long d=2 sigma", [](ngp_ctx *) { return cq.components_long(true, true); }, make, drop},
        {"ngp_factor_predict_origins logml", [](ngp_ctx *) { return cq.predict_origins(true); }, make, drop},
        {"ngp_factor_predict_origins", [](ngp_ctx *) { return cq.predict_origins(false); }, make, drop},
    };
}

// the long-horizon family on the two factors of Long: n = 191 with m = 70 dates (two blocks of sigma
// for the sampler), n = 20 with m = 6
inline std::vector<Entry> long_table() {
    static Long l191(191, 70), l20(20, 6);
    std::vector<Entry> all;
    for (Long *lp : {&l191, &l20}) {
        Long &l = *lp;
        auto make = [&l](ngp_ctx *c) { return l.create(c); };
        auto drop = [&l] { l.destroy(); };
        const std::string at = " n=" + std::to_string(l.n);
        auto add = [&](const char *name, std::function<ngp_status()> call) {
            all.push_back({name + at, [call](ngp_ctx *) { return call(); }, make, drop});
        };
        add("ngp_factor_sample_long d=0", [&l] { return l.sample_long(false); });
        add("ngp_factor_sample_long d=2 D=3", [&l] { return l.sample_long(true); });
        add("ngp_factor_sample_long d=2 D=3 out alone", [&l] { return l.sample_long(true, false); });
        add("ngp_factor_components_long d=0 sigma", [&l] { return l.components_long(false, true); });
        add("ngp_factor_components_long d=0", [&l] { return l.components_long(false, false); });
        add("ngp_factor_components_long d=2 D=3 sigma", [&l] { return l.components_long(true, true); });
        add("ngp_factor_components_long d=2 D=3", [&l] { return l.components_long(true, false); });
        add("ngp_factor_predict_origins logml", [&l] { return l.predict_origins(true); });
        add("ngp_factor_predict_origins", [&l] { return l.predict_origins(false); });
    }
    return all;
}

}  // namespace oneshot

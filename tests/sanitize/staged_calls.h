// The staged paths of the C-ABI as sequences of steps at the smallest shapes that still take each
// route: the table that staged_trace.cpp records and staged_faults.cpp breaks.  A sequence owns its
// job; its last step destroys it.  A stage step destroys the job of an earlier stage first, so every
// step can be repeated on the job the steps before it left.
#pragma once
#include <climits>
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ngp.h"

namespace staged {

struct Step {
    std::string name;
    std::function<ngp_status(ngp_ctx *)> call;
    // the first copies of the step that are staging copies of a job: a failed one is NGP_ERR_STATE,
    // every other failed copy of a step the HIP code
    long state_copies = 0;
    // the first copies of the step that belong to work done once per job (the maps of a job's first
    // trajectory): when one of them fails, the repeat is a first call again, not a re-run
    long once_copies = 0;
    // an ordinary re-run of the step, where that is more than the call again (new parameters first)
    std::function<ngp_status(ngp_ctx *)> rerun;
};
struct Sequence {
    std::string name;
    std::vector<Step> steps;   // the last one destroys the job and cannot fail
};

struct Data {   // a regular series (step 1 / 128: a lattice) or one pushed off every lattice
    std::vector<double> t, y, t_add, y_add, t_new;
    Data(int n, int d, int D, int m, bool lattice = true) {
        auto at = [&](int i) {
            const double x = i * 0.6180339887498949;
            return (i + (lattice ? 0.0 : 0.3 * (x - (double)(long)x))) / 128.0;
        };
        for (int i = 0; i < n; ++i) { t.push_back(at(i)); y.push_back(((i * 37) % 11) / 11.0 - 0.5); }
        for (int i = 0; i < d; ++i) t_add.push_back(at(n + i));
        for (int i = 0; i < D * d; ++i) y_add.push_back(0.1 * (i % 3));
        for (int i = 0; i < m; ++i) t_new.push_back(at(n + d + i));
    }
};

struct Trees {   // item i: stationary (SqExp + Periodic) or not (Linear x SqExp), by `stationary(i)`
    std::vector<std::vector<int32_t>> ops;
    std::vector<std::vector<double>> par;
    std::vector<ngp_kernel> ks;
    std::vector<double> params, noise;   // the caller's flat parameter vector, moved a little
    Trees(int B, std::function<bool(int)> stationary) : ops((size_t)B), par((size_t)B), ks((size_t)B) {
        for (int i = 0; i < B; ++i) {
            if (stationary(i)) {
                ops[(size_t)i] = {NGP_OP_SQEXP, NGP_OP_PERIODIC, NGP_OP_PLUS};
                par[(size_t)i] = {0.3 + 0.01 * i, 0.8, 0.4, 0.25, 0.5};
            } else {
                ops[(size_t)i] = {NGP_OP_LINEAR, NGP_OP_SQEXP, NGP_OP_TIMES};
                par[(size_t)i] = {0.5, 0.1, 0.5, 0.2 + 0.01 * i, 0.7};
            }
            ks[(size_t)i] = ngp_kernel{3, 5, ops[(size_t)i].data(), par[(size_t)i].data(), 0.02 + 0.01 * i};
            for (double p : par[(size_t)i]) params.push_back(1.0625 * p);
            noise.push_back(0.03 + 0.01 * i);
        }
    }
};

// ---- value jobs: ngp_nowcast_stage -> ngp_job_run -> ngp_job_run -> ngp_job_fetch -> destroy ------
struct Value {
    int P, n, d, D, m, precision;
    Trees tr;
    Data s;
    ngp_job *job = nullptr;
    std::vector<double> lb, lf, mu, sigma;
    std::vector<int32_t> info;
    Value(int P_, int n_, int d_, int D_, int m_, int precision_ = NGP_PREC_F64)
        : P(P_), n(n_), d(d_), D(D_), m(m_), precision(precision_), tr(P_, [](int i) { return i % 2 == 0; }),
          s(n_, d_, D_, m_), lb((size_t)P_), lf((size_t)P_ * D_), mu((size_t)P_ * D_ * m_),
          sigma((size_t)P_ * m_ * m_), info((size_t)P_) {}
    ngp_status stage(ngp_ctx *c) {
        ngp_job_destroy(job);
        job = nullptr;
        ngp_spec old, sp;
        ngp_status st = ngp_get_spec(c, &old);
        if (st) return st;
        sp = old;
        sp.precision = precision;   // a staged job keeps the spec it was staged under
        if ((st = ngp_set_spec(c, &sp))) return st;
        st = ngp_nowcast_stage(c, P, tr.ks.data(), n, s.t.data(), s.y.data(), d, s.t_add.data(), D,
                               s.y_add.data(), m, s.t_new.data(), 1, &job);
        (void)ngp_set_spec(c, &old);
        return st;
    }
    ngp_status run() { return ngp_job_run(job); }
    ngp_status fetch() { return ngp_job_fetch(job, lb.data(), lf.data(), mu.data(), sigma.data(), info.data()); }
    ngp_status destroy() { ngp_job_destroy(job); job = nullptr; return NGP_OK; }
};
inline Sequence value_sequence(const std::string &name, std::shared_ptr<Value> v) {
    return {name,
            {{"ngp_nowcast_stage", [v](ngp_ctx *c) { return v->stage(c); }, LONG_MAX},
             {"ngp_job_run", [v](ngp_ctx *) { return v->run(); }},
             {"ngp_job_run again", [v](ngp_ctx *) { return v->run(); }},
             {"ngp_job_fetch", [v](ngp_ctx *) { return v->fetch(); }},
             {"ngp_job_destroy", [v](ngp_ctx *) { return v->destroy(); }}}};
}

// ---- a resident factor: ngp_factor_create -> ngp_factor_nowcast -> destroy -----------------------
struct Factor {
    static constexpr int P = 3, n = 136, d = 2, D = 2, m = 3;
    Trees tr{P, [](int i) { return i % 2 == 0; }};
    Data s{n, d, D, m};
    ngp_factor *f = nullptr;
    double lb[P], lf[P * D], mu[P * D * m], sigma[P * m * m];
    int32_t info[P];
    ngp_status create(ngp_ctx *c) {
        ngp_factor_destroy(f);
        f = nullptr;
        return ngp_factor_create(c, P, tr.ks.data(), n, s.t.data(), s.y.data(), 0, &f);
    }
    ngp_status nowcast() {
        return ngp_factor_nowcast(f, d, s.t_add.data(), D, s.y_add.data(), m, s.t_new.data(), 1, lb, lf, mu, sigma,
                                  info);
    }
    ngp_status destroy() { ngp_factor_destroy(f); f = nullptr; return NGP_OK; }
};

// ---- gradient jobs: ngp_grad_stage -> run -> set_params -> run -> destroy; trajectories ----------
struct Grad {
    int B, n;
    bool invariant;   // staged on a batch-invariant context: a small mixed batch then runs its leaves side by side
    Trees tr;
    Data s;
    ngp_grad_job *job = nullptr;
    std::vector<double> lm, g, z0, mom, z1, mom1, theta1, sc, trace;
    std::vector<int32_t> info;
    std::vector<uint8_t> kind;
    ngp_hmc_config cfg{};
    Grad(int B_, int n_, std::function<bool(int)> stationary, bool lattice, bool invariant_ = false)
        : B(B_), n(n_), invariant(invariant_), tr(B_, stationary), s(n_, 0, 1, 0, lattice), lm((size_t)B_),
          g((size_t)B_ * 6), z0((size_t)B_ * 6, 0.125), mom((size_t)B_ * 6, 0.25), z1((size_t)B_ * 6),
          mom1((size_t)B_ * 6), theta1((size_t)B_ * 6), sc((size_t)B_ * 5), trace((size_t)B_ * 6 * 3),
          info((size_t)B_), kind((size_t)B_ * 6, 0) {
        cfg.n_leapfrog = 2;
        cfg.eps = 0.01;
        for (int k = 0; k < 5; ++k) { cfg.prior_mu[k] = 0.0; cfg.prior_sigma[k] = 1.0; }
    }
    ngp_status stage(ngp_ctx *c) {
        ngp_grad_job_destroy(job);
        job = nullptr;
        if (invariant) (void)ngp_set_batch_invariant(c, 1);
        const ngp_status st = ngp_grad_stage(c, B, tr.ks.data(), n, s.t.data(), s.y.data(), 0, &job);
        if (invariant) (void)ngp_set_batch_invariant(c, 0);
        return st;
    }
    ngp_status run() { return ngp_grad_job_run(job, lm.data(), g.data(), info.data()); }
    ngp_status set_run() {
        const ngp_status st = ngp_grad_job_set_params(job, tr.params.data(), tr.noise.data());
        return st ? st : run();
    }
    ngp_status hmc(bool with_trace) {
        double *o = sc.data();
        return ngp_grad_job_hmc(job, &cfg, kind.data(), nullptr, z0.data(), mom.data(), z1.data(), mom1.data(),
                                theta1.data(), o, o + B, o + 2 * B, o + 3 * B, o + 4 * B, info.data(),
                                with_trace ? trace.data() : nullptr);
    }
    ngp_status destroy() { ngp_grad_job_destroy(job); job = nullptr; return NGP_OK; }
};
inline Sequence grad_sequence(const std::string &name, std::shared_ptr<Grad> q) {
    auto set_run = [q](ngp_ctx *) { return q->set_run(); };
    return {name,
            {{"ngp_grad_stage", [q](ngp_ctx *c) { return q->stage(c); }, LONG_MAX},
             // (an ordinary re-run of a gradient job is one with new parameters: the programs go up)
             {"ngp_grad_job_run", [q](ngp_ctx *) { return q->run(); }, 0, 0, set_run},
             {"ngp_grad_job_set_params + ngp_grad_job_run", set_run},
             {"ngp_grad_job_destroy", [q](ngp_ctx *) { return q->destroy(); }}}};
}

inline std::vector<Sequence> table() {
    auto factor = std::make_shared<Factor>();
    // dates off every lattice: the new programs of a re-run travel as a copy of their own
    auto hmc = std::make_shared<Grad>(3, 70, [](int) { return false; }, false);
    // 1 MiB of results is the limit of the packed fetch: 5 items x 170 x 170 forecast covariances pass it
    return {
        value_sequence("value job P=3 n=136 d=2 D=2 m=3", std::make_shared<Value>(3, 136, 2, 2, 3)),
        value_sequence("value job P=5 n=136 d=2 D=2 m=170, results above the packed fetch",
                       std::make_shared<Value>(5, 136, 2, 2, 170)),
        value_sequence("value job P=3 n=128 d=2 D=2 m=3, NGP_PREC_MIXED refined",
                       std::make_shared<Value>(3, 128, 2, 2, 3, NGP_PREC_MIXED)),
        value_sequence("value job P=3 n=40 d=2 D=2 m=3, no main block", std::make_shared<Value>(3, 40, 2, 2, 3)),
        {"resident factor P=3 n=136",
         {{"ngp_factor_create", [factor](ngp_ctx *c) { return factor->create(c); }, 1},
          {"ngp_factor_nowcast d=2 D=2 m=3", [factor](ngp_ctx *) { return factor->nowcast(); }, 1},
          {"ngp_factor_destroy", [factor](ngp_ctx *) { return factor->destroy(); }}}},
        grad_sequence("gradient job B=3 n=70, non-stationary trees, dates off the lattice",
                      std::make_shared<Grad>(3, 70, [](int) { return false; }, false)),
        grad_sequence("gradient job B=4 n=260, stationary and non-stationary trees side by side",
                      std::make_shared<Grad>(4, 260, [](int i) { return i % 2 == 0; }, true, true)),
        {"trajectories B=3 n=70 n_leapfrog=2",
         {{"ngp_grad_stage", [hmc](ngp_ctx *c) { return hmc->stage(c); }, LONG_MAX},
          {"ngp_grad_job_hmc with a trace", [hmc](ngp_ctx *) { return hmc->hmc(true); }, 0, 1},
          {"ngp_grad_job_hmc", [hmc](ngp_ctx *) { return hmc->hmc(false); }},
          {"ngp_grad_job_destroy", [hmc](ngp_ctx *) { return hmc->destroy(); }}}},
    };
}

}  // namespace staged

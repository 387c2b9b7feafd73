// ngp_host_combine.h — flat combining of concurrent one-shot callers: ngp_comb_req, comb_key /
// comb_same, comb_run_one / comb_run_group, comb_execute, combine_submit, ngp_set_combining,
// ngp_combine_stats, and the entry points that are requests: ngp_logml_batch, ngp_predict_batch,
// ngp_logml_grad_batch, ngp_grad_job_run, ngp_mixture_sample.
// Included from ngp_api.hip behind that file's own code (ngp_ctx, which declares ngp_comb_req and
// holds the queue and its switches; check_program; stage_general, ngp_job_run / _fetch / _destroy,
// logml_direct, predict_direct; ngp_grad_job, GradRoute with grad_route_of / grad_route_same,
// logml_grad_direct, grad_job_run_resident) and behind ngp_host_mixture.h (MixInput,
// mixture_sample_impl): a group of one runs on exactly those.
#pragma once

// ---------------------------------------------------------------------------------------
// Combining concurrent callers (flat combining)
//
// The reference enters the boundary from one task per nowcast scenario (Threads.@spawn,
// src/forecasting.jl:131-159): D tasks, each with the P particles of its own clone, all on the same
// dates.  Serialised on the context they are D calls of P items — the small-batch regime D times
// over.  Here a one-shot call (ngp_logml_batch, ngp_predict_batch, ngp_logml_grad_batch,
// ngp_mixture_sample with S = 1) is a REQUEST: it joins `pending`; whoever finds nobody serving takes
// everything that is pending, sorts it into groups of compatible requests — same entry point, same
// series length, bytewise identical dates (a hash, then memcmp), same forecast dates / flags — and
// runs every group as ONE launch sequence over the concatenated items with per-item observation
// rows (the `ldy = n` form every entry point already has; a group of one takes the unchanged
// one-shot path), scatters the results and wakes the callers.  No timer and no extra thread:
// requests pile up by themselves while the device is busy with the previous sequence.  A server
// that has finished its own request hands the role to the first waiter, so nobody serves forever.
// Requests that are not compatible run in arrival order, as before; staged jobs, resident factors
// and the collective do not combine (they take ctx->mu as they always did).
// A merged group that fails as a whole (device memory, a HIP error) is re-run request by request,
// so every caller gets the status its own call would have had.
// ---------------------------------------------------------------------------------------
enum { CK_LOGML = 0, CK_PREDICT = 1, CK_GRAD = 2, CK_MIXTURE = 3 };
struct ngp_comb_req {
    int kind = CK_LOGML;
    // CK_LOGML / CK_PREDICT / CK_GRAD
    int32_t B = 0, n = 0, m = 0, noise_on_new = 0;
    const ngp_kernel *k = nullptr;
    const double *t = nullptr, *y = nullptr, *t_new = nullptr;
    int64_t ldy = 0;
    double *logml = nullptr, *grad = nullptr, *mu = nullptr, *sigma = nullptr;
    int32_t *info = nullptr;
    ngp_grad_job *gj = nullptr;   // CK_GRAD from ngp_grad_job_run: alone it runs on its resident inputs
    GradRoute route;              // CK_GRAD: the job's staged spec and switches, or (one-shot calls) the
                                  // context's when the batch is served (comb_execute)
    // CK_MIXTURE (one mixture of P components: ngp_mixture_sample with S = 1)
    int32_t P = 0, draws = 0;
    const double *w = nullptr, *cmu = nullptr, *csigma = nullptr;
    uint64_t seed = 0;
    double *out = nullptr;
    int32_t *comp = nullptr;
    // what must be equal for two requests to share a launch sequence, hashed by the caller
    uint64_t key = 0;
    ngp_status st = NGP_OK;
    bool done = false;
    std::condition_variable cv;
};

namespace {

inline uint64_t fnv_words(uint64_t h, const void *p, size_t bytes) {
    const unsigned char *b = (const unsigned char *)p;
    size_t i = 0;
    for (; i + 8 <= bytes; i += 8) {
        uint64_t w;
        std::memcpy(&w, b + i, 8);
        h = (h ^ w) * 0x100000001b3ull;
        h ^= h >> 29;
    }
    for (; i < bytes; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

uint64_t comb_key(const ngp_comb_req &r) {
    uint64_t h = 0xcbf29ce484222325ull;
    const int32_t head[6] = {r.kind, r.n, r.m, r.noise_on_new, r.P, r.draws};
    h = fnv_words(h, head, sizeof(head));
    if (r.kind != CK_MIXTURE) {
        h = fnv_words(h, r.t, 8 * (size_t)r.n);
        if (r.m > 0) h = fnv_words(h, r.t_new, 8 * (size_t)r.m);
    }
    return h;
}

bool comb_same(const ngp_comb_req &a, const ngp_comb_req &b) {
    if (a.kind != b.kind || a.key != b.key || a.n != b.n || a.m != b.m ||
        a.noise_on_new != b.noise_on_new || a.P != b.P || a.draws != b.draws)
        return false;
    if (a.kind == CK_MIXTURE) return true;
    if (a.kind == CK_GRAD && !grad_route_same(a.route, b.route)) return false;
    if (std::memcmp(a.t, b.t, 8 * (size_t)a.n) != 0) return false;
    return a.m == 0 || std::memcmp(a.t_new, b.t_new, 8 * (size_t)a.m) == 0;
}

// the request alone: the one-shot path as it always was
ngp_status comb_run_one(ngp_ctx *c, ngp_comb_req &r) {
    switch (r.kind) {
    case CK_LOGML: return logml_direct(c, r.B, r.k, r.n, r.t, r.y, r.ldy, r.logml, r.info);
    case CK_PREDICT:
        return predict_direct(c, r.B, r.k, r.n, r.t, r.y, r.ldy, r.m, r.t_new, r.noise_on_new, r.mu,
                              r.sigma, r.logml, r.info);
    case CK_GRAD:
        if (r.gj) return grad_job_run_resident(r.gj, r.logml, r.grad, r.info);
        return logml_grad_direct(c, r.B, r.k, r.n, r.t, r.y, r.ldy, nullptr, r.logml, r.grad, r.info);
    default:
        return mixture_sample_impl(c, MixInput{r.P, 1, r.m, r.draws, r.w, r.cmu, r.csigma, r.seed, nullptr},
                                   r.out, r.comp, r.info);
    }
}

// a group of compatible requests as ONE call; the results go back to every request's own arrays
ngp_status comb_run_group(ngp_ctx *c, const std::vector<ngp_comb_req *> &grp, bool *shared_k) {
    const ngp_comb_req &r0 = *grp[0];
    *shared_k = false;
    if (r0.kind == CK_MIXTURE) {
        // K mixtures of P components each = ngp_mixture_sample_indep with one seed per request
        const size_t K = grp.size(), P = (size_t)r0.P, m = (size_t)r0.m, dr = (size_t)r0.draws;
        std::vector<double> w(K * P), mu(K * P * m), sg(K * P * m * m), out(K * dr * m);
        std::vector<uint64_t> seeds(K);
        std::vector<int32_t> comp(K * dr), info(K * P);
        for (size_t a = 0; a < K; ++a) {
            std::memcpy(w.data() + a * P, grp[a]->w, 8 * P);
            std::memcpy(mu.data() + a * P * m, grp[a]->cmu, 8 * P * m);
            std::memcpy(sg.data() + a * P * m * m, grp[a]->csigma, 8 * P * m * m);
            seeds[a] = grp[a]->seed;
        }
        const MixInput mix{r0.P, (int32_t)K, r0.m, r0.draws, w.data(), mu.data(), sg.data(), 0, seeds.data()};
        const ngp_status st = mixture_sample_impl(c, mix, out.data(), comp.data(), info.data());
        if (st) return st;
        for (size_t a = 0; a < K; ++a) {
            std::memcpy(grp[a]->out, out.data() + a * dr * m, 8 * dr * m);
            if (grp[a]->comp) std::memcpy(grp[a]->comp, comp.data() + a * dr, 4 * dr);
            if (grp[a]->info) std::memcpy(grp[a]->info, info.data() + a * P, 4 * P);
        }
        return NGP_OK;
    }
    // ---- the scenario tasks of the reference's DEFAULT mode (n_mcmc = n_hmc = 0, src/forecasting.jl:120):
    // every task holds a clone of the same model — the same trees and parameters — on the same
    // dates, and its observations differ from the others' only in the appended nowcast points
    // (src/create_nowcast_data.jl:36-37).  K does not depend on y: such a group is ONE factorisation
    // per particle with the tasks' appended observations as scenarios — the shared-K form of
    // ngp_nowcast_batch (SURVEY.md section 8d "dedupe rule") — instead of one per (particle, task).
    // Recognised, not assumed: same kernels byte for byte, one y per request, a common prefix of the
    // observations up to a few last points.  Not under ngp_set_batch_invariant (another route to the
    // same numbers: equal to rounding, not bit for bit).
    bool invariant;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        invariant = c->invariant;
    }
    if ((r0.kind == CK_LOGML || r0.kind == CK_PREDICT) && !invariant) {
        constexpr int SHARED_K_MAX_TAIL = 16;
        bool same = true;
        for (size_t a = 1; a < grp.size() && same; ++a) {
            const ngp_comb_req &r = *grp[a];
            same = r.B == r0.B && r.ldy == 0 && r0.ldy == 0;
            for (int b = 0; same && b < r.B; ++b) {
                const ngp_kernel &ka = r0.k[b], &kb = r.k[b];
                same = ka.n_ops == kb.n_ops && ka.n_params == kb.n_params && ka.noise == kb.noise &&
                       std::memcmp(ka.ops, kb.ops, 4 * (size_t)ka.n_ops) == 0 &&
                       (ka.n_params == 0 || std::memcmp(ka.params, kb.params, 8 * (size_t)ka.n_params) == 0);
            }
        }
        int npre = r0.n;   // observations every request shares
        for (size_t a = 1; a < grp.size() && same; ++a) {
            int i = 0;
            while (i < npre && grp[a]->y[i] == r0.y[i]) ++i;
            npre = i;
        }
        int dt = std::max(r0.n - npre, 1);
        npre = r0.n - dt;
        if (same && grp[0]->ldy == 0 && dt <= SHARED_K_MAX_TAIL && npre >= 1 &&
            (npre % NB) + dt + r0.m + 1 <= NGP_MAX_AUX) {
            const size_t P = (size_t)r0.B, D = grp.size(), m = (size_t)r0.m;
            std::vector<double> yadd(D * (size_t)dt), lf(P * D), mu(P * D * m), sg(P * m * m);
            std::vector<int32_t> info(P);
            for (size_t a = 0; a < D; ++a) std::memcpy(yadd.data() + a * dt, grp[a]->y + npre, 8 * (size_t)dt);
            ngp_job *job = nullptr;
            ngp_status st = stage_general(c, (int)P, r0.k, npre, r0.t, r0.y, 0, dt, r0.t + npre, (int)D,
                                          yadd.data(), 0, r0.m, r0.t_new, r0.noise_on_new, &job);
            if (!st) {
                st = ngp_job_run(job);
                if (!st) st = ngp_job_fetch(job, nullptr, lf.data(), m ? mu.data() : nullptr,
                                            m ? sg.data() : nullptr, info.data());
                ngp_job_destroy(job);
            }
            if (st) return st;
            for (size_t a = 0; a < D; ++a) {
                ngp_comb_req *r = grp[a];
                for (size_t b = 0; b < P; ++b) {
                    if (r->logml) r->logml[b] = lf[b * D + a];
                    if (m && r->mu) std::memcpy(r->mu + b * m, mu.data() + (b * D + a) * m, 8 * m);
                }
                if (m && r->sigma) std::memcpy(r->sigma, sg.data(), 8 * P * m * m);
                if (r->info) std::memcpy(r->info, info.data(), 4 * P);
            }
            *shared_k = true;
            return NGP_OK;
        }
    }
    size_t Bt = 0;
    for (const ngp_comb_req *r : grp) Bt += (size_t)r->B;
    if (Bt > (size_t)0x7fffffff) return NGP_ERR_TOO_LARGE;
    std::vector<ngp_kernel> ks;
    std::vector<const double *> rows;
    ks.reserve(Bt);
    rows.reserve(Bt);
    for (const ngp_comb_req *r : grp)
        for (int b = 0; b < r->B; ++b) {
            ks.push_back(r->k[b]);
            rows.push_back(r->y + (int64_t)b * r->ldy);
        }
    std::vector<double> lm(Bt);
    std::vector<int32_t> info(Bt);
    if (r0.kind == CK_GRAD) {
        size_t ng = 0;
        for (const ngp_kernel &k : ks) ng += (size_t)k.n_params + 1;
        std::vector<double> grad(ng);
        // under the members' own spec and switches (comb_same), not the context's current ones: a
        // job keeps what it was staged under whatever ngp_set_spec did since
        const ngp_status st = logml_grad_direct(c, (int32_t)Bt, ks.data(), r0.n, r0.t, nullptr, 0,
                                                rows.data(), lm.data(), grad.data(), info.data(),
                                                &r0.route);
        if (st) return st;
        size_t b0 = 0, g0 = 0;
        for (ngp_comb_req *r : grp) {
            size_t len = 0;
            for (int b = 0; b < r->B; ++b) len += (size_t)r->k[b].n_params + 1;
            std::memcpy(r->grad, grad.data() + g0, 8 * len);
            if (r->logml) std::memcpy(r->logml, lm.data() + b0, 8 * (size_t)r->B);
            if (r->info) std::memcpy(r->info, info.data() + b0, 4 * (size_t)r->B);
            b0 += (size_t)r->B;
            g0 += len;
        }
        return NGP_OK;
    }
    const size_t m = (size_t)r0.m;
    std::vector<double> mu(Bt * m), sg(Bt * m * m);
    static const double dummy = 0.0;
    ngp_job *job = nullptr;
    ngp_status st = stage_general(c, (int)Bt, ks.data(), r0.n, r0.t, nullptr, 0, 0, &dummy, 1, &dummy, 0,
                                  r0.m, r0.t_new, r0.noise_on_new, &job, rows.data());
    if (st) return st;
    st = ngp_job_run(job);
    if (!st) st = ngp_job_fetch(job, nullptr, lm.data(), m ? mu.data() : nullptr,
                                m ? sg.data() : nullptr, info.data());
    ngp_job_destroy(job);
    if (st) return st;
    size_t b0 = 0;
    for (ngp_comb_req *r : grp) {
        const size_t B = (size_t)r->B;
        if (r->logml) std::memcpy(r->logml, lm.data() + b0, 8 * B);
        if (r->info) std::memcpy(r->info, info.data() + b0, 4 * B);
        if (m && r->mu) std::memcpy(r->mu, mu.data() + b0 * m, 8 * B * m);
        if (m && r->sigma) std::memcpy(r->sigma, sg.data() + b0 * m * m, 8 * B * m * m);
        b0 += B;
    }
    return NGP_OK;
}

// everything one server took from `pending`: groups in order of their first member's arrival
void comb_execute(ngp_ctx *c, const std::vector<ngp_comb_req *> &batch, int64_t stats[6]) {
    {
        // one-shot gradient calls run under the context's spec and switches as they are now (as
        // they would alone); a staged job brought its own (ngp_grad_job_run)
        std::lock_guard<std::mutex> lk(c->mu);
        const GradRoute now = grad_route_of(c);
        for (ngp_comb_req *r : batch)
            if (r->kind == CK_GRAD && !r->gj) r->route = now;
    }
    std::vector<char> taken(batch.size(), 0);
    for (size_t i = 0; i < batch.size(); ++i) {
        if (taken[i]) continue;
        std::vector<ngp_comb_req *> grp{batch[i]};
        taken[i] = 1;
        for (size_t j = i + 1; j < batch.size(); ++j)
            if (!taken[j] && comb_same(*batch[i], *batch[j])) {
                grp.push_back(batch[j]);
                taken[j] = 1;
            }
        stats[0] += (int64_t)grp.size();
        if (grp.size() > 1) {
            bool shared_k = false;
            const ngp_status st = comb_run_group(c, grp, &shared_k);
            if (st == NGP_OK) {
                for (ngp_comb_req *r : grp) r->st = NGP_OK;
                if (shared_k) stats[4] += (int64_t)grp.size();
                stats[1] += 1;
                stats[2] = std::max<int64_t>(stats[2], (int64_t)grp.size());
                stats[3] += (int64_t)grp.size();
                continue;
            }
        }
        for (ngp_comb_req *r : grp) {   // alone, or the merged call failed: each for itself
            r->st = comb_run_one(c, *r);
            stats[1] += 1;
            stats[2] = std::max<int64_t>(stats[2], 1);
        }
    }
}

// A caller that finds nobody serving, but whose predecessors came in company, gives that company
// this long to arrive before it serves (tasks that were woken together by the previous sequence do
// their host work and come back within microseconds of each other: without the wait the first one
// back runs alone and the convoy alternates 1, T-1, 1, T-1 ...).  Bounded, and never paid twice in
// vain: a wait that ends short of the expected company lowers the expectation to what did arrive,
// so a caller that is alone waits at most once after a concurrent phase and never otherwise.
constexpr int COMB_LINGER_US = 200;

ngp_status combine_submit(ngp_ctx *c, ngp_comb_req &r) {
    r.key = comb_key(r);   // outside the lock: 16 KB of dates at n = 2048
    std::unique_lock<std::mutex> q(c->qmu);
    if (!c->combine_on) {
        q.unlock();
        return comb_run_one(c, r);
    }
    c->pending.push_back(&r);
    c->comb_arrival.notify_all();
    // Invariant: a request that is not done is either in `pending` or in the batch of the one
    // serving thread (combining == true).  So a thread that finds nobody serving finds its own
    // request in `pending`.
    while (!r.done) {
        if (c->combining) {
            r.cv.wait(q);
            continue;
        }
        c->combining = true;
        if (c->combine_linger && c->pending.size() < c->comb_expect) {
            const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(COMB_LINGER_US);
            (void)c->comb_arrival.wait_until(q, deadline, [&] { return c->pending.size() >= c->comb_expect; });
        }
        std::vector<ngp_comb_req *> batch;
        batch.swap(c->pending);
        c->comb_expect = std::max<size_t>(batch.size(), 1);
        q.unlock();
        int64_t stats[6] = {0, 0, 0, 0, 0, 0};
        comb_execute(c, batch, stats);
        q.lock();
        c->comb_stats[0] += stats[0];
        c->comb_stats[1] += stats[1];
        c->comb_stats[2] = std::max(c->comb_stats[2], stats[2]);
        c->comb_stats[3] += stats[3];
        c->comb_stats[4] += stats[4];
        // (qmu is held from `done = true` to the notify: a woken caller cannot leave — and take its
        // request off its stack — before this loop is through with it)
        for (ngp_comb_req *x : batch) {
            x->done = true;
            if (x != &r) x->cv.notify_one();
        }
        c->combining = false;
        // what arrived meanwhile is served by its first waiter, not by this thread
        if (!c->pending.empty()) c->pending.front()->cv.notify_one();
    }
    return r.st;
}

}  // namespace

extern "C" ngp_status ngp_set_combining(ngp_ctx *c, int32_t on) {
    if (!c) return NGP_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->qmu);
    c->combine_on = on != 0;
    c->combine_linger = on != 2;   // 2: combine what is pending, never wait for company
    return NGP_OK;
}

extern "C" ngp_status ngp_combine_stats(ngp_ctx *c, int64_t *out6, int32_t reset) {
    if (!c || !out6) return NGP_ERR_ARG;
    std::lock_guard<std::mutex> lk(c->qmu);
    for (int i = 0; i < 6; ++i) out6[i] = c->comb_stats[i];
    if (reset) for (int i = 0; i < 6; ++i) c->comb_stats[i] = 0;
    return NGP_OK;
}

// Arguments the merged form could not carry (null arrays, a malformed tree, empty sizes) never
// join a group: the direct path reports them exactly as before.
static bool comb_value_args_ok(ngp_ctx *c, int32_t B, const ngp_kernel *k, int32_t n, const double *t,
                               const double *y) {
    if (!c || !k || !t || !y || B <= 0 || n <= 0) return false;
    for (int i = 0; i < B; ++i)
        if (check_program(&k[i]) != NGP_OK) return false;
    return true;
}

extern "C" ngp_status ngp_logml_batch(ngp_ctx *c, int32_t B, const ngp_kernel *k, int32_t n,
                                      const double *t, const double *y, int64_t ldy, double *logml,
                                      int32_t *info) {
    if (!comb_value_args_ok(c, B, k, n, t, y)) return logml_direct(c, B, k, n, t, y, ldy, logml, info);
    ngp_comb_req r;
    r.kind = CK_LOGML;
    r.B = B; r.k = k; r.n = n; r.t = t; r.y = y; r.ldy = ldy;
    r.logml = logml; r.info = info;
    return combine_submit(c, r);
}

extern "C" ngp_status ngp_predict_batch(ngp_ctx *c, int32_t B, const ngp_kernel *k, int32_t n,
                                        const double *t, const double *y, int64_t ldy, int32_t m,
                                        const double *t_new, int32_t noise_on_new, double *mu,
                                        double *sigma, double *logml, int32_t *info) {
    if (!comb_value_args_ok(c, B, k, n, t, y) || m <= 0 || !t_new)
        return predict_direct(c, B, k, n, t, y, ldy, m, t_new, noise_on_new, mu, sigma, logml, info);
    ngp_comb_req r;
    r.kind = CK_PREDICT;
    r.B = B; r.k = k; r.n = n; r.t = t; r.y = y; r.ldy = ldy;
    r.m = m; r.t_new = t_new; r.noise_on_new = noise_on_new ? 1 : 0;
    r.mu = mu; r.sigma = sigma; r.logml = logml; r.info = info;
    return combine_submit(c, r);
}

extern "C" ngp_status ngp_logml_grad_batch(ngp_ctx *c, int32_t B, const ngp_kernel *kernels,
                                           int32_t n, const double *t, const double *y,
                                           int64_t ldy, double *logml, double *grad,
                                           int32_t *info) {
    if (!grad || !comb_value_args_ok(c, B, kernels, n, t, y))
        return logml_grad_direct(c, B, kernels, n, t, y, ldy, nullptr, logml, grad, info);
    ngp_comb_req r;
    r.kind = CK_GRAD;
    r.B = B; r.k = kernels; r.n = n; r.t = t; r.y = y; r.ldy = ldy;
    r.logml = logml; r.grad = grad; r.info = info;
    return combine_submit(c, r);
}

// A resident job that still has the one-shot form of its inputs (small jobs) is a gradient request
// like any other: with company it shares one call over everybody's items, alone it runs on its
// resident inputs.
extern "C" ngp_status ngp_grad_job_run(ngp_grad_job *j, double *logml, double *grad, int32_t *info) {
    if (!j || !grad) return NGP_ERR_ARG;
    if (j->h_k.empty()) return grad_job_run_resident(j, logml, grad, info);
    ngp_comb_req r;
    r.kind = CK_GRAD;
    r.gj = j;
    r.route = j->route;
    r.B = j->B; r.k = j->h_k.data(); r.n = j->n; r.t = j->h_t.data();
    r.y = j->h_y.data(); r.ldy = j->h_ldy;
    r.logml = logml; r.grad = grad; r.info = info;
    return combine_submit(j->ctx, r);
}

extern "C" ngp_status ngp_mixture_sample(ngp_ctx *c, int32_t P, int32_t S, int32_t m,
                                         const double *w, const double *mu, const double *sigma,
                                         int32_t draws, uint64_t seed, double *out, int32_t *comp,
                                         int32_t *info) {
    // S mixtures over shared components stay one call of their own; ONE mixture (what
    // predict_mvn(...) |> rand of a scenario task asks for, src/forecasting.jl:46-47) can share a
    // launch with other tasks' mixtures of the same shape
    const MixInput mix{P, S, m, draws, w, mu, sigma, seed, nullptr};
    if (S != 1 || !c || !out || !mix.args_ok() || mix.too_large(false)) return mixture_sample_impl(c, mix, out, comp, info);
    ngp_comb_req r;
    r.kind = CK_MIXTURE;
    r.P = P; r.m = m; r.draws = draws; r.w = w;
    r.cmu = mu; r.csigma = sigma;
    r.seed = seed; r.out = out; r.comp = comp; r.info = info;
    return combine_submit(c, r);
}

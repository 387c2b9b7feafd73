// ngp_host_mixture.h — the forecast mixture: weight normalisation (ngp_weights_normalize, _cols),
// MixInput, the sampler (mixture_sample_impl, ngp_mixture_sample_indep), MixStaged / mixture_stage
// and the summaries (ngp_mixture_cdf / _quantiles / _crps), the mapped CRPS with its
// microbenchmark, the trajectory targets (path_targets_impl) and the ensemble and path scores
// (score_args, scores_impl).
// Included from ngp_api.hip behind that file's own code.  Of it this header needs HIPCHK, PinVec,
// ScopedEvent (the microbenchmark), ngp_ctx (stream, mem_cap, refresh_mem_cap) and DevCall — no job,
// factor or gradient code — and of ngp_internal.h the launch_mixture_* / launch_mixmap_* /
// launch_path_targets / launch_scores launchers with their MIX_* / PATH_* / SCORE_* limits, and the
// planner of ngp_mixmap_plan.h (mixmap_plan, mixmap_refine, the MIXMAP_* record).  ngp_mixture_sample
// enters through the combiner and is in ngp_host_combine.h.
#pragma once

// one column of a [P x ld]-strided log-weight matrix (ld = 1: a plain vector)
static void weights_normalize_strided(int P, const double *logw, long ld, double *w_norm, long ldw,
                                      double *ess, double *log_norm) {
    // a particle whose factorisation failed carries -inf (or NaN after -inf - -inf): weight 0, it
    // must not poison the others
    double mx = -INFINITY;
    for (int i = 0; i < P; ++i)
        if (std::isfinite(logw[i * ld]) && logw[i * ld] > mx) mx = logw[i * ld];
    if (!(mx > -INFINITY)) {
        if (ess) *ess = NAN;
        if (log_norm) *log_norm = -INFINITY;
        if (w_norm) for (int i = 0; i < P; ++i) w_norm[i * ldw] = NAN;
        return;
    }
    auto e = [&](int i) { return std::isfinite(logw[i * ld]) ? std::exp(logw[i * ld] - mx) : 0.0; };
    double sum = 0.0;
    for (int i = 0; i < P; ++i) sum += e(i);
    double sq = 0.0;
    for (int i = 0; i < P; ++i) {
        const double w = e(i) / sum;
        if (w_norm) w_norm[i * ldw] = w;
        sq += w * w;
    }
    if (ess) *ess = 1.0 / sq;
    if (log_norm) *log_norm = mx + std::log(sum);
}

extern "C" ngp_status ngp_weights_normalize(int32_t P, const double *logw, double *w_norm,
                                            double *ess, double *log_norm) {
    if (P <= 0 || !logw) return NGP_ERR_ARG;
    weights_normalize_strided(P, logw, 1, w_norm, 1, ess, log_norm);
    return NGP_OK;
}

extern "C" ngp_status ngp_weights_normalize_cols(int32_t P, int32_t D, const double *logw,
                                                 double *w_norm, double *ess, double *log_norm) {
    if (P <= 0 || D <= 0 || !logw) return NGP_ERR_ARG;
    for (int s = 0; s < D; ++s)
        weights_normalize_strided(P, logw + s, D, w_norm ? w_norm + s : nullptr, D,
                                  ess ? ess + s : nullptr, log_norm ? log_norm + s : nullptr);
    return NGP_OK;
}

// A forecast mixture as a caller hands it in: what the sampler and every consumer of its paths (the
// trajectory targets, the path scores) take.  seeds == nullptr: S mixtures over the SAME P components,
// mu [P x S x m], sigma [P x m x m], one key (seed); seeds [S]: every mixture has its own P components,
// mu [S x P x m], sigma [S x P x m x m], its own key.  (MixStaged below: the per-date marginals.)
struct MixInput {
    int32_t P, S, m, draws;
    const double *w, *mu, *sigma;
    uint64_t seed; const uint64_t *seeds;   // one or the other
    size_t blocks() const { return seeds ? (size_t)S * P : (size_t)P; }   // covariance blocks
    size_t nw() const { return (size_t)S * P; }
    size_t nmu() const { return nw() * (size_t)m; }
    size_t nsg() const { return blocks() * (size_t)m * m; }
    int64_t N() const { return (int64_t)S * draws; }                       // paths
    // NGP_ERR_ARG and NGP_ERR_TOO_LARGE apart: the calls have checks of their own between the two
    bool args_ok() const { return w && mu && sigma && P > 0 && S > 0 && m > 0 && draws > 0; }
    // counts: the calls that index paths and blocks with 32 bits bound N and S P as well
    bool too_large(bool counts) const { return m > NGP_MAX_AUX || (counts && (N() > INT32_MAX || nw() > INT32_MAX)); }
    void up(DevCall &call, double *dw, double *dmu, double *dsg, uint64_t *dseeds) const {
        call.up(dw, w, 8 * nw()).up(dmu, mu, 8 * nmu()).up(dsg, sigma, 8 * nsg());
        if (seeds) call.up(dseeds, seeds, 8 * (size_t)S);
    }
    // a failed component (info [blocks()]: the Cholesky factorisations) that paths can come from,
    // in its own mixture or, shared, in any of the S: nothing a call returns is free of it
    bool tainted(const int32_t *info) const {
        for (size_t k = 0; k < blocks(); ++k)
            for (int32_t sc = 0; info[k] && sc < (seeds ? 1 : S); ++sc)
                if (w[seeds ? k : (size_t)sc * P + k] > 0.0) return true;
        return false;
    }
};

// shared body of ngp_mixture_sample and ngp_mixture_sample_indep
static ngp_status mixture_sample_impl(ngp_ctx *c, const MixInput &mix, double *out, int32_t *comp, int32_t *info) {
    if (!c || !out || !mix.args_ok()) return NGP_ERR_ARG;
    if (mix.too_large(false)) return NGP_ERR_TOO_LARGE;
    DevCall call(c);
    const size_t nout = (size_t)mix.N() * mix.m, ncomp = (size_t)mix.N();
    double *dw = nullptr, *dmu = nullptr, *dsg = nullptr, *dout = nullptr;
    int32_t *dcomp = nullptr, *dinfo = nullptr;
    uint64_t *dseeds = nullptr;
    call.take(&dw, mix.nw()).take(&dmu, mix.nmu()).take(&dsg, mix.nsg()).take(&dout, nout).take(&dcomp, ncomp)
        .take(&dinfo, mix.blocks());
    if (mix.seeds) call.take(&dseeds, (size_t)mix.S);
    mix.up(call, dw, dmu, dsg, dseeds);
    call.run([&] {
            launch_mixture_sample(mix.P, mix.S, mix.m, dw, dmu, dsg, mix.draws, mix.seed, dseeds, dout, dcomp,
                                  dinfo, c->stream);
        })
        .down(out, dout, 8 * nout);
    if (comp) call.down(comp, dcomp, 4 * ncomp);
    if (info) call.down(info, dinfo, 4 * mix.blocks());
    return call.sync();
}

extern "C" ngp_status ngp_mixture_sample_indep(ngp_ctx *c, int32_t P, int32_t S, int32_t m,
                                               const double *w, const double *mu,
                                               const double *sigma, int32_t draws,
                                               const uint64_t *seeds, double *out, int32_t *comp,
                                               int32_t *info) {
    if (!seeds) return NGP_ERR_ARG;
    return mixture_sample_impl(c, MixInput{P, S, m, draws, w, mu, sigma, 0, seeds}, out, comp, info);
}

// ---------------------------------------------------------------------------------------
// Summaries of a mixture's per-date marginals (ngp_mixture_cdf / _quantiles / _crps)
//
// The host pass validates, reports bad dates and restages the mixture for the kernels of
// ngp_mixture_kernels.h: components of weight zero are dropped (they are to be ignored, bad values
// included) and the rest goes DATE-MAJOR.  A date with a bad component is computed on harmless
// stand-in values and comes out as NaN; nothing it holds reaches the arithmetic of another date.
namespace {
struct MixStaged {
    int32_t C = 0;                       // components of positive weight
    PinVec<double> w, mu, var;           // [C], [m][C], [m][C]
    std::vector<char> bad;               // [m]
};

ngp_status mixture_stage(int32_t C, int32_t m, const double *w, const double *mu, const double *var,
                         int32_t *info, MixStaged *out) {
    if (!w || !mu || !var || !info || C < 1 || m < 1) return NGP_ERR_ARG;
    if (C > MIX_MAX_COMPONENTS || m > MIX_MAX_DATES) return NGP_ERR_TOO_LARGE;
    std::vector<int32_t> keep;
    keep.reserve(C);
    for (int32_t c = 0; c < C; ++c) {
        if (!(w[c] >= 0.0) || !std::isfinite(w[c])) return NGP_ERR_ARG;
        if (w[c] > 0.0) keep.push_back(c);
    }
    if (keep.empty()) return NGP_ERR_ARG;
    const size_t Cn = keep.size();
    out->C = (int32_t)Cn;
    out->w.resize(Cn);
    out->mu.resize(Cn * m);
    out->var.resize(Cn * m);
    out->bad.assign(m, 0);
    for (int32_t j = 0; j < m; ++j) info[j] = 0;
    for (size_t k = 0; k < Cn; ++k) {
        const int32_t c = keep[k];
        out->w[k] = w[c];
        const double *mc = mu + (size_t)c * m, *vc = var + (size_t)c * m;
        for (int32_t j = 0; j < m; ++j) {
            const bool ok = std::isfinite(mc[j]) && std::isfinite(vc[j]) && vc[j] > 0.0;
            if (!ok && !info[j]) info[j] = c + 1;      // components come in ascending order
            out->mu[(size_t)j * Cn + k] = mc[j];
            out->var[(size_t)j * Cn + k] = vc[j];
        }
    }
    for (int32_t j = 0; j < m; ++j) {
        if (!info[j]) continue;
        out->bad[j] = 1;
        for (size_t k = 0; k < Cn; ++k) {
            out->mu[(size_t)j * Cn + k] = 0.0;
            out->var[(size_t)j * Cn + k] = 1.0;
        }
    }
    return NGP_OK;
}

// every level strictly inside (0, 1) (a NaN is not)
bool probs_open_unit(const double *probs, int32_t n) {
    for (int32_t i = 0; i < n; ++i)
        if (!(probs[i] > 0.0 && probs[i] < 1.0)) return false;
    return true;
}

// a known kind and finite parameters (what more a call asks of the map is checked at that call)
bool inv_transform_ok(const ngp_inv_transform *inv) {
    return inv->kind >= NGP_INV_IDENTITY && inv->kind <= NGP_INV_BOXCOX && std::isfinite(inv->lam) &&
           std::isfinite(inv->offset) && std::isfinite(inv->cap);
}

// the map as the calls that transform whole paths ask for it: Box-Cox with a positive cap
bool path_inv_ok(const ngp_inv_transform *inv) {
    return inv_transform_ok(inv) && (inv->kind != NGP_INV_BOXCOX || inv->cap > 0.0);
}

// observations on the scoring scale: an unknown scale, a shift not finite and non-negative; then the
// caller's own size limits (too_large) BEFORE y is read; then a y not finite or with s(y) undefined
ngp_status score_obs_check(int32_t scale, double shift, bool too_large, const double *y, int32_t m) {
    if (scale != NGP_SCORE_NATURAL && scale != NGP_SCORE_LOG) return NGP_ERR_ARG;
    if (!std::isfinite(shift) || shift < 0.0) return NGP_ERR_ARG;
    if (too_large) return NGP_ERR_TOO_LARGE;
    for (int32_t j = 0; j < m; ++j)
        if (!std::isfinite(y[j]) || (scale == NGP_SCORE_LOG && !(y[j] + shift > 0.0))) return NGP_ERR_ARG;
    return NGP_OK;
}

enum { MIX_CDF = 0, MIX_QUANTILES = 1, MIX_CRPS = 2 };

// pts: x [m x npts] (CDF), probs [npts] (quantiles), y [m] (CRPS, npts = 1); res [m x npts]
ngp_status mixture_summary(ngp_ctx *c, int kind, int32_t C, int32_t m, const double *w,
                           const double *mu, const double *var, int32_t npts, const double *pts,
                           double *res, int32_t *info) {
    if (!c || !pts || !res || npts < 1) return NGP_ERR_ARG;
    if (npts > MIX_MAX_POINTS) return NGP_ERR_TOO_LARGE;
    if (kind == MIX_QUANTILES && !probs_open_unit(pts, npts)) return NGP_ERR_ARG;
    MixStaged h;
    ngp_status st = mixture_stage(C, m, w, mu, var, info, &h);
    if (st) return st;
    const size_t Cn = (size_t)h.C, nres = (size_t)m * npts;
    const size_t npin = kind == MIX_QUANTILES ? (size_t)npts : nres;
    DevCall call(c);
    hipStream_t s = c->stream;
    double *dw = nullptr, *dmu = nullptr, *dvar = nullptr, *daux = nullptr, *dpts = nullptr,
           *dres = nullptr;
    // aux: inv [m][C] for the CDF and the quantiles, the slab of tile partials for the CRPS
    const size_t naux = kind == MIX_CRPS ? (size_t)m * (size_t)mix_tile_pairs(h.C) : Cn * m;
    call.take(&dw, Cn).take(&dmu, Cn * m).take(&dvar, Cn * m).take(&daux, naux).take(&dpts, npin)
        .take(&dres, nres);
    call.up(dw, h.w.data(), 8 * Cn)
        .up(dmu, h.mu.data(), 8 * Cn * m)
        .up(dvar, h.var.data(), 8 * Cn * m)
        .up(dpts, pts, 8 * npin)
        .run([&] {
            if (kind == MIX_CRPS) {
                launch_mixture_crps(h.C, m, dw, dmu, dvar, dpts, daux, dres, s);
            } else {
                launch_mixture_prep(dvar, daux, (int64_t)(Cn * m), s);
                if (kind == MIX_CDF) launch_mixture_cdf(h.C, m, dw, dmu, daux, npts, dpts, dres, s);
                else launch_mixture_quantiles(h.C, m, dw, dmu, daux, npts, dpts, dres, s);
            }
        })
        .down(res, dres, 8 * nres);
    if ((st = call.sync())) return st;
    for (int32_t j = 0; j < m; ++j)
        if (h.bad[j])
            for (int32_t k = 0; k < npts; ++k) res[(size_t)j * npts + k] = std::nan("");
    return NGP_OK;
}
}  // namespace

extern "C" ngp_status ngp_mixture_cdf(ngp_ctx *c, int32_t C, int32_t m, const double *w,
                                      const double *mu, const double *var, int32_t K,
                                      const double *x, double *cdf, int32_t *info) {
    return mixture_summary(c, MIX_CDF, C, m, w, mu, var, K, x, cdf, info);
}

extern "C" ngp_status ngp_mixture_quantiles(ngp_ctx *c, int32_t C, int32_t m, const double *w,
                                            const double *mu, const double *var, int32_t Q,
                                            const double *probs, double *q, int32_t *info) {
    return mixture_summary(c, MIX_QUANTILES, C, m, w, mu, var, Q, probs, q, info);
}

extern "C" ngp_status ngp_mixture_crps(ngp_ctx *c, int32_t C, int32_t m, const double *w,
                                       const double *mu, const double *var, const double *y,
                                       double *crps, int32_t *info) {
    return mixture_summary(c, MIX_CRPS, C, m, w, mu, var, 1, y, crps, info);
}

// ---------------------------------------------------------------------------------------
// CRPS and mean after a monotone map (ngp_mixture_crps_mapped; ngp_mixture_mapped_kernels.h)
//
// The host validates, stages as the summaries above do, reads back one small record per date
// (the scan kernel: range, boundaries of the map, the point where it crosses y), plans each date's
// panels from its record alone and runs the panel and reduce kernels; dates whose error estimate
// is above the tolerance go round again at half the width, alone, until the per-date cap.
extern "C" ngp_status ngp_mixture_crps_mapped(ngp_ctx *c, int32_t C, int32_t m, const double *w,
                                              const double *mu, const double *var, const void *inv_,
                                              int32_t scale, double shift, const double *y,
                                              double tol, double *crps, double *mean, double *err,
                                              int32_t *info) {
    const ngp_inv_transform *inv = (const ngp_inv_transform *)inv_;
    if (!c || !inv || !y || !crps || !info || m < 1) return NGP_ERR_ARG;
    if (!inv_transform_ok(inv) || !std::isfinite(tol)) return NGP_ERR_ARG;
    ngp_status st = score_obs_check(scale, shift, m > MIX_MAX_DATES, y, m);
    if (st) return st;
    if (!(tol > 0.0)) tol = MIXMAP_DEFAULT_TOL;
    MixStaged h;
    if ((st = mixture_stage(C, m, w, mu, var, info, &h))) return st;
    const size_t Cn = (size_t)h.C;
    std::vector<double> rec((size_t)m * MIXMAP_REC, 0.0);   // (before the call: it outlives what reads and writes it)
    std::vector<MixMapPlan> work;
    std::vector<double> res;
    DevCall call(c);
    hipStream_t s = c->stream;
    double *dw = nullptr, *dmu = nullptr, *dvar = nullptr, *dinv = nullptr, *dy = nullptr,
           *drec = nullptr;
    call.take(&dw, Cn).take(&dmu, Cn * m).take(&dvar, Cn * m).take(&dinv, Cn * m).take(&dy, (size_t)m)
        .take(&drec, (size_t)m * MIXMAP_REC);
    call.up(dw, h.w.data(), 8 * Cn)
        .up(dmu, h.mu.data(), 8 * Cn * m)
        .up(dvar, h.var.data(), 8 * Cn * m)
        .up(dy, y, 8 * (size_t)m)
        .run([&] {
            launch_mixture_prep(dvar, dinv, (int64_t)(Cn * m), s);
            launch_mixmap_scan(h.C, m, *inv, scale, shift, dw, dmu, dinv, dy, drec, s);
        })
        .down(rec.data(), drec, 8 * rec.size());
    if ((st = call.sync())) return st;

    const double nan = std::nan("");
    work.reserve(m);
    for (int32_t j = 0; j < m; ++j) {
        crps[j] = nan;
        if (mean) mean[j] = nan;
        if (err) err[j] = nan;
        if (h.bad[j]) continue;
        if (rec[(size_t)j * MIXMAP_REC + MIXMAP_REC_FLAG] != 0.0) {
            info[j] = NGP_INFO_NOT_FINITE;
            continue;
        }
        work.push_back(mixmap_plan(j, &rec[(size_t)j * MIXMAP_REC]));
    }
    while (!work.empty()) {
        const size_t nw = work.size();
        int32_t maxp = 1;
        for (const MixMapPlan &p : work) maxp = std::max(maxp, p.npanels);
        DevCall round(call);                               // this width's buffers, given back below
        MixMapPlan *dplan = nullptr;
        double *dslab = nullptr, *dres = nullptr;
        round.take(&dplan, nw).take(&dslab, nw * (size_t)maxp * 3).take(&dres, nw * 3);
        res.assign(nw * 3, 0.0);
        round.up(dplan, work.data(), nw * sizeof(MixMapPlan))
            .run([&] {
                launch_mixmap_panels(h.C, (int)nw, maxp, *inv, scale, shift, dplan, dw, dmu, dinv, dslab,
                                     dres, s);
            })
            .down(res.data(), dres, 8 * res.size());
        if ((st = round.sync())) return st;
        std::vector<MixMapPlan> next;
        for (size_t k = 0; k < nw; ++k) {
            const int32_t j = work[k].date;
            const double *r = &rec[(size_t)j * MIXMAP_REC];
            const double cj = res[k * 3] + r[MIXMAP_REC_CLIP], ej = res[k * 3 + 1];
            const double mj = r[MIXMAP_REC_PSI0] + res[k * 3 + 2];
            if (!std::isfinite(cj) || !std::isfinite(mj) || !std::isfinite(ej)) {
                info[j] = NGP_INFO_NOT_FINITE;             // the outputs stay NaN
                continue;
            }
            const bool done = ej <= tol * std::fabs(cj);
            if (!done && mixmap_refine(&work[k])) {
                next.push_back(work[k]);
                continue;
            }
            crps[j] = cj;
            if (mean) mean[j] = mj;
            if (err) err[j] = ej;
            if (!done) info[j] = NGP_INFO_NOT_CONVERGED;
        }
        work.swap(next);
    }
    return NGP_OK;
}

// pair terms of the CRPS cross sum per second with the operands in registers (no loads, no LDS):
// the ceiling mix_crps_pairs_kernel is measured against (scripts/summary_probe.py)
extern "C" ngp_status ngp_microbench_mixture_pairs(ngp_ctx *c, int32_t iters, double *pairs_per_s) {
    if (!c || !pairs_per_s || iters <= 0) return NGP_ERR_ARG;
    DevCall call(c);
    const int blocks = 256 * 8;
    double *out = nullptr;
    call.take(&out, (size_t)blocks * 256);
    ScopedEvent a, b;
    call.run([&] {
            launch_mixture_pair_rate(iters, blocks, out, c->stream);  // warm-up
            return hipEventRecord(a, c->stream);
        })
        .run([&] {
            launch_mixture_pair_rate(iters, blocks, out, c->stream);
            return hipEventRecord(b, c->stream);
        });
    if (call.sync()) return call.status();
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    *pairs_per_s = (double)blocks * 256.0 * (double)iters / ((double)ms * 1e-3);
    return NGP_OK;
}

// ---------------------------------------------------------------------------------------
// Trajectory targets (ngp_mixture_path_targets / _indep; kernels: ngp_path_kernels.h)
//
// The host validates, turns the levels into ranks (ascending, distinct: the select passes work
// on those; q is filled per level from them), stages, launches and scatters the few results.
namespace {
ngp_status path_targets_impl(ngp_ctx *c, const MixInput &mix, const ngp_inv_transform *inv, int32_t T,
                             const ngp_path_target *targets, int32_t Q, const double *probs,
                             double *q, double *mean, int64_t *count, int64_t *hist,
                             double *values, int32_t *info) {
    const int32_t m = mix.m;
    if (!c || !mix.args_ok() || !inv || !targets || !probs || !q || !mean || !count || !hist || T < 1 || Q < 1)
        return NGP_ERR_ARG;
    if (!path_inv_ok(inv)) return NGP_ERR_ARG;
    if (T > PATH_MAX_TARGETS || Q > PATH_MAX_LEVELS) return NGP_ERR_TOO_LARGE;   // bounds the loops below
    for (int32_t t = 0; t < T; ++t) {
        const ngp_path_target &tg = targets[t];
        if (tg.kind < NGP_TARGET_SUM || tg.kind > NGP_TARGET_EXCEED || tg.j0 < 0 || tg.j1 >= m ||
            tg.j0 > tg.j1 || !std::isfinite(tg.thr))
            return NGP_ERR_ARG;
    }
    if (!probs_open_unit(probs, Q)) return NGP_ERR_ARG;
    if (mix.too_large(true)) return NGP_ERR_TOO_LARGE;
    const int64_t N = mix.N();

    // levels -> ranks, ascending and distinct; lvl[i]: where level i's rank sits among them
    std::vector<int64_t> rank_of(Q), ranks;
    for (int32_t i = 0; i < Q; ++i)
        rank_of[i] = std::min<int64_t>(std::max<int64_t>((int64_t)std::ceil(probs[i] * (double)N), 1), N);
    ranks = rank_of;
    std::sort(ranks.begin(), ranks.end());
    ranks.erase(std::unique(ranks.begin(), ranks.end()), ranks.end());
    std::vector<int32_t> real;
    for (int32_t t = 0; t < T; ++t)
        if (targets[t].kind <= NGP_TARGET_DIFF) real.push_back(t);

    PathGeom g{};
    g.P = mix.P; g.S = mix.S; g.m = m; g.draws = mix.draws;
    g.B = (int32_t)mix.blocks();
    g.indep = mix.seeds ? 1 : 0;
    g.PW = path_pw(m);
    g.T = T; g.Tr = (int32_t)real.size(); g.R = (int32_t)ranks.size();
    g.N = N;
    const size_t Nn = (size_t)N, B = mix.blocks(), Tn = (size_t)T, R = ranks.size(),
                 Tr = std::max<size_t>(real.size(), 1), slices = (size_t)path_slices(N);
    const size_t nw = mix.nw(), nmu = mix.nmu(), nsg = mix.nsg();

    std::vector<int32_t> hinfo(B, 0);
    std::vector<double> hq(Tr * R, 0.0);
    DevCall call(c);
    if (call.status()) return call.status();
    c->refresh_mem_cap();
    if ((double)(8 * Tn + 12) * (double)Nn + 8.0 * (double)(nw + nmu + nsg) > (double)c->mem_cap)
        return NGP_ERR_TOO_LARGE;
    double *dw = nullptr, *dmu = nullptr;
    uint64_t *dseeds = nullptr;
    int64_t *dranks = nullptr;
    int32_t *dreal = nullptr;
    ngp_path_target *dtargets = nullptr;
    PathBufs b{};
    call.take(&dw, nw).take(&dmu, nmu).take(&b.chol, nsg);
    if (mix.seeds) call.take(&dseeds, (size_t)mix.S);
    call.take(&b.info, B).take(&b.bkt, Nn).take(&b.order, Nn).take(&b.rank, Nn).take(&b.cnt, B)
        .take(&b.off, B + 1).take(&b.wgoff, B + 1).take(&dtargets, Tn).take(&dreal, Tr).take(&dranks, R)
        .take(&b.values, Tn * Nn).take(&b.partial, Tn * slices).take(&b.mean, Tn).take(&b.count, Tn)
        .take(&b.hist, Tn * m).take(&b.prefix, Tr * R).take(&b.gpre, Tr * R).take(&b.krem, Tr * R)
        .take(&b.grp, Tr * R).take(&b.ng, Tr).take(&b.ghist, Tr * R * 256).take(&b.q, Tr * R);

    b.w = dw; b.mu = dmu; b.seeds = dseeds; b.targets = dtargets; b.real = dreal; b.ranks = dranks;

    mix.up(call, dw, dmu, b.chol, dseeds);
    call.up(dtargets, targets, sizeof(ngp_path_target) * Tn);
    if (!real.empty()) call.up(dreal, real.data(), 4 * real.size());
    call.up(dranks, ranks.data(), 8 * R)
        .run([&] { return launch_path_targets(g, b, *inv, mix.seed, c->stream); })
        .down(mean, b.mean, 8 * Tn)
        .down(count, b.count, 8 * Tn)
        .down(hist, b.hist, 8 * Tn * m);
    if (!real.empty()) call.down(hq.data(), b.q, 8 * real.size() * R);
    if (values) call.down(values, b.values, 8 * Tn * Nn);
    call.down(hinfo.data(), b.info, 4 * B);
    if (call.sync()) return call.status();

    if (info) std::copy(hinfo.begin(), hinfo.end(), info);
    const double nan = std::nan("");
    for (size_t i = 0; i < Tn * (size_t)Q; ++i) q[i] = nan;
    for (size_t y = 0; y < real.size(); ++y)
        for (int32_t i = 0; i < Q; ++i) {
            const size_t r = std::lower_bound(ranks.begin(), ranks.end(), rank_of[i]) - ranks.begin();
            q[(size_t)real[y] * Q + i] = hq[y * R + r];
        }
    if (mix.tainted(hinfo.data())) {
        for (size_t i = 0; i < Tn * (size_t)Q; ++i) q[i] = nan;
        for (size_t t = 0; t < Tn; ++t) { mean[t] = nan; count[t] = 0; }
        for (size_t i = 0; i < Tn * (size_t)m; ++i) hist[i] = 0;
        if (values) for (size_t i = 0; i < Tn * Nn; ++i) values[i] = nan;
    }
    return NGP_OK;
}
}  // namespace

extern "C" ngp_status ngp_mixture_path_targets(ngp_ctx *c, int32_t P, int32_t S, int32_t m,
                                               const double *w, const double *mu,
                                               const double *sigma, int32_t draws, uint64_t seed,
                                               const void *inv, int32_t T, const void *targets,
                                               int32_t Q, const double *probs, double *q,
                                               double *mean, int64_t *count, int64_t *hist,
                                               double *values, int32_t *info) {
    return path_targets_impl(c, MixInput{P, S, m, draws, w, mu, sigma, seed, nullptr},
                             (const ngp_inv_transform *)inv, T, (const ngp_path_target *)targets, Q,
                             probs, q, mean, count, hist, values, info);
}

extern "C" ngp_status ngp_mixture_path_targets_indep(ngp_ctx *c, int32_t P, int32_t S, int32_t m,
                                                     const double *w, const double *mu,
                                                     const double *sigma, int32_t draws,
                                                     const uint64_t *seeds,
                                                     const void *inv, int32_t T,
                                                     const void *targets, int32_t Q,
                                                     const double *probs, double *q, double *mean,
                                                     int64_t *count, int64_t *hist, double *values,
                                                     int32_t *info) {
    if (!seeds) return NGP_ERR_ARG;
    return path_targets_impl(c, MixInput{P, S, m, draws, w, mu, sigma, 0, seeds},
                             (const ngp_inv_transform *)inv, T, (const ngp_path_target *)targets, Q,
                             probs, q, mean, count, hist, values, info);
}

// ---------------------------------------------------------------------------------------
// Energy score and sample CRPS of paths (ngp_ensemble_scores / ngp_mixture_path_scores; kernels:
// ngp_score_kernels.h)
//
// The host validates, stages the paths (ensemble form) or has the sampler draw them into a device
// buffer (mixture form), launches, and turns the two [W] totals into the scores.
namespace {
// what both forms ask of N, m, the windows and y; TOO_LARGE before any array is read
ngp_status score_args(int64_t N, int32_t m, int32_t m_max, const double *y, int32_t scale, double shift,
                      int32_t fair, int32_t W, const int32_t *win, const double *es) {
    if (!y || !win || !es || N < 1 || m < 1 || W < 1) return NGP_ERR_ARG;
    if ((fair != 0 && fair != 1) || (fair == 1 && N < 2)) return NGP_ERR_ARG;
    const bool too_large = N > SCORE_MAX_PATHS || W > SCORE_MAX_WINDOWS || m > m_max;
    if (ngp_status st = score_obs_check(scale, shift, too_large, y, m)) return st;
    for (int32_t w = 0; w < W; ++w)
        if (win[2 * w] < 0 || win[2 * w + 1] >= m || win[2 * w] > win[2 * w + 1]) return NGP_ERR_ARG;
    return NGP_OK;
}

// x: the ensemble form's paths; mix, inv, chol_info: the mixture form's inputs instead
ngp_status scores_impl(ngp_ctx *c, int32_t N, int32_t m, const double *x, const double *y, int32_t scale,
                       double shift, int32_t fair, int32_t W, const int32_t *win, double *es,
                       double *term_obs, double *term_pair, int32_t *info, const MixInput *mix = nullptr,
                       const ngp_inv_transform *inv = nullptr, int32_t *chol_info = nullptr) {
    const size_t Nn = (size_t)N, Wn = (size_t)W, nxm = Nn * (size_t)m;
    const size_t prow = (size_t)score_tile_pairs(N), orow = (size_t)score_slices(N);
    const size_t prow1 = (size_t)score_folded((int64_t)prow), orow1 = (size_t)score_folded((int64_t)orow);
    bool long_windows = false;
    for (int32_t w = 0; w < W; ++w) long_windows = long_windows || win[2 * w + 1] - win[2 * w] >= SCORE_FOLD;
    const size_t B = mix ? mix->blocks() : 0;
    const size_t nw = mix ? mix->nw() : 0, nmu = mix ? mix->nmu() : 0, nsg = mix ? mix->nsg() : 0;

    std::vector<int32_t> hflag((size_t)m, 0), hcinfo(B, 0);
    std::vector<double> hobs(Wn, 0.0), hpair(Wn, 0.0);
    DevCall call(c);
    if (call.status()) return call.status();
    c->refresh_mem_cap();
    if (8.0 * ((double)nxm * 2.0 + (double)Wn * (double)(prow + prow1 + orow + orow1) +
               (double)(nw + nmu + nsg)) > (double)c->mem_cap)
        return NGP_ERR_TOO_LARGE;
    ScoreBufs b{};
    double *dx = nullptr, *dy = nullptr, *dw = nullptr, *dmu = nullptr, *dsg = nullptr;
    int32_t *dwin = nullptr, *dcinfo = nullptr;
    uint64_t *dseeds = nullptr;
    call.take(&dx, nxm).take(&dy, (size_t)m).take(&b.u, nxm).take(&b.v, (size_t)m).take(&b.flag, (size_t)m)
        .take(&dwin, 2 * Wn).take(&b.pair[0], prow * Wn).take(&b.pair[1], prow1 * Wn)
        .take(&b.obs[0], orow * Wn).take(&b.obs[1], orow1 * Wn);
    if (mix) {
        call.take(&dw, nw).take(&dmu, nmu).take(&dsg, nsg).take(&dcinfo, B);
        if (mix->seeds) call.take(&dseeds, (size_t)mix->S);
        mix->up(call, dw, dmu, dsg, dseeds);
        call.run([&] {   // the sampler as ngp_mixture_sample launches it, its paths kept on the device
            launch_mixture_sample(mix->P, mix->S, m, dw, dmu, dsg, mix->draws, mix->seed, dseeds, dx, nullptr,
                                  dcinfo, c->stream);
        });
    } else {
        call.up(dx, x, 8 * nxm);
    }
    b.x = dx; b.y = dy; b.win = dwin;
    const double *dobs = nullptr, *dpair = nullptr;
    call.up(dy, y, 8 * (size_t)m).up(dwin, win, 8 * Wn)
        .run([&] {
            return launch_scores(N, m, W, long_windows, inv, scale, shift, b, &dobs, &dpair, c->stream);
        });
    if (call.status()) return call.status();
    call.down(hobs.data(), dobs, 8 * Wn).down(hpair.data(), dpair, 8 * Wn).down(hflag.data(), b.flag, 4 * (size_t)m);
    if (mix) call.down(hcinfo.data(), dcinfo, 4 * B);
    if (call.sync()) return call.status();

    if (chol_info) std::copy(hcinfo.begin(), hcinfo.end(), chol_info);
    const bool failed = mix && mix->tainted(hcinfo.data());
    const double nan = std::nan("");
    const double pairs = fair ? 0.5 * (double)N * (double)(N - 1) : 0.5 * (double)N * (double)N;
    for (int32_t w = 0; w < W; ++w) {
        bool bad = failed;
        for (int32_t j = win[2 * w]; j <= win[2 * w + 1] && !bad; ++j) bad = hflag[j] != 0;
        // finite values whose differences overflow when squared (1e155 and beyond; the largest finite
        // double a Box-Cox image is capped at): the window has no finite score either
        bad = bad || !std::isfinite(hobs[w]) || !std::isfinite(hpair[w]);
        const double to = bad ? nan : hobs[w] / (double)N;
        const double tp = bad ? nan : hpair[w] / pairs;
        es[w] = bad ? nan : to - 0.5 * tp;
        if (term_obs) term_obs[w] = to;
        if (term_pair) term_pair[w] = tp;
        if (info) info[w] = bad ? NGP_INFO_NOT_FINITE : 0;
    }
    return NGP_OK;
}
}  // namespace

extern "C" ngp_status ngp_ensemble_scores(ngp_ctx *c, int32_t N, int32_t m, const double *x,
                                          const double *y, int32_t scale, double shift, int32_t fair,
                                          int32_t W, const int32_t *win, double *es, double *term_obs,
                                          double *term_pair, int32_t *info) {
    if (!c || !x) return NGP_ERR_ARG;
    if (ngp_status st = score_args(N, m, SCORE_MAX_DATES, y, scale, shift, fair, W, win, es)) return st;
    return scores_impl(c, N, m, x, y, scale, shift, fair, W, win, es, term_obs, term_pair, info);
}

extern "C" ngp_status ngp_mixture_path_scores(ngp_ctx *c, int32_t P, int32_t S, int32_t m,
                                              const double *w, const double *mu, const double *sigma,
                                              int32_t indep, int32_t draws, const uint64_t *seeds,
                                              const void *inv_, const double *y, int32_t scale,
                                              double shift, int32_t fair, int32_t W, const int32_t *win,
                                              double *es, double *term_obs, double *term_pair,
                                              int32_t *info, int32_t *chol_info) {
    const ngp_inv_transform *inv = (const ngp_inv_transform *)inv_;
    if (!c || !seeds || !inv || (indep != 0 && indep != 1)) return NGP_ERR_ARG;
    const MixInput mix{P, S, m, draws, w, mu, sigma, indep ? 0 : seeds[0], indep ? seeds : nullptr};
    if (!mix.args_ok() || !path_inv_ok(inv)) return NGP_ERR_ARG;
    if (ngp_status st = score_args(mix.N(), m, NGP_MAX_AUX, y, scale, shift, fair, W, win, es)) return st;
    if (mix.too_large(true)) return NGP_ERR_TOO_LARGE;
    return scores_impl(c, (int32_t)mix.N(), m, nullptr, y, scale, shift, fair, W, win, es, term_obs, term_pair,
                       info, &mix, inv, chol_info);
}

"""ngp_factor_components_nowcast on the device (include/ngp.h "sum-of-products terms; the
decomposition conditioned on nowcasts"): the joint posterior of every
particle's additive parts given the training data, d appended points and D scenarios of their
values, out of ONE query of the resident factor, judged

  1. against the long double restatement tests/component_nowcast_reference.py,
  2. against ngp_factor_nowcast of the same arguments without noise on the new points: per scenario
     the means add up to its mean, the blocks to its covariance, logml_full agrees,
  3. d = 0, D = 1: the bits of ngp_factor_components,
  4. scenario s of a D = 4 call: the bits of the D = 1 call on that scenario; two calls the same
     bits; var = diag(sigma) bit for bit, also from a call without sigma,
  5. shared y against per-particle y, structured storage on and off, both cp_form values,
  6. a particle that failed at creation and a non-positive-definite appended block: info, NaN
     outputs, the neighbours' bits unchanged,
  7. through nowcast.forecast_components_with_nowcasts on a small fitted model,

under the suite's condition-aware comparison with the floor of the predictive moments
(tests/util.check, TOL_PRED: the tolerances of tests/test_components_gpu.py).  Six hand-made
particles: three sums (1, 2, 3 parts), a ChangePoint root split into three windowed terms, a product
of sums distributed into four products, a sum with an unsplit ChangePoint.  n = 40 (no main block),
64 (no tail: A is the appended points alone), 127 (tail 63: with d = 3, da = 66 rows), 130 (tail
2), 300 (tail 44); d = 1, 3; D = 1, 4; m = 1, 7; a weekly lattice and an irregular grid; da = 80
(past what the epilogue keeps in LDS: the work-buffer path); the aux limit met exactly, and missed
by one row.
"""
import functools

import numpy as np
import pytest

from nowcastautogp_amd import _lib, gp
from nowcastautogp_amd._abi import default_spec
from tests import component_nowcast_reference as cnr
from tests import hp_reference as hr
from tests.util import TOL_LOGML, TOL_PRED, check

pytestmark = pytest.mark.gpu

NGP_ERR_ARG, NGP_ERR_PROGRAM, NGP_ERR_TOO_LARGE = -1, -2, -3
DMAX = 4


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    c = _lib.Context(0)
    yield c
    c.close()


def ensemble():
    lin, per, se = gp.Linear(0.3, 0.1, 0.8), gp.Periodic(1.2, 0.2, 0.4), gp.SquaredExponential(0.1, 0.3)
    trees = [
        (gp.Periodic(1.0, 0.25, 0.5), 0),
        (gp.Plus(lin, per), 0),
        (gp.Plus(gp.Plus(gp.Linear(0.6, 0.05, 0.5), gp.Periodic(0.9, 0.125, 0.3)), se), 0),
        (gp.ChangePoint(gp.Plus(gp.Linear(0.4, 0.1, 0.6), gp.SquaredExponential(0.2, 0.5)),
                        gp.Periodic(1.0, 0.3, 0.3), 0.5, 0.1), cnr.SPLIT_CHANGEPOINT),
        (gp.Times(gp.Plus(gp.Linear(0.2, 0.1, 0.6), gp.Constant(0.5)),
                  gp.Plus(gp.Periodic(1.0, 0.15, 0.5), gp.SquaredExponential(0.3, 0.4))),
         cnr.SPLIT_CHANGEPOINT | cnr.SPLIT_TIMES),
        (gp.Plus(gp.ChangePoint(gp.SquaredExponential(0.2, 0.5), gp.Periodic(1.0, 0.3, 0.3), 0.5, 0.1),
                 gp.Linear(0.4, 0.1, 0.6)), 0),
    ]
    noise = [0.05, 0.08, 0.06, 0.1, 0.07, 0.09]
    progs = [gp.to_program(tr) + (nz,) for (tr, _), nz in zip(trees, noise)]
    return progs, [cnr.terms(p, sp) for p, (_, sp) in zip(progs, trees)]


PROGS, COMPS = ensemble()
assert [len(c) for c in COMPS] == [1, 2, 3, 3, 4, 2]


@functools.lru_cache(maxsize=None)
def series(n, d, m, irregular=False):
    """(t, y, t_add, y_add [DMAX, d], t_new): a weekly lattice on [0, 1] continued by the d appended
    and the m query dates, or an irregular grid"""
    rng = np.random.default_rng(2000 + n)
    if irregular:
        tt = np.sort(rng.uniform(0.0, 1.0 + (d + m + 1.0) / n, n + d + m))
    else:
        tt = 7.0 * np.arange(n + d + m) / (7.0 * (n - 1))
    t, t_add, t_new = tt[:n].copy(), tt[n:n + d].copy(), tt[n + d:].copy()
    f = lambda x: 0.8 * (x - 0.4) + 0.5 * np.sin(2 * np.pi * x / 0.25)
    y = f(t) + 0.1 * rng.standard_normal(n)
    y_add = f(t_add)[None, :] + 0.3 * rng.standard_normal((DMAX, d))
    return t, y, t_add, y_add, t_new


@functools.lru_cache(maxsize=None)
def reference(n, d, m, irregular=False, cp_form=0):
    """per particle the reference of all DMAX scenarios (a call with fewer takes the first ones)"""
    t, y, t_add, y_add, t_new = series(n, d, m, irregular)
    spec = dict(se_form=0, periodic_form=0, cp_form=1, jitter=1e-5) if cp_form else None
    return [cnr.evaluate(p, c, t, y, t_add, y_add, t_new, spec) for p, c in zip(PROGS, COMPS)]


def judge(what, n, d, D, m, irregular, out, fac, cp_form=0):
    t, y, t_add, y_add, t_new = series(n, d, m, irregular)
    refs = reference(n, d, m, irregular, cp_form)
    assert not out["info"].any(), out["info"]
    pr = fac.nowcast(t_add, y_add[:D], t_new, noise_on_new=False)
    assert not pr["info"].any()
    for p, r in enumerate(refs):
        assert r.info == 0
        mu, sg, var = out["mu"][p], out["sigma"][p], out["var"][p]
        C = mu.shape[0]
        assert mu.shape == (C, D, m)
        ctx_ = (n, d, D, m, p)
        # 1. the long double restatement
        check(f"{what}: mu vs long double", mu, r.mu[:, :D].astype(float), TOL_PRED, r.cond, ctx=ctx_)
        check(f"{what}: sigma vs long double", sg, r.sigma.astype(float), TOL_PRED, r.cond, ctx=ctx_)
        check(f"{what}: logml vs long double", out["logml_full"][p], r.logml_full[:D].astype(float),
              TOL_LOGML, r.cond, ctx=ctx_)
        # 2. the parts add up to the noise-free nowcast of the same factor
        check(f"{what}: sum of means vs nowcast", mu.sum(axis=0), pr["mu"][p], TOL_PRED, r.cond, ctx=ctx_)
        check(f"{what}: sum of blocks vs nowcast", sg.reshape(C, m, C, m).sum(axis=(0, 2)), pr["sigma"][p],
              TOL_PRED, r.cond, ctx=ctx_)
        check(f"{what}: logml vs nowcast", out["logml_full"][p], pr["logml_full"][p], TOL_LOGML, r.cond,
              ctx=ctx_)
        # 4. var is the diagonal of sigma, bit for bit
        assert np.array_equal(var.reshape(-1), np.diag(sg)), ctx_


def same_bits(a, b, keys=("mu", "var", "sigma")):
    assert np.array_equal(a["info"], b["info"])
    for k in keys:
        for x, y_ in zip(a[k], b[k]):
            assert np.array_equal(x, y_, equal_nan=True), k


def sweep(ctx, n, d, irregular):
    """every D and m of one (n, d): the checks 1, 2 and 4 of the docstring"""
    for m in (1, 7):
        t, y, t_add, y_add, t_new = series(n, d, m, irregular)     # (an irregular grid depends on m)
        fac = ctx.factor(PROGS, t, y)
        try:
            full = fac.components_nowcast(COMPS, t_add, y_add, t_new)
            judge("components nowcast", n, d, DMAX, m, irregular, full, fac)
            one = fac.components_nowcast(COMPS, t_add, y_add[:1], t_new)
            judge("components nowcast", n, d, 1, m, irregular, one, fac)
            # scenario s of the D = 4 call: the bits of the D = 1 call on that scenario
            for s in range(DMAX):
                o = one if s == 0 else fac.components_nowcast(COMPS, t_add, y_add[s:s + 1], t_new)
                same_bits(full, o, keys=("var", "sigma"))
                for p in range(len(PROGS)):
                    assert np.array_equal(full["mu"][p][:, s], o["mu"][p][:, 0]), (n, d, m, s, p)
                    assert full["logml_full"][p, s] == o["logml_full"][p, 0], (n, d, m, s, p)
            again = fac.components_nowcast(COMPS, t_add, y_add, t_new)
            same_bits(full, again)
            assert np.array_equal(full["logml_full"], again["logml_full"])
            lean = fac.components_nowcast(COMPS, t_add, y_add, t_new, want_sigma=False)
            assert lean["sigma"] is None
            same_bits(full, lean, keys=("mu", "var"))
        finally:
            fac.close()


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("n", [40, 64, 127, 130, 300])
def test_components_nowcast_on_a_weekly_lattice(ctx, n, d):
    sweep(ctx, n, d, False)


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("n", [40, 64, 127, 130, 300])
def test_components_nowcast_on_an_irregular_grid(ctx, n, d):
    sweep(ctx, n, d, True)


@pytest.mark.parametrize("n", [40, 64, 127, 130, 300])
def test_without_appended_points_it_is_ngp_factor_components_bit_for_bit(ctx, n):
    m = 7
    t, y, _, _, t_new = series(n, 0, m)
    fac = ctx.factor(PROGS, t, y)
    try:
        old = fac.components(COMPS, t_new)
        new = fac.components_nowcast(COMPS, np.zeros(0), np.zeros((1, 0)), t_new)
        assert np.array_equal(old["info"], new["info"])
        for p in range(len(PROGS)):
            assert np.array_equal(old["mu"][p], new["mu"][p][:, 0]), p
            assert np.array_equal(old["var"][p], new["var"][p]), p
            assert np.array_equal(old["sigma"][p], new["sigma"][p]), p
        pr = fac.nowcast(np.zeros(0), np.zeros((1, 0)), t_new, noise_on_new=False)
        for p, r in enumerate(reference(n, 0, m)):
            check("components nowcast d = 0: logml vs predict", new["logml_full"][p], pr["logml_full"][p],
                  TOL_LOGML, r.cond)
    finally:
        fac.close()


def test_more_rows_to_eliminate_than_lds_holds(ctx):
    """n = 127 (tail 63) and d = 17: da = 80 > 76, L_A lives in the per-item work buffer"""
    n, d, m = 127, 17, 7
    t, y, t_add, y_add, t_new = series(n, d, m)
    fac = ctx.factor(PROGS, t, y)
    try:
        out = fac.components_nowcast(COMPS, t_add, y_add, t_new)
        judge("components nowcast, da = 80", n, d, DMAX, m, False, out, fac)
        one = fac.components_nowcast(COMPS, t_add, y_add[2:3], t_new)
        for p in range(len(PROGS)):
            assert np.array_equal(out["mu"][p][:, 2], one["mu"][p][:, 0])
    finally:
        fac.close()


def test_the_aux_limit_exactly_and_one_row_over(ctx):
    """n = 131: a tail of 3 and d = 2, so 3 + 2 + 1 + C m <= 192 leaves 186 = 3 x 62 component rows for
    the three-part particles; the four-part particle is cut to three"""
    n, d, m = 131, 2, 62
    t, y, t_add, y_add, t_new = series(n, d, m + 1)
    comps = list(COMPS)
    comps[4] = COMPS[4][:3]
    fac = ctx.factor(PROGS, t, y)
    try:
        out = fac.components_nowcast(comps, t_add, y_add, t_new[:m])
        assert not out["info"].any() and out["mu"][3].shape == (3, DMAX, m)
        pr = fac.nowcast(t_add, y_add, t_new[:m], noise_on_new=False)
        for p in (0, 1, 2, 3, 5):                        # (particle 4's three parts do not sum to it)
            cond = reference(n, d, 1)[p].cond
            check("components nowcast at the aux limit: sum of means", out["mu"][p].sum(axis=0), pr["mu"][p],
                  TOL_PRED, cond)
        with pytest.raises(_lib.NgpError) as e:
            fac.components_nowcast(comps, t_add, y_add, t_new)
        assert e.value.status == NGP_ERR_TOO_LARGE
    finally:
        fac.close()


def test_argument_errors_return_before_the_device(ctx):
    n, d, m = 64, 3, 3
    t, y, t_add, y_add, t_new = series(n, d, m)
    fac = ctx.factor(PROGS, t, y)
    L = _lib.load()
    from nowcastautogp_amd._abi import KernelArray, dptr, iptr
    try:
        ka = KernelArray([p for c in COMPS for p in c])
        counts = np.array([len(c) for c in COMPS], np.int32)
        tot = int(counts.sum())
        mu, info = np.empty((tot, DMAX, m)), np.zeros(len(PROGS), np.int32)
        ya = np.ascontiguousarray(y_add)

        def call(d_=d, ta_=dptr(t_add), D_=DMAX, ya_=dptr(ya), counts_=counts, ka_=ka.arr, m_=m,
                 t_=dptr(t_new), mu_=dptr(mu)):
            return L.ngp_factor_components_nowcast(fac._h, d_, ta_, D_, ya_,
                                                   None if counts_ is None else iptr(counts_), ka_, m_, t_,
                                                   None, mu_, None, None, iptr(info))

        assert call() == 0
        assert call(d_=-1) == NGP_ERR_ARG
        assert call(D_=0) == NGP_ERR_ARG
        assert call(ta_=None) == NGP_ERR_ARG
        assert call(ya_=None) == NGP_ERR_ARG
        assert call(counts_=None) == NGP_ERR_ARG
        assert call(ka_=None) == NGP_ERR_ARG
        assert call(t_=None) == NGP_ERR_ARG
        assert call(mu_=None) == NGP_ERR_ARG
        assert call(m_=0) == NGP_ERR_ARG
        zero = counts.copy()
        zero[2] = 0
        assert call(counts_=zero) == NGP_ERR_ARG
        bad = [p for c in COMPS for p in c]
        bad[4] = (np.array([6], np.int32), np.zeros(0), 0.0)      # a Plus without operands
        assert call(ka_=KernelArray(bad).arr) == NGP_ERR_PROGRAM
        assert call(d_=0, ta_=None, D_=1, ya_=None) == 0          # no appended points: no arrays needed
    finally:
        fac.close()


def test_shared_y_and_per_particle_y_agree(ctx):
    n, d, m = 130, 3, 7
    t, y, t_add, y_add, t_new = series(n, d, m)
    P = len(PROGS)
    fa, fb = ctx.factor(PROGS, t, y), ctx.factor(PROGS, t, np.tile(y, (P, 1)))
    try:
        a = fa.components_nowcast(COMPS, t_add, y_add, t_new)
        b = fb.components_nowcast(COMPS, t_add, y_add, t_new)
        judge("components nowcast, per-particle y", n, d, DMAX, m, False, b, fb)
        for p, r in enumerate(reference(n, d, m)):
            check("components nowcast shared vs per-particle y", a["mu"][p], b["mu"][p], TOL_PRED, r.cond)
            check("components nowcast shared vs per-particle y", a["sigma"][p], b["sigma"][p], TOL_PRED, r.cond)
    finally:
        fa.close()
        fb.close()


def test_structured_storage_on_and_off_agree(ctx):
    n, d, m = 300, 3, 7
    t, y, t_add, y_add, t_new = series(n, d, m)
    outs = []
    try:
        for on in (True, False):
            ctx.set_structured_storage(on)
            fac = ctx.factor(PROGS, t, y)
            try:
                outs.append(fac.components_nowcast(COMPS, t_add, y_add, t_new))
                judge(f"components nowcast storage {'on' if on else 'off'}", n, d, DMAX, m, False, outs[-1], fac)
            finally:
                fac.close()
    finally:
        ctx.set_structured_storage(True)
    for p, r in enumerate(reference(n, d, m)):
        check("components nowcast storage on vs off", outs[0]["mu"][p], outs[1]["mu"][p], TOL_PRED, r.cond)
        check("components nowcast storage on vs off", outs[0]["sigma"][p], outs[1]["sigma"][p], TOL_PRED, r.cond)


@pytest.mark.parametrize("irregular", [False, True])
def test_windowed_terms_under_the_other_cp_form(ctx, irregular):
    n, d, m = 130, 3, 7
    t, y, t_add, y_add, t_new = series(n, d, m, irregular)
    sp = default_spec()
    sp.cp_form = 1
    ctx.set_spec(sp)
    try:
        fac = ctx.factor(PROGS, t, y)
        try:
            out = fac.components_nowcast(COMPS, t_add, y_add, t_new)
            judge("components nowcast cp_form 1", n, d, DMAX, m, irregular, out, fac, cp_form=1)
        finally:
            fac.close()
    finally:
        ctx.set_spec(default_spec())


def test_a_particle_that_failed_at_creation(ctx):
    """Particle 1 replaced by Periodic + Periodic of period 5 h with noise -1e-4 (the `period` matrix of
    tests/test_pivot_info_gpu.py): minor 6 of its training matrix is not positive."""
    n, d, m = 130, 3, 7
    t, y, t_add, y_add, t_new = series(n, d, m)
    per = gp.Periodic(3.0 / 5, 5 * (t[1] - t[0]), 0.5)
    bad = gp.to_program(gp.Plus(per, per)) + (-1e-4,)
    progs, comps = list(PROGS), list(COMPS)
    progs[1], comps[1] = bad, cnr.terms(bad, 0)
    _, k_ref, piv = hr.cholesky_ld(hr.cov(bad, t, t, None, add_diag=True), pivots=True)
    assert k_ref == 6 and float(piv[-1]) < -1e-6 and float(piv[:-1].min()) > 1e-6, (k_ref, piv)
    neighbours_untouched(ctx, progs, comps, t, y, t_add, y_add, t_new, 6)


def test_an_appended_block_that_is_not_positive_definite(ctx):
    """Particle 1 replaced by a short SquaredExponential with noise -1e-4 (noise + jitter = -9e-5): its
    training matrix is positive definite, the appended dates hold a duplicate, whose pivot is then
    about 2 (noise + jitter) < 0: the pivot n + 2 of the long double factorisation, n0 + k here."""
    n, d, m = 64, 3, 7
    t, y, t_add, y_add, t_new = series(n, d, m)
    t_add = t_add.copy()
    t_add[1] = t_add[0]
    bad = gp.to_program(gp.SquaredExponential(0.01, 1.0)) + (-1e-4,)
    progs, comps = list(PROGS), list(COMPS)
    progs[1], comps[1] = bad, [bad]
    tt = np.concatenate([t, t_add])
    _, k_ref, piv = hr.cholesky_ld(hr.cov(bad, tt, tt, None, add_diag=True), pivots=True)
    assert k_ref == n + 2 and float(piv[-1]) < -1e-5 and float(piv[:-1].min()) > 1e-2, (k_ref, piv)
    neighbours_untouched(ctx, progs, comps, t, y, t_add, y_add, t_new, n + 2)


def neighbours_untouched(ctx, progs, comps, t, y, t_add, y_add, t_new, want_info):
    good_progs, good_comps = list(progs), list(comps)
    good_progs[1], good_comps[1] = PROGS[0], COMPS[0]
    fac_ok, fac_bad = ctx.factor(good_progs, t, y), ctx.factor(progs, t, y)
    try:
        good = fac_ok.components_nowcast(good_comps, t_add, y_add, t_new)
        out = fac_bad.components_nowcast(comps, t_add, y_add, t_new)
    finally:
        fac_ok.close()
        fac_bad.close()
    assert out["info"][1] == want_info and not np.delete(out["info"], 1).any(), out["info"]
    assert not good["info"].any()
    assert np.isnan(out["mu"][1]).all() and np.isnan(out["var"][1]).all() and np.isnan(out["sigma"][1]).all()
    assert np.isnan(out["logml_full"][1]).all()
    for p in range(len(progs)):
        if p != 1:
            for k in ("mu", "var", "sigma"):
                assert np.array_equal(out[k][p], good[k][p]), (k, p)
            assert np.array_equal(out["logml_full"][p], good["logml_full"][p]), p


def test_forecast_components_with_nowcasts_of_a_fitted_model():
    """Same seed on both calls: offset + the weighted means of the groups is the mean of
    forecast_mixture_with_nowcasts, and per (s, p) the summed block diagonals plus noise_p / slope^2
    are that mixture's component variances (noise_p: what the predictive adds on new points, the
    particle's noise and the spec's jitter)."""
    import datetime as dt

    from nowcastautogp_amd import autogp
    from nowcastautogp_amd import nowcast as nc
    from oracle import oracle_np
    n, P, D, m = 130, 6, 4, 9
    rng = np.random.default_rng(3)
    ds = [dt.date(2020, 1, 5) + dt.timedelta(days=7 * i) for i in range(n)]
    x = np.arange(n) / n
    y = 40.0 + 25.0 * x + 6.0 * np.sin(2 * np.pi * np.arange(n) / 13.0) + rng.standard_normal(n)
    model = autogp.GPModel(ds, y, n_particles=P, seed=11)
    autogp.fit_smc(model, schedule=autogp.Schedule.linear_schedule(n, 0.5), n_mcmc=1, n_hmc=1)
    nd = [ds[-1] + dt.timedelta(days=7 * (i + 1)) for i in range(2)]
    fd = [nd[-1] + dt.timedelta(days=7 * (i + 1)) for i in range(m)]
    nows = [nc.TData(nd, list(y[-1] + 1.5 * rng.standard_normal(2)), transformation=lambda v: v)
            for _ in range(D)]
    a, b = model.clone(), model.clone()
    fc = nc.forecast_components_with_nowcasts(a, nows, fd, ess_threshold=0.5)
    mix = nc.forecast_mixture_with_nowcasts(b, nows, fd, ess_threshold=0.5)
    assert len(fc.means) == D * P and fc.date_blocks is None
    assert np.array_equal(fc.weights, mix.weights)
    t, _ = model._obs()
    conds = [np.linalg.cond(oracle_np.cov(pr, t, t, True)) for pr in model.programs()]
    slope = model.y_transform.slope
    noise = [pr[2] + default_spec().jitter for pr in model.programs()]
    for s in range(D):
        for p in range(P):
            e = s * P + p
            C = fc.means[e].shape[0]
            assert fc.sigma[e] is fc.sigma[p] and fc.var[e] is fc.var[p]
            check("forecast_components_with_nowcasts: parts + offset vs the mixture's component mean",
                  fc.means[e].sum(axis=0) + fc.offset, mix.means[e], TOL_PRED, conds[p])
            diag = np.einsum("ajbj->j", fc.sigma[e].reshape(C, m, C, m))
            check("forecast_components_with_nowcasts: blocks + noise vs the mixture's component variance",
                  diag + noise[p] / slope ** 2, mix.variances[e], TOL_PRED, conds[p])
    g = fc.grouped()
    total = sum(marg.mean() for marg in g.values()) + fc.offset
    check("forecast_components_with_nowcasts: offset + groups vs the mixture's mean", total, mix.mean(), TOL_PRED,
          max(conds))
    # the split is recorded, and the default one names the windows of a ChangePoint root
    parts = autogp.decompose(model, "changepoint")
    assert all(c.split == "changepoint" for ps in parts for c in ps)

"""ngp_factor_components on the device (include/ngp.h "additive decomposition", DESIGN.md section
4.19): the joint posterior of every particle's additive parts out of ONE query of the resident
factor, judged

  1. against the long double restatement tests/component_reference.py,
  2. against the noise-free predict of the same factor: the means add up to its mean, the blocks of
     the joint covariance to its covariance,
  3. for a particle with one component: equal to that predict,
  4. var = diag(sigma) bit for bit (also from a call without sigma), two calls the same bits,
  5. structured storage on and off,
  6. a particle that is not positive definite: info > 0, NaN outputs, the neighbours' bits unchanged,
  7. through autogp.predict_components on a small fitted model, original scale, two date blocks,

all under the suite's condition-aware comparison with the floor of the predictive moments
(tests/util.check, TOL_PRED).  Six hand-made particles with 1, 2, 3, 4, 2, 2 components (one
component a ChangePoint, one a Times with a Linear in it); n = 40 (no main block), 64 (no tail),
130 (tail of 2), 300 (several block columns, tail of 44); m = 1 and 7; a regular weekly lattice and
an irregular grid; the aux limit met exactly, and missed by one row.
"""
import functools

import numpy as np
import pytest

from nowcastautogp_amd import _lib, gp
from oracle import oracle_np
from tests import component_reference as cr
from tests import hp_reference as hr
from tests.util import TOL_PRED, check, tol

pytestmark = pytest.mark.gpu

NGP_ERR_ARG, NGP_ERR_PROGRAM, NGP_ERR_TOO_LARGE = -1, -2, -3


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    c = _lib.Context(0)
    yield c
    c.close()


def ensemble():
    trees = [
        gp.Periodic(1.0, 0.25, 0.5),
        gp.Plus(gp.Linear(0.3, 0.1, 0.8), gp.Periodic(1.2, 0.2, 0.4)),
        gp.Plus(gp.Plus(gp.Linear(0.6, 0.05, 0.5), gp.Periodic(0.9, 0.125, 0.3)),
                gp.SquaredExponential(0.1, 0.3)),
        gp.Plus(gp.Plus(gp.Constant(0.2), gp.SquaredExponential(0.15, 0.4)),
                gp.Plus(gp.Periodic(1.1, 0.3, 0.3), gp.GammaExponential(0.3, 1.5, 0.2))),
        gp.Plus(gp.ChangePoint(gp.SquaredExponential(0.2, 0.5), gp.Periodic(1.0, 0.3, 0.3), 0.5, 0.1),
                gp.Linear(0.4, 0.1, 0.6)),
        gp.Plus(gp.Times(gp.Linear(0.2, 0.1, 0.6), gp.Periodic(1.0, 0.15, 0.5)),
                gp.SquaredExponential(0.3, 0.4)),
    ]
    noise = [0.05, 0.08, 0.06, 0.1, 0.07, 0.09]
    return [gp.to_program(tr) + (nz,) for tr, nz in zip(trees, noise)]


PROGS = ensemble()
COMPS = [cr.components(p) for p in PROGS]
assert [len(c) for c in COMPS] == [1, 2, 3, 4, 2, 2]


@functools.lru_cache(maxsize=None)
def series(n, m, irregular=False):
    """(t, y, t_new): a weekly lattice on [0, 1] continued by the m query dates, or an irregular grid"""
    rng = np.random.default_rng(1000 + n)
    if irregular:
        tt = np.sort(rng.uniform(0.0, 1.0 + (m + 1.0) / n, n + m))
    else:
        tt = 7.0 * np.arange(n + m) / (7.0 * (n - 1))
    t, t_new = tt[:n].copy(), tt[n:].copy()
    y = 0.8 * (t - 0.4) + 0.5 * np.sin(2 * np.pi * t / 0.25) + 0.1 * rng.standard_normal(n)
    return t, y, t_new


@functools.lru_cache(maxsize=None)
def reference(n, m, irregular=False):
    t, y, t_new = series(n, m, irregular)
    return [cr.evaluate(p, c, t, y, t_new) for p, c in zip(PROGS, COMPS)]


def sums(mu, sigma, m):
    """(sum_c mu_c, sum_cc' Sigma_cc') of one particle"""
    C = mu.shape[0]
    return mu.sum(axis=0), sigma.reshape(C, m, C, m).sum(axis=(0, 2))


def judge(what, n, m, irregular, out, fac):
    t, y, t_new = series(n, m, irregular)
    refs = reference(n, m, irregular)
    assert not out["info"].any(), out["info"]
    pr = fac.nowcast(np.zeros(0), np.zeros((1, 0)), t_new, noise_on_new=False)
    assert not pr["info"].any()
    for p, r in enumerate(refs):
        assert r.info == 0
        mu, sg, var = out["mu"][p], out["sigma"][p], out["var"][p]
        ctx_ = (n, m, p)
        # 1. the long double restatement
        check(f"{what}: mu vs long double", mu, r.mu.astype(float), TOL_PRED, r.cond, ctx=ctx_)
        check(f"{what}: sigma vs long double", sg, r.sigma.astype(float), TOL_PRED, r.cond, ctx=ctx_)
        check(f"{what}: var vs long double", var.reshape(-1), np.diag(r.sigma).astype(float), TOL_PRED,
              r.cond, ctx=ctx_)
        # 2. the parts add up to the noise-free predict of the same factor
        smu, ssg = sums(mu, sg, m)
        check(f"{what}: sum of means vs predict", smu, pr["mu"][p, 0], TOL_PRED, r.cond, ctx=ctx_)
        check(f"{what}: sum of blocks vs predict", ssg, pr["sigma"][p], TOL_PRED, r.cond, ctx=ctx_)
        # 3. one component: the predict itself
        if mu.shape[0] == 1:
            check(f"{what}: single component vs predict", mu[0], pr["mu"][p, 0], TOL_PRED, r.cond, ctx=ctx_)
            check(f"{what}: single component vs predict", sg, pr["sigma"][p], TOL_PRED, r.cond, ctx=ctx_)
        # 4. var is the diagonal of sigma, bit for bit
        assert np.array_equal(var.reshape(-1), np.diag(sg)), ctx_
        # every diagonal block is positive semi-definite (to rounding of its own size)
        for c in range(mu.shape[0]):
            blk = sg[c * m:(c + 1) * m, c * m:(c + 1) * m]
            ev = np.linalg.eigvalsh(blk)
            assert ev[0] >= -tol(TOL_PRED, r.cond) * ev[-1], (ctx_, c, ev[0], ev[-1])


def same_bits(a, b):
    assert np.array_equal(a["info"], b["info"])
    for k in ("mu", "var", "sigma"):
        for x, y_ in zip(a[k], b[k]):
            assert np.array_equal(x, y_, equal_nan=True), k


@pytest.mark.parametrize("m", [1, 7])
@pytest.mark.parametrize("n", [40, 64, 130, 300])
def test_components_on_a_weekly_lattice(ctx, n, m):
    t, y, t_new = series(n, m)
    fac = ctx.factor(PROGS, t, y)
    try:
        out = fac.components(COMPS, t_new)
        judge("components lattice", n, m, False, out, fac)
        again = fac.components(COMPS, t_new)
        same_bits(out, again)                                   # 4. reproducible from call to call
        lean = fac.components(COMPS, t_new, want_sigma=False)   # var alone: the same bits
        assert lean["sigma"] is None
        for a, b in zip(out["var"], lean["var"]):
            assert np.array_equal(a, b)
        for a, b in zip(out["mu"], lean["mu"]):
            assert np.array_equal(a, b)
    finally:
        fac.close()


def test_components_on_an_irregular_grid(ctx):
    n, m = 130, 7
    t, y, t_new = series(n, m, True)
    fac = ctx.factor(PROGS, t, y)
    try:
        judge("components irregular", n, m, True, fac.components(COMPS, t_new), fac)
    finally:
        fac.close()


def test_the_aux_limit_exactly_and_one_row_over(ctx):
    """n = 131: a tail of 3, so 3 + 1 + C m <= 192 leaves 188 = 4 x 47 component rows"""
    n, m = 131, 47
    t, y, t_new = series(n, m)
    fac = ctx.factor(PROGS, t, y)
    try:
        judge("components at the aux limit", n, m, False, fac.components(COMPS, t_new), fac)
        t1 = np.concatenate([t_new, [t_new[-1] + (t_new[-1] - t_new[-2])]])
        with pytest.raises(_lib.NgpError) as e:
            fac.components(COMPS, t1)
        assert e.value.status == NGP_ERR_TOO_LARGE
        # the limit is per particle: without the four-component particle the longer horizon fits
        three = [c for c in COMPS]
        three[3] = COMPS[3][:3]
        out = fac.components(three, t1)
        assert not out["info"].any() and out["mu"][3].shape == (3, 48)
    finally:
        fac.close()


def test_argument_errors_return_before_the_device(ctx):
    n, m = 64, 3
    t, y, t_new = series(n, m)
    fac = ctx.factor(PROGS, t, y)
    L = _lib.load()
    from nowcastautogp_amd._abi import KernelArray, dptr, iptr
    try:
        ka = KernelArray([p for c in COMPS for p in c])
        counts = np.array([len(c) for c in COMPS], np.int32)
        tot = int(counts.sum())
        mu, info = np.empty((tot, m)), np.zeros(len(PROGS), np.int32)

        def call(counts_=counts, ka_=ka.arr, m_=m, t_=dptr(t_new), mu_=dptr(mu)):
            return L.ngp_factor_components(fac._h, None if counts_ is None else iptr(counts_), ka_, m_,
                                           t_, mu_, None, None, iptr(info))

        assert call() == 0
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
    finally:
        fac.close()


def test_any_kernels_may_stand_for_the_components(ctx):
    """The library does not check that the components sum to the particle's kernel: the formulas
    hold for any k_c (K stays the factor's), and a component's noise field is ignored."""
    n, m = 130, 7
    t, y, t_new = series(n, m)
    other = [[(c[0], c[1], 123.0) for c in COMPS[(p + 1) % len(COMPS)]] for p in range(len(PROGS))]
    fac = ctx.factor(PROGS, t, y)
    try:
        out = fac.components(other, t_new)
        assert not out["info"].any()
        for p in range(len(PROGS)):
            r = cr.evaluate(PROGS[p], other[p], t, y, t_new)
            check("components of another kernel: mu", out["mu"][p], r.mu.astype(float), TOL_PRED, r.cond)
            check("components of another kernel: sigma", out["sigma"][p], r.sigma.astype(float), TOL_PRED,
                  r.cond)
    finally:
        fac.close()


def test_structured_storage_on_and_off_agree(ctx):
    n, m = 300, 7
    t, y, t_new = series(n, m)
    refs = reference(n, m)
    outs = []
    try:
        for on in (True, False):
            ctx.set_structured_storage(on)
            fac = ctx.factor(PROGS, t, y)
            try:
                outs.append(fac.components(COMPS, t_new))
                judge(f"components storage {'on' if on else 'off'}", n, m, False, outs[-1], fac)
            finally:
                fac.close()
    finally:
        ctx.set_structured_storage(True)
    for p, r in enumerate(refs):
        check("components storage on vs off", outs[0]["mu"][p], outs[1]["mu"][p], TOL_PRED, r.cond)
        check("components storage on vs off", outs[0]["sigma"][p], outs[1]["sigma"][p], TOL_PRED, r.cond)


@pytest.mark.parametrize("n", [40, 130])
def test_a_failed_particle_reports_info_and_leaves_its_neighbours_alone(ctx, n):
    """Particle 1 replaced by Periodic + Periodic of period 5 h with noise -1e-4 (the `period` matrix of
    tests/test_pivot_info_gpu.py: rows i and i + 5 of K coincide, minor 6 is not positive) — at
    n = 130 its factor fails at creation, at n = 40 (no main block) in the tail of the query."""
    m = 7
    t, y, t_new = series(n, m)
    h = t[1] - t[0]
    per = gp.Periodic(3.0 / 5, 5 * h, 0.5)
    bad = gp.to_program(gp.Plus(per, per)) + (-1e-4,)
    progs = list(PROGS)
    progs[1] = bad
    comps = list(COMPS)
    comps[1] = cr.components(bad)
    assert len(comps[1]) == len(COMPS[1])
    _, k_ref, piv = hr.cholesky_ld(hr.cov(bad, t, t, None, add_diag=True), pivots=True)
    assert k_ref == 6 and float(piv[-1]) < -1e-6 and float(piv[:-1].min()) > 1e-6, (k_ref, piv)
    fac_ok, fac_bad = ctx.factor(PROGS, t, y), ctx.factor(progs, t, y)
    try:
        good, out = fac_ok.components(COMPS, t_new), fac_bad.components(comps, t_new)
    finally:
        fac_ok.close()
        fac_bad.close()
    assert out["info"][1] == 6 and not np.delete(out["info"], 1).any(), out["info"]
    assert np.isnan(out["mu"][1]).all() and np.isnan(out["var"][1]).all() and np.isnan(out["sigma"][1]).all()
    for p in range(len(PROGS)):
        if p != 1:
            for k in ("mu", "var", "sigma"):
                assert np.array_equal(out[k][p], good[k][p]), (k, p)


def test_predict_components_of_a_fitted_model():
    """autogp.predict_components on the original scale: the parts plus the offset add up to
    predict_mvn without noise, and a horizon of two date blocks agrees per date with single-block calls."""
    import datetime as dt

    from nowcastautogp_amd import autogp
    n = 130
    rng = np.random.default_rng(3)
    ds = [dt.date(2020, 1, 5) + dt.timedelta(days=7 * i) for i in range(n)]
    x = np.arange(n) / n
    y = 40.0 + 25.0 * x + 6.0 * np.sin(2 * np.pi * np.arange(n) / 13.0) + rng.standard_normal(n)
    model = autogp.GPModel(ds, y, n_particles=8, seed=11)
    autogp.fit_smc(model, schedule=autogp.Schedule.linear_schedule(n, 0.5), n_mcmc=1, n_hmc=1)
    parts = autogp.decompose(model)
    assert len(parts) == 8 and all(len(p) >= 1 for p in parts)
    new = [ds[-1] + dt.timedelta(days=7 * (i + 1)) for i in range(9)]
    fc = autogp.predict_components(model, new)
    mix = autogp.predict_mvn(model, new, noise_on_new=False)
    t, _ = model._obs()
    for p in range(8):
        cond = np.linalg.cond(oracle_np.cov(model.programs()[p], t, t, True))
        C = len(parts[p])
        assert fc.means[p].shape == (C, 9) and fc.sigma[p].shape == (C * 9, C * 9)
        smu, ssg = sums(fc.means[p], fc.sigma[p], 9)
        check("predict_components: parts + offset vs predict_mvn", smu + fc.offset, mix.means[p], TOL_PRED, cond)
        check("predict_components: blocks vs predict_mvn", ssg, mix.covs[p], TOL_PRED, cond)
        assert np.array_equal(fc.var[p].reshape(-1), np.diag(fc.sigma[p]))
    assert np.allclose(fc.weights, mix.weights, rtol=0, atol=1e-15)
    # a horizon that needs two date blocks (C m rows share the aux block): per date the single-block values
    Cmax = max(len(p) for p in parts)
    m_long = (192 - (n % 64) - 1) // Cmax + 3
    far = [ds[-1] + dt.timedelta(days=7 * (i + 1)) for i in range(m_long)]
    long = autogp.predict_components(model, far)
    assert long.date_blocks is not None and len(long.date_blocks) == 2
    for lo, hi in long.date_blocks:
        one = autogp.predict_components(model, far[lo:hi])
        assert one.date_blocks is None
        for p in range(8):
            assert np.array_equal(long.means[p][:, lo:hi], one.means[p])
            assert np.array_equal(long.var[p][:, lo:hi], one.var[p])
            # sigma: the single-block values inside a block of dates ...
            C, k = len(parts[p]), hi - lo
            S = long.sigma[p].reshape(C, m_long, C, m_long)
            assert np.array_equal(S[:, lo:hi, :, lo:hi], one.sigma[p].reshape(C, k, C, k))
    # ... and zeros across blocks (cross-block covariances are not formed)
    (lo0, hi0), (lo1, hi1) = long.date_blocks
    for p in range(8):
        C = len(parts[p])
        S = long.sigma[p].reshape(C, m_long, C, m_long)
        assert not S[:, lo0:hi0, :, lo1:hi1].any() and not S[:, lo1:hi1, :, lo0:hi0].any()
        assert np.array_equal(long.var[p].reshape(-1), np.diag(long.sigma[p]))
    g = fc.grouped()
    assert set(g) <= {"trend", "seasonal", "other"} and g
    for marg in g.values():
        q = marg.quantile([0.025, 0.975])
        assert q.shape == (9, 2) and np.all(q[:, 0] <= q[:, 1])

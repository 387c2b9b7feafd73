"""ngp_factor_predict_origins on the device: the forecasts of one resident factor from many forecast
origins, origin r knowing the first cut[r] observations, in ONE query.

The yardsticks are the existing entry points on a factor created on the prefix
(ngp_factor_predict_long without sigma, ngp_factor_logml), the CPU oracle on the prefix and, at
cut = n, the same factor's own long query; programs, series, floors and condition estimates are
those of tests/test_predict_long_gpu.py, the condition number that of the PREFIX matrix.

n = 20: no main block (every origin is in the conditioning block); 64: one block, no tail; 127: n0 =
64 and a tail of 63; 191: n0 = 128 and a tail of 63.  The cuts sit at 1, 2, either side of 64, of n0
and of n.  The dates start eight observations before the end of the series (for most origins: dates
after the origin but inside the series) and run beyond it; m = 65 and 300 need more than one wave of
64 date rows.
"""
import numpy as np
import pytest

from nowcastautogp_amd import _lib, autogp
from nowcastautogp_amd import nowcast as nc
from tests import mirror_contracts as mc
from tests import mixture_reference as R
from tests import value_cases as vc
from tests.engine_oracle import OracleEngine
from tests.test_predict_long_gpu import H, PROGRAMS, cond, series
from tests.util import TOL_LOGML, TOL_PRED, check

pytestmark = pytest.mark.gpu

SIZES = [20, 64, 127, 191]
MS = [1, 17, 65, 300]


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    c = _lib.Context(0)
    c.set_combining(False)
    yield c
    c.close()


def cuts_of(n):
    n0 = n // 64 * 64
    return sorted({c for c in (1, 2, 63, 64, 65, n0 - 1, n0, n0 + 1, n - 1, n) if 1 <= c <= n})


def dates(n, m):
    t, _ = series(n)
    return t[-1] + H * (np.arange(m) - 8)


_FACTORS, _PREFIX = {}, {}


def factor(ctx, n):
    if n not in _FACTORS:
        t, y = series(n)
        _FACTORS[n] = ctx.factor(PROGRAMS, t, y)
    return _FACTORS[n]


def prefix(ctx, n, c, m):
    """(mu [P, m], var [P, m], logml [P]) of a factor created on the first c observations: computed
    once and shared"""
    if (n, c, m) not in _PREFIX:
        t, y = series(n)
        f = ctx.factor(PROGRAMS, t[:c], y[:c])
        try:
            lm, info0 = f.logml()
            for mm in MS:
                mu, var, _, info = f.predict_long(dates(n, mm), want_sigma=False)
                assert not info.any() and not info0.any()
                _PREFIX[(n, c, mm)] = (mu[:, 0], var, lm)
        finally:
            f.close()
    return _PREFIX[(n, c, m)]


# ---- 1. every origin against a factor created on the prefix ----------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("m", MS)
def test_every_origin_is_the_long_query_of_the_prefix(ctx, n, m):
    t, y = series(n)
    cuts = cuts_of(n)
    mu, var, lm, info = factor(ctx, n).predict_origins(cuts, dates(n, m))
    assert not info.any() and mu.shape == var.shape == (3, len(cuts), m) and lm.shape == (3, len(cuts))
    for r, c in enumerate(cuts):
        rmu, rvar, rlm = prefix(ctx, n, c, m)
        for p in range(3):
            k = cond(p, t[:c])
            check("test_every_origin:predict_long", mu[p, r], rmu[p], TOL_PRED, k, ctx=(n, m, c, p))
            check("test_every_origin:predict_long", var[p, r], rvar[p], TOL_PRED, k, ctx=(n, m, c, p))
            check("test_every_origin:logml", lm[p, r], rlm[p], TOL_LOGML, k, ctx=(n, m, c, p))
    assert np.all(var > 0)


@pytest.mark.parametrize("n,m", [(20, 17), (64, 65), (127, 300), (191, 65)])
def test_every_origin_against_the_oracle(ctx, n, m):
    t, y = series(n)
    cuts = cuts_of(n)
    t_new = dates(n, m)
    mu, var, lm, info = factor(ctx, n).predict_origins(cuts, t_new)
    assert not info.any()
    for r, c in enumerate(cuts):
        omu, osg, olm, oinfo = OracleEngine().predict(PROGRAMS, t[:c], y[:c], t_new, True)
        assert not oinfo.any()
        for p in range(3):
            k = cond(p, t[:c])
            check("test_every_origin:oracle", mu[p, r], omu[p], TOL_PRED, k, ctx=(n, m, c, p))
            check("test_every_origin:oracle", var[p, r], np.diag(osg[p]), TOL_PRED, k, ctx=(n, m, c, p))
            check("test_every_origin:oracle_logml", lm[p, r], olm[p], TOL_LOGML, k, ctx=(n, m, c, p))


@pytest.mark.parametrize("n", SIZES)
def test_the_last_origin_is_the_factors_own_long_query(ctx, n):
    t, y = series(n)
    f = factor(ctx, n)
    for m in (17, 300):
        t_new = dates(n, m)
        mu, var, lm, info = f.predict_origins([n], t_new)
        rmu, rvar, _, rinfo = f.predict_long(t_new, want_sigma=False)
        rlm, _ = f.logml()
        assert not info.any() and not rinfo.any()
        for p in range(3):
            k = cond(p, t)
            check("test_last_origin:own_long_query", mu[p, 0], rmu[p, 0], TOL_PRED, k, ctx=(n, m, p))
            check("test_last_origin:own_long_query", var[p, 0], rvar[p], TOL_PRED, k, ctx=(n, m, p))
            check("test_last_origin:own_logml", lm[p, 0], rlm[p], TOL_LOGML, k, ctx=(n, m, p))


@pytest.mark.parametrize("n,m", [(20, 17), (127, 65), (191, 300)])
def test_per_item_data_rows(ctx, n, m):
    """a factor created with one y row per particle: row 0 of the panel, the tail part of y_c and
    every per-item offset behind them"""
    t, y = series(n)
    Y = np.stack([y, 0.5 * y + 0.1, -y])
    cuts = cuts_of(n)
    t_new = dates(n, m)
    f = ctx.factor(PROGRAMS, t, Y)
    try:
        mu, var, lm, info = f.predict_origins(cuts, t_new)
    finally:
        f.close()
    assert not info.any()
    for r, c in enumerate(cuts):
        g = ctx.factor(PROGRAMS, t[:c], Y[:, :c])
        try:
            rmu, rvar, _, rinfo = g.predict_long(t_new, want_sigma=False)
            rlm, _ = g.logml()
        finally:
            g.close()
        assert not rinfo.any()
        for p in range(3):
            k = cond(p, t[:c])
            check("test_per_item_data_rows:predict_long", mu[p, r], rmu[p, 0], TOL_PRED, k, ctx=(n, m, c, p))
            check("test_per_item_data_rows:predict_long", var[p, r], rvar[p], TOL_PRED, k, ctx=(n, m, c, p))
            check("test_per_item_data_rows:logml", lm[p, r], rlm[p], TOL_LOGML, k, ctx=(n, m, c, p))
    assert np.max(np.abs(mu[0] - mu[2])) > 1e-3      # the rows differ: so do the means


@pytest.mark.parametrize("n,m", [(20, 17), (64, 1), (127, 65), (191, 300)])
def test_without_noise_on_the_dates(ctx, n, m):
    """the flag moves the variances by the particle's noise + the default jitter and nothing else"""
    f = factor(ctx, n)
    cuts = cuts_of(n)
    mu1, var1, lm1, _ = f.predict_origins(cuts, dates(n, m), noise_on_new=True)
    mu0, var0, lm0, info = f.predict_origins(cuts, dates(n, m), noise_on_new=False)
    assert not info.any()
    np.testing.assert_array_equal(mu0, mu1)
    np.testing.assert_array_equal(lm0, lm1)
    for p in range(3):
        np.testing.assert_allclose(var1[p] - var0[p], PROGRAMS[p][2] + 1e-5, rtol=1e-9)


# ---- 2. bit-level contracts --------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(20, 65), (64, 17), (127, 300), (191, 65)])
def test_bit_level_contracts(ctx, n, m):
    f = factor(ctx, n)
    n0 = n // 64 * 64
    cuts = cuts_of(n)
    t_new = dates(n, m)
    mu, var, lm, info = f.predict_origins(cuts, t_new)
    mu2, var2, lm2, _ = f.predict_origins(cuts, t_new)
    assert not info.any()
    for a, b in ((mu, mu2), (var, var2), (lm, lm2)):                    # call to call
        np.testing.assert_array_equal(a, b)
    for r, c in enumerate(cuts):                                        # an origin alone
        mu1, var1, lm1, _ = f.predict_origins([c], t_new)
        np.testing.assert_array_equal(mu1[:, 0], mu[:, r])
        np.testing.assert_array_equal(var1[:, 0], var[:, r])
        np.testing.assert_array_equal(lm1[:, 0], lm[:, r])
    # more data never widens a forecast: exactly so in the running sums of the main block
    main = [r for r, c in enumerate(cuts) if c <= n0]
    for a, b in zip(main, main[1:]):
        assert np.all(var[:, b] <= var[:, a]), (n, m, cuts[a], cuts[b])


def test_a_failed_factorisation_stays_with_its_particle(ctx):
    from tests.test_pivot_info_gpu import failing_case, reference_k
    n, k, m = 130, 70, 70
    k_ref = reference_k("duplicate", n, k)
    bad, t, _ = failing_case("duplicate", n, k)
    _, y = vc.series(n, True, seed=41)
    good = list(vc._items(31, vc.SIZES, 3, n, 5, 7, True))
    t_new = t[-1] + (np.arange(m) - 8) / (n - 1)
    cuts = [1, 64, 100, 128, 129, 130]
    outs = []
    for progs in ([good[0], bad, good[2]], good):
        f = ctx.factor(progs, t, y)
        try:
            outs.append(f.predict_origins(cuts, t_new))
        finally:
            f.close()
    (mu, var, lm, info), (cmu, cvar, clm, cinfo) = outs
    assert not cinfo.any() and info[1] == k_ref and info[0] == 0 and info[2] == 0
    assert np.all(np.isnan(mu[1])) and np.all(np.isnan(var[1])) and np.all(np.isnan(lm[1]))
    for p in (0, 2):
        np.testing.assert_array_equal(mu[p], cmu[p])
        np.testing.assert_array_equal(var[p], cvar[p])
        np.testing.assert_array_equal(lm[p], clm[p])
    assert np.all(np.isfinite(cmu)) and np.all(np.isfinite(cvar)) and np.all(np.isfinite(clm))


# ---- 3. the mirror -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge
    ge.build()
    e = autogp.HipEngine(0)
    yield e
    e.ctx.close()


def count_calls(monkeypatch):
    calls = []
    real = _lib.Factor.predict_origins

    def predict_origins(fac, cuts, t_new, noise_on_new=True):
        calls.append(dict(cuts=list(np.asarray(cuts)), m=np.size(t_new)))
        return real(fac, cuts, t_new, noise_on_new)
    monkeypatch.setattr(_lib.Factor, "predict_origins", predict_origins)
    return calls


def test_mirror_makes_one_call_and_agrees_with_its_host_fallback(eng, monkeypatch):
    model = mc.fitted(eng, seed=5, n_particles=3)
    model.log_weights = np.array([-0.3, 0.4, 0.1])
    origins, ds = [5, 12, 12, 20], mc.days(10, 40)
    levels = np.array([0.025, 0.5, 0.975])
    with monkeypatch.context() as mp:                 # the same engine without the device call
        mp.delattr(_lib.Factor, "predict_origins")
        host, host_ess = autogp.predict_origins(model.clone(), origins, ds)
        host_w, _ = autogp.predict_origins(model.clone(), origins, ds, weights="origin")
    calls = count_calls(monkeypatch)
    got, ess = autogp.predict_origins(model, origins, ds)
    assert calls == [dict(cuts=[5, 12, 20], m=30)]
    got_w, ess_w = autogp.predict_origins(model, origins, ds, weights="origin")
    assert len(calls) == 2 and calls[1]["cuts"] == [5, 12, 20]
    fitted_w = np.exp(model.log_weights - model.log_weights.max())
    fitted_w /= fitted_w.sum()
    np.testing.assert_allclose(ess, host_ess, rtol=1e-12)
    for r in range(4):
        assert got[r].means.shape == host[r].means.shape == (3, 30)
        np.testing.assert_allclose(got[r].weights, fitted_w, rtol=1e-12)
        R.check_quantiles(f"predict_origins[{r}]", R.Mixture(host[r].weights, host[r].means, host[r].variances),
                          levels, got[r].quantile(levels))
        np.testing.assert_allclose(got_w[r].weights, host_w[r].weights, rtol=1e-7, atol=1e-12)
    # reweighting by the evidence of the whole series is no reweighting
    np.testing.assert_allclose(got_w[3].weights, fitted_w, rtol=1e-12, atol=1e-12)
    assert not np.allclose(got_w[0].weights, fitted_w, rtol=1e-3)
    assert ess_w.shape == (4,) and np.all(ess_w >= 1.0 - 1e-12) and np.all(ess_w <= 3.0 + 1e-12)


def test_hindcast_table_is_finite_where_dates_exist(eng, monkeypatch):
    model = mc.fitted(eng, seed=5, n_particles=3)
    calls = count_calls(monkeypatch)
    origins, horizons = [5, 12, 19, 20], [1, 2, 7]
    hc = nc.hindcast(model, origins, horizons)
    assert len(calls) == 1 and calls[0]["cuts"] == origins and calls[0]["m"] == len(hc.union_dates)
    exists = np.array([[c + h - 1 < 20 for h in horizons] for c in origins])
    crps, pit = hc.crps(), hc.pit()
    assert crps.shape == (4, 3)
    assert np.array_equal(np.isfinite(crps), exists) and np.array_equal(np.isnan(crps), ~exists)
    assert np.all(crps[exists] > 0) and np.all((pit[exists] >= 0) & (pit[exists] <= 1))
    assert np.array_equal(np.isfinite(hc.quantile([0.5])[..., 0]), exists)

"""ngp_factor_predict_long on the device: a horizon of up to 4,096 dates from the resident factor in
ONE query (the dates are the panel of a triangular solve, not aux rows).

The yardsticks are the existing entry point (ngp_factor_nowcast, where both apply), the CPU oracle
(unlimited m) and the pairwise assembly over the existing query (autogp.predict_in_blocks); floors
and condition estimates are those tests/test_gpu_parity.py uses for ngp_factor_nowcast.

Three particles: a stationary tree (GammaExp + Periodic), a tree with Linear (Linear + SqExp) and a
ChangePoint over a product (CP(Linear * SqExp, Periodic)).

The solve works the panel in tiles of LONG_TILE = 64 columns per wave, LONG_WG_TILE = 256 per
workgroup (csrc/ngp_internal.h); the panel holds y, the tail + appended points and the dates, so
at n = 64 (no tail) m = 62, 63, 64 puts 63, 64, 65 columns into it, and at n = 191 (tail 63)
m = 191, 192, 193 puts 255, 256, 257.
"""
import numpy as np
import pytest

from nowcastautogp_amd import _lib, autogp
from nowcastautogp_amd import nowcast as nc
from nowcastautogp_amd._abi import NgpSpec
from oracle import oracle_np
from tests import mirror_contracts as mc
from tests import mixture_reference as R
from tests import value_cases as vc
from tests.engine_oracle import OracleEngine
from tests.util import TOL_PRED, check

pytestmark = pytest.mark.gpu

LONG_TILE, LONG_WG_TILE = 64, 256
H = 1.0 / 200
PROGRAMS = [
    (np.array(vc.FILL_SINGLE[1][0], np.int32), np.array(vc.FILL_SINGLE[1][1], float), vc.FILL_SINGLE[1][2]),
    (np.array(vc.FILL_CHAIN[0][0], np.int32), np.array(vc.FILL_CHAIN[0][1], float), vc.FILL_CHAIN[0][2]),
    (np.array([2, 3, 7, 5, 8], np.int32),
     np.array([0.4, 0.1, 0.6, 0.2, 0.8, 0.8, 0.13, 0.7, 0.55, 0.06]), 5e-3),
]


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    c = _lib.Context(0)
    c.set_combining(False)
    yield c
    c.close()


def series(n):
    t = np.arange(n) * H
    rng = np.random.default_rng(100 + n)
    return t, np.sin(9.0 * t) + 0.3 * t + 0.1 * rng.standard_normal(n)


def query(n, d, D, m):
    t, y = series(n)
    t_add = t[-1] + H * np.arange(1, d + 1)
    rng = np.random.default_rng(7 * n + d)
    y_add = y[-1] + 0.2 * rng.standard_normal((D, d)) if d else np.zeros((1, 0))
    t_new = t[-1] + H * (d + np.arange(1, m + 1))
    return t, y, t_add, y_add, t_new


_FACTORS, _CONDS = {}, {}


def factor(ctx, n):
    if n not in _FACTORS:
        t, y = series(n)
        _FACTORS[n] = ctx.factor(PROGRAMS, t, y)
    return _FACTORS[n]


def cond(p, tt):
    key = (p, tt.size, float(tt[-1]))
    if key not in _CONDS:
        _CONDS[key] = float(np.linalg.cond(oracle_np.cov(PROGRAMS[p], tt, tt, True)))
    return _CONDS[key]


def room(n, d):
    return 192 - n % 64 - d - 1


# ---- 1. agreement with ngp_factor_nowcast where both apply ----------------------------------------
@pytest.mark.parametrize("n", [20, 64, 127, 191])
@pytest.mark.parametrize("d,D", [(0, 1), (3, 1), (3, 3), (60, 2)])
def test_agrees_with_factor_nowcast_where_both_apply(ctx, n, d, D):
    f = factor(ctx, n)
    ran = 0
    for m in (1, 17, 64, 65):
        if m > room(n, d):
            continue
        t, y, t_add, y_add, t_new = query(n, d, D, m)
        ref = f.nowcast(t_add, y_add, t_new)
        mu, var, sg, info = f.predict_long(t_new, t_add, y_add)
        assert not ref["info"].any() and not info.any()
        assert mu.shape == ref["mu"].shape and sg.shape == ref["sigma"].shape
        tt = np.concatenate([t, t_add])
        for p in range(3):
            c = cond(p, tt)
            check("test_agrees_with_factor_nowcast_where_both_apply:predictive", mu[p], ref["mu"][p],
                  TOL_PRED, c, ctx=(n, d, D, m, p))
            check("test_agrees_with_factor_nowcast_where_both_apply:predictive", sg[p], ref["sigma"][p],
                  TOL_PRED, c, ctx=(n, d, D, m, p))
        ran += 1
    if n % 64 + d + 2 <= 192:
        assert ran, "no horizon of this case fits beside the factor"


@pytest.mark.parametrize("n,d,D,m", [(20, 0, 1, 17), (127, 3, 3, 64), (191, 60, 2, 65), (64, 3, 1, 1)])
def test_without_noise_on_the_dates(ctx, n, d, D, m):
    """noise_on_new = False: no noise + jitter on the diagonal of sigma, nor in var"""
    f = factor(ctx, n)
    t, y, t_add, y_add, t_new = query(n, d, D, m)
    ref = f.nowcast(t_add, y_add, t_new, noise_on_new=False)
    mu, var, sg, info = f.predict_long(t_new, t_add, y_add, noise_on_new=False)
    mu1, var1, _, _ = f.predict_long(t_new, t_add, y_add, noise_on_new=True)
    assert not ref["info"].any() and not info.any()
    tt = np.concatenate([t, t_add])
    for p in range(3):
        c = cond(p, tt)
        check("test_without_noise_on_the_dates:predictive", mu[p], ref["mu"][p], TOL_PRED, c, ctx=(n, d, m, p))
        check("test_without_noise_on_the_dates:predictive", sg[p], ref["sigma"][p], TOL_PRED, c, ctx=(n, d, m, p))
        # the flag moves nothing but the diagonal, by the particle's noise + the default jitter
        np.testing.assert_array_equal(mu[p], mu1[p])
        np.testing.assert_allclose(var1[p] - var[p], PROGRAMS[p][2] + 1e-5, rtol=1e-9)
    np.testing.assert_array_equal(var, np.einsum("pjj->pj", sg))


@pytest.mark.parametrize("n,d,D,m", [(20, 3, 2, 40), (127, 0, 1, 17), (191, 3, 3, 65), (191, 3, 2, 300)])
def test_per_item_data_rows(ctx, n, d, D, m):
    """a factor created with one y row per particle: the panel's y' row, the tail part of y_c and
    every per-item offset behind them, against ngp_factor_nowcast of the same factor where the
    horizon fits beside it and against the oracle particle by particle"""
    t, y, t_add, y_add, t_new = query(n, d, D, m)
    Y = np.stack([y, 0.5 * y + 0.1, -y])
    f = ctx.factor(PROGRAMS, t, Y)
    try:
        mu, var, sg, info = f.predict_long(t_new, t_add, y_add)
        ref = f.nowcast(t_add, y_add, t_new) if m <= room(n, d) else None
    finally:
        f.close()
    assert not info.any()
    tt = np.concatenate([t, t_add])
    for p in range(3):
        c = cond(p, tt)
        if d:
            o = OracleEngine().nowcast(PROGRAMS[p:p + 1], t, Y[p], t_add, y_add, t_new, True)
            omu, osg = o["mu"][0], o["sigma"][0]
        else:
            a, b, _, oi = OracleEngine().predict(PROGRAMS[p:p + 1], t, Y[p], t_new, True)
            omu, osg = a[0][None], b[0]
        check("test_per_item_data_rows:oracle", mu[p], omu, TOL_PRED, c, ctx=(n, d, m, p))
        check("test_per_item_data_rows:oracle", sg[p], osg, TOL_PRED, c, ctx=(n, d, m, p))
        if ref is not None:
            check("test_per_item_data_rows:nowcast", mu[p], ref["mu"][p], TOL_PRED, c, ctx=(n, d, m, p))
            check("test_per_item_data_rows:nowcast", sg[p], ref["sigma"][p], TOL_PRED, c, ctx=(n, d, m, p))
    assert np.max(np.abs(mu[0] - mu[2])) > 1e-3      # the rows differ: so do the means


# ---- 2. beyond the room -----------------------------------------------------------------------------
def oracle(n, d, D, m):
    t, y, t_add, y_add, t_new = query(n, d, D, m)
    if d:
        o = OracleEngine().nowcast(PROGRAMS, t, y, t_add, y_add, t_new, True)
        return o["mu"], o["sigma"]
    mu, sg, _, info = OracleEngine().predict(PROGRAMS, t, y, t_new, True)
    assert not info.any()
    return mu[:, None, :], sg


def judge(what, got_mu, got_sg, ref_mu, ref_sg, tt, where):
    for p in range(3):
        c = cond(p, tt)
        check(what, got_mu[p], ref_mu[p], TOL_PRED, c, ctx=where + (p,))
        check(what, got_sg[p], ref_sg[p], TOL_PRED, c, ctx=where + (p,))


@pytest.mark.parametrize("n", [20, 191])
@pytest.mark.parametrize("d", [0, 3])
@pytest.mark.parametrize("m", [193, 300])
def test_beyond_the_room_against_the_oracle_and_the_pairwise_assembly(ctx, n, d, m):
    D = 2 if d else 1
    f = factor(ctx, n)
    t, y, t_add, y_add, t_new = query(n, d, D, m)
    assert m > room(n, d)
    mu, var, sg, info = f.predict_long(t_new, t_add, y_add)
    assert not info.any() and mu.shape == (3, D, m) and sg.shape == (3, m, m)
    tt = np.concatenate([t, t_add])
    rmu, rsg = oracle(n, d, D, m)
    judge("test_beyond_the_room:oracle", mu, sg, rmu, rsg, tt, (n, d, m))

    def call(ts):
        o = f.nowcast(t_add, y_add, ts)
        return o["mu"], o["sigma"], o["info"], None
    bmu, bsg, binfo, _ = autogp.predict_in_blocks(call, t_new, autogp.horizon_blocks(n, d, m))
    assert not binfo.any()
    judge("test_beyond_the_room:pairwise", mu, sg, bmu, bsg, tt, (n, d, m))


@pytest.mark.parametrize("n,ms,width", [(64, (62, 63, 64), LONG_TILE), (191, (191, 192, 193), LONG_WG_TILE)])
def test_panel_one_column_under_at_and_over_the_tile_width(ctx, n, ms, width):
    f = factor(ctx, n)
    for m, cols in zip(ms, (width - 1, width, width + 1)):
        assert 1 + n % 64 + m == cols                   # y, the tail, the dates
        t, y, t_add, y_add, t_new = query(n, 0, 1, m)
        mu, var, sg, info = f.predict_long(t_new)
        assert not info.any()
        rmu, rsg = oracle(n, 0, 1, m)
        judge("test_panel_tile_width:oracle", mu, sg, rmu, rsg, t, (n, m))


# ---- 3. bit-level contracts ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,D,m", [(20, 0, 1, 65), (191, 3, 3, 300), (127, 60, 2, 17), (64, 0, 1, 193)])
def test_bit_level_contracts(ctx, n, d, D, m):
    f = factor(ctx, n)
    t, y, t_add, y_add, t_new = query(n, d, D, m)
    mu, var, sg, info = f.predict_long(t_new, t_add, y_add)
    mu2, var2, sg2, info2 = f.predict_long(t_new, t_add, y_add)
    mu0, var0, sg0, info0 = f.predict_long(t_new, t_add, y_add, want_sigma=False)
    assert not info.any() and not info0.any() and sg0 is None
    np.testing.assert_array_equal(var, np.einsum("pjj->pj", sg))         # var is diag(sigma)
    np.testing.assert_array_equal(mu0, mu)                                # sigma = NULL: the same bits
    np.testing.assert_array_equal(var0, var)
    for a, b in ((mu, mu2), (var, var2), (sg, sg2)):                      # call to call
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(sg, sg.transpose(0, 2, 1))              # exactly symmetric
    assert np.all(var > 0)


# ---- 4. faults stay per item ----------------------------------------------------------------------------
def test_a_failed_factorisation_stays_with_its_particle(ctx):
    from tests.test_pivot_info_gpu import failing_case, reference_k
    n, k, m = 130, 70, 200
    k_ref = reference_k("duplicate", n, k)
    bad, t, _ = failing_case("duplicate", n, k)
    _, y = vc.series(n, True, seed=41)
    good = list(vc._items(31, vc.SIZES, 3, n, 5, 7, True))
    t_new = t[-1] + (1 + np.arange(m)) / (n - 1)
    outs = []
    for progs in ([good[0], bad, good[2]], good):
        f = ctx.factor(progs, t, y)
        try:
            outs.append(f.predict_long(t_new))
        finally:
            f.close()
    (mu, var, sg, info), (cmu, cvar, csg, cinfo) = outs
    assert not cinfo.any() and info[1] == k_ref and info[0] == 0 and info[2] == 0
    assert np.all(np.isnan(mu[1])) and np.all(np.isnan(var[1])) and np.all(np.isnan(sg[1]))
    for p in (0, 2):
        np.testing.assert_array_equal(mu[p], cmu[p])
        np.testing.assert_array_equal(var[p], cvar[p])
        np.testing.assert_array_equal(sg[p], csg[p])


def test_the_conditioning_block_reports_its_pivot(ctx):
    """tests/test_pivot_info_gpu.py has no appended point ON a training date at jitter 0; its
    duplicate case with k = n + 1 is that construction under the default jitter (the appended point
    repeats the last training date, noise -1e-4), its margins asserted by the long-double
    factorisation there — used here instead."""
    from tests.test_pivot_info_gpu import failing_case, reference_k
    n, d, m = 130, 3, 200
    k = n + 1
    k_ref = reference_k("duplicate", n, k, d)
    bad, t, t_add = failing_case("duplicate", n, k, d)
    assert t_add[0] == t[-1]
    _, y = vc.series(n, True, seed=41)
    good = list(vc._items(31, vc.SIZES, 3, n, 5, 7, True))
    y_add = np.random.default_rng(5).standard_normal((2, d))
    t_new = t[-1] + (d + 1 + np.arange(m)) / (n - 1)
    f = ctx.factor([good[0], bad, good[2]], t, y)
    try:
        _, info0 = f.logml()
        mu, var, sg, info = f.predict_long(t_new, t_add, y_add)
        ref = f.nowcast(t_add, y_add, t_new[:5])
    finally:
        f.close()
    assert not info0.any()                      # the training matrix itself is fine
    assert info[1] == k_ref == ref["info"][1] and info[0] == 0 and info[2] == 0
    assert np.all(np.isnan(mu[1])) and np.all(np.isnan(var[1])) and np.all(np.isnan(sg[1]))
    assert np.all(np.isfinite(mu[[0, 2]])) and np.all(np.isfinite(sg[[0, 2]]))


# ---- 5. the mirror -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge
    ge.build()
    e = autogp.HipEngine(0)
    yield e
    e.ctx.close()


class Counter:
    def __init__(self, monkeypatch):
        self.long, self.nowcast = [], []
        real_long, real_now = _lib.Factor.predict_long, _lib.Factor.nowcast
        outer = self

        def predict_long(fac, t_new, t_add=None, y_add=None, noise_on_new=True, want_sigma=True):
            outer.long.append(dict(m=np.size(t_new), want_sigma=want_sigma))
            return real_long(fac, t_new, t_add, y_add, noise_on_new, want_sigma)

        def nowcast(fac, t_add, y_add, t_new, noise_on_new=True):
            outer.nowcast.append(np.size(t_new))
            return real_now(fac, t_add, y_add, t_new, noise_on_new)
        monkeypatch.setattr(_lib.Factor, "predict_long", predict_long)
        monkeypatch.setattr(_lib.Factor, "nowcast", nowcast)


def scenarios():
    ident = lambda v: v  # noqa: E731
    return [nc.TData(mc.days(20, 22), v, transformation=ident) for v in ([111.0, 112.0], [109.0, 113.0])]


def test_mirror_makes_one_long_query(eng, monkeypatch):
    model = mc.fitted(eng, seed=5, n_particles=3)
    cnt = Counter(monkeypatch)
    mix = autogp.predict_mvn(model, mc.days(20, 320))
    assert [c["m"] for c in cnt.long] == [300] and cnt.nowcast == []
    assert mix.covs.shape == (3, 300, 300) and mix.sampler is None
    fcn = nc.forecast_with_nowcasts(model, scenarios(), mc.days(22, 322), 3)
    assert fcn.shape == (300, 6) and np.isfinite(fcn).all()
    assert [c["m"] for c in cnt.long] == [300, 300]
    assert cnt.nowcast == [0]                       # the weight update: a query without dates


def test_forecast_mixture_never_receives_an_m_by_m_array(eng, monkeypatch):
    model = mc.fitted(eng, seed=5, n_particles=3)
    dates, ndates = mc.days(20, 320), mc.days(22, 322)
    levels = np.array([0.025, 0.5, 0.975])
    # the pairwise path's marginals first: the same engine without the long query
    with monkeypatch.context() as mp:
        mp.delattr(_lib.Factor, "predict_long")
        pair = nc.forecast_mixture(model.clone(), dates)
        pair_n = nc.forecast_mixture_with_nowcasts(model.clone(), scenarios(), ndates)
    cnt = Counter(monkeypatch)
    mix = nc.forecast_mixture(model.clone(), dates)
    assert cnt.long == [dict(m=300, want_sigma=False)] and cnt.nowcast == []
    mix_n = nc.forecast_mixture_with_nowcasts(model.clone(), scenarios(), ndates)
    assert cnt.long[1:] == [dict(m=300, want_sigma=False)] and cnt.nowcast == [0]
    for label, got, ref in (("forecast_mixture", mix, pair), ("with nowcasts", mix_n, pair_n)):
        assert got.means.shape == ref.means.shape == got.variances.shape
        np.testing.assert_allclose(got.weights, ref.weights, rtol=1e-12)
        R.check_quantiles(label, R.Mixture(ref.weights, ref.means, ref.variances), levels,
                          got.quantile(levels))

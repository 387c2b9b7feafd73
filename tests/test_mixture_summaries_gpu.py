"""ngp_mixture_cdf / ngp_mixture_quantiles / ngp_mixture_crps on the device against the long-double
reference (tests/c/mixture_ref.c, tolerances in tests/mixture_reference.py), their bitwise
reproducibility, the per-date info contract, and the mirror on the HIP engine.

Measured on an MI355X, worst over all cases below: CDF 5.6e-16 (bound 1e-13), quantiles 0.153 of
their bound (the eight-decade case), CRPS 5.2e-16 of T1 + T2 / 2 (bound 1e-12); DESIGN.md 4.16."""
import numpy as np
import pytest

from nowcastautogp_amd import autogp
from nowcastautogp_amd import nowcast as nc
from tests import mirror_contracts as mc
from tests import mixture_reference as R
from tests.test_mixture_summaries_cpu import shares_match

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge
    ge.build()
    e = autogp.HipEngine(0)
    yield e
    e.ctx.close()


def run_all(ctx, label, mix, only_date=-1):
    q, info = ctx.mixture_quantiles(mix.w, mix.mu, mix.var, R.LEVELS)
    assert not info.any()
    R.check_quantiles(label, mix, R.LEVELS, q)
    Y = R.y_points(mix)                                           # [5, m]
    F, info = ctx.mixture_cdf(mix.w, mix.mu, mix.var, np.ascontiguousarray(Y.T))
    assert not info.any()
    R.check_cdf(label, mix, Y.T, F)
    crps = []
    for y in Y:
        c, info = ctx.mixture_crps(mix.w, mix.mu, mix.var, y)
        assert not info.any()
        crps.append(c)
    R.check_crps(label, mix, Y, np.stack(crps), only_date)


@pytest.mark.parametrize("m", [1, 9, 52, 300])           # 300 > NGP_MAX_AUX on purpose
@pytest.mark.parametrize("Cn", [1, 2, 63, 64, 65, 1000, 3000])
def test_against_the_long_double_reference(eng, Cn, m):
    run_all(eng.ctx, f"C={Cn} m={m}", R.make_mixture(Cn, m, seed=11))


@pytest.mark.parametrize("kind", ["decades", "sparse"])
def test_spread_variances_and_zero_weights(eng, kind):
    run_all(eng.ctx, kind, R.make_mixture(1000, 9, seed=12, kind=kind))


def test_full_size(eng):
    """64 particles x 200 scenarios; the CRPS reference (82 million pairs in long double) on one
    date only, CDF and quantiles on all nine."""
    run_all(eng.ctx, "C=12800 m=9", R.make_mixture(12800, 9, seed=13), only_date=4)


def test_bitwise_reproducible(eng):
    ctx = eng.ctx
    mix = R.make_mixture(1000, 9, seed=14)
    Y = R.y_points(mix)
    x = np.ascontiguousarray(Y.T)

    def calls(w, mu, var, xx, yy):
        return (ctx.mixture_quantiles(w, mu, var, R.LEVELS)[0], ctx.mixture_cdf(w, mu, var, xx)[0],
                ctx.mixture_crps(w, mu, var, yy)[0])

    first, again = calls(mix.w, mix.mu, mix.var, x, Y[1]), calls(mix.w, mix.mu, mix.var, x, Y[1])
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)
    # a level alone equals the level inside the 23-level call
    q23 = ctx.mixture_quantiles(mix.w, mix.mu, mix.var, R.HUB_LEVELS)[0]
    for k in (0, 7, 11, 22):
        alone = ctx.mixture_quantiles(mix.w, mix.mu, mix.var, R.HUB_LEVELS[k:k + 1])[0]
        np.testing.assert_array_equal(alone[:, 0], q23[:, k])
    back = ctx.mixture_quantiles(mix.w, mix.mu, mix.var, R.HUB_LEVELS[::-1].copy())[0]
    np.testing.assert_array_equal(back[:, ::-1], q23)
    # the dates of an m = 9 call equal nine m = 1 calls
    for j in range(9):
        one = calls(mix.w, mix.mu[:, j:j + 1].copy(), mix.var[:, j:j + 1].copy(), x[j:j + 1],
                    Y[1][j:j + 1])
        for a, b in zip(first, one):
            np.testing.assert_array_equal(a[j], b[0])


def test_info_per_date(eng):
    ctx = eng.ctx
    mix = R.make_mixture(200, 9, seed=15)
    Y = R.y_points(mix)
    x = np.ascontiguousarray(Y.T)
    clean = (ctx.mixture_quantiles(mix.w, mix.mu, mix.var, R.LEVELS)[0],
             ctx.mixture_cdf(mix.w, mix.mu, mix.var, x)[0], ctx.mixture_crps(mix.w, mix.mu, mix.var, Y[0])[0])
    mu, var = mix.mu.copy(), mix.var.copy()
    assert mix.w[17] > 0 and mix.w[40] > 0 and mix.w[90] > 0
    mu[90, 3] = np.nan
    var[40, 3] = 0.0
    var[17, 6] = -1.0
    for bad_w, want in ((mix.w, {3: 41, 6: 18}), (None, {})):
        w = mix.w
        if bad_w is None:            # the same bad values under weight zero are ignored
            w = mix.w.copy()
            w[[17, 40, 90]] = 0.0
            w /= w.sum()
            ref = R.Mixture(w, mix.mu, mix.var)
        outs = (ctx.mixture_quantiles(w, mu, var, R.LEVELS), ctx.mixture_cdf(w, mu, var, x),
                ctx.mixture_crps(w, mu, var, Y[0]))
        for (val, info), base in zip(outs, clean):
            for j in range(9):
                assert info[j] == want.get(j, 0)
                if j in want:
                    assert np.all(np.isnan(val[j]))
                elif bad_w is not None:
                    np.testing.assert_array_equal(val[j], base[j])
        if bad_w is None:
            R.check_quantiles("zero-weight bad values", ref, R.LEVELS, outs[0][0])
            R.check_cdf("zero-weight bad values", ref, x, outs[1][0])
            R.check_crps("zero-weight bad values", ref, Y[0], outs[2][0])


@pytest.mark.parametrize("mode", [dict(), dict(n_hmc=1)], ids=["default", "hmc-lockstep"])
def test_mirror_mixture_is_the_one_the_draws_come_from(eng, mode):
    """24 particles x 40 scenarios x 500 draws at n = 208."""
    rng = np.random.default_rng(21)
    n = 208
    tt = np.arange(n)
    values = 50 + 0.05 * tt + 4 * np.sin(2 * np.pi * tt / 52) + rng.standard_normal(n)
    base = mc.fitted(eng, values=values, seed=9, n_particles=24, n_mcmc=1, n_hmc=1)
    nd, fd = mc.days(n, n + 2), mc.days(n + 2, n + 11)
    nows = [nc.TData(nd, list(values[-1] + 1.5 * rng.standard_normal(2)), transformation=lambda v: v)
            for _ in range(40)]
    a, b = base.clone(), base.clone()
    draws = nc.forecast_with_nowcasts(a, nows, fd, 500, **mode)
    mix = nc.forecast_mixture_with_nowcasts(b, nows, fd, **mode)
    assert mix.engine is eng and mix.means.shape == (24 * 40, 9)
    shares_match(mix, draws)
    # the engine's results equal the host path's within the tolerances of the reference
    host = autogp.MixtureMarginals(mix.means, mix.variances, mix.weights)
    ref = R.Mixture(mix.weights, mix.means, mix.variances)
    for label, mm in (("engine", mix), ("host", host)):
        R.check_quantiles(label, ref, R.LEVELS, mm.quantile(R.LEVELS))
        y = ref.centre_and_sd()[0]
        R.check_crps(label, ref, y, mm.crps(y))
        R.check_cdf(label, ref, y[:, None], mm.pit(y)[:, None])

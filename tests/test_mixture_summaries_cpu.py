"""Exact summaries of the forecast mixture, the parts that need no GPU: the three C-ABI entry points
refuse malformed calls before anything touches a device; ``MixtureMarginals`` on its host path
against the long-double reference (tests/c/mixture_ref.c) and, for one component, the textbook
Gaussian forms; ``forecast_mixture_with_nowcasts`` on the oracle engine returns the mixture that
``forecast_with_nowcasts`` draws from."""
import ctypes as C
import math

import numpy as np
import pytest

from nowcastautogp_amd import _lib, autogp
from nowcastautogp_amd import nowcast as nc
from tests import mirror_contracts as mc
from tests import mixture_reference as R
from tests.engine_oracle import OracleEngine


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def test_symbols_are_declared_and_exported(lib):
    import os
    header = open(os.path.join(R.ROOT, "include", "ngp.h")).read()
    for name in ("ngp_mixture_cdf", "ngp_mixture_quantiles", "ngp_mixture_crps"):
        assert name in _lib.SYMBOLS and f"{name}(" in header
        assert getattr(lib, name) is not None


def test_entry_points_reject_malformed_calls_without_a_gpu(lib):
    """NGP_ERR_ARG before anything touches a device: the "context" below is a block of zeros that a
    call which got as far as using it could not survive unnoticed (its lock is never taken)."""
    NGP_ERR_ARG = lib.ngp_logml_batch(None, 0, None, 0, None, None, 0, None, None)
    assert NGP_ERR_ARG != 0
    fake = C.create_string_buffer(1 << 16)
    ctx = C.cast(fake, C.c_void_p)
    Cn, m, K = 3, 2, 4
    w = np.array([0.2, 0.3, 0.5])
    mu, var = np.zeros((Cn, m)), np.ones((Cn, m))
    x, out = np.zeros((m, K)), np.zeros((m, K))
    probs = np.array([0.1, 0.5, 0.9, 0.99])
    y, info = np.zeros(m), np.zeros(m, dtype=np.int32)
    d, i = _lib.dptr, _lib.iptr

    def cdf(c=ctx, C_=Cn, m_=m, w_=w, mu_=mu, var_=var, K_=K, x_=x, out_=out, info_=info):
        return lib.ngp_mixture_cdf(c, C_, m_, None if w_ is None else d(w_),
                                   None if mu_ is None else d(mu_), None if var_ is None else d(var_),
                                   K_, None if x_ is None else d(x_),
                                   None if out_ is None else d(out_),
                                   None if info_ is None else i(info_))

    def qnt(c=ctx, C_=Cn, m_=m, w_=w, Q_=K, p_=probs, out_=out, info_=info):
        return lib.ngp_mixture_quantiles(c, C_, m_, d(w_), d(mu), d(var), Q_,
                                         None if p_ is None else d(p_),
                                         None if out_ is None else d(out_),
                                         None if info_ is None else i(info_))

    def crps(c=ctx, C_=Cn, m_=m, w_=w, y_=y, out_=y.copy(), info_=info):
        return lib.ngp_mixture_crps(c, C_, m_, d(w_), d(mu), d(var), None if y_ is None else d(y_),
                                    None if out_ is None else d(out_),
                                    None if info_ is None else i(info_))

    for call in (cdf, qnt, crps):
        assert call(c=None) == NGP_ERR_ARG                      # null context
        assert call(C_=0) == NGP_ERR_ARG and call(m_=0) == NGP_ERR_ARG
        assert call(C_=-1) == NGP_ERR_ARG and call(m_=-5) == NGP_ERR_ARG
        assert call(out_=None) == NGP_ERR_ARG and call(info_=None) == NGP_ERR_ARG
        assert call(w_=np.array([0.5, -0.1, 0.6])) == NGP_ERR_ARG       # negative weight
        assert call(w_=np.array([0.5, np.nan, 0.5])) == NGP_ERR_ARG     # non-finite weights
        assert call(w_=np.array([0.5, np.inf, 0.5])) == NGP_ERR_ARG
        assert call(w_=np.zeros(3)) == NGP_ERR_ARG                      # all zero
    assert cdf(w_=None) == NGP_ERR_ARG and cdf(mu_=None) == NGP_ERR_ARG
    assert cdf(var_=None) == NGP_ERR_ARG and cdf(x_=None) == NGP_ERR_ARG
    assert cdf(K_=0) == NGP_ERR_ARG and qnt(Q_=0) == NGP_ERR_ARG and qnt(p_=None) == NGP_ERR_ARG
    assert crps(y_=None) == NGP_ERR_ARG
    for bad in (0.0, 1.0, -0.2, 1.5, np.nan):
        assert qnt(p_=np.array([0.1, bad, 0.9, 0.99])) == NGP_ERR_ARG


@pytest.mark.parametrize("Cn", [1, 2, 37, 500])
def test_host_path_against_the_long_double_reference(Cn):
    mix = R.make_mixture(Cn, 5, seed=2)
    mm = autogp.MixtureMarginals(mix.mu, mix.var, mix.w)
    assert mm.engine is None
    q = mm.quantile(R.LEVELS)
    R.check_quantiles(f"host C={Cn}", mix, R.LEVELS, q)
    Y = R.y_points(mix)                                           # [5, m]
    F = mm.cdf(np.ascontiguousarray(Y.T))                         # [m, 5]
    R.check_cdf(f"host C={Cn}", mix, Y.T, F)
    np.testing.assert_array_equal(mm.pit(Y[1]), F[:, 1])
    R.check_crps(f"host C={Cn}", mix, Y, np.stack([mm.crps(y) for y in Y]))
    np.testing.assert_allclose(mm.mean(), mix.w @ mix.mu, rtol=1e-14)


def test_one_component_is_the_textbook_gaussian():
    mix = R.make_mixture(1, 5, seed=3)
    mm = autogp.MixtureMarginals(mix.mu, mix.var, mix.w)
    mu, sd = mix.mu[0], np.sqrt(mix.var[0])
    # q = mu + sd Phi^-1(p), Phi^-1 from the reference's own bisection on a standard normal
    z = R.ref_quantiles(R.Mixture([1.0], [[0.0]], [[1.0]]), R.LEVELS)[0]
    q = mm.quantile(R.LEVELS)
    want = mu[:, None] + sd[:, None] * z[None, :]
    # the CDF bound carried over to x: an error of 1e-13 in F moves q by 1e-13 / f(q); plus rounding
    dens = np.exp(-0.5 * z * z)[None, :] / (sd[:, None] * math.sqrt(2 * math.pi))
    bound = R.TOL_CDF / dens + 4 * np.spacing(np.abs(want))
    print("textbook quantiles: worst share of the bound", np.max(np.abs(q - want) / bound))
    assert np.all(np.abs(q - want) <= bound)
    # CRPS of N(mu, sd^2) at y: sd [ z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi) ]
    for y in R.y_points(mix):
        zz = (y - mu) / sd
        Phi = np.array([0.5 * math.erfc(-v / math.sqrt(2)) for v in zz])
        phi = np.exp(-0.5 * zz * zz) / math.sqrt(2 * math.pi)
        want = sd * (zz * (2 * Phi - 1) + 2 * phi - 1 / math.sqrt(math.pi))
        np.testing.assert_allclose(mm.crps(y), want, rtol=0, atol=1e-13 * np.max(np.abs(y - mu) + sd))


def test_interface_orientation_pool_and_bad_values():
    mix = R.make_mixture(6, 4, seed=4)
    mm = autogp.MixtureMarginals(mix.mu, mix.var, mix.w)
    assert mm.quantile([0.25, 0.5, 0.75]).shape == (4, 3) and mm.quantile(0.5).shape == (4, 1)
    assert mm.cdf(np.zeros(4)).shape == (4,) and mm.cdf(np.zeros((4, 7))).shape == (4, 7)
    assert mm.crps(np.zeros(4)).shape == (4,) and mm.pit(np.zeros(4)).shape == (4,)
    # a monotone inverse transformation applied to the exact quantiles is the quantile there
    q = mm.quantile([0.1, 0.9])
    np.testing.assert_array_equal(mm.quantile([0.1, 0.9], inv_transformation=math.exp), np.exp(q))
    np.testing.assert_array_equal(mm.quantile([0.1, 0.9], inv_transformation=np.exp), np.exp(q))
    # pool: 1 / D each, and explicit weights
    other = R.make_mixture(3, 4, seed=5)
    mo = autogp.MixtureMarginals(other.mu, other.var, other.w)
    pooled = autogp.MixtureMarginals.pool([mm, mo])
    np.testing.assert_allclose(pooled.weights, np.concatenate([mix.w / 2, other.w / 2]), rtol=1e-15)
    x = np.full(4, 0.3)
    np.testing.assert_allclose(pooled.cdf(x), 0.5 * mm.cdf(x) + 0.5 * mo.cdf(x), atol=1e-15)
    p2 = autogp.MixtureMarginals.pool([mm, mo], weights=[0.25, 0.75])
    np.testing.assert_allclose(p2.cdf(x), 0.25 * mm.cdf(x) + 0.75 * mo.cdf(x), atol=1e-15)
    # MixtureMVN.marginals: the diagonal of every covariance
    covs = np.stack([np.diag(v) + 0.01 * v.min() for v in mix.var])
    mv = autogp.MixtureMVN(mix.mu, covs, mix.w, np.random.default_rng(0))
    np.testing.assert_array_equal(mv.marginals().variances, np.einsum("kjj->kj", covs))
    # a non-positive variance under positive weight is an error, under weight zero it is ignored
    var = mix.var.copy()
    var[2, 1] = 0.0
    with pytest.raises(autogp.PosDefException):
        autogp.MixtureMarginals(mix.mu, var, mix.w).quantile([0.5])
    w0 = mix.w.copy()
    w0[2] = 0.0
    autogp.MixtureMarginals(mix.mu, var, w0).crps(np.zeros(4))
    with pytest.raises(ValueError):
        mm.quantile([0.0, 0.5])
    with pytest.raises(ValueError):
        autogp.MixtureMarginals(mix.mu, mix.var[:, :2], mix.w)


class SamplingOracle(OracleEngine):
    """The oracle engine plus a host stand-in for the device sampler (same signature and layout as
    ``ngp_mixture_sample``), so that ``forecast_with_nowcasts`` takes the path it takes on the
    device: all scenarios resampled first, then one sampling call."""

    def mixture_sample(self, w, mu, sigma, draws, seed):
        rng = np.random.default_rng(int(seed))
        S, P = w.shape
        m = mu.shape[2]
        L = np.linalg.cholesky(sigma)
        out = np.empty((S, draws, m))
        comp = np.empty((S, draws), dtype=np.int32)
        for s in range(S):
            comp[s] = rng.choice(P, size=draws, p=w[s])
            z = rng.standard_normal((draws, m))
            out[s] = mu[comp[s], s] + np.einsum("dij,dj->di", L[comp[s]], z)
        return out, comp, np.zeros(P, dtype=np.int32)


def shares_match(mixture, draws, levels=R.LEVELS, alpha=1e-9):
    """Hoeffding at fixed points with a union bound over the m x Q quantiles: the share of the n
    pooled draws below each exact quantile is within eps of its level with probability 1 - alpha
    (valid for equal draws per scenario: a sum of independent bounded terms)."""
    q = mixture.quantile(levels)
    m, n = draws.shape
    eps = math.sqrt(math.log(2 * m * len(levels) / alpha) / (2 * n))
    assert eps <= 0.03, eps
    share = (draws[:, None, :] <= q[:, :, None]).mean(axis=2)
    worst = float(np.max(np.abs(share - np.asarray(levels)[None, :])))
    print(f"worst |share - level| = {worst:.4f} (eps {eps:.4f}, n = {n})")
    assert worst <= eps, (worst, eps)


@pytest.mark.parametrize("mode", [dict(), dict(ess_threshold=1.0), dict(n_hmc=1),
                                  dict(n_hmc=1, lockstep=False)],
                         ids=["default", "resampled", "hmc-lockstep", "hmc-loop"])
def test_mixture_is_the_one_forecast_with_nowcasts_draws_from(mode):
    eng = SamplingOracle()
    values = np.array([10.0, 15, 12, 18, 22, 25, 20, 16, 14, 11])
    base = mc.fitted(eng, values=values, seed=7, n_particles=4)
    nd, fd = mc.days(10, 12), mc.days(12, 15)
    rng = np.random.default_rng(5)
    nows = [nc.TData(nd, list(12.0 + 1.5 * rng.standard_normal(2)), transformation=lambda v: v)
            for _ in range(4)]
    per = 4500                                                    # n = 18,000: eps = 0.0268
    a, b = base.clone(), base.clone()                             # same snapshot, same streams
    draws = nc.forecast_with_nowcasts(a, nows, fd, per, **mode)
    mix = nc.forecast_mixture_with_nowcasts(b, nows, fd, **mode)
    assert isinstance(mix, autogp.MixtureMarginals)
    assert mix.means.shape == (4 * 4, 3) and abs(mix.weights.sum() - 1) < 1e-12
    shares_match(mix, draws)
    # both consumed the same from the base model's shared stream
    assert a.rng_shared.integers(0, 2**62) == b.rng_shared.integers(0, 2**62)


def test_single_model_mixture_and_argument_checks():
    eng = SamplingOracle()
    base, multi = mc.nowcast_fixture(eng)
    fd = mc.days(12, 14)
    mix = nc.forecast_mixture(base, fd)
    ref = autogp.predict_mvn(base, fd)
    np.testing.assert_array_equal(mix.means, ref.means)
    np.testing.assert_array_equal(mix.variances, np.einsum("kjj->kj", ref.covs))
    shares_match(mix, nc.forecast(base.clone(), fd, 20000), levels=R.HUB_LEVELS)
    # the asserts of forecast_with_nowcasts (test/test_nowcast_functions.jl:218-275)
    with pytest.raises(AssertionError):
        nc.forecast_mixture_with_nowcasts(base, [], fd)
    with pytest.raises(AssertionError):
        nc.forecast_mixture_with_nowcasts(base, multi, fd, n_mcmc=1, n_hmc=0)
    for bad in (-0.1, 1.5):
        with pytest.raises(AssertionError):
            nc.forecast_mixture_with_nowcasts(base, multi, fd, ess_threshold=bad)
    with pytest.raises(TypeError):
        nc.forecast_mixture_with_nowcasts(base, multi, fd, forecast_n_hmc=1)

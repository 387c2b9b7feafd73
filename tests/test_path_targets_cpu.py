"""Trajectory targets without a device: the host path of ``autogp.path_targets`` against the
restatement (tests/path_targets_reference.py), the device-struct descriptions of the named
transformations against ``get_transformations``' own inverses, the rank formula, and what the GPU
tests assume about their inputs."""
import numpy as np
import pytest

from nowcastautogp_amd import _abi, autogp
from nowcastautogp_amd import nowcast as nc
from oracle import oracle_np
from tests import path_targets_reference as R
from tests.engine_oracle import OracleEngine


class PhiloxOracle(OracleEngine):
    """The oracle engine plus the library's sampler stream restated on the host."""

    def mixture_sample(self, w, mu, sigma, draws, seed):
        out, comp = oracle_np.mixture_sample(w, mu, sigma, draws, seed)
        return out, comp, np.zeros(w.shape[1], dtype=np.int32)


def test_abi_mirror_of_the_structs():
    import ctypes as C
    assert C.sizeof(_abi.NgpInvTransform) == 32 and C.sizeof(_abi.NgpPathTarget) == 24
    assert _abi.NgpPathTarget.thr.offset == 16 and _abi.NgpInvTransform.lam.offset == 8
    assert (R.IDENTITY, R.EXP, R.LOGISTIC100, R.BOXCOX) == (
        _abi.NGP_INV_IDENTITY, _abi.NGP_INV_EXP, _abi.NGP_INV_LOGISTIC100, _abi.NGP_INV_BOXCOX)
    assert autogp.TARGET_KINDS == dict(sum=R.SUM, max=R.MAX, diff=R.DIFF, argmax=R.ARGMAX, exceed=R.EXCEED)


@pytest.mark.parametrize("N,p,k", [(1, 0.01, 1), (1, 0.99, 1), (4, 0.25, 1), (4, 0.5, 2), (4, 0.75, 3),
                                   (4, 0.76, 4), (100, 0.01, 1), (100, 0.99, 99), (10**6, 0.5, 500000),
                                   (10**6, 0.999999, 999999), (3, 0.9999999, 3), (7, 1e-12, 1)])
def test_rank_formula(N, p, k):
    assert R.rank(p, N) == k and autogp.quantile_rank(p, N) == k
    x = np.arange(1.0, N + 1.0) if N <= 100 else None
    if x is not None:       # the order statistic it names: the smallest x with share(<= x) >= p
        assert np.sort(x)[k - 1] == x[np.searchsorted(np.arange(1, N + 1) / N, p - 1e-15)]


def _grid(lam):
    """model-scale points that reach every branch: the pole and the 1e-10 floor of the base on
    both sides, the clamp at 0, overflow, and ordinary values"""
    pts = [-1e300, -800.0, -50.0, -5.0, -1.0, -1e-9, 0.0, 1e-9, 0.5, 1.0, 5.0, 50.0, 800.0, 1e300]
    if lam != 0.0:
        pole = -1.0 / lam
        for eps in (0.0, 1e-13, 1e-11, 1e-10, 1e-9, 1e-6, 1e-3):
            pts += [pole + eps / abs(lam), pole - eps / abs(lam)]
        pts += [(1e-10 - 1.0) / lam, 1e5 / lam, -1e5 / lam]
    return np.array(pts)


@pytest.mark.parametrize("name,values", [("positive", [0.0, 2.0, 5.0, 9.0]), ("positive", [1.0, 2.0, 5.0]),
                                         ("percentage", [0.0, 20.0, 55.0, 90.0]),
                                         ("percentage", [10.0, 20.0, 55.0])])
def test_named_inverses_are_described_by_their_struct(name, values):
    _, inv = nc.get_transformations(name, values)
    kind, lam, offset, cap = inv.ngp_inv
    assert kind == (R.EXP if name == "positive" else R.LOGISTIC100)
    assert offset == (min(v for v in values if v > 0) / 2 if min(values) == 0 else 0.0)
    x = _grid(0.0)
    with np.errstate(all="ignore"):
        np.testing.assert_array_equal(R.inv_numpy(inv.ngp_inv)(x), inv(x) + 0.0)
    assert R.inv_numpy(inv.ngp_inv)(np.array([-800.0]))[0] == 0.0 or offset == 0.0


@pytest.mark.parametrize("lam", [0.5, 2.0, 0.04, -0.3, -2.0, -0.01, 0.0])
@pytest.mark.parametrize("offset", [0.0, 0.75])
def test_boxcox_inverse_is_described_by_its_struct(lam, offset):
    inv = nc._inv_boxcox(lam, offset, 40.0)
    assert inv.ngp_inv == (R.BOXCOX, lam, offset, 40000.0)
    x = _grid(lam)
    got, want = R.inv_numpy(inv.ngp_inv)(x), inv(x)
    np.testing.assert_array_equal(got, want + 0.0)
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0) and not np.any(np.signbit(got))
    if lam < 0:         # the three regions of the rule are all on the grid
        base = lam * x + 1.0
        assert np.any(base <= 0) and np.any((base > 0) & (base <= 1e-10)) and np.any(base > 1e-10)
        assert np.any(got == 40000.0 - offset)
    if 0 <= lam < 1:    # the power (the exponential) overflows at 1e300: the largest finite number
        assert got[x == 1e300][0] == np.finfo(float).max


def test_fitted_boxcox_carries_its_struct():
    vals = np.array([3.0, 8.0, 1.0, 20.0, 6.0, 2.5, 11.0])
    _, inv = nc.get_transformations("boxcox", vals)
    kind, lam, offset, cap = inv.ngp_inv
    assert kind == R.BOXCOX and offset == 0.0 and cap == 1000.0 * 20.0 and np.isfinite(lam)
    x = np.linspace(-3.0, 6.0, 41)
    np.testing.assert_array_equal(R.inv_numpy(inv.ngp_inv)(x), inv(x) + 0.0)


@pytest.mark.parametrize("name", ["n257_boxcox_neg", "shared_s5", "indep_s5", "n63_exp", "one_path"])
def test_host_path_equals_the_restatement(name):
    c = R.make_case(name)
    ref = R.restate(**c)
    eng = PhiloxOracle()
    if not np.isscalar(c["seed"]):     # independent mixtures: S calls of the sampler with S = 1
        eng.mixture_sample_indep = lambda w, mu, sg, d, seeds: (
            np.stack([oracle_np.mixture_sample(w[s:s + 1], mu[s][:, None, :], sg[s], d, seeds[s])[0][0]
                      for s in range(len(seeds))]), None, np.zeros(w.shape, dtype=np.int32))
    g = R.inv_numpy(c["inv"])
    g.ngp_inv = c["inv"]              # no device entry on this engine: still the host path
    for inv_t in (g, lambda y: R.inv_numpy(c["inv"])(y)):
        res = autogp.path_targets((c["w"], c["mu"], c["sigma"]), c["targets"], c["probs"], c["draws"],
                                  c["seed"], inv_t, engine=eng, want_values=True)
        assert not res.device
        np.testing.assert_array_equal(res._values, ref["values"])
        np.testing.assert_array_equal(res.q, ref["q"])
        np.testing.assert_array_equal(res.count, ref["count"])
        np.testing.assert_array_equal(res.hist, ref["hist"])
        np.testing.assert_allclose(res._mean, ref["mean"], rtol=1e-13)
    N = res.N
    for t, (kind, j0, j1, thr) in enumerate(c["targets"][:10]):
        if kind in R.REAL:
            assert res.quantile(t).shape == (len(c["probs"]),)
            assert res.prob_above(t) == ref["count"][t] / N
        elif kind == R.ARGMAX:
            pd = res.peak_distribution(t)
            assert abs(pd.sum() - 1.0) < 1e-12 and not pd[:j0].any() and not pd[j1 + 1:].any()
            with pytest.raises(ValueError):
                res.quantile(t)
        else:
            assert res.prob_above(t) == res.mean(t)


def test_argument_checks_of_the_python_layer():
    c = R.make_case("shared_s5")
    arrs = (c["w"], c["mu"], c["sigma"])
    for bad in ([("sum", 0, 7)], [("sum", 3, 2)], [("median", 0, 1)], [("exceed", 0, 1, np.inf)], []):
        with pytest.raises((ValueError, KeyError)):
            autogp.path_targets(arrs, bad, [0.5], 5, 1, None, engine=PhiloxOracle())
    for bad in ([0.0], [1.0], []):
        with pytest.raises(ValueError):
            autogp.path_targets(arrs, [("sum", 0, 1)], bad, 5, 1, None, engine=PhiloxOracle())
    with pytest.raises(ValueError):
        autogp.path_targets(arrs, [("sum", 0, 1)], [0.5], 5, None, None, engine=PhiloxOracle())


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_gpu_cases_keep_the_pathwise_comparison_meaningful(name):
    """What tests/test_path_targets_gpu.py assumes of its inputs: where ARGMAX / EXCEED are compared
    path by path, at most 0.1 % of the paths are close enough to a tie, to thr or to a clamp value
    to be left out; the clamped case has more than half of its values at exactly 0; the constant
    case has all values equal."""
    spec = R.CASES[name]
    if name == "m192" or spec["draws"] > 5000:
        c = R.make_case(name)          # (the large ones: fewer draws tell the same about the inputs)
        c["draws"] = min(c["draws"], 3000)
    else:
        c = R.make_case(name)
    ref = R.restate(**c)
    if spec["pathwise"]:
        share = R.fragile(ref["v"], c["targets"], c["inv"]).mean(axis=1)
        assert share.max() <= R.MAX_FRAGILE_SHARE, share
        # continuous draws: a real-valued target has no ties worth speaking of
        for t, (kind, *_r) in enumerate(c["targets"]):
            if kind == R.MAX and ref["values"].shape[1] > 1:
                assert np.unique(ref["values"][t]).size >= 0.99 * ref["values"].shape[1]
    if name == "n131073_clamped":
        assert np.mean(ref["values"][1] == 0.0) > 0.5 and np.mean(ref["values"][1] > 0.0) > 0.01
    if name == "constant":
        assert all(np.unique(v).size == 1 for v in ref["values"])
    k_all = {kind for kind, *_r in c["targets"]}
    assert k_all <= {0, 1, 2, 3, 4}
    for kind, j0, j1, thr in c["targets"]:
        assert 0 <= j0 <= j1 < spec["m"]


TARGETS = [("sum", 0, 2, 40.0), ("max", 0, 2, 14.0), ("diff", 0, 2, 0.0), ("argmax", 0, 2), ("exceed", 0, 2, 15.0)]


def _fitted_positive(eng):
    from tests import mirror_contracts as mc
    values = np.array([10.0, 15, 12, 18, 22, 25, 20, 16, 14, 11])
    fwd, inv = nc.get_transformations("positive", values)
    base = mc.fitted(eng, values=[float(fwd(v)) for v in values], seed=7, n_particles=4)
    return mc, base, fwd, inv, values


def _equals_numpy_on(res, mat, probs):
    """the result against numpy functionals and summaries of the matrix [m, N] of the same paths"""
    ref = R.functionals(np.ascontiguousarray(mat.T), res.targets)
    np.testing.assert_array_equal(res._values, ref)
    own = R.summaries(ref, res.targets, probs, mat.shape[0])
    np.testing.assert_array_equal(res.q, own["q"])
    np.testing.assert_array_equal(res.count, own["count"])
    np.testing.assert_array_equal(res.hist, own["hist"])


def test_forecast_targets_summarises_the_matrix_forecast_returns():
    """One model: from one snapshot and seed, forecast_targets is numpy on forecast()'s matrix (here on
    the host path, where the one-mixture sampler call keyed by the stream's seed is the same call)."""
    mc, base, fwd, inv, _ = _fitted_positive(PhiloxOracle())
    fd, probs = mc.days(10, 13), [0.1, 0.5, 0.9]
    a, b = base.clone(), base.clone()
    mat = nc.forecast(a, fd, 300, inv_transformation=inv)
    res = nc.forecast_targets(b, fd, TARGETS, 300, probs=probs, inv_transformation=inv, want_values=True)
    assert res.N == 300 and not res.device
    _equals_numpy_on(res, mat, probs)
    assert a.rng_shared.integers(0, 2**62) == b.rng_shared.integers(0, 2**62)


@pytest.mark.parametrize("mode", [dict(), dict(ess_threshold=1.0), dict(n_hmc=1), dict(n_hmc=1, lockstep=False)],
                         ids=["default", "resampled", "hmc-lockstep", "hmc-loop"])
def test_forecast_targets_with_nowcasts_follows_forecast_with_nowcasts(mode):
    mc, base, fwd, inv, values = _fitted_positive(PhiloxOracle())
    nd, fd, probs = mc.days(10, 12), mc.days(12, 15), [0.1, 0.5, 0.9]
    rng = np.random.default_rng(5)
    nows = [nc.TData(nd, list(12.0 + 1.5 * rng.random(2)), transformation=fwd) for _ in range(3)]
    a, b = base.clone(), base.clone()
    mat = nc.forecast_with_nowcasts(a, nows, fd, 50, inv_transformation=inv, **mode)
    res = nc.forecast_targets_with_nowcasts(b, nows, fd, TARGETS, 50, probs=probs,
                                            inv_transformation=inv, want_values=True, **mode)
    assert res.N == 150
    _equals_numpy_on(res, mat, probs)
    assert a.rng_shared.integers(0, 2**62) == b.rng_shared.integers(0, 2**62)
    with pytest.raises(AssertionError):
        nc.forecast_targets_with_nowcasts(base, [], fd, TARGETS, 5)
    with pytest.raises(AssertionError):
        nc.forecast_targets_with_nowcasts(base, nows, fd, TARGETS, 5, n_mcmc=1, n_hmc=0)

"""ngp_factor_predict_long without a GPU: the symbol, its refusals before a device is touched, and
the mirror's routing (autogp.predict_mvn, nowcast.forecast_with_nowcasts, nowcast.forecast_mixture*)
through a fake engine whose resident factor records its calls and answers from the CPU oracle."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
from nowcastautogp_amd import _abi, _lib, autogp
from nowcastautogp_amd import nowcast as nc
from tests import mirror_contracts as mc
from tests.engine_oracle import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NGP_ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return _lib.load()


def test_symbol_is_bound_and_declared(lib):
    hdr = open(os.path.join(ROOT, "include", "ngp.h")).read()
    assert "ngp_factor_predict_long" in _lib.SYMBOLS
    assert re.search(r"\bngp_status\s+ngp_factor_predict_long\s*\(", hdr)
    assert hasattr(lib, "ngp_factor_predict_long")
    assert int(re.search(r"#define\s+NGP_MAX_LONG_HORIZON\s+(\d+)", hdr).group(1)) == 4096 \
        == _abi.NGP_MAX_LONG_HORIZON


def test_a_null_handle_is_refused_without_a_device(lib):
    """in the pattern of test_abi.test_round3_entry_points_reject_bad_arguments_without_a_gpu: a null
    factor is NGP_ERR_ARG whatever else is passed, before anything touches a device"""
    one = np.ones(4)
    info = np.zeros(1, np.int32)
    p, ip = _abi.dptr(one), _lib.iptr(info)
    assert lib.ngp_factor_predict_long(None, 0, None, 1, None, 4, p, 1, p, p, None, ip) == NGP_ERR_ARG
    assert lib.ngp_factor_predict_long(None, 0, None, 1, None, 0, None, 1, None, None, None, None) == NGP_ERR_ARG
    assert lib.ngp_factor_predict_long(None, -1, p, 1, p, 4, p, 1, p, p, p, ip) == NGP_ERR_ARG


# ---- the mirror's routing -------------------------------------------------------------------------
class FakeFactor:
    """What _lib.Factor offers, answered by the oracle; every query is recorded."""

    def __init__(self, eng, programs, t, y, long_query):
        self.eng, self.programs, self.t, self.y = eng, programs, np.array(t), np.array(y)
        if long_query:
            self.predict_long = self._predict_long

    def _ask(self, t_add, y_add, t_new, noise_on_new):
        t_add = np.zeros(0) if t_add is None else np.asarray(t_add, float)
        t_new = np.asarray(t_new, float)
        if t_add.size == 0:      # plain predict (the oracle's nowcast wants an appended point)
            mu, sg, lm, info = self.eng.oracle.predict(self.programs, self.t, self.y, t_new, noise_on_new)
            return dict(logml_base=lm, logml_full=lm[:, None], mu=mu[:, None, :], sigma=sg, info=info)
        y_add = np.asarray(y_add, float).reshape(-1, t_add.size)
        return self.eng.oracle.nowcast(self.programs, self.t, self.y, t_add, y_add, t_new, noise_on_new)

    def nowcast(self, t_add, y_add, t_new, noise_on_new=True):
        self.eng.calls.append(("nowcast", np.size(t_new)))
        if np.size(t_new) == 0:  # the oracle wants a date: the weight update does not depend on it
            o = self._ask(t_add, y_add, np.array([self.t[-1] + 1.0]), noise_on_new)
            return dict(o, mu=None, sigma=None)
        return self._ask(t_add, y_add, t_new, noise_on_new)

    def predict(self, t_new, noise_on_new=True):
        r = self.nowcast(np.zeros(0), np.zeros((1, 0)), t_new, noise_on_new)
        return r["mu"][:, 0], r["sigma"], r["logml_full"][:, 0], r["info"]

    def _predict_long(self, t_new, t_add=None, y_add=None, noise_on_new=True, want_sigma=True):
        self.eng.calls.append(("predict_long", np.size(t_new), bool(want_sigma)))
        o = self._ask(t_add, y_add, t_new, noise_on_new)
        var = np.einsum("pjj->pj", o["sigma"])
        return o["mu"], var, (o["sigma"] if want_sigma else None), o["info"]

    def close(self):
        pass


class FakeEngine(OracleEngine):
    def __init__(self, long_query=True):
        super().__init__()
        self.oracle, self.calls, self.long_query = OracleEngine(), [], long_query

    def factor(self, programs, t, y):
        return FakeFactor(self, programs, t, y, self.long_query)


def scenarios():
    ident = lambda v: v  # noqa: E731
    return [nc.TData(mc.days(20, 22), v, transformation=ident) for v in ([111.0, 112.0], [109.0, 113.0])]


def models():
    """the same fitted ensemble on a factor with the long query, on one without, and on the plain
    oracle engine (no resident factor at all)"""
    base = mc.fitted(OracleEngine(), seed=5, n_particles=3)
    snap = base.to_dict()
    import copy
    return [nc.GPModel.from_dict(copy.deepcopy(snap), engine=e)
            for e in (FakeEngine(True), FakeEngine(False), OracleEngine())]


def test_predict_mvn_routes_a_long_horizon_through_one_long_query():
    with_long, without, plain = models()
    long_dates, short_dates = mc.days(20, 320), mc.days(20, 60)
    a = autogp.predict_mvn(with_long, long_dates)
    assert with_long._eng().calls == [("predict_long", 300, True)]
    b = autogp.predict_mvn(without, long_dates)
    pair_calls = without._eng().calls
    blocks = autogp.horizon_blocks(20, 0, 300)
    assert len(pair_calls) == len(blocks) * (len(blocks) - 1) // 2 and all(c[0] == "nowcast" for c in pair_calls)
    c = autogp.predict_mvn(plain, long_dates)
    for other in (b, c):                      # same numbers whichever way the dates travel
        np.testing.assert_allclose(a.means, other.means, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(a.covs, other.covs, rtol=1e-9, atol=1e-9)
        np.testing.assert_array_equal(a.weights, other.weights)
    assert a.sampler is None                  # above 192 dates the draws stay on the host
    # a short horizon: the unchanged path, one aux query
    with_long._eng().calls.clear()
    s = autogp.predict_mvn(with_long, short_dates)
    assert with_long._eng().calls == [("nowcast", 40)]
    np.testing.assert_allclose(s.means, autogp.predict_mvn(plain, short_dates).means, rtol=1e-9, atol=1e-9)


def test_forecast_with_nowcasts_routes_a_long_horizon_through_one_long_query():
    with_long, without, _ = models()
    dates = mc.days(22, 322)
    a = nc.forecast_with_nowcasts(with_long, scenarios(), dates, 3)
    assert with_long._eng().calls == [("nowcast", 0), ("predict_long", 300, True)]
    b = nc.forecast_with_nowcasts(without, scenarios(), dates, 3)
    assert all(c[0] == "nowcast" and c[1] > 0 for c in without._eng().calls)
    assert a.shape == b.shape == (300, 6)
    np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-6)
    # a short horizon: one aux query, no long one
    with_long._eng().calls.clear()
    nc.forecast_with_nowcasts(with_long, scenarios(), mc.days(22, 40), 3)
    assert with_long._eng().calls == [("nowcast", 18)]


def test_forecast_mixture_asks_for_variances_alone():
    with_long, without, plain = models()
    levels = np.array([0.025, 0.5, 0.975])
    a = nc.forecast_mixture(with_long, mc.days(20, 320))
    assert with_long._eng().calls == [("predict_long", 300, False)]
    b = nc.forecast_mixture(without, mc.days(20, 320))
    assert all(c[0] == "nowcast" for c in without._eng().calls)
    c = nc.forecast_mixture(plain, mc.days(20, 320))
    for other in (b, c):
        np.testing.assert_allclose(a.means, other.means, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(a.variances, other.variances, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(a.quantile(levels), other.quantile(levels), rtol=1e-8, atol=1e-8)
    with_long._eng().calls.clear()
    without._eng().calls.clear()
    an = nc.forecast_mixture_with_nowcasts(with_long, scenarios(), mc.days(22, 322))
    assert with_long._eng().calls == [("nowcast", 0), ("predict_long", 300, False)]
    bn = nc.forecast_mixture_with_nowcasts(without, scenarios(), mc.days(22, 322))
    assert an.means.shape == bn.means.shape == (6, 300)
    np.testing.assert_allclose(an.means, bn.means, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(an.variances, bn.variances, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(an.weights, bn.weights, rtol=1e-9)
    # a short horizon keeps the aux query
    with_long._eng().calls.clear()
    nc.forecast_mixture(with_long, mc.days(20, 60))
    assert with_long._eng().calls == [("nowcast", 40)]

"""ngp_factor_sample_long without a GPU: the symbol, its refusals before a device is touched, the
mirror's routing of ``device_paths=True`` through a fake engine whose resident factor records its
calls and answers from the CPU oracle, and the yardstick of tests/test_sample_long_gpu.py.

r64_long, the worst |(x - mu_k)_i - (L z)_i| / (sqrt(sigma_ii) max(1, |z|_inf)) of the fp64 oracle
``oracle_np.mixture_sample`` against the long-double reference over the table of
tests/sample_long_cases.py, is 2.81e-14 (126 eps; case (64, 3, 3, 300, 1), cond 5.5e4) — far below
the short sampler's 2.82e-12, whose worst case is a jitter-only covariance of cond 2.4e6 that this
table, with noise on the dates, has no equal of.  The GPU test's floor is 4 r64_long.
"""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
from nowcastautogp_amd import _abi, _lib, autogp
from nowcastautogp_amd import nowcast as nc
from oracle import oracle_np
from tests import hp_reference as hr
from tests import mirror_contracts as mc
from tests import sample_long_cases as lc
from tests import sampler_cases as sc
from tests import sampler_reference as sr
from tests.engine_oracle import OracleEngine
from tests.test_predict_long_cpu import FakeEngine, FakeFactor, scenarios

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NGP_ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return _lib.load()


def test_symbol_is_bound_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "ngp.h")).read()
    assert "ngp_factor_sample_long" in _lib.SYMBOLS
    assert re.search(r"\bngp_status\s+ngp_factor_sample_long\s*\(", hdr)
    assert hasattr(lib, "ngp_factor_sample_long")
    assert hasattr(_lib.Factor, "sample_long")


def test_bad_arguments_are_refused_without_a_device(lib):
    one = np.ones(4)
    ints = np.zeros(4, np.int32)
    p, ip = _abi.dptr(one), _lib.iptr(ints)
    call = lib.ngp_factor_sample_long
    assert call(None, 0, None, 1, None, 4, p, 1, p, 1, 7, p, ip, p, p, ip, ip) == NGP_ERR_ARG
    assert call(None, 0, None, 1, None, 4, p, 1, p, 0, 7, p, ip, None, None, None, None) == NGP_ERR_ARG   # draws = 0
    assert call(None, 0, None, 1, None, 0, p, 1, p, 1, 7, p, None, None, None, None, None) == NGP_ERR_ARG  # m = 0
    assert call(None, -1, p, 1, p, 4, p, 1, p, 1, 7, p, ip, p, p, ip, ip) == NGP_ERR_ARG


# ---- the mirror's routing -----------------------------------------------------------------------------
class SamplingFactor(FakeFactor):
    """FakeFactor with the device's sample_long, answered by the oracle's moments and sampler"""

    def sample_long(self, t_new, w, draws, seed, t_add=None, y_add=None, noise_on_new=True,
                    want_moments=False):
        self.eng.calls.append(("sample_long", np.size(t_new), int(draws)))
        self.eng.seeds.append(int(seed))
        o = self._ask(t_add, y_add, t_new, noise_on_new)
        out, comp = oracle_np.mixture_sample(np.asarray(w, float).reshape(-1, o["mu"].shape[0]), o["mu"],
                                             o["sigma"], int(draws), int(seed))
        zero = np.zeros(o["mu"].shape[0], np.int32)
        return out, comp, o["info"], zero


class SamplingEngine(FakeEngine):
    def __init__(self, with_sampler=True):
        super().__init__(True)
        self.seeds, self.with_sampler = [], with_sampler

    def factor(self, programs, t, y):
        cls = SamplingFactor if self.with_sampler else FakeFactor
        return cls(self, programs, t, y, True)


def model_on(engine):
    import copy
    snap = mc.fitted(OracleEngine(), seed=5, n_particles=3).to_dict()
    return nc.GPModel.from_dict(copy.deepcopy(snap), engine=engine)


def test_forecast_with_nowcasts_draws_a_long_horizon_in_one_device_call():
    dates = mc.days(22, 322)
    a = model_on(SamplingEngine())
    twin = model_on(SamplingEngine())
    x = nc.forecast_with_nowcasts(a, scenarios(), dates, 3, device_paths=True)
    eng = a._eng()
    assert eng.calls == [("nowcast", 0), ("sample_long", 300, 3)]
    assert x.shape == (300, 6)
    # restated: the weights of the query without dates, no scenario low at threshold 0, one seed
    # from the shared stream; the oracle's moments on the model's scale
    seed = int(twin.rng_shared.integers(0, 2**63 - 1))
    assert eng.seeds == [seed]
    assert a.rng_shared.bit_generator.state == twin.rng_shared.bit_generator.state
    t, y = twin._obs()
    t_add = twin.ds_transform.apply(autogp.to_days(list(scenarios()[0].ds)))
    y_add = np.stack([twin.y_transform.apply(np.asarray(s.y, float)) for s in scenarios()])
    t_new = twin.ds_transform.apply(autogp.to_days(dates))
    o = OracleEngine().nowcast(twin.programs(), t, y, t_add, y_add, t_new, True)
    logw = twin.log_weights[:, None] + (o["logml_full"] - o["logml_base"][:, None])
    w = np.exp(logw - logw.max(axis=0))
    w = np.ascontiguousarray((w / w.sum(axis=0)).T)
    ref, _ = oracle_np.mixture_sample(w, o["mu"], o["sigma"], 3, seed)
    tr = twin.y_transform
    np.testing.assert_allclose(x, ((ref - tr.intercept) / tr.slope).reshape(6, 300).T, rtol=1e-9, atol=1e-9)
    # without the keyword: what test_forecast_with_nowcasts_routes_a_long_horizon_through_one_long_query pins
    b = model_on(SamplingEngine())
    nc.forecast_with_nowcasts(b, scenarios(), dates, 3)
    assert b._eng().calls == [("nowcast", 0), ("predict_long", 300, True)]


def test_a_low_scenario_is_resampled_in_the_device_form():
    dates = mc.days(22, 322)
    a, twin = model_on(SamplingEngine()), model_on(SamplingEngine())
    nc.forecast_with_nowcasts(a, scenarios(), dates, 3, device_paths=True, ess_threshold=1.0)
    # the short-horizon device path from the same snapshot: one multinomial over the low scenarios,
    # then one integers draw
    sc_ = nc._Scenarios(twin, scenarios(), mc.days(22, 40), ess_threshold=1.0)
    sc_.run()
    assert sc_.low.any()
    sc_.resample_for_device()
    assert a.rng_shared.bit_generator.state == twin.rng_shared.bit_generator.state


@pytest.mark.parametrize("what", ["short horizon", "refinement", "no sample_long"])
def test_device_paths_falls_back_silently(what):
    kw, dates, sampler = {}, mc.days(22, 322), True
    if what == "short horizon":
        dates = mc.days(22, 62)
    elif what == "refinement":
        kw = dict(n_hmc=2)
    else:
        sampler = False
    a, b = model_on(SamplingEngine(sampler)), model_on(SamplingEngine(sampler))
    xa = nc.forecast_with_nowcasts(a, scenarios(), dates, 3, device_paths=True, **kw)
    xb = nc.forecast_with_nowcasts(b, scenarios(), dates, 3, **kw)
    assert a._eng().calls == b._eng().calls and not any(c[0] == "sample_long" for c in a._eng().calls)
    np.testing.assert_array_equal(xa, xb)


def test_forecast_without_nowcasts_takes_the_models_weights():
    a, twin = model_on(SamplingEngine()), model_on(SamplingEngine())
    x = nc.forecast(a, mc.days(20, 320), 4, device_paths=True)
    assert a._eng().calls == [("sample_long", 300, 4)] and x.shape == (300, 4)
    assert a._eng().seeds == [int(twin.rng_shared.integers(0, 2**63 - 1))]
    nc.forecast(twin, mc.days(20, 320), 4)
    assert twin._eng().calls == [("predict_long", 300, True)]


# ---- the yardstick of the GPU test ----------------------------------------------------------------------
def test_r64_long_is_the_oracles_own_error_on_the_table():
    worst, at = 0.0, None
    for case in lc.TABLE:
        n, d, D, m, draws = case
        w, seed = lc.weights(D), lc.seed_of(case)
        comp, margin = lc.picks(w, draws, seed)
        assert margin.min() > sr.PICK_MARGIN, case
        counts = np.bincount(comp.ravel(), minlength=lc.P)
        assert counts[1] == 0
        if D == 3 and draws == 70:
            assert 15 <= counts[2] <= 17 and counts[0] > 2 * 64, (case, counts)
        mu, sg = lc.oracle_moments(case)
        x, comp64 = oracle_np.mixture_sample(w, mu, sg, draws, seed)
        ref = sr.sample(w, mu, sg, draws, seed)
        assert np.array_equal(comp64, ref.comp) and np.array_equal(comp, ref.comp) and not ref.info.any()
        e, cond = sc.scaled_errors(x, ref, mu, sg)
        if np.nanmax(e) > worst:
            worst, at = float(np.nanmax(e)), case
    print(f"r64_long = {worst:.4e} at {at}")
    assert abs(worst - lc.R64_LONG) <= 0.05 * lc.R64_LONG, (worst, at)


def test_the_noise_free_case_is_one_the_reference_can_judge():
    """without noise on the dates only particle 0's sigma factorises in long double at m = 65: the
    case puts all the weight there"""
    mu, sg = lc.oracle_moments(lc.NOISE_FREE, False)
    infos = [hr.cholesky_ld(sg[k].astype(hr.LD))[1] for k in range(lc.P)]
    assert infos[0] == 0 and infos[1] > 0 and infos[2] > 0
    w = lc.weights_noise_free(lc.NOISE_FREE[2])
    assert np.array_equal(w.max(axis=0) > 0, np.array(infos) == 0)
    _, margin = lc.picks(w, lc.NOISE_FREE[4], lc.seed_of(lc.NOISE_FREE))
    assert margin.min() > sr.PICK_MARGIN

"""ngp_factor_sample_long_indep without a GPU: the symbol and its refusals before a device is
touched, the restatement the GPU test judges against, and the mirror's routing of
``refined_device_paths=True`` through a fake engine whose resident factor records its calls and
answers from the CPU oracle.

The restatement: mixture s of a call is ``oracle_np.mixture_sample(w[s:s+1], mu_s, sigma_s, draws,
seeds[s])`` on the moments of the oracle's predict for the mixture's own items — S = 1, so the
scenario counter is 0 and the key is seeds[s], which is what include/ngp.h states.
"""
import copy
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
from tests import sample_long_indep_cases as ic
from tests import sampler_reference as sr
from tests.engine_oracle import OracleEngine
from tests.test_predict_long_cpu import FakeEngine, FakeFactor, scenarios

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NGP_ERR_ARG, NGP_ERR_TOO_LARGE = -1, -3


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return _lib.load()


def test_symbol_is_bound_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "ngp.h")).read()
    assert "ngp_factor_sample_long_indep" in _lib.SYMBOLS
    assert re.search(r"\bngp_status\s+ngp_factor_sample_long_indep\s*\(", hdr)
    assert hasattr(lib, "ngp_factor_sample_long_indep")
    assert hasattr(_lib.Factor, "sample_long_indep")
    jl = open(os.path.join(ROOT, "julia", "NGPAutoGP.jl"), encoding="utf-8").read()
    assert re.search(r"function sample_long_indep\(f::Factor", jl) and ":ngp_factor_sample_long_indep" in jl


def test_bad_arguments_are_refused_without_a_device(lib):
    import ctypes as C
    one, ints = np.ones(4), np.zeros(4, np.int32)
    seeds = np.arange(4, dtype=np.uint64)
    p, ip, sp = _abi.dptr(one), _lib.iptr(ints), seeds.ctypes.data_as(C.POINTER(C.c_uint64))
    call = lib.ngp_factor_sample_long_indep
    assert call(None, 1, 4, p, 1, p, 1, sp, p, ip, p, p, ip, ip) == NGP_ERR_ARG          # null factor
    assert call(None, 1, 4, p, 1, p, 1, None, p, None, None, None, None, None) == NGP_ERR_ARG
    assert call(None, 1, 4, p, 1, p, 0, sp, p, None, None, None, None, None) == NGP_ERR_ARG
    assert call(None, 0, 4, p, 1, p, 1, sp, p, None, None, None, None, None) == NGP_ERR_ARG


# ---- the restatement ---------------------------------------------------------------------------------
def restated(w, mu4, sg4, draws, seeds):
    """w [S, P'], mu4 [S, P', m], sg4 [S, P', m, m] -> out [S, draws, m], comp [S, draws]"""
    got = [oracle_np.mixture_sample(w[s:s + 1], np.ascontiguousarray(mu4[s][:, None, :]), sg4[s], int(draws),
                                    int(seeds[s])) for s in range(len(seeds))]
    return np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])


def test_the_case_inputs_keep_every_sigma_positive_definite():
    for n in ic.NS:
        for S, Pm in ic.FORMS:
            for m in ic.MS:
                _, sg = ic.oracle_moments(n, S, Pm, m)
                for k in range(S * Pm):
                    assert hr.cholesky_ld(sg[k].astype(hr.LD))[1] == 0, (n, S, Pm, m, k)
    assert any(8 in ic.programs(S, Pm)[k][0] for S, Pm in ic.FORMS for k in range(5))   # a ChangePoint


@pytest.mark.parametrize("case", [c for c in ic.TABLE if c[0] == 70 and c[3] != 193], ids=str)
def test_the_restatement_is_the_definition_of_the_header(case):
    """per mixture the shared form with S = 1 and seed = seeds[s] IS the independent form of the
    long-double reference (scenario counter 0, key seeds[s]): the same picks — those the stream and
    the weights alone give — and the same paths to fp64 rounding"""
    n, S, Pm, m, draws = case
    w, seeds = ic.case_weights(case), ic.seeds_of(case)
    mu, sg = ic.oracle_moments(n, S, Pm, m)
    mu4, sg4 = mu.reshape(S, Pm, m), sg.reshape(S, Pm, m, m)
    x, comp = restated(w, mu4, sg4, draws, seeds)
    ref = sr.sample_indep(w, mu4, sg4, draws, list(seeds))
    assert np.array_equal(comp, ref.comp) and ref.margin.min() > sr.PICK_MARGIN
    np.testing.assert_allclose(x, ref.x.astype(np.float64), rtol=1e-9, atol=1e-9)
    for s in range(S):
        ref_comp, _ = ic.picks(w[s], draws, seeds[s])
        assert np.array_equal(comp[s], ref_comp)
        assert 0 <= comp[s].min() and comp[s].max() < Pm and not (w[s][comp[s]] == 0).any()
        if draws == 70:
            assert np.sum(comp[s] == 0) > 64


# ---- the mirror's routing -----------------------------------------------------------------------------
class IndepFactor(FakeFactor):
    """FakeFactor with sample_long_indep, answered by the oracle's moments and sampler; refuses more
    than ``eng.most`` scenarios' items with NGP_ERR_TOO_LARGE"""

    def __init__(self, eng, programs, t, y):
        super().__init__(eng, programs, t, y, True)
        eng.calls.append(("factor", len(programs), np.ndim(y)))

    def _refuse(self, where):
        if self.eng.most is not None and len(self.programs) > self.eng.most * self.eng.per:
            raise _lib.NgpError(NGP_ERR_TOO_LARGE, where)

    def _predict_long(self, t_new, t_add=None, y_add=None, noise_on_new=True, want_sigma=True):
        self._refuse("predict_long")
        return super()._predict_long(t_new, t_add, y_add, noise_on_new, want_sigma)

    def sample_long_indep(self, t_new, w, draws, seeds, noise_on_new=True):
        self._refuse("sample_long_indep")
        seeds = [int(s) for s in seeds]
        self.eng.calls.append(("sample_long_indep", len(self.programs), np.size(t_new), int(draws)))
        self.eng.seeds.extend(seeds)
        o = self._ask(None, None, t_new, noise_on_new)
        S, P = len(seeds), len(self.programs)
        w = np.asarray(w, float).reshape(S, P // S)
        m = np.size(t_new)
        out, comp = restated(w, o["mu"][:, 0].reshape(S, P // S, m), o["sigma"].reshape(S, P // S, m, m),
                             draws, seeds)
        zero = np.zeros(P, np.int32)
        return out, comp, o["info"], zero

    def close(self):
        self.eng.calls.append(("close",))


class IndepEngine(FakeEngine):
    def __init__(self, with_indep=True, most=None, per=3):
        super().__init__(True)
        self.seeds, self.with_indep, self.most, self.per = [], with_indep, most, per

    def predict(self, programs, t, y, t_new, noise_on_new=True):
        self.calls.append(("predict", len(programs), np.size(t_new)))
        return super().predict(programs, t, y, t_new, noise_on_new)

    def factor(self, programs, t, y):
        if not self.with_indep:
            return FakeFactor(self, programs, t, y, True)
        return IndepFactor(self, programs, t, y)


SNAP = None


def model_on(engine):
    global SNAP
    if SNAP is None:
        SNAP = mc.fitted(OracleEngine(), seed=5, n_particles=3).to_dict()
    return nc.GPModel.from_dict(copy.deepcopy(SNAP), engine=engine)


LONG, SHORT, KW = mc.days(22, 222), mc.days(22, 62), dict(n_hmc=1)


def refined(engine, dates=LONG):
    sc_ = nc._Scenarios(model_on(engine), scenarios(), dates, refined_device_paths=True, **KW)
    sc_.run()
    engine.calls.clear()
    return sc_


def test_the_keyword_draws_the_refined_ensemble_on_the_device():
    eng = IndepEngine()
    a = model_on(eng)
    x = nc.forecast_with_nowcasts(a, scenarios(), LONG, 4, refined_device_paths=True, **KW)
    tail = eng.calls[-3:]
    assert tail == [("factor", 6, 2), ("sample_long_indep", 6, 200, 4), ("close",)]
    assert not any(c[0] == "predict" and c[2] > 0 and c[1] == 6 for c in eng.calls)
    assert x.shape == (200, 2 * 4) and np.isfinite(x).all()
    # the seeds: one integers draw of every clone's shared stream, in model order — where the
    # independent form of rand_lockstep takes them, so the streams end where that form leaves them
    sc_ = refined(IndepEngine())
    twins = [copy.deepcopy(m.rng_shared) for m in sc_.models]
    paths = sc_.host_matrix(4)
    assert sc_.base._eng().seeds == [int(r.integers(0, 2**63 - 1)) for r in twins] == eng.seeds
    for m_, r in zip(sc_.models, twins):
        assert m_.rng_shared.bit_generator.state == r.bit_generator.state
    np.testing.assert_array_equal(paths, x)
    # the numbers: the restated sampler on the clones' own moments (today's predict_mvn_lockstep)
    ref = refined(IndepEngine(False))
    mixes = autogp.predict_mvn_lockstep(ref.models, LONG)
    for j, mx in enumerate(mixes):
        want, _ = oracle_np.mixture_sample(mx.weights[None, :], mx.means[:, None, :], mx.covs, 4, eng.seeds[j])
        np.testing.assert_allclose(x[:, 4 * j:4 * j + 4], want[0].T, rtol=1e-9, atol=1e-9)


def test_chunks_halve_where_the_device_refuses():
    whole, halved = refined(IndepEngine()), refined(IndepEngine(most=1))
    a, b = whole.host_matrix(3), halved.host_matrix(3)
    np.testing.assert_array_equal(a, b)
    assert halved.base._eng().calls == [
        ("factor", 6, 2), ("close",),
        ("factor", 3, 1), ("sample_long_indep", 3, 200, 3), ("close",),
        ("factor", 3, 1), ("sample_long_indep", 3, 200, 3), ("close",)]
    assert halved.base._eng().seeds == whole.base._eng().seeds
    # one scenario that does not fit is the error
    with pytest.raises(_lib.NgpError) as err:
        refined(IndepEngine(most=0)).host_matrix(3)
    assert err.value.status == NGP_ERR_TOO_LARGE


@pytest.mark.parametrize("what", ["keyword off", "short horizon", "no sample_long_indep", "shared", "loop"])
def test_otherwise_todays_calls_and_todays_bits(what):
    kw, dates, on, indep = dict(KW), LONG, True, True
    if what == "keyword off":
        on = False
    elif what == "short horizon":
        dates = SHORT
    elif what == "no sample_long_indep":
        indep = False
    elif what == "shared":
        kw = {}
    else:
        kw = dict(KW, lockstep=False)
    a, b = model_on(IndepEngine(indep)), model_on(IndepEngine(indep))
    xa = nc.forecast_with_nowcasts(a, scenarios(), dates, 3, refined_device_paths=on, **kw)
    xb = nc.forecast_with_nowcasts(b, scenarios(), dates, 3, **kw)
    ca = [c for c in a._eng().calls if c[0] not in ("factor", "close")]
    cb = [c for c in b._eng().calls if c[0] not in ("factor", "close")]
    assert ca == cb and not any(c[0] == "sample_long_indep" for c in ca)
    np.testing.assert_array_equal(xa, xb)
    assert a.rng_shared.bit_generator.state == b.rng_shared.bit_generator.state


def test_targets_and_scores_take_the_paths_of_the_route():
    x = refined(IndepEngine()).host_matrix(3)
    targets = [(kind, 0, 199) for kind in sorted(autogp.TARGET_KINDS)[:2]]
    tg = nc.forecast_targets_with_nowcasts(model_on(IndepEngine()), scenarios(), LONG, targets, 3,
                                           refined_device_paths=True, want_values=True, **KW)
    tgs = autogp._target_tuples(targets, 200)
    ref = autogp.path_functionals(np.ascontiguousarray(x.T), tgs)
    for i in range(len(tgs)):
        np.testing.assert_array_equal(tg.values(i), ref[i])
    y = np.full(200, 120.0)
    got = nc.forecast_scores_with_nowcasts(model_on(IndepEngine()), scenarios(), LONG, y, 3, scale="natural",
                                           refined_device_paths=True, **KW)
    want = autogp.ensemble_scores(x, y, None, "natural", 0.0, True, None)
    np.testing.assert_allclose(got.crps, want.crps, rtol=1e-12)


def test_marginals_never_ask_for_sigma():
    eng = IndepEngine()
    got = nc.forecast_mixture_with_nowcasts(model_on(eng), scenarios(), LONG, refined_device_paths=True, **KW)
    longs = [c for c in eng.calls if c[0] == "predict_long"]
    assert longs == [("predict_long", 200, False)]
    assert not any(c[0] == "predict" and c[1] == 6 for c in eng.calls)
    want = nc.forecast_mixture_with_nowcasts(model_on(IndepEngine(False)), scenarios(), LONG, **KW)
    np.testing.assert_array_equal(got.weights, want.weights)
    np.testing.assert_allclose(got.means, want.means, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(got.variances, want.variances, rtol=1e-9, atol=1e-12)
    # chunked: the same marginals
    half = nc.forecast_mixture_with_nowcasts(model_on(IndepEngine(most=1)), scenarios(), LONG,
                                             refined_device_paths=True, **KW)
    np.testing.assert_array_equal(half.means, got.means)

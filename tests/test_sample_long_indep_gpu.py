"""ngp_factor_sample_long_indep on the device: the paths of S mixtures that share no component,
drawn in ONE call from a factor over all their items.

1. One call replaces S calls: for every mixture a factor of its own items and
   ``ngp_factor_sample_long`` (d = 0, seed = seeds[s]) give its paths, picks, moments and reports bit
   for bit — the new pick, normals and grouping against code tests/test_sample_long_gpu.py judges.
2. Against the restatement of tests/test_sample_long_indep_cpu.py, by the yardstick of
   tests/test_sample_long_gpu.py as it stands: the long-double reference fed with the device's own
   moments, every coordinate within ``tests.util.tol(sample_long_cases.FLOOR, cond(sigma_k))``.
3. The invariances of the header, 4. zero weight and failure, 5. the refusals, 6. the mirror.

The failure of (4) needs an indefinite sigma on a healthy factor.  tests/test_sample_long_gpu.py has
a construction for an ``info`` report only (an appended point, which this form does not have), so
this file builds on the "duplicate" recipe of tests/test_pivot_info_gpu.failing_case: a forecast
date that occurs twice, under a negative noise.  The 2 x 2 block of the twin dates is then
[[v + s, v], [v, v + s]] with s < 0, whose second pivot is s (2 v + s) / (v + s) < 0 whatever the
rounding; the other items, with positive noise, factorise.
"""
import numpy as np
import pytest

from nowcastautogp_amd import _lib, autogp
from nowcastautogp_amd import nowcast as nc
from oracle import oracle_np
from tests import mirror_contracts as mc
from tests import sample_long_cases as lc
from tests import sample_long_indep_cases as ic
from tests import sampler_cases as sc
from tests import sampler_reference as sr
from tests.util import TOL_PRED, check

pytestmark = pytest.mark.gpu
NGP_ERR_ARG, NGP_ERR_TOO_LARGE = -1, -3


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    c = _lib.Context(0)
    c.set_combining(False)
    yield c
    c.close()


_FACTORS = {}


def factor(ctx, n, S, Pm, only=None):
    """the factor over all S P' items, or (``only`` = s) over mixture s's items alone"""
    key = (n, S, Pm, only)
    if key not in _FACTORS:
        t, Y = ic.item_y(n, S, Pm)
        progs = ic.programs(S, Pm)
        rows = slice(None) if only is None else slice(only * Pm, (only + 1) * Pm)
        _FACTORS[key] = ctx.factor(progs[rows], t, Y[rows])
    return _FACTORS[key]


def ask(ctx, case, draws=None, w=None, seeds=None, **kw):
    n, S, Pm, m, dr = case
    return factor(ctx, n, S, Pm).sample_long_indep(
        ic.dates(n, m), ic.case_weights(case) if w is None else w, dr if draws is None else draws,
        ic.seeds_of(case) if seeds is None else seeds, **kw)


@pytest.mark.parametrize("case", ic.TABLE, ids=str)
def test_one_call_replaces_one_call_per_mixture(ctx, case):
    n, S, Pm, m, draws = case
    w, seeds = ic.case_weights(case), ic.seeds_of(case)
    out, comp, info, cinfo, mu, var = ask(ctx, case, want_moments=True)
    assert out.shape == (S, draws, m) and comp.shape == (S, draws) and mu.shape == (S * Pm, m)
    assert not info.any() and not cinfo.any() and np.isfinite(out).all()
    if draws == 70:
        assert (np.sum(comp == 0, axis=1) > 64).all()           # a second wave on every mixture's item 0
    for s in range(S):
        o1, c1, i1, ci1, mu1, var1 = factor(ctx, n, S, Pm, only=s).sample_long(
            ic.dates(n, m), w[s:s + 1], draws, seeds[s], want_moments=True)
        rows = slice(s * Pm, (s + 1) * Pm)
        assert np.array_equal(c1[0], comp[s]) and np.array_equal(o1[0], out[s]), (case, s)
        assert np.array_equal(mu1[:, 0], mu[rows]) and np.array_equal(var1, var[rows])
        assert np.array_equal(i1, info[rows]) and np.array_equal(ci1, cinfo[rows])


@pytest.mark.parametrize("case", ic.TABLE, ids=str)
def test_against_the_restatement(ctx, case):
    n, S, Pm, m, draws = case
    w, seeds = ic.case_weights(case), ic.seeds_of(case)
    out, comp, info, cinfo, mu, var = ask(ctx, case, want_moments=True)
    mu_l, var_l, sg, info_l = factor(ctx, n, S, Pm).predict_long(ic.dates(n, m))
    assert not info_l.any() and np.array_equal(mu_l[:, 0], mu) and np.array_equal(var_l, var)
    worst = 0.0
    for s in range(S):
        rows = slice(s * Pm, (s + 1) * Pm)
        mu_s, sg_s = np.ascontiguousarray(mu[rows][:, None, :]), sg[rows]
        ref = sr.sample(w[s:s + 1], mu_s, sg_s, draws, seeds[s])
        assert ref.margin.min() > sr.PICK_MARGIN and not ref.info[w[s] > 0].any()
        worst = max(worst, sc.judge(f"sample_long_indep vs reference {case} mixture {s}", out[s:s + 1],
                                    comp[s:s + 1], ref, mu_s, sg_s, floor=lc.FLOOR))
    print(f"sample_long_indep {case}: worst {worst:.3e} (floor {lc.FLOOR:.3e})")


CASE70 = (130, 3, 2, 200, 70)


def test_fewer_draws_are_the_first_of_more_and_calls_repeat(ctx):
    a, b = ask(ctx, CASE70), ask(ctx, CASE70)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    one = ask(ctx, CASE70, draws=1)
    assert np.array_equal(one[0], a[0][:, :1]) and np.array_equal(one[1], a[1][:, :1])
    assert np.array_equal(one[2], a[2]) and np.array_equal(one[3], a[3])


@pytest.mark.parametrize("case", [CASE70, (70, 2, 5, 193, 70)], ids=str)
def test_mixtures_in_reversed_order(ctx, case):
    n, S, Pm, m, draws = case
    out, comp, info, cinfo = ask(ctx, case)
    t, Y = ic.item_y(n, S, Pm)
    progs = ic.programs(S, Pm)
    order = np.concatenate([np.arange(s * Pm, (s + 1) * Pm) for s in reversed(range(S))])
    f = ctx.factor([progs[i] for i in order], t, Y[order])
    try:
        o2, c2, i2, ci2 = f.sample_long_indep(ic.dates(n, m), ic.case_weights(case)[::-1], draws,
                                              ic.seeds_of(case)[::-1])
    finally:
        f.close()
    assert np.array_equal(o2[::-1], out) and np.array_equal(c2[::-1], comp)
    assert np.array_equal(i2, info[order]) and np.array_equal(ci2, cinfo[order])


def test_one_mixture_on_a_factor_of_its_own(ctx):
    n, S, Pm, m, draws = CASE70
    out, comp, _, _ = ask(ctx, CASE70)
    for s in range(S):
        o1, c1, i1, ci1 = factor(ctx, n, S, Pm, only=s).sample_long_indep(
            ic.dates(n, m), ic.case_weights(CASE70)[s:s + 1], draws, ic.seeds_of(CASE70)[s:s + 1])
        assert not i1.any() and not ci1.any()
        assert np.array_equal(o1[0], out[s]) and np.array_equal(c1[0], comp[s])


def test_an_item_without_weight_is_not_factorised(ctx):
    case = (70, 2, 5, 65, 70)
    assert not ic.case_weights(case)[:, 1].any()
    out, comp, info, cinfo = ask(ctx, case)
    assert cinfo[1] == 0 and cinfo[6] == 0 and not (comp == 1).any() and np.isfinite(out).all()
    # also where its sigma would not factorise (the failing item below, here without weight)
    bad, f, t_new, w, seeds = failing(ctx, weight=0.0)
    try:
        o, c, i, ci = f.sample_long_indep(t_new, w, 70, seeds)
    finally:
        f.close()
    assert not i.any() and not ci.any() and not (c[1] == 1).any() and np.isfinite(o).all()


def failing(ctx, weight, healthy=False):
    """(index of the bad item, factor, dates, w, seeds): n = 70, S = 3 mixtures of 2; item 1 of mixture
    1 carries a negative noise (unless ``healthy``) and date 11 repeats date 10"""
    n, S, Pm, m = 70, 3, 2, 65
    t, Y = ic.item_y(n, S, Pm)
    progs = list(ic.programs(S, Pm))
    bad = 1 * Pm + 1
    progs[bad] = (np.array([3], np.int32), np.array([0.5 * ic.H, 1.0]), 1e-2 if healthy else -1e-2)
    t_new = ic.dates(n, m)
    t_new[11] = t_new[10]
    w = ic.weights(S, Pm)
    w[1] = [1.0 - weight, weight]
    return bad, ctx.factor(progs, t, Y), t_new, w, (501, 502, 503)


def test_a_failed_item_keeps_its_failure_to_itself(ctx):
    bad, f, t_new, w, seeds = failing(ctx, weight=0.4)
    try:
        out, comp, info, cinfo = f.sample_long_indep(t_new, w, 70, seeds)
    finally:
        f.close()
    _, g, _, _, _ = failing(ctx, weight=0.4, healthy=True)
    try:
        clean, comp_c, info_c, cinfo_c = g.sample_long_indep(t_new, w, 70, seeds)
    finally:
        g.close()
    assert not info.any() and cinfo[bad] == 12 and not np.delete(cinfo, bad).any()
    assert not info_c.any() and not cinfo_c.any() and np.isfinite(clean).all()
    assert np.array_equal(comp, comp_c)
    lost = np.zeros(comp.shape, bool)
    lost[1] = comp[1] == 1
    assert lost.any() and (~lost[1]).any()
    assert np.isnan(out[lost]).all() and np.isfinite(out[~lost]).all()
    assert np.array_equal(out[~lost], clean[~lost])


def test_refusals(ctx):
    import ctypes as C
    n, S, Pm = 70, 3, 2
    f = factor(ctx, n, S, Pm)
    lib = _lib.load()
    t_new = ic.dates(n, 4097)
    w, out = np.full(6, 0.5), np.empty(4097 * 6)
    seeds = np.arange(1, 7, dtype=np.uint64)
    sp = seeds.ctypes.data_as(C.POINTER(C.c_uint64))
    p = _lib.dptr

    def call(S_, m, draws, seeds_):
        return lib.ngp_factor_sample_long_indep(f._h, S_, m, p(t_new), 1, p(w), draws, seeds_, p(out), None,
                                                None, None, None, None)

    assert call(4, 65, 1, sp) == NGP_ERR_ARG                    # 6 items are not 4 mixtures
    assert call(3, 65, 1, None) == NGP_ERR_ARG
    assert call(3, 65, 0, sp) == NGP_ERR_ARG
    assert call(0, 65, 1, sp) == NGP_ERR_ARG
    assert call(3, 4097, 1, sp) == NGP_ERR_TOO_LARGE
    assert call(3, 65, 1, sp) == 0


# ---- the mirror -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge
    ge.build()
    e = autogp.HipEngine(0)
    yield e
    e.ctx.close()


def scenarios():
    ident = lambda v: v  # noqa: E731
    return [nc.TData(mc.days(68, 70), v, transformation=ident) for v in ([135.0, 136.0], [133.0, 137.0], [134.0, 134.5])]


def series68():
    rng = np.random.default_rng(9)
    return 100.0 + 0.5 * np.arange(1, 69) + 2.0 * rng.standard_normal(68)


def test_mirror_end_to_end(eng, monkeypatch):
    """n = 70 (68 observations and two nowcast points), 2 particles, 3 scenarios, n_hmc = 1, m = 200"""
    import copy
    model = mc.fitted(eng, values=series68(), seed=5, n_particles=2)
    dates, draws, kw = mc.days(70, 270), 4, dict(n_hmc=1)
    calls, kept = [], {}
    orig = _lib.Factor.sample_long_indep

    def wrap(self, t_new, w, k, seeds, *a, **k2):
        calls.append((self.P, np.size(t_new), int(k)))
        kept["args"] = (np.array(t_new), np.array(w), [int(s) for s in seeds])
        kept["moments"] = self.predict_long(t_new)
        return orig(self, t_new, w, k, seeds, *a, **k2)

    monkeypatch.setattr(_lib.Factor, "sample_long_indep", wrap)
    a, b = model.clone(root=11), model.clone(root=11)
    x = nc.forecast_with_nowcasts(a, scenarios(), dates, draws, refined_device_paths=True, **kw)
    assert calls == [(6, 200, draws)] and x.shape == (200, 3 * draws) and np.isfinite(x).all()
    # today's route from the same snapshot: the base model's shared stream ends where it does here
    sc_ = nc._Scenarios(b, scenarios(), dates, **kw)
    sc_.run()
    assert a.rng_shared.bit_generator.state == b.rng_shared.bit_generator.state
    # the refined clones' own moments (the long query of the very factor), the restated sampler
    t_new, w, seeds = kept["args"]
    mu, var, sg, info = kept["moments"]
    assert not info.any()
    twins = [copy.deepcopy(m_.rng_shared) for m_ in sc_.models]
    assert seeds == [int(r.integers(0, 2**63 - 1)) for r in twins]
    tr = model.y_transform
    for s in range(3):
        rows = slice(2 * s, 2 * s + 2)
        mu_s, sg_s = np.ascontiguousarray(mu[rows]), sg[rows]
        got = (x[:, s * draws:(s + 1) * draws].T * tr.slope + tr.intercept)[None]
        ref64, comp64 = oracle_np.mixture_sample(w[s:s + 1], mu_s, sg_s, draws, seeds[s])
        ref = sr.sample(w[s:s + 1], mu_s, sg_s, draws, seeds[s])
        assert np.array_equal(comp64, ref.comp)
        sc.judge(f"mirror, scenario {s}", got, None, ref, mu_s, sg_s, floor=lc.FLOOR)
    # the pooled marginals against the host route's, to the tolerance of tests/test_predict_long_gpu.py
    # (tests.util.check under TOL_PRED, at its floor: cond = 1)
    c, d = model.clone(root=11), model.clone(root=11)
    mx = nc.forecast_mixture_with_nowcasts(c, scenarios(), dates, refined_device_paths=True, **kw)
    my = nc.forecast_mixture_with_nowcasts(d, scenarios(), dates, **kw)
    np.testing.assert_allclose(mx.weights, my.weights, rtol=1e-12)
    check("mirror: pooled means", mx.means, my.means, TOL_PRED)
    check("mirror: pooled variances", mx.variances, my.variances, TOL_PRED)

"""The long-horizon queries on DEEP resident factors, on the device, against long double.

tests/test_predict_long_gpu.py, tests/test_predict_origins_gpu.py and tests/test_components_long_gpu.py
stop at nb0 <= 2 block columns (components: 4, once) and judge normwise.  Here the factors have
3 .. 32 block columns (tests/long_depth_cases.py, whose table says what each case is there for) and
every output is judged componentwise against tests/hp_reference.py / tests/long_reference.py:
mu on sqrt(s_aa), var and sigma on sqrt(s_aa s_bb), logml relative, floors TOL_PRED / TOL_LOGML, the
reference's cond and tol_factor.  tests/test_long_depth_cpu.py holds the fp64 oracle to the same
judgement at a quarter of the tolerance, case by case.

Beside the reference: agreement with ngp_factor_nowcast where the horizon also fits beside the
factor, and of the origin cut = n with the same factor's own long query (rounding: FLOOR_RT on the
same scales); bit contracts at n = 1090.
"""
import numpy as np
import pytest

from nowcastautogp_amd import _lib
from tests import long_depth_cases as ld
from tests import value_cases as vc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    c = _lib.Context(0)
    c.set_combining(False)
    yield c
    _FACTORS.clear()
    c.close()


_FACTORS = {}


def factor(ctx, n, data="lattice"):
    """one resident factor per series, shared by the tests"""
    if (n, data) not in _FACTORS:
        t, y = ld.irregular_series(n) if data == "irregular" else ld.series(n)
        _FACTORS[(n, data)] = ctx.factor(ld.programs(n), t, ld.per_item_rows(y) if data == "per_item" else y)
    return _FACTORS[(n, data)]


def agree(what, got, other, scale, cond, where):
    return ld._judge(what, got, other, scale, vc.FLOOR_RT, ld._Cond(cond), where, 1.0, True)


# ---- 1. predict_long ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ld.LONGS, ids=lambda c: c.id)
def test_predict_long_against_long_double(ctx, case):
    f = factor(ctx, case.n, case.data)
    t, y, t_add, y_add, t_new = case.inputs()
    mu, var, sg, info = f.predict_long(t_new, t_add, y_add, want_sigma=case.sigma)
    assert not info.any() and mu.shape == (ld.P, case.D, case.m) and var.shape == (ld.P, case.m)
    assert (sg is not None) == case.sigma
    if case.sigma:                                       # on the full device array
        np.testing.assert_array_equal(var, np.einsum("pjj->pj", sg))
        for p in range(ld.P):
            assert np.array_equal(sg[p], sg[p].T), (case.id, p)
    for p in range(ld.P):
        r = ld.long_reference(case, p)
        ld.judge_long("predict_long at depth vs long double", mu[p], var[p], sg[p] if case.sigma else None, r,
                      ctx=(case.id, p))
    if case.data == "per_item":
        assert np.max(np.abs(mu[0] - mu[2])) > 1e-3      # the rows differ: so do the means


@pytest.mark.parametrize("case", ld.AGREE, ids=lambda c: c.id)
def test_predict_long_agrees_with_factor_nowcast_where_both_apply(ctx, case):
    """rounding: value_cases.judge_against_run's judgement (FLOOR_RT, condition-aware, the reference's
    scales), on ``ld.agree_programs`` — the particles whose mean the fp64 oracle itself holds to a
    quarter of this tolerance (tests/long_depth_cases.py says why particle 2 is not among them)"""
    t, y, t_add, y_add, t_new = case.inputs()
    f = ctx.factor(ld.agree_programs(case.n), t, y)
    try:
        mu, var, sg, info = f.predict_long(t_new, t_add, y_add, want_sigma=case.sigma)
        ref = f.nowcast(t_add, y_add, t_new)
    finally:
        f.close()
    assert not info.any() and not ref["info"].any()
    for p in range(ld.P):
        ld.judge_agreement("predict_long at depth vs factor_nowcast", mu[p], var[p], sg[p] if case.sigma else None,
                           ref["mu"][p], ref["sigma"][p], ld.agree_reference(case, p), ctx=(case.id, p))


# ---- 2. predict_origins ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ld.ORIGINS, ids=lambda c: c.id)
def test_predict_origins_against_long_double(ctx, case):
    f = factor(ctx, case.n, case.data)
    t, y, cuts, t_new = case.inputs()
    R = len(cuts)
    mu, var, lm, info = f.predict_origins(cuts, t_new)
    assert not info.any() and mu.shape == var.shape == (ld.P, R, case.m) and lm.shape == (ld.P, R)
    own = f.predict_long(t_new, want_sigma=False) if cuts[-1] == case.n else None
    for p in range(ld.P):
        r = ld.origins_reference(case, p)
        ld.judge_origins("predict_origins at depth vs long double", mu[p], var[p], lm[p], r, ctx=(case.id, p))
        if own is not None:
            assert not own[3].any()
            s = np.abs(np.asarray(r.var[-1], float))
            where = (case.id, p)
            agree("predict_origins at depth, cut = n vs predict_long: mu", mu[p, -1], own[0][p, 0], np.sqrt(s),
                  r.cond, where)
            agree("predict_origins at depth, cut = n vs predict_long: var", var[p, -1], own[1][p], s, r.cond, where)
    assert np.all(var > 0)


# ---- 3. components_long ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ld.COMPONENTS, ids=lambda c: f"n{c[0]}")
def test_components_long_against_long_double(ctx, case):
    n, d, D, m = case
    f = factor(ctx, n)
    comps = ld.comps_of(n)
    t, y, t_add, y_add, t_new = ld.query(n, d, D, m)
    out = f.components_long(comps, t_new, t_add, y_add, want_sigma=True)
    assert not out["info"].any()
    for p, prog in enumerate(ld.programs(n)):
        r = ld.components_reference(case, p)
        assert out["mu"][p].shape == (len(comps[p]), D, m)
        ld.judge_components("components_long at depth vs long double", out["mu"][p], out["cross"][p],
                            out["sigma"][p], r, prog, ctx=(case, p))


# ---- 4. bit contracts at depth --------------------------------------------------------------------------
def test_bit_level_contracts_of_the_long_query_at_depth(ctx):
    case = ld.BITS_LONG
    f = factor(ctx, case.n)
    t, y, t_add, y_add, t_new = case.inputs()
    mu, var, sg, info = f.predict_long(t_new, t_add, y_add)
    mu2, var2, sg2, _ = f.predict_long(t_new, t_add, y_add)
    mu0, var0, sg0, info0 = f.predict_long(t_new, t_add, y_add, want_sigma=False)
    assert not info.any() and not info0.any() and sg0 is None
    for a, b in ((mu, mu2), (var, var2), (sg, sg2)):                      # call to call
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(mu0, mu)                                # sigma = NULL: the same bits
    np.testing.assert_array_equal(var0, var)
    np.testing.assert_array_equal(var, np.einsum("pjj->pj", sg))
    np.testing.assert_array_equal(sg, sg.transpose(0, 2, 1))


def test_bit_level_contracts_of_the_origins_at_depth(ctx):
    case = ld.BITS_ORIGINS
    f = factor(ctx, case.n)
    t, y, cuts, t_new = case.inputs()
    mu, var, lm, info = f.predict_origins(cuts, t_new)
    mu2, var2, lm2, _ = f.predict_origins(cuts, t_new)
    assert not info.any()
    for a, b in ((mu, mu2), (var, var2), (lm, lm2)):                      # call to call
        np.testing.assert_array_equal(a, b)
    # an origin's bits do not depend on which other cuts share the call: every third cut, which
    # breaks the run of five, and the cuts behind the main block alone
    n0 = ld.n0_of(case.n)
    for idx in (list(range(0, len(cuts), 3)), [k for k, c in enumerate(cuts) if c > n0],
                [k for k, c in enumerate(cuts) if c in (1024, n0)]):
        assert idx
        mu1, var1, lm1, _ = f.predict_origins([cuts[k] for k in idx], t_new)
        np.testing.assert_array_equal(mu1, mu[:, idx])
        np.testing.assert_array_equal(var1, var[:, idx])
        np.testing.assert_array_equal(lm1, lm[:, idx])
    main = [k for k, c in enumerate(cuts) if c <= n0]                     # more data never widens a forecast
    for a, b in zip(main, main[1:]):
        assert np.all(var[:, b] <= var[:, a]), (cuts[a], cuts[b])

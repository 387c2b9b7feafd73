"""Admissibility of the date layouts (tests/date_cases.py), on the CPU.

1. For every (layout, sampled item, forecast-date set) that tests/test_date_layouts_gpu.py judges, the
   plain fp64 oracle with direct evaluation (oracle/oracle_np.py) is judged by the same call against
   tests/hp_reference.py and must pass at A QUARTER of the tolerance; no case is judged above the floor
   (50 eps cond <= 1e-8) and none is skipped.  Noise is chosen as value_cases does.

2. The parameter map keeps its promise: the extended-precision reference of every layout that
   re-expresses ``unit`` gives the logml, mu and sigma of ``unit``.  The reference is the yardstick
   here, never the library.

   The bound.  ``days_over_last`` cannot supply it: 7 k / (7 (N - 1)) is the correctly rounded
   quotient of the same rational as k / (N - 1), the same bits, and the reference's deviation from
   ``unit`` is 0 (measured: logml, mu and sigma all exactly equal).  What separates the other layouts
   from ``unit`` is not the reference's arithmetic (eps_ld = 1e-19) but the fp64 REPRESENTATION of
   what it is given: each date and mapped parameter is rounded to eps of its own magnitude, and the
   reference takes the rounded numbers as exact.  So the yardstick is the reference's own response to
   representation noise of that size, measured on ``unit``: every date and parameter moved by -1, 0
   or +1 ulp (two seeded draws), worst deviation over the sampled items and date sets,
        n = 321:  logml 7.1e-13 (relative), mu 1.7e-13 (of sqrt s_aa), sigma 8.9e-14 (of sqrt s_aa s_bb)
        n = 130:  logml 3.6e-14,            mu 8.0e-14,                sigma 5.2e-14
   with a margin of x 4, times the layout's noise relative to ``unit``'s: the date differences a
   kernel tree sees carry eps max|t| where ``unit`` carries eps span, a factor max|t| / span (1 for
   ``raw_days``, whose dates are exact and whose parameters are rounded as ``unit``'s dates are; 160
   for ``decimal_years``; 1e4 for ``shift1e4``).  Measured against that bound the layouts use at most
   0.17 of it.
"""
import numpy as np
import pytest

from oracle import oracle_np
from tests import date_cases as dc
from tests import hp_reference as hr
from tests import value_cases as vc


@pytest.mark.parametrize("n", dc.NS)
@pytest.mark.parametrize("name", dc.LAYOUTS)
def test_fp64_oracle_passes_every_sampled_triple_at_a_quarter_of_the_tolerance(name, n):
    p = dc.problem(name, n)
    assert len(p.progs) == dc.B and p.t.size == n and p.t_add.size == dc.D_ADD
    assert p.y_add.shape == (dc.D_SCEN, dc.D_ADD)
    tt = np.concatenate([p.t, p.t_add])
    assert np.unique(tt).size == tt.size
    for k, (t_new, non) in p.sets.items():
        assert t_new.size == (dc.M - 1 if name == "sparse_hi" else dc.M)
        inner = t_new[:-1] if name.startswith("sparse") else t_new     # (the sparse sets end in the anchor)
        if k == "between":
            assert not np.isin(inner, tt).any() and inner.min() > tt.min() and inner.max() < tt.max()
        if k == "on_f":
            assert not non and np.isin(inner, tt).all()
        if k == "beyond":
            assert t_new.min() > tt.max()
        if k.startswith("before"):
            assert t_new.max() < tt.min()
    for i in dc.sample(n):
        assert vc.noise_floor(n) <= p.progs[i][2] <= 1e-1
        for k, (t_new, non) in p.sets.items():
            r = dc.reference(name, n, i, k)
            assert r.info == 0 and vc.cond_within_floor(r), (name, n, i, k, r.cond)
            lb, lf, mu, sg, info = oracle_np.nowcast(p.progs[i], p.t, p.y, p.t_add, p.y_add, t_new, non)
            assert info == 0
            vc.judge_against_reference("date cases (fp64 oracle, 1/4 tol)",
                                       dict(logml_base=lb, logml_full=lf, mu=mu, sigma=sg), r,
                                       ctx=(name, n, i, k), frac=0.25)


def test_the_layouts_are_what_they_say():
    for n in dc.NS:
        u = dc.problem("unit", n)
        assert np.array_equal(dc.problem("days_over_last", n).t, u.t)        # the same bits
        raw = dc.problem("raw_days", n)
        assert np.array_equal(raw.t, np.round(raw.t)) and np.all(np.diff(raw.t) == 14.0)
        assert dc.problem("decimal_years", n).t[0] == 2020.0 and dc.problem("shift1e4", n).t[0] == 1e4
        neg = dc.problem("negative", n)
        assert neg.t.max() < 0 and neg.t[0] == -1.0
        de = dc.problem("descending", n)
        assert np.array_equal(de.t, u.t[::-1]) and np.array_equal(de.y_add, u.y_add[:, ::-1])
        pe = dc.problem("permuted", n)
        assert np.array_equal(np.sort(pe.t), u.t) and not np.array_equal(pe.t, u.t)
        order = np.argsort(pe.t)
        assert np.array_equal(pe.y[order], u.y)
        bc = dc.problem("backcast", n)
        assert all(tn.max() < bc.t.min() for tn, _ in bc.sets.values())
        lo, hi = dc.problem("sparse_lo", n), dc.problem("sparse_hi", n)
        assert np.array_equal(lo.t, hi.t) and np.array_equal(lo.y, hi.y)
        for e in dc.NUDGES:
            nu = dc.problem(f"nudged_{e}", n)
            moved = np.flatnonzero(nu.t != u.t)
            assert moved.size == 1 and 0 < moved[0] < n - 1 and nu.t[moved[0]] > u.t[moved[0]]
        j = n // 2 + 3
        assert dc.problem("nudged_8ulp", n).t[j] - u.t[j] == 8 * np.spacing(u.t[j])
    kinds = set()
    for i in dc.sample(321):
        kinds |= {int(o) for o in dc.unit_programs(321)[i][0]}
    assert {2, 3, 5, 6, 7, 8} <= kinds
    assert sorted(len(p[0]) for p in dc.unit_programs(321)[:dc.LINEAR_ITEM]).count(7) >= 3


# ---- 2. the parameter map -------------------------------------------------------------------------------
def _deviation(r, ru, p):
    """(logml relative, mu on sqrt s_aa, sigma on sqrt s_aa s_bb) of a reference against ``unit``'s"""
    d, dd = hr.pred_scales(ru.sigma)
    lm = np.concatenate([[r.logml_base], np.asarray(r.logml_full)])
    lu = np.concatenate([[ru.logml_base], np.asarray(ru.logml_full)])
    o = p.restore(dict(mu=np.asarray(r.mu), sigma=np.asarray(r.sigma)))
    return np.array([float(np.max(np.abs((lm - lu) / lu))), float(np.max(np.abs(o["mu"] - ru.mu) / d[None, :])),
                     float(np.max(np.abs(o["sigma"] - ru.sigma) / dd))])


@pytest.fixture(scope="module", params=dc.NS)
def yardstick(request):
    """the reference's response to 1 ulp of representation noise on ``unit`` (docstring)"""
    n = request.param
    u = dc.problem("unit", n)
    rng = np.random.default_rng(5)

    def jig(x):
        x = np.asarray(x, float)
        return x + rng.integers(-1, 2, x.shape) * np.spacing(x)
    worst = np.zeros(3)
    for i in dc.sample(n):
        for k, (t_new, non) in u.sets.items():
            ru = dc.reference("unit", n, i, k)
            for _ in range(2):
                ops, par, nz = u.progs[i]
                rj = hr.nowcast((ops, jig(par), nz), jig(u.t), u.y, jig(u.t_add), u.y_add, jig(t_new), None,
                                noise_on_new=non)
                worst = np.maximum(worst, _deviation(rj, ru, u))
    print(f"yardstick n = {n}: logml {worst[0]:.2e} mu {worst[1]:.2e} sigma {worst[2]:.2e}")
    return n, worst


def test_every_affine_layout_is_the_same_gp(yardstick):
    n, worst = yardstick
    assert np.all(worst > 0) and np.all(worst < 1e-11)
    used = 0.0
    for name in dc.AFFINE + ("descending", "permuted"):
        p = dc.problem(name, n)
        for k, (t_new, _) in p.sets.items():
            tt = np.concatenate([p.t, p.t_add, t_new])
            ratio = max(1.0, float(np.abs(tt).max() / (tt.max() - tt.min())))
            for i in dc.sample(n):
                dv = _deviation(dc.reference(name, n, i, k), dc.reference("unit", n, i, k), p)
                if name == "days_over_last":
                    assert not dv.any(), (n, k, i, dv)          # the same bits in, the same numbers out
                used = max(used, float(np.max(dv / (4 * worst * ratio))))
                assert np.all(dv <= 4 * worst * ratio), (name, n, k, i, dv, worst, ratio)
    print(f"n = {n}: at most {used:.2f} of the bound used")


def test_a_wrong_parameter_map_is_noticed():
    """the invariance check has teeth: scaling the Periodic lengthscale as well (it is dimensionless)
    or leaving the Linear amplitude alone moves the reference by many orders more than the bound"""
    n = 130
    u, p = dc.problem("unit", n), dc.problem("raw_days", n)
    t_new, non = p.sets["between"]
    for i, op, pos, factor in ((dc.sample(n)[0], 5, 0, p.a), (dc.LINEAR_ITEM, 2, 2, p.a * p.a)):
        ops, par, nz = p.progs[i]
        par = par.copy()
        at, q = None, 0
        for o in (int(o) for o in ops):
            if o == op and at is None:
                at = q + pos
            q += dc._NPAR[o]
        par[at] *= factor
        r = hr.nowcast((ops, par, nz), p.t, p.y, p.t_add, p.y_add, t_new, None, noise_on_new=non)
        dv = _deviation(r, dc.reference("unit", n, i, "between"), p) if r.info == 0 else np.array([np.inf])
        assert np.max(dv) > 1e-6, (i, dv)

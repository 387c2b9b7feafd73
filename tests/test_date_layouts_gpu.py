"""Lattice detection and the table-driven fills on real date layouts (tests/date_cases.py).

Every kernel that runs on "lattice" dates trusts one host decision, detect_lattice (csrc/ngp_plan.h):
once it accepts a series, a stationary subtree is read from a table at |q_i - q_j| h instead of being
evaluated at t_i - t_j.  The rest of the suite feeds it k / (n - 1) and i / 4096 only; here ONE
problem is written down as day counts, raw day numbers, decimal years, shifted, negative, descending,
permuted, back-cast, sparse and nudged dates, and on every layout
  a. ngp_cov_batch agrees entrywise with hp_reference.cov (nerr < 1e-13, the bound of
     tests/test_gpu_parity.py).  ngp_cov_batch evaluates every entry from the dates (it never asks
     detect_lattice), so this is the statement that direct evaluation is right on every layout;
  b. ngp_nowcast_batch and ngp_factor_create + ngp_factor_nowcast agree with hp_reference.nowcast of
     THAT layout (vc.judge_against_reference: TOL_LOGML, TOL_PRED), with the item alone (FLOOR_RT),
     with structured storage off (same bits, as the header of tests/test_value_routes_gpu.py
     promises), and with the ``unit`` layout (FLOOR_RT on the reference's scales, condition-aware);
  c. the staged gradient job agrees with hr.evaluate (FLOOR_REF) and with the item alone (FLOOR_RT),
     the Toeplitz leaf with the general leaf, and ngp_grad_job_info names the leaf;
  d. the layouts a caller's [0, 1] rescale or whole-day numbers give are still recognised as lattices.
tests/test_date_cases_cpu.py is the admissibility condition: the fp64 oracle passes every sampled
(layout, item, set) at a quarter of the tolerance, none judged above the floor.

Against ``unit``: the layouts are the same GP in exact arithmetic, but the fp64 dates and mapped
parameters a layout passes are rounded (1e4 + k / (N - 1) carries 1e-12 of noise per date), and the
reference takes them as exact: its own answers differ between layouts by up to 5.7e-10 on these
scales (shift1e4, measured; tests/test_date_cases_cpu.py bounds it).  The comparison therefore takes
that known difference out first — (got - ref) of the layout against (got - ref) of ``unit`` — and
then asks FLOOR_RT, no more.

Before detect_lattice judged the fit at the scale of the span (it allowed 16 eps max(|t|, 1) per
point), these tests failed on the device for ``decimal_years``, ``shift100`` and ``shift1e4``: DESIGN.md,
"Lattice dates are judged at the scale of the span".
"""
import numpy as np
import pytest

from nowcastautogp_amd import _lib
from nowcastautogp_amd._abi import KernelArray
from tests import date_cases as dc
from tests import hp_reference as hr
from tests import value_cases as vc
from tests.test_value_routes_gpu import item, launches, same_bits, switches
from tests.util import TOL_LOGML, check, check_components, nerr, tol

pytestmark = pytest.mark.gpu

FLOOR_REF, FLOOR_RT = 1e-10, 1e-11        # gradients, as tests/test_routes_gpu.py
LD = np.longdouble


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    c = _lib.Context(0)
    c.set_combining(False)
    yield c
    c.close()


def sides_of(n):
    """n = 130 fits the one-launch kernel: run it with the short-series path on and off"""
    return [("default", {})] + ([("sweep", {"short": False})] if n <= 256 else [])


# ---- a. covariances ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.LAYOUTS)
def test_cov_batch_on_the_layouts_dates(ctx, name):
    """a 37 x 53 rectangle (training dates against later training, appended and forecast dates) and a
    40 x 40 square with add_diag, all twelve items, entrywise against the long-double reference"""
    p = dc.problem(name, 130)
    late = np.concatenate([p.t[90:], p.t_add] + [tn for tn, _ in p.sets.values()])
    t1, t2, sq = p.t[5:42], late[:53], p.t[60:100]
    assert t1.size == 37 and t2.size == 53 and sq.size == 40
    K, Kd = ctx.cov_batch(p.progs, t1, t2), ctx.cov_batch(p.progs, sq, sq, add_diag=True)
    for b, prog in enumerate(p.progs):
        e1 = nerr(K[b], hr.cov(prog, t1, t2).astype(float))
        e2 = nerr(Kd[b], hr.cov(prog, sq, sq, add_diag=True).astype(float))
        print(f"cov {name} item {b}: {e1:.2e} {e2:.2e}")
        assert e1 < 1e-13 and e2 < 1e-13, (name, b, e1, e2)


# ---- b. the value path ---------------------------------------------------------------------------------
def run(ctx, p, k, only=None, profile=False):
    progs = [p.progs[only]] if only is not None else p.progs
    t_new, non = p.sets[k]
    if profile:
        ctx.profile_enable(True)
        ctx.profile_reset()
    try:
        out = ctx.nowcast_batch(progs, p.t, p.y, p.t_add, p.y_add, t_new, non)
        prof = ctx.profile_get() if profile else None
    finally:
        if profile:
            ctx.profile_enable(False)
    assert not out["info"].any(), (p.name, k, np.flatnonzero(out["info"]))
    out["profile"] = prof
    return out


def minus_reference_shift(got, r, ru, p):
    """one item's outputs on layout p, in ``unit`` order, less what the reference itself says the two
    fp64 problems differ by (r: of the layout, ru: of ``unit``)"""
    g = p.restore(got)
    rr = p.restore(dict(mu=np.asarray(r.mu), sigma=np.asarray(r.sigma)))
    return dict(logml_base=g["logml_base"] - float(LD(r.logml_base) - LD(ru.logml_base)),
                logml_full=np.asarray(g["logml_full"]) - (np.asarray(r.logml_full, LD) - np.asarray(ru.logml_full, LD)).astype(float),
                mu=np.asarray(g["mu"]) - (rr["mu"] - np.asarray(ru.mu)).astype(float),
                sigma=np.asarray(g["sigma"]) - (rr["sigma"] - np.asarray(ru.sigma)).astype(float))


VS_UNIT = dc.AFFINE + ("descending", "permuted")


@pytest.mark.parametrize("n", dc.NS)
@pytest.mark.parametrize("name", dc.LAYOUTS)
def test_value_path_on_the_layout(ctx, name, n):
    p = dc.problem(name, n)
    u = dc.problem("unit", n)
    for k in p.sets:
        t_new, non = p.sets[k]
        for label, sw in sides_of(n):
            c = (name, n, k, label)
            with switches(ctx, **sw):
                out = run(ctx, p, k)
                alone = {i: run(ctx, p, k, only=i) for i in dc.sample(n)}
                unit = run(ctx, u, k) if name in VS_UNIT else None
            with switches(ctx, **{**sw, "storage": False}):
                same_bits(out, run(ctx, p, k), ctx=c + ("storage",))
            for i in dc.sample(n):
                r = dc.reference(name, n, i, k)
                assert r.info == 0 and vc.cond_within_floor(r)       # (tests/test_date_cases_cpu.py)
                got = item(out, i)
                vc.judge_against_reference(f"date layouts {name}", got, r, ctx=c + (i,))
                vc.judge_against_run(f"date layouts {name}: vs item alone", got, item(alone[i], 0), r,
                                     ctx=c + (i,))
                if unit is not None:
                    ru = dc.reference("unit", n, i, k)
                    vc.judge_against_run(f"date layouts {name}: vs unit", minus_reference_shift(got, r, ru, p),
                                         item(unit, i), ru, ctx=c + (i,))
        # the resident factor: ngp_factor_create + ngp_factor_nowcast
        f = ctx.factor(p.progs, p.t, p.y)
        try:
            lm0, info0 = f.logml()
            assert not info0.any()
            q = f.nowcast(p.t_add, p.y_add, t_new, non)
            assert not q["info"].any()
            for i in dc.sample(n):
                r = dc.reference(name, n, i, k)
                vc.judge_against_reference(f"date layouts {name}: resident factor", item(q, i), r, ctx=(name, n, k, i))
                assert abs(lm0[i] - float(r.logml_base)) <= tol(TOL_LOGML, r.cond) * abs(float(r.logml_base))
        finally:
            f.close()


@pytest.mark.parametrize("n", dc.NS)
def test_sparse_lattice_accepted_and_refused_agree(ctx, n):
    """the table-cost refusal, qmax > 16 (dates of the call) + 4096: the same training data with six
    forecast dates (tables) and with five (direct evaluation), compared on the dates both hold"""
    lo, hi = dc.problem("sparse_lo", n), dc.problem("sparse_hi", n)
    cl, ch = dc.SPARSE_SHARED
    assert np.array_equal(lo.t, hi.t) and np.array_equal(lo.y_add, hi.y_add)
    for k in lo.sets:
        assert np.array_equal(lo.sets[k][0][cl], hi.sets[k][0][ch])
        for label, sw in sides_of(n):
            with switches(ctx, **sw):
                a, b = run(ctx, lo, k, profile=True), run(ctx, hi, k, profile=True)
            # the tables kernel is one more launch of the fill's class
            assert launches(a["profile"], "fill") > launches(b["profile"], "fill"), (a["profile"], b["profile"])
            for i in dc.sample(n):
                r = dc.reference("sparse_hi", n, i, k)
                ga, gb = item(a, i), item(b, i)
                ga = dict(ga, mu=ga["mu"][:, cl], sigma=ga["sigma"][np.ix_(cl, cl)])
                gb = dict(gb, mu=gb["mu"][:, ch], sigma=gb["sigma"][np.ix_(ch, ch)])
                rr = hr.NowcastRef()
                rr.sigma, rr.cond = np.asarray(r.sigma)[np.ix_(ch, ch)], r.cond
                vc.judge_against_run("date layouts sparse: tables vs direct", ga, gb, rr, ctx=(n, k, label, i))


# ---- c. gradients --------------------------------------------------------------------------------------
def grad_run(ctx, progs, t, y):
    ka = KernelArray(progs)
    job = ctx.stage_grad(ka, t, y)
    try:
        lm, g, info = job.run()
        layout = job.info()
    finally:
        job.close()
    assert not info.any(), np.nonzero(info)
    off = np.concatenate([[0], np.cumsum(ka._npar + 1)])
    return lm, [g[off[b]:off[b + 1]] for b in range(len(progs))], layout


def expected_toeplitz(name):
    """items on the Toeplitz leaf when the stationary trees travel alone (None: either way)"""
    if name in dc.GUARDED:
        return len(dc.stationary_items())
    if name in ("permuted", "sparse_lo", "sparse_hi") + dc.NUDGES_REFUSED:
        return 0
    return None


@pytest.mark.parametrize("name", dc.LAYOUTS)
def test_gradients_on_the_layout(ctx, name):
    """n = 321.  The whole ensemble (a mixed batch of twelve: one general chunk, filled from tables
    where the dates are a lattice), then its ten stationary trees alone — a batch of stationary trees
    on a regular series always takes the Toeplitz leaf (grad_batch_route, csrc/ngp_plan.h) — and
    those again with structured storage off: the general leaf."""
    n = 321
    p = dc.problem(name, n)
    lm, g, lay = grad_run(ctx, p.progs, p.t, p.y)
    assert lay["toeplitz_items"] == 0 and lay["general_items"] == dc.B, lay
    stat = dc.stationary_items()
    sprogs = [p.progs[i] for i in stat]
    lm_s, g_s, lay_s = grad_run(ctx, sprogs, p.t, p.y)
    want = expected_toeplitz(name)
    assert want is None or lay_s["toeplitz_items"] == want, (name, lay_s)
    assert lay_s["toeplitz_items"] in (0, len(stat)), lay_s
    ctx.set_structured_storage(False)
    try:
        lm_g, g_g, lay_g = grad_run(ctx, sprogs, p.t, p.y)
    finally:
        ctx.set_structured_storage(True)
    assert lay_g["toeplitz_items"] == 0, lay_g
    for i in dc.sample(n):
        r = hr.evaluate(p.progs[i], p.t, p.y)
        assert r.info == 0
        lm_a, g_a, _ = grad_run(ctx, [p.progs[i]], p.t, p.y)
        runs = [("batch", lm[i], g[i])]
        if i in stat:
            runs += [("stationary batch", lm_s[i], g_s[i]), ("general leaf", lm_g[i], g_g[i])]
        for what, l, gg in runs:
            c = (name, what, i)
            check(f"date layouts {name}: logml vs reference", l, float(r.logml), TOL_LOGML, r.cond, ctx=c)
            check_components(f"date layouts {name}: gradient vs reference", gg, r.grad, r.scale, FLOOR_REF,
                             r.cond, ctx=c, factor=r.tol_factor)
            assert abs(l - lm_a[0]) <= tol(1e-12, r.cond) * abs(lm_a[0]), c
            check_components(f"date layouts {name}: gradient vs item alone", gg, g_a[0], r.scale, FLOOR_RT,
                             r.cond, ctx=c)
        if i in stat:
            check_components(f"date layouts {name}: stationary batch vs general leaf", g_s[i], g_g[i], r.scale,
                             FLOOR_RT, r.cond, ctx=(name, i))


# ---- d. route guards -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", dc.NS)
def test_rescaled_and_whole_day_dates_are_still_lattices(ctx, n):
    """``unit``, ``days_over_last``, ``raw_days`` and ``descending`` keep the table route: a lattice job
    launches the tables kernel before its fill, one more launch of class ``fill`` than the same job
    on refused dates (``nudged_1e-8``: the Euclid loop ends below span / 2^20; ``sparse_hi``: the
    table cost), and so are the nudges of 8 ulp and more; ``nudged_1ulp`` may go either way.  Structured storage on a lattice does not show in the profile (the same launches):
    stores_structured (csrc/ngp_plan.h) decides from the stride detect_lattice returns, and the bits
    are compared with it off in the value test above.  Gradient jobs: ngp_grad_job_info, in
    test_gradients_on_the_layout."""
    def fills(name, sw):
        with switches(ctx, **sw):
            return launches(run(ctx, dc.problem(name, n), "on_f", profile=True)["profile"], "fill")
    for label, sw in sides_of(n):
        refused = fills("nudged_1e-8", sw)
        assert fills("sparse_hi", sw) == refused
        for name in dc.GUARDED + ("permuted", "sparse_lo"):
            assert fills(name, sw) > refused, (name, n, label)
        assert fills("unit", sw) == fills("raw_days", sw) == fills("descending", sw)
        for name in dc.NUDGES_REFUSED:
            assert fills(name, sw) == refused, (name, n, label)

"""The one-launch gradient job on the 16-row grid of tests/small_grad_cases.py, componentwise against
the extended-precision reference: chol_small_kernel with small_inverse_column, then
grad_kinv_small_kernel (csrc/ngp_small_kernels.h), at every nbe = ceil(n / 16) from 1 to 16, with 16
and with 1 real rows in the last block (the pairs n = 16 k | 16 k + 1), at nbe = 16 with 15 | 16, inside
the first block, mid-block, on irregular dates, with per-item observation rows and with the pivots
moved sixteen decades (tests/test_short_series_gpu.py judges this path normwise, at 1e-7).

Every row is a staged gradient job of the 9 items and runs
  one-launch   the default: chol_small once, no chol_diag, no chol_col_grad, no Toeplitz item
  sweep        the short path off, on the general leaf alone: the column sweep, no chol_small
  invariant    ngp_set_batch_invariant
and, in each of these ways, every judged item (the first stationary, Linear and ChangePoint tree) in
a job of its own.  Judged, with the project's numbers only: logml against hp_reference.evaluate at
TOL_LOGML; every gradient component on its scale s_i at FLOOR_REF; one-launch against sweep and
batch against alone at FLOOR_RT on the same scales, logml at tol(1e-12, cond); under invariant the
batch and the item alone have the same bits; info is zero.  The two sides of a pair run in one
test.  The scale rows set the jitter to 1e-5 c (small_grad_cases.scaled_spec), each judged against
its own reference.

The sweep-companion rows (n = 368 .. 433, nbe = 23 .. 28: grad_kinv_small_kernel behind the column
sweep) run the default, invariant and alone, on the Linear and the ChangePoint item.

tests/test_small_grad_cases_cpu.py admits every judged (row, item) with the fp64 oracle at a quarter
of these tolerances, compares the restated plan with the compiled one and shows that seven wrong
versions of a model of these kernels fail this judge.
"""
import contextlib

import numpy as np
import pytest

from nowcastautogp_amd import _lib
from tests import hp_reference as hr
from tests import small_grad_cases as sg
from tests import value_cases as vc
from tests.test_routes_gpu import FLOOR_REF, FLOOR_RT, one_general_chunk
from tests.test_routes_gpu import _run as grad_run
from tests.test_value_routes_gpu import launches, switches
from tests.util import TOL_LOGML, check, check_components, tol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    c = _lib.Context(0)
    c.set_combining(False)
    yield c
    c.close()


@contextlib.contextmanager
def spec_of(ctx, case):
    """the row's spec (the scale rows: the jitter times c), the context's own afterwards"""
    sp = case.spec()
    if sp is None:
        yield
        return
    old, new = ctx.get_spec(), ctx.get_spec()
    new.jitter = sp["jitter"]
    ctx.set_spec(new)
    try:
        yield
    finally:
        ctx.set_spec(old)


# the short path off runs under general_leaf_only (structured storage off): no item takes the
# Toeplitz leaf, the batch is one general chunk on the column sweep
WAYS = (("one-launch", {}), ("sweep", dict(short=False, storage=False)), ("invariant", dict(invariant=True)))
SWEEP_WAYS = (("default", {}), ("invariant", dict(invariant=True)))


def _route(way, p, lay):
    if way == "one-launch":
        assert launches(p, "chol_small") == 1 and "chol_diag" not in p and "chol_col_grad" not in p, p
        assert lay["toeplitz_items"] == 0 and lay["general_items"] == sg.B, lay
    elif way == "sweep":
        assert "chol_small" not in p, p
        one_general_chunk(sg.B, lay)
    elif way == "default":          # (sweep companion: the mixed batch of 9 stays whole on the column sweep)
        assert "chol_small" not in p and p["chol_col_grad"]["launches"] > 0, p
        one_general_chunk(sg.B, lay)
    else:
        assert lay["general_items"] + lay["toeplitz_items"] == sg.B, lay


def _judge_row(ctx, kind, name, case, ways):
    t, y = case.data()
    progs = case.progs()
    sample = case.sample()
    refs = {i: hr.evaluate(progs[i], t, case.y_of(i), case.spec()) for i in sample}
    assert all(r.info == 0 and vc.cond_within_floor(r) and r.tol_factor == 1.0 for r in refs.values())
    res = {}
    with spec_of(ctx, case):
        for way, sw in ways:
            with switches(ctx, **sw):
                lm, g, p, lay = grad_run(ctx, progs, t, y, profile=True)
                _route(way, p, lay)
                alone = {i: grad_run(ctx, [progs[i]], t, case.y_of(i))[:2] for i in sample}
            res[way] = (lm, g, alone)
    for way, (lm, g, alone) in res.items():
        for i in sample:
            r, c = refs[i], (name, way, i)
            check(f"small grad {kind}: logml vs reference", lm[i], float(r.logml), TOL_LOGML, r.cond, ctx=c)
            check_components(f"small grad {kind}: gradient vs reference", g[i], r.grad, r.scale, FLOOR_REF,
                             r.cond, ctx=c, factor=r.tol_factor)
            lm_a, g_a = alone[i]
            check(f"small grad {kind}: alone, logml vs reference", lm_a[0], float(r.logml), TOL_LOGML, r.cond,
                  ctx=c)
            check_components(f"small grad {kind}: alone, gradient vs reference", g_a[0], r.grad, r.scale,
                             FLOOR_REF, r.cond, ctx=c, factor=r.tol_factor)
            assert abs(lm[i] - lm_a[0]) <= tol(1e-12, r.cond) * abs(lm_a[0]), c
            check_components(f"small grad {kind}: gradient vs item alone", g[i], g_a[0], r.scale, FLOOR_RT,
                             r.cond, ctx=c)
            if way == "invariant":
                assert lm_a[0] == lm[i] and np.array_equal(g_a[0], g[i]), c
    if "sweep" in res:
        for i in sample:
            r, c = refs[i], (name, "one-launch vs sweep", i)
            lm_s, g_s, _ = res["sweep"]
            lm_o, g_o, _ = res["one-launch"]
            assert abs(lm_o[i] - lm_s[i]) <= tol(1e-12, r.cond) * abs(lm_s[i]), c
            check_components(f"small grad {kind}: gradient, one-launch vs sweep", g_o[i], g_s[i], r.scale,
                             FLOOR_RT, r.cond, ctx=c)


SINGLE = [n for n in sg.ROWS if not any(n in pr for pr in sg.PAIRS)]


def _kind(name):
    return "irregular" if name.endswith("_irr") else "per-item y" if name.endswith("_rows") else \
        "scale" if "_c" in name else "smallest" if name in ("n1", "n5") else "mid-block"


@pytest.mark.parametrize("lo,hi", sg.PAIRS)
def test_edge_pairs(ctx, lo, hi):
    """n = 16 k | 16 k + 1 (and 255 | 256): the same series with one more point, both sides here"""
    for name in (lo, hi):
        _judge_row(ctx, "ends" if lo == "n255" else "edge pair", name, sg.ROWS[name], WAYS)


@pytest.mark.parametrize("name", SINGLE)
def test_rows(ctx, name):
    _judge_row(ctx, _kind(name), name, sg.ROWS[name], WAYS)


@pytest.mark.parametrize("lo,hi", sg.SWEEP_PAIRS)
def test_sweep_companion_pairs(ctx, lo, hi):
    """grad_kinv_small_kernel behind the column sweep, nbe = 23 .. 28 (kinv_route: KINV_SMALL for a
    chunk of 9 and of 1 at nb0 < 8, asserted from the compiled plan on the CPU)"""
    for name in (lo, hi):
        _judge_row(ctx, "sweep companion", name, sg.SWEEP[name], SWEEP_WAYS)

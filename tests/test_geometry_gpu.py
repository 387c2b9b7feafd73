"""The column sweep on the geometry grid of tests/geometry_cases.py, against the extended-precision
reference: block counts 2 .. 12 (pairing from column 0 and from column 1, the first joined
diag-ahead tile, the four-wave tile, split-k on and off) and series whose last rows fall on either
side of a 16-row edge of a 64 x 64 tile (aux tiles of value jobs with 16 | 17 and 80 | 81 rows, the
padded last row tile of gradient jobs with 16 | 17, 32 | 33, 48 | 49 real rows).

Value rows (ngp_nowcast_batch, 9 items), every forecast-date set of the case, every way below judged
against the ONE reference of (item, dates):
  default      the switches as they come
  sweep        the short path off, where nb0 <= 4 (the one-launch kernel would take the job)
  invariant    ngp_set_batch_invariant (no split-k, chol_diag_kernel): the bits of the item alone
  prefix513    nb0 >= 8: the same 9 items as the prefix of a 513-item batch (split-k off by size;
               a test of its own below)
and in every way: the first stationary, Linear and ChangePoint item against hp_reference.nowcast
(TOL_PRED, TOL_LOGML, condition-aware) and against the item in a call of its own (FLOOR_RT); on
lattice dates structured storage on and off give the same bits; info is zero.

Gradient rows (a staged gradient job, 9 items): logml (TOL_LOGML) and every gradient component on its
scale (FLOOR_REF) against hp_reference.evaluate for one stationary item and one Linear chain, and
against the item alone (FLOOR_RT), four ways: default (the mixed batch stays on the general leaf),
the general leaf alone, batch-invariant, and the stationary items as a batch of their own (the
Toeplitz leaf), which is also compared with the general leaf.

tests/test_geometry_cases_cpu.py admits every judged triple with the fp64 oracles at a quarter of
these tolerances, proves the reach from the compiled csrc/ngp_plan.h and shows that wrong kernels
fail this judge.
"""
import numpy as np
import pytest

from nowcastautogp_amd import _lib
from tests import geometry_cases as gm
from tests import hp_reference as hr
from tests import value_cases as vc
from tests.test_routes_gpu import FLOOR_REF, FLOOR_RT, general_leaf_only, one_general_chunk
from tests.test_routes_gpu import _run as grad_run
from tests.test_value_routes_gpu import KEYS, item, launches, same_bits, switches
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


# ---- value rows ---------------------------------------------------------------------------------------
def run(ctx, case, set_name, progs, profile=False):
    t, y, t_add, y_add, _ = case.data()
    t_new, non = case.date_sets()[set_name]
    if profile:
        ctx.profile_enable(True)
        ctx.profile_reset()
    try:
        out = ctx.nowcast_batch(progs, t, y, t_add, y_add, t_new, non)
        prof = ctx.profile_get() if profile else None
    finally:
        if profile:
            ctx.profile_enable(False)
    assert not out["info"].any(), (set_name, np.flatnonzero(out["info"]))
    out["profile"] = prof
    return out


def value_ways(case):
    """[(label, items, switches)]"""
    nb0 = gm.value_geometry(case)[0]
    progs = case.progs()
    off = {"short": False} if nb0 <= 4 else {}
    ways = [("default", progs, {})]
    if nb0 <= 4:
        ways.append(("sweep", progs, off))
    ways.append(("invariant", progs, {**off, "invariant": True}))
    return ways


def assert_route(label, nb0, p):
    """from the kernel-class profile: fat steps are class chol_col, thin and full steps chol_col_thin"""
    if label == "default" and nb0 <= 4:
        assert launches(p, "chol_small") == 1 and "chol_col" not in p, (label, p)
        return
    assert "chol_small" not in p and launches(p, "gram") >= 1, (label, p)
    if label == "prefix513":
        assert launches(p, "chol_col") > 0 and launches(p, "chol_col_thin") > 0, (label, p)
        return
    fat = (nb0 - gm.col_pair_offset(nb0)) // 2
    assert fat == sum(gm.col_step(nb0, jj)[0] == gm.COL_FAT for jj in range(nb0))
    assert launches(p, "chol_col") == fat and launches(p, "chol_col_thin") == nb0 - fat, (label, p)
    assert launches(p, "chol_diag") == nb0, (label, p)


@pytest.mark.parametrize("name", list(gm.VALUE))
def test_value_rows(ctx, name):
    case = gm.VALUE[name]
    nb0, naux = gm.value_geometry(case)
    row = name.split("_nb")[0]
    sample = gm.value_sample(case)
    progs = case.progs()
    for k in case.date_sets():
        res = {}
        for label, items, sw in value_ways(case):
            with switches(ctx, **sw):
                out = res[label] = run(ctx, case, k, items, profile=True)
            assert out["info"].shape == (len(items),)
            assert_route(label, nb0, out["profile"])
            if case.lattice:
                with switches(ctx, **{**sw, "storage": False}):
                    same_bits(out, run(ctx, case, k, items), ctx=(name, k, label, "storage"))
        for i in sample:
            r = vc.reference(case, i, k)
            assert r.info == 0 and vc.cond_within_floor(r) and r.tol_factor == 1.0
            for label, items, sw in value_ways(case):
                c = (name, k, label, i)
                with switches(ctx, **sw):
                    alone = run(ctx, case, k, [progs[i]])
                got = item(res[label], i)
                vc.judge_against_reference(f"geometry {row}", got, r, ctx=c)
                vc.judge_against_run(f"geometry {row}: vs item alone", got, item(alone, 0), r, ctx=c)
                if label == "invariant":
                    for kk in KEYS:
                        assert np.array_equal(alone[kk][0], res[label][kk][i]), (c, kk)


@pytest.mark.parametrize("name", [n for n, c in gm.VALUE.items() if gm.value_geometry(c)[0] >= 8])
def test_value_rows_as_the_prefix_of_513_items(ctx, name):
    """nb0 >= 8: the same 9 items as the prefix of a 513-item batch — split-k off by size
    (SPLITK_MAX_ITEMS), chol_diag_kernel, the late diag-ahead launch.  Only the 9 are judged: first
    every sampled triple against the reference, then against the item alone.

    The item alone is a chunk of one and runs WITH split-k and the wave form of the diagonal kernel:
    that comparison crosses a change of summation order at tol(FLOOR_RT, cond), which is why
    tests/test_geometry_cases_cpu.py admits every triple for it with two fp64 evaluations in
    different orders."""
    case = gm.VALUE[name]
    nb0, _ = gm.value_geometry(case)
    row = name.split("_nb")[0] + " prefix513"
    progs, big = case.progs(), gm.value_big_batch(case)
    res = {}
    for k in case.date_sets():
        out = res[k] = run(ctx, case, k, big, profile=True)
        assert out["info"].shape == (gm.BIG_B,)
        assert_route("prefix513", nb0, out["profile"])
        if case.lattice:
            with switches(ctx, storage=False):
                same_bits(out, run(ctx, case, k, big), ctx=(name, k, "storage"))
        for i in gm.value_sample(case):
            r = vc.reference(case, i, k)
            assert r.info == 0 and vc.cond_within_floor(r) and r.tol_factor == 1.0
            vc.judge_against_reference(f"geometry {row}", item(out, i), r, ctx=(name, k, i))
    for k in case.date_sets():
        for i in gm.value_sample(case):
            alone = run(ctx, case, k, [progs[i]])
            vc.judge_against_run(f"geometry {row}: vs item alone", item(res[k], i), item(alone, 0),
                                 vc.reference(case, i, k), ctx=(name, k, i))


# ---- gradient rows ------------------------------------------------------------------------------------
def _judge_grad(row, what, lm, g, r, ctx=None):
    check(f"geometry {row}: logml vs reference", lm, float(r.logml), TOL_LOGML, r.cond, ctx=(what, ctx))
    check_components(f"geometry {row}: gradient vs reference", g, r.grad, r.scale, FLOOR_REF, r.cond,
                     ctx=(what, ctx), factor=r.tol_factor)


def _judge_grad_run(row, what, lm, g, lm_o, g_o, r, ctx=None):
    assert abs(lm - lm_o) <= tol(1e-12, r.cond) * abs(lm_o), (what, ctx)
    check_components(f"geometry {row}: gradient {what}", g, g_o, r.scale, FLOOR_RT, r.cond, ctx=ctx)


@pytest.mark.parametrize("name", list(gm.GRAD))
def test_gradient_rows(ctx, name):
    case = gm.GRAD[name]
    row = f"grad r={case.r}"
    t, y = case.data()
    progs = case.progs()
    sample = case.sample()
    stat = case.stationary()
    refs = {i: hr.evaluate(progs[i], t, y) for i in sample}
    assert all(r.info == 0 and vc.cond_within_floor(r) and r.tol_factor == 1.0 for r in refs.values())

    def sweep_profile(p):
        assert "chol_small" not in p and p["chol_col_grad"]["launches"] > 0, p

    res = {}
    # default: a mixed batch of 9 stays whole, on the general leaf
    lm, g, p, lay = grad_run(ctx, progs, t, y, profile=True)
    one_general_chunk(9, lay)
    sweep_profile(p)
    res["default"] = (lm, g, {i: grad_run(ctx, [progs[i]], t, y)[:2] for i in sample})
    with general_leaf_only(ctx):
        lm, g, p, lay = grad_run(ctx, progs, t, y, profile=True)
        one_general_chunk(9, lay)
        sweep_profile(p)
        assert "chol_col" not in p, p
        res["general leaf"] = (lm, g, {i: grad_run(ctx, [progs[i]], t, y)[:2] for i in sample})
    ctx.set_batch_invariant(True)
    try:
        lm, g, p, lay = grad_run(ctx, progs, t, y, profile=True)
        assert lay["general_items"] + lay["toeplitz_items"] == 9, lay
        sweep_profile(p)
        res["invariant"] = (lm, g, {i: grad_run(ctx, [progs[i]], t, y)[:2] for i in sample})
    finally:
        ctx.set_batch_invariant(False)
    for way, (lm, g, alone) in res.items():
        for i in sample:
            c = (name, way, i)
            _judge_grad(row, way, lm[i], g[i], refs[i], ctx=c)
            lm_a, g_a = alone[i]
            _judge_grad_run(row, "vs item alone", lm[i], g[i], lm_a[0], g_a[0], refs[i], ctx=c)
            if way == "invariant":
                assert lm_a[0] == lm[i] and np.array_equal(g_a[0], g[i]), c
    # the stationary items as a batch of their own: the Toeplitz leaf
    lm, g, p, lay = grad_run(ctx, [progs[i] for i in stat], t, y, profile=True)
    assert lay["toeplitz_items"] == len(stat) and lay["general_items"] == 0, lay
    assert "chol_col_grad" not in p and "chol_small" not in p and p["chol_col"]["launches"] > 0, p
    for i in sample:
        if i in stat:
            k = stat.index(i)
            c = (name, "toeplitz leaf", i)
            _judge_grad(row, "toeplitz leaf", lm[k], g[k], refs[i], ctx=c)
            _judge_grad_run(row, "Toeplitz vs general leaf", lm[k], g[k], res["general leaf"][0][i],
                            res["general leaf"][1][i], refs[i], ctx=c)
            lm_a, g_a = grad_run(ctx, [progs[i]], t, y)[:2]
            _judge_grad_run(row, "vs item alone", lm[k], g[k], lm_a[0], g_a[0], refs[i], ctx=c)

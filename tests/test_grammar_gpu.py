"""Every kernel-tree evaluator of the device on the grammar zoo (tests/grammar_cases.py), in both
formula forms, componentwise against the extended-precision reference (tests/hp_reference.py).

The covariance of an item is an RPN tree that separate pieces of device code restate; each row below
reaches some of them with ALL forty trees of the zoo — nested and swapped ChangePoints, general
subtrees on both sides, register stacks up to 6, eight sigmoid and 32 table slots:

  cov *       ngp_cov_batch, 37 x 53 and 40 x 40 + diagonal     cov_kernel / keval, entrywise
  V-direct *  nowcast, n = 130 irregular                        fill_kernel, direct epilogue, chol_small
  V-one       nowcast, n = 130 lattice                          FILL_VALUE_ONE, tables, between_off without
  V-lists     nowcast, n = 321 lattice, storage on = off        fill_single / fill_chain / fill_lattice
  V-factor    resident factor at n = 321, one query             aux-only fill
  V-mixed     NGP_PREC_MIXED, n = 321 lattice and irregular     the kapply_kernel modes
  G-direct *  gradient, n = 130 irregular                       grad_contract_kernel
  G-sized *   gradient, n = 130 lattice, six size prefixes      lists kernels NL = 1, 2, 4, 8, two-pass 16,
                                                                lattice_kernel<false>; FILL_GRAD_SMALL
  G-own       the same under ngp_set_batch_invariant            each item on ITS instantiation; = alone, bitwise
  G-sweep     gradient, n = 321 lattice, storage off            FILL_GRAD_LISTS, the sweep's general leaf
  G-toep      gradient, n = 321 lattice, eligible prefixes      DIAG instantiations of the Toeplitz leaf
Every item runs under (0,0,0) and (1,1,1); rows marked * also under the three single flips.

Tolerances are the project's: TOL_LOGML, TOL_PRED on the pred_scales yardsticks, FLOOR_REF = 1e-10 per
gradient component on its scale s_i, FLOOR_RT = 1e-11 between two GPU runs, and test_mixed_gpu's 1e-6
(normwise) for V-mixed.  The cov row has no project number; its bound is measured on the CPU
(tests/test_grammar_cases_cpu.py): fp64 numpy against long double is at worst 4.41e-15 of max |K_item|
(19.9 eps) over every item and spec, and the device gets 8 times that, 3.53e-14 — its exp / pow /
tanh / sin are a couple of ulp where glibc is under one, and its product order differs.

Which contraction instantiation a prefix ran is not visible in the kernel-class profile; the mock
runtime's launch trace confirms it (tests/test_route_trace.py).  Admissibility (the fp64 oracle passes
every judged triple at a quarter of the tolerance) and adequacy (wrong formulas fail on the zoo) are
tests/test_grammar_cases_cpu.py.  References at n = 321 take seconds each in long double: the
gradient rows there judge grammar_cases.sample321() and the Toeplitz-eligible items.
"""
import contextlib

import numpy as np
import pytest

from nowcastautogp_amd import _lib
from nowcastautogp_amd._abi import NGP_INFO_NOT_REFINED, NGP_PREC_MIXED, KernelArray, default_spec
from tests import grammar_cases as gc
from tests import hp_reference as hr
from tests import value_cases as vc
from tests.util import TOL_LOGML, check, check_components, tol

pytestmark = pytest.mark.gpu

FLOOR_REF = 1e-10
FLOOR_RT = 1e-11
TOL_MIXED = 1e-6        # tests/test_mixed_gpu.py
B = len(gc.ZOO)
KEYS = ("logml_base", "logml_full", "mu", "sigma")


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    c = _lib.Context(0)
    c.set_combining(False)
    yield c
    c.close()


@contextlib.contextmanager
def under(ctx, s, precision=0, storage=True, invariant=False, profile=False):
    """the spec and the switches of one run, restored afterwards"""
    ctx.set_spec(gc.ngp_spec(s, precision))
    ctx.set_structured_storage(storage)
    ctx.set_batch_invariant(invariant)
    if profile:
        ctx.profile_enable(True)
        ctx.profile_reset()
    try:
        yield
    finally:
        ctx.profile_enable(False)
        ctx.set_spec(default_spec())
        ctx.set_structured_storage(True)
        ctx.set_batch_invariant(False)


def tag(s):
    return "".join(str(v) for v in s)


def launches(prof, name):
    return prof.get(name, {}).get("launches", 0)


# ---- cov ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", gc.SPECS, ids=tag)
def test_cov(ctx, s):
    t1, t2, t3 = gc.cov_dates()
    with under(ctx, s):
        rect = ctx.cov_batch(gc.PROGRAMS, t1, t2)
        sq = ctx.cov_batch(gc.PROGRAMS, t3, t3, add_diag=True)
    for i, prog in enumerate(gc.PROGRAMS):
        e = gc.spec_dict(gc.effective_spec(i, s))
        for got, ref in ((rect[i], hr.cov(prog, t1, t2, e)), (sq[i], hr.cov(prog, t3, t3, e, add_diag=True))):
            ref = np.asarray(ref, float)
            check_components(f"grammar cov {tag(s)}", got, ref, np.full(ref.shape, np.max(np.abs(ref))),
                             gc.COV_BOUND, ctx=(gc.NAMES[i], s))


# ---- value rows ------------------------------------------------------------------------------------------
def item(out, i):
    return {k: out[k][i] for k in KEYS}


def judge_values(row, case, s, k, out):
    assert not out["info"].any(), (row, s, k, np.flatnonzero(out["info"]))
    for i in range(B):
        r = gc.value_reference(case, i, k, gc.effective_spec(i, s))
        assert vc.cond_within_floor(r)
        vc.judge_against_reference(f"grammar {row} {tag(s)}", item(out, i), r, ctx=(row, gc.NAMES[i], s, k))


def nowcast(ctx, case, k):
    t, y, t_add, y_add, _ = case.data()
    t_new, non = case.date_sets()[k]
    return ctx.nowcast_batch(gc.PROGRAMS, t, y, t_add, y_add, t_new, non)


@pytest.mark.parametrize("s", gc.SPECS, ids=tag)
def test_v_direct(ctx, s):
    """irregular dates: every entry from the dates themselves (fill_kernel, the direct epilogue), one
    launch (chol_small_kernel)"""
    case = gc.value_case(130, False)
    for k in case.date_sets():
        with under(ctx, s, profile=True):
            out = nowcast(ctx, case, k)
            prof = ctx.profile_get()
        assert launches(prof, "chol_small") == 1, prof
        judge_values("V-direct", case, s, k, out)


@pytest.mark.parametrize("s", gc.BOTH_FORMS, ids=tag)
def test_v_one(ctx, s):
    """lattice dates on the one-launch path: ONE fill launch on the general kernel from tables;
    between_off dates leave no lattice, hence no tables"""
    case = gc.value_case(130, True)
    assert set(case.date_sets()) == set(vc.DATE_SETS)
    for k in case.date_sets():
        with under(ctx, s, profile=True):
            out = nowcast(ctx, case, k)
            prof = ctx.profile_get()
        assert launches(prof, "chol_small") == 1, prof
        judge_values("V-one", case, s, k, out)


@pytest.mark.parametrize("s", gc.BOTH_FORMS, ids=tag)
def test_v_lists(ctx, s):
    """n = 321 (nb0 = 5): the column sweep, main tiles by program shape (single table | chain | other);
    structured storage on and off give the same bits"""
    case = gc.value_case(321, True)
    for k in case.date_sets():
        with under(ctx, s, profile=True):
            out = nowcast(ctx, case, k)
            prof = ctx.profile_get()
        assert "chol_small" not in prof and launches(prof, "chol_diag") > 0, prof
        with under(ctx, s, storage=False):
            off = nowcast(ctx, case, k)
        for key in KEYS + ("info",):
            assert np.array_equal(out[key], off[key]), (key, s, k)
        judge_values("V-lists", case, s, k, out)


@pytest.mark.parametrize("s", gc.BOTH_FORMS, ids=tag)
def test_v_factor(ctx, s):
    """a resident factor, then one query: only the aux rows are filled"""
    case = gc.value_case(321, True)
    t, y, t_add, y_add, _ = case.data()
    t_new, non = case.date_sets()["beyond"]
    with under(ctx, s):
        f = ctx.factor(gc.PROGRAMS, t, y)
        try:
            out = f.nowcast(t_add, y_add, t_new, non)
        finally:
            f.close()
    judge_values("V-factor", case, s, "beyond", out)


@pytest.mark.parametrize("lattice", [True, False], ids=["lattice", "irregular"])
@pytest.mark.parametrize("s", gc.BOTH_FORMS, ids=tag)
def test_v_mixed(ctx, s, lattice):
    """NGP_PREC_MIXED: the refinement re-applies K through kapply_kernel (tables | direct); every item
    refined, and within test_mixed_gpu's tolerance of the reference"""
    case = gc.value_case(321, lattice)
    t, y, t_add, y_add, _ = case.data()
    for k in gc.MIXED_SETS:
        t_new, non = case.date_sets()[k]
        with under(ctx, s, precision=NGP_PREC_MIXED):
            job = ctx.stage_nowcast(gc.PROGRAMS, t, y, t_add, y_add, t_new, non)
            try:
                out = job.run().fetch()
                stats = job.mixed_stats()
            finally:
                job.close()
        assert not (out["info"] == NGP_INFO_NOT_REFINED).any() and not out["info"].any(), out["info"]
        assert (stats["refine_steps"] >= 1).all(), stats
        for i in range(B):
            r = gc.value_reference(case, i, k, gc.effective_spec(i, s))
            c = (gc.NAMES[i], s, k)
            what = f"grammar V-mixed {tag(s)}"
            check(f"{what}: logml", out["logml_full"][i], np.asarray(r.logml_full, float), TOL_MIXED, ctx=c)
            check(f"{what}: mu", out["mu"][i], np.asarray(r.mu, float), TOL_MIXED, ctx=c)
            check(f"{what}: variances", np.diag(out["sigma"][i]), np.diag(np.asarray(r.sigma, float)),
                  TOL_MIXED, ctx=c)


# ---- gradient rows ---------------------------------------------------------------------------------------
def run_grad(ctx, idx, t, y, profile=False):
    """one staged gradient job over the items idx: {item: (logml, gradient)}, profile, layout"""
    ka = KernelArray([gc.PROGRAMS[i] for i in idx])
    job = ctx.stage_grad(ka, t, y)
    try:
        if profile:
            ctx.profile_reset()
        lm, g, info = job.run()
        prof = ctx.profile_get() if profile else None
        layout = job.info()
    finally:
        job.close()
    assert not info.any(), [gc.NAMES[idx[b]] for b in np.flatnonzero(info)]
    off = np.concatenate([[0], np.cumsum(ka._npar + 1)])
    return {i: (lm[b], g[off[b]:off[b + 1]]) for b, i in enumerate(idx)}, prof, layout


def judge_grad(row, s, i, got, r):
    c = (row, gc.NAMES[i], s)
    check(f"grammar {row} {tag(s)}: logml", got[0], float(r.logml), TOL_LOGML, r.cond, ctx=c)
    check_components(f"grammar {row} {tag(s)}: gradient", got[1], r.grad, r.scale, FLOOR_REF, r.cond,
                     ctx=c, factor=r.tol_factor)


def same_to_rounding(row, s, i, a, b, r):
    c = (row, gc.NAMES[i], s)
    assert abs(a[0] - b[0]) <= tol(1e-12, r.cond) * abs(b[0]), c
    check_components(f"grammar {row} {tag(s)}: gradient, run against run", a[1], b[1], r.scale, FLOOR_RT,
                     r.cond, ctx=c)


@pytest.mark.parametrize("s", gc.SPECS, ids=tag)
def test_g_direct(ctx, s):
    """irregular dates: grad_contract_kernel re-evaluates every tree from the dates"""
    t, y = gc.grad_series(130, False)
    with under(ctx, s):
        res, _, _ = run_grad(ctx, list(range(B)), t, y)
    for i in range(B):
        judge_grad("G-direct", s, i, res[i], gc.grad_reference(i, 130, False, gc.effective_spec(i, s)))


@pytest.mark.parametrize("s", gc.BOTH_FORMS, ids=tag)
def test_g_sized_every_tree_on_every_larger_instantiation(ctx, s):
    """the zoo sorted by size, as the six prefixes whose largest tree has <= 1, 3, 7, 15, 31, 63
    operators: without contract_by_size a chunk runs on the kernel sized by its largest tree, so
    every tree runs on its own instantiation and on every larger one.  Each against the reference,
    and the runs of an item against each other."""
    t, y = gc.grad_series(130, True)
    runs = []
    for p in gc.prefixes(gc.BY_SIZE):
        with under(ctx, s, profile=True):
            res, prof, layout = run_grad(ctx, p, t, y, profile=True)
        assert launches(prof, "chol_small") > 0 and layout["toeplitz_items"] == 0, (prof, layout)
        runs.append(res)
    assert len(runs) == 6 and len(runs[-1]) == B
    for i in range(B):
        r = gc.grad_reference(i, 130, True, gc.effective_spec(i, s))
        mine = [res[i] for res in runs if i in res]
        for got in mine:
            judge_grad("G-sized", s, i, got, r)
        for got in mine[:-1]:
            same_to_rounding("G-sized", s, i, got, mine[-1], r)


@pytest.mark.parametrize("s", gc.SINGLE_FLIPS, ids=tag)
def test_g_sized_single_flips_on_the_whole_zoo(ctx, s):
    t, y = gc.grad_series(130, True)
    with under(ctx, s):
        res, _, _ = run_grad(ctx, gc.BY_SIZE, t, y)
    for i in range(B):
        judge_grad("G-sized", s, i, res[i], gc.grad_reference(i, 130, True, gc.effective_spec(i, s)))


@pytest.mark.parametrize("s", gc.BOTH_FORMS, ids=tag)
def test_g_own_each_item_on_the_instantiation_of_its_size(ctx, s):
    """batch-invariant: contract_by_size always, and an item in the batch has the bits of the item
    alone"""
    t, y = gc.grad_series(130, True)
    with under(ctx, s, invariant=True):
        res, _, _ = run_grad(ctx, gc.BY_SIZE, t, y)
        alone = {i: run_grad(ctx, [i], t, y)[0][i] for i in range(B)}
    for i in range(B):
        judge_grad("G-own", s, i, res[i], gc.grad_reference(i, 130, True, gc.effective_spec(i, s)))
        assert res[i][0] == alone[i][0] and np.array_equal(res[i][1], alone[i][1]), (gc.NAMES[i], s)


@pytest.mark.parametrize("s", gc.BOTH_FORMS, ids=tag)
def test_g_sweep_and_g_toep(ctx, s):
    """n = 321 on the column sweep.  Storage off: the whole zoo on the general leaf (FILL_GRAD_LISTS).
    Storage on: the Toeplitz-eligible items as cumulative prefixes by size — all of them on the
    Toeplitz leaf (its DIAG contraction, sized by the largest tree) — and then with the 17-leaf tree
    added, which sends the batch to the general leaf.  An eligible item agrees with itself across the
    prefixes and with the general leaf to rounding; sampled items agree with the reference."""
    t, y = gc.grad_series(321, True)
    with under(ctx, s, storage=False, profile=True):
        gen, prof, layout = run_grad(ctx, gc.BY_SIZE, t, y, profile=True)
    assert layout["general_items"] == B and layout["toeplitz_items"] == 0, layout
    assert "chol_small" not in prof and launches(prof, "chol_col_grad") > 0, prof
    for i in gc.sample321():
        judge_grad("G-sweep", s, i, gen[i], gc.grad_reference(i, 321, True, gc.effective_spec(i, s)))
    runs = []
    for p in gc.prefixes(gc.TOEP):
        with under(ctx, s, profile=True):
            res, prof, layout = run_grad(ctx, p, t, y, profile=True)
        assert layout["toeplitz_items"] == len(p) and layout["general_items"] == 0, layout
        assert "chol_col_grad" not in prof and launches(prof, "chol_col") > 0, prof
        runs.append(res)
    with under(ctx, s):
        mixed, _, layout = run_grad(ctx, gc.TOEP + [gc.STAT17], t, y)
    assert layout["toeplitz_items"] == 0 and layout["general_items"] == len(gc.TOEP) + 1, layout
    for i in gc.TOEP + [gc.STAT17]:
        r = gc.grad_reference(i, 321, True, gc.effective_spec(i, s))
        mine = [res[i] for res in runs if i in res]
        for got in mine + [mixed[i]]:
            judge_grad("G-toep", s, i, got, r)
        for got in mine + [mixed[i]]:
            same_to_rounding("G-toep", s, i, got, gen[i], r)
        for got in mine[:-1]:
            same_to_rounding("G-toep", s, i, got, mine[-1], r)

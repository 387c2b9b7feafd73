"""The 16-row grid of the one-launch gradient job (tests/small_grad_cases.py) on the CPU.

  table          the rows are what their names say: every nbe from 1 to 16, every pair on opposite
                 sides of a 16-edge, all four remainders of the K^-1 k-loop, an inverse column of 16
                 stages, and — with geometry_cases.GRAD and the n = 448 rows of test_routes_gpu.py —
                 every nbe from 17 to 28 behind the column sweep
  plan           nbe, ident, the sweeps and colwave restated in small_grad_cases are what the compiled
                 csrc/ngp_plan.h says (tests/sanitize/plan_columns.cpp, argument "small")
  admissibility  the fp64 oracle (oracle_np.logml_grad) passes the judgement of
                 tests/test_small_grad_gpu.py on every judged (row, item) at A QUARTER of the
                 tolerance; every reference has info 0, tol_factor 1 and a condition number within
                 the floor — the scale rows too (their matrices are c times the row c = 1), so no
                 row is judged condition-aware.  A case that fails is changed by the seed rule, never
                 the tolerance.
  adequacy       tests/small_grad_model.py — the device algebra in numpy — passes the same judgement
                 at a quarter of the tolerance on every row, and each of seven wrong versions of it
                 FAILS the judge on the rows named for it; the extra point of every pair moves the
                 reference gradient by more than ten times the tolerance.
No device code runs here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle_np
from tests import geometry_cases as gm
from tests import hp_reference as hr
from tests import small_grad_cases as sg
from tests import util
from tests import value_cases as vc
from tests.small_grad_model import grad_job_model
from tests.util import TOL_LOGML, check_components, tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
FLOOR_REF = 1e-10        # (tests/test_routes_gpu.py)


def _ref(case, i):
    t, _ = case.data()
    return hr.evaluate(case.progs()[i], t, case.y_of(i), case.spec())


# ---- the table is what its names say ------------------------------------------------------------------
def test_the_table_holds_the_geometries_its_names_give():
    kinds = [gm.kind(p) for p in sg.items()]
    assert len(kinds) == 9 and {len(p[0]) for p in sg.items()} == {1, 3, 5}
    assert [kinds[i] for i in sg.sample()] == ["stationary", "linear", "changepoint"]
    for name, c in sg.ALL.items():
        t, y = c.data()
        assert t.size == c.n and int(name.split("_")[-1 if name.startswith("sweep") else 0].lstrip("n")) == c.n, name
        assert y.shape == ((9, c.n) if c.per_item_y else (c.n,))
        assert len(c.progs()) == 9 and c.lattice == (not name.endswith("_irr"))
        assert (c.n <= 256) == (name in sg.ROWS) and c.n <= hr.HP_MAX_N
    # every nbe, at rho = 16 and (from 2 on) at rho = 1; rho = 15 and rho = 9; the 64-edges
    geo = {(sg.nbe(c.n), sg.rho(c.n)) for c in sg.ROWS.values()}
    assert {(k, 16) for k in range(1, 17)} <= geo and {(k, 1) for k in range(1, 17)} <= geo
    assert (16, 15) in geo and {(1, 9), (6, 9), (10, 9), (14, 9)} <= geo and (1, 5) in geo
    assert {sg.n0(c.n) for c in sg.ROWS.values()} == {64, 128, 192, 256}
    for lo, hi in sg.PAIRS[:-1]:
        a, b = sg.ROWS[lo], sg.ROWS[hi]
        assert b.n == a.n + 1 and sg.rho(a.n) == 16 and sg.rho(b.n) == 1 and sg.nbe(b.n) == sg.nbe(a.n) + 1
        assert (sg.n0(b.n) > sg.n0(a.n)) == (a.n in (64, 128, 192))
    # the two sides of a pair: the same items on the same series, one more point
    for lo, hi in sg.PAIRS + sg.SWEEP_PAIRS:
        a, b = sg.ALL[lo], sg.ALL[hi]
        (ta, ya), (tb, yb) = a.data(), b.data()
        assert b.n == a.n + 1 and np.array_equal(ta, tb[:-1]) and np.array_equal(ya, yb[:-1])
        assert sg.nbe(a.n) == (a.n + 15) // 16 and (a.n % 16 == 0 or (a.n, b.n) == (255, 256))
    # all four remainders of the K^-1 k-loop, with one to four live groups in the last chunk
    rem = {sg.kinv_remainder(sg.nbe(c.n), a) for c in sg.ROWS.values() for a in range(sg.nbe(c.n))}
    assert rem == {0, 16, 32, 48}
    assert {sg.kinv_chunks(sg.nbe(c.n), a) for c in sg.ROWS.values() for a in range(sg.nbe(c.n))} == \
        {(ch, lv) for ch in (1, 2, 3, 4) for lv in (1, 2, 3, 4)}
    assert sg.kinv_chunks(16, 0) == (4, 4) and sg.kinv_chunks(13, 0) == (4, 1) and sg.kinv_chunks(1, 0) == (1, 1)
    # an inverse column of 16 stages' length: only at nbe = 16, column 0
    lens = {name: max(sg.inv_len(sg.nbe(c.n), j) for j in range(sg.nbe(c.n))) for name, c in sg.ROWS.items()}
    assert sorted(n for n, v in lens.items() if v == 16) == ["n241", "n241_irr", "n255", "n256"]
    # behind the column sweep: nbe = 17 .. 28 with the rows of the other files
    reached = {sg.nbe(c.n) for c in sg.SWEEP.values()} | {sg.nbe(c.n) for c in gm.GRAD.values() if c.nb0 < 8} | \
        {sg.nbe(448)}
    assert reached >= set(range(23, 29)) and {sg.nbe(c.n) for c in sg.SWEEP.values()} == set(range(23, 29))
    assert reached == {17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28}
    assert all(gm.kinv_route(gm.GradCase(0, c.n, 0).nb0, 9, False) == gm.KINV_SMALL for c in sg.SWEEP.values())
    # the scale rows: the covariance of the row c is c times the covariance of the row 1
    one = sg.ROWS["n208_c1"]
    t, _ = one.data()
    for name in sg.SCALE_ROWS:
        c = sg.ROWS[name]
        for i in sg.sample():
            K1 = oracle_np.cov(one.progs()[i], t, t, True, one.spec())
            Kc = oracle_np.cov(c.progs()[i], t, t, True, c.spec())
            assert np.abs(Kc / c.c - K1).max() <= 8 * util.EPS * np.abs(K1).max(), (name, i)
        assert np.allclose(c.data()[1], one.data()[1] * np.sqrt(c.c), rtol=1e-15, atol=0)


# ---- the restatement is the plan ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """what the compiled csrc/ngp_plan.h says of a gradient job of n = 1 .. 256 points"""
    if HIPCC is None:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("plan") / "plan_columns")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-w",
                           os.path.join(ROOT, "tests", "sanitize", "plan_columns.cpp"), "-o", exe])
    out = subprocess.run([exe, "small"], capture_output=True, text=True, timeout=120, check=True).stdout
    p = {}
    for ln in out.split("\n"):
        w = ln.split()
        if not w:
            continue
        assert w[0] == "small", ln
        v = [int(x) for x in w[1:]]
        n, nbe = v[0], v[1]
        assert nbe > 0, ln                                   # none is refused
        ident, ns = v[2], v[3]
        p[n] = (nbe, ident, ns, tuple(v[4:4 + ns]), v[4 + ns:])
        assert len(p[n][4]) == nbe
    return p


def test_the_restated_plan_is_the_plan(plan):
    assert sorted(plan) == list(range(1, 257))
    for n, got in plan.items():
        assert sg.small_plan(n) == got, n
    for c in sg.ROWS.values():
        assert plan[c.n][0] == sg.nbe(c.n)
    # a different assignment for each nbe
    assert len({tuple(plan[16 * k][4]) for k in range(1, 17)}) == 16


# ---- admissibility --------------------------------------------------------------------------------------
def _judge(what, lm, g, r, ctx, frac):
    # (check is strict and has no share: the logml bound at a quarter is asserted directly)
    assert abs(lm - float(r.logml)) <= frac * tol(TOL_LOGML, r.cond) * abs(float(r.logml)), (what, ctx)
    check_components(f"small grad: gradient ({what})", g, r.grad, r.scale, FLOOR_REF, r.cond, ctx=ctx,
                     factor=frac * r.tol_factor, record=frac < 1.0)


@pytest.mark.parametrize("name", list(sg.ALL))
def test_fp64_oracle_passes_every_judged_item_at_a_quarter_of_the_tolerance(name):
    case = sg.ALL[name]
    t, _ = case.data()
    for i in case.sample():
        r = _ref(case, i)
        assert r.info == 0 and vc.cond_within_floor(r) and r.tol_factor == 1.0, (name, i, r.cond)
        lm, g, info = oracle_np.logml_grad(case.progs()[i], t, case.y_of(i), case.spec())
        assert info == 0
        _judge("fp64 oracle, 1/4 tol", lm, g, r, (name, i), 0.25)
    if name in sg.SCALE_ROWS:
        # the same condition number on all three (the pivots differ by sixteen decades)
        conds = [_ref(sg.ROWS[k], i).cond for k in sg.SCALE_ROWS for i in case.sample()[:1]]
        assert max(conds) / min(conds) < 1 + 1e-6, conds


# ---- adequacy -------------------------------------------------------------------------------------------
def _model_failures(name, hooks, frac):
    """the judged items of the row on which the model fails the judge"""
    case = sg.ALL[name]
    t, _ = case.data()
    failed = []
    for i in case.sample():
        r = _ref(case, i)
        with np.errstate(all="ignore"):
            try:
                lm, g = grad_job_model(case.progs()[i], t, case.y_of(i), case.spec(), hooks)
            except np.linalg.LinAlgError:
                lm, g = np.nan, np.full(r.grad.size, np.nan)
        try:
            assert np.isfinite(lm)
            _judge("model", lm, g, r, (name, i), frac)
        except AssertionError:
            failed.append(i)
    return failed


@pytest.mark.parametrize("name", list(sg.ALL))
def test_the_model_passes_the_judge_at_a_quarter_of_the_tolerance(name):
    assert not _model_failures(name, None, 0.25), name
    # hooks that say what the kernels do change nothing
    right = dict(inv_stop=lambda ln: ln - 1, ring_stale=lambda ln, P: False, kinv_drop=lambda rem: False,
                 alpha_end=lambda n, nbe: 16 * nbe)
    assert not _model_failures(name, right, 0.25), name


def _rows(pred):
    return sorted(name for name, c in sg.ROWS.items() if pred(c.n))


def _has_remainder_16(n):
    return any(sg.kinv_remainder(sg.nbe(n), a) == 16 for a in range(sg.nbe(n)))


# mutant: (hooks, the rows on which it MUST fail, the rows on which it is right and must pass)
MUTANTS = {
    "(a) an inverse column of 16 stops one stage early":
        (dict(inv_stop=lambda ln: ln - 2 if ln == 16 else ln - 1),
         _rows(lambda n: sg.nbe(n) == 16), _rows(lambda n: sg.nbe(n) < 16)),
    "(b) a product reads the ring slot of product P - 6":
        (dict(ring_stale=lambda ln, P: P == sg.SM_RING),
         _rows(lambda n: sg.nbe(n) >= 5), _rows(lambda n: sg.nbe(n) < 5)),
    "(c) the k-loop drops the last chunk when the remainder is 16":
        (dict(kinv_drop=lambda rem: rem == 16), list(sg.ROWS), []),
    "(d) the clamped re-read is multiplied in":
        (dict(kinv_clamped=True), list(sg.ROWS), []),
    "(e) alpha sums to 16 floor(n / 16)":
        (dict(alpha_end=lambda n, nbe: 16 * (n // 16)),
         _rows(lambda n: sg.rho(n) < 16), _rows(lambda n: sg.rho(n) == 16)),
    "(f) logdet over a padded diagonal that was not reset":
        (dict(logdet_padded=True), _rows(lambda n: sg.rho(n) < 16), _rows(lambda n: sg.rho(n) == 16)),
    "(g) the extra point of a pair is ignored":
        (dict(rho1_as_0=True), _rows(lambda n: sg.rho(n) == 1), _rows(lambda n: sg.rho(n) != 1)),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_a_wrong_kernel_fails_the_judge_on_the_rows_named_for_it(mutant):
    hooks, wrong_on, right_on = MUTANTS[mutant]
    assert wrong_on, mutant
    passed = [name for name in wrong_on if not _model_failures(name, hooks, 1.0)]
    assert not passed, (mutant, "passes the judge on", passed)
    # (the mutant is wrong about THAT geometry alone: on the other rows it is the model)
    for name in right_on[::5]:
        assert not _model_failures(name, hooks, 0.25), (mutant, name)


def test_every_row_meets_a_remainder_of_16():
    """(why mutants (c) and (d) are named for every row: block row a = nbe - 1 has the remainder 16 and
    three dead groups in its only chunk)"""
    assert all(_has_remainder_16(c.n) for c in sg.ROWS.values())


@pytest.mark.parametrize("lo,hi", sg.PAIRS + sg.SWEEP_PAIRS)
def test_the_extra_point_of_every_pair_moves_the_reference_gradient(lo, hi):
    """the reference gradient on n + 1 points differs from the one on n points by more than ten
    times the tolerance on a judged component, for every judged item: a kernel that dropped (or
    invented) the row at the edge fails one of the sides"""
    a, b = sg.ALL[lo], sg.ALL[hi]
    for i in a.sample():
        ra, rb = _ref(a, i), _ref(b, i)
        scale = np.maximum(np.asarray(ra.scale, float), np.asarray(rb.scale, float))
        bound = 10 * tol(FLOOR_REF, max(ra.cond, rb.cond)) * scale
        diff = np.abs(np.asarray(rb.grad - ra.grad, float))
        assert (diff > bound).any(), (lo, hi, i, diff / scale)
        assert abs(float(rb.logml - ra.logml)) > 10 * tol(TOL_LOGML, rb.cond) * abs(float(rb.logml))

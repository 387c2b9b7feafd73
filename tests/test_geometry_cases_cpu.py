"""The geometry grid (tests/geometry_cases.py) on the CPU: admissibility, reach, adequacy.

  admissibility  for every (case, sampled item, date set) that tests/test_geometry_gpu.py judges
                 against the extended-precision reference, the plain fp64 oracle passes the same
                 judgement at A QUARTER of the tolerance (oracle_np.nowcast for the value rows,
                 oracle_c.logml_grad for the gradient rows); none is skipped and none is judged
                 above the floor.  For the value rows' comparisons of one run with another (the item
                 alone: tol(FLOOR_RT, cond)), two fp64 evaluations in different summation orders —
                 the LAPACK oracle and tests/blocked_model.py — agree at a quarter of THAT tolerance.
                 A case that fails is changed, never the tolerance.
  reach          the schedule restated in geometry_cases (col_pair_offset, col_step,
                 diag_ahead_waves, splitk_eligible, diag_wave, kinv_route) is what the compiled
                 csrc/ngp_plan.h says (tests/sanitize/plan_columns.cpp), and by it the grid holds
                 what it claims: the first joined diag-ahead tile under each pairing offset with
                 and without split-k, a fat step at column 0 (no tile ahead), diag-ahead tiles of
                 one and of four waves, all three K^-1 routes; every pair lies on opposite sides of
                 its 16-row rule.
  adequacy       tests/blocked_model.py, made wrong in the ways a column kernel can be wrong about
                 this geometry, FAILS the judge of the GPU file on the case named for it (and passes
                 it, at a quarter of the tolerance, when right); the reference gradients of the two
                 sides of a gradient pair differ by more than ten times the tolerance, so a kernel
                 that ignored the extra row could not pass both.
No device code runs here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle_c, oracle_np
from tests import geometry_cases as gm
from tests import hp_reference as hr
from tests import value_cases as vc
from tests.blocked_model import nowcast_model
from tests import util
from tests.util import TOL_LOGML, check_components, tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
FLOOR_REF = 1e-10        # (tests/test_routes_gpu.py)


# ---- the tables are what the rows' names say -----------------------------------------------------------
def test_the_tables_hold_the_geometries_their_names_give():
    for name, c in gm.VALUE.items():
        nb0, naux = gm.value_geometry(c)
        assert c.B == 9 and c.n + c.d <= 832 and c.d == 1, name
        assert int(name.split("_nb")[1].split("_")[0]) == nb0, name
        assert naux == (39 if name.startswith("blocks") else int(name[3:5])), (name, naux)
        assert c.lattice == (not name.endswith("_irr"))
        progs = c.progs()
        assert [gm.kind(progs[i]) for i in gm.value_sample(c)] == ["stationary", "linear", "changepoint"]
        assert {len(p[0]) for p in progs} == {1, 3, 5}
        big = gm.value_big_batch(c)
        assert len(big) == gm.BIG_B and all(a is b for a, b in zip(big, progs))
    assert sorted(gm.value_geometry(c)[0] for n, c in gm.VALUE.items() if n.startswith("blocks")) == \
        [6, 6, 7, 8, 9, 9, 10, 11, 11, 12]
    assert len(gm.VALUE) == 22 and len(gm.GRAD) == 16
    for name, c in gm.GRAD.items():
        assert name == f"grad_n{c.n}" and c.n <= 831 and c.nb0 == c.k + 1
        progs = c.progs()
        assert len(progs) == 9 and {len(p[0]) for p in progs} == {1, 3, 5}
        assert [gm.kind(progs[i]) for i in c.sample()] == ["stationary", "linear"]
        assert "changepoint" not in {gm.kind(p) for p in progs}
        t, _ = c.data()
        assert t.size == c.n and hr.HP_MAX_N >= c.n
    assert sorted({c.nb0 for c in gm.GRAD.values()}) == [5, 6, 9, 10]
    # the two sides of a gradient pair: the same items on the same series, one more point
    for lo, hi in gm.GRAD_PAIRS:
        a, b = gm.GRAD[lo], gm.GRAD[hi]
        (ta, ya), (tb, yb) = a.data(), b.data()
        assert b.n == a.n + 1 and np.array_equal(ta, tb[:-1]) and np.array_equal(ya, yb[:-1])
        assert all(p is q for p, q in zip(a.progs(), b.progs()))


# ---- admissibility ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gm.VALUE))
def test_fp64_oracle_passes_every_value_triple_at_a_quarter_of_the_tolerance(name):
    case = gm.VALUE[name]
    progs = case.progs()
    t, y, t_add, y_add, _ = case.data()
    sets = case.date_sets()
    assert set(sets) == set(vc.DATE_SETS) - (set() if case.lattice else {"between_off"})
    for i in gm.value_sample(case):
        assert vc.noise_floor(case.n) <= progs[i][2] <= 1e-1
        for k, (t_new, non) in sets.items():
            r = vc.reference(case, i, k)
            assert r.info == 0 and vc.cond_within_floor(r) and r.tol_factor == 1.0, (name, i, k, r.cond)
            lb, lf, mu, sg, info = oracle_np.nowcast(progs[i], t, y, t_add, y_add, t_new, non)
            assert info == 0
            vc.judge_against_reference("geometry cases (fp64 oracle, 1/4 tol)",
                                       dict(logml_base=lb, logml_full=lf, mu=mu, sigma=sg), r,
                                       ctx=(name, i, k), frac=0.25)
            # ... and for the comparisons of one device run with another (the item alone, across a
            # change of summation order): two fp64 evaluations in different orders agree within a
            # quarter of tol(FLOOR_RT, cond)
            mb, mf, mm, ms = nowcast_model(progs[i], t, y, t_add, y_add, t_new, non)
            vc.judge_against_run("geometry cases (fp64 oracle vs blocked model, 1/4 tol)",
                                 dict(logml_base=mb, logml_full=mf, mu=mm, sigma=ms),
                                 dict(logml_base=lb, logml_full=lf, mu=mu, sigma=sg), r,
                                 ctx=(name, i, k), frac=0.25)


@pytest.mark.parametrize("name", list(gm.GRAD))
def test_fp64_oracle_passes_every_gradient_item_at_a_quarter_of_the_tolerance(name):
    case = gm.GRAD[name]
    t, y = case.data()
    progs = case.progs()
    for i in case.sample():
        r = hr.evaluate(progs[i], t, y)
        assert r.info == 0 and vc.cond_within_floor(r) and r.tol_factor == 1.0, (name, i, r.cond)
        lm, g, info = oracle_c.logml_grad(progs[i], t, y)
        assert info == 0
        assert abs(lm - float(r.logml)) <= 0.25 * tol(TOL_LOGML, r.cond) * abs(float(r.logml)), (name, i)
        check_components("geometry gradient (fp64 oracle, 1/4 tol)", g, r.grad, r.scale, FLOOR_REF,
                         r.cond, ctx=(name, i), factor=0.25)


# ---- reach --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """what the compiled csrc/ngp_plan.h says (tests/sanitize/plan_columns.cpp)"""
    if HIPCC is None:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("plan") / "plan_columns")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-w",
                           os.path.join(ROOT, "tests", "sanitize", "plan_columns.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, check=True).stdout
    p = dict(offset={}, step={}, waves={}, route={})
    for ln in out.split("\n"):
        w = ln.split()
        if not w:
            continue
        v = [int(x) for x in w[1:]]
        if w[0] == "constants":
            p["constants"] = v
        elif w[0] == "offset":
            p["offset"][v[0]] = v[1]
        elif w[0] == "step":
            p["step"][v[0], v[1]] = (v[2], v[3], v[4], bool(v[5]), bool(v[6]))
        elif w[0] == "waves":
            p["waves"][v[0]] = v[1]
        else:
            assert w[0] == "route", ln
            p["route"][v[0], bool(v[1])] = (bool(v[2]), bool(v[3]), v[4])
    return p


def test_the_restated_schedule_is_the_schedule(plan):
    assert plan["constants"] == [gm.NB, gm.COL_FULL, gm.COL_FAT, gm.COL_THIN, gm.DIAG_AHEAD_SPLIT_K, gm.B]
    assert sorted(plan["offset"]) == list(range(1, 13))
    assert len(plan["step"]) == sum(range(1, 13)) and len(plan["route"]) == 24
    for nb0, o in plan["offset"].items():
        assert gm.col_pair_offset(nb0) == o, nb0
        for jj in range(nb0):
            assert gm.col_step(nb0, jj) == plan["step"][nb0, jj], (nb0, jj)
    for jj, w in plan["waves"].items():
        assert gm.diag_ahead_waves(jj) == w, jj
    for (nb0, inv), (sk, dw, kr) in plan["route"].items():
        assert gm.splitk_eligible(nb0, gm.B, inv) == sk, (nb0, inv)
        assert gm.diag_wave(gm.B, inv) == dw, (nb0, inv)
        assert gm.kinv_route(nb0, gm.B, inv) == kr, (nb0, inv)
    # every column is accumulated exactly once over [0, 64 jj): a thin step adds what its fat step
    # left ([64 (jj - 1), 64 jj)), and a tile that is joined was forked two columns earlier
    for nb0 in plan["offset"]:
        for jj in range(nb0):
            mode, k0_col, k0_diag, ahead, join = plan["step"][nb0, jj]
            assert k0_col == (64 * (jj - 1) if mode == gm.COL_THIN else 0)
            assert join == (jj >= 2 and plan["step"][nb0, jj - 2][3]), (nb0, jj)
            assert k0_diag == (64 * (jj - 1) if mode == gm.COL_THIN else 64 * (jj - 2) if join else 0), (nb0, jj)


def _value_runs():
    """(nb0, items of the chunk, invariant) of every way tests/test_geometry_gpu.py runs a value row"""
    runs = set()
    for c in gm.VALUE.values():
        nb0 = gm.value_geometry(c)[0]
        runs |= {(nb0, gm.B, False), (nb0, gm.B, True)}
        if nb0 >= 8:
            runs.add((nb0, gm.BIG_B, False))
    return runs


def test_the_grid_reaches_what_it_claims(plan):
    """by the COMPILED schedule"""
    runs = _value_runs()
    counts = {nb0 for nb0, _, _ in runs}
    assert counts == {2, 3, 6, 7, 8, 9, 10, 11, 12}
    # the first joined tile under each offset — without split-k, with it, and past the switch with
    # split-k off by the batch size and by ngp_set_batch_invariant
    first_join = {}
    for o in (0, 1):
        jj = min(j for (nb0, j), st in plan["step"].items() if plan["offset"][nb0] == o and st[4])
        assert jj == (4 if o == 0 else 3)
        first_join[o] = jj
        have = {(gm.splitk_eligible(nb0, bc, inv), bc > 512, inv) for nb0, bc, inv in runs
                if plan["offset"][nb0] == o and plan["step"].get((nb0, jj), (0,) * 5)[4]}
        assert {(False, False, False), (True, False, False), (False, True, False),
                (False, False, True)} <= have, (o, have)
        assert all(plan["route"][nb0, inv][0] == sk for nb0, bc, inv in runs if bc == gm.B
                   for sk in [gm.splitk_eligible(nb0, bc, inv)])
    # a fat step that launches nothing ahead because it is column 0, next to fat steps that do
    at0 = [nb0 for nb0 in counts if plan["step"][nb0, 0][0] == gm.COL_FAT and nb0 > 2]
    assert at0 and all(not plan["step"][nb0, 0][3] and plan["step"][nb0, 2][3] for nb0 in at0)
    # the odd counts send column 0 alone (FULL: only the solve) and the last column is thin
    for nb0 in counts:
        modes = [plan["step"][nb0, jj][0] for jj in range(nb0)]
        if nb0 >= 3 and nb0 % 2:
            assert modes[0] == gm.COL_FULL and modes[1] == gm.COL_FAT and modes[-1] == gm.COL_THIN
        else:
            assert modes[0] == gm.COL_FAT and modes[-1] == gm.COL_THIN
    # diag-ahead tiles of one and of four waves
    waves = {plan["waves"][jj] for nb0 in counts for jj in range(nb0) if plan["step"][nb0, jj][3]}
    assert waves == {1, 4}
    # both diagonal forms, and all three K^-1 routes on the gradient rows
    assert {plan["route"][nb0, inv][1] for nb0, bc, inv in runs if bc == gm.B} == {True, False}
    gcounts = {c.nb0 for c in gm.GRAD.values()}
    kinv = {(nb0, inv): plan["route"][nb0, inv][2] for nb0 in gcounts for inv in (False, True)}
    assert set(kinv.values()) == {gm.KINV_SMALL, gm.KINV_WAVE, gm.KINV_LDS}
    assert all(kinv[nb0, False] == (gm.KINV_SMALL if nb0 < 8 else gm.KINV_LDS) for nb0 in gcounts)
    assert all(kinv[nb0, True] == (gm.KINV_WAVE if nb0 < 8 else gm.KINV_LDS) for nb0 in gcounts)
    # the gradient rows are off the one-launch path, under both offsets, and every one has a join
    assert min(gcounts) > gm.SM_MAX_NB and {plan["offset"][nb0] for nb0 in gcounts} == {0, 1}
    assert all(plan["step"][nb0, first_join[plan["offset"][nb0]]][4] for nb0 in gcounts)


def test_every_pair_lies_on_opposite_sides_of_its_16_row_rule():
    for lo, hi, tile in gm.AUX_PAIRS:
        a, b = gm.value_geometry(gm.VALUE[lo]), gm.value_geometry(gm.VALUE[hi])
        assert a[0] == b[0] and b[1] == a[1] + 1 == 64 * tile + 17
        assert gm.aux_tile_groups(a[1], tile) == 1 and gm.aux_tile_groups(b[1], tile) == 4
        assert all(gm.aux_tile_groups(g[1], u) == 4 for g in (a, b) for u in range(tile))
        assert (a[1] + 63) // 64 == (b[1] + 63) // 64 == tile + 1
    for c in gm.VALUE.values():            # the block-count rows: three real 16-row groups
        if gm.value_geometry(c)[1] == 39:
            assert gm.aux_tile_groups(39, 0) == 4 and (39 + 15) // 16 == 3
    for lo, hi in gm.GRAD_PAIRS:
        a, b = gm.GRAD[lo], gm.GRAD[hi]
        assert a.nb0 == b.nb0 and a.r % 16 == 0 and b.r == a.r + 1
        # K^-1's k-loop ends one 16-chunk later on the other side
        assert gm.kinv_kend(a.n) == 64 * a.k + a.r and gm.kinv_kend(b.n) == gm.kinv_kend(a.n) + 16
        if a.r == 16:
            assert gm.last_row_tile_groups(a.n) == 1 and gm.last_row_tile_groups(b.n) == 4
        else:
            assert gm.last_row_tile_groups(a.n) == gm.last_row_tile_groups(b.n) == 4
    assert sorted({(gm.GRAD[lo].k, gm.GRAD[lo].r) for lo, _ in gm.GRAD_PAIRS}) == \
        [(4, 16), (4, 32), (4, 48), (5, 16), (8, 16), (8, 32), (8, 48), (9, 16)]


# ---- adequacy -----------------------------------------------------------------------------------------------
def _thin_starts_late(offset):
    """a thin step that starts its k-range at 64 jj instead of 64 (jj - 1), under one pairing offset"""
    def k_omit(nb0, jj):
        if gm.col_pair_offset(nb0) == offset and gm.col_step(nb0, jj)[0] == gm.COL_THIN:
            return 64 * (jj - 1), 64 * jj
        return None
    return dict(k_omit=k_omit)


MUTANTS = {
    # an aux tile with 17 real rows treated as one of at most 16: rows 16 .. of W left zero
    "17 rows as 16": ("aux17_nb3", dict(aux_groups=lambda naux, tile: 1 if naux - 64 * tile <= 17 else 4)),
    "second aux tile dropped": ("aux81_nb3", dict(aux_groups=lambda naux, tile: 0 if tile == 1 else 4)),
    "thin step one block late, pairs from column 1": ("blocks_nb7", _thin_starts_late(1)),
    "thin step one block late, pairs from column 0": ("blocks_nb6", _thin_starts_late(0)),
}


def _model_judged(name, hooks, frac):
    """the blocked model on every sampled triple of the case, judged as the GPU file judges the
    device: the triples that FAIL"""
    case = gm.VALUE[name]
    t, y, t_add, y_add, _ = case.data()
    failed, total, recorded = [], 0, len(util.RECORDS)
    for i in gm.value_sample(case):
        for k, (t_new, non) in case.date_sets().items():
            r = vc.reference(case, i, k)
            with np.errstate(all="ignore"):
                try:
                    lb, lf, mu, sg = nowcast_model(case.progs()[i], t, y, t_add, y_add, t_new, non, hooks=hooks)
                except np.linalg.LinAlgError:          # (a wrong model may lose definiteness)
                    lb, lf, mu, sg = np.nan, np.full(case.D, np.nan), np.full((case.D, case.m), np.nan), \
                        np.full((case.m, case.m), np.nan)
            total += 1
            try:
                vc.judge_against_reference(f"geometry adequacy {name}", dict(logml_base=lb, logml_full=lf,
                                           mu=mu, sigma=sg), r, ctx=(name, i, k), frac=frac)
            except AssertionError:
                failed.append((i, k))
    if frac == 1.0:                 # judgements that are meant to fail stay out of the parity record
        del util.RECORDS[recorded:]
    return failed, total


@pytest.mark.parametrize("name", sorted({n for n, _ in MUTANTS.values()}))
def test_the_blocked_model_passes_the_judge_at_a_quarter_of_the_tolerance(name):
    failed, total = _model_judged(name, None, 0.25)
    assert not failed and total == 3 * 5, (name, failed)
    # hooks that say what the kernels do change nothing
    right = dict(aux_groups=lambda naux, tile: min(4, (naux - 64 * tile + 15) // 16), k_omit=lambda nb0, jj: None)
    failed, _ = _model_judged(name, right, 0.25)
    assert not failed, (name, failed)


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_a_wrong_kernel_fails_the_judge(mutant):
    name, hooks = MUTANTS[mutant]
    failed, total = _model_judged(name, hooks, 1.0)
    assert failed, (mutant, name)
    # (the mutant is wrong about THIS geometry: its neighbour on the other side of the rule passes)
    other = {"aux17_nb3": "aux16_nb3", "aux81_nb3": "aux16_nb3", "blocks_nb7": "blocks_nb6",
             "blocks_nb6": "blocks_nb7"}[name]
    assert not _model_judged(other, hooks, 0.25)[0], (mutant, other)


@pytest.mark.parametrize("lo,hi", gm.GRAD_PAIRS)
def test_the_extra_point_of_a_gradient_pair_moves_the_gradient(lo, hi):
    """no device model of the gradient path: instead, the reference gradient on n + 1 points differs
    from the one on n points by more than ten times the tolerance on a judged component, for every
    sampled item — a kernel that dropped (or invented) the row at the edge fails one of the sides"""
    a, b = gm.GRAD[lo], gm.GRAD[hi]
    for i in a.sample():
        ra, rb = hr.evaluate(a.progs()[i], *a.data()), hr.evaluate(b.progs()[i], *b.data())
        scale = np.maximum(np.asarray(ra.scale, float), np.asarray(rb.scale, float))
        bound = 10 * tol(FLOOR_REF, max(ra.cond, rb.cond)) * scale
        diff = np.abs(np.asarray(rb.grad - ra.grad, float))
        assert (diff > bound).any(), (lo, hi, i, diff / scale)
        assert abs(float(rb.logml - ra.logml)) > 10 * tol(TOL_LOGML, rb.cond) * abs(float(rb.logml))

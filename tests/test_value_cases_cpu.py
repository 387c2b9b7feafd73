"""Admissibility of the value-path case table (tests/value_cases.py), on the CPU.

For every (case, sampled item, forecast-date set) that tests/test_value_routes_gpu.py judges against
the extended-precision reference, the plain fp64 oracle (oracle/oracle_np.py: LAPACK potrf, one
refactorisation per scenario) is judged by the same call — mu on sqrt(s_aa), sigma on
sqrt(s_aa s_bb), logml relative — and must pass at A QUARTER of the tolerance: the margin a correct
fp64 kernel with another summation order needs.  No case is skipped and none is judged above the
floor (50 eps cond <= 1e-8): a case that fails here is changed (more noise, another date), never
the tolerance."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle_np
from tests import value_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


@pytest.mark.parametrize("name", list(vc.CASES))
def test_fp64_oracle_passes_every_sampled_case_at_a_quarter_of_the_tolerance(name):
    case = vc.CASES[name]
    progs = case.progs()
    t, y, t_add, y_add, _ = case.data()
    assert len(progs) == case.B and max(case.batch_sizes()) == case.B
    sets = case.date_sets()
    assert set(sets) == set(vc.DATE_SETS) - (set() if case.lattice else {"between_off"})
    # the sets are what they say: strictly inside a gap of the training dates / on a training date
    tt = np.concatenate([t, t_add])
    assert np.all(np.diff(tt) > 0)
    for k in ("between", "between_off"):
        if k in sets:
            pos = np.searchsorted(tt, sets[k][0])
            assert np.all((pos > 0) & (pos < tt.size)) and not np.isin(sets[k][0], tt).any()
    assert np.isin(sets["on"][0], tt).all() and np.array_equal(sets["on"][0], sets["on_f"][0])
    assert sets["beyond"][0].min() > tt[-1] and not sets["on_f"][1] and sets["on"][1]
    var = []
    for i in case.sample():
        nz = progs[i][2]
        assert vc.noise_floor(case.n) <= nz <= 1e-1
        for k, (t_new, non) in sets.items():
            r = vc.reference(case, i, k)
            assert r.info == 0 and vc.cond_within_floor(r), (name, i, k, r.cond)
            lb, lf, mu, sg, info = oracle_np.nowcast(progs[i], t, y, t_add, y_add, t_new, non)
            assert info == 0
            vc.judge_against_reference("value cases (fp64 oracle, 1/4 tol)",
                                       dict(logml_base=lb, logml_full=lf, mu=mu, sigma=sg), r,
                                       ctx=(name, i, k), frac=0.25)
        var += [np.diag(np.asarray(vc.reference(case, i, k).sigma, float)) for k in sets]
        # the same item with its own observation row, where a GPU row runs it so
        per_item = vc.PER_ITEM_Y.get(name)
        for k in sets if per_item else ():
            prog, t_, y_, ta_, ya_, t_new, non = vc.inputs(case, i, k, per_item)
            r = vc.reference(case, i, k, per_item)
            assert r.info == 0 and vc.cond_within_floor(r), (name, i, k, r.cond)
            lb, lf, mu, sg, info = oracle_np.nowcast(prog, t_, y_, ta_, ya_, t_new, non)
            assert info == 0
            vc.judge_against_reference("value cases, per-item y (fp64 oracle, 1/4 tol)",
                                       dict(logml_base=lb, logml_full=lf, mu=mu, sigma=sg), r,
                                       ctx=(name, i, k), frac=0.25)
    # the smallest predictive variance judged in the case is well below the largest
    var = np.concatenate(var)
    assert var.min() > 0 and var.max() >= 10 * var.min(), (name, var.min(), var.max())


def test_the_table_reaches_every_noise_level_tree_kind_and_sweep_count():
    nz, kinds = [], set()
    for case in vc.CASES.values():
        progs = case.progs()
        for i in case.sample():
            nz.append(progs[i][2])
            kinds |= {int(o) for o in progs[i][0]}
    assert min(nz) <= 1e-3 and max(nz) >= 1e-1
    assert kinds == {1, 2, 3, 4, 5, 6, 7, 8}
    # the fill-kernel row holds three items of each kind, by compile_program's rule
    fill = [vc.fill_kind(p) for p in vc.CASES["fill3"].progs()]
    assert fill == list(vc.FILL_KINDS) * 3, fill
    Y = vc.CASES["scen8"].per_item_y()
    assert Y.shape == (16, 130) and not np.array_equal(Y[0, 128:], Y[1, 128:])     # the tails differ


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
def test_the_restated_planner_is_the_planner(tmp_path):
    """value_cases.small_plan_sweeps against small_plan itself (tests/sanitize/plan_sweeps.cpp
    compiles csrc/ngp_plan.h, through ngp_internal.h, on the host) over every value geometry, and the sweeps rows:
    one, two and three sweeps.  With NGP_MAX_AUX = 192 aux rows (12 row-blocks of 16) and at least
    160 // 16 = 10 row-blocks per further sweep, a value job never needs the fourth sweep and never
    falls back for want of one: the planner itself says so here."""
    exe = str(tmp_path / "plan_sweeps")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-w",
                           os.path.join(ROOT, "tests", "sanitize", "plan_sweeps.cpp"), "-o", exe])
    lines = subprocess.run([exe], capture_output=True, text=True, timeout=120, check=True).stdout.split("\n")
    assert [int(v) for v in lines[0].split()[1:]] == [vc.SM_WAVES, vc.SM_NSLOT, vc.SM_MAX_PANEL,
                                                      vc.SM_MAX_SWEEPS, vc.NGP_MAX_AUX]
    plan = {(int(a), int(b)): int(c) for a, b, c in (ln.split() for ln in lines[1:] if ln)}
    assert len(plan) == 5 * vc.NGP_MAX_AUX
    for (n0, naux), ns in plan.items():
        assert vc.small_plan_sweeps(n0, 0, naux - 1) == ns, (n0, naux, ns)
        assert (1 <= ns <= 3) if n0 <= 256 else ns == 0, (n0, naux, ns)
    got = []
    for k in ("sweeps1", "sweeps2", "sweeps3"):
        c = vc.CASES[k]
        got.append(plan[(c.n // 64 * 64, c.n % 64 + c.d + c.m + 1)])
        assert vc.small_plan_sweeps(c.n, c.d, c.m) == got[-1]
    assert got == [1, 2, 3], got

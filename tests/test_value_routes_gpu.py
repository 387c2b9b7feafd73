"""Route switch points of the VALUE path (ngp_nowcast_batch and what shares its schedule), tested from
both sides, componentwise, against the extended-precision reference.

factor_chunk, stage_general and ngp_job_run (csrc/ngp_api.hip) choose kernels and summation orders
from the batch size, the series length, the aux-row count, the dates and the scenario count.  For
every switch the cases of tests/value_cases.py run on both sides, with forecast dates beyond the
data, between training dates (on and off the lattice) and on observed dates (with and without
noise_on_new), and on each side
  1. sampled items agree with hp_reference.nowcast: mu on sqrt(s_aa), sigma on sqrt(s_aa s_bb)
     (TOL_PRED), logml relative (TOL_LOGML), condition-aware;
  2. sampled items agree with the item in a call of its own (FLOOR_RT on the same scales);
  3. where both sides hold the same data, the two sides agree with each other (FLOOR_RT);
  4. on lattice dates, structured storage on and off give the same bits.  The switch only acts on
     jobs that reach the column sweep with nb0 >= 2 (stores_structured, csrc/ngp_plan.h): the
     4,097-item side, the diagonal-block, split-k, two-lane, aux-tile and fill-kernel rows, nb0 = 5
     and every side run with the short path off at nb0 >= 2; on the one-launch sides and at
     nb0 = 1 the comparison is of two identical jobs (and between_off dates leave no lattice);
  5. with ngp_set_batch_invariant the sides and the item alone give the same bits.
tests/test_value_cases_cpu.py is the admissibility condition of 1: the fp64 oracle passes every
sampled (case, item, date set) at a quarter of the tolerance, none judged above the floor.

The route a side took is asserted from the kernel-class profile where launch classes or counts tell
the routes apart; where they cannot, the row's docstring names the constant that decides.
"""
import contextlib

import numpy as np
import pytest

from nowcastautogp_amd import _lib
from tests import value_cases as vc
from tests.value_cases import CASES

pytestmark = pytest.mark.gpu

KEYS = ("logml_base", "logml_full", "mu", "sigma", "info")


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    c = _lib.Context(0)
    c.set_combining(False)
    yield c
    c.close()


@contextlib.contextmanager
def switches(ctx, short=True, storage=True, invariant=False):
    ctx.set_short_series_path(short)
    ctx.set_structured_storage(storage)
    ctx.set_batch_invariant(invariant)
    try:
        yield
    finally:
        ctx.set_short_series_path(True)
        ctx.set_structured_storage(True)
        ctx.set_batch_invariant(False)


def run(ctx, case, set_name, B=None, only=None, profile=False):
    """ngp_nowcast_batch over the first B items of the case (only: that one item alone)"""
    progs = case.progs()
    progs = [progs[only]] if only is not None else progs[:B or case.B]
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


def item(out, i):
    return {k: out[k][i] for k in KEYS[:4]}


def same_bits(a, b, n=None, ctx=None):
    for k in KEYS:
        assert np.array_equal(a[k][:n], b[k][:n]), (k, ctx)


def launches(prof, name):
    return prof.get(name, {}).get("launches", 0)


def judge(ctx, row, case, sides=None, route=None, storage=None):
    """sides: [(label, B, switches)] (default: the case's batch sizes under the default switches);
    route(label, B, profile) asserts the route of a side.  Returns {set: {label: out}}."""
    sides = sides or [(str(B), B, {}) for B in case.batch_sizes()]
    Bmin = min(B for _, B, _ in sides)
    sample = case.sample(Bmin)
    storage = case.lattice if storage is None else storage
    res = {}
    for k in case.date_sets():
        res[k] = {}
        for label, B, sw in sides:
            with switches(ctx, **sw):
                out = res[k][label] = run(ctx, case, k, B, profile=route is not None)
            if route is not None:
                route(label, B, out["profile"])
            if storage:        # the header promises the same bits
                with switches(ctx, **{**sw, "storage": False}):
                    same_bits(out, run(ctx, case, k, B), ctx=(row, k, label, "storage"))
        for i in sample:
            r = vc.reference(case, i, k)
            assert vc.cond_within_floor(r)          # (admissibility: never judged above the floor)
            for label, B, sw in sides:
                c = (row, k, label, i)
                with switches(ctx, **sw):
                    alone = run(ctx, case, k, only=i)
                got = item(res[k][label], i)
                vc.judge_against_reference(f"value routes {row}", got, r, ctx=c)
                vc.judge_against_run(f"value routes {row}: vs item alone", got, item(alone, 0), r, ctx=c)
            for label, B, sw in sides[1:]:
                vc.judge_against_run(f"value routes {row}: one side vs the other",
                                     item(res[k][label], i), item(res[k][sides[0][0]], i), r,
                                     ctx=(row, k, label, i))
    return res


def invariant_bits(ctx, row, case, sides=None):
    """batch-invariant mode: the same bits on every side (sides that differ in batch size only) and
    for the sampled items in a call of their own"""
    sides = sides or [(str(B), B, {}) for B in case.batch_sizes()]
    Bmin = min(B for _, B, _ in sides)
    for k in case.date_sets():
        outs = []
        for label, B, sw in sides:
            with switches(ctx, **{**sw, "invariant": True}):
                outs.append(run(ctx, case, k, B))
        for o in outs[1:]:
            same_bits(o, outs[0], Bmin, ctx=(row, k))
        with switches(ctx, **{**sides[0][2], "invariant": True}):
            for i in case.sample(Bmin):
                a = run(ctx, case, k, only=i)
                for kk in KEYS:
                    assert np.array_equal(a[kk][0], outs[0][kk][i]), (row, k, i, kk)


# ---- one-launch kernel against the column sweep -----------------------------------------------------
def test_one_launch_main_block_319_vs_320_points(ctx):
    """n = 319 (n0 = 256, nb0 = 4: chol_small_kernel, which leaves G itself — no gram launch) against
    n = 320 (nb0 = 5: column sweep; small_plan refuses nb0 > 4), and the n = 319 items on both routes
    (ngp_set_short_series_path).  The rule is the geometry's alone (header): already invariant."""
    def route(label, B, p):
        if label == "319":
            assert launches(p, "chol_small") == 1 and "gram" not in p and "chol_diag" not in p, p
        else:
            assert "chol_small" not in p and launches(p, "gram") == 1, p
            assert launches(p, "chol_diag") == (5 if label == "320" else 4), p
    c = CASES["short319"]
    judge(ctx, "one-launch n=319 on|off", c, [("319", c.B, {}), ("319-sweep", c.B, {"short": False})], route)
    judge(ctx, "one-launch n=320", CASES["short320"], [("320", 24, {})], route)
    invariant_bits(ctx, "one-launch n=319", c)
    invariant_bits(ctx, "one-launch n=320", CASES["short320"])


@pytest.mark.parametrize("name", ["items4097_lat", "items4097_irr"])
def test_one_launch_4096_vs_4097_items(ctx, name):
    """SM_MAX_ITEMS: 4,096 items of n = 200 in one launch each, 4,097 on the column sweep; on lattice
    dates the larger side also turns structured storage on (stage_general: g.toep unless the job is
    a short one of at most SM_MAX_ITEMS items).  Batch-invariant jobs take the one-launch kernel
    whatever the batch (small_job: Bc <= SM_MAX_ITEMS || g.invariant)."""
    def route(label, B, p):
        if B <= 4096:
            assert launches(p, "chol_small") == 1 and "gram" not in p and "chol_col" not in p, p
        else:
            assert "chol_small" not in p and launches(p, "chol_diag") == 3 and launches(p, "gram") == 1, p
    c = CASES[name]
    judge(ctx, f"one-launch 4096|4097 {name[-3:]}", c, route=route)
    invariant_bits(ctx, name, c)


@pytest.mark.parametrize("name,sweeps", [("sweeps1", 1), ("sweeps2", 2), ("sweeps3", 3)])
def test_one_launch_aux_sweeps(ctx, name, sweeps):
    """aux rows beyond what the main sweep's registers hold go through further sweeps of the same
    launch (small_plan): 1, 2 and 3 sweeps at n0 = 256, counted with the planner's own arithmetic
    (value_cases.small_plan_sweeps).  NGP_MAX_AUX = 192 rows are 12 row-blocks and every further
    sweep takes at least 10, so a fourth sweep and the fall-back for want of one cannot be reached
    by a value job (tests/test_value_cases_cpu.py checks that over every geometry).  The sweep
    count does not show in the profile (one launch, class 13); both routes are run instead."""
    c = CASES[name]
    assert vc.small_plan_sweeps(c.n, c.d, c.m) == sweeps

    def route(label, B, p):
        assert (launches(p, "chol_small") == 1) == (label == "one-launch"), p
    judge(ctx, f"aux sweeps {sweeps}", c, [("one-launch", c.B, {}), ("sweep", c.B, {"short": False})],
          route)
    invariant_bits(ctx, name, c)


# ---- the column sweep ----------------------------------------------------------------------------------
def test_diagonal_blocks_512_vs_513_items(ctx):
    """DIAG_WAVE_MAX_ITEMS / AHEAD_EARLY_MAX_ITEMS (diag_wave / ahead_early, csrc/ngp_plan.h): up to
    512 items in the chunk chol_diag_wave_kernel and the early diag-ahead launch, above them
    chol_diag_kernel and the late one.  Both diagonal kernels are class 1 and the launch counts are
    the same, so the profile cannot tell them apart; it does show one chunk on the sweep."""
    def route(label, B, p):
        assert launches(p, "chol_diag") == 7 and launches(p, "gram") == 1 and "chol_small" not in p, p
    c = CASES["diag513"]
    judge(ctx, "diag blocks 512|513", c, route=route)
    invariant_bits(ctx, "diag513", c)


def test_split_k_fat_steps(ctx):
    """split-k fat steps (splitk_eligible, csrc/ngp_plan.h): chunks of at most 512 items from nb0 = 8 on — nb0 = 7 | 8
    at 40 items, 512 | 513 items at nb0 = 8.  chol_col_glds_kernel<.., SPLITK> shares class 0 with
    the plain fat step: the profile cannot tell.  Batch-invariant jobs never split."""
    for name in ("splitk_nb7", "splitk_nb8"):
        nb0 = CASES[name].n // 64

        def route(label, B, p):
            assert launches(p, "chol_diag") == nb0 and launches(p, "chol_col") == nb0 // 2, p
        judge(ctx, f"split-k {name}", CASES[name], route=route)
        invariant_bits(ctx, name, CASES[name])
    judge(ctx, "split-k 512|513", CASES["splitk513"])
    invariant_bits(ctx, "splitk513", CASES["splitk513"])


def test_two_lanes(ctx):
    """TWO_LANE_MIN_NB / TWO_LANE_MIN_ITEMS (two_lane, csrc/ngp_plan.h): from 24 block columns and 64 items on
    the chunk is swept as two half-chunks side by side — every launch of the sweep twice.  Items 31
    and 32 sit on either side of the half-chunk seam.  n > HP_MAX_N: the reference is fp64
    (tol_factor 2)."""
    def route(label, B, p):
        nb0 = 24 if label in ("63", "64") else 23
        assert launches(p, "chol_diag") == (2 * nb0 if label == "64" else nb0), (label, p)
    c = CASES["lanes_nb24"]
    assert vc.reference(c, 0, "on_f").tol_factor == 2.0
    judge(ctx, "two lanes 63|64", c, route=route)
    invariant_bits(ctx, "lanes_nb24", c)
    c = CASES["lanes_nb23"]
    judge(ctx, "two lanes nb0=23", c, [("nb23", 64, {})], route)
    invariant_bits(ctx, "lanes_nb23", c)


@pytest.mark.parametrize("tail", [1, 63])
@pytest.mark.parametrize("nb0", [1, 2, 3, 4, 5])
def test_column_pairing(ctx, nb0, tail):
    """block columns go in pairs (fat step, class 0, then thin step, class 6); an odd count of three
    or more sends column 0 alone (col_pair_offset / col_step, csrc/ngp_plan.h), a count of one is a single full step.
    Up to nb0 = 4 the one-launch kernel is the other side."""
    c = CASES[f"pairs_nb{nb0}_tail{tail}"]
    fat = (nb0 - (1 if nb0 >= 3 and nb0 % 2 else 0)) // 2

    def route(label, B, p):
        if label == "one-launch":
            assert launches(p, "chol_small") == 1 and "chol_col" not in p, p
        else:
            assert launches(p, "chol_col") == fat and launches(p, "chol_col_thin") == nb0 - fat, p
            assert launches(p, "chol_diag") == nb0 and "chol_small" not in p, p
    sides = [("sweep", c.B, {"short": False})] + ([("one-launch", c.B, {})] if nb0 <= 4 else [])
    judge(ctx, f"pairing nb0={nb0} tail={tail}", c, sides, route)
    invariant_bits(ctx, f"pairs {nb0} {tail}", c, sides[:1])


@pytest.mark.parametrize("name", ["auxtiles64", "auxtiles65", "auxtiles128", "auxtiles129"])
def test_aux_tiles_of_the_sweep_and_the_resident_factor(ctx, name):
    """naux = 64 | 65 | 128 | 129: one, two and three aux tiles at nb0 = 5 (an
    aux tile's zero rows are neither multiplied nor stored); the tile count does not show in the
    profile.  The same queries through ngp_factor_create + ngp_factor_nowcast, whose aux rows are
    solved by chol_col_kernel (class 6) and aux_update_kernel (class 7) against the resident L."""
    c = CASES[name]
    assert 1 + c.d + c.m + 1 == int(name[8:])
    sets = tuple(c.date_sets())
    res = judge(ctx, name, c)
    invariant_bits(ctx, name, c)
    t, y, t_add, y_add, _ = c.data()
    f = ctx.factor(c.progs(), t, y)
    try:
        lm0, info0 = f.logml()
        assert not info0.any()
        for k in sets:
            t_new, non = c.date_sets()[k]
            ctx.profile_enable(True)
            ctx.profile_reset()
            q = f.nowcast(t_add, y_add, t_new, non)
            p = ctx.profile_get()
            ctx.profile_enable(False)
            assert launches(p, "chol_col_thin") > 0 and launches(p, "aux_update") > 0 and "chol_col" not in p, p
            assert not q["info"].any()
            batch = res[k][str(c.B)]
            for i in c.sample():
                r = vc.reference(c, i, k)
                vc.judge_against_reference(f"value routes {name}: resident factor", item(q, i), r, ctx=(k, i))
                vc.judge_against_run(f"value routes {name}: resident factor vs one-shot call", item(q, i),
                                     item(batch, i), r, ctx=(k, i))
                assert abs(lm0[i] - float(r.logml_base)) <= vc.TOL_LOGML * abs(float(r.logml_base))
    finally:
        f.close()


def _d9_first_8(b, i):
    return dict(logml_base=b["logml_base"][i], logml_full=b["logml_full"][i][:8], mu=b["mu"][i][:8],
                sigma=b["sigma"][i])


def test_scenario_solve_8_vs_9_scenarios(ctx):
    """the epilogue solves up to 8 scenarios one after the other with every row's dot product spread
    over the wave, more than 8 with one lane per scenario (launch_epilogue in csrc/ngp_kernels.hip, g.D <= 8): the
    same kernel, so nothing in the profile.  Scenarios 0..7 are the same on both sides.  Here y is
    shared by the items (ngp_nowcast_batch takes one y); the next test gives every item its own."""
    c8, c9 = CASES["scen8"], CASES["scen9"]
    assert np.array_equal(c8.data()[3], c9.data()[3][:8])
    r8, r9 = judge(ctx, "scenarios D=8", c8), judge(ctx, "scenarios D=9", c9)
    for k in r8:
        for i in c8.sample():
            vc.judge_against_run("value routes scenarios: D=9 vs D=8", _d9_first_8(r9[k]["16"], i),
                                 item(r8[k]["16"], i), vc.reference(c8, i, k), ctx=(k, i))
    invariant_bits(ctx, "scen8", c8)
    invariant_bits(ctx, "scen9", c9)


def test_scenario_solve_with_per_item_observation_rows(ctx):
    """D = 8 | 9 with y [B, n]: ngp_factor_create takes per-item rows and ngp_factor_nowcast stages its
    D scenarios with them (g.y_shared = 0), so the epilogue reads item b's block ya + b D da on both
    branches; n = 130 has a tail of two points, which is part of that block and differs per item.
    Every logml_full[s] and mu[s] of the sampled items against the reference of (item, Y[item]), and
    against a resident factor of the item alone."""
    outs = {}
    for name in ("scen8", "scen9"):
        c = CASES[name]
        t, _, t_add, y_add, _ = c.data()
        Y, progs = c.per_item_y(), c.progs()
        f = ctx.factor(progs, t, Y)
        alone = {i: ctx.factor([progs[i]], t, Y[i]) for i in c.sample()}
        try:
            assert not f.logml()[1].any()
            for k, (t_new, non) in c.date_sets().items():
                q = outs[name, k] = f.nowcast(t_add, y_add, t_new, non)
                assert not q["info"].any()
                for i in c.sample():
                    r = vc.reference(c, i, k, "factor")      # (admitted by tests/test_value_cases_cpu.py)
                    assert vc.cond_within_floor(r)
                    vc.judge_against_reference(f"value routes per-item y D={c.D}", item(q, i), r, ctx=(k, i))
                    a = alone[i].nowcast(t_add, y_add, t_new, non)
                    vc.judge_against_run(f"value routes per-item y D={c.D}: vs item alone", item(q, i),
                                         item(a, 0), r, ctx=(k, i))
        finally:
            f.close()
            for a in alone.values():
                a.close()
    c8 = CASES["scen8"]
    for k in c8.date_sets():
        for i in c8.sample():
            vc.judge_against_run("value routes per-item y: D=9 vs D=8", _d9_first_8(outs["scen9", k], i),
                                 item(outs["scen8", k], i), vc.reference(c8, i, k, "factor"), ctx=(k, i))


@pytest.mark.parametrize("name", ["epi_lat", "epi_irr"])
def test_epilogue_schur_blocks_tables_vs_direct_evaluation(ctx, name):
    """a single-chunk job on lattice dates reads the small Schur blocks' covariances from the resident
    tables; a batch-invariant job (ngp_job_run: the epilogue's resident tables) and any job on irregular dates (or with one
    forecast date off the lattice: the between_off set) evaluates them directly.  Both are class 3;
    each is judged against the reference, and the two against each other."""
    c = CASES[name]
    sides = [("default", c.B, {}), ("invariant", c.B, {"invariant": True})]
    judge(ctx, f"epilogue {name[-3:]}", c, sides)
    invariant_bits(ctx, name, c)


def test_fill_kernels_single_table_chain_and_other_items(ctx):
    """fill_single / fill_chain / fill_other (the fill lists of stage_general; fill_route, csrc/ngp_plan.h) in one batch, three
    items of each by compile_program's rule (value_cases.fill_kind restates it): pure stationary trees
    (one table), trees in which one operand of every general node is a table or a Linear leaf (chain),
    and trees with a general node between two general subtrees (other); every item is sampled.  The
    three are launches of class 4 whose count does not depend on the lists, so the profile cannot
    tell which kernel filled an item.  n = 321 is on the column sweep; the n = 200 ensemble (single
    tables and chains) is filled for the column sweep as well as for the one-launch kernel."""
    c = CASES["fill3"]
    assert c.sample() == list(range(9))
    assert [vc.fill_kind(p) for p in c.progs()] == list(vc.FILL_KINDS) * 3
    judge(ctx, "fill kernels", c, [("sweep", 9, {}), ("invariant", 9, {"invariant": True})])
    c2 = CASES["epi_lat"]
    assert {vc.fill_kind(c2.progs()[i]) for i in c2.sample()} == {"single", "chain"}
    judge(ctx, "fill kernels n=200", c2, [("one-launch", c2.B, {}), ("sweep", c2.B, {"short": False})])


# ---- the other entry points ------------------------------------------------------------------------------
def test_predict_batch_gives_the_bits_of_nowcast_batch_and_per_item_rows(ctx):
    """ngp_predict_batch = ngp_nowcast_batch with d = 0, D = 1: same bits; with per-item observation
    rows every sampled item against the reference and against the item alone"""
    c = CASES["epi_lat"]
    progs = c.progs()
    t, y, _, _, _ = c.data()
    Y = c.per_item_y()
    for k, (t_new, non) in c.date_sets().items():
        mu, sg, lm, info = ctx.predict_batch(progs, t, y, t_new, non)
        nc = ctx.nowcast_batch(progs, t, y, np.zeros(0), np.zeros((1, 0)), t_new, non)
        assert not info.any() and not nc["info"].any()
        assert np.array_equal(mu, nc["mu"][:, 0]) and np.array_equal(sg, nc["sigma"])
        assert np.array_equal(lm, nc["logml_full"][:, 0]) and np.array_equal(lm, nc["logml_base"])
        mu, sg, lm, info = ctx.predict_batch(progs, t, Y, t_new, non)
        assert not info.any()
        for i in c.sample():
            r = vc.reference(c, i, k, "predict")       # (admitted by tests/test_value_cases_cpu.py)
            assert vc.cond_within_floor(r)
            got = dict(logml_base=lm[i], logml_full=lm[i:i + 1], mu=mu[i], sigma=sg[i])
            vc.judge_against_reference("value routes predict, per-item y", got, r, ctx=(k, i))
            mu1, sg1, lm1, _ = ctx.predict_batch([progs[i]], t, Y[i], t_new, non)
            one = dict(logml_base=lm1[0], logml_full=lm1, mu=mu1[0], sigma=sg1[0])
            vc.judge_against_run("value routes predict, per-item y: vs item alone", got, one, r, ctx=(k, i))


def test_staged_job_run_twice_gives_the_bits_of_the_one_shot_call(ctx):
    c = CASES["epi_lat"]
    t, y, t_add, y_add, _ = c.data()
    for k in ("between", "on_f"):
        t_new, non = c.date_sets()[k]
        ref = ctx.nowcast_batch(c.progs(), t, y, t_add, y_add, t_new, non)
        job = ctx.stage_nowcast(c.progs(), t, y, t_add, y_add, t_new, non)
        try:
            for _ in range(2):
                same_bits(job.run().fetch(), ref, ctx=k)
        finally:
            job.close()

"""Admissibility and adequacy of the grammar zoo (tests/grammar_cases.py), on the CPU.

  contract   the zoo holds every shape, order, route and parameter edge it promises;
  fairness   for every (item, spec, series) that tests/test_grammar_gpu.py judges against the
             extended-precision reference, the plain fp64 oracles (oracle_np.nowcast / cov,
             oracle_c.logml_grad) pass the same judgement at A QUARTER of the tolerance — a case that
             fails is changed, never the tolerance;
  reference  hp_reference._derivs against central differences of hp_reference._value in long double,
             on every tree with a ChangePoint, in both cp_forms;
  adequacy   deliberately wrong variants of the long-double formulas (MUTANTS) must each FAIL the
             judgement on some item at the GPU tolerance: a kernel wrong in that way would be caught;
  flips      every single spec flip moves the logml of every item that holds the affected node.
No device code runs here."""
import collections

import numpy as np
import pytest

from oracle import oracle_c, oracle_np
from tests import grammar_cases as gc
from tests import hp_reference as hr
from tests import value_cases as vc
from tests.util import EPS, TOL_LOGML, check_components, tol

FLOOR_REF = 1e-10
LD = hr.LD
# the cov row's bound (module docstring of tests/test_grammar_gpu.py): measured here
COV_BOUND_FACTOR, COV_BOUND_MIN = 8.0, 16 * EPS


# ---- the coverage contract ------------------------------------------------------------------------------
def test_the_zoo_file_is_current():
    with open(gc.ZOO_FILE) as f:
        assert f.read() == gc.zoo_text(), "run python -m tests.grammar_cases"


def test_operand_kinds_and_changepoint_shapes():
    assert 35 <= len(gc.ZOO) <= 45
    inc = set().union(*(gc.incidences(p[0]) for p in gc.PROGRAMS))
    want = {(op, side, k) for op in (6, 7, 8) for side in "LR" for k in gc.KINDS}
    assert len(want) == 48 and inc == want, want - inc
    cps = [c for p in gc.PROGRAMS for c in gc.changepoints(p)]
    assert any(lg and rg for _, _, lg, rg, _, _ in cps)            # both children general subtrees
    assert any(c[4] for c in cps) and any(c[5] for c in cps)       # a ChangePoint inside the left / right
    assert max(len(gc.changepoints(p)) for p in gc.PROGRAMS) >= 8  # sigmoid slots
    assert any(gc.stationary(p[0]) and gc.n_leaves(p[0]) == 32 for p in gc.PROGRAMS)   # table slots
    sizes = [len(p[0]) for p in gc.PROGRAMS]
    assert min(sizes) == 1 and max(sizes) == 63
    for ops, par, _ in gc.PROGRAMS:        # within the library's limits (include/ngp.h)
        assert len(ops) <= 64 and len(par) <= 96
        assert max(np.cumsum([1 if o < 6 else -1 for o in ops])) <= 16


def test_orders_depths_and_the_parameter_permutation():
    orders, needs, moved = set(), {}, 0
    for name, (ops, par, _) in zip(gc.NAMES, gc.PROGRAMS):
        perm, need, od = gc.device_order(ops)
        assert sorted(perm) == list(range(len(par)))
        orders |= set(od)
        needs[name] = need
        moved += perm != list(range(len(par)))
    for op in (7, 8):
        assert {(op, "swapped"), (op, "left"), (op, "tie")} <= orders, orders
    assert needs["full32"] == 6 and gc.n_leaves(gc.PROGRAMS[gc.NAMES.index("full32")][0]) == 32
    assert max(needs.values()) == 6 and sorted(set(needs.values()))[:3] == [1, 2, 3]
    for name, kind in (("right13", "swapped"), ("left13", "left")):
        ops = gc.PROGRAMS[gc.NAMES.index(name)][0]
        od = gc.device_order(ops)[2]
        assert gc.n_leaves(ops) == 13 and needs[name] == 2
        assert sum(o == kind for _, o in od) == 11 and sum(o == "tie" for _, o in od) == 1, od
    # the mirror holds the same nodes: as many of every kind
    count = [collections.Counter(int(o) for o in gc.PROGRAMS[gc.NAMES.index(k)][0]) for k in ("right13", "left13")]
    assert count[0] == count[1]
    assert moved >= 5, moved


def test_routes():
    kinds = collections.Counter(vc.fill_kind(p) for p in gc.PROGRAMS)
    assert all(kinds[k] >= 3 for k in vc.FILL_KINDS), kinds
    sizes = [len(p[0]) for p in gc.PROGRAMS]
    buckets = collections.Counter(gc.grad_bucket(k) for k in sizes)
    assert all(buckets[b] >= 2 for b in range(6)), buckets
    assert {1, 3, 7, 15, 31, 33} <= set(sizes)
    assert len(gc.TOEP) >= 10 and any(gc.n_leaves(gc.PROGRAMS[i][0]) == 16 for i in gc.TOEP)
    ops17 = gc.PROGRAMS[gc.STAT17][0]
    assert gc.stationary(ops17) and gc.n_leaves(ops17) == 17 and gc.STAT17 not in gc.TOEP
    # the six G-sized prefixes end on six different buckets, the last one is the whole zoo
    pre = gc.prefixes(gc.BY_SIZE)
    assert [gc.grad_bucket(max(len(gc.PROGRAMS[i][0]) for i in p)) for p in pre] == list(range(6))
    assert len(pre[-1]) == len(gc.ZOO)
    assert len(gc.prefixes(gc.TOEP)) == 5
    s = gc.sample321()
    assert {gc.grad_bucket(len(gc.PROGRAMS[i][0])) for i in s} == set(range(6))


def _all_series():
    """(label, training dates) of every series a GPU row runs the zoo on"""
    out = []
    for n in (130, 321):
        for lat in (True, False):
            out.append((f"grad n={n} lattice={lat}", gc.grad_series(n, lat)[0]))
            t, _, t_add, _, _ = gc.value_case(n, lat).data()
            out.append((f"value n={n} lattice={lat}", np.concatenate([t, t_add])))
    return out


def test_parameters():
    gam, per, cps, lin, nz = set(), [], [], [], []
    for ops, par, noise in gc.PROGRAMS:
        nz.append(noise)
        pi = 0
        for op in (int(o) for o in ops):
            if op == 4:
                gam.add(par[pi + 1])
            if op == 5:
                per.append(par[pi + 1])
            if op == 2:
                lin.append(par[pi])
            pi += gc.N_PAR[op]
        cps += [(c[0], c[1]) for c in gc.changepoints((ops, par, noise))]
    assert {0.3, 1.0, 1.99} <= gam
    assert any(abs(p * 129 - round(p * 129)) < 1e-12 for p in per)        # 43 steps of the n = 130 lattice
    assert any(abs(p * 320 - round(p * 320)) < 1e-12 for p in per)        # 40 steps of the n = 321 lattice
    assert any(p > 1.0 for p in per)                                       # longer than the span
    assert any(not 0 <= c <= 1 for c in lin)
    assert (0.5, 0.01) in cps and (1.15, 0.1) in cps
    t130 = gc.grad_series(130, True)[0]
    assert any(np.isin(loc, t130) for loc, _ in cps)                       # on a training date
    assert min(nz) == gc.NOISE_LO == vc.noise_floor(321) and max(nz) == gc.NOISE_HI == 1e-1
    assert all(vc.noise_floor(130) <= v for v in nz)
    # never totally saturated: a training date within one scale of every location, on every series.
    # The ChangePoint at 1.15 with scale 0.1 lies outside the data by construction: its nearest date is
    # the last one, u = (1.15 - 1) / 0.1 = 1.5 on the gradient series and below 1.6 on the value
    # series (which end at 0.992), where d sigma / du = sech^2(u) / 2 is still 0.07.
    for label, tt in _all_series():
        for loc, sc in cps:
            u = np.min(np.abs(loc - tt)) / sc
            assert u <= (1.6 if (loc, sc) == (1.15, 0.1) else 1.0), (label, loc, sc, u)


def test_every_item_is_well_conditioned_on_every_series():
    """cond_within_floor for every item, both forms, every series: nothing is skipped and no value is
    judged above the floor"""
    for label, tt in _all_series():
        for name, p in zip(gc.NAMES, gc.PROGRAMS):
            for s in gc.BOTH_FORMS:
                K = np.asarray(hr.cov(p, tt, tt, gc.spec_dict(s), add_diag=True, dtype=np.float64))
                ev = np.linalg.eigvalsh(K)
                assert ev[0] > 0 and 50 * EPS * ev[-1] / ev[0] <= 1e-8, (label, name, s, ev[-1] / ev[0])


# ---- fairness --------------------------------------------------------------------------------------------
# the (series, specs) of the value rows: V-direct | V-one | V-lists, V-factor, V-mixed | V-mixed
VALUE_ROWS = {"n130_irregular": (130, False, gc.SPECS), "n130_lattice": (130, True, gc.BOTH_FORMS),
              "n321_lattice": (321, True, gc.BOTH_FORMS), "n321_irregular": (321, False, gc.BOTH_FORMS)}


@pytest.mark.parametrize("row", list(VALUE_ROWS))
def test_fp64_oracle_passes_the_value_rows_at_a_quarter_of_the_tolerance(row):
    n, lattice, specs = VALUE_ROWS[row]
    case = gc.value_case(n, lattice)
    t, y, t_add, y_add, _ = case.data()
    sets = case.date_sets() if n == 130 or lattice else {k: case.date_sets()[k] for k in gc.MIXED_SETS}
    for i, prog in enumerate(gc.PROGRAMS):
        for s in gc.effective_specs(i, specs):
            for k, (t_new, non) in sets.items():
                r = gc.value_reference(case, i, k, s)
                assert r.info == 0 and vc.cond_within_floor(r), (row, gc.NAMES[i], s, k, r.cond)
                lb, lf, mu, sg, info = oracle_np.nowcast(prog, t, y, t_add, y_add, t_new, non, gc.spec_dict(s))
                assert info == 0
                vc.judge_against_reference("grammar (fp64 oracle, 1/4 tol)",
                                           dict(logml_base=lb, logml_full=lf, mu=mu, sigma=sg), r,
                                           ctx=(row, gc.NAMES[i], s, k), frac=0.25)


GRAD_ROWS = {"n130_irregular": (130, False, gc.SPECS, None), "n130_lattice": (130, True, gc.SPECS, None),
             "n321_lattice": (321, True, gc.BOTH_FORMS, "sample")}


@pytest.mark.parametrize("row", list(GRAD_ROWS))
def test_fp64_oracle_passes_the_gradient_rows_at_a_quarter_of_the_tolerance(row):
    n, lattice, specs, sample = GRAD_ROWS[row]
    t, y = gc.grad_series(n, lattice)
    for i in (gc.sample321() if sample else range(len(gc.ZOO))):
        for s in gc.effective_specs(i, specs):
            r = gc.grad_reference(i, n, lattice, s)
            assert r.info == 0 and vc.cond_within_floor(r), (row, gc.NAMES[i], s, r.cond)
            lm, g, info = oracle_c.logml_grad(gc.PROGRAMS[i], t, y, gc.ngp_spec(s))
            assert info == 0
            c = (row, gc.NAMES[i], s)
            assert abs(lm - float(r.logml)) <= 0.25 * tol(TOL_LOGML, r.cond) * abs(float(r.logml)), c
            check_components("grammar gradient (fp64 oracle, 1/4 tol)", g, r.grad, r.scale, FLOOR_REF,
                             r.cond, ctx=c, factor=0.25)


def test_fp64_cov_against_the_reference_gives_the_bound_of_the_cov_row():
    """oracle_np.cov (fp64 numpy) against hp_reference.cov, entrywise on max |K_item|, over every item
    and spec: the worst value is where a correct fp64 evaluation lands; the GPU row allows 8 times
    that (device exp / pow / tanh / sin are a couple of ulp where glibc is under one, and the product
    order differs), and not less than 16 eps.  gc.COV_WORST_FP64 is the figure recorded; the
    measured one must not exceed it."""
    t1, t2, t3 = gc.cov_dates()
    worst = 0.0
    for i, prog in enumerate(gc.PROGRAMS):
        for s in gc.effective_specs(i, gc.SPECS):
            for a, b, diag in ((t1, t2, False), (t3, t3, True)):
                ref = hr.cov(prog, a, b, gc.spec_dict(s), add_diag=diag)
                got = oracle_np.cov(prog, a, b, diag, gc.spec_dict(s))
                e = float(np.max(np.abs(got.astype(LD) - ref)) / np.max(np.abs(ref)))
                worst = max(worst, e)
    print(f"fp64 cov against long double, worst |d| / max |K|: {worst:.3e} = {worst / EPS:.2f} eps")
    assert 0 < worst <= gc.COV_WORST_FP64, worst
    assert gc.COV_BOUND == max(COV_BOUND_FACTOR * gc.COV_WORST_FP64, COV_BOUND_MIN)


# ---- the reference's derivatives ------------------------------------------------------------------------
@pytest.mark.parametrize("cp_form", [0, 1])
def test_reference_derivatives_match_central_differences_on_every_changepoint_tree(cp_form):
    """dK / d theta_i of hp_reference._derivs against (K(theta + h e_i) - K(theta - h e_i)) / 2h in long
    double, h = 1e-6 |theta_i|: the truncation error, h^2 K(3) / 6, stays below 1e-9 of max |dK_i| (a
    location moves u by 1e-6 / scale <= 1e-4), and the rounding error of the difference is a few
    eps_LD max |K| / 2h <= 8 x 1.1e-19 / 2e-8 = 4.4e-11 max |K| for |theta_i| >= 0.01.
    Bound: 1e-8 max |dK_i| + 1e-10 max |K|.  On a 12 x 12 grid that straddles the locations."""
    sp = (0, 0, cp_form, 1e-5)
    tg = np.concatenate([np.linspace(0.0, 1.0, 9), [0.495, 0.505, 1.0 / 3.0]])
    T1, T2 = tg.astype(LD)[:, None], tg.astype(LD)[None, :]
    seen = 0
    for name, (ops, par, _) in zip(gc.NAMES, gc.PROGRAMS):
        if 8 not in ops:
            continue
        seen += 1
        tree = hr.rpn_to_tree(ops, par)
        dks = [np.broadcast_to(d, (tg.size, tg.size)) for d in hr._derivs(tree, T1, T2, sp, {}, None)]
        assert len(dks) == len(par)
        kmax = float(np.max(np.abs(hr._value(tree, T1, T2, sp, {}))))
        assert min(abs(v) for v in par) >= 0.01
        for i, dk in enumerate(dks):
            h = LD(1e-6) * LD(abs(par[i]))
            hi, lo = np.array(par, dtype=LD), np.array(par, dtype=LD)
            hi[i] += h
            lo[i] -= h
            # (rpn_to_tree takes floats: build the trees from long-double parameters directly)
            fd = (hr._value(_ld_tree(ops, hi), T1, T2, sp, {}) - hr._value(_ld_tree(ops, lo), T1, T2, sp, {})) / (2 * h)
            err = float(np.max(np.abs(np.broadcast_to(fd, dk.shape) - dk)))
            assert err <= 1e-8 * float(np.max(np.abs(dk))) + 1e-10 * kmax, (name, i, err, float(np.max(np.abs(dk))))
    assert seen >= 15


def _ld_tree(ops, params):
    stack, p = [], 0
    for op in (int(o) for o in ops):
        k = gc.N_PAR[op]
        pr = tuple(params[p:p + k])
        p += k
        if op < 6:
            stack.append((op, pr, None, None))
        else:
            r, l = stack.pop(), stack.pop()
            stack.append((op, pr, l, r))
    return stack[0]


# ---- adequacy: wrong formulas must fail ---------------------------------------------------------------
class Mutant:
    """hp_reference's covariance and derivatives with ONE deliberate error (mut = None: none)"""

    def __init__(self, prog, sp, mut):
        self.sp, self.mut = sp, mut
        self.tree = hr.rpn_to_tree(prog[0], prog[1])
        self.perm = gc.device_order(prog[0])[0]
        # ChangePoints in the device's evaluation order (their sigmoid slots), swapped ones marked
        self.slots, self.swapped = [], set()
        self._walk(self.tree)

    def _need(self, nd):
        if nd[0] < 6:
            return 1
        a, b = self._need(nd[2]), self._need(nd[3])
        return a + 1 if a == b else max(a, b)

    def _walk(self, nd):
        if nd[0] < 6:
            return
        swap = self._need(nd[3]) > self._need(nd[2])
        for ch in ((nd[3], nd[2]) if swap else (nd[2], nd[3])):
            self._walk(ch)
        if nd[0] == 8:
            self.slots.append(nd)
            if swap:
                self.swapped.add(id(nd))

    def leaf(self, nd, T1, T2):
        sp = self.sp
        if nd[0] == 5 and self.mut == "se_form applied to Periodic":
            sp = (sp[0], sp[0], sp[2], sp[3])
        if nd[0] == 5 and self.mut == "periodic_form ignored":
            sp = (sp[0], 0, sp[2], sp[3])
        v, d = hr._leaf(nd, T1, T2, sp, True)
        if nd[0] == 4 and self.mut == "GammaExp: factor gamma / l dropped":
            d[0] = d[0] * LD(nd[1][0]) / LD(nd[1][1])
        return v, d

    def cp(self, nd, T1, T2):
        """(first-role child, second-role child, u1, u2, s1, s2): value = s1 s2 first + (1-s1)(1-s2) second"""
        src = nd
        if self.mut == "second sigmoid slot read as the first" and len(self.slots) > 1 and nd is self.slots[1]:
            src = self.slots[0]
        a, b = nd[2], nd[3]
        if self.mut == "ChangePoint children exchanged" or \
                (self.mut == "swapped ChangePoint treated as natural" and id(nd) in self.swapped):
            a, b = b, a
        return (a, b) + hr._sig(src, T1, T2, self.sp[2])

    def value(self, nd, T1, T2):
        op = nd[0]
        if op <= 5:
            return self.leaf(nd, T1, T2)[0]
        if op == 6:
            return self.value(nd[2], T1, T2) + self.value(nd[3], T1, T2)
        if op == 7:
            return self.value(nd[2], T1, T2) * self.value(nd[3], T1, T2)
        a, b, _, _, s1, s2 = self.cp(nd, T1, T2)
        return s1 * s2 * self.value(a, T1, T2) + (1 - s1) * (1 - s2) * self.value(b, T1, T2)

    def derivs(self, nd, T1, T2, M):
        op = nd[0]
        if op <= 5:
            for dv in self.leaf(nd, T1, T2)[1]:
                yield M * dv
        elif op == 6:
            yield from self.derivs(nd[2], T1, T2, M)
            yield from self.derivs(nd[3], T1, T2, M)
        elif op == 7:
            other = nd[2] if self.mut == "adjoint of x: the same operand twice" else nd[3]
            yield from self.derivs(nd[2], T1, T2, M * self.value(other, T1, T2))
            yield from self.derivs(nd[3], T1, T2, M * self.value(nd[2], T1, T2))
        else:
            a, b, u1, u2, s1, s2 = self.cp(nd, T1, T2)
            for ch in (nd[2], nd[3]):          # caller's parameter order: left subtree, right subtree
                yield from self.derivs(ch, T1, T2, M * (s1 * s2 if ch is a else (1 - s1) * (1 - s2)))
            va, vb = self.value(a, T1, T2), self.value(b, T1, T2)
            sgn = -1 if self.sp[2] else 1
            if self.mut == "cp_form ignored in the derivative":
                sgn = 1
            sc = LD(nd[1][1])
            ds1, ds2 = 2 * s1 * (1 - s1), 2 * s2 * (1 - s2)
            g1, g2 = va * s2 - vb * (1 - s2), va * s1 - vb * (1 - s1)
            loc_sign = -1 if self.mut == "sign of d / d location" else 1
            yield M * (g1 * ds1 + g2 * ds2) * (loc_sign * sgn / sc)
            w1 = u2 if self.mut == "u2 in both d / d scale terms" else u1
            yield M * (g1 * ds1 * (-w1 / sc) + g2 * ds2 * (-u2 / sc))

    def evaluate(self, noise, t, y):
        """(logml, gradient in the caller's order + d / d noise), long double"""
        n = t.size
        T1, T2 = t.astype(LD)[:, None], t.astype(LD)[None, :]
        K = np.array(np.broadcast_to(self.value(self.tree, T1, T2), (n, n)), dtype=LD)
        K[np.arange(n), np.arange(n)] += LD(noise) + LD(self.sp[3])
        L, info = hr.cholesky_ld(K)
        assert info == 0
        z = hr.solve_lower(L, y.astype(LD))
        alpha = hr.solve_upper_t(L, z)
        W = hr.solve_lower(L, np.eye(n, dtype=LD))
        kinv = W.T @ W
        lm = -(z @ z) / 2 - np.sum(np.log(np.diag(L))) - LD(n) / 2 * np.log(2 * hr.PI_LD)
        one = np.ones((1, 1), dtype=LD)
        g = [(alpha @ np.broadcast_to(dK, (n, n)) @ alpha - np.sum(kinv * dK)) / 2
             for dK in self.derivs(self.tree, T1, T2, one)]
        if self.mut == "gradient in device order":
            g = [g[k] for k in self.perm]
        g.append((alpha @ alpha - np.trace(kinv)) / 2)
        return lm, np.array(g, dtype=LD)


# (the error, the spec it shows under, items that hold what it breaks — tried in turn)
MUTANTS = [
    ("ChangePoint children exchanged", (0, 0, 0), ("cp_SE_C", "cp_GE_LIN")),
    ("swapped ChangePoint treated as natural", (0, 0, 0), ("cp_C_TIMES", "cp_LIN_CP", "cp8")),
    ("sign of d / d location", (0, 0, 0), ("cp_SE_C", "plus_PER_CP")),
    ("u2 in both d / d scale terms", (0, 0, 0), ("cp_SE_C", "cp_both_general")),
    ("cp_form ignored in the derivative", (1, 1, 1), ("cp_PER_SE", "cp8")),
    ("se_form applied to Periodic", (1, 0, 0), ("per_third", "plus_LIN_PER")),
    ("periodic_form ignored", (1, 1, 1), ("per_third", "times_PER_LIN")),
    ("GammaExp: factor gamma / l dropped", (0, 0, 0), ("ge_gamma03", "plus_C_GE")),
    ("adjoint of x: the same operand twice", (0, 0, 0), ("times_GE_C", "times_PER_LIN")),
    ("gradient in device order", (0, 0, 0), ("plus_SE_PLUS", "times_C_PLUS", "cp8")),
    ("second sigmoid slot read as the first", (0, 0, 0), ("cp_LIN_CP", "cp_CP_PLUS", "cp8")),
]


def _judged(name, s, mut):
    """does the (mutated) evaluation of the item pass the G-sized row's judgement?"""
    i = gc.NAMES.index(name)
    t, y = gc.grad_series(130, True)
    r = gc.grad_reference(i, 130, True, s)
    lm, g = Mutant(gc.PROGRAMS[i], hr.spec_tuple(gc.spec_dict(s)), mut).evaluate(gc.PROGRAMS[i][2], t, y)
    try:
        assert abs(float(lm) - float(r.logml)) <= tol(TOL_LOGML, r.cond) * abs(float(r.logml))
        check_components("mutant", g, r.grad, r.scale, FLOOR_REF, r.cond, record=False)
    except AssertionError:
        return False
    return True


def test_the_unmutated_restatement_is_the_reference():
    for name, s in (("cp8", (0, 0, 0)), ("cp_LIN_CP", (1, 1, 1)), ("times_C_PLUS", (1, 0, 0)),
                    ("right13", (0, 1, 0)), ("gen15", (0, 0, 1))):
        assert _judged(name, s, None), (name, s)


@pytest.mark.parametrize("mut,s,names", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_every_wrong_formula_fails_on_some_item(mut, s, names):
    assert len(MUTANTS) >= 10
    assert not all(_judged(name, s, mut) for name in names), mut


# ---- the spec flips matter ------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", gc.SINGLE_FLIPS)
def test_a_single_flip_moves_every_item_that_holds_the_node(flip):
    kind, n_seen = gc.FLIP_KIND[flip], 0
    t, y = gc.grad_series(130, True)
    for i, prog in enumerate(gc.PROGRAMS):
        if kind not in prog[0]:
            assert gc.effective_specs(i, [flip]) == [(0, 0, 0)]
            continue
        n_seen += 1
        a = hr.evaluate(prog, t, y, gc.spec_dict((0, 0, 0)), grad=False)
        b = hr.evaluate(prog, t, y, gc.spec_dict(flip), grad=False)
        move = abs(float(b.logml) - float(a.logml))
        assert move > 1e4 * tol(TOL_LOGML, a.cond) * abs(float(a.logml)), (gc.NAMES[i], flip, move)
    assert n_seen >= 10

"""The items, series and forecast dates of the value-path tests, in one table.

tests/test_value_routes_gpu.py runs these cases through the HIP kernels; tests/test_value_cases_cpu.py
runs the SAME sampled (case, item, forecast-date set) triples through the plain fp64 oracle and
requires it to pass the same judgement at a quarter of the tolerance — a case the fp64 oracle
cannot pass with that margin would make the GPU test unfair, so it does not belong here.

Dates.  ``Case.data`` draws 2 (n + d) + 1 dates with ``series`` and trains on every second one: the
n + d training dates (t, then t_add) have an unobserved date in every gap — on a lattice series the
odd lattice points (missing weeks; the main block keeps a constant stride of two lattice steps, so
structured storage still applies).  Forecast-date sets of m dates:
  beyond       after the last appended date (the everyday forecast)
  between      the unobserved date inside m gaps spread over the main block, its 64-block seams, the
               tail and the appended points (lattice series: ON the lattice)
  between_off  lattice series only: 0.37 of the way through the same gaps — off the lattice, so the
               job has no tables at all and every covariance entry is evaluated directly
  on / on_f    m observed dates (first, last appended, spread between), with the noise added to the
               predictive variance (noise_on_new = 1) and without (0: the variance of f itself,
               which is what is left of K22 - V'V after almost complete cancellation)
Noise is log-uniform in [max(1e-3, 5e-6 n), 1e-1]: the smallest predictive variance of a case is
well below its largest, and cond(K) <= about n k(0) / noise stays below 9e5 (50 eps cond <= 1e-8:
no case is judged above the floor, none is skipped; the CPU test asserts it).
"""
import functools
from dataclasses import dataclass, field

import numpy as np

from tests import hp_reference as hr
from tests.util import EPS, TOL_LOGML, TOL_PRED, check_components

FLOOR_RT = 1e-11        # one side of a switch against the other / the item alone (rounding)


# ---- items (shared with tests/test_routes_gpu.py) --------------------------------------------------
def _leaf(rng, stationary=True, small=False):
    """(op, params) of one leaf, sized for dates in [0, 1] (small: at most two parameters)"""
    kinds = [1, 3] if small else [1, 3, 4, 5] if stationary else [2, 3, 5]
    op = int(rng.choice(kinds))
    if op == 1:
        return op, [rng.uniform(0.1, 0.5)]
    if op == 2:
        return op, [rng.uniform(0.3, 0.7), rng.uniform(0.05, 0.2), rng.uniform(0.2, 0.8)]
    if op == 3:
        return op, [rng.uniform(0.05, 0.3), rng.uniform(0.2, 1.0)]
    if op == 4:
        return op, [rng.uniform(0.05, 0.3), rng.uniform(1.0, 1.9), rng.uniform(0.2, 1.0)]
    return op, [rng.uniform(0.8, 2.0), rng.uniform(0.05, 0.3), rng.uniform(0.2, 1.0)]


def tree(rng, n_ops, stationary=True, linear=False, cp=False):
    """an RPN program of exactly n_ops operators (odd): a left fold of leaves by +, x (and one
    ChangePoint), stack depth 2"""
    assert n_ops % 2 == 1
    leaves = (n_ops + 1) // 2
    small = leaves > 16                    # NGP_MAX_PARAMS = 96
    op, pr = _leaf(rng, stationary, small)
    if linear:
        op, pr = 2, [0.5, 0.1, 0.5]
    ops, params = [op], list(pr)
    for k in range(1, leaves):
        op, pr = _leaf(rng, stationary, small)
        ops.append(op)
        params += pr
        if cp and k == leaves - 1:
            ops.append(8)
            params += [rng.uniform(0.3, 0.7), 0.05]
        else:
            # products of more than two factors would make K too small to matter: mostly sums
            ops.append(7 if k % 4 == 1 else 6)
    return np.array(ops, np.int32), np.array(params, float), float(rng.uniform(0.02, 0.1))


def series(n, lattice=True, seed=0):
    rng = np.random.default_rng(seed)
    if lattice:
        t = np.arange(n, dtype=float) / (n - 1)
    else:
        t = np.sort(rng.uniform(0.0, 1.0, n))
        t += np.arange(n) * 1e-4                                   # no two dates within 1e-4
        t /= t[-1]
    y = np.sin(2 * np.pi * t * 3) + 0.5 * t + 0.1 * rng.standard_normal(n)
    return t, y


def ensemble(seed, sizes, B, stationary=True, linear_every=0, cp_every=0):
    """B items whose op counts cycle through ``sizes``"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(B):
        lin = bool(linear_every) and i % linear_every == linear_every - 1
        cpi = bool(cp_every) and i % cp_every == cp_every - 1
        out.append(tree(rng, sizes[i % len(sizes)], stationary and not lin and not cpi, lin, cpi))
    return out


# ---- the cases ----------------------------------------------------------------------------------------
SIZES = (1, 3, 5, 7, 9)
DATE_SETS = ("beyond", "between", "between_off", "on", "on_f")


def noise_floor(n):
    return max(1e-3, 5e-6 * n)


@functools.lru_cache(maxsize=None)
def _items(seed, sizes, B, n, linear_every, cp_every, stationary):
    progs = ensemble(seed, list(sizes), B, stationary, linear_every, cp_every)
    rng = np.random.default_rng(seed + 7919)
    lo = noise_floor(n)
    nz = np.exp(rng.uniform(np.log(lo), np.log(1e-1), B))
    nz[0], nz[-1] = lo, 1e-1                       # both ends of the range are always present
    return tuple((ops, par, float(v)) for (ops, par, _), v in zip(progs, nz))


@dataclass(frozen=True)
class Case:
    n: int
    B: int                      # items of the larger side
    d: int = 2
    D: int = 2
    m: int = 5
    lattice: bool = True
    seed: int = 1               # of the series
    item_seed: int = 21
    sizes: tuple = SIZES
    linear_every: int = 5
    cp_every: int = 7
    sides: tuple = ()           # batch sizes run on the GPU (default: B alone)
    extra: tuple = ()           # items sampled beyond first / last / one per tree size
    per_size: bool = True
    explicit: tuple = field(default=(), compare=False)   # programs given outright (fill-kernel row)

    def progs(self):
        if self.explicit:
            return list(self.explicit)
        # stationary trees, with every linear_every-th a Linear chain and every cp_every-th a
        # ChangePoint tree (both general: not stationary)
        return list(_items(self.item_seed, self.sizes, self.B, self.n, self.linear_every,
                           self.cp_every, True))

    def batch_sizes(self):
        return self.sides or (self.B,)

    def data(self):
        """t [n], y [n], t_add [d], y_add [D, d] and every date of the underlying series"""
        N = 2 * (self.n + self.d) + 1
        ta, ya = series(N, self.lattice, self.seed)
        tr = np.arange(self.n + self.d) * 2
        rng = np.random.default_rng(self.seed + 31)
        y_add = ya[tr[self.n:]][None, :] + 0.1 * rng.standard_normal((self.D, self.d))
        return ta[tr[:self.n]], ya[tr[:self.n]], ta[tr[self.n:]], y_add, ta

    def per_item_y(self):
        """Y [B, n]: every item its own observation row (the tail of a row is part of the item's
        appended block in the epilogue)"""
        _, y, _, _, _ = self.data()
        rng = np.random.default_rng(self.seed + 77)
        return y[None, :] + 0.05 * rng.standard_normal((self.B, self.n))

    def date_sets(self):
        """{set name: (t_new [m], noise_on_new)}"""
        n, d, m = self.n, self.d, self.m
        t, _, t_add, _, ta = self.data()
        nt = n + d
        assert m <= nt - 1
        gaps = np.unique(np.round(np.linspace(0, nt - 2, m)).astype(int))
        obs = np.unique(np.round(np.linspace(0, nt - 1, m)).astype(int))
        assert gaps.size == m and obs.size == m
        step = ta[2] - ta[0] if self.lattice else 2.0 / (ta.size - 1)
        out = {"beyond": (ta[2 * nt - 2] + step * np.arange(1, m + 1), True),
               "between": (ta[2 * gaps + 1].copy(), True)}
        if self.lattice:
            out["between_off"] = (ta[2 * gaps] + 0.37 * (ta[2 * gaps + 2] - ta[2 * gaps]), True)
        out["on"] = (ta[2 * obs].copy(), True)
        out["on_f"] = (ta[2 * obs].copy(), False)
        return out

    def sample(self, B=None):
        """first, last, one item of every op count, one Linear and one ChangePoint tree, the extra
        items — of the smaller side, so
        that every side holds them"""
        B = B or min(self.batch_sizes())
        progs = self.progs()
        seen, idx = set(), {0, B - 1, *self.extra}
        if not self.explicit:            # the first Linear chain and the first ChangePoint tree
            idx |= {self.linear_every - 1, self.cp_every - 1}
        if self.per_size:
            for i in range(B):
                k = len(progs[i][0])
                if k not in seen:
                    seen.add(k)
                    idx.add(i)
        return sorted(i for i in idx if 0 <= i < B)


def _c(**kw):
    return Case(**kw)


# explicit items of the fill-kernel row (csrc/ngp_api.hip, stage_general: fill_single / fill_chain /
# fill_other from compile_program's reduced program; ``fill_kind`` below restates the rule): a pure
# stationary tree is ONE table; a tree in which one operand of every general node is a leaf of the
# reduced program (a stationary subtree or a Linear node) is a chain; a general node whose two
# operands are both general subtrees needs the stack (other)
FILL_SINGLE = (((3,), (0.21, 0.9), 2e-3), ((4, 5, 6), (0.3, 1.3, 0.5, 0.9, 0.25, 0.4), 3e-3),
               ((5, 3, 7, 1, 6), (0.8, 0.13, 0.7, 0.2, 0.6, 0.3), 1e-1))
FILL_CHAIN = (((2, 3, 6), (0.37, 0.11, 0.8, 0.15, 0.7), 4e-3),
              ((3, 2, 7, 5, 6), (0.25, 0.9, 0.5, 0.1, 0.5, 1.1, 0.2, 0.5), 2e-2),
              ((3, 2, 3, 7, 6), (0.1, 0.5, 0.5, 0.1, 0.5, 0.3, 0.7), 1e-2))
FILL_OTHER = (((2, 3, 7, 2, 5, 7, 6), (0.4, 0.1, 0.6, 0.2, 0.8, 0.6, 0.05, 0.4, 0.9, 0.2, 0.5), 5e-3),
              ((3, 2, 7, 4, 2, 7, 6), (0.15, 0.7, 0.5, 0.1, 0.5, 0.2, 1.5, 0.6, 0.4, 0.05, 0.3), 3e-2),
              ((2, 3, 6, 2, 5, 6, 8), (0.4, 0.1, 0.4, 0.2, 0.7, 0.6, 0.05, 0.5, 1.1, 0.2, 0.5, 0.5, 0.05),
               2e-3))
FILL_KINDS = ("single", "chain", "other")


def _explicit(groups):
    out = []
    for g in zip(*groups):                  # interleaved: single, chain, other, single, ...
        for ops, par, nz in g:
            out.append((np.array(ops, np.int32), np.array(par, float), float(nz)))
    return tuple(out)


def fill_kind(program):
    """which fill kernel an item gets on lattice dates — compile_program's reduced program
    (csrc/ngp_api.hip): stationary subtrees are table leaves; at a general binary node the operand
    that needs the deeper stack goes first (the left one on a tie) and the other rides along with
    the instruction if it is a table or a Linear leaf; rchain = every instruction after the first
    carries such a leaf"""
    arity = {1: 0, 2: 0, 3: 0, 4: 0, 5: 0, 6: 2, 7: 2, 8: 2}
    stack = []                       # (stationary, need, is Linear leaf, chain)
    for op in (int(o) for o in program[0]):
        if arity[op] == 0:
            stack.append((op != 2, 1, op == 2, True))
            continue
        r, l = stack.pop(), stack.pop()
        stat = op != 8 and l[0] and r[0]
        need = l[1] + 1 if l[1] == r[1] else max(l[1], r[1])
        first, second = (r, l) if r[1] > l[1] else (l, r)
        leaf2 = second[0] or second[2]
        stack.append((stat, need, False, stat or (leaf2 and (first[0] or first[3]))))
    (stat, _, _, chain), = stack
    return "single" if stat else "chain" if chain else "other"


CASES = {
    # one-launch kernel | column sweep: the main block (n0 = 256 | 320, small_plan: nb0 <= 4)
    "short319": _c(n=319, B=24, D=3, m=6, seed=2),
    "short320": _c(n=320, B=24, D=3, m=6, seed=2),
    # ... and the batch size (SM_MAX_ITEMS)
    "items4097_lat": _c(n=200, B=4097, sides=(4096, 4097), extra=(1, 2047, 2048, 4094, 4095), seed=3),
    "items4097_irr": _c(n=200, B=4097, sides=(4096, 4097), extra=(1, 2047, 2048, 4094, 4095), seed=3,
                        lattice=False),
    # aux sweeps of the one-launch kernel at n0 = 256 (nbe = 16): naux = 3 + 2 + m + 1
    "sweeps1": _c(n=259, B=12, m=5, seed=4),
    "sweeps2": _c(n=259, B=12, m=60, seed=4),
    "sweeps3": _c(n=259, B=12, m=180, seed=4),
    # diagonal blocks, 512 | 513 items in one chunk, nb0 = 7 + a tail of one point
    "diag513": _c(n=449, B=513, sides=(512, 513), extra=(255, 256, 511), m=6, seed=5),
    # split-k fat steps: nb0 = 7 | 8 at 40 items, 512 | 513 items at nb0 = 8
    "splitk_nb7": _c(n=449, B=40, m=6, seed=5),
    "splitk_nb8": _c(n=513, B=40, m=6, seed=6),
    "splitk513": _c(n=513, B=513, sides=(512, 513), extra=(255, 256, 511), m=6, seed=6),
    # two lanes: nb0 = 23 | 24 at 64 items, 63 | 64 items at nb0 = 24 (reference in fp64: tol_factor 2)
    "lanes_nb23": _c(n=1473, B=64, d=1, m=4, extra=(31, 32), per_size=False, seed=7, linear_every=4),
    "lanes_nb24": _c(n=1537, B=64, sides=(63, 64), d=1, m=4, extra=(30, 31, 32), per_size=False,
                     seed=8, linear_every=4),
    # aux tiles of the column sweep at nb0 = 5: naux = 1 + 2 + m + 1 = 64 | 65 | 128 | 129
    "auxtiles64": _c(n=321, B=10, m=60, seed=9),
    "auxtiles65": _c(n=321, B=10, m=61, seed=9),
    "auxtiles128": _c(n=321, B=10, m=124, seed=9),
    "auxtiles129": _c(n=321, B=10, m=125, seed=9),
    # scenario solve of the epilogue: D = 8 | 9
    "scen8": _c(n=130, B=16, d=3, D=8, seed=10),
    "scen9": _c(n=130, B=16, d=3, D=9, seed=10),
    # epilogue tables (lattice, single chunk) | direct evaluation
    "epi_lat": _c(n=200, B=32, D=3, m=8, seed=11),
    "epi_irr": _c(n=200, B=32, D=3, m=8, seed=11, lattice=False),
    # the three fill kernels in one batch
    "fill3": _c(n=321, B=9, m=6, seed=12, explicit=_explicit((FILL_SINGLE, FILL_CHAIN, FILL_OTHER)),
                extra=tuple(range(9))),
}
# column pairing: nb0 = 1 .. 5, each with a ragged tail of 1 and of 63 points
for _nb in (1, 2, 3, 4, 5):
    for _tail in (1, 63):
        CASES[f"pairs_nb{_nb}_tail{_tail}"] = _c(n=64 * _nb + _tail, B=8, d=1, m=4, seed=13 + _nb,
                                                 sizes=(1, 3, 5), per_size=False)


# ---- the planner of the one-launch kernel, restated (csrc/ngp_plan.h small_plan, value jobs) -----
SM_WAVES, SM_NSLOT, SM_MAX_PANEL, SM_MAX_SWEEPS, NGP_MAX_AUX = 8, 20, 34, 4, 192


def small_plan_sweeps(n, d, m):
    """sweeps the one-launch kernel makes over a value job of this geometry (0: the column sweep
    takes it) — a restatement of small_plan; tests/test_value_cases_cpu.py compares it with the
    planner's own code (tests/sanitize/plan_sweeps.cpp) over every value geometry"""
    n0 = n // 64 * 64
    naux = (n - n0) + d + m + 1
    if n0 <= 0 or n0 // 64 > 4:
        return 0
    nbe = n0 // 16
    cap_main, cap_aux = (SM_WAVES - 1) * SM_NSLOT, SM_WAVES * SM_NSLOT
    used = nbe * (nbe - 1) // 2
    if used > cap_main:
        return 0
    nba = (naux + 15) // 16
    a = min(nba, (cap_main - used) // nbe, SM_MAX_PANEL - nbe)
    ns, npanel = 1, nbe + a
    while a < nba:
        if ns == SM_MAX_SWEEPS:
            return 0
        b = min(nba, a + min(cap_aux // nbe, SM_MAX_PANEL - nbe))
        ns, npanel, a = ns + 1, max(npanel, nbe + b - a), b
    return 0 if npanel > SM_MAX_PANEL else ns


# ---- the judgement both tests make -----------------------------------------------------------------
# cases that also run with per-item observation rows (ngp_factor_create / ngp_predict_batch take
# y [B, n]); "predict": without the appended points (d = 0, D = 1)
PER_ITEM_Y = {"scen8": "factor", "scen9": "factor", "epi_lat": "predict"}


def inputs(case, i, set_name, per_item=None):
    """(program, t, y, t_add, y_add, t_new, noise_on_new) of one sampled triple; per_item: the
    item's own observation row, "predict" without appended points"""
    t, y, t_add, y_add, _ = case.data()
    t_new, non = case.date_sets()[set_name]
    if per_item:
        y = case.per_item_y()[i]
    if per_item == "predict":
        t_add, y_add = np.zeros(0), np.zeros((1, 0))
    return case.progs()[i], t, y, t_add, y_add, t_new, non


def reference(case, i, set_name, per_item=None):
    prog, t, y, t_add, y_add, t_new, non = inputs(case, i, set_name, per_item)
    return hr.nowcast(prog, t, y, t_add, y_add, t_new, None, noise_on_new=non)


def judge_against_reference(what, out, r, ctx=None, frac=1.0):
    """``out``: logml_base, logml_full [D], mu [D, m], sigma [m, m] of ONE item, against the
    reference ``r`` (hp_reference.nowcast): mu on the scale sqrt(s_aa), sigma on sqrt(s_aa s_bb),
    logml relative.  frac: the share of the tolerance allowed (1/4 for the fp64 oracle on the CPU)"""
    assert r.info == 0, ctx
    f = r.tol_factor * frac
    d, dd = hr.pred_scales(r.sigma)
    lm_ref = np.concatenate([[float(r.logml_base)], np.asarray(r.logml_full, float)])
    lm = np.concatenate([[out["logml_base"]], np.asarray(out["logml_full"], float).reshape(-1)])
    check_components(f"{what}: logml vs reference", lm, lm_ref, np.abs(lm_ref), TOL_LOGML, r.cond,
                     ctx=ctx, factor=f)
    mu = np.asarray(out["mu"], float).reshape(-1, d.size)
    check_components(f"{what}: mu vs reference", mu, np.asarray(r.mu, float), d[None, :], TOL_PRED,
                     r.cond, ctx=ctx, factor=f)
    check_components(f"{what}: sigma vs reference", out["sigma"], r.sigma, dd, TOL_PRED, r.cond,
                     ctx=ctx, factor=f)


def judge_against_run(what, out, other, r, ctx=None, frac=1.0):
    """one GPU run of an item against another run of it (the other side of a switch, the item in a
    call of its own): rounding, FLOOR_RT on the same scales.  frac: the share of the tolerance
    allowed (1/4 for two fp64 evaluations on the CPU, tests/test_geometry_cases_cpu.py)"""
    d, dd = hr.pred_scales(r.sigma)
    lm = np.concatenate([[out["logml_base"]], np.asarray(out["logml_full"], float).reshape(-1)])
    lo = np.concatenate([[other["logml_base"]], np.asarray(other["logml_full"], float).reshape(-1)])
    check_components(f"{what}: logml", lm, lo, np.abs(lo), 1e-12, r.cond, ctx=ctx, factor=frac)
    check_components(f"{what}: mu", out["mu"], other["mu"], d[None, :], FLOOR_RT, r.cond, ctx=ctx,
                     factor=frac)
    check_components(f"{what}: sigma", out["sigma"], other["sigma"], dd, FLOOR_RT, r.cond, ctx=ctx,
                     factor=frac)


def cond_within_floor(r):
    return 50 * EPS * r.cond <= 1e-8

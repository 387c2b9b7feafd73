"""The grammar zoo: about forty kernel trees written down by hand, one for every way a tree can be
put together, judged on every evaluator of the device (tests/test_grammar_gpu.py) and admitted on
the CPU (tests/test_grammar_cases_cpu.py).

tests/value_cases.py::tree is a left fold of leaves — stack depth 2, at most one ChangePoint, at the
root.  The zoo holds what that shape cannot: every node kind as the left and as the right operand of
every binary node, nested ChangePoints, general subtrees on both sides, children the device
evaluates in the other order (Sethi-Ullman: csrc/ngp_api.hip compile_program, restated in
``device_order`` below), register stacks up to depth 6, eight sigmoid slots, 32 table slots, and
parameters at the edges of their ranges.  Every item runs under both formula forms (``SPECS``).

Dates live in [0, 1] (value_cases.series).  The gradient rows use series(130) and series(321)
themselves: lattice steps 1/129 and 1/320.  The value rows use value_cases.Case: every second point
of a lattice of step 1/264 (n = 130, d = 2) or 1/646 (n = 321).  1/3 = 43/129 = 88/264 is a date of
both n = 130 lattices, 1/2 = 160/320 of the n = 321 gradient lattice.

Noise: value_cases' range with the floor of the longer series, noise_floor(321) = 1.605e-3 ... 1e-1,
both ends present; amplitudes are sized so that cond(K) stays below 9e5 (cond_within_floor).

``python -m tests.grammar_cases`` rewrites tests/golden/grammar_zoo_v1.txt, the zoo as the mock-runtime
driver reads it (tests/sanitize/route_trace.cpp --grammar); the CPU test asserts that it is current.
"""
import os
from collections import namedtuple

import numpy as np

from nowcastautogp_amd import gp
from nowcastautogp_amd._abi import default_spec
from nowcastautogp_amd.gp import ChangePoint as CP
from nowcastautogp_amd.gp import Constant as C
from nowcastautogp_amd.gp import GammaExponential as GE
from nowcastautogp_amd.gp import Linear as LIN
from nowcastautogp_amd.gp import Periodic as PER
from nowcastautogp_amd.gp import Plus as P
from nowcastautogp_amd.gp import SquaredExponential as SE
from nowcastautogp_amd.gp import Times as T
from tests import hp_reference as hr
from tests import value_cases as vc

ZOO_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grammar_zoo_v1.txt")

# (se_form, periodic_form, cp_form): both forms, then the three single flips (rows marked * only)
SPECS = ((0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1))
BOTH_FORMS, SINGLE_FLIPS = SPECS[:2], SPECS[2:]
FLIP_KIND = {(1, 0, 0): gp.SQUARED_EXPONENTIAL, (0, 1, 0): gp.PERIODIC, (0, 0, 1): gp.CHANGE_POINT}

NOISE_LO, NOISE_HI = vc.noise_floor(321), 1e-1
THIRD = 43.0 / 129.0            # a training date of both n = 130 lattices (= 88 / 264)
KINDS = ("C", "LIN", "SE", "GE", "PER", "PLUS", "TIMES", "CP")
KIND_OF_OP = dict(zip(range(1, 9), KINDS))

Item = namedtuple("Item", "name tree noise")


# ---- operands of the pair table: one subtree of every kind for the left side, one for the right ----
def left(kind):
    return {"C": lambda: C(0.3),
            "LIN": lambda: LIN(0.4, 0.1, 0.6),
            "SE": lambda: SE(0.12, 0.7),
            "GE": lambda: GE(0.25, 1.0, 0.6),                       # gamma = 1: |d| itself
            "PER": lambda: PER(0.9, THIRD, 0.5),                    # period = 43 lattice steps (n = 130)
            "PLUS": lambda: P(SE(0.3, 0.4), C(0.1)),
            "TIMES": lambda: T(PER(1.2, 0.25, 0.8), SE(0.5, 0.9)),
            "CP": lambda: CP(SE(0.08, 0.5), C(0.2), 0.35, 0.08)}[kind]()


def right(kind):
    return {"C": lambda: C(0.15),
            "LIN": lambda: LIN(-0.2, 0.05, 0.3),                    # intercept outside [0, 1]
            "SE": lambda: SE(0.4, 0.5),
            "GE": lambda: GE(0.6, 1.99, 0.4),                       # gamma at the upper edge
            "PER": lambda: PER(0.7, 1.7, 0.6),                      # a period longer than the span
            "PLUS": lambda: P(LIN(0.6, 0.1, 0.4), SE(0.2, 0.3)),
            "TIMES": lambda: T(SE(0.15, 0.8), GE(0.3, 0.3, 0.9)),   # gamma at the lower edge
            "CP": lambda: CP(C(0.25), SE(0.1, 0.6), 0.65, 0.05)}[kind]()


# the right operand's kind for every left kind: a shift of KINDS per binary node, so that the eight
# items of a node cover its sixteen (kind, side) incidences and the three child orders
SHIFT = {"plus": 3, "times": 5, "cp": 6}
JOIN = {"plus": P, "times": T, "cp": lambda l, r: CP(l, r, 0.55, 0.06)}


def _pair_items():
    nz = (2e-2, 3e-2, 4e-3, 1.5e-2, 6e-3, 2.5e-2, 5e-2, 8e-3)
    out = []
    for what in ("plus", "times", "cp"):
        for i, k in enumerate(KINDS):
            k2 = KINDS[(i + SHIFT[what]) % 8]
            out.append(Item(f"{what}_{k}_{k2}", JOIN[what](left(k), right(k2)), nz[i]))
    return out


# ---- large trees ---------------------------------------------------------------------------------------
def balanced(leaves, joins):
    """a complete binary tree over the leaves (a power of two of them); joins[level] cycles over the
    pairs of that level, level 0 at the leaves"""
    level, depth = list(leaves), 0
    while len(level) > 1:
        js = joins[depth % len(joins)]
        level = [js[k % len(js)](level[2 * k], level[2 * k + 1]) for k in range(len(level) // 2)]
        depth += 1
    return level[0]


def _stationary_leaves(k):
    """k stationary leaves of small amplitude (a sum of 32 of them stays near 1.5): SE with
    lengthscales 0.05 .. 0.5, every fourth a Periodic, every eighth a GammaExp / a Constant"""
    out = []
    for i in range(k):
        if i % 8 == 7:
            out.append(C(0.02 + 0.001 * i))
        elif i % 8 == 3:
            out.append(GE(0.1 + 0.02 * i, (0.3, 1.0, 1.99, 1.5)[(i // 8) % 4], 0.06))
        elif i % 4 == 1:
            out.append(PER(0.8 + 0.05 * i, (0.125, THIRD, 0.21, 1.7)[(i // 4) % 4], 0.05))
        else:
            out.append(SE(0.05 + 0.015 * i, 0.04 + 0.002 * i))
    return out


SUMS, MIXED = (P,), (P, T)


def _chain13(right_leaning):
    """thirteen leaves in a chain, a Linear leaf at the far end and a ChangePoint half way: the
    right-leaning form is evaluated last-leaf-first by the device (every node swapped), the
    left-leaning mirror as written"""
    lv = [LIN(0.5, 0.1, 0.4)] + _stationary_leaves(12)
    acc = lv[0]
    for k in range(1, 13):
        if k == 6:
            join = lambda a, b: CP(a, b, 0.4, 0.1)          # noqa: E731
        else:
            join = T if k % 4 == 1 else P
        acc = join(lv[k], acc) if right_leaning else join(acc, lv[k])
    return acc


def _cp8():
    """eight ChangePoints over nine leaves, on training dates (1/3, 1/2) and between them;
    ChangePoints inside the left and inside the right child of others; a right subtree that is
    evaluated first (need 3 against 1).  A leaf under nested ChangePoints is weighted by a product
    of sigmoids; whichever cp_form holds, that product is far from zero somewhere only if the
    nested transitions overlap, so the locations lie within about one scale of their parent's: a
    leaf whose window is empty would have every term at rounding level (not covered)."""
    lft = CP(CP(SE(0.1, 0.8), LIN(0.3, 0.1, 0.5), 0.30, 0.08),
             CP(PER(1.1, 0.125, 0.6), C(0.3), THIRD, 0.07), 0.38, 0.1)
    rgt = CP(GE(0.2, 1.5, 0.7),
             CP(CP(SE(0.3, 0.5), SE(0.05, 0.9), 0.55, 0.1),
                CP(C(0.2), SE(0.15, 0.6), 0.5, 0.06), 0.6, 0.08), 0.52, 0.2)
    return CP(lft, rgt, 0.45, 0.15)


def _full32_general():
    """a complete tree of 32 leaves with Linear leaves and six ChangePoints: register stack 6, six
    sigmoid slots, and general subtrees on both sides of nearly every node"""
    lv = _stationary_leaves(32)
    for i in (0, 9, 18, 27):
        lv[i] = LIN(0.2 + 0.02 * i, 0.02, 0.05)
    for i in (3, 11, 19):                  # (96 parameters at most: three-parameter leaves made Constants)
        lv[i] = C(0.03)
    # (nested transitions overlap: see _cp8)
    cps = iter([(0.4, 0.1), (THIRD, 0.15), (0.45, 0.12), (0.6, 0.1), (0.55, 0.15), (0.5, 0.2)])

    def cp(a, b):
        loc, sc = next(cps)
        return CP(a, b, loc, sc)
    return balanced(lv, [(P, T, P, P), (P, cp, P, P), (cp, P), (P, cp), (cp,)])


ZOO = [
    # ---- one leaf (grad_bucket 0): the NL = 1 contraction, one table, Linear alone
    Item("se", SE(0.21, 0.9), NOISE_LO),
    Item("ge_gamma03", GE(0.3, 0.3, 0.8), 5e-3),
    Item("per_third", PER(0.9, THIRD, 0.7), 4e-3),          # period = 43 steps of 1/129, 88 of 1/264
    Item("per_eighth", PER(1.3, 0.125, 0.6), 6e-3),         # period = 40 steps of 1/320
    Item("lin_outside", LIN(1.3, 0.1, 0.3), 5e-2),          # intercept outside [0, 1]
    Item("const", C(0.4), NOISE_HI),
    # ---- every kind on either side of +, x and ChangePoint (3 to 7 operators)
    *_pair_items(),
    # ---- ChangePoint shapes
    Item("cp_both_general", CP(T(LIN(0.5, 0.1, 0.7), SE(0.2, 0.8)), P(LIN(0.1, 0.05, 0.4), PER(0.8, 0.3, 0.5)),
                               0.5, 0.01), 1e-2),           # 7 operators; sharp, mid-range
    Item("cp8", _cp8(), 1.2e-2),                            # 17 operators
    # ---- 15 operators: a stationary and a general complete tree of 8 leaves (need 4)
    Item("stat8", balanced(_stationary_leaves(8), [MIXED, SUMS]), 3e-3),
    Item("gen15", P(T(CP(LIN(0.7, 0.1, 0.5), SE(0.1, 0.7), THIRD, 0.05), P(SE(0.3, 0.6), C(0.2))),
                    CP(T(PER(0.9, 0.25, 0.9), LIN(0.2, 0.3, 0.4)), P(GE(0.2, 1.0, 0.5), SE(0.06, 0.4)),
                       1.15, 0.1)), 2e-2),                  # outside the data
    # ---- chains of 13 leaves (25 operators)
    Item("right13", _chain13(True), 1.5e-2),
    Item("left13", _chain13(False), 1.5e-2),
    # ---- the Toeplitz leaf's edge: 16 leaves (31 operators) | 17 (33)
    Item("toep16", balanced(_stationary_leaves(16), [MIXED, SUMS]), 2e-3),
    Item("stat17", P(balanced(_stationary_leaves(16), [SUMS, MIXED, SUMS]), SE(0.33, 0.2)), 4e-3),
    # ---- 63 operators: 32 table slots; register stack 6
    Item("full32", balanced(_stationary_leaves(32), [MIXED, SUMS]), 2.5e-3),
    Item("full32_general", _full32_general(), 3e-2),
]
NAMES = [it.name for it in ZOO]
assert len(set(NAMES)) == len(NAMES)


def program(item):
    ops, par = gp.to_program(item.tree)
    return ops, par, float(item.noise)


PROGRAMS = [program(it) for it in ZOO]
# sorted by operator count (stable): the order of the G-sized / G-toep prefixes
BY_SIZE = sorted(range(len(ZOO)), key=lambda i: len(PROGRAMS[i][0]))
PREFIX_OPS = (1, 3, 7, 15, 31, 63)


def prefixes(idx):
    """the cumulative prefixes of ``idx`` (sorted by size) whose largest tree has <= 1, 3, ... operators"""
    out = []
    for cap in PREFIX_OPS:
        p = [i for i in idx if len(PROGRAMS[i][0]) <= cap]
        if p and (not out or len(p) > len(out[-1])):
            out.append(p)
    return out


# ---- the host's rules, restated -----------------------------------------------------------------------
N_PAR = (0, 1, 3, 2, 3, 3, 0, 0, 2)


def device_order(ops):
    """compile_program's reordering (csrc/ngp_api.hip), restated: need(leaf) = 1, need(node) =
    need + 1 on a tie, else the larger; the child with the larger need goes first (the left one on a
    tie).  Returns (perm, need of the root, [(operator, "swapped" | "left" | "tie")] in device order):
    perm[device parameter index] = caller's parameter index."""
    nodes, stack, pi = [], [], 0
    for op in (int(o) for o in ops):
        nd = dict(op=op, l=None, r=None, p=pi, need=1)
        if op >= 6:
            nd["r"], nd["l"] = stack.pop(), stack.pop()
            a, b = nodes[nd["l"]]["need"], nodes[nd["r"]]["need"]
            nd["need"] = a + 1 if a == b else max(a, b)
        pi += N_PAR[op]
        nodes.append(nd)
        stack.append(len(nodes) - 1)
    perm, orders = [], []

    def emit(k):
        nd = nodes[k]
        if nd["op"] >= 6:
            a, b = nodes[nd["l"]]["need"], nodes[nd["r"]]["need"]
            first, second = (nd["r"], nd["l"]) if b > a else (nd["l"], nd["r"])
            emit(first)
            emit(second)
            orders.append((nd["op"], "swapped" if b > a else "left" if a > b else "tie"))
        perm.extend(range(nd["p"], nd["p"] + N_PAR[nd["op"]]))
    emit(stack[-1])
    return perm, nodes[stack[-1]]["need"], orders


def incidences(ops):
    """{(binary operator, "L" | "R", kind of that operand)} of a program"""
    stack, out = [], set()
    for op in (int(o) for o in ops):
        if op >= 6:
            r, l = stack.pop(), stack.pop()
            out |= {(op, "L", KIND_OF_OP[l]), (op, "R", KIND_OF_OP[r])}
        stack.append(op)
    return out


def changepoints(prog):
    """(location, scale, left is general, right is general, a ChangePoint inside the left child,
    inside the right child) of every ChangePoint, in program order"""
    ops, par = prog[0], prog[1]
    stack, out, pi = [], [], 0
    for op in (int(o) for o in ops):
        if op < 6:
            stack.append((op == 2, False))
        else:
            r, l = stack.pop(), stack.pop()
            if op == 8:
                out.append((par[pi], par[pi + 1], l[0], r[0], l[1], r[1]))
            stack.append((op == 8 or l[0] or r[0], op == 8 or l[1] or r[1]))
        pi += N_PAR[op]
    return out


def n_leaves(ops):
    return int(np.sum(np.asarray(ops) < 6))


def stationary(ops):
    return not np.isin(ops, (2, 8)).any()


def toeplitz_eligible(ops):
    """grad_stage_impl: no Linear, no ChangePoint, at most 16 leaves (31 operators)"""
    return stationary(ops) and len(ops) <= 31


def grad_bucket(n_ops):
    """csrc/ngp_plan.h"""
    return 0 if n_ops <= 1 else 1 if n_ops <= 3 else 2 if n_ops <= 7 else 3 if n_ops <= 15 else \
        4 if n_ops <= 31 else 5


TOEP = [i for i in BY_SIZE if toeplitz_eligible(PROGRAMS[i][0])]
STAT17 = NAMES.index("stat17")


# ---- series, specs, references --------------------------------------------------------------------------
def spec_dict(s):
    return dict(se_form=s[0], periodic_form=s[1], cp_form=s[2], jitter=1e-5)


def ngp_spec(s, precision=0):
    sp = default_spec(precision)
    sp.se_form, sp.periodic_form, sp.cp_form = s
    return sp


def effective_spec(i, s):
    """the spec with the flags of node kinds the item does not hold cleared: the same function, so the
    same (cached) reference — the device still runs under ``s`` itself"""
    ops = PROGRAMS[i][0]
    return tuple(int(f and k in ops) for f, k in zip(s, (3, 5, 8)))


def effective_specs(i, specs):
    out = []
    for s in specs:
        e = effective_spec(i, s)
        if e not in out:
            out.append(e)
    return out


# V-mixed judges these date sets (the refinement does not depend on the forecast dates)
MIXED_SETS = ("beyond", "on_f")

# the cov row: worst |fp64 numpy - long double| / max |K_item| over every item and spec, measured by
# tests/test_grammar_cases_cpu.py (which asserts that it still holds), and the GPU bound from it
COV_WORST_FP64 = 4.41e-15       # 19.9 eps
COV_BOUND = max(8.0 * COV_WORST_FP64, 16 * vc.EPS)


def grad_series(n, lattice):
    # (seeds with an irregular date inside the sharp ChangePoint's transition, 0.5 +- 0.01)
    return vc.series(n, lattice, seed={130: 42, 321: 46}[n])


def value_case(n, lattice, **kw):
    """the zoo as a value_cases.Case: its date sets and its judgement apply unchanged"""
    return vc.Case(n=n, B=len(ZOO), lattice=lattice, seed=50 + n % 7, explicit=tuple(PROGRAMS),
                   extra=tuple(range(len(ZOO))), per_size=False, **kw)


def value_reference(case, i, set_name, s):
    prog, t, y, t_add, y_add, t_new, non = vc.inputs(case, i, set_name)
    return hr.nowcast(prog, t, y, t_add, y_add, t_new, spec_dict(s), noise_on_new=non)


def grad_reference(i, n, lattice, s):
    t, y = grad_series(n, lattice)
    return hr.evaluate(PROGRAMS[i], t, y, spec_dict(s))


def sample321():
    """the items judged against the reference at n = 321 (a long-double gradient there takes seconds):
    first, last, one per bucket, every ChangePoint shape"""
    idx, seen = {BY_SIZE[0], BY_SIZE[-1]}, set()
    for i in BY_SIZE:
        b = grad_bucket(len(PROGRAMS[i][0]))
        if b not in seen:
            seen.add(b)
            idx.add(i)
    idx |= {NAMES.index(k) for k in ("cp_both_general", "cp8", "gen15", "cp_CP_PLUS", "cp_LIN_CP",
                                     "right13")}
    return sorted(idx)


def cov_dates():
    """37 x 53 irregular dates (rectangular) and 40 dates for the square case with the diagonal"""
    rng = np.random.default_rng(77)
    return np.sort(rng.uniform(0, 1, 37)), np.sort(rng.uniform(-0.05, 1.2, 53)), np.sort(rng.uniform(0, 1, 40))


# ---- the zoo as the mock-runtime driver reads it -------------------------------------------------------
def zoo_text():
    lines = []
    for it, (ops, par, nz) in zip(ZOO, PROGRAMS):
        lines.append(f"{it.name} | {' '.join(str(int(o)) for o in ops)} | "
                     f"{' '.join(repr(float(v)) for v in par)} | {nz!r}")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    with open(ZOO_FILE, "w") as f:
        f.write(zoo_text())
    print(f"{len(ZOO)} items -> {ZOO_FILE}")

"""Extended-precision reference of the decomposition conditioned on nowcasts, and of the
sum-of-products terms of a tree (TEST INFRASTRUCTURE ONLY).

A plain restatement of include/ngp.h "sum-of-products terms; the decomposition conditioned on
nowcasts" in ``np.longdouble``, on the approach of tests/component_reference.py: with
t+ = [t; t_add], y+_s = [y; y_add_s], K+ = k(t+, t+) + (noise + jitter) I and X_c = k_c(t*, t+),

    mu_c,s     = X_c (K+)^-1 y+_s
    Sigma_c,c' = delta_cc' k_c(t*, t*) - X_c (K+)^-1 X_c'^T
    logml_s    = -1/2 y+_s' (K+)^-1 y+_s - sum log diag L+ - (n + d)/2 log 2 pi

The terms are restated on the nested tuples of ``oracle_np.rpn_to_tree`` — independent of the
library's ngp_kernel_terms.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle_np
from tests import component_reference as cr
from tests.hp_reference import LD, PI_LD, solve_lower

SPLIT_PLUS, SPLIT_CHANGEPOINT, SPLIT_TIMES = 0, 1, 2
PLUS, TIMES, CP = 6, 7, 8
ZERO = (1, [0.0], None, None)

_CACHE: dict = {}


def term_trees(node, split):
    """the terms of a tree (nested tuples (op, params, left, right)), left to right"""
    op, par, l, r = node
    if op == PLUS:
        return term_trees(l, split) + term_trees(r, split)
    if op == CP and split & SPLIT_CHANGEPOINT:
        return ([(CP, list(par), x, ZERO) for x in term_trees(l, split)]
                + [(CP, list(par), ZERO, y) for y in term_trees(r, split)])
    if op == TIMES and split & SPLIT_TIMES:
        return [(TIMES, [], x, y) for x in term_trees(l, split) for y in term_trees(r, split)]
    return [node]


def terms(program, split):
    """[(ops, params, noise)] of the terms of ``program``"""
    tree = oracle_np.rpn_to_tree(program[0], program[1])
    return [cr.tree_to_program(nd) + (float(program[2]),) for nd in term_trees(tree, split)]


class ComponentNowcastRef:
    """mu [C, D, m], sigma [C m, C m] (row = c m + j), logml_full [D], cond of K+, info"""
    __slots__ = ("mu", "sigma", "logml_full", "cond", "info")


def evaluate(program, comps, t, y, t_add, y_add, t_new, spec=None):
    """The reference of one particle: ``program`` gives K+, ``comps`` the k_c (any kernels).
    Cached on its inputs; computed once and left unchanged."""
    t, y, t_add, t_new = (np.asarray(a, np.float64).reshape(-1) for a in (t, y, t_add, t_new))
    d = t_add.size
    y_add = np.asarray(y_add, np.float64).reshape(-1, d) if d else np.zeros((1, 0))
    sp = oracle_np._spec(spec)
    key = (tuple(map(int, program[0])), tuple(map(float, program[1])), float(program[2]),
           tuple((tuple(map(int, c[0])), tuple(map(float, c[1]))) for c in comps),
           t.tobytes(), y.tobytes(), t_add.tobytes(), y_add.tobytes(), t_new.tobytes(),
           repr(sorted(sp.items())))
    if key in _CACHE:
        return _CACHE[key]
    n, m, C, D = t.size, t_new.size, len(comps), y_add.shape[0]
    tt = np.concatenate([t, t_add])
    r = ComponentNowcastRef()
    L, r.info, r.cond = cr._factor(program, tt, spec, sp)
    if r.info:
        r.mu, r.sigma = np.full((C, D, m), np.nan), np.full((C * m, C * m), np.nan)
        r.logml_full = np.full(D, np.nan)
        _CACHE[key] = r
        return r
    Y = np.concatenate([np.repeat(y.astype(LD)[:, None], D, axis=1), y_add.astype(LD).T], axis=0)
    Z = solve_lower(L, Y)                                                       # [n + d, D]
    r.logml_full = (-np.sum(Z * Z, axis=0) / 2 - np.sum(np.log(np.diag(L)))
                    - LD(n + d) / 2 * np.log(2 * PI_LD))
    X = np.concatenate([cr.cov_ld(c, t_new, tt, spec) for c in comps], axis=0)  # [C m, n + d]
    V = solve_lower(L, X.T)                                                     # [n + d, C m]
    sig = -(V.T @ V)
    for c, prog in enumerate(comps):
        sig[c * m:(c + 1) * m, c * m:(c + 1) * m] += cr.cov_ld(prog, t_new, t_new, spec)
    r.mu = (V.T @ Z).reshape(C, m, D).transpose(0, 2, 1)
    r.sigma = (sig + sig.T) / 2
    _CACHE[key] = r
    return r

"""Extended-precision reference of the additive decomposition (TEST INFRASTRUCTURE ONLY).

A plain restatement of include/ngp.h "additive decomposition" in ``np.longdouble``: for a particle
with kernel k = sum_c k_c, K = k(t, t) + (noise + jitter) I and X_c = k_c(t*, t),

    mu_c       = X_c K^-1 y
    Sigma_c,c' = delta_cc' k_c(t*, t*) - X_c K^-1 X_c'^T

with the dense matrices from ``oracle_np``'s kernel evaluation (of the full tree for K, of each
slice for X_c and the prior blocks) on long double dates, and the solves through the long double
Cholesky of tests/hp_reference.py.  The slicing is restated here too, on the nested tuples of
``oracle_np.rpn_to_tree`` — independent of the library's ngp_kernel_components.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle_np
from tests.hp_reference import LD, cholesky_ld, solve_lower

_CACHE: dict = {}


def split_tree(node):
    """maximal non-Plus subtrees reached from the root through Plus nodes only, left to right"""
    if node[0] == 6:
        return split_tree(node[2]) + split_tree(node[3])
    return [node]


def tree_to_program(node):
    """nested tuples -> (ops, params) in postfix order"""
    ops, params = [], []

    def walk(nd):
        if nd[2] is not None:
            walk(nd[2])
            walk(nd[3])
        ops.append(nd[0])
        params.extend(nd[1])

    walk(node)
    return np.asarray(ops, np.int32), np.asarray(params, np.float64)


def components(program):
    """[(ops, params, noise)] of the components of ``program``"""
    tree = oracle_np.rpn_to_tree(program[0], program[1])
    return [tree_to_program(nd) + (float(program[2]),) for nd in split_tree(tree)]


def cov_ld(program, t1, t2, spec=None):
    """k(t1, t2) of a program in long double (oracle_np's formulas on long double dates)"""
    sp = oracle_np._spec(spec)
    T1 = np.asarray(t1, np.float64).astype(LD)[:, None]
    T2 = np.asarray(t2, np.float64).astype(LD)[None, :]
    K = oracle_np._eval(oracle_np.rpn_to_tree(program[0], program[1]), T1, T2, sp)
    return np.array(np.broadcast_to(K, (T1.shape[0], T2.shape[1])), dtype=LD)


def _factor(program, t, spec, sp):
    """(L, info, cond) of K = k(t, t) + (noise + jitter) I, cached: the date sets queried on one
    series share the factorisation"""
    key = ("factor", tuple(map(int, program[0])), tuple(map(float, program[1])), float(program[2]),
           t.tobytes(), repr(sorted(sp.items())))
    if key not in _CACHE:
        n = t.size
        K = cov_ld(program, t, t, spec)
        K[np.arange(n), np.arange(n)] += LD(program[2]) + LD(sp["jitter"])
        ev = np.linalg.eigvalsh(K.astype(np.float64))
        L, info = cholesky_ld(K)
        _CACHE[key] = (L, info, float(ev[-1] / ev[0]) if ev[0] > 0 else float("inf"))
    return _CACHE[key]


class ComponentRef:
    """mu [C, m], sigma [C m, C m] (row = c m + j), cond of K, info"""
    __slots__ = ("mu", "sigma", "cond", "info")


def evaluate(program, comps, t, y, t_new, spec=None):
    """The reference of one particle: ``program`` gives K, ``comps`` the k_c (any kernels).
    Cached on its inputs; computed once and left unchanged."""
    key = (tuple(map(int, program[0])), tuple(map(float, program[1])), float(program[2]),
           tuple((tuple(map(int, c[0])), tuple(map(float, c[1]))) for c in comps),
           np.asarray(t, np.float64).tobytes(), np.asarray(y, np.float64).tobytes(),
           np.asarray(t_new, np.float64).tobytes(), repr(sorted(oracle_np._spec(spec).items())))
    if key in _CACHE:
        return _CACHE[key]
    sp = oracle_np._spec(spec)
    t, y, t_new = (np.asarray(a, np.float64) for a in (t, y, t_new))
    n, m, C = t.size, t_new.size, len(comps)
    r = ComponentRef()
    L, r.info, r.cond = _factor(program, t, spec, sp)
    if r.info:
        r.mu, r.sigma = np.full((C, m), np.nan), np.full((C * m, C * m), np.nan)
        _CACHE[key] = r
        return r
    z = solve_lower(L, y.astype(LD))
    X = np.concatenate([cov_ld(c, t_new, t, spec) for c in comps], axis=0)     # [C m, n]
    V = solve_lower(L, X.T)                                                     # [n, C m]
    sig = -(V.T @ V)
    for c, prog in enumerate(comps):
        sig[c * m:(c + 1) * m, c * m:(c + 1) * m] += cov_ld(prog, t_new, t_new, spec)
    r.mu = (V.T @ z).reshape(C, m)
    r.sigma = (sig + sig.T) / 2
    _CACHE[key] = r
    return r

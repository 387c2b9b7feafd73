"""Extended-precision references of the long-horizon queries at depth (TEST INFRASTRUCTURE ONLY).

Two additions to tests/hp_reference.py, on its factor cache (``hr._factor_full``: the date sets, the
row sets and the origins of one item share ONE factorisation) and under its rule above
``hr.HP_MAX_N`` points (fp64 LAPACK, ``tol_factor = 2``):

``nowcast_rows``  ``hr.nowcast`` for a horizon too long for its m x m array: the mean and the
                  variance of every date, and the rows ``rows`` of sigma.  Nothing m x m is formed.
``origins``       the forecasts and the evidence of every forecast origin of one series from the
                  factor of the WHOLE series: the leading c x c block of a Cholesky factor is the
                  factor of the first c observations, so with z = L^-1 y and V = L^-1 k(t, t*)

                      mu_c    = sum_{k < c} V_k z_k
                      var_c   = k(t*, t*) - sum_{k < c} V_k^2  (+ noise + jitter)
                      logml_c = sum_{k < c} (-z_k^2 / 2 - log L_kk) - c / 2 log 2 pi

                  are cumulative sums along k.  tests/test_long_depth_cpu.py holds them against
                  ``hr.evaluate`` of each prefix, which factorises the prefix itself.
"""
from __future__ import annotations

import numpy as np
from scipy.linalg import solve_triangular

from oracle.oracle_np import rpn_to_tree
from tests import hp_reference as hr
from tests.hp_reference import LD, PI_LD


class RowsRef:
    """mu [D, m], var [m], sigma_rows [len(rows), m], rows, cond, info, tol_factor"""
    __slots__ = ("mu", "var", "sigma_rows", "rows", "cond", "info", "tol_factor", "n", "d")


class OriginsRef:
    """mu [R, m], var [R, m], logml [R], cuts, cond (of the whole matrix), info, tol_factor"""
    __slots__ = ("mu", "var", "logml", "cuts", "cond", "info", "tol_factor", "n")


def _program(program):
    return (np.asarray(program[0], np.int32), np.asarray(program[1], np.float64), float(program[2]))


def _solver(hp):
    return hr.solve_lower if hp else (lambda A, B: solve_triangular(A, B, lower=True, check_finite=False))


def kdiag(program, t_new, spec=None, dtype=LD):
    """k(t*_i, t*_i) of every date, without the m x m matrix"""
    T = np.asarray(t_new, np.float64).astype(dtype)
    v = hr._value(rpn_to_tree(program[0], program[1]), T, T, hr.spec_tuple(spec), {})
    return np.array(np.broadcast_to(v, T.shape), dtype=dtype)


def nowcast_rows(program, t, y, t_add, y_add, t_new, rows, spec=None, noise_on_new=True):
    program = _program(program)
    t, y = np.asarray(t, np.float64), np.asarray(y, np.float64)
    t_add = np.asarray(t_add, np.float64).reshape(-1)
    n, d = t.size, t_add.size
    y_add = np.asarray(y_add, np.float64).reshape(-1, d) if d else np.zeros((1, 0))
    t_new = np.asarray(t_new, np.float64).reshape(-1)
    rows = np.asarray(rows, np.int64).reshape(-1)
    key = hr._key("nowcast_rows", *program, t, y, t_add, y_add, t_new, rows, hr.spec_tuple(spec),
                  bool(noise_on_new))
    if key in hr._CACHE:
        return hr._CACHE[key]
    sp = hr.spec_tuple(spec)
    tt = np.concatenate([t, t_add])
    L, info, cond, dt = hr._factor_full(program, tt, spec)
    hp = dt is LD
    r = RowsRef()
    r.n, r.d, r.cond, r.info, r.tol_factor, r.rows = n, d, cond, info, 1.0 if hp else 2.0, rows
    D, m = y_add.shape[0], t_new.size
    if info:
        r.mu, r.var = np.full((D, m), np.nan), np.full(m, np.nan)
        r.sigma_rows = np.full((rows.size, m), np.nan)
        hr._CACHE[key] = r
        return r
    solve = _solver(hp)
    Y = np.concatenate([np.repeat(y.astype(dt)[:, None], D, axis=1), y_add.astype(dt).T], axis=0)
    Z = solve(L, Y)                                               # [n + d, D]
    V = solve(L, hr.cov(program, tt, t_new, spec, dtype=dt))      # [n + d, m]
    nz = dt(program[2]) + dt(sp[3]) if noise_on_new else dt(0)
    r.mu = (V.T @ Z).T
    r.var = kdiag(program, t_new, spec, dt) - np.sum(V * V, axis=0) + nz
    sg = hr.cov(program, t_new[rows], t_new, spec, dtype=dt) - V[:, rows].T @ V
    sg[np.arange(rows.size), rows] += nz
    r.sigma_rows = sg
    hr._CACHE[key] = r
    return r


def origins(program, t, y, cuts, t_new, spec=None, noise_on_new=True):
    program = _program(program)
    t, y = np.asarray(t, np.float64), np.asarray(y, np.float64)
    t_new = np.asarray(t_new, np.float64).reshape(-1)
    cuts = np.asarray(cuts, np.int64).reshape(-1)
    n = t.size
    assert cuts.size and cuts.min() >= 1 and cuts.max() <= n
    key = hr._key("origins", *program, t, y, cuts, t_new, hr.spec_tuple(spec), bool(noise_on_new))
    if key in hr._CACHE:
        return hr._CACHE[key]
    sp = hr.spec_tuple(spec)
    L, info, cond, dt = hr._factor_full(program, t, spec)
    hp = dt is LD
    r = OriginsRef()
    r.n, r.cond, r.info, r.tol_factor, r.cuts = n, cond, info, 1.0 if hp else 2.0, cuts
    R, m = cuts.size, t_new.size
    if info:
        r.mu, r.var, r.logml = np.full((R, m), np.nan), np.full((R, m), np.nan), np.full(R, np.nan)
        hr._CACHE[key] = r
        return r
    solve = _solver(hp)
    z = solve(L, y.astype(dt))                                    # [n]
    V = solve(L, hr.cov(program, t, t_new, spec, dtype=dt))       # [n, m]
    nz = dt(program[2]) + dt(sp[3]) if noise_on_new else dt(0)
    at = cuts - 1
    r.mu = np.cumsum(V * z[:, None], axis=0)[at]
    r.var = kdiag(program, t_new, spec, dt)[None, :] - np.cumsum(V * V, axis=0)[at] + nz
    log2pi = np.log(dt(2 * PI_LD if hp else 2 * np.pi))
    r.logml = np.cumsum(-z * z / 2 - np.log(np.diag(L)))[at] - cuts.astype(dt) / 2 * log2pi
    hr._CACHE[key] = r
    return r

"""Extended-precision reference of the GP operations (TEST INFRASTRUCTURE ONLY).

A plain restatement of the covariance, the Cholesky factorisation, logml, alpha, K^-1, the
predictive moments and the logml gradient in ``np.longdouble`` (80-bit extended on x86: eps about
1.1e-19), so that the fp64 kernels are judged against something three decimal digits better than
themselves instead of against another fp64 implementation.  Nothing but the RPN tree decoding (the
grammar, no arithmetic) comes from ``oracle/``.

The gradient is formed in forward mode, one dK/dtheta_i at a time, and the same pass gives every
component's scale

    s_i = 1/2 (|alpha|' |dK_i| |alpha| + sum |K^-1| o |dK_i|),

the size of the terms the component is summed from: an fp64 evaluation of component i carries an
error of about eps cond(K) s_i, however small g_i itself is after cancellation.  That is what
``tests.util.check_components`` judges against.

Numpy's long double has no LAPACK: the factorisation is a left-looking column loop with vectorised
column updates, O(n^3) in C loops of numpy, a second or two at n = 1,000.  Above ``HP_MAX_N`` the
same formulas run in fp64 on LAPACK and the result says so (``tol_factor = 2``: the reference is
then only as good as what it judges).
"""
from __future__ import annotations

import hashlib

import numpy as np
from scipy.linalg import cholesky, solve_triangular

from oracle.oracle_np import rpn_to_tree

LD = np.longdouble
PI_LD = 4 * np.arctan(LD(1))
EPS_LD = float(np.finfo(LD).eps)
HP_MAX_N = 1100

_CACHE: dict = {}


def spec_tuple(spec):
    """(se_form, periodic_form, cp_form, jitter) from an NgpSpec, a dict or None (the defaults)."""
    if spec is None:
        return (0, 0, 0, 1e-5)
    if isinstance(spec, dict):
        return (int(spec.get("se_form", 0)), int(spec.get("periodic_form", 0)),
                int(spec.get("cp_form", 0)), float(spec.get("jitter", 1e-5)))
    return (int(spec.se_form), int(spec.periodic_form), int(spec.cp_form), float(spec.jitter))


# ---- covariance and its parameter derivatives ----------------------------------------------------
def _sig(node, T1, T2, cp_form):
    loc, sc = (T1.dtype.type(v) for v in node[1])
    sgn = -1 if cp_form else 1
    u1, u2 = sgn * (loc - T1) / sc, sgn * (loc - T2) / sc
    return u1, u2, (1 + np.tanh(u1)) / 2, (1 + np.tanh(u2)) / 2


def _leaf(node, T1, T2, sp, want_d):
    """value of a leaf and (want_d) the derivatives by its own parameters, in order"""
    dt = T1.dtype.type
    op, pr = node[0], [dt(v) for v in node[1]]
    se_form, per_form = sp[0], sp[1]
    if op == 1:
        v = np.full(np.broadcast(T1, T2).shape, pr[0], dtype=dt)
        return v, ([np.ones_like(v)] if want_d else None)
    if op == 2:
        c, bias, amp = pr
        u, w = T1 - c, T2 - c
        v = bias + amp * u * w
        return v, ([-amp * (u + w), np.ones_like(v), u * w] if want_d else None)
    d = np.abs(T1 - T2)
    if op == 3:
        ls, amp = pr
        den = ls if se_form else ls * ls
        e = np.exp(-d * d / (2 * den))
        dden = dt(1) if se_form else 2 * ls
        return amp * e, ([amp * e * d * d / (2 * den * den) * dden, e] if want_d else None)
    if op == 4:
        ls, gam, amp = pr
        q = d / ls
        pw = np.power(q, gam)
        e = np.exp(-pw)
        if not want_d:
            return amp * e, None
        lq = np.log(np.where(q > 0, q, dt(1)))
        return amp * e, [amp * e * pw * gam / ls, -amp * e * pw * lq, e]
    if op == 5:
        ls, per, amp = pr
        c = 2 / ls if per_form else 2 / (ls * ls)
        dc = -2 / (ls * ls) if per_form else -4 / (ls * ls * ls)
        arg = dt(PI_LD) * d / per
        sn = np.sin(arg)
        e = np.exp(-c * sn * sn)
        if not want_d:
            return amp * e, None
        return amp * e, [-amp * e * sn * sn * dc, amp * e * c * 2 * sn * np.cos(arg) * arg / per, e]
    raise ValueError(op)


def _value(node, T1, T2, sp, memo):
    key = id(node)
    if key in memo:
        return memo[key]
    op, _, l, r = node
    if op <= 5:
        v = _leaf(node, T1, T2, sp, False)[0]
    elif op == 6:
        v = _value(l, T1, T2, sp, memo) + _value(r, T1, T2, sp, memo)
    elif op == 7:
        v = _value(l, T1, T2, sp, memo) * _value(r, T1, T2, sp, memo)
    else:
        _, _, s1, s2 = _sig(node, T1, T2, sp[2])
        v = s1 * s2 * _value(l, T1, T2, sp, memo) + (1 - s1) * (1 - s2) * _value(r, T1, T2, sp, memo)
    memo[key] = v
    return v


def _derivs(node, T1, T2, sp, memo, M):
    """dK/dtheta for every parameter of the subtree in RPN order (a generator: one matrix at a
    time), M the product of the factors between the subtree and the root (None: 1)"""
    op, _, l, r = node

    def mul(a, b):
        return b if a is None else a * b

    if op <= 5:
        for dv in _leaf(node, T1, T2, sp, True)[1]:
            yield mul(M, dv)
    elif op == 6:
        yield from _derivs(l, T1, T2, sp, memo, M)
        yield from _derivs(r, T1, T2, sp, memo, M)
    elif op == 7:
        yield from _derivs(l, T1, T2, sp, memo, mul(M, _value(r, T1, T2, sp, memo)))
        yield from _derivs(r, T1, T2, sp, memo, mul(M, _value(l, T1, T2, sp, memo)))
    else:
        u1, u2, s1, s2 = _sig(node, T1, T2, sp[2])
        yield from _derivs(l, T1, T2, sp, memo, mul(M, s1 * s2))
        yield from _derivs(r, T1, T2, sp, memo, mul(M, (1 - s1) * (1 - s2)))
        vl, vr = _value(l, T1, T2, sp, memo), _value(r, T1, T2, sp, memo)
        sgn = -1 if sp[2] else 1
        sc = T1.dtype.type(node[1][1])
        ds1, ds2 = 2 * s1 * (1 - s1), 2 * s2 * (1 - s2)          # d s / d u
        g1, g2 = vl * s2 - vr * (1 - s2), vl * s1 - vr * (1 - s1)  # d value / d s1, d s2
        yield mul(M, (g1 * ds1 + g2 * ds2) * (sgn / sc))
        yield mul(M, g1 * ds1 * (-u1 / sc) + g2 * ds2 * (-u2 / sc))


def cov(program, t1, t2, spec=None, add_diag=False, dtype=LD):
    ops, params, noise = program
    sp = spec_tuple(spec)
    T1 = np.asarray(t1, dtype=np.float64).astype(dtype)[:, None]
    T2 = np.asarray(t2, dtype=np.float64).astype(dtype)[None, :]
    K = _value(rpn_to_tree(ops, params), T1, T2, sp, {}).astype(dtype)
    K = np.array(np.broadcast_to(K, (T1.shape[0], T2.shape[1])), dtype=dtype)
    if add_diag:
        k = min(K.shape)
        K[np.arange(k), np.arange(k)] += dtype(noise) + dtype(sp[3])
    return K


# ---- factorisation and solves ------------------------------------------------------------------
def cholesky_ld(A, pivots=False):
    """lower L with L L' = A, column by column (left-looking); (L, info), info = k > 0 when the
    k-th leading minor is not positive.  pivots=True: (L, info, piv) with piv[j] the Schur pivot
    a_jj - sum_k l_jk^2 of every column reached, the non-positive one (piv[info - 1]) included"""
    n = A.shape[0]
    L = np.zeros_like(A)
    piv = np.zeros(n, dtype=A.dtype)
    for j in range(n):
        col = A[j:, j] - L[j:, :j] @ L[j, :j]
        piv[j] = col[0]
        if not (col[0] > 0) or not np.isfinite(col[0]):
            return (None, j + 1, piv[:j + 1]) if pivots else (None, j + 1)
        d = np.sqrt(col[0])
        L[j, j] = d
        L[j + 1:, j] = col[1:] / d
    return (L, 0, piv) if pivots else (L, 0)


def solve_lower(L, B):
    """L X = B by forward substitution (B a vector or a matrix of columns)"""
    X = np.array(B, dtype=L.dtype)
    for j in range(L.shape[0]):
        X[j] = (X[j] - L[j, :j] @ X[:j]) / L[j, j]
    return X


def solve_upper_t(L, B):
    """L' X = B by back substitution"""
    X = np.array(B, dtype=L.dtype)
    for j in range(L.shape[0] - 1, -1, -1):
        X[j] = (X[j] - L[j + 1:, j] @ X[j + 1:]) / L[j, j]
    return X


class Ref:
    """logml, alpha, K^-1 (and gradient + scales, predictive) of one item"""
    # (kept in the precision they were computed in: np.longdouble up to HP_MAX_N points)
    __slots__ = ("logml", "alpha", "kinv", "grad", "scale", "mu", "sigma", "cond", "info",
                 "tol_factor", "n")


def _key(*parts):
    h = hashlib.sha1()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes() if isinstance(p, np.ndarray) else repr(p).encode())
    return h.hexdigest()


def evaluate(program, t, y, spec=None, grad=True, t_new=None, noise_on_new=True):
    """the reference of one item (cached on its inputs: an item is never computed twice in a run)"""
    ops, params, noise = program
    ops = np.asarray(ops, np.int32)
    params = np.asarray(params, np.float64)
    t = np.asarray(t, np.float64)
    y = np.asarray(y, np.float64)
    tn = None if t_new is None else np.asarray(t_new, np.float64)
    key = _key(ops, params, float(noise), t, y, spec_tuple(spec), bool(grad),
               tn if tn is not None else "-", bool(noise_on_new))
    if key in _CACHE:
        return _CACHE[key]
    r = _evaluate((ops, params, float(noise)), t, y, spec, grad, tn, noise_on_new)
    _CACHE[key] = r
    return r


def _evaluate(program, t, y, spec, want_grad, t_new, noise_on_new):
    n = t.size
    hp = n <= HP_MAX_N
    dt = LD if hp else np.float64
    sp = spec_tuple(spec)
    r = Ref()
    r.n, r.tol_factor = n, 1.0 if hp else 2.0
    K = cov(program, t, t, spec, add_diag=True, dtype=dt)
    ev = np.linalg.eigvalsh(K.astype(np.float64))
    r.cond = float(ev[-1] / ev[0]) if ev[0] > 0 else float("inf")
    if hp:
        L, r.info = cholesky_ld(K)
    else:
        try:
            L, r.info = cholesky(K, lower=True, check_finite=False), 0
        except np.linalg.LinAlgError:
            L, r.info = None, 1
    if r.info:
        r.logml = float("nan")
        return r
    yy = y.astype(dt)
    if hp:
        z = solve_lower(L, yy)
        alpha = solve_upper_t(L, z)
        W = solve_lower(L, np.eye(n, dtype=dt))               # L^-1
    else:
        z = solve_triangular(L, yy, lower=True, check_finite=False)
        alpha = solve_triangular(L, z, lower=True, trans="T", check_finite=False)
        W = solve_triangular(L, np.eye(n), lower=True, check_finite=False)
    two_pi = 2 * PI_LD if hp else 2 * np.pi
    lm = -(z @ z) / 2 - np.sum(np.log(np.diag(L))) - dt(n) / 2 * np.log(dt(two_pi))
    r.logml, r.alpha = lm, alpha
    r.kinv = W.T @ W
    if want_grad:
        T1, T2 = t.astype(dt)[:, None], t.astype(dt)[None, :]
        memo = {}
        tree = rpn_to_tree(program[0], program[1])
        aa, ak = np.abs(alpha), np.abs(r.kinv)
        g, s = [], []
        for dK in _derivs(tree, T1, T2, sp, memo, None):
            dK = np.broadcast_to(dK, (n, n))
            g.append((alpha @ dK @ alpha - np.sum(r.kinv * dK)) / 2)
            s.append((aa @ np.abs(dK) @ aa + np.sum(ak * np.abs(dK))) / 2)
        g.append((alpha @ alpha - np.trace(r.kinv)) / 2)       # noise: dK = I
        s.append((aa @ aa + np.trace(ak)) / 2)
        r.grad = np.array(g, dtype=dt)
        r.scale = np.array(s, dtype=dt)
    if t_new is not None:
        K21 = cov(program, t_new, t, spec, dtype=dt)
        K22 = cov(program, t_new, t_new, spec, dtype=dt)
        V = W @ K21.T
        sig = K22 - V.T @ V
        sig = (sig + sig.T) / 2
        if noise_on_new:
            m = t_new.size
            sig[np.arange(m), np.arange(m)] += dt(program[2]) + dt(sp[3])
        r.mu, r.sigma = K21 @ alpha, sig
    return r


class NowcastRef:
    """the nowcast fan-out of one item: logml_base, logml_full [D], mu [D, m], sigma [m, m]"""
    __slots__ = ("logml_base", "logml_full", "mu", "sigma", "cond", "info", "tol_factor", "n", "d")


def _factor_full(program, tt, spec):
    """(L, info, cond, dtype) of the matrix on the dates tt, cached: the forecast-date sets of one
    item share it"""
    key = _key("factor", program[0], program[1], float(program[2]), tt, spec_tuple(spec))
    if key in _CACHE:
        return _CACHE[key]
    hp = tt.size <= HP_MAX_N
    dt = LD if hp else np.float64
    K = cov(program, tt, tt, spec, add_diag=True, dtype=dt)
    ev = np.linalg.eigvalsh(K.astype(np.float64))
    cond = float(ev[-1] / ev[0]) if ev[0] > 0 else float("inf")
    if hp:
        L, info = cholesky_ld(K)
    else:
        try:
            L, info = cholesky(K, lower=True, check_finite=False), 0
        except np.linalg.LinAlgError as e:
            msg = str(e)
            L, info = None, (int(msg.split("-th")[0].split()[-1]) if "-th" in msg else 1)
    _CACHE[key] = (L, info, cond, dt)
    return _CACHE[key]


def nowcast(program, t, y, t_add, y_add, t_new, spec=None, noise_on_new=True):
    """The reference of ``ngp_nowcast_batch`` for one item (cached on its inputs).  The matrix on
    the n + d dates (t, t_add) is factorised ONCE; its leading n-block is the factor of the base
    matrix, so logml_base comes from the first n rows of the same factor and of the same forward
    solve.  cond is that of the (n + d) matrix; above HP_MAX_N points fp64 LAPACK, tol_factor 2."""
    ops = np.asarray(program[0], np.int32)
    params = np.asarray(program[1], np.float64)
    program = (ops, params, float(program[2]))
    t, y = np.asarray(t, np.float64), np.asarray(y, np.float64)
    t_add = np.asarray(t_add, np.float64).reshape(-1)
    n, d = t.size, t_add.size
    y_add = np.asarray(y_add, np.float64).reshape(-1, d) if d else np.zeros((1, 0))
    t_new = np.asarray(t_new, np.float64).reshape(-1)
    key = _key("nowcast", ops, params, program[2], t, y, t_add, y_add, t_new, spec_tuple(spec),
               bool(noise_on_new))
    if key in _CACHE:
        return _CACHE[key]
    sp = spec_tuple(spec)
    tt = np.concatenate([t, t_add])
    L, info, cond, dt = _factor_full(program, tt, spec)
    hp = dt is LD
    r = NowcastRef()
    r.n, r.d, r.cond, r.info, r.tol_factor = n, d, cond, info, 1.0 if hp else 2.0
    D, m = y_add.shape[0], t_new.size
    if info:
        r.logml_base = float("nan")
        r.logml_full = np.full(D, np.nan)
        r.mu, r.sigma = np.full((D, m), np.nan), np.full((m, m), np.nan)
        _CACHE[key] = r
        return r
    solve = solve_lower if hp else (lambda A, B: solve_triangular(A, B, lower=True, check_finite=False))
    log2pi = np.log(dt(2 * PI_LD if hp else 2 * np.pi))
    ldiag = np.log(np.diag(L))
    # one right-hand side per scenario: they share their first n rows
    Y = np.concatenate([np.repeat(y.astype(dt)[:, None], D, axis=1), y_add.astype(dt).T], axis=0)
    Z = solve(L, Y)                                               # [n + d, D]
    r.logml_base = -(Z[:n, 0] @ Z[:n, 0]) / 2 - np.sum(ldiag[:n]) - dt(n) / 2 * log2pi
    r.logml_full = -np.sum(Z * Z, axis=0) / 2 - np.sum(ldiag) - dt(n + d) / 2 * log2pi
    K21 = cov(program, t_new, tt, spec, dtype=dt)
    K22 = cov(program, t_new, t_new, spec, dtype=dt)
    V = solve(L, K21.T)                                           # [n + d, m]
    sig = K22 - V.T @ V
    sig = (sig + sig.T) / 2
    if noise_on_new:
        sig[np.arange(m), np.arange(m)] += dt(program[2]) + dt(sp[3])
    r.mu, r.sigma = (V.T @ Z).T, sig                              # mu_s = K21 K^-1 y_s = V' z_s
    _CACHE[key] = r
    return r


def pred_scales(sigma_ref):
    """the yardsticks of predictive outputs: sqrt(s_aa) for mu_a, sqrt(s_aa s_bb) for s_ab"""
    d = np.sqrt(np.abs(np.diag(np.asarray(sigma_ref, np.float64))))
    return d, np.outer(d, d)

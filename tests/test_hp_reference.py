"""The extended-precision reference (tests/hp_reference.py) and the componentwise judgement built on
it (tests/util.check_components): against mpmath at 40 digits on small cases of every node type and
spec flag, against the two fp64 oracles at n = 200, and a sensitivity check — a perturbation of
1e-6 in a small gradient component or a small predictive variance that the normwise ``check``
accepts must be rejected componentwise.  CPU only."""
import mpmath as mp
import numpy as np
import pytest

from oracle import oracle_c, oracle_np
from oracle.oracle_np import rpn_to_tree
from tests import hp_reference as hr
from tests.util import EPS, TOL_PRED, check_components, nerr
from tests.util import tol as tol_of

LD = np.longdouble

# every node type: Const 1, Linear 2, SE 3, GammaExp 4, Periodic 5, Plus 6, Times 7, ChangePoint 8
PROGRAMS = {
    "se+per*lin": ([3, 5, 2, 7, 6], [3.0, 1.5, 1.2, 4.0, 0.8, 5.0, 0.1, 0.02], 0.05),
    "cp(ge,const)": ([4, 1, 8], [2.0, 1.4, 0.7, 0.3, 6.0, 1.5], 0.02),
    "se*per+cp(lin,se)": ([3, 5, 7, 2, 3, 8, 6],
                          [2.5, 1.1, 1.0, 3.0, 0.9, 4.0, 0.2, 0.05, 1.5, 0.6, 5.0, 2.0], 0.03),
}
SPECS = {"forms0": dict(se_form=0, periodic_form=0, cp_form=0, jitter=1e-5),
         "forms1": dict(se_form=1, periodic_form=1, cp_form=1, jitter=1e-4)}


def _prog(name):
    ops, params, noise = PROGRAMS[name]
    return np.array(ops, np.int32), np.array(params, float), noise


def _series(n, seed):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0.0, 12.0, n))
    y = np.sin(t) + 0.3 * t + 0.1 * rng.standard_normal(n)
    return t, y


# ---- an mpmath restatement (scalar, 40 digits): the gradient by central differences ----------
def _mp_k(node, a, b, sp):
    op, pr, l, r = node
    pr = [mp.mpf(v) for v in pr]
    d = abs(a - b)
    if op == 1:
        return pr[0]
    if op == 2:
        return pr[1] + pr[2] * (a - pr[0]) * (b - pr[0])
    if op == 3:
        den = pr[0] if sp["se_form"] else pr[0] ** 2
        return pr[1] * mp.exp(-d * d / (2 * den))
    if op == 4:
        return pr[2] * mp.exp(-(d / pr[0]) ** pr[1]) if d > 0 else pr[2]
    if op == 5:
        c = 2 / pr[0] if sp["periodic_form"] else 2 / pr[0] ** 2
        return pr[2] * mp.exp(-c * mp.sin(mp.pi * d / pr[1]) ** 2)
    if op == 6:
        return _mp_k(l, a, b, sp) + _mp_k(r, a, b, sp)
    if op == 7:
        return _mp_k(l, a, b, sp) * _mp_k(r, a, b, sp)
    sgn = -1 if sp["cp_form"] else 1
    s1 = (1 + mp.tanh(sgn * (pr[0] - a) / pr[1])) / 2
    s2 = (1 + mp.tanh(sgn * (pr[0] - b) / pr[1])) / 2
    return s1 * s2 * _mp_k(l, a, b, sp) + (1 - s1) * (1 - s2) * _mp_k(r, a, b, sp)


def _mp_K(ops, params, noise, t1, t2, sp, diag):
    tree = rpn_to_tree(ops, params)
    K = mp.matrix(len(t1), len(t2))
    for i, a in enumerate(t1):
        for j, b in enumerate(t2):
            K[i, j] = _mp_k(tree, mp.mpf(a), mp.mpf(b), sp)
    if diag:
        for i in range(len(t1)):
            K[i, i] += mp.mpf(noise) + mp.mpf(sp["jitter"])
    return K


def _mp_logml(ops, params, noise, t, y, sp):
    K = _mp_K(ops, params, noise, t, t, sp, True)
    L = mp.cholesky(K)
    z = mp.lu_solve(L, mp.matrix([mp.mpf(v) for v in y]))
    n = len(t)
    return (-sum(z[i] ** 2 for i in range(n)) / 2 - sum(mp.log(L[i, i]) for i in range(n))
            - n * mp.log(2 * mp.pi) / 2), K


def _ld(x):
    return LD(mp.nstr(x, 30))


@pytest.mark.parametrize("spec", list(SPECS))
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_reference_matches_mpmath(name, spec):
    mp.mp.dps = 40
    sp = SPECS[spec]
    ops, params, noise = _prog(name)
    t, y = _series(10, seed=len(name))
    t_new = np.array([12.5, 14.0])
    r = hr.evaluate((ops, params, noise), t, y, sp, t_new=t_new, noise_on_new=True)
    assert r.info == 0
    tol = 50 * hr.EPS_LD * r.cond
    lm, K = _mp_logml(ops, params, noise, t, y, sp)
    assert abs(r.logml - _ld(lm)) <= tol * max(abs(r.logml), 1), (r.logml, lm)
    yv = mp.matrix([mp.mpf(v) for v in y])
    alpha = mp.cholesky_solve(K, yv)
    a_mp = np.array([_ld(alpha[i]) for i in range(len(t))])
    assert np.max(np.abs(r.alpha - a_mp)) <= tol * np.max(np.abs(a_mp))
    # predictive moments
    K21 = _mp_K(ops, params, noise, t_new, t, sp, False)
    K22 = _mp_K(ops, params, noise, t_new, t_new, sp, False)
    mu = K21 * alpha
    V = mp.matrix(len(t), len(t_new))
    for j in range(len(t_new)):
        col = mp.cholesky_solve(K, mp.matrix([K21[j, i] for i in range(len(t))]))
        for i in range(len(t)):
            V[i, j] = col[i]
    S = K22 - K21 * V
    for j in range(len(t_new)):
        S[j, j] += mp.mpf(noise) + mp.mpf(sp["jitter"])
    m = len(t_new)
    mu_mp = np.array([_ld(mu[a]) for a in range(m)])
    S_mp = np.array([[_ld(S[a, b]) for b in range(m)] for a in range(m)])
    d = np.sqrt(np.diag(S_mp))
    assert np.all(np.abs(r.mu - mu_mp) <= tol * d)
    assert np.all(np.abs(r.sigma - S_mp) <= tol * np.outer(d, d))
    # gradient: central differences of the 40-digit logml (error ~ h^2: far below the test)
    g_mp = []
    for j in range(params.size + 1):
        def f(delta):
            p = [mp.mpf(v) for v in params]
            nz = mp.mpf(noise)
            if j < params.size:
                p[j] += delta
            else:
                nz += delta
            return _mp_logml_p(ops, p, nz, t, y, sp)
        h = mp.mpf("1e-15") * max(abs(params[j]) if j < params.size else noise, 1e-3)
        g_mp.append((f(h) - f(-h)) / (2 * h))
    g_mp = np.array([_ld(v) for v in g_mp])
    assert r.grad.shape == g_mp.shape
    assert np.all(np.abs(r.grad - g_mp) <= tol * r.scale), (r.grad, g_mp, r.scale)


def _mp_logml_p(ops, p, nz, t, y, sp):
    """logml at mp-valued parameters (no rounding of the perturbed parameters to fp64)"""
    tree = _mp_tree(ops, p)
    n = len(t)
    K = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            K[i, j] = _mp_k(tree, mp.mpf(t[i]), mp.mpf(t[j]), sp)
        K[i, i] += nz + mp.mpf(sp["jitter"])
    L = mp.cholesky(K)
    z = mp.lu_solve(L, mp.matrix([mp.mpf(v) for v in y]))
    return (-sum(z[i] ** 2 for i in range(n)) / 2 - sum(mp.log(L[i, i]) for i in range(n))
            - n * mp.log(2 * mp.pi) / 2)


def _mp_tree(ops, p):
    """rpn_to_tree with the parameters kept as mpf"""
    counts = {1: 1, 2: 3, 3: 2, 4: 3, 5: 3}
    stack, k = [], 0
    for op in ops:
        op = int(op)
        if op in counts:
            stack.append((op, tuple(p[k:k + counts[op]]), None, None))
            k += counts[op]
        else:
            r, l = stack.pop(), stack.pop()
            np_ = 2 if op == 8 else 0
            stack.append((op, tuple(p[k:k + np_]), l, r))
            k += np_
    return stack[0]


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_reference_matches_the_fp64_oracles(name):
    ops, params, noise = _prog(name)
    t, y = _series(200, seed=3)
    t = t * 20.0                                  # 200 points over 240 days
    prog = (ops, params, noise)
    r = hr.evaluate(prog, t, y, None, t_new=t[-4:] + 3.0)
    assert r.info == 0
    tol = 50 * EPS * r.cond
    lm_np, g_np, _ = oracle_np.logml_grad(prog, t, y)
    lm_c, g_c, _ = oracle_c.logml_grad(prog, t, y)
    mu, sg, _, _ = oracle_np.predict(prog, t, y, t[-4:] + 3.0)
    for lm in (lm_np, lm_c):
        assert abs(lm - float(r.logml)) <= tol * abs(float(r.logml))
    check_components("hp reference vs fp64 oracle: gradient (numpy)", g_np, r.grad, r.scale, 1e-12, r.cond)
    check_components("hp reference vs fp64 oracle: gradient (C)", g_c, r.grad, r.scale, 1e-12, r.cond)
    d, dd = hr.pred_scales(r.sigma)
    check_components("hp reference vs fp64 oracle: mean", mu, r.mu, d, 1e-12, r.cond)
    check_components("hp reference vs fp64 oracle: covariance", sg, r.sigma, dd, 1e-12, r.cond)


def test_componentwise_check_rejects_what_the_normwise_check_accepts():
    # a gradient whose largest component (the noise derivative of a near-noiseless fit) is over
    # 1e4 x a small one that is not itself the result of cancellation (|g_i| >= 1e-2 s_i)
    ops, params, _ = _prog("cp(ge,const)")
    t, y = _series(60, seed=9)
    r = hr.evaluate((ops, params, 1e-4), t, y, None)
    g = np.asarray(r.grad, float)
    s = np.asarray(r.scale, float)
    small = int(np.argmin(np.where(np.abs(g) >= 1e-2 * s, np.abs(g), np.inf)))
    assert np.max(np.abs(g)) >= 1e4 * np.abs(g[small]), g
    bad = g.copy()
    bad[small] *= 1 + 1e-6
    # (what ``check(..., 1e-7)`` asserts, unrecorded: this is a test of the judgement itself)
    assert nerr(bad, g) < tol_of(1e-7)
    with pytest.raises(AssertionError):
        check_components("sensitivity: componentwise gradient", bad, g, s, 1e-9, r.cond, record=False)
    # the smallest predictive variance (a forecast date on an observed one, no noise added)
    # against the largest (a date far from the data, where the linear factor grows)
    ops, params, _ = _prog("se+per*lin")
    r = hr.evaluate((ops, params, 1e-4), t, y, None, t_new=np.array([t[5], t[30], 40.0]),
                    noise_on_new=False)
    sg = np.asarray(r.sigma, float)
    a = int(np.argmin(np.diag(sg)))
    assert np.max(np.diag(sg)) >= 1e3 * sg[a, a], np.diag(sg)
    bad = sg.copy()
    bad[a, a] *= 1 + 1e-6
    assert nerr(bad, sg) < tol_of(TOL_PRED)
    _, dd = hr.pred_scales(sg)
    with pytest.raises(AssertionError):
        check_components("sensitivity: componentwise covariance", bad, sg, dd, TOL_PRED, r.cond,
                         record=False)


# ---- the nowcast fan-out ----------------------------------------------------------------------------
def _nowcast_case(n, seed):
    t, y = _series(n + 2, seed)
    rng = np.random.default_rng(seed + 100)
    y_add = y[n:][None, :] + 0.2 * rng.standard_normal((2, 2))
    # a date between two training dates, one on an observed date, one beyond the last
    t_new = np.array([(t[3] + t[4]) / 2, t[6], t[-1] + 1.5])
    return t[:n], y[:n], t[n:], y_add, t_new


@pytest.mark.parametrize("spec", list(SPECS))
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_nowcast_reference_matches_mpmath(name, spec):
    """10 points, d = 2 appended, D = 2 scenarios, against 40 digits"""
    mp.mp.dps = 40
    sp = SPECS[spec]
    ops, params, noise = _prog(name)
    t, y, t_add, y_add, t_new = _nowcast_case(10, seed=len(name))
    r = hr.nowcast((ops, params, noise), t, y, t_add, y_add, t_new, sp, noise_on_new=True)
    assert r.info == 0 and r.tol_factor == 1.0
    tol = 50 * hr.EPS_LD * r.cond
    lb, _ = _mp_logml(ops, params, noise, t, y, sp)
    assert abs(r.logml_base - _ld(lb)) <= tol * max(abs(r.logml_base), 1)
    tt = np.concatenate([t, t_add])
    K = _mp_K(ops, params, noise, tt, tt, sp, True)
    K21 = _mp_K(ops, params, noise, t_new, tt, sp, False)
    K22 = _mp_K(ops, params, noise, t_new, t_new, sp, False)
    m = len(t_new)
    S = K22 - K21 * mp.inverse(K) * K21.T
    for j in range(m):
        S[j, j] += mp.mpf(noise) + mp.mpf(sp["jitter"])
    S_mp = np.array([[_ld(S[a, b]) for b in range(m)] for a in range(m)])
    d = np.sqrt(np.diag(S_mp))
    assert np.all(np.abs(r.sigma - S_mp) <= tol * np.outer(d, d))
    for s in range(2):
        yy = np.concatenate([y, y_add[s]])
        lf, _ = _mp_logml(ops, params, noise, tt, yy, sp)
        assert abs(r.logml_full[s] - _ld(lf)) <= tol * max(abs(r.logml_full[s]), 1)
        mu = K21 * mp.cholesky_solve(K, mp.matrix([mp.mpf(v) for v in yy]))
        mu_mp = np.array([_ld(mu[a]) for a in range(m)])
        assert np.all(np.abs(r.mu[s] - mu_mp) <= tol * d), (s, r.mu[s], mu_mp)


@pytest.mark.parametrize("non", [True, False])
@pytest.mark.parametrize("name", list(PROGRAMS))
def test_nowcast_reference_matches_the_fp64_oracle_and_evaluate(name, non):
    ops, params, noise = _prog(name)
    prog = (ops, params, noise)
    t, y, t_add, y_add, t_new = _nowcast_case(200, seed=3)
    r = hr.nowcast(prog, t, y, t_add, y_add, t_new, None, noise_on_new=non)
    assert r.info == 0
    assert hr.nowcast(prog, t, y, t_add, y_add, t_new, None, noise_on_new=non) is r      # cached
    # oracle_np.nowcast: one refactorisation per scenario, in fp64
    lb, lf, mu, sg, info = oracle_np.nowcast(prog, t, y, t_add, y_add, t_new, non)
    assert info == 0
    tol = 50 * EPS * r.cond
    assert abs(lb - float(r.logml_base)) <= tol * abs(float(r.logml_base))
    assert np.all(np.abs(lf - r.logml_full.astype(float)) <= tol * np.abs(lf))
    d, dd = hr.pred_scales(r.sigma)
    for s in range(2):
        check_components("hp nowcast vs fp64 oracle: mean", mu[s], r.mu[s], d, 1e-12, r.cond)
    check_components("hp nowcast vs fp64 oracle: covariance", sg, r.sigma, dd, 1e-12, r.cond)
    # evaluate on the concatenated series, scenario by scenario, and on the base series: the same
    # arithmetic in the same precision, so agreement to long-double rounding
    tol = 50 * hr.EPS_LD * r.cond
    tt = np.concatenate([t, t_add])
    e0 = hr.evaluate(prog, t, y, None, grad=False)
    assert abs(e0.logml - r.logml_base) <= tol * abs(e0.logml)
    for s in range(2):
        e = hr.evaluate(prog, tt, np.concatenate([y, y_add[s]]), None, grad=False, t_new=t_new,
                        noise_on_new=non)
        assert abs(e.logml - r.logml_full[s]) <= tol * abs(e.logml)
        assert np.all(np.abs(e.mu - r.mu[s]) <= tol * d)
        assert np.all(np.abs(e.sigma - r.sigma) <= tol * dd)
        assert e.cond == r.cond


def test_reference_pivots_include_the_non_positive_one():
    A = np.array([[4.0, 2.0, 2.0], [2.0, 2.0, 1.0], [2.0, 1.0, 0.5]]).astype(LD)
    L, info, piv = hr.cholesky_ld(A, pivots=True)
    # pivots 4, 2 - 1 = 1, 0.5 - 1 - 0 = -0.5
    assert L is None and info == 3 and np.allclose(piv.astype(float), [4.0, 1.0, -0.5])
    assert hr.cholesky_ld(A)[1] == 3
    L, info, piv = hr.cholesky_ld(A[:2, :2], pivots=True)
    assert info == 0 and np.allclose(piv.astype(float), [4.0, 1.0]) and np.allclose(
        (L @ L.T).astype(float), A[:2, :2].astype(float))


def test_reference_reports_an_indefinite_matrix_and_caches():
    t = np.array([0.0, 1.0, 2.0])
    prog = (np.array([1], np.int32), np.array([-5.0]), 0.0)    # a negative constant kernel
    r = hr.evaluate(prog, t, np.ones(3), dict(jitter=0.0))
    assert r.info == 1 and np.isnan(float(r.logml))
    ops, params, noise = _prog("cp(ge,const)")
    a = hr.evaluate((ops, params, noise), *_series(30, 1))
    assert hr.evaluate((ops, params, noise), *_series(30, 1)) is a

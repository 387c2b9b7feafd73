"""Admissibility of the deep long-horizon cases (tests/long_depth_cases.py), on the CPU.

1. Fairness (the rule of tests/test_date_cases_cpu.py).  For every case that
   tests/test_long_depth_gpu.py judges, the plain fp64 oracle is judged by the same call against the
   same reference and must pass at A QUARTER of the tolerance; for the origins this is the oracle run
   on every prefix.  The oracle is ``OracleEngine`` (oracle/ngp_oracle.c); the 1,024 prefixes of the
   "all1024" case go through ``oracle_np`` (the same formulas on LAPACK: the C loops would take
   minutes), and the parts of a decomposition, which the oracle does not offer, through a plain fp64
   restatement below.  The worst ratios are the R64_* constants of the cases file.

2. No long-double-judged case is above the floor (50 eps cond <= 1e-8); the fp64-judged ones
   (n = 2110) are condition-aware and say so in RECORDS.

3. ``long_reference.origins`` (one factorisation, cumulative sums) against ``hr.evaluate`` of each
   prefix (its own factorisation) to long-double rounding.

4. Teeth: a Schur sum that skips one block column, and an origin one term short, FAIL the judgement.
"""
import functools

import numpy as np
import pytest
from scipy.linalg import cholesky, solve_triangular

from oracle import oracle_np
from tests import hp_reference as hr
from tests import long_depth_cases as ld
from tests import long_reference as lr
from tests import value_cases as vc
from tests.engine_oracle import OracleEngine

QUARTER = 0.25


def within_floor(r, ctx):
    if r.tol_factor == 1.0:
        assert vc.cond_within_floor(r), (ctx, r.cond)
    else:
        assert r.n > hr.HP_MAX_N - 10, ctx          # only the headline depth leaves long double


# ---- 1 + 2. fairness ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_long(case):
    t, y, t_add, y_add, t_new = case.inputs()
    worst = 0.0
    for p, prog in enumerate(ld.programs(case.n)):
        r = ld.long_reference(case, p)
        within_floor(r, (case.id, p))
        yp = ld._row(y, p)
        if case.d:
            o = OracleEngine().nowcast([prog], t, yp, t_add, y_add, t_new, True)
            assert not o["info"].any()
            mu, sg = o["mu"][0], o["sigma"][0]
        else:
            a, b, _, info = OracleEngine().predict([prog], t, yp, t_new, True)
            assert not info.any()
            mu, sg = a[0][None], b[0]
        worst = max(worst, ld.judge_long("long depth (fp64 oracle, 1/4 tol)", mu, np.diag(sg).copy(),
                                         sg if case.sigma else None, r, ctx=(case.id, p), frac=QUARTER))
    return worst


@functools.lru_cache(maxsize=None)
def oracle_origins(case):
    t, y, cuts, t_new = case.inputs()
    worst = 0.0
    for p, prog in enumerate(ld.programs(case.n)):
        r = ld.origins_reference(case, p)
        within_floor(r, (case.id, p))
        yp = ld._row(y, p)
        mu, var, lm = (np.empty((len(cuts), t_new.size)), np.empty((len(cuts), t_new.size)),
                       np.empty(len(cuts)))
        for k, c in enumerate(cuts):
            if case.kind == "all1024":
                a, b, lm[k], info = oracle_np.predict(prog, t[:c], yp[:c], t_new, True)
                mu[k], var[k] = a, np.diag(b)
            else:
                a, b, l1, info = OracleEngine().predict([prog], t[:c], yp[:c], t_new, True)
                mu[k], var[k], lm[k], info = a[0], np.diag(b[0]), l1[0], info[0]
            assert info == 0, (case.id, p, c)
        worst = max(worst, ld.judge_origins("origins depth (fp64 oracle, 1/4 tol)", mu, var, lm, r,
                                            ctx=(case.id, p), frac=QUARTER))
    return worst


def fp64_components(prog, comps, t, y, t_add, y_add, t_new):
    """tests/component_nowcast_reference.py's formulas in fp64 on LAPACK"""
    tt = np.concatenate([t, t_add])
    D, m, C = y_add.shape[0], t_new.size, len(comps)
    L = cholesky(oracle_np.cov(prog, tt, tt, True), lower=True, check_finite=False)
    Y = np.concatenate([np.repeat(y[:, None], D, axis=1), y_add.T], axis=0)
    Z = solve_triangular(L, Y, lower=True, check_finite=False)
    X = np.concatenate([oracle_np.cov(c, t_new, tt) for c in comps], axis=0)
    V = solve_triangular(L, X.T, lower=True, check_finite=False)
    sig = -(V.T @ V)
    for c, cp in enumerate(comps):
        sig[c * m:(c + 1) * m, c * m:(c + 1) * m] += oracle_np.cov(cp, t_new, t_new)
    sig = (sig + sig.T) / 2
    return (V.T @ Z).reshape(C, m, D).transpose(0, 2, 1), sig


@functools.lru_cache(maxsize=None)
def oracle_components(case):
    n, d, D, m = case
    t, y, t_add, y_add, t_new = ld.query(n, d, D, m)
    worst = 0.0
    for p, prog in enumerate(ld.programs(n)):
        r = ld.components_reference(case, p)
        assert r.info == 0 and 50 * 2.220446049250313e-16 * r.cond <= 1e-8, (case, p, r.cond)
        comps = ld.comps_of(n)[p]
        assert len(comps) == 1 + (p + n) % 3
        mu, sig = fp64_components(prog, comps, t, y, t_add, y_add, t_new)
        C = len(comps)
        cross = np.einsum("ajbj->abj", sig.reshape(C, m, C, m))
        worst = max(worst, ld.judge_components("components depth (fp64, 1/4 tol)", mu, cross, sig, r, prog,
                                               ctx=(case, p), frac=QUARTER))
    return worst


def _oracle_moments(prog, case, yp):
    t, y, t_add, y_add, t_new = case.inputs()
    if case.d:
        o = OracleEngine().nowcast([prog], t, yp, t_add, y_add, t_new, True)
        assert not o["info"].any()
        return o["mu"][0], o["sigma"][0]
    a, b, _, info = OracleEngine().predict([prog], t, yp, t_new, True)
    assert not info.any()
    return a[0][None], b[0]


@functools.lru_cache(maxsize=None)
def oracle_agreement(case):
    """the agreement judgement of the GPU test, the oracle against the reference itself"""
    y = case.inputs()[1]
    worst = 0.0
    for p, prog in enumerate(ld.agree_programs(case.n)):
        r = ld.agree_reference(case, p)
        within_floor(r, (case.id, p))
        mu, sg = _oracle_moments(prog, case, ld._row(y, p))
        worst = max(worst, ld.judge_agreement("agreement at depth (fp64 oracle, 1/4 tol)", mu, np.diag(sg).copy(),
                                              sg if case.sigma else None, np.asarray(r.mu, float), r.sigma, r,
                                              ctx=(case.id, p), frac=QUARTER))
    return worst


@pytest.mark.parametrize("case", ld.AGREE, ids=lambda c: c.id)
def test_fp64_oracle_meets_the_agreement_tolerance_at_a_quarter(case):
    assert oracle_agreement(case) < 1.0


def test_the_original_changepoint_particle_cannot_meet_the_agreement_tolerance():
    """why ``agree_programs`` replaces it: the oracle's own mean is beyond a quarter of
    the agreement tolerance (here beyond all of it) although it passes the judgement against the
    reference — nothing a device path could be held to"""
    case = ld.Long(1090, 0, 1, 65)
    assert case in ld.AGREE
    prog = ld.programs(case.n)[2]
    r = ld.long_reference(case, 2)
    mu, sg = _oracle_moments(prog, case, case.inputs()[1])
    with pytest.raises(AssertionError):
        ld.judge_agreement("unfair", mu, np.diag(sg).copy(), sg, np.asarray(r.mu, float), r.sigma, r,
                           frac=QUARTER, record=False)


@pytest.mark.parametrize("case", ld.LONGS, ids=lambda c: c.id)
def test_fp64_oracle_passes_every_long_query_at_a_quarter_of_the_tolerance(case):
    assert oracle_long(case) < 1.0


@pytest.mark.parametrize("case", ld.ORIGINS, ids=lambda c: c.id)
def test_fp64_oracle_on_every_prefix_passes_at_a_quarter_of_the_tolerance(case):
    assert oracle_origins(case) < 1.0


@pytest.mark.parametrize("case", ld.COMPONENTS, ids=lambda c: f"n{c[0]}")
def test_fp64_parts_pass_at_a_quarter_of_the_tolerance(case):
    assert oracle_components(case) < 1.0


def test_the_fairness_constants_are_the_oracles_worst_ratios():
    """error / FULL tolerance (the ratios above are of the quarter)"""
    got = dict(predict=QUARTER * max(oracle_long(c) for c in ld.LONGS),
               origins=QUARTER * max(oracle_origins(c) for c in ld.ORIGINS),
               components=QUARTER * max(oracle_components(c) for c in ld.COMPONENTS),
               agree=QUARTER * max(oracle_agreement(c) for c in ld.AGREE))
    print("worst error / tolerance of the fp64 oracle:", {k: f"{v:.3e}" for k, v in got.items()})
    want = dict(predict=ld.R64_PREDICT, origins=ld.R64_ORIGINS, components=ld.R64_COMPONENTS,
                agree=ld.R64_AGREE)
    for k in got:
        assert got[k] < QUARTER and abs(got[k] - want[k]) <= 0.1 * want[k], (k, got[k], want[k])


def test_the_cases_reach_what_they_are_there_for():
    for n, n0, nb0, tail in ((192, 192, 3, 0), (257, 256, 4, 1), (577, 576, 9, 1), (1090, 1088, 17, 2),
                             (2110, 2048, 32, 62)):
        assert ld.n0_of(n) == n0 and n0 // 64 == nb0 and n - n0 == tail
        assert any(c.n == n and c.d == 0 for c in ld.DEPTH) and any(c.n == n and c.d == 3 for c in ld.DEPTH)
    assert {c.m for c in ld.DEPTH if c.n >= 192 and c.sigma} >= {1, 65, 300, 1000}
    assert sorted(c.n % 64 + c.d for c in ld.COND_BLOCK) == [88, 89, 101, 163, 163]
    for c in ld.LONGS:
        assert c.n % 64 + c.d + 1 <= 192 and c.m <= 4096
    wrap = 4096 * 256
    fill = lambda c: (1 + c.n % 64 + c.d + c.m + 63) // 64 * 64 * ld.n0_of(c.n)     # noqa: E731
    assert sum(fill(c) > wrap for c in ld.LONGS) >= 2
    assert any(c.sigma and c.m * c.m > wrap for c in ld.LONGS)
    for case in ld.ORIGINS:
        t, y, cuts, t_new = case.inputs()
        n0 = ld.n0_of(case.n)
        assert cuts == sorted(set(cuts)) and cuts[0] >= 1 and cuts[-1] <= case.n and len(cuts) <= 1024
        if case.kind == "edges":
            assert {1, 63, 64, 65, 128, 129, n0 - 1, n0, n0 + 1, case.n} <= set(cuts)
            assert case.n < 1026 or {1023, 1024, 1025} <= set(cuts)
            tiles = sorted({(c - 1) // 64 for c in cuts if c <= n0})
            five = [k for k in tiles if sum((c - 1) // 64 == k for c in cuts) >= 5]
            assert five, case.id
            if case.n >= 577:                   # two cut-free tiles, then a tile with cuts
                assert five[0] - 1 not in tiles and five[0] - 2 not in tiles, case.id
        if case.kind == "half":
            assert max(cuts) <= n0 // 2
    assert any(c.kind == "all1024" and c.n == 1090 and c.m == 17 for c in ld.ORIGINS)
    assert {c.m for c in ld.ORIGINS} == {17, 65, 300}
    t, _ = ld.irregular_series(577)
    assert np.all(np.diff(t) > 0) and np.unique(np.round(np.diff(t), 12)).size > 500
    assert abs(t[-1] - 576 * ld.H) < 1e-12 and t[0] == 0.0


# ---- 3. the origins reference ----------------------------------------------------------------------------
def test_origins_reference_is_the_reference_of_every_prefix():
    n, m = 150, 17
    t, y = ld.series(n)
    cuts = [1, 64, 65, 149, 150]
    t_new = ld.origin_dates(n, m)
    for p, prog in enumerate(ld.programs(n)):
        r = lr.origins(prog, t, y, cuts, t_new)
        assert r.info == 0 and r.tol_factor == 1.0 and r.mu.dtype == hr.LD
        bound = 1e3 * hr.EPS_LD * r.cond
        for k, c in enumerate(cuts):
            e = hr.evaluate(prog, t[:c], y[:c], None, grad=False, t_new=t_new)
            assert e.info == 0 and e.cond <= r.cond * (1 + 1e-9)
            s = np.abs(np.diag(e.sigma))
            dev = max(float(np.max(np.abs(r.mu[k] - e.mu) / np.sqrt(s))),
                      float(np.max(np.abs(r.var[k] - np.diag(e.sigma)) / s)),
                      float(abs(r.logml[k] - e.logml) / abs(e.logml)))
            assert dev <= bound, (p, c, dev, bound)
    # and the rows reference is hr.nowcast where both can be formed
    tq, yq, t_add, y_add, tn = ld.query(n, 3, 2, 40)
    rows = [0, 7, 39]
    for prog in ld.programs(n):
        a = lr.nowcast_rows(prog, tq, yq, t_add, y_add, tn, rows)
        b = hr.nowcast(prog, tq, yq, t_add, y_add, tn)
        d, dd = hr.pred_scales(b.sigma)
        bound = 1e3 * hr.EPS_LD * b.cond
        assert a.cond == b.cond and a.tol_factor == b.tol_factor == 1.0
        assert float(np.max(np.abs(a.mu - b.mu) / d)) <= bound
        assert float(np.max(np.abs(a.var - np.diag(b.sigma)) / (d * d))) <= bound
        assert float(np.max(np.abs(a.sigma_rows - b.sigma[rows]) / dd[rows])) <= bound


# ---- 4. teeth ----------------------------------------------------------------------------------------------
def fp64_panel(prog, tt, Y, t_new):
    L = cholesky(oracle_np.cov(prog, tt, tt, True), lower=True, check_finite=False)
    Z = solve_triangular(L, Y, lower=True, check_finite=False)
    V = solve_triangular(L, oracle_np.cov(prog, tt, t_new), lower=True, check_finite=False)
    return L, Z, V


def test_a_schur_sum_that_skips_a_block_column_fails():
    case = ld.Long(577, 3, 2, 65)
    assert case in ld.LONGS
    t, y, t_add, y_add, t_new = case.inputs()
    tt = np.concatenate([t, t_add])
    Y = np.concatenate([np.repeat(y[:, None], case.D, axis=1), y_add.T], axis=0)
    for p, prog in enumerate(ld.programs(case.n)):
        r = ld.long_reference(case, p)
        _, Z, V = fp64_panel(prog, tt, Y, t_new)
        for skip in (False, True):
            W = V.copy()
            if skip:
                W[128:192] = 0.0
            sg = oracle_np.cov(prog, t_new, t_new) - W.T @ W
            sg[np.arange(case.m), np.arange(case.m)] += prog[2] + 1e-5
            args = ("teeth", (W.T @ Z).T, np.diag(sg).copy(), sg, r)
            if skip:
                with pytest.raises(AssertionError):
                    ld.judge_long(*args, record=False)
            else:
                ld.judge_long(*args, record=False)


def test_an_origin_one_term_short_fails():
    case = ld.Origins(577, "edges", 17)
    t, y, cuts, t_new = case.inputs()
    at = np.asarray(cuts) - 1
    for p, prog in enumerate(ld.programs(case.n)):
        r = ld.origins_reference(case, p)
        L, z, V = fp64_panel(prog, t, y, t_new)
        kss = np.diag(oracle_np.cov(prog, t_new, t_new)) + prog[2] + 1e-5
        lmk = -z * z / 2 - np.log(np.diag(L))
        for short in (0, 1):
            mu = np.cumsum(V * z[:, None], axis=0)[at]
            var = kss[None, :] - np.cumsum(V * V, axis=0)[at]
            lm = np.cumsum(lmk)[at] - np.asarray(cuts) / 2 * np.log(2 * np.pi)
            if short:
                c = 64 * 5 + 34                                  # the last of the five in one tile
                k = cuts.index(c)
                mu[k] -= V[c - 1] * z[c - 1]
                var[k] += V[c - 1] ** 2
                lm[k] -= lmk[c - 1]
                with pytest.raises(AssertionError):
                    ld.judge_origins("teeth", mu, var, lm, r, record=False)
            else:
                ld.judge_origins("teeth", mu, var, lm, r, record=False)

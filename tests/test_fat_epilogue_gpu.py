"""The fat steps' epilogue shared between the two sibling waves of a row tile (DESIGN.md section
4.2): the column-(j+1) wave runs the last 16-row pass of its sibling's solve X' = M C' from the S'
rows handed over in LDS, and at pair 0 (empty k-range) no longer reads and rewrites its own tile.

The smallest series at which that hand-over can go wrong, on the column sweep (the one-launch path
of short series is switched off), each with 3 and 17 items (item -> workgroup decode off the
multiples of 8), stationary trees (structured storage: K' generated in the epilogue, by both waves)
next to trees with a Linear or ChangePoint node (K' read from HBM) in one batch (a batch that holds
both also keeps the stationary items' gradients on the general leaf, i.e. on the fat kernel's
gradient instantiation), through the predictive path and the gradient:

  n = 128        one pair, epilogue-only fat step, no row tile below: aux tiles only
  n = 192        one fat pair, then a FULL step on the odd last column
  n = 256, 257   two pairs, ragged aux tail; in the second pair k-loop and hand-over are both live
  n = 448        a late pair with an odd number of row tiles below it

and n = 256 once under NGP_PREC_MIXED (the tile maxima are merged across the two waves).
Judged against oracle_np / oracle_c with the tolerances of tests/test_gpu_parity.py (logml 1e-10,
predictive 1e-8, gradient 1e-7, condition-aware) and of tests/test_mixed_gpu.py (1e-6)."""
import numpy as np
import pytest

from nowcastautogp_amd import _lib, gp
from nowcastautogp_amd._abi import NGP_PREC_MIXED, default_spec
from oracle import oracle_c, oracle_np
from tests.util import TOL_LOGML, TOL_PRED, check, nerr

pytestmark = pytest.mark.gpu

TOL_GRAD = 1e-7          # tests/test_gpu_parity.py
TOL_MIXED = 1e-6         # tests/test_mixed_gpu.py
M_NEW = 5                # forecast dates: with the tail and y' they fit one aux tile's first 16 rows


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    c = _lib.Context(0)
    c.set_short_series_path(False)     # n <= 256 on the column sweep as well
    yield c
    c.close()


def batch(n, B):
    """B items on a regular grid of n points: even items stationary, odd ones with a Linear or a
    ChangePoint node, every item with parameters of its own"""
    rng = np.random.Generator(np.random.PCG64(1000 * n + B))
    progs = []
    for b in range(B):
        f = np.exp(0.1 * rng.standard_normal(4))
        if b % 2 == 0:
            tree = gp.Plus(gp.SquaredExponential(0.25 * f[0], 0.8 * f[1]), gp.Periodic(0.9 * f[2], 0.17 * f[3], 0.5))
        elif b % 4 == 1:
            tree = gp.Plus(gp.Linear(0.3 * f[0], 0.2 * f[1], 0.6 * f[2]), gp.Periodic(0.8, 0.21 * f[3], 0.6))
        else:
            tree = gp.ChangePoint(gp.SquaredExponential(0.2 * f[0], 0.9), gp.Periodic(0.7 * f[1], 0.2 * f[2], 0.6),
                                  0.55 * f[3], 0.08)
        progs.append(gp.to_program(tree) + (0.05 * float(f[0]),))
    t = np.arange(n) / (n - 1.0)
    y = np.sin(9.0 * t) + 0.3 * t + 0.2 * rng.standard_normal(n)
    t_new = 1.0 + np.arange(1, M_NEW + 1) / (n - 1.0)
    return progs, t, y, t_new


_REFS = {}


def reference(n, B):
    """per item: cond(K), the predictive and logml of oracle_np — computed once per (n, B)"""
    if (n, B) not in _REFS:
        progs, t, y, t_new = batch(n, B)
        _REFS[(n, B)] = [(float(np.linalg.cond(oracle_np.cov(p, t, t, True))),) + tuple(oracle_np.predict(p, t, y, t_new))
                         for p in progs]
    return _REFS[(n, B)]


@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("n", [128, 192, 256, 257, 448])
def test_predictive_through_the_shared_solve(ctx, n, B):
    progs, t, y, t_new = batch(n, B)
    mu, sg, lm, info = ctx.predict_batch(progs, t, y, t_new)
    assert not info.any(), info
    for b, (cond, rmu, rsg, rlm, oi) in enumerate(reference(n, B)):
        assert oi == 0
        check("test_fat_epilogue:logml", lm[b], rlm, TOL_LOGML, cond, ctx=(n, B, b))
        check("test_fat_epilogue:predictive", mu[b], rmu, TOL_PRED, cond, ctx=(n, B, b))
        check("test_fat_epilogue:predictive", sg[b], rsg, TOL_PRED, cond, ctx=(n, B, b))


@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("n", [128, 192, 256, 257, 448])
def test_gradient_through_the_shared_solve(ctx, n, B):
    progs, t, y, _ = batch(n, B)
    lm, grads, info = ctx.logml_grad_batch(progs, t, y)
    assert not info.any(), info
    ref = reference(n, B)
    for b in range(B):
        check("test_fat_epilogue:logml", lm[b], ref[b][3], TOL_LOGML, ref[b][0], ctx=(n, B, b))
    # the forward-mode oracle costs n^3 per parameter: first, middle and last items (both kinds of
    # tree, both sides of a multiple of 8)
    for b in sorted({0, 1, 2, B // 2, B // 2 + 1, B - 2, B - 1}):
        rlm, rg, oi = oracle_c.logml_grad(progs[b], t, y)
        assert oi == 0 and grads[b].shape == rg.shape
        check("test_fat_epilogue:gradient", grads[b], rg, TOL_GRAD, ref[b][0], ctx=(n, B, b))


def test_mixed_precision_tile_maxima_across_the_two_waves(ctx):
    n, B = 256, 17
    progs, t, y, t_new = batch(n, B)
    ctx.set_spec(default_spec(NGP_PREC_MIXED))
    try:
        mu, sg, lm, info = ctx.predict_batch(progs, t, y, t_new)
    finally:
        ctx.set_spec(default_spec())
    assert not info.any(), info
    for b, (cond, rmu, rsg, rlm, oi) in enumerate(reference(n, B)):
        assert nerr(lm[b], rlm) < TOL_MIXED, (b, cond)
        assert nerr(mu[b], rmu) < TOL_MIXED, (b, cond)
        assert nerr(np.diag(sg[b]), np.diag(rsg)) < TOL_MIXED, (b, cond)
    # the merged maxima decide which tile products run in fp32: the share the device reports against
    # the host model's counts (tests/mixed_model.py; the allowance is tests/mixed_cases.count_error's)
    from tests import mixed_cases, mixed_model
    sp = default_spec(NGP_PREC_MIXED)
    ctx.set_spec(sp)
    try:
        job = ctx.stage_predict(progs, t, y, t_new)
        frac = job.run().mixed_stats()["frac_f32"]
        job.close()
    finally:
        ctx.set_spec(default_spec())
    for b, p in enumerate(progs):
        m = mixed_model.item_counts(p, t, y, t_new, sp.mixed_tau, sp.jitter)
        err, allowed = mixed_cases.count_error(frac[b], m)
        assert m["n32"] + m["n64"] == 8 and m["borderline"] == 0
        assert err <= allowed, (b, frac[b], m["n32"], m["n64"])

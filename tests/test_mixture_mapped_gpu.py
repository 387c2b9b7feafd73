"""ngp_mixture_crps_mapped on the device against the independent host integrator
(tests/mixture_mapped_reference.py).  The accuracy contract of include/ngp.h, with ``ref`` and
``S = E|Y - s(y)|`` both from the reference:

    |crps - ref| <= err + 1e-13 S          err <= tol |crps| whenever info = 0

The mean has no error estimate of its own; it is the K15 sum of an integrand that is smoother than
the CRPS's (F instead of F^2) on the same panels, so it is held to the requested relative accuracy
(the default tol, 1e-10) of S plus the 1e-13 floor on the two numbers it is the sum of:
|mean - ref| <= 1e-10 S + 1e-13 (|psi(x0)| + S) <= 1e-10 S + 1e-13 (|ref| + 2 S), plus twice the
reference's own last change of its mean (``mean_err``, ~1e-16 S in every case below).

Every check prints the figures it judges before it asserts."""
import math

import numpy as np
import pytest

from nowcastautogp_amd import _abi, autogp
from nowcastautogp_amd import nowcast as nc
from tests import mirror_contracts as mc
from tests import mixture_mapped_reference as M
from tests import mixture_reference as R

pytestmark = pytest.mark.gpu

DEFAULT_TOL = 1e-10
CAP = 1e6       # the cap of a Box-Cox inverse with lam < 0 (1000 x the largest observation)


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge
    ge.build()
    e = autogp.HipEngine(0)
    yield e
    e.ctx.close()


@pytest.fixture(scope="module")
def ctx(eng):
    return eng.ctx


def mixture(Cn, m, seed, centre, spread, sd0):
    rng = np.random.default_rng([seed, Cn, m])
    mu = centre + spread * rng.standard_normal((Cn, m))
    sd = sd0 * np.exp(0.4 * rng.standard_normal((Cn, m)))
    w = np.exp(rng.standard_normal(Cn))
    return R.Mixture(w / w.sum(), mu, sd * sd)


def y_near(mix, inv, k=0.7):
    """observations on the original scale: g at the pool's centre + k pooled sd"""
    c, s = mix.centre_and_sd()
    return np.asarray(M.g_of(inv, c + k * s), dtype=np.float64)


def check(ctx, label, mix, inv, scale, shift, y, tol=0.0, want_info=0):
    crps, mean, err, info = ctx.mixture_crps_mapped(mix.w, mix.mu, mix.var, inv, scale, shift, y, tol)
    ref = M.reference(mix, inv, scale, shift, y)
    assert not ref["status"].any(), (label, ref["status"])
    miss, S = np.abs(crps - ref["crps"]), ref["S"]
    mmiss = np.abs(mean - ref["mean"])
    mbound = DEFAULT_TOL * S + 1e-13 * (np.abs(ref["mean"]) + 2 * S) + 2 * ref["mean_err"]
    t = tol if tol > 0 else DEFAULT_TOL
    print(f"{label}: info {info}, |crps - ref| / S {miss / S}, err / S {err / S}, "
          f"err / |crps| {err / np.abs(crps)} (tol {t:.0e}), |mean - ref| / bound {mmiss / mbound}")
    assert np.all(info == want_info), (label, info)
    assert np.all(np.isfinite(crps)) and np.all(np.isfinite(mean)) and np.all(err >= 0), label
    assert np.all(miss <= err + 1e-13 * S), (label, miss, err, S)
    if want_info == 0:
        assert np.all(err <= t * np.abs(crps)), (label, err, crps)
    if want_info == 0:
        assert np.all(mmiss <= mbound), (label, mmiss, mbound)
    return crps, mean, err


BC03 = (M.BOXCOX, 0.3, 0.0, CAP)


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("Cn", [1, 2, 255, 256, 257, 600])      # the component tile is 256
def test_component_tile_edges(ctx, Cn, m):
    mix = mixture(Cn, m, 21, centre=5.0, spread=0.4, sd0=0.15)
    check(ctx, f"boxcox 0.3 natural C={Cn} m={m}", mix, BC03, M.NATURAL, 0.0, y_near(mix, BC03))
    inv = (M.EXP, 0.0, 0.0, 0.0)
    check(ctx, f"exp log+1 C={Cn} m={m}", mix, inv, M.LOG, 1.0, y_near(mix, inv, -1.1))


KINDS = [
    ("identity", (M.IDENTITY, 0.0, 0.0, 0.0), 6.0, 0.3, 0.1),
    ("exp", (M.EXP, 0.0, 0.0, 0.0), 3.0, 0.5, 0.2),
    ("exp offset", (M.EXP, 0.0, 0.5, 0.0), 6.0, 0.3, 0.1),
    ("logistic", (M.LOGISTIC100, 0.0, 0.0, 0.0), 0.3, 0.6, 0.25),
    ("logistic offset", (M.LOGISTIC100, 0.0, 0.01, 0.0), 0.3, 0.6, 0.25),
    ("boxcox 0", (M.BOXCOX, 0.0, 0.0, CAP), 3.0, 0.5, 0.2),
    ("boxcox 0.3", BC03, 5.0, 0.5, 0.2),
    ("boxcox 0.3 offset", (M.BOXCOX, 0.3, 0.5, CAP), 8.0, 0.4, 0.12),
    ("boxcox 1", (M.BOXCOX, 1.0, 0.0, CAP), 20.0, 2.0, 1.0),
    ("boxcox 2", (M.BOXCOX, 2.0, 0.0, CAP), 30.0, 3.0, 1.5),
    ("boxcox -0.2", (M.BOXCOX, -0.2, 0.0, CAP), 1.5, 0.15, 0.06),     # the pole is at x = 5
]


@pytest.mark.parametrize("scale,shift", [(M.NATURAL, 0.0), (M.LOG, 0.0), (M.LOG, 1.0)])
@pytest.mark.parametrize("name,inv,centre,spread,sd0", KINDS, ids=[k[0] for k in KINDS])
def test_every_kind_on_both_scales(ctx, name, inv, centre, spread, sd0, scale, shift):
    mix = mixture(7, 3, 22, centre, spread, sd0)
    check(ctx, f"{name} scale={scale} shift={shift}", mix, inv, scale, shift, y_near(mix, inv))


def test_identities(ctx):
    mix = mixture(40, 3, 23, centre=1.0, spread=0.5, sd0=0.2)
    y = mix.centre_and_sd()[0] + 0.3
    c, _, _, info = ctx.mixture_crps_mapped(mix.w, mix.mu, mix.var, (M.IDENTITY, 0, 0, 0), M.NATURAL, 0.0, y)
    assert not info.any()
    R.check_crps("identity + natural = ngp_mixture_crps", mix, y, c)
    closed, _ = ctx.mixture_crps(mix.w, mix.mu, mix.var, y)
    _, scale_ = R.ref_crps(mix, y)
    assert np.all(np.abs(c - closed) <= 2 * R.TOL_CRPS * scale_)
    c, _, _, info = ctx.mixture_crps_mapped(mix.w, mix.mu, mix.var, (M.EXP, 0, 0, 0), M.LOG, 0.0, np.exp(y))
    assert not info.any()
    R.check_crps("exp + log = ngp_mixture_crps(log y)", mix, np.log(np.exp(y)), c)
    mu, sd, yy = 0.4, 0.3, 1.7
    one = R.Mixture([1.0], [[mu]], [[sd * sd]])
    c, mean, _, info = ctx.mixture_crps_mapped(one.w, one.mu, one.var, (M.EXP, 0, 0, 0), M.NATURAL, 0.0, [yy])
    want = M.lognormal_crps(mu, sd, yy)
    S = M.reference(one, (M.EXP, 0, 0, 0), M.NATURAL, 0.0, [yy])["S"][0]
    print(f"lognormal closed form: |crps - closed| / S = {abs(c[0] - want) / S:.3e} (bound {R.TOL_CRPS:.0e})")
    assert info[0] == 0 and abs(c[0] - want) <= R.TOL_CRPS * S
    # E exp(X) = sum w exp(mu + var / 2)
    mean_ = ctx.mixture_crps_mapped(mix.w, mix.mu, mix.var, (M.EXP, 0, 0, 0), M.NATURAL, 0.0, np.exp(y))[1]
    want = mix.w @ np.exp(mix.mu + 0.5 * mix.var)
    print("lognormal mean: relative miss", np.abs(mean_ - want) / want)
    assert np.all(np.abs(mean_ - want) <= 1e-10 * want)


@pytest.mark.parametrize("side", [-1, 1])
def test_y_far_in_a_tail_clips_the_crossing(ctx, side):
    mix = mixture(5, 3, 24, centre=3.0, spread=0.3, sd0=0.1)
    for inv, scale, shift in (((M.EXP, 0, 0, 0), M.NATURAL, 0.0), (BC03, M.LOG, 1.0),
                              ((M.IDENTITY, 0, 0, 0), M.NATURAL, 0.0)):
        c, s = mix.centre_and_sd()
        y = np.asarray(M.g_of(inv, c + side * 60.0 * s), dtype=np.float64)
        check(ctx, f"far tail {side} kind={inv[0]}", mix, inv, scale, shift, y)


def atom_case():
    """date 0: half the mass on the clamp of exp(x) - 1 at x = 0; dates 1, 2: none of it"""
    rng = np.random.default_rng(25)
    mu = np.stack([0.2 * rng.standard_normal(6), 5 + 0.2 * rng.standard_normal(6),
                   4 + 0.2 * rng.standard_normal(6)], axis=1)
    return R.Mixture(np.full(6, 1 / 6), mu, np.tile([0.25, 0.01, 0.01], (6, 1))), (M.EXP, 0.0, 1.0, 0.0)


def test_mass_on_the_clamp(ctx):
    mix, inv = atom_case()
    for y in (np.array([0.0, 150.0, 50.0]), np.array([0.4, 140.0, 60.0])):      # y = 0: on the atom
        check(ctx, f"atom natural y0={y[0]}", mix, inv, M.NATURAL, 0.0, y)
        check(ctx, f"atom log+1 y0={y[0]}", mix, inv, M.LOG, 1.0, y)
    y = np.array([0.4, 140.0, 60.0])
    crps, mean, err, info = ctx.mixture_crps_mapped(mix.w, mix.mu, mix.var, inv, M.LOG, 0.0, y)
    ref = M.reference(mix, inv, M.LOG, 0.0, y)
    print("atom, log with shift 0:", info, crps, ref["status"])
    assert list(info) == [_abi.NGP_INFO_NOT_FINITE, 0, 0] and list(ref["status"]) == [-3, 0, 0]
    assert np.isnan(crps[0]) and np.isnan(mean[0]) and np.isnan(err[0])
    assert np.all(np.isfinite(crps[1:])) and np.all(np.isfinite(mean[1:]))
    assert np.all(np.abs(crps[1:] - ref["crps"][1:]) <= err[1:] + 1e-13 * ref["S"][1:])


def test_negative_lambda_and_the_pole(ctx):
    inv = (M.BOXCOX, -0.2, 0.0, CAP)                        # pole at x = 5
    mix = mixture(6, 2, 26, centre=1.5, spread=0.15, sd0=0.06)
    y = y_near(mix, inv)
    check(ctx, "lam -0.2 below the pole", mix, inv, M.NATURAL, 0.0, y)
    mu, var = mix.mu.copy(), mix.var.copy()
    mu[2, 1], var[2, 1] = 4.9, 0.04                         # straddles the pole, date 1 only
    bad = R.Mixture(mix.w, mu, var)
    crps, mean, err, info = ctx.mixture_crps_mapped(bad.w, bad.mu, bad.var, inv, M.NATURAL, 0.0, y)
    ref = M.reference(bad, inv, M.NATURAL, 0.0, y)
    print("pole:", info, crps, ref["status"])
    assert list(info) == [0, _abi.NGP_INFO_NOT_FINITE] and list(ref["status"]) == [0, -3]
    assert np.isnan(crps[1]) and np.isfinite(crps[0])
    assert abs(crps[0] - ref["crps"][0]) <= err[0] + 1e-13 * ref["S"][0]


def test_zero_weights_are_ignored_and_bad_components_reported(ctx):
    mix = mixture(9, 3, 27, centre=5.0, spread=0.4, sd0=0.15)
    y = y_near(mix, BC03)
    w, mu, var = mix.w.copy(), mix.mu.copy(), mix.var.copy()
    w[[1, 4]] = 0.0
    w /= w.sum()
    mu[1], var[4] = np.nan, -1.0
    sparse = R.Mixture(w, mu, var)
    got = check(ctx, "zero weights carrying NaN", sparse, BC03, M.NATURAL, 0.0, y)
    var2 = var.copy()
    var2[5, 1] = 0.0                                        # positive weight, date 1
    crps, mean, err, info = ctx.mixture_crps_mapped(w, mu, var2, BC03, M.NATURAL, 0.0, y)
    assert list(info) == [0, 6, 0] and np.isnan(crps[1]) and np.isnan(mean[1])
    for k in (0, 2):                                        # the other dates: the same bits
        assert crps[k] == got[0][k] and mean[k] == got[1][k] and err[k] == got[2][k]


def sd_ratio_case():
    return R.Mixture([0.5, 0.5], [[0.0], [0.3]], [[1.0], [1e-8]]), (M.EXP, 0.0, 0.0, 0.0), np.array([1.2])


def test_panel_cap(ctx):
    """sd ratio 1e4 at tol 1e-12: 18 sd_max / sd_min is more panels than a date may have"""
    mix, inv, y = sd_ratio_case()
    check(ctx, "sd ratio 1e4", mix, inv, M.NATURAL, 0.0, y, tol=1e-12,
          want_info=_abi.NGP_INFO_NOT_CONVERGED)


def test_bitwise_reproducible_and_date_independent(ctx):
    mix = mixture(300, 3, 28, centre=5.0, spread=0.4, sd0=0.15)
    y = y_near(mix, BC03)
    a = ctx.mixture_crps_mapped(mix.w, mix.mu, mix.var, BC03, M.LOG, 1.0, y)
    b = ctx.mixture_crps_mapped(mix.w, mix.mu, mix.var, BC03, M.LOG, 1.0, y)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    for j in range(3):
        one = ctx.mixture_crps_mapped(mix.w, mix.mu[:, j:j + 1], mix.var[:, j:j + 1], BC03, M.LOG, 1.0,
                                      y[j:j + 1])
        for u, v in zip(a, one):
            assert u[j] == v[0], (j, u[j], v[0])


def test_through_the_mirror(eng):
    rng = np.random.default_rng(5)
    n = 24
    values = np.maximum(40.0 + 1.5 * np.arange(n) + 6.0 * rng.standard_normal(n), 1.0)
    fwd, inv = nc.get_transformations("boxcox", values)
    data = nc.create_transformed_data(mc.days(0, n), values, transformation=fwd)
    model = nc.make_and_fit_model(data, engine=eng, seed=3, **{**mc.FAST, "n_particles": 6})
    mix = nc.forecast_mixture(model, mc.days(n, n + 3))
    assert mix.engine is eng
    y = values[-1] + np.array([2.0, -5.0, 9.0])
    crps, err = mix.crps(y, inv_transformation=inv, scale="log", shift=1, return_error=True)
    mean = mix.mean(inv_transformation=inv, scale="log", shift=1)
    rm = R.Mixture(mix.weights, mix.means, mix.variances)
    ref = M.reference(rm, inv.ngp_inv, M.LOG, 1.0, y)
    print("mirror:", crps, err, np.abs(crps - ref["crps"]) / ref["S"])
    assert np.all(np.abs(crps - ref["crps"]) <= err + 1e-13 * ref["S"])
    print("mirror mean: |mean - ref| / S", np.abs(mean - ref["mean"]) / ref["S"])
    assert np.all(np.isfinite(mean))
    # the sample estimator on 20,000 draws: mean |Y - yt| - mean |Y - Y'| / 2; its standard error
    # from the projection of the U-statistic, h_i = |Y_i - yt| - mean_k |Y_i - Y_k|
    N = 20000
    yt = np.log(y + 1.0)
    for j in range(3):
        comp = rng.choice(rm.C, size=N, p=rm.w / rm.w.sum())
        x = rm.mu[comp, j] + np.sqrt(rm.var[comp, j]) * rng.standard_normal(N)
        Y = np.sort(np.log(inv(x) + 1.0))
        cs = np.concatenate([[0.0], np.cumsum(Y)])
        i = np.arange(N)
        g = (Y * i - cs[:-1] + (cs[-1] - cs[1:]) - Y * (N - 1 - i)) / N      # mean_k |Y_i - Y_k|
        est = float(np.mean(np.abs(Y - yt[j])) - 0.5 * np.mean(g))
        se = float(np.std(np.abs(Y - yt[j]) - g, ddof=1) / math.sqrt(N))
        print(f"date {j}: exact {crps[j]:.6f}, sample estimator {est:.6f}, standard error {se:.2e}")
        assert abs(crps[j] - est) <= 5 * se

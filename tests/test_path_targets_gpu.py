"""Trajectory targets on the device (ngp_mixture_path_targets / _indep) at the shapes where they
can go wrong (tests/path_targets_reference.py ``CASES``): m in {1, 2, 7, 33, 192}, P in {1, 3, 17}
with a component of weight zero, S in {1, 2, 5}, N in {1, 63, 257, 4099, 2^17 + 1}, the windows
[0,0], [m-1,m-1], [0,m-1], all five kinds at T = 64 and T = 1, Q = 1 and Q = 64 with repeated
levels, both entry points.

Pathwise tolerance (test 2): BASELINE is the deviation of the library's own ``ngp_mixture_sample``
output, passed through the numpy transformation and functionals, from the restatement on
``oracle_np`` draws, measured over the same cases in the same session (largest over the cases of
max |a - b| / max |b| per real-valued target); the new call's values may deviate 8 x BASELINE.
Measured on an MI355X: BASELINE = 1.39e-15 (tolerance 1.11e-14); the new call's largest deviation
over the cases = 1.39e-15, over the mirror tests = 2.90e-15 (n = 130, Box-Cox)."""
import numpy as np
import pytest

import __graft_entry__ as ge
from nowcastautogp_amd import _lib, autogp
from nowcastautogp_amd import nowcast as nc
from tests import mirror_contracts as mc
from tests import path_targets_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    ge.build()
    return _lib.Context(0)


_memo = {}


def run(ctx, name):
    """(case, restatement, the device call's result) — each computed once per session"""
    if name not in _memo:
        c = R.make_case(name)
        ref = R.restate(**c)
        out = ctx.mixture_path_targets(c["w"], c["mu"], c["sigma"], c["draws"], c["seed"], c["inv"],
                                       c["targets"], c["probs"], want_values=True)
        _memo[name] = (c, ref, out)
    return _memo[name]


PATHWISE = [n for n in sorted(R.CASES) if R.CASES[n]["pathwise"]]


@pytest.fixture(scope="module")
def baseline(ctx):
    """the existing sampler's deviation from the restatement, through the same numpy steps"""
    worst = 0.0
    for name in PATHWISE:
        c, ref, _ = run(ctx, name)
        if np.isscalar(c["seed"]):
            x = ctx.mixture_sample(c["w"], c["mu"], c["sigma"], c["draws"], c["seed"])[0]
        else:
            x = ctx.mixture_sample_indep(c["w"], c["mu"], c["sigma"], c["draws"], c["seed"])[0]
        v = R.inv_numpy(c["inv"])(x.reshape(-1, x.shape[-1]))
        worst = max(worst, R.deviation(R.functionals(v, c["targets"]), ref["values"], c["targets"],
                                       R.fragile(ref["v"], c["targets"], c["inv"]))[0])
    print(f"BASELINE (sampler + numpy vs restatement) = {worst:.3e}")
    assert worst > 0.0
    return worst


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_selection_and_counting_are_exact(ctx, name):
    """q, count and hist are, bit for bit and integer for integer, what numpy computes from the
    call's own values; the mean is their sum in another order."""
    c, _, out = run(ctx, name)
    assert not np.any(out["info"])
    vals = out["values"]
    assert not np.any(np.signbit(vals[vals == 0.0]))
    own = R.summaries(vals, c["targets"], c["probs"], c["mu"].shape[2])
    np.testing.assert_array_equal(out["q"], own["q"])
    np.testing.assert_array_equal(out["count"], own["count"])
    np.testing.assert_array_equal(out["hist"], own["hist"])
    N = vals.shape[1]
    tol = 4.0 * N * np.finfo(float).eps * np.abs(vals).sum(axis=1) / N
    assert np.all(np.abs(out["mean"] - own["mean"]) <= tol), (out["mean"], own["mean"])
    if name == "n131073_clamped":
        assert np.mean(vals[1] == 0.0) > 0.5
    if name == "constant":
        assert all(np.unique(v).size == 1 for v in vals)


@pytest.mark.parametrize("name", PATHWISE)
def test_paths_are_the_samplers_paths(ctx, baseline, name):
    c, ref, out = run(ctx, name)
    skip = R.fragile(ref["v"], c["targets"], c["inv"])
    assert skip.mean(axis=1).max() <= R.MAX_FRAGILE_SHARE
    dev, wrong = R.deviation(out["values"], ref["values"], c["targets"], skip)
    print(f"{name}: deviation {dev:.3e}, baseline {baseline:.3e}, tolerance {8 * baseline:.3e}")
    assert wrong == 0
    assert dev <= 8.0 * baseline, (dev, baseline)


@pytest.mark.parametrize("name", ["n257_boxcox_neg", "indep_s5", "n131073_clamped"])
def test_determinism_and_independence_of_the_levels(ctx, name):
    c, _, out = run(ctx, name)
    args = (c["w"], c["mu"], c["sigma"], c["draws"], c["seed"], c["inv"], c["targets"])
    again = ctx.mixture_path_targets(*args, c["probs"], want_values=True)
    for k in ("q", "mean", "count", "hist", "values"):
        assert out[k].tobytes() == again[k].tobytes(), k
    for i in (0, len(c["probs"]) // 2, len(c["probs"]) - 1):      # Q = 1: the same bits per level
        one = ctx.mixture_path_targets(*args, [c["probs"][i]])
        assert one["values"] is None
        assert one["q"][:, 0].tobytes() == out["q"][:, i].tobytes()
        assert one["mean"].tobytes() == out["mean"].tobytes()


def test_errors_and_info(ctx):
    c = R.make_case("shared_s5")
    w, mu, sg, d, seed, inv = c["w"], c["mu"], c["sigma"], c["draws"], c["seed"], c["inv"]
    ok_t, ok_p = [(0, 0, 6, 0.0)], [0.5]

    def status(**kw):
        a = dict(w=w, mu=mu, sigma=sg, draws=d, seed=seed, inv=inv, targets=ok_t, probs=ok_p)
        a.update(kw)
        try:
            ctx.mixture_path_targets(a["w"], a["mu"], a["sigma"], a["draws"], a["seed"], a["inv"],
                                     a["targets"], a["probs"])
        except _lib.NgpError as e:
            return e.status
        return 0

    assert status() == 0
    for bad in (dict(targets=[(0, 0, 7, 0.0)]), dict(targets=[(0, 3, 2, 0.0)]), dict(targets=[(5, 0, 1, 0.0)]),
                dict(targets=[(-1, 0, 1, 0.0)]), dict(targets=[(4, 0, 1, np.nan)]), dict(targets=[]),
                dict(probs=[0.0]), dict(probs=[0.5, 1.0]), dict(probs=[]), dict(draws=0),
                dict(inv=(4, 0.0, 0.0, 0.0)), dict(inv=(3, 0.3, 0.0, 0.0)), dict(inv=(3, 0.3, 0.0, -1.0)),
                dict(inv=(1, np.inf, 0.0, 0.0)), dict(inv=(1, 0.0, np.nan, 0.0)), dict(inv=(0, 0.0, 0.0, np.inf))):
        assert status(**bad) == -1, bad            # NGP_ERR_ARG
    for big in (dict(targets=ok_t * 65), dict(probs=[0.5] * 65), dict(draws=(2**31 - 1) // 5 + 1),
                dict(draws=(2**31 - 1) // 5, targets=ok_t * 64)):     # the last: 8 T N bytes = 1.1 TB
        assert status(**big) == -3, big            # NGP_ERR_TOO_LARGE
    m193 = 193
    assert status(mu=np.zeros((3, 5, m193)), sigma=np.tile(np.eye(m193), (3, 1, 1)),
                  targets=[(0, 0, 192, 0.0)]) == -3
    # a covariance that is not positive definite: info names the pivot; under positive weight every
    # output is NaN, under weight zero nothing changes
    bad_sg = sg.copy()
    bad_sg[2] = -np.eye(7)
    out = ctx.mixture_path_targets(w, mu, bad_sg, d, seed, inv, c["targets"], c["probs"], want_values=True)
    assert out["info"].tolist() == [0, 0, 1]
    assert np.isnan(out["q"]).all() and np.isnan(out["mean"]).all() and np.isnan(out["values"]).all()
    assert not out["count"].any() and not out["hist"].any()
    w0 = w.copy()
    w0[:, 2] = 0.0
    w0 /= w0.sum(axis=1, keepdims=True)
    a = ctx.mixture_path_targets(w0, mu, bad_sg, d, seed, inv, c["targets"], c["probs"], want_values=True)
    b = ctx.mixture_path_targets(w0, mu, sg, d, seed, inv, c["targets"], c["probs"], want_values=True)
    assert a["info"].tolist() == [0, 0, 1] and not b["info"].any()
    for k in ("q", "mean", "count", "hist", "values"):
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("n", [40, 130])
@pytest.mark.parametrize("transform", ["positive", "boxcox", "lambda"])
def test_mirror_summarises_the_matrix_forecast_with_nowcasts_returns(ctx, baseline, n, transform):
    """From one snapshot and seed, forecast_targets_with_nowcasts equals numpy functionals of the
    matrix forecast_with_nowcasts returns (P = 8, D = 3, m = 6), to test 2's tolerance."""
    eng = autogp.HipEngine(0)
    rng = np.random.default_rng(n)
    values = 12.0 + 4.0 * np.sin(np.arange(n) / 5.0) + rng.random(n)
    if transform == "lambda":
        fwd, inv = (lambda y: np.log(y)), (lambda y: np.exp(y))
    else:
        fwd, inv = nc.get_transformations(transform, values)
    base = mc.fitted(eng, values=[float(fwd(v)) for v in values], seed=11, n_particles=8)
    nd, fd = mc.days(n, n + 2), mc.days(n + 2, n + 8)
    nows = [nc.TData(nd, list(values[-2:] * (1.0 + 0.05 * k)), transformation=fwd) for k in range(3)]
    targets = [("sum", 0, 3, 50.0), ("max", 0, 5, 15.0), ("diff", 0, 5, 0.0), ("argmax", 0, 5), ("exceed", 0, 5, 16.0)]
    probs = [0.025, 0.5, 0.975]
    a, b = base.clone(), base.clone()
    mat = nc.forecast_with_nowcasts(a, nows, fd, 400, inv_transformation=inv)          # [m, D draws]
    res = nc.forecast_targets_with_nowcasts(b, nows, fd, targets, 400, probs=probs,
                                            inv_transformation=inv, want_values=True)
    assert res.device == (transform != "lambda")
    tgs = res.targets
    ref = R.functionals(np.ascontiguousarray(mat.T), tgs)
    inv_desc = getattr(inv, "ngp_inv", (R.EXP, 0.0, 0.0, 0.0))
    skip = R.fragile(np.ascontiguousarray(mat.T), tgs, inv_desc)
    dev, wrong = R.deviation(res._values, ref, tgs, skip)
    print(f"mirror n={n} {transform}: deviation {dev:.3e} (tolerance {8 * baseline:.3e})")
    assert wrong == 0 and dev <= 8.0 * baseline
    own = R.summaries(res._values, tgs, probs, 6)
    np.testing.assert_array_equal(res.q, own["q"])
    np.testing.assert_array_equal(res.count, own["count"])
    np.testing.assert_array_equal(res.hist, own["hist"])
    assert a.rng_shared.integers(0, 2**62) == b.rng_shared.integers(0, 2**62)


MIRROR_TARGETS = [("sum", 0, 3, 50.0), ("max", 0, 5, 15.0), ("diff", 0, 5, 0.0), ("argmax", 0, 5),
                  ("exceed", 0, 5, 16.0)]


def _mirror_fixture(n=40):
    eng = autogp.HipEngine(0)
    rng = np.random.default_rng(n)
    values = 12.0 + 4.0 * np.sin(np.arange(n) / 5.0) + rng.random(n)
    fwd, inv = nc.get_transformations("boxcox", values)
    base = mc.fitted(eng, values=[float(fwd(v)) for v in values], seed=11, n_particles=8)
    return base, values, fwd, inv


def _check_against_matrix(res, mat, inv, baseline, what):
    paths = np.ascontiguousarray(mat.T)
    ref = R.functionals(paths, res.targets)
    dev, wrong = R.deviation(res._values, ref, res.targets, R.fragile(paths, res.targets, inv.ngp_inv))
    print(f"{what}: deviation {dev:.3e} (tolerance {8 * baseline:.3e})")
    assert res.device and wrong == 0 and dev <= 8.0 * baseline
    own = R.summaries(res._values, res.targets, res.probs, mat.shape[0])
    np.testing.assert_array_equal(res.q, own["q"])
    np.testing.assert_array_equal(res.count, own["count"])
    np.testing.assert_array_equal(res.hist, own["hist"])


def test_forecast_targets_summarises_the_matrix_forecast_returns(ctx, baseline):
    """One model: S = 1 through the independent form, keyed by the seed the mixture's own stream
    gives, draws the paths forecast() draws."""
    base, values, fwd, inv = _mirror_fixture()
    fd = mc.days(40, 46)
    a, b = base.clone(), base.clone()
    mat = nc.forecast(a, fd, 500, inv_transformation=inv)
    res = nc.forecast_targets(b, fd, MIRROR_TARGETS, 500, probs=[0.025, 0.5, 0.975],
                              inv_transformation=inv, want_values=True)
    assert res.N == 500
    _check_against_matrix(res, mat, inv, baseline, "forecast_targets")
    assert a.rng_shared.integers(0, 2**62) == b.rng_shared.integers(0, 2**62)


def test_lockstep_refined_clones_go_through_the_independent_form(ctx, baseline):
    """n_hmc = 1: the D clones no longer share particles; one _indep call keyed by the clones' own
    streams summarises the matrix forecast_with_nowcasts returns for the same mode."""
    base, values, fwd, inv = _mirror_fixture()
    nd, fd = mc.days(40, 42), mc.days(42, 48)
    nows = [nc.TData(nd, list(values[-2:] * (1.0 + 0.05 * k)), transformation=fwd) for k in range(3)]
    a, b = base.clone(), base.clone()
    mat = nc.forecast_with_nowcasts(a, nows, fd, 200, inv_transformation=inv, n_hmc=1)
    res = nc.forecast_targets_with_nowcasts(b, nows, fd, MIRROR_TARGETS, 200, probs=[0.025, 0.5, 0.975],
                                            inv_transformation=inv, n_hmc=1, want_values=True)
    assert res.N == 600
    _check_against_matrix(res, mat, inv, baseline, "lockstep-refined clones")
    assert a.rng_shared.integers(0, 2**62) == b.rng_shared.integers(0, 2**62)

"""Energy score and sample CRPS of forecast paths without a device: the numpy fallback of
``autogp.ensemble_scores`` against the long double restatement (tests/ensemble_scores_reference.py),
the identities of the estimator, the vignette's ``crps`` transcribed literally, and the argument
checks of the two C entry points through the real library (they return before a device is needed).
Also what the GPU tests at large N stand on: the sorted closed form of a one-date pair sum against
the restatement's pair loop, the exact "lattice line" ensembles against the restatement (equal after
conversion) and against the fallback (bit for bit, N = 1,000), and the exactness condition of every
(N, direction, codes) row the GPU file scores."""
import ctypes as C
import os

import numpy as np
import pytest

from nowcastautogp_amd import _lib, autogp, nowcast
from nowcastautogp_amd._abi import NgpInvTransform, dptr, iptr
from tests import ensemble_scores_reference as E
from tests.ensemble_scores_reference import CASES, RTOL, make_paths, scores_ld, windows_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def close(got, want, scale=None):
    scale = np.abs(want) if scale is None else scale
    return np.all(np.abs(got - want) <= RTOL * scale)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-N{c[1]}-m{c[2]}-s{c[3]}-f{int(c[5])}")
def test_fallback_matches_long_double(case):
    kind, N, m, scale, shift, fair = case
    x, y = make_paths(kind, N, m, seed=N * 100 + m)
    win = windows_for(m)
    es, to, tp = scores_ld(x, y, win, scale, shift, fair)
    got = autogp.host_ensemble_scores(x, y, win, scale, shift, fair)
    assert not got["info"].any()
    assert close(got["term_obs"], to) and close(got["term_pair"], tp)
    assert close(got["es"], es, to + 0.5 * tp)
    # the same window given twice: the same bits
    assert got["es"][2] == got["es"][5]


@pytest.mark.parametrize("case", [c for c in CASES if c[1] >= 2] + [("lognormal", 1000, 3, 0, 0.0, True),
                                                                  ("lognormal", 1000, 3, 1, 0.5, True)],
                         ids=lambda c: f"{c[0]}-N{c[1]}-m{c[2]}-s{c[3]}")
def test_sorted_closed_form_matches_the_long_double_pairs_on_one_date_windows(case):
    """pair_sum_sorted is what judges one-date windows where the O(N^2) restatement cannot follow:
    long double against long double, so far inside RTOL (measured: at most 1e-18 relative)"""
    kind, N, m, scale, shift, _ = case
    x, y = make_paths(kind, N, m, seed=N * 100 + m)
    dates = sorted({0, m // 2, m - 1})
    obs, pair = E.sums_ld(x, y, [(j, j) for j in dates], scale, shift)
    obs2, pair2 = E.sums_one_date_ld(x, y, dates, scale, shift)
    assert obs2.dtype == E.LD and pair2.dtype == E.LD
    err = float(np.max(np.abs(pair2 - pair) / pair))
    print(f"{kind} N={N} scale={scale}: sorted form against the pair loop {err:.1e}")
    assert np.all(np.abs(pair2 - pair) <= 1e-17 * pair) and np.all(np.abs(obs2 - obs) <= 1e-17 * obs)


@pytest.mark.parametrize("codes", ["index", "range"])
@pytest.mark.parametrize("d", ["d34", "d4", "pm33"])
@pytest.mark.parametrize("N", [129, 300])
def test_line_ensembles_are_exact_in_the_long_double_restatement(N, d, codes):
    """the integer reference and the restatement that judges everything else agree to the bit: the
    sums of ``sums_ld``, converted, ARE the integer totals"""
    x, y, k, ky = E.make_line_paths(N, d, codes)
    win = E.LINE_WINDOWS[d]
    obs_q, pair_q = E.line_totals(k, ky, E.line_norms(E.LINE_D[d], win))
    obs, pair = E.sums_ld(x, y, win)
    assert obs.astype(np.float64).tolist() == [q / 4.0 for q in obs_q]
    assert pair.astype(np.float64).tolist() == [q / 4.0 for q in pair_q]
    if codes == "index":
        assert len(set(k.tolist())) == N          # no two paths tie
    # a pair dropped or counted twice moves the total by at least a quarter
    assert all(q > 0 for q in pair_q)


@pytest.mark.parametrize("row", E.LINE_GPU_ROWS + E.LINE_GRID_ROWS, ids=lambda r: f"N{r[0]}-{r[1]}-{r[2]}")
def test_every_exact_row_of_the_gpu_tests_keeps_the_exactness_condition(row):
    """make_line_paths and line_totals assert it in integer arithmetic; here it is seen to hold for
    each row, and the codes to be as large as it allows"""
    N, d, codes = row
    x, y, k, ky = E.make_line_paths(N, d, codes)
    norms = E.line_norms(E.LINE_D[d], E.LINE_WINDOWS[d])
    obs_q, pair_q = E.line_totals(k, ky, norms)
    span = int(k.max() - k.min())
    assert (span * max(norms)) ** 2 < 2 ** 53 and max(pair_q) < 2 ** 53 and max(obs_q) < 2 ** 53
    assert x.shape == (N, len(E.LINE_D[d])) and np.all(x > 0.0)
    if codes == "index":
        assert N <= E.LINE_INDEX_MAX_N and np.array_equal(np.sort(k), np.arange(N))
    else:
        K = E.line_K(N, max(norms))
        assert K & (K - 1) == 0 and not E.line_exact(N, 4 * K, max(norms)) and np.max(np.abs(k)) <= K
    if N == 1 << 20:
        assert E.line_K(N, 5) == 1024


@pytest.mark.parametrize("fair", [True, False])
@pytest.mark.parametrize("d,codes", [("d34", "index"), ("pm33", "index"), ("d34", "range")])
def test_fallback_is_exact_on_a_line_ensemble(d, codes, fair):
    """the numpy fallback is bound by the same argument as the device: bit for bit the integers"""
    x, y, k, ky = E.make_line_paths(1000, d, codes)
    win = E.LINE_WINDOWS[d]
    es, to, tp = E.line_scores(k, ky, E.line_norms(E.LINE_D[d], win), fair)
    got = autogp.host_ensemble_scores(x, y, win, 0, 0.0, fair)
    assert not got["info"].any()
    np.testing.assert_array_equal(got["term_obs"], to)
    np.testing.assert_array_equal(got["term_pair"], tp)
    np.testing.assert_array_equal(got["es"], es)


def vignette_crps(y, X):
    """docs/vignettes/getting-started.jl:689-702 of the reference, line by line"""
    n = len(X)
    term1 = np.mean(np.abs(X - y))
    term2 = np.mean([abs(X[i] - X[j]) for i in range(n) for j in range(i + 1, n)])
    return term1 - 0.5 * term2


def test_one_date_window_is_the_vignettes_crps_and_score_forecast_its_mean():
    x, y = make_paths("lognormal", 40, 5, seed=3)
    sc = autogp.ensemble_scores(x.T, y, scale="log")
    want = np.array([vignette_crps(np.log(y[j]), np.log(x[:, j])) for j in range(5)])
    assert np.allclose(sc.crps, want, rtol=1e-12, atol=0)
    assert sc.crps.shape == (5,) and sc.energy.shape == (1,) and not sc.device
    mean_crps, energy = nowcast.score_forecast(x.T, y, horizon=4)
    assert np.isclose(mean_crps, want[:4].mean(), rtol=1e-12)
    assert np.isclose(energy, autogp.ensemble_scores(x.T[:4], y[:4], [(0, 3)], "log").es[0], rtol=1e-14)
    with pytest.raises(AssertionError):
        nowcast.score_forecast(x.T, y, horizon=6)


def test_energy_score_of_a_window_of_several_dates_by_a_plain_double_loop():
    """independent of the fallback's and the restatement's blocks and masks: every pair i < k by
    hand, the Euclidean norm over the window from math.sqrt"""
    import math
    x, y = make_paths("lognormal", 23, 6, seed=8)
    j0, j1 = 1, 4
    u = [[math.log(x[i, j] + 0.5) for j in range(j0, j1 + 1)] for i in range(23)]
    v = [math.log(y[j] + 0.5) for j in range(j0, j1 + 1)]
    norm = lambda a, b: math.sqrt(sum((p - q) ** 2 for p, q in zip(a, b)))
    obs = sum(norm(ui, v) for ui in u) / 23
    pairs = [norm(u[i], u[k]) for i in range(23) for k in range(i + 1, 23)]
    assert len(pairs) == 23 * 22 // 2
    for fair, D in ((True, len(pairs)), (False, 23 * 23 / 2)):
        want = obs - 0.5 * sum(pairs) / D
        got = autogp.ensemble_scores(x.T, y, [(0, 0), (j0, j1)], "log", 0.5, fair)
        assert np.isclose(got.es[1], want, rtol=1e-13, atol=0)
        assert np.isclose(got.terms["term_pair"][1], sum(pairs) / D, rtol=1e-13, atol=0)
        ld = scores_ld(x, y, [(j0, j1)], 1, 0.5, fair)
        assert np.isclose(ld[0][0], want, rtol=1e-13, atol=0)


def test_one_date_window_equals_the_energy_score_with_m_1():
    x, y = make_paths("lognormal", 33, 4, seed=5)
    a = autogp.host_ensemble_scores(x, y, [(2, 2)])
    b = autogp.host_ensemble_scores(x[:, 2:3].copy(), y[2:3], [(0, 0)])
    for k in ("es", "term_obs", "term_pair"):
        assert a[k][0] == b[k][0]


def test_identical_paths_and_a_y_equal_to_every_path():
    rng = np.random.default_rng(0)
    row = 3.0 + rng.random(6)
    x = np.tile(row, (17, 1))
    y = row + np.array([0.3, -0.1, 0.0, 0.2, 0.4, -0.2])
    for scale in (0, 1):
        o = autogp.host_ensemble_scores(x, y, [(0, 5), (1, 1)], scale)
        s = np.log if scale else (lambda v: v)
        assert np.all(o["term_pair"] == 0.0)
        assert np.isclose(o["es"][0], np.linalg.norm(s(row) - s(y)), rtol=1e-14)
        assert np.isclose(o["es"][1], abs(s(row[1]) - s(y[1])), rtol=1e-14)
        z = autogp.host_ensemble_scores(x, row, [(0, 5), (1, 1)], scale)
        assert np.all(z["es"] == 0.0)


def test_v_statistic_is_the_fair_value_times_n_minus_1_over_n():
    x, y = make_paths("lognormal", 31, 3, seed=9)
    win = windows_for(3)
    f = autogp.host_ensemble_scores(x, y, win, fair=True)
    v = autogp.host_ensemble_scores(x, y, win, fair=False)
    assert np.allclose(v["term_pair"], f["term_pair"] * 30.0 / 31.0, rtol=1e-14, atol=0)
    assert np.array_equal(v["term_obs"], f["term_obs"])


def test_log_with_shift_0_on_paths_that_hold_0_flags_only_the_windows_that_meet_them():
    x, y = make_paths("lognormal", 20, 4, seed=1)
    x[3, 2] = 0.0
    sc = autogp.ensemble_scores(x.T, y, [(0, 1), (2, 2), (1, 3), (3, 3)], scale="log")
    assert list(sc.info) == [0, autogp.NGP_INFO_NOT_FINITE, autogp.NGP_INFO_NOT_FINITE, 0]
    assert np.isfinite(sc.es[[0, 3]]).all() and np.isnan(sc.es[[1, 2]]).all()
    assert np.isnan(sc.terms["term_obs"][1]) and np.isnan(sc.terms["term_pair"][2])


def test_finite_values_whose_squares_overflow_flag_their_windows():
    x, y = make_paths("lognormal", 20, 4, seed=1)
    x[3, 2], x[5, 2] = 1.0e200, np.finfo(np.float64).max
    sc = autogp.ensemble_scores(x.T, y, [(0, 1), (2, 2), (1, 3), (3, 3)])
    assert list(sc.info) == [0, autogp.NGP_INFO_NOT_FINITE, autogp.NGP_INFO_NOT_FINITE, 0]
    assert np.isfinite(sc.es[[0, 3]]).all()
    for a in (sc.es, sc.terms["term_obs"], sc.terms["term_pair"]):
        assert np.isnan(a[[1, 2]]).all()


def test_python_argument_checks():
    x, y = make_paths("lognormal", 5, 3, seed=2)
    for bad in (dict(windows=[(0, 3)]), dict(windows=[(2, 1)]), dict(windows=[]), dict(scale="sqrt"),
                dict(shift=-1.0), dict(shift=np.inf)):
        with pytest.raises(ValueError):
            autogp.ensemble_scores(x.T, y, **bad)
    with pytest.raises(ValueError):
        autogp.ensemble_scores(x.T, np.array([1.0, np.nan, 1.0]))
    with pytest.raises(ValueError):
        autogp.ensemble_scores(x.T, np.array([1.0, 0.0, 1.0]), scale="log")
    with pytest.raises(ValueError):
        autogp.ensemble_scores(x.T[:, :1], y, fair=True)


def test_the_abi_declares_and_binds_both_entry_points():
    header = open(os.path.join(ROOT, "include", "ngp.h"), encoding="utf-8").read()
    for name in ("ngp_ensemble_scores", "ngp_mixture_path_scores"):
        assert name in _lib.SYMBOLS and f"{name}(" in header
    for name in ("score_forecast", "forecast_scores_with_nowcasts"):
        assert name in nowcast.__all__
    assert hasattr(autogp.HipEngine, "ensemble_scores") and hasattr(autogp.HipEngine, "mixture_path_scores")


# ---- NGP_ERR_ARG through the real library: refused before a device is needed -------------------
NGP_ERR_ARG = -1


class EnsembleCall:
    def __init__(self):
        self.N, self.m, self.W = 4, 3, 2
        self.x = np.ones((4, 3))
        self.y = np.ones(3)
        self.win = np.array([[0, 0], [0, 2]], dtype=np.int32)
        self.scale, self.shift, self.fair = 0, 0.0, 1
        self.es = np.zeros(2)
        self.null = set()

    def p(self, name, ptr):
        return None if name in self.null else ptr

    def __call__(self, ctx=None):
        return _lib.load().ngp_ensemble_scores(
            ctx, self.N, self.m, self.p("x", dptr(self.x)), self.p("y", dptr(self.y)), self.scale,
            self.shift, self.fair, self.W, self.p("win", iptr(self.win)), self.p("es", dptr(self.es)),
            None, None, None)


@pytest.fixture(scope="module")
def lib():
    """the real library, built if need be: a missing or unloadable one is an error, not a skip"""
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def test_a_null_context_is_an_argument_error(lib):
    assert EnsembleCall()() == NGP_ERR_ARG


_FAKE = C.create_string_buffer(1 << 16)


def _bogus_ctx():
    """the "context" is a block of zeros: every call below is refused by the argument checks,
    which come before anything touches the context or a device"""
    return C.cast(_FAKE, C.c_void_p)


@pytest.mark.parametrize("change", [
    lambda c: c.null.add("x"), lambda c: c.null.add("y"), lambda c: c.null.add("win"),
    lambda c: c.null.add("es"), lambda c: setattr(c, "N", 0), lambda c: setattr(c, "m", 0),
    lambda c: setattr(c, "W", 0), lambda c: (setattr(c, "N", 1), setattr(c, "fair", 1)),
    lambda c: c.win.__setitem__((1, 1), 3), lambda c: c.win.__setitem__((0, 0), -1),
    lambda c: c.win.__setitem__((1, 0), 3), lambda c: setattr(c, "scale", 2),
    lambda c: setattr(c, "scale", -1), lambda c: setattr(c, "fair", 2),
    lambda c: setattr(c, "shift", -0.5), lambda c: setattr(c, "shift", float("nan")),
    lambda c: setattr(c, "shift", float("inf")), lambda c: c.y.__setitem__(1, np.nan),
    lambda c: c.y.__setitem__(1, np.inf),
    lambda c: (setattr(c, "scale", 1), c.y.__setitem__(2, 0.0)),
    lambda c: (setattr(c, "scale", 1), setattr(c, "shift", 0.5), c.y.__setitem__(2, -0.5)),
])
def test_malformed_ensemble_calls_are_argument_errors(lib, change):
    call = EnsembleCall()
    change(call)
    assert call(_bogus_ctx()) == NGP_ERR_ARG


class MixtureCall:
    def __init__(self):
        self.P, self.S, self.m, self.draws, self.indep, self.W = 2, 2, 3, 4, 0, 1
        self.w = np.full((2, 2), 0.5)
        self.mu = np.zeros((2, 2, 3))
        self.sigma = np.tile(np.eye(3), (2, 1, 1))
        self.seeds = np.array([7, 8], dtype=np.uint64)
        self.inv = NgpInvTransform(3, 0.3, 0.5, 1.0e4)
        self.y = np.ones(3)
        self.win = np.array([[0, 2]], dtype=np.int32)
        self.scale, self.shift, self.fair = 0, 0.0, 1
        self.es = np.zeros(1)
        self.null = set()

    def p(self, name, ptr):
        return None if name in self.null else ptr

    def __call__(self, ctx):
        return _lib.load().ngp_mixture_path_scores(
            ctx, self.P, self.S, self.m, self.p("w", dptr(self.w)), self.p("mu", dptr(self.mu)),
            self.p("sigma", dptr(self.sigma)), self.indep, self.draws,
            self.p("seeds", self.seeds.ctypes.data_as(C.POINTER(C.c_uint64))),
            self.p("inv", C.byref(self.inv)), self.p("y", dptr(self.y)), self.scale, self.shift,
            self.fair, self.W, self.p("win", iptr(self.win)), self.p("es", dptr(self.es)), None, None,
            None, None)


@pytest.mark.parametrize("change", [
    lambda c: c.null.add("w"), lambda c: c.null.add("mu"), lambda c: c.null.add("sigma"),
    lambda c: c.null.add("seeds"), lambda c: c.null.add("inv"), lambda c: c.null.add("y"),
    lambda c: c.null.add("win"), lambda c: c.null.add("es"), lambda c: setattr(c, "P", 0),
    lambda c: setattr(c, "S", 0), lambda c: setattr(c, "m", 0), lambda c: setattr(c, "draws", 0),
    lambda c: setattr(c, "W", 0), lambda c: setattr(c, "indep", 2),
    lambda c: (setattr(c, "S", 1), setattr(c, "draws", 1)),          # fair with one path
    lambda c: setattr(c.inv, "kind", 4), lambda c: setattr(c.inv, "lam", float("inf")),
    lambda c: setattr(c.inv, "offset", float("nan")), lambda c: setattr(c.inv, "cap", 0.0),
    lambda c: c.win.__setitem__((0, 1), 3), lambda c: setattr(c, "scale", 5),
    lambda c: setattr(c, "shift", -1.0), lambda c: c.y.__setitem__(0, np.nan),
    lambda c: (setattr(c, "scale", 1), c.y.__setitem__(0, 0.0)),
])
def test_malformed_mixture_calls_are_argument_errors(lib, change):
    call = MixtureCall()
    assert call(None) == NGP_ERR_ARG          # a null context
    change(call)
    assert call(_bogus_ctx()) == NGP_ERR_ARG

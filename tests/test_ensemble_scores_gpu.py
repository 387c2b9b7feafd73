"""Energy score and sample CRPS of paths on the device (ngp_ensemble_scores /
ngp_mixture_path_scores) at the shapes where the kernels can go wrong: N in {1, 2, 63, 64, 65, 257,
1000} (one tile, the tile and slice edges, several tiles, a ragged last tile), m in {1, 3, 33}
(one chunk of staged dates, three), the windows [0,0], [m-1,m-1], [0,m-1], two that overlap and one
given twice, both scales, both estimators, and one horizon beyond 2,048 dates (the second
accumulator of a squared distance).

Accuracy: both terms against the long double restatement (tests/ensemble_scores_reference.py) to
1e-12 relative each, es to 1e-12 (term_obs + term_pair / 2) — the floor include/ngp.h grants
ngp_mixture_crps; the summation bound (2,048 + m + 8) 2^-53 <= 2.6e-13 covers it.  Near-identical
paths (1e6 + 1e-3 z) are judged on the natural scale only: on the log scale their distances are
1e-9 of log(1e6), so ONE ulp between the device's log and numpy's moves a pair by 1e-6 of itself —
that would judge the log, not the score.

Edges: N in {127, 128, 129, 255, 256, 383, 384, 385} x m in {15, 16, 17, 32} with the windows
(0, m-1), (1, 16), (5, 20), (5, 21) where they fit (both sides of the 128-path tile and of the
16-date chunk, windows that do not start at date 0); m = 4,200 with windows of 2,047 | 2,048 | 2,049
and 4,095 | 4,096 | 4,097 dates (two moves to the second accumulator).

At scale, where the O(N^2 m) restatement cannot follow, two judgements:
  * exact — "lattice line" ensembles (tests/ensemble_scores_reference.py: x = a + (k / 4) d with
    integers k, d and integer window norms), on which every difference, square, square root and
    partial sum of the device is exactly representable, so every order of summation gives the
    same bits and the outputs must EQUAL what the host forms from the integer totals: tobytes(),
    no tolerance.  A tolerance cannot see one dropped or doubled pair at these sizes (2 / N^2 of the
    term); this sees a quarter of a unit in a total below 2^53 quarters.  N = 8,065 (64 tiles, 2,080
    slab rows: a second fold level with a ragged block of 32 rows), 20,000 (the workload: 12,403 rows,
    also every window alone, W = 1, against the call with all of them), 131,073 (1,025 tiles, the
    last of one path), 524,160 | 524,161 (the pair kernel's grid gets a second row), 524,289 (the obs
    slab folds twice, the pair slab three times, ragged at each) and 2^20 (the limit); fair and not,
    paths as drawn, sorted and permuted.  The 2^20 row found the pair kernel's launch asking for
    2^25 + 2^12 workgroups of 256 threads in one grid dimension — more than 2^32 threads, which a
    launch does not take: term_pair came back as 0.1036 for 853.6, with status 0.  The grid is cut
    into rows since.  A fold that rounds its block count down (tried once on a scratch build) fails
    every exact and long double test from 8,065 up and no test at N <= 1,000.
  * long double — lognormal paths at N = 8,065 (window (0, 1) by the restatement, 1.4 s on the
    CPU), 20,000 and 131,073 (one-date windows by the sorted closed form), both scales, at RTOL.
Measured on an MI355X, wall time of one exact call (upload, kernels, download), d = (3, 4) with
three windows / the 33-date vector with seven: N = 8,065: 0.3 / 1.1 ms; 20,000: 0.8 / 3.2 ms;
131,073: 24 / 105 ms; 524,289: 377 ms; 2^20 (one window of two dates): 628 ms.  Largest error of a
term against long double at the new sizes: 2.2e-16 (edges), 2.1e-16 (at scale), 1.9e-16 (m = 4,200).

Mixture form: ngp_mixture_path_scores against ngp_ensemble_scores of the numpy-transformed output of
ngp_mixture_sample / _indep for the same seeds, largest relative deviation of a term over the
windows; it may be 8 x BASELINE, BASELINE being the same deviation between the scores of that
sampler output and of the ``oracle_np`` restatement's paths through the same numpy transformation,
measured over the same cases in the same session.
Measured on an MI355X: BASELINE = 4.08e-16 (tolerance 3.26e-15); the new call's largest deviation
over the cases = 4.08e-16, over the mirror tests = 4.07e-16, on ``indep_s5`` with 1,613 draws per
scenario (N = 8,065: the pair slab folds twice) = 1.3e-16; the largest error of a term against
long double over the shapes of the first paragraph = 2.4e-16."""
import numpy as np
import pytest

import __graft_entry__ as ge
from nowcastautogp_amd import _lib, autogp
from nowcastautogp_amd import nowcast as nc
from tests import ensemble_scores_reference as E
from tests import mirror_contracts as mc
from tests import path_targets_reference as R

pytestmark = pytest.mark.gpu

NOT_FINITE = -3


@pytest.fixture(scope="module")
def ctx():
    ge.build()
    return _lib.Context(0)


_sums = {}


def reference(kind, N, m, scale, shift, fair):
    """(x, y, windows, (es, term_obs, term_pair)): the long double sums once per data set"""
    key = (kind, N, m, scale, shift)
    if key not in _sums:
        x, y = E.make_paths(kind, N, m, seed=1000 * N + m)
        win = E.windows_for(m)
        _sums[key] = (x, y, win, E.sums_ld(x, y, win, scale, shift))
    x, y, win, (obs, pair) = _sums[key]
    return x, y, win, E.scores_from_sums(obs, pair, N, fair)


def check(got, want, what):
    es, to, tp = want
    for name, g, w in (("term_obs", got["term_obs"], to), ("term_pair", got["term_pair"], tp)):
        err = np.max(np.abs(g - w) / np.where(w != 0.0, np.abs(w), 1.0))
        print(f"{what} {name}: largest relative error {err:.2e}")
        assert np.all(np.abs(g - w) <= E.RTOL * np.abs(w)), (what, name, g, w)
    assert np.all(np.abs(got["es"] - es) <= E.RTOL * (to + 0.5 * tp)), (what, got["es"], es)
    assert not got["info"].any()


@pytest.mark.parametrize("scale,shift", [(0, 0.0), (1, 0.5)])
@pytest.mark.parametrize("m", [1, 3, 33])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, 1000])
def test_terms_match_long_double(ctx, N, m, scale, shift):
    for fair in ([False, True] if N >= 2 else [False]):
        x, y, win, want = reference("lognormal", N, m, scale, shift, fair)
        got = ctx.ensemble_scores(x, y, win, scale, shift, fair)
        check(got, want, f"N={N} m={m} scale={scale} fair={int(fair)}")
        assert got["es"][2].tobytes() == got["es"][5].tobytes()        # the window given twice
    if N == 1:
        assert np.all(got["term_pair"] == 0.0)


@pytest.mark.parametrize("kind,N,m,scale,shift", [
    ("near_identical", 257, 3, 0, 0.0), ("near_identical", 130, 33, 0, 0.0),
    ("clamped", 257, 3, 0, 0.0), ("clamped", 130, 33, 0, 0.0), ("clamped", 257, 3, 1, 1.0),
])
def test_near_identical_and_clamped_paths_keep_their_distances(ctx, kind, N, m, scale, shift):
    """what a distance from Gram products loses: 1e-3 at a level of 1e6, and a third of the values
    clamped at exactly 0"""
    x, y, win, want = reference(kind, N, m, scale, shift, True)
    if kind == "clamped":
        assert 0.25 < np.mean(x == 0.0) < 0.45
    check(ctx.ensemble_scores(x, y, win, scale, shift, True), want, f"{kind} N={N} m={m} scale={scale}")


# ---- edges of the tile (128 paths) and of the staged chunk (16 dates) -------------------------------
_edge_sums = {}


def edge_windows(m):
    return [w for w in [(0, m - 1), (1, 16), (5, 20), (5, 21)] if w[1] < m]


@pytest.mark.parametrize("scale,shift", [(0, 0.0), (1, 0.5)])
@pytest.mark.parametrize("m", [15, 16, 17, 32])
@pytest.mark.parametrize("N", [127, 128, 129, 255, 256, 383, 384, 385])
def test_terms_match_long_double_on_both_sides_of_the_tile_and_chunk_edges(ctx, N, m, scale, shift):
    """one path short of a tile, a full one, one path into the next; windows of 15 | 16 | 17 dates
    from date 0 and of 16 | 17 dates that do not start there"""
    key = (N, m, scale)
    if key not in _edge_sums:
        x, y = E.make_paths("lognormal", N, m, seed=1000 * N + m)
        win = edge_windows(m)
        _edge_sums[key] = (x, y, win, E.sums_ld(x, y, win, scale, shift))
    x, y, win, (obs, pair) = _edge_sums[key]
    for fair in (False, True):
        got = ctx.ensemble_scores(x, y, win, scale, shift, fair)
        check(got, E.scores_from_sums(obs, pair, N, fair), f"edges N={N} m={m} scale={scale} fair={int(fair)}")


# ---- exact at scale: line ensembles against integers ------------------------------------------------
_line = {}


def line_case(N, d, codes):
    """(x, y, windows, k, k_y, norms), made once; the tests leave it unchanged"""
    key = (N, d, codes)
    if key not in _line:
        x, y, k, ky = E.make_line_paths(N, d, codes)
        win = E.LINE_WINDOWS[d]
        _line[key] = (x, y, win, k, ky, E.line_norms(E.LINE_D[d], win))
    return _line[key]


def assert_same_bits(got, want, what):
    es, to, tp = want
    assert not got["info"].any(), what
    for name, w in (("term_obs", to), ("term_pair", tp), ("es", es)):
        assert got[name].tobytes() == np.asarray(w).tobytes(), (what, name, got[name], w)
        np.testing.assert_array_equal(got[name], w)


@pytest.mark.parametrize("order", ["drawn", "sorted", "permuted"])
@pytest.mark.parametrize("row", E.LINE_GPU_ROWS, ids=lambda r: f"N{r[0]}-{r[1]}-{r[2]}")
def test_line_ensembles_are_scored_exactly_at_scale(ctx, row, order):
    """every pair counted once, no rounding anywhere: the integer reference bit for bit, whatever
    tile a path falls in.  8,065: a second fold level with a ragged block of 32 rows; 20,000: the
    workload; 131,073: 1,025 tiles, the last of one path; 524,289: two levels of the obs fold, three
    of the pair fold, ragged at each; 2^20: the limit (one window there: the structure is the point)"""
    import time
    N, d, codes = row
    x, y, win, k, ky, norms = line_case(*row)
    if N == 1 << 20:
        win, norms = win[2:], norms[2:]
    if order == "sorted":
        x = np.ascontiguousarray(x[np.argsort(k, kind="stable")])
    elif order == "permuted":
        x = np.ascontiguousarray(x[np.random.default_rng(N).permutation(N)])
    for fair in (True, False):
        t0 = time.perf_counter()
        got = ctx.ensemble_scores(x, y, win, 0, 0.0, fair)
        print(f"exact N={N} {d} {codes} {order} fair={int(fair)} W={len(win)}: {(time.perf_counter() - t0) * 1e3:.1f} ms")
        assert_same_bits(got, E.line_scores(k, ky, norms, fair), f"N={N} {d} {codes} {order} fair={int(fair)}")


@pytest.mark.parametrize("row", E.LINE_GRID_ROWS, ids=lambda r: f"N{r[0]}")
def test_line_ensembles_on_both_sides_of_the_pair_grids_second_row(ctx, row):
    """a launch takes fewer than 2^32 threads per dimension, so the pair kernel's grid is cut into
    rows: 524,160 paths are the last size with one row, 524,161 the first with two (the 2^20 row
    above has five, 524,289 two with an idle block at the end)"""
    x, y, win, k, ky, norms = line_case(*row)
    got = ctx.ensemble_scores(x, y, win, 0, 0.0, True)
    assert_same_bits(got, E.line_scores(k, ky, norms, True), f"N={row[0]} grid split")


@pytest.mark.parametrize("d,codes", [("d34", "index"), ("pm33", "index"), ("d34", "range")])
def test_a_window_alone_has_the_bits_it_has_among_others_at_the_workload_size(ctx, d, codes):
    """12,403 slab rows fold to 7 and then to 1: [row][W] indexing with W = 1 and with W > 1"""
    N = 20000
    x, y, win, k, ky, norms = line_case(N, d, codes)
    together = ctx.ensemble_scores(x, y, win, 0, 0.0, True)
    want = E.line_scores(k, ky, norms, True)
    assert_same_bits(together, want, f"N={N} {d} {codes} together")
    for i, w in enumerate(win):
        alone = ctx.ensemble_scores(x, y, [w], 0, 0.0, True)
        for name in ("es", "term_obs", "term_pair"):
            assert alone[name][0].tobytes() == together[name][i].tobytes(), (w, name)


# ---- long double at scale ---------------------------------------------------------------------------
_big = {}


@pytest.mark.parametrize("scale,shift", [(0, 0.0), (1, 0.5)])
@pytest.mark.parametrize("N", [8065, 20000, 131073])
def test_general_position_paths_match_long_double_at_multi_level_sizes(ctx, N, scale, shift):
    """lognormal paths, m = 2: the one-date windows against the sorted closed form in long double
    at every N, the window (0, 1) against the O(N^2) restatement where it can follow (8,065)"""
    key = (N, scale)
    if key not in _big:
        x, y = E.make_paths("lognormal", N, 2, seed=1000 * N + 2)
        obs, pair = E.sums_one_date_ld(x, y, [0, 1], scale, shift)
        win = [(0, 0), (1, 1)]
        if N == 8065:
            o2, p2 = E.sums_ld(x, y, [(0, 1)], scale, shift)
            obs, pair, win = np.concatenate([obs, o2]), np.concatenate([pair, p2]), win + [(0, 1)]
        _big[key] = (x, y, win, obs, pair)
    x, y, win, obs, pair = _big[key]
    for fair in (True, False):
        got = ctx.ensemble_scores(x, y, win, scale, shift, fair)
        check(got, E.scores_from_sums(obs, pair, N, fair), f"at scale N={N} scale={scale} fair={int(fair)}")


def test_a_horizon_beyond_4096_dates(ctx):
    """two moves to the second accumulator, and windows on both sides of one move and of two; the
    2,048-date window runs the short kernel alone and the LONG one beside a longer window: same bits"""
    N, m = 65, 4200
    x = np.exp(5.0 + 0.3 * np.random.default_rng(11).standard_normal((N, m)))
    y = np.full(m, np.exp(5.0))
    win = [(0, 2046), (0, 2047), (7, 2055), (0, 4094), (100, 4195), (3, 4099), (0, m - 1), (2100, 4147)]
    assert [b - a + 1 for a, b in win] == [2047, 2048, 2049, 4095, 4096, 4097, 4200, 2048]
    got = ctx.ensemble_scores(x, y, win, 1, 0.0, True)
    check(got, E.scores_ld(x, y, win, 1, 0.0, True), "m=4200")
    for i in (0, 1, 7):
        alone = ctx.ensemble_scores(x, y, [win[i]], 1, 0.0, True)
        for k in ("es", "term_obs", "term_pair"):
            assert alone[k][0].tobytes() == got[k][i].tobytes(), (i, k)


def test_a_horizon_beyond_2048_dates(ctx):
    """the squared distance moves to a second accumulator every 2,048 dates: accuracy of the long
    window, and a short window's bits are the same with and without a long one in the call"""
    N, m = 65, 2100
    x = np.exp(5.0 + 0.3 * np.random.default_rng(7).standard_normal((N, m)))
    y = np.full(m, np.exp(5.0))
    win = [(0, m - 1), (3, 40), (0, 2047), (10, 2058)]
    got = ctx.ensemble_scores(x, y, win, 1, 0.0, True)
    check(got, E.scores_ld(x, y, win, 1, 0.0, True), "m=2100")
    for i in (1, 2):
        alone = ctx.ensemble_scores(x, y, [win[i]], 1, 0.0, True)
        for k in ("es", "term_obs", "term_pair"):
            assert alone[k][0].tobytes() == got[k][i].tobytes(), (i, k)


def test_reproducible_and_independent_of_the_other_windows(ctx):
    x, y, win, want = reference("lognormal", 1000, 33, 1, 0.5, True)
    a = ctx.ensemble_scores(x, y, win, 1, 0.5, True)
    b = ctx.ensemble_scores(x, y, win, 1, 0.5, True)
    for k in ("es", "term_obs", "term_pair"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for i, w in enumerate(win):
        one = ctx.ensemble_scores(x, y, [w], 1, 0.5, True)
        for k in ("es", "term_obs", "term_pair"):
            assert one[k][0].tobytes() == a[k][i].tobytes(), (w, k)
    perm = np.random.default_rng(0).permutation(1000)
    check(ctx.ensemble_scores(np.ascontiguousarray(x[perm]), y, win, 1, 0.5, True), want, "permuted paths")


def test_log_with_shift_0_on_paths_that_hold_0(ctx):
    x, y = E.make_paths("clamped", 130, 5, seed=4)
    x[:, 0] += 1.0
    x[:, 4] += 1.0                 # dates 1 .. 3 hold zeros
    assert np.all(x[:, [0, 4]] > 0.0) and all(np.any(x[:, j] == 0.0) for j in (1, 2, 3))
    win = [(0, 0), (0, 4), (4, 4), (2, 3), (0, 0)]
    got = ctx.ensemble_scores(x, y, win, 1, 0.0, True)
    assert got["info"].tolist() == [0, NOT_FINITE, 0, NOT_FINITE, 0]
    for k in ("es", "term_obs", "term_pair"):
        assert np.isnan(got[k][[1, 3]]).all() and np.isfinite(got[k][[0, 2, 4]]).all()
    clean = ctx.ensemble_scores(x, y, [(0, 0), (4, 4)], 1, 0.0, True)
    assert clean["es"].tobytes() == got["es"][[0, 2]].tobytes()
    x[7, 4] = np.nan                # a NaN path value, natural scale
    got = ctx.ensemble_scores(x, y, win, 0, 0.0, False)
    assert got["info"].tolist() == [0, NOT_FINITE, NOT_FINITE, 0, 0]


def test_finite_values_whose_squares_overflow_flag_their_windows(ctx):
    """1e200 and the largest finite double (what a Box-Cox image is capped at) are finite on the
    natural scale; their squared differences are not"""
    x, y = E.make_paths("lognormal", 130, 4, seed=6)
    x[3, 2], x[129, 2] = 1.0e200, np.finfo(np.float64).max
    win = [(0, 1), (2, 2), (1, 3), (3, 3)]
    got = ctx.ensemble_scores(x, y, win, 0, 0.0, True)
    assert got["info"].tolist() == [0, NOT_FINITE, NOT_FINITE, 0]
    for k in ("es", "term_obs", "term_pair"):
        assert np.isnan(got[k][[1, 2]]).all() and np.isfinite(got[k][[0, 3]]).all()
    host = autogp.host_ensemble_scores(x, y, win, 0, 0.0, True)
    assert host["info"].tolist() == got["info"].tolist()


def test_limits_and_argument_errors(ctx):
    x, y = np.ones((4, 3)), np.ones(3)

    def status(f, *a):
        try:
            f(*a)
        except _lib.NgpError as e:
            return e.status
        return 0

    assert status(ctx.ensemble_scores, x, y, [(0, 2)]) == 0
    assert status(ctx.ensemble_scores, x, y, [(0, 3)]) == -1
    assert status(ctx.ensemble_scores, x, y, [(0, 2)], 2) == -1
    assert status(ctx.ensemble_scores, x[:1], y, [(0, 2)], 0, 0.0, True) == -1
    assert status(ctx.ensemble_scores, np.ones(((1 << 20) + 1, 1)), np.ones(1), [(0, 0)]) == -3
    assert status(ctx.ensemble_scores, x, y, [(0, 0)] * 4097) == -3
    assert status(ctx.ensemble_scores, np.ones((2, 65536)), np.ones(65536), [(0, 0)]) == -3


# ---- the mixture form ----------------------------------------------------------------------------
MIX_CASES = ["n63_exp", "n257_boxcox_neg", "shared_s5", "indep_s5", "indep_s2_m33"]
_mix = {}


def mix_case(ctx, name, draws=None):
    """(case, y, windows, scores of the sampler's transformed output, scores of the restatement's
    paths, the new call's result) — each computed once per session; ``draws``: the case with that
    many draws per scenario instead of its own"""
    if draws is not None:
        name = (name, draws)
    if name not in _mix:
        c = R.make_case(name) if draws is None else dict(R.make_case(name[0]), draws=draws)
        g = R.inv_numpy(c["inv"])
        v_ref = g(R.sample_paths(c["w"], c["mu"], c["sigma"], c["draws"], c["seed"]))
        if np.isscalar(c["seed"]):
            xs = ctx.mixture_sample(c["w"], c["mu"], c["sigma"], c["draws"], c["seed"])[0]
        else:
            xs = ctx.mixture_sample_indep(c["w"], c["mu"], c["sigma"], c["draws"], c["seed"])[0]
        v_dev = g(xs.reshape(-1, xs.shape[-1]))
        m = v_ref.shape[1]
        y = 1.1 * np.median(v_ref, axis=0) + 0.05
        win = E.windows_for(m)
        a = ctx.ensemble_scores(v_dev, y, win, 1, 1.0, True)
        b = ctx.ensemble_scores(v_ref, y, win, 1, 1.0, True)
        o = ctx.mixture_path_scores(c["w"], c["mu"], c["sigma"], c["draws"], c["seed"], c["inv"], y, win,
                                    1, 1.0, True)
        _mix[name] = (c, y, win, a, b, o)
    return _mix[name]


def term_deviation(a, b):
    return max(float(np.max(np.abs(a[k] - b[k]) / np.abs(b[k]))) for k in ("term_obs", "term_pair"))


@pytest.fixture(scope="module")
def baseline(ctx):
    worst = 0.0
    for name in MIX_CASES:
        _, _, _, a, b, _ = mix_case(ctx, name)
        worst = max(worst, term_deviation(a, b))
    print(f"BASELINE (scores of sampler + numpy vs of the restatement's paths) = {worst:.3e}")
    assert worst > 0.0
    return worst


@pytest.mark.parametrize("name", MIX_CASES)
def test_mixture_form_scores_the_samplers_paths(ctx, baseline, name):
    c, y, win, a, _, o = mix_case(ctx, name)
    assert not o["info"].any() and not o["chol_info"].any()
    assert o["chol_info"].shape == (np.shape(c["w"]) if not np.isscalar(c["seed"]) else (c["w"].shape[1],))
    dev = term_deviation(o, a)
    print(f"{name}: deviation {dev:.3e}, baseline {baseline:.3e}, tolerance {8 * baseline:.3e}")
    assert dev <= 8.0 * baseline, (dev, baseline)
    assert np.all(np.abs(o["es"] - a["es"]) <= 8.0 * baseline * (a["term_obs"] + 0.5 * a["term_pair"]))


def test_mixture_form_at_a_size_whose_pair_slab_folds_twice(ctx, baseline):
    """``indep_s5`` with 1,613 draws per scenario: N = 8,065, the smallest N with a second fold
    level; judged as the cases above are, by the same BASELINE"""
    c, y, win, a, _, o = mix_case(ctx, "indep_s5", draws=1613)
    assert c["w"].shape[0] * c["draws"] == 8065
    assert not o["info"].any() and not o["chol_info"].any()
    dev = term_deviation(o, a)
    print(f"indep_s5 x 1613 draws: deviation {dev:.3e}, baseline {baseline:.3e}, tolerance {8 * baseline:.3e}")
    assert dev <= 8.0 * baseline, (dev, baseline)
    assert np.all(np.abs(o["es"] - a["es"]) <= 8.0 * baseline * (a["term_obs"] + 0.5 * a["term_pair"]))


def test_a_failed_component_of_positive_weight_makes_everything_nan(ctx):
    c, y, win, _, _, good = mix_case(ctx, "shared_s5")
    bad_sg = c["sigma"].copy()
    bad_sg[2] = -np.eye(7)
    args = (c["draws"], c["seed"], c["inv"], y, win, 1, 1.0, True)
    o = ctx.mixture_path_scores(c["w"], c["mu"], bad_sg, *args)
    assert o["chol_info"].tolist() == [0, 0, 1]
    for k in ("es", "term_obs", "term_pair"):
        assert np.isnan(o[k]).all()
    assert np.all(o["info"] == NOT_FINITE)
    w0 = c["w"].copy()
    w0[:, 2] = 0.0
    w0 /= w0.sum(axis=1, keepdims=True)
    a = ctx.mixture_path_scores(w0, c["mu"], bad_sg, *args)
    b = ctx.mixture_path_scores(w0, c["mu"], c["sigma"], *args)
    assert a["chol_info"].tolist() == [0, 0, 1] and not b["chol_info"].any() and not a["info"].any()
    for k in ("es", "term_obs", "term_pair"):
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- the mirror ------------------------------------------------------------------------------------
def _fitted(n=40, n_particles=8):
    eng = autogp.HipEngine(0)
    rng = np.random.default_rng(n)
    values = 12.0 + 4.0 * np.sin(np.arange(n) / 5.0) + rng.random(n)
    fwd, inv = nc.get_transformations("boxcox", values)
    base = mc.fitted(eng, values=[float(fwd(v)) for v in values], seed=11, n_particles=n_particles)
    return eng, base, values, fwd, inv


@pytest.mark.parametrize("n_hmc", [0, 1])
def test_forecast_scores_with_nowcasts_scores_the_matrix_forecast_with_nowcasts_returns(ctx, baseline, n_hmc):
    """n_hmc = 0: shared components, one seed; n_hmc = 1: lockstep-refined clones, the independent
    form.  Same snapshot and seed, P = 8, D = 3, m = 6."""
    eng, base, values, fwd, inv = _fitted()
    nd, fd = mc.days(40, 42), mc.days(42, 48)
    nows = [nc.TData(nd, list(values[-2:] * (1.0 + 0.05 * k)), transformation=fwd) for k in range(3)]
    y = 12.0 + np.arange(6.0)
    a, b = base.clone(), base.clone()
    mat = nc.forecast_with_nowcasts(a, nows, fd, 200, inv_transformation=inv, n_hmc=n_hmc)
    res = nc.forecast_scores_with_nowcasts(b, nows, fd, y, 200, inv_transformation=inv, n_hmc=n_hmc,
                                           shift=1.0)
    assert res.device and not res.info.any()
    want = autogp.ensemble_scores(mat, y, None, "log", 1.0, True, eng)
    dev = max(float(np.max(np.abs(res.terms[k] - want.terms[k]) / want.terms[k])) for k in res.terms)
    print(f"mirror n_hmc={n_hmc}: deviation {dev:.3e} (tolerance {8 * baseline:.3e})")
    assert dev <= 8.0 * baseline
    mean_crps, energy = nc.score_forecast(mat, y, shift=1.0, engine=eng)
    assert abs(mean_crps - res.crps.mean()) <= 8.0 * baseline * want.terms["term_obs"].max()
    assert abs(energy - res.energy[0]) <= 8.0 * baseline * want.terms["term_obs"].max()
    assert a.rng_shared.integers(0, 2**62) == b.rng_shared.integers(0, 2**62)


def test_score_forecast_on_draws_made_with_hmc_before_every_draw(ctx):
    """forecast_n_hmc = 1 has no single mixture: its draws come back and are scored from the matrix,
    on the device as by the numpy fallback"""
    eng, base, values, fwd, inv = _fitted(n=40, n_particles=3)
    mat = nc.forecast(base, mc.days(40, 44), 12, inv_transformation=inv, forecast_n_hmc=1)
    y = np.array([12.0, 13.0, 14.0, 13.5])
    dev_scores = nc.score_forecast(mat, y, shift=1.0, engine=eng)
    host_scores = nc.score_forecast(mat, y, shift=1.0)
    assert np.allclose(dev_scores, host_scores, rtol=1e-12, atol=0.0)

"""Long double restatement of the energy score / sample CRPS of include/ngp.h ("scores of the
paths themselves") and the cases the CPU and GPU tests share.

    term_obs  = (1 / N) sum_i |u_i - v|       term_pair = (1 / D) sum_(i < k) |u_i - u_k|
    es        = term_obs - term_pair / 2      D = N (N - 1) / 2 (fair) or N^2 / 2

u = s(x), v = s(y) are taken in float64 — the values the library scores (numpy's log; the library's
log may differ from it by an ulp, which moves a term by far less than the tolerance) — and every
difference, square, square root and sum from there on runs in numpy ``longdouble``, the pairs in
blocks of rows so that N^2 numbers are never held at once.

That is O(N^2 m).  For the sizes it cannot reach: ``pair_sum_sorted`` / ``sums_one_date_ld``, the
long double sums of one-date windows in O(N log N), and the exact "lattice line" ensembles
(``make_line_paths``, ``line_scores``), whose scores are integers over 4 N and 4 D and which the
device, the fallback and the restatement must each reproduce bit for bit."""
import numpy as np

LD = np.longdouble
RTOL = 1e-12          # per term; es: RTOL * (term_obs + term_pair / 2)


def sums_ld(x, y, windows, scale=0, shift=0.0):
    """x [N, m] paths, y [m], windows [(j0, j1)] -> (sum_i |u_i - v|, sum_(i < k) |u_i - u_k|) per
    window as longdouble arrays; NaN for a window that holds a value that is not finite on the
    score scale.  A window that repeats is computed once."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    N = x.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (np.log(x + shift) if scale == 1 else x).astype(LD)
        v = (np.log(y + shift) if scale == 1 else y).astype(LD)
    rows = max(1, (1 << 20) // N)
    idx = np.arange(N)
    done = {}
    for j0, j1 in windows:
        if (j0, j1) in done:
            continue
        uw = u[:, j0:j1 + 1]
        if not np.all(np.isfinite(uw.astype(np.float64))):
            done[(j0, j1)] = (LD(np.nan), LD(np.nan))
            continue
        obs = np.sqrt(((uw - v[j0:j1 + 1]) ** 2).sum(axis=1)).sum()
        total = LD(0)
        for a in range(0, N, rows):
            blk = uw[a:a + rows]
            d2 = np.zeros((blk.shape[0], N), dtype=LD)
            for j in range(uw.shape[1]):
                df = blk[:, j][:, None] - uw[:, j][None, :]
                d2 += df * df
            total += np.sqrt(d2)[idx[None, :] > idx[a:a + rows][:, None]].sum()      # i < k only
        done[(j0, j1)] = (obs, total)
    return (np.array([done[tuple(w)][0] for w in windows], dtype=LD),
            np.array([done[tuple(w)][1] for w in windows], dtype=LD))


def scores_from_sums(obs, pair, N, fair=True):
    """(es, term_obs, term_pair) as float64 arrays from the sums of ``sums_ld``"""
    D = LD(N) * LD(N - 1) / 2 if fair else LD(N) * LD(N) / 2
    to = obs / LD(N)
    tp = pair / D
    return (to - tp / 2).astype(np.float64), to.astype(np.float64), tp.astype(np.float64)


def scores_ld(x, y, windows, scale=0, shift=0.0, fair=True):
    obs, pair = sums_ld(x, y, windows, scale, shift)
    return scores_from_sums(obs, pair, np.asarray(x).shape[0], fair)


def pair_sum_sorted(u):
    """sum_(i < k) |u_i - u_k| of ONE date's values u [N] (float64, already on the score scale) in
    longdouble, in O(N log N): sum_r (2 r - N + 1) u_(r) over the sorted values.  The coefficients
    add up to 0, so the middle value is taken off first: the terms are then of the size of the
    spread, not of the level."""
    s = np.sort(np.asarray(u, dtype=np.float64)).astype(LD)
    N = s.size
    coef = (2 * np.arange(N, dtype=np.int64) - (N - 1)).astype(LD)
    return (coef * (s - s[N // 2])).sum()


def sums_one_date_ld(x, y, dates, scale=0, shift=0.0):
    """what ``sums_ld`` gives for the windows [(j, j) for j in dates], at any N: the obs sums
    directly, the pair sums from ``pair_sum_sorted``; u and v taken as ``sums_ld`` takes them"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    u = np.log(x + shift) if scale == 1 else x
    v = np.log(y + shift) if scale == 1 else y
    assert np.all(np.isfinite(u[:, list(dates)]))
    obs = [np.abs(u[:, j].astype(LD) - LD(v[j])).sum() for j in dates]
    return np.array(obs, dtype=LD), np.array([pair_sum_sorted(u[:, j]) for j in dates], dtype=LD)


def windows_for(m):
    """first date, last date, whole horizon, two overlapping windows, and the whole horizon again"""
    a, b = (0, (2 * m) // 3), (m // 3, m - 1)
    return [(0, 0), (m - 1, m - 1), (0, m - 1), a, b, (0, m - 1)]


def make_paths(kind, N, m, seed):
    """paths [N, m] on the original scale (positive unless the kind says otherwise) and y [m]"""
    rng = np.random.default_rng(seed)
    if kind == "lognormal":          # counts of a few hundred with a common trend
        x = np.exp(5.0 + 0.3 * rng.standard_normal((N, m)) + 0.1 * np.arange(m))
        y = np.exp(5.0 + 0.1 * np.arange(m)) * (1.0 + 0.05 * rng.standard_normal(m))
    elif kind == "near_identical":   # 1e6 + 1e-3 z: a Gram-product distance has nothing left
        x = 1.0e6 + 1.0e-3 * rng.standard_normal((N, m))
        y = 1.0e6 + 1.0e-3 * rng.standard_normal(m)
    elif kind == "clamped":          # Box-Cox paths (lam = 0.3), a third of the values clamped at exactly 0
        z = 1.2 * rng.standard_normal((N, m)) + 0.113          # g(z) <= 0 for z <= -0.404: a third
        x = np.maximum(np.maximum(0.3 * z + 1.0, 1e-10) ** (1.0 / 0.3) - 0.65, 0.0)
        y = np.full(m, 0.8)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(x), np.abs(y)


# ---- exact "lattice line" ensembles ---------------------------------------------------------------
# x[i, j] = a_j + (k_i / 4) d_j with integers k_i, d_j; y on the same line at k_y.  Over a window
# whose sum of d_j^2 is a perfect square n^2, |u_i - u_k| = |k_i - k_k| n / 4.  On the natural scale
# every step of the device is then exact in binary64: a difference is a multiple of 1/4 below 2^53
# quarters, a square and every partial sum of squares is an integer number of sixteenths at most
# (max |k_i - k_k| n)^2 < 2^53, the square root is that of a perfect square (IEEE: exact), and every
# partial sum of distances is a number of quarters at most the total < 2^53.  Sums of exactly
# representable terms whose partial sums are all exactly representable give the same bits in every
# order — so the device's totals ARE the integers below, whatever its tiles, masks and folds, and a
# pair that is dropped or counted twice changes them.
LINE_D = {
    "d34": [3, 4],
    "d4": [1, -1, 1, 1],
    # 33 dates of +-1: a window of n^2 dates has norm n
    "pm33": [1, -1, -1, 1, 1, 1, -1, 1, -1, -1, 1, -1, 1, 1, -1, -1, 1,
             -1, 1, 1, 1, -1, -1, 1, -1, 1, -1, -1, 1, 1, -1, 1, 1],
}
LINE_WINDOWS = {
    "d34": [(0, 0), (1, 1), (0, 1)],                                     # norms 3, 4, 5
    "d4": [(0, 3), (2, 2), (0, 3)],                                      # norms 2, 1, 2
    # 1, 4, 9, 16, 16, 25, 25 dates, across the edges of the 16-date chunks
    "pm33": [(7, 7), (14, 17), (12, 20), (5, 20), (16, 31), (8, 32), (0, 24)],
}
LINE_INDEX_MAX_N = 131073


def line_norms(d, windows):
    """the integer Euclidean norm of d over each window; asserts that it is one"""
    out = []
    for j0, j1 in windows:
        s = sum(int(v) * int(v) for v in d[j0:j1 + 1])
        n = int(np.sqrt(s) + 0.5)
        assert n * n == s, (j0, j1, s)
        out.append(n)
    return out


def line_exact(N, kspan, norm_max):
    """the exactness condition, in integer arithmetic: kspan >= max |k_i - k_k|.  (kspan norm)^2 is
    the largest squared distance in sixteenths, kspan N^2 / 2 norm bounds the largest total in
    quarters (the pairs; the obs total, at most kspan N norm, is far below it)."""
    return (kspan * norm_max) ** 2 < 2 ** 53 and kspan * N * N * norm_max < 2 ** 54


def line_K(N, norm_max):
    """the largest power of two K such that codes in [-K, K] keep ``line_exact``"""
    K = 1
    while line_exact(N, 4 * K, norm_max):
        K *= 2
    assert line_exact(N, 2 * K, norm_max)
    return K


def make_line_paths(N, d, codes, K=None, seed=0):
    """-> x [N, m], y [m], k [N] int64, k_y: the line ensemble of direction d (a LINE_D name).
    codes "range": k_i uniform integers in [-K, K] (K None: ``line_K``); "index": k a fixed
    permutation of 0 .. N - 1, so that no two paths tie (N <= LINE_INDEX_MAX_N).  Asserts the
    exactness condition for the windows LINE_WINDOWS[d]."""
    dv = np.array(LINE_D[d], dtype=np.int64)
    norm_max = max(line_norms(LINE_D[d], LINE_WINDOWS[d]))
    rng = np.random.default_rng(seed + 7919 * N)
    if codes == "index":
        assert N <= LINE_INDEX_MAX_N
        k = rng.permutation(N).astype(np.int64)
        ky, kspan = N // 3, N - 1
    else:
        assert codes == "range"
        K = line_K(N, norm_max) if K is None else int(K)
        k = rng.integers(-K, K + 1, N).astype(np.int64)
        ky, kspan = K // 5 + 1, 2 * K
    assert line_exact(N, kspan, norm_max), (N, d, codes, kspan)
    a = np.float64(kspan + 8)                    # a_j + (k / 4) d_j >= a - kspan > 0 (|d_j| <= 4)
    assert int(np.max(np.abs(dv))) <= 4 and float(a) + kspan < 2.0 ** 50       # quarters of it exact
    x = a + (k[:, None].astype(np.float64) / 4.0) * dv[None, :].astype(np.float64)
    y = a + (np.float64(ky) / 4.0) * dv.astype(np.float64)
    assert np.all(x > 0.0) and np.all((x * 4.0) == np.rint(x * 4.0))
    return np.ascontiguousarray(x), y, k, ky


def line_totals(k, ky, norms):
    """(sum_i |k_i - k_y| n, sum_(i < k) |k_i - k_k| n) per window norm n, in quarters, as Python
    integers: the pairs from the sorted closed form sum_r (2 r - N + 1) k_(r), all in int64"""
    k = np.asarray(k, dtype=np.int64)
    N = k.size
    srt = np.sort(k)
    assert int(np.max(np.abs(srt))) * 2 * N * N < 2 ** 63
    pair = int(((2 * np.arange(N, dtype=np.int64) - (N - 1)) * srt).sum())
    obs = int(np.abs(k - np.int64(ky)).sum())
    for n in norms:
        assert 0 <= obs * n < 2 ** 53 and 0 <= pair * n < 2 ** 53
    return [obs * n for n in norms], [pair * n for n in norms]


def line_scores(k, ky, norms, fair):
    """(es, term_obs, term_pair), float64 [W], formed from the exact totals as the host forms them
    from the device's: the bits ``ngp_ensemble_scores`` must return"""
    N = len(k)
    obs, pair = line_totals(k, ky, norms)
    D = 0.5 * N * (N - 1) if fair else 0.5 * N * N
    to = np.array([np.float64(o) / 4.0 for o in obs]) / np.float64(N)
    tp = np.array([np.float64(p) / 4.0 for p in pair]) / np.float64(D)
    return to - 0.5 * tp, to, tp


# (N, direction, codes) of the exact GPU tests; the CPU suite asserts the condition for each
LINE_GPU_ROWS = [
    (8065, "d34", "index"), (8065, "pm33", "index"),
    (20000, "d34", "index"), (20000, "pm33", "index"), (20000, "d34", "range"),
    (131073, "d34", "index"), (131073, "pm33", "index"),
    (524289, "d34", "range"),
    (1 << 20, "d34", "range"),
]
# both sides of the size from which the pair kernel's grid has more than one row (4,095 | 4,096 tiles:
# 8,386,560 | 8,390,656 tile pairs against 2^23 workgroups per row)
LINE_GRID_ROWS = [(524160, "d34", "range"), (524161, "d34", "range")]


# (kind, N, m, scale, shift, fair): sizes around the tile (128) and slice (256) edges kept small
CASES = [
    ("lognormal", 2, 1, 0, 0.0, True),
    ("lognormal", 1, 3, 0, 0.0, False),
    ("lognormal", 63, 3, 1, 0.0, True),
    ("lognormal", 65, 33, 1, 0.5, False),
    ("lognormal", 257, 3, 0, 0.0, True),
    ("near_identical", 129, 3, 0, 0.0, True),
    ("near_identical", 64, 33, 1, 0.0, False),
    ("clamped", 130, 3, 0, 0.0, True),
    ("clamped", 257, 3, 1, 1.0, True),
]

"""Long double restatement of the energy score / sample CRPS of include/ngp.h ("scores of the
paths themselves") and the cases the CPU and GPU tests share.

    term_obs  = (1 / N) sum_i |u_i - v|       term_pair = (1 / D) sum_(i < k) |u_i - u_k|
    es        = term_obs - term_pair / 2      D = N (N - 1) / 2 (fair) or N^2 / 2

u = s(x), v = s(y) are taken in float64 — the values the library scores (numpy's log; the library's
log may differ from it by an ulp, which moves a term by far less than the tolerance) — and every
difference, square, square root and sum from there on runs in numpy ``longdouble``, the pairs in
blocks of rows so that N^2 numbers are never held at once."""
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

"""Restatement of the trajectory targets (include/ngp.h "trajectory targets") for the tests:
``oracle_np.mixture_sample`` draws, numpy inverse transformation, the functionals, ``np.sort``.
Written from the header's text, independent of ``autogp.path_targets``' host path — the CPU tests
hold the two against each other.  Also the shapes the GPU tests run (``CASES``), kept here so that
the CPU suite can check what it must about them without a device."""
import math

import numpy as np

from oracle import oracle_np

IDENTITY, EXP, LOGISTIC100, BOXCOX = 0, 1, 2, 3
SUM, MAX, DIFF, ARGMAX, EXCEED = 0, 1, 2, 3, 4
REAL = (SUM, MAX, DIFF)
FMAX = np.finfo(np.float64).max


def inv_numpy(inv):
    """g of an ``ngp_inv_transform`` (kind, lam, offset, cap), elementwise on arrays."""
    kind, lam, offset, cap = inv

    def g(x):
        x = np.asarray(x, dtype=np.float64)
        with np.errstate(all="ignore"):
            if kind == IDENTITY:
                r = x.copy()
            elif kind == EXP:
                r = np.maximum(np.exp(x) - offset, 0.0)
            elif kind == LOGISTIC100:
                r = np.maximum(100.0 / (1.0 + np.exp(-x)) - offset, 0.0)
            else:
                base = lam * x + 1.0
                if lam > 0:
                    r = np.maximum(base, 1.0e-10) ** (1.0 / lam) - offset
                elif lam < 0:
                    pw = np.where(base > 0, base, 1.0) ** (1.0 / lam)
                    r = np.where(base > 1.0e-10, pw - offset,
                                 np.where(base <= 0, 0.0, np.minimum(pw, cap) - offset))
                else:
                    r = np.exp(x) - offset
                r = np.maximum(r, 0.0)
                r = np.where(np.isfinite(r), r, FMAX)
        return r + 0.0
    return g


def rank(p, N):
    """k = clamp((int64) ceil(p * (double) N), 1, N)"""
    return min(max(int(math.ceil(float(p) * float(N))), 1), N)


def sample_paths(w, mu, sigma, draws, seed):
    """[N, m]: the paths of ngp_mixture_sample (one seed) / _indep (S seeds), path (s, d) at s draws + d."""
    w, mu, sigma = (np.asarray(a, dtype=np.float64) for a in (w, mu, sigma))
    if np.isscalar(seed):
        out, _ = oracle_np.mixture_sample(w, mu, sigma, draws, int(seed))
    else:
        out = np.stack([oracle_np.mixture_sample(w[s:s + 1], mu[s][:, None, :], sigma[s], draws,
                                                 int(seed[s]))[0][0] for s in range(w.shape[0])])
    return out.reshape(-1, out.shape[-1])


def functionals(v, targets):
    """values [T, N] of the paths v [N, m] (already on the original scale)"""
    out = np.empty((len(targets), v.shape[0]))
    for t, (kind, j0, j1, thr) in enumerate(targets):
        win = v[:, j0:j1 + 1]
        if kind == SUM:
            acc = np.zeros(v.shape[0])
            for j in range(j0, j1 + 1):         # ascending, as the header says
                acc += v[:, j]
            out[t] = acc
        elif kind == MAX:
            out[t] = win.max(axis=1)
        elif kind == DIFF:
            out[t] = v[:, j1] - v[:, j0]
        elif kind == ARGMAX:
            out[t] = j0 + win.argmax(axis=1)    # first index of the maximum
        else:
            out[t] = (win > thr).any(axis=1)
    return out + 0.0


def summaries(values, targets, probs, m):
    T, N = values.shape
    q = np.full((T, len(probs)), np.nan)
    count = np.zeros(T, dtype=np.int64)
    hist = np.zeros((T, m), dtype=np.int64)
    for t, (kind, j0, j1, thr) in enumerate(targets):
        if kind in REAL:
            srt = np.sort(values[t])
            q[t] = [srt[rank(p, N) - 1] for p in probs]
            count[t] = np.count_nonzero(values[t] > thr)
        elif kind == ARGMAX:
            hist[t] = np.bincount(values[t].astype(np.int64), minlength=m)
        else:
            count[t] = np.count_nonzero(values[t] == 1.0)
    return dict(q=q, mean=values.sum(axis=1) / N, count=count, hist=hist)


def restate(w, mu, sigma, draws, seed, inv, targets, probs):
    v = inv_numpy(inv)(sample_paths(w, mu, sigma, draws, seed))
    values = functionals(v, targets)
    return dict(summaries(values, targets, probs, v.shape[1]), values=values, v=v)


def fragile(v, targets, inv, rel=1e-9):
    """[T, N] bool: paths whose ARGMAX / EXCEED value a rounding error of the path could change —
    the window's two largest values, or its maximum and thr or a clamp value, closer than ``rel``
    of the window's scale."""
    clamps = [0.0] if inv[0] != IDENTITY else []
    if inv[0] == BOXCOX:
        clamps += [inv[3] - inv[2], FMAX]
    out = np.zeros((len(targets), v.shape[0]), dtype=bool)
    for t, (kind, j0, j1, thr) in enumerate(targets):
        if kind in REAL:
            continue
        win = v[:, j0:j1 + 1]
        scale = float(np.max(np.abs(win)))
        top = np.sort(win, axis=1)
        if win.shape[1] > 1:
            out[t] |= (top[:, -1] - top[:, -2]) < rel * scale
        near = [thr] if kind == EXCEED else []
        for c in near + clamps:
            out[t] |= np.abs(top[:, -1] - c) < rel * scale
    return out


def deviation(values, ref, targets, skip=None):
    """max over the real-valued targets of max |a - b| / max |b|; for ARGMAX / EXCEED the number of
    paths outside ``skip`` that differ (second result)."""
    worst, wrong = 0.0, 0
    for t, (kind, *_r) in enumerate(targets):
        if kind in REAL:
            worst = max(worst, float(np.max(np.abs(values[t] - ref[t])) / max(np.max(np.abs(ref[t])), 1e-300)))
        else:
            keep = ~skip[t] if skip is not None else slice(None)
            wrong += int(np.count_nonzero(values[t][keep] != ref[t][keep]))
    return worst, wrong


# ---- the shapes of the GPU tests ---------------------------------------------------------------
def _mixture(rng, P, S, m, indep, center, spread, zero_weight):
    w = rng.random((S, P)) + 0.2
    if zero_weight and P > 1:
        w[:, 1] = 0.0
    w /= w.sum(axis=1, keepdims=True)
    nmat = (S, P) if indep else (P,)
    a = rng.standard_normal(nmat + (m, m)) / math.sqrt(m)
    sigma = spread * spread * (a @ np.swapaxes(a, -1, -2) + 0.1 * np.eye(m))
    mu = center + spread * rng.standard_normal(((S, P, m) if indep else (P, S, m)))
    return w, mu, sigma


def all_kinds(m, T, thr):
    """T targets that cycle through the five kinds and the windows [0,0], [m-1,m-1], [0,m-1] and
    inner ones"""
    wins = [(0, 0), (m - 1, m - 1), (0, m - 1), (m // 3, (2 * m) // 3), (min(1, m - 1), m - 1)]
    return [(t % 5, *wins[(t // 5 + t) % len(wins)], thr * (1.0 + 0.01 * (t // 5))) for t in range(T)]


def levels(Q):
    base = [0.01, 0.025, 0.5, 0.5, 0.975, 0.99, 0.25, 0.5]      # repeated levels, not sorted
    if Q == 1:
        return [0.5]
    return (base + [(i + 0.5) / Q for i in range(Q)])[:Q]


def make_case(name):
    """-> dict(w, mu, sigma, draws, seed, inv, targets, probs); pathwise: compared path by path"""
    spec = CASES[name]
    rng = np.random.default_rng(spec["rng"])
    P, S, m, indep = spec["P"], spec["S"], spec["m"], spec.get("indep", False)
    w, mu, sigma = _mixture(rng, P, S, m, indep, spec["center"], spec["spread"], spec.get("zero_weight", False))
    seed = [int(v) for v in rng.integers(1, 2**62, S)] if indep else int(rng.integers(1, 2**62))
    return dict(w=w, mu=mu, sigma=sigma, draws=spec["draws"], seed=seed, inv=spec["inv"],
                targets=spec["targets"], probs=levels(spec["Q"]))


CASES = {
    # N = 1: every rank is 1
    "one_path": dict(rng=1, P=1, S=1, m=1, draws=1, center=1.0, spread=0.3, inv=(IDENTITY, 0.0, 0.0, 0.0),
                     targets=[(SUM, 0, 0, 0.0)], Q=1, pathwise=True),
    "n63_exp": dict(rng=2, P=3, S=1, m=2, draws=63, center=1.0, spread=0.3, inv=(EXP, 0.0, 0.0, 0.0),
                    targets=[(MAX, 0, 1, 3.0)], Q=64, pathwise=True),
    # all five kinds at T = 64, a component of weight zero, the Box-Cox pole side
    "n257_boxcox_neg": dict(rng=3, P=17, S=1, m=7, draws=257, center=1.0, spread=0.15, zero_weight=True,
                            inv=(BOXCOX, -0.3, 0.0, 5.0e4), targets=all_kinds(7, 64, 4.0), Q=64,
                            pathwise=True),
    "n4099_logistic": dict(rng=4, P=3, S=1, m=33, draws=4099, center=-1.0, spread=0.5,
                           inv=(LOGISTIC100, 0.0, 0.5, 0.0), targets=all_kinds(33, 10, 40.0), Q=23,
                           pathwise=True),
    # a clamp puts more than half of the values at exactly 0 (exactness only: ties everywhere)
    "n131073_clamped": dict(rng=5, P=3, S=1, m=7, draws=2**17 + 1, center=1.0, spread=0.3,
                            inv=(EXP, 0.0, 5.0, 0.0),
                            targets=[(SUM, 0, 6, 1.0), (MAX, 0, 6, 0.5), (DIFF, 0, 6, 0.0),
                                     (MAX, 3, 3, 0.0)], Q=23, pathwise=False),
    "n131073_exp": dict(rng=6, P=17, S=1, m=7, draws=2**17 + 1, center=1.0, spread=0.3, zero_weight=True,
                        inv=(EXP, 0.0, 0.0, 0.0), targets=all_kinds(7, 5, 4.0), Q=23, pathwise=True),
    # the LDS tiling limit, two scenarios over shared components
    "m192": dict(rng=7, P=17, S=2, m=192, draws=32, center=0.5, spread=0.3, zero_weight=True,
                 inv=(IDENTITY, 0.0, 0.0, 0.0), targets=all_kinds(192, 5, 1.2), Q=23, pathwise=True),
    "shared_s5": dict(rng=8, P=3, S=5, m=7, draws=13, center=1.0, spread=0.3,
                      inv=(BOXCOX, 0.4, 0.25, 1.0e4), targets=all_kinds(7, 5, 4.0), Q=1, pathwise=True),
    # independent mixtures
    "indep_s5": dict(rng=9, P=3, S=5, m=7, draws=13, indep=True, center=1.0, spread=0.3, zero_weight=True,
                     inv=(BOXCOX, 0.4, 0.25, 1.0e4), targets=all_kinds(7, 64, 4.0), Q=64, pathwise=True),
    "indep_s2_m33": dict(rng=10, P=1, S=2, m=33, draws=130, indep=True, center=1.0, spread=0.3,
                         inv=(EXP, 0.0, 0.0, 0.0), targets=all_kinds(33, 5, 5.0), Q=23, pathwise=True),
    # zero variance: every path of the single component is its mean, all values equal
    "constant": dict(rng=11, P=1, S=1, m=7, draws=257, center=1.0, spread=1e-150,
                     inv=(EXP, 0.0, 0.0, 0.0), targets=[(SUM, 0, 6, 1.0), (MAX, 0, 6, 0.5)], Q=23,
                     pathwise=False),
}
MAX_FRAGILE_SHARE = 1e-3

"""Long-double reference for the mixture summaries (tests/c/mixture_ref.c), the generators of the
test mixtures and the three acceptance checks, shared by the CPU and the GPU tests.

Every check prints the figure it judges before it asserts.  The tolerances are derived, not fitted:
fp64 erf / exp are good to a few ulp and the weights sum to 1, so

    CDF        |F - F_ld|              <= 1e-13 absolute
    quantile   |F_ld(q) - p|           <= 1e-13 + 4 f_ld(q) spacing(q)     (judged THROUGH the
               reference CDF — independent of how flat the distribution is; the second term is
               what one ulp of q is worth), q non-decreasing in p
    CRPS       |CRPS - CRPS_ld|        <= 1e-12 (T1 + T2 / 2), the size of the two sums the value
               is the difference of (not relative to CRPS itself: near the centre they cancel)
"""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "mixture_ref.c")

TOL_CDF = 1e-13
TOL_CRPS = 1e-12
HUB_LEVELS = np.concatenate([[0.01, 0.025], np.arange(1, 20) * 0.05, [0.975, 0.99]])   # 23
LEVELS = np.concatenate([[1e-6], HUB_LEVELS, [1 - 1e-6]])

_lib = None


def _load():
    global _lib
    if _lib is not None:
        return _lib
    tmp = tempfile.mkdtemp(prefix="mixture_ref_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    so = os.path.join(tmp, "libmixture_ref.so")
    base = ["gcc", "-std=c11", "-O2", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-o", so, SRC]
    try:        # dates in parallel where the compiler has OpenMP; serial otherwise
        subprocess.check_call(base + ["-fopenmp", "-lm"], stderr=subprocess.DEVNULL)
    except subprocess.CalledProcessError:
        subprocess.check_call(base + ["-Wno-unknown-pragmas", "-lm"])
    L = C.CDLL(so)
    dp, i32 = C.POINTER(C.c_double), C.c_int
    L.mixref_cdf.argtypes = [i32, i32, dp, dp, dp, i32, dp, dp, dp, dp]
    L.mixref_quantiles.argtypes = [i32, i32, dp, dp, dp, i32, dp, dp]
    L.mixref_crps.argtypes = [i32, i32, dp, dp, dp, i32, dp, i32, dp, dp, dp]
    for f in (L.mixref_cdf, L.mixref_quantiles, L.mixref_crps):
        f.restype = None
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


class Mixture:
    """w [C], mu [C, m], var [C, m] in the layout of the C-ABI"""

    def __init__(self, w, mu, var):
        self.w, self.mu, self.var = _f64(w), _f64(mu), _f64(var)
        self.C, self.m = self.mu.shape

    def centre_and_sd(self):
        """mean and standard deviation of the pool per date (fp64 is plenty for picking points)"""
        act = self.w > 0                      # (components of weight zero may hold anything)
        mean = self.w[act] @ self.mu[act]
        second = self.w[act] @ (self.var[act] + self.mu[act] ** 2)
        return mean, np.sqrt(second - mean ** 2)


def ref_cdf(mix: Mixture, x, minus_p=None):
    """x [m, K] -> (F [m, K], density [m, K]); with ``minus_p`` [K]: F - p taken in long double"""
    x = _f64(x)
    F, f = np.empty(x.shape), np.empty(x.shape)
    mp = _f64(minus_p) if minus_p is not None else None
    _load().mixref_cdf(mix.C, mix.m, _p(mix.w), _p(mix.mu), _p(mix.var), x.shape[1], _p(x),
                       _p(mp) if mp is not None else None, _p(F), _p(f))
    return F, f


def ref_quantiles(mix: Mixture, probs):
    probs = _f64(probs)
    q = np.empty((mix.m, probs.size))
    _load().mixref_quantiles(mix.C, mix.m, _p(mix.w), _p(mix.mu), _p(mix.var), probs.size, _p(probs),
                             _p(q))
    return q


def ref_crps(mix: Mixture, y, only_date=-1):
    """y [m] or [ny, m] -> (crps, scale = T1 + T2 / 2) of the same shape; ``only_date``: the other
    dates come back as NaN"""
    y = _f64(y)
    ys = y.reshape(-1, mix.m)
    crps, t1 = np.full(ys.shape, np.nan), np.full(ys.shape, np.nan)
    t2 = np.full(mix.m, np.nan)
    _load().mixref_crps(mix.C, mix.m, _p(mix.w), _p(mix.mu), _p(mix.var), ys.shape[0], _p(ys),
                        int(only_date), _p(crps), _p(t1), _p(t2))
    scale = t1 + 0.5 * t2[None, :]
    return crps.reshape(y.shape), scale.reshape(y.shape)


# ---- test mixtures ------------------------------------------------------------------------------
def make_mixture(C_, m, seed, kind="pool") -> Mixture:
    """``pool``: means N(0.3, 0.25^2), standard deviations 0.05 exp(0.7 z), weights ~ exp(3 z) (a few
    components carry most of the mass, as after a weight update); ``decades``: the same with
    variances spread over eight decades; ``sparse``: the same with 90 % of the weights zero (and
    garbage in the moments of those components: they are to be ignored)."""
    rng = np.random.default_rng([seed, C_, m])
    mu = 0.3 + 0.25 * rng.standard_normal((C_, m))
    sd = 0.05 * np.exp(0.7 * rng.standard_normal((C_, m)))
    w = np.exp(3.0 * rng.standard_normal(C_))
    if kind == "decades":
        sd = 10.0 ** rng.uniform(-5.0, -1.0, size=(C_, m))          # variances 1e-10 ... 1e-2
    elif kind == "sparse":
        zero = rng.random(C_) < 0.9
        zero[int(rng.integers(C_))] = False
        w[zero] = 0.0
        mu[zero] = np.nan
        sd[zero] = -1.0
    else:
        assert kind == "pool"
    w = w / w.sum()
    return Mixture(w, mu, np.where(sd > 0, sd * sd, sd))


def y_points(mix: Mixture):
    """[5, m]: the pool's centre, +-3 and +-8 pooled standard deviations"""
    c, s = mix.centre_and_sd()
    return np.stack([c, c - 3 * s, c + 3 * s, c - 8 * s, c + 8 * s])


# ---- the acceptance checks ------------------------------------------------------------------------
def check_cdf(label, mix, x, F_dev):
    F_ref, _ = ref_cdf(mix, x)
    err = float(np.max(np.abs(F_dev - F_ref)))
    print(f"{label}: CDF worst |F - F_ld| = {err:.3e} (bound {TOL_CDF:.0e})")
    assert err <= TOL_CDF, (label, err)


def check_quantiles(label, mix, probs, q_dev):
    probs = _f64(probs)
    assert q_dev.shape == (mix.m, probs.size) and np.all(np.isfinite(q_dev)), label
    miss, dens = ref_cdf(mix, q_dev, minus_p=probs)
    bound = 1e-13 + 4.0 * dens * np.spacing(np.abs(q_dev))
    ratio = float(np.max(np.abs(miss) / bound))
    print(f"{label}: quantiles worst |F_ld(q) - p| = {np.max(np.abs(miss)):.3e}, "
          f"worst share of its bound {ratio:.3f}")
    assert ratio <= 1.0, (label, ratio)
    order = np.argsort(probs, kind="stable")
    assert np.all(np.diff(q_dev[:, order], axis=1) >= 0), f"{label}: quantiles decrease in p"


def check_crps(label, mix, y, crps_dev, only_date=-1):
    ref, scale = ref_crps(mix, y, only_date)
    keep = np.isfinite(ref)
    assert keep.any() and np.all(np.isfinite(np.asarray(crps_dev)[keep])), label
    rel = float(np.max(np.abs(np.asarray(crps_dev)[keep] - ref[keep]) / scale[keep]))
    print(f"{label}: CRPS worst |CRPS - CRPS_ld| / (T1 + T2/2) = {rel:.3e} (bound {TOL_CRPS:.0e})")
    assert rel <= TOL_CRPS, (label, rel)

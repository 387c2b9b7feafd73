"""Host reference for ``ngp_mixture_crps_mapped``: CRPS and mean of psi(X), X a Gaussian mixture,
psi = s o g with g an inverse transformation of ``nowcast.get_transformations`` (edge rules
included) and s the identity or log(. + shift) — independent of the device's rule:

* Phi in long double from tests/mixture_reference.py (tests/c/mixture_ref.c); an upper tail
  1 - F(x) is the CDF of the reflected mixture at -x, so it keeps its relative accuracy;
* composite Gauss-Legendre 20 (not Gauss-Kronrod) on panels split at the MATHEMATICAL breakpoints:
  where g leaves its clamp / floor, the Box-Cox pole, and the point where psi crosses s(y);
* the range is mu -+ 14 sd, widened upwards by 2 sd^2 for the growth of exp — its own rule;
* the panel width is halved until two successive results differ by less than 1e-15 relative
  (the integrands and their sums are carried in long double); the mean is a by-product, its
  own last change is returned as ``mean_err``.

With x0 the crossing point clipped to where psi moves,

    CRPS = int_{x<x0} F^2 dpsi + int_{x>x0} (1-F)^2 dpsi + |s(y) - psi(x0)|
    E[Y] = psi(x0) + int_{x>x0} (1-F) dpsi - int_{x<x0} F dpsi
    S    = E|Y - s(y)| = int_{x<x0} F dpsi + int_{x>x0} (1-F) dpsi + |s(y) - psi(x0)|
"""
import math

import numpy as np

from tests import mixture_reference as R

IDENTITY, EXP, LOGISTIC100, BOXCOX = 0, 1, 2, 3
NATURAL, LOG = 0, 1
LD = np.longdouble
_GLX, _GLW = np.polynomial.legendre.leggauss(20)
_GLX, _GLW = _GLX.astype(LD), _GLW.astype(LD)
FLOOR = LD(1e-10)


def g_of(inv, x):
    """the inverse transformation in long double, edge rules of include/ngp.h"""
    kind, lam, offset, cap = inv
    x = np.asarray(x, dtype=LD)
    with np.errstate(all="ignore"):
        if kind == IDENTITY:
            return x
        if kind == EXP or (kind == BOXCOX and lam == 0):
            return np.maximum(np.exp(x) - LD(offset), 0)
        if kind == LOGISTIC100:
            return np.maximum(100 / (1 + np.exp(-x)) - LD(offset), 0)
        base = LD(lam) * x + 1
        if lam > 0:
            r = np.maximum(base, FLOOR) ** (1 / LD(lam)) - LD(offset)
        else:
            safe = np.where(base > 0, base, 1)
            p = safe ** (1 / LD(lam))
            r = np.where(base > FLOOR, p - LD(offset),
                         np.where(base <= 0, 0, np.minimum(p, LD(cap)) - LD(offset)))
        return np.maximum(r, 0)


def psi_of(inv, scale, shift, x):
    v = g_of(inv, x)
    with np.errstate(all="ignore"):
        return np.log(v + LD(shift)) if scale == LOG else v


def dpsi_of(inv, scale, shift, x):
    """psi'(x) where g is strictly increasing"""
    kind, lam, offset, cap = inv
    x = np.asarray(x, dtype=LD)
    with np.errstate(all="ignore"):
        if kind == IDENTITY:
            d = np.ones_like(x)
        elif kind == EXP or (kind == BOXCOX and lam == 0):
            d = np.exp(x)
        elif kind == LOGISTIC100:
            sg = 1 / (1 + np.exp(-x))
            d = 100 * sg * (1 - sg)
        else:
            d = (LD(lam) * x + 1) ** (1 / LD(lam) - 1)
        if scale == LOG:
            d = d / (g_of(inv, x) + LD(shift))
    return d


def moving_interval(inv, scale, shift):
    """(xL, xR): where psi is strictly increasing; gmin = g(-inf)"""
    kind, lam, offset, cap = inv
    xL, xR = -math.inf, math.inf
    if kind == IDENTITY:
        return (-shift if scale == LOG else -math.inf), math.inf, -math.inf
    gmin = float(g_of(inv, -math.inf))
    if kind == EXP or (kind == BOXCOX and lam == 0):
        if offset > 0:
            xL = math.log(offset)
    elif kind == LOGISTIC100:
        if offset >= 100:
            xL = math.inf
        elif offset > 0:
            xL = math.log(offset / (100 - offset))
    else:
        edge = float((FLOOR - 1) / LD(lam))
        if lam > 0:
            xL = edge
        else:
            xR = edge
        if offset > 0:
            xL = max(xL, float((LD(offset) ** LD(lam) - 1) / LD(lam)))
    return xL, xR, gmin


def crossing(inv, y, gmin):
    """inf {x : g(x) >= y} in long double"""
    kind, lam, offset, cap = inv
    if kind == IDENTITY:
        return LD(y)
    v = LD(y) + LD(offset)
    if y <= gmin or not v > 0:
        return LD(-math.inf)
    if kind == EXP or (kind == BOXCOX and lam == 0):
        return np.log(v)
    if kind == LOGISTIC100:
        u = v / 100
        return LD(math.inf) if u >= 1 else np.log(u / (1 - u))
    return (v ** LD(lam) - 1) / LD(lam)


def _tail_sums(mix1, mirror1, x, upper):
    """F (lower) or 1 - F (upper) of ONE date at x [K], as long double"""
    if upper:
        F, _ = R.ref_cdf(mirror1, -x[None, :])
    else:
        F, _ = R.ref_cdf(mix1, x[None, :])
    return F[0].astype(LD)


def _integrate(mix1, mirror1, inv, scale, shift, a, b, upper, width):
    """(int T^2 dpsi, int T dpsi) over [a, b] in panels no wider than ``width``"""
    if not b > a:
        return LD(0), LD(0)
    n = max(1, int(math.ceil(float(b - a) / width)))
    edges = LD(a) + (LD(b) - LD(a)) * np.arange(n + 1, dtype=LD) / n
    half = 0.5 * (edges[1:] - edges[:-1])
    x = ((edges[:-1] + half)[:, None] + half[:, None] * _GLX[None, :]).reshape(-1)
    wts = (half[:, None] * _GLW[None, :]).reshape(-1)
    T = _tail_sums(mix1, mirror1, np.ascontiguousarray(x.astype(np.float64)), upper)
    d = dpsi_of(inv, scale, shift, x.astype(np.float64).astype(LD)) * wts
    return np.sum(T * T * d), np.sum(T * d)


def reference(mix: R.Mixture, inv, scale, shift, y, max_levels=12):
    """per date: dict(crps, mean, S, status) with status 0, or -3 where the score is infinite /
    psi is not monotone where the mass is (the contract of include/ngp.h)"""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    m = mix.m
    out = dict(crps=np.full(m, np.nan), mean=np.full(m, np.nan), S=np.full(m, np.nan),
               status=np.zeros(m, dtype=int), levels=np.zeros(m, dtype=int), mean_err=np.zeros(m))
    act = mix.w > 0
    xL, xR, gmin = moving_interval(inv, scale, shift)
    for j in range(m):
        mu, var = mix.mu[act, j], mix.var[act, j]
        sd = np.sqrt(var)
        mix1 = R.Mixture(mix.w[act], mu[:, None], var[:, None])
        mirror1 = R.Mixture(mix.w[act], -mu[:, None], var[:, None])
        lo = float(np.min(mu - 14 * sd))
        hi = float(np.max(mu + (14 + 2 * sd) * sd))
        if xR < hi:
            beyond = float(R.ref_cdf(mirror1, np.array([[-xR]]))[0][0, 0])
            if beyond > 1e-12:
                out["status"][j] = -3
                continue
        if scale == LOG and not gmin + shift > 0 and xL > lo:
            # the log of 0 with mass on it: "mass" is what exceeds the 1e-18 tail budget
            if float(R.ref_cdf(mix1, np.array([[min(xL, hi)]]))[0][0, 0]) > 1e-18:
                out["status"][j] = -3
                continue
        alo = min(max(lo, xL), hi)
        ahi = max(min(hi, xR), alo)
        xy = crossing(inv, y[j], gmin)
        x0 = min(max(xy, LD(alo)), LD(ahi))
        psi0 = psi_of(inv, scale, shift, x0)
        yt = np.log(LD(y[j]) + LD(shift)) if scale == LOG else LD(y[j])
        clip = LD(0) if alo < xy < ahi else abs(yt - psi0)
        width = 6.0 * float(sd.min())
        prev = None
        for level in range(max_levels):
            lo2, lo1 = _integrate(mix1, mirror1, inv, scale, shift, alo, x0, False, width)
            up2, up1 = _integrate(mix1, mirror1, inv, scale, shift, x0, ahi, True, width)
            cur = (lo2 + up2 + clip, psi0 + up1 - lo1, lo1 + up1 + clip)
            # the rule is on the CRPS; the mean is a by-product whose own last change is reported
            # as mean_err (where mass sits on a Box-Cox floor with lam > 1, psi' has an integrable
            # singularity that F, unlike F^2, does not flatten: the mean converges algebraically)
            if prev is not None and abs(cur[0] - prev[0]) <= LD(1e-15) * abs(cur[0]):
                break
            before, prev = prev, cur
            width *= 0.5
        else:
            raise AssertionError(f"the reference did not converge at date {j}: {before} -> {cur}")
        out["crps"][j], out["mean"][j], out["S"][j] = (float(v) for v in cur)
        out["levels"][j] = level
        out["mean_err"][j] = float(abs(cur[1] - prev[1]))
    return out


def lognormal_crps(mu, sd, y):
    """Baran & Lerch (2015), one lognormal component; Phi from the long double reference"""
    one = R.Mixture([1.0], [[0.0]], [[1.0]])

    def Phi(z):
        return LD(R.ref_cdf(one, np.array([[float(z)]]))[0][0, 0])
    mu, sd, y = LD(mu), LD(sd), LD(y)
    z = (np.log(y) - mu) / sd
    return float(y * (2 * Phi(z) - 1)
                 - 2 * np.exp(mu + sd * sd / 2) * (Phi(z - sd) + Phi(sd / np.sqrt(LD(2))) - 1))

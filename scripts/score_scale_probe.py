"""Times ngp_mixture_crps_mapped at the size of a pooled nowcast forecast (C = 12,800 components,
m = 32 dates, Box-Cox lambda = 0.3, natural and log(. + 1) scale) against the two routes there were
before it for the same number:

  cdf route     nodes built on the host (Gauss-Legendre 20 on panels of one sd_min between the same
                breakpoints), F at the nodes from ngp_mixture_cdf in slices of K <= 4096 points per
                date, the weighted sum on the host (the panels are not split at the crossing
                point, so this route is good to about 1e-3 here: it is the time that is compared)
  sample route  the O(N log N) sample estimator on N = 2,000 draws per date of the same marginals
                (what a user gets from forecast_targets values), drawn on the host

Prints one JSON line.  Usage: python scripts/score_scale_probe.py [--C 12800] [--m 32]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--C", type=int, default=12800)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ge.build()
    from nowcastautogp_amd import _lib
    ctx = _lib.Context(0)
    rng = np.random.default_rng(7)
    C, m, lam = a.C, a.m, 0.3
    mu = 5.0 + 0.4 * rng.standard_normal((C, m))
    sd = 0.15 * np.exp(0.4 * rng.standard_normal((C, m)))
    w = np.exp(rng.standard_normal(C))
    w /= w.sum()
    var = sd * sd
    inv = (3, lam, 0.0, 1e6)
    centre = w @ mu
    y = (lam * (centre + 0.1) + 1.0) ** (1.0 / lam)
    out = {"C": C, "m": m, "lam": lam}

    def best(fn):
        fn()
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter()
            r = fn()
            ts.append(time.perf_counter() - t)
        return min(ts), r

    for name, scale, shift in (("natural", 0, 0.0), ("log", 1, 1.0)):
        t, (crps, mean, err, info) = best(lambda: ctx.mixture_crps_mapped(w, mu, var, inv, scale, shift, y))
        out[f"device_{name}_ms"] = 1e3 * t
        out[f"device_{name}_rel_err"] = float(np.max(err / np.abs(crps)))
        out[f"device_{name}_info"] = int(np.max(np.abs(info)))
        dev = crps

        def psi(x):
            v = (lam * x + 1.0) ** (1.0 / lam)
            return np.log(v + shift) if scale else v

        def dpsi(x):
            d = (lam * x + 1.0) ** (1.0 / lam - 1.0)
            return d / ((lam * x + 1.0) ** (1.0 / lam) + shift) if scale else d

        def cdf_route():
            gx, gw = np.polynomial.legendre.leggauss(20)
            lo, hi, h = (mu - 10 * sd).min(axis=0), (mu + 11 * sd).max(axis=0), sd.min(axis=0)
            lo = np.maximum(lo, (1e-10 - 1.0) / lam)                  # the Box-Cox floor: flat below
            x0 = ((y ** lam) - 1.0) / lam
            n = int(np.ceil(np.max((hi - lo) / h)))
            e = lo[:, None] + (hi - lo)[:, None] * np.arange(n + 1)[None, :] / n       # [m, n + 1]
            half = 0.5 * np.diff(e, axis=1)
            x = ((e[:, :-1] + half)[:, :, None] + half[:, :, None] * gx[None, None, :]).reshape(m, -1)
            wt = (half[:, :, None] * gw[None, None, :]).reshape(m, -1)
            F = np.concatenate([ctx.mixture_cdf(w, mu, var, np.ascontiguousarray(x[:, k:k + 4096]))[0]
                                for k in range(0, x.shape[1], 4096)], axis=1)
            T = np.where(x >= x0[:, None], 1.0 - F, F)
            return np.sum(T * T * dpsi(x) * wt, axis=1)

        t, via_cdf = best(cdf_route)
        out[f"cdf_route_{name}_ms"] = 1e3 * t
        out[f"cdf_route_{name}_rel_diff"] = float(np.max(np.abs(via_cdf - dev) / dev))

        def sample_route():
            N = 2000
            r = np.random.default_rng(11)
            res = np.empty(m)
            for j in range(m):
                comp = r.choice(C, size=N, p=w)
                Y = np.sort(psi(mu[comp, j] + sd[comp, j] * r.standard_normal(N)))
                i = np.arange(N)
                res[j] = np.mean(np.abs(Y - psi(x0_[j]))) - np.sum((2 * i - N + 1) * Y) / (N * N)
            return res

        x0_ = ((y ** lam) - 1.0) / lam
        t, via_draws = best(sample_route)
        out[f"sample_route_{name}_ms"] = 1e3 * t
        out[f"sample_route_{name}_rel_diff"] = float(np.max(np.abs(via_draws - dev) / dev))
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

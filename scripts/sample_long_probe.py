"""Paths of a long horizon: ngp_factor_sample_long against the path it replaces.

At P = 64 particles, D = 200 scenarios of 3 appended points, 100 draws per scenario and n = 2049
observations, for every horizon m asked for (default 365, 1024 and 4096), two wall times:

  device   one ``Factor.sample_long`` call (sigma formed, factorised and used on the device)
  host     what the mirror does without ``device_paths``: ``predict_long(want_sigma=True)``,
           ``np.linalg.cholesky`` per particle, then the draws on the host (one matrix-vector
           product per path, as ``MixtureMVN.rand`` makes them)

Runs on a machine with the device; writes profiles/sample_long_probe.json (``--out``).
    python scripts/sample_long_probe.py [--m 365 1024 4096] [--out profiles/sample_long_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402
from nowcastautogp_amd import _lib  # noqa: E402

P, D, DRAWS, N, d = 64, 200, 100, 2049, 3
H = 1.0 / 365


def ensemble(rng):
    """Plus(Plus(Linear, Periodic), SqExp) with jittered parameters, P times"""
    progs = []
    for _ in range(P):
        par = np.array([0.2, 0.1, 0.5, 0.9, 0.3, 0.7, 0.21, 0.4]) * (1.0 + 0.2 * rng.random(8))
        progs.append((np.array([2, 5, 6, 3, 6], np.int32), par, 0.05))
    return progs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, nargs="+", default=[365, 1024, 4096])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_long_probe.json"))
    args = ap.parse_args()
    ge.build()
    rng = np.random.default_rng(1)
    t = np.arange(N) * H
    y = np.sin(2 * np.pi * t) + 0.2 * t + 0.1 * rng.standard_normal(N)
    t_add = t[-1] + H * np.arange(1, d + 1)
    y_add = y[-1] + 0.2 * rng.standard_normal((D, d))
    w = rng.random((D, P))
    w /= w.sum(axis=1, keepdims=True)
    ctx = _lib.Context(0)
    fac = ctx.factor(ensemble(rng), t, y)
    rows = []
    for m in args.m:
        t_new = t[-1] + H * (d + np.arange(1, m + 1))
        fac.sample_long(t_new, w[:, :], 1, 1, t_add, y_add)              # warm the allocator
        t0 = time.perf_counter()
        out, comp, info, cinfo = fac.sample_long(t_new, w, DRAWS, 7, t_add, y_add)
        dev = time.perf_counter() - t0
        assert not info.any() and not cinfo.any() and np.isfinite(out).all()
        t0 = time.perf_counter()
        mu, _, sg, info = fac.predict_long(t_new, t_add, y_add)
        t_query = time.perf_counter() - t0
        L = np.stack([np.linalg.cholesky(sg[k]) for k in range(P)])
        t_chol = time.perf_counter() - t0 - t_query
        host_rng = np.random.default_rng(7)
        x = np.empty((D, DRAWS, m))
        for s in range(D):
            for k, c in enumerate(host_rng.choice(P, size=DRAWS, p=w[s])):
                x[s, k] = mu[c, s] + L[c] @ host_rng.standard_normal(m)
        host = time.perf_counter() - t0
        rows.append(dict(m=m, P=P, D=D, draws=DRAWS, n=N, device_s=dev, host_s=host, host_query_s=t_query,
                         host_cholesky_s=t_chol, host_draws_s=host - t_query - t_chol))
        print(json.dumps(rows[-1]), flush=True)
        del sg, L, x, out
    fac.close()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(dict(what="ngp_factor_sample_long against predict_long + host Cholesky + host draws, wall seconds",
                       rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()

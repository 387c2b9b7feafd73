"""Paths of a long horizon for a refined scenario ensemble: ngp_factor_sample_long_indep against the
route it replaces.

P = 64 particles per scenario, D scenarios whose clones have parameters and data of their own,
n = 2049 observations, 100 draws per scenario; for every (D, m) asked for (default D = 8 and 50,
m = 365 and 1024), two wall times on the same build and box:

  device   the route of ``refined_device_paths=True``: factors over whole scenarios (items
           mixture-major, per-item y rows; halved where the device refuses) and one
           ``Factor.sample_long_indep`` call per factor
  host     today's route: the P D items predicted in pairwise blocks of dates
           (``autogp.predict_in_blocks`` over the one-shot predict, every call a factorisation of all
           items), every covariance brought to the host, ``np.linalg.cholesky`` per item, then the
           draws on the host (one matrix-vector product per path, as ``MixtureMVN.rand`` makes them)

Runs on a machine with the device; writes profiles/sample_long_indep_probe.json (``--out``).
    python scripts/sample_long_indep_probe.py [--D 8 50] [--m 365 1024] [--skip-host]
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
from nowcastautogp_amd import _lib, autogp  # noqa: E402

P, DRAWS, N = 64, 100, 2049
H = 1.0 / 365
TOO_LARGE = -3


def ensemble(rng, count):
    """Plus(Plus(Linear, Periodic), SqExp) with jittered parameters, one per item"""
    progs = []
    for _ in range(count):
        par = np.array([0.2, 0.1, 0.5, 0.9, 0.3, 0.7, 0.21, 0.4]) * (1.0 + 0.2 * rng.random(8))
        progs.append((np.array([2, 5, 6, 3, 6], np.int32), par, 0.05))
    return progs


def device_route(ctx, progs, t, Y, t_new, w, seeds, draws):
    """as autogp.sample_long_lockstep chunks: all scenarios first, halved on NGP_ERR_TOO_LARGE"""
    D = w.shape[0]
    out, j0, per, factors = [], 0, D, 0
    while j0 < D:
        k = min(per, D - j0)
        rows = slice(j0 * P, (j0 + k) * P)
        fac = None
        try:
            fac = ctx.factor(progs[rows], t, Y[rows])
            o, _, info, cinfo = fac.sample_long_indep(t_new, w[j0:j0 + k], draws, seeds[j0:j0 + k])
            assert not info.any() and not cinfo.any()
            out.append(o)
            factors += 1
        except _lib.NgpError as e:
            if e.status != TOO_LARGE or k == 1:
                raise
            per = max(1, k // 2)
            continue
        finally:
            if fac is not None:
                fac.close()
        j0 += k
    return np.concatenate(out), factors


def host_route(ctx, progs, t, Y, t_new, w, draws):
    def call(ts):
        o = ctx.predict_batch(progs, t, Y, ts)
        return o["mu"], o["sigma"], o["info"], None

    t0 = time.perf_counter()
    blocks = autogp.horizon_blocks(t.size, 0, t_new.size)
    mu, sg, info, _ = autogp.predict_in_blocks(call, t_new, blocks)
    assert not np.any(info)
    t_query = time.perf_counter() - t0
    L = np.stack([np.linalg.cholesky(sg[k]) for k in range(sg.shape[0])])
    t_chol = time.perf_counter() - t0 - t_query
    rng = np.random.default_rng(7)
    D, m = w.shape[0], t_new.size
    x = np.empty((D, draws, m))
    for s in range(D):
        for k, c in enumerate(rng.choice(P, size=draws, p=w[s])):
            x[s, k] = mu[s * P + c] + L[s * P + c] @ rng.standard_normal(m)
    total = time.perf_counter() - t0
    return dict(host_s=total, host_query_s=t_query, host_cholesky_s=t_chol, host_draws_s=total - t_query - t_chol,
                host_calls=len(blocks) * (len(blocks) - 1) // 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, nargs="+", default=[8, 50])
    ap.add_argument("--m", type=int, nargs="+", default=[365, 1024])
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_long_indep_probe.json"))
    args = ap.parse_args()
    ge.build()
    ctx = _lib.Context(0)
    rows = []
    for D in args.D:
        rng = np.random.default_rng(1)
        t = np.arange(N) * H
        base = np.sin(2 * np.pi * t) + 0.2 * t
        Y = np.repeat(np.stack([base + 0.1 * rng.standard_normal(N) for _ in range(D)]), P, axis=0)
        progs = ensemble(rng, P * D)
        w = rng.random((D, P))
        w /= w.sum(axis=1, keepdims=True)
        seeds = [int(s) for s in rng.integers(0, 2**63 - 1, size=D)]
        for m in args.m:
            t_new = t[-1] + H * np.arange(1, m + 1)
            device_route(ctx, progs[:P], t, Y[:P], t_new, w[:1], seeds[:1], 1)     # warm the allocator
            t0 = time.perf_counter()
            out, factors = device_route(ctx, progs, t, Y, t_new, w, seeds, DRAWS)
            dev = time.perf_counter() - t0
            assert np.isfinite(out).all()
            row = dict(m=m, P=P, D=D, draws=DRAWS, n=N, device_s=dev, device_factors=factors)
            if not args.skip_host:
                row.update(host_route(ctx, progs, t, Y, t_new, w, DRAWS))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del out
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(dict(what="ngp_factor_sample_long_indep on factors over whole scenarios against pairwise predict "
                            "blocks + host Cholesky + host draws, wall seconds", rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()

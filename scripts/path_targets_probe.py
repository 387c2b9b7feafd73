"""Times the trajectory targets (ngp_mixture_path_targets) at the headline pool — 64 particles x 200
scenarios, m = 28 dates, T = 6 targets, Q = 23 hub levels — with N = 10^6 and N = 2 x 10^4 pooled
paths, against the route a caller had before it in the same session on the same device:
ngp_mixture_sample, the copy of [S x draws x m] doubles to the host, then numpy for the inverse
transformation, the functionals and the quantiles.

Every figure: median of `--reps` timed calls after `--warmup` untimed ones, with the min-max
spread; wall times include validation and every copy.  The per-kernel split (pick, paths, select)
comes from a kernel trace of this script in a run of its own (`--device-only` leaves the host
route out of it).

    python scripts/path_targets_probe.py [--out path_targets.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

HUB = np.concatenate([[0.01, 0.025], np.arange(1, 20) * 0.05, [0.975, 0.99]])


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def pool(P, S, m, seed=5):
    rng = np.random.default_rng([seed, P, S, m])
    w = np.exp(1.5 * rng.standard_normal((S, P)))
    w /= w.sum(axis=1, keepdims=True)
    a = rng.standard_normal((P, m, m)) / np.sqrt(m)
    sigma = 0.09 * (a @ a.transpose(0, 2, 1) + 0.1 * np.eye(m))
    mu = 1.0 + 0.3 * rng.standard_normal((P, S, m))
    return w, mu, sigma


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    ge.build()
    from nowcastautogp_amd import _lib, autogp
    ctx = _lib.Context(0)
    P, S, m = 64, 200, 28
    w, mu, sigma = pool(P, S, m)
    inv = (1, 0.0, 0.5, 0.0)                                  # max(exp(x) - 0.5, 0)
    targets = [(0, 0, 3, 10.0), (0, 0, m - 1, 80.0), (1, 0, m - 1, 5.0), (2, 0, 3, 0.0),
               (3, 0, m - 1, 0.0), (4, 0, m - 1, 6.0)]
    lines = []
    for draws in (5000, 100):
        N = S * draws

        def device():
            return ctx.mixture_path_targets(w, mu, sigma, draws, 7, inv, targets, HUB)

        def host():
            x = ctx.mixture_sample(w, mu, sigma, draws, 7)[0].reshape(N, m)
            v = np.maximum(np.exp(x) - 0.5, 0.0)
            vals = autogp.path_functionals(v, targets)
            return autogp.summarize_path_values(vals, targets, HUB, m)

        td = timed(device, a.warmup, a.reps)
        lines.append(f"N = {N:>8d}  ngp_mixture_path_targets          {td[0]:9.2f} ms  [{td[1]:.2f}, {td[2]:.2f}]")
        if not a.device_only:
            th = timed(host, a.warmup, max(2, a.reps // 2))
            lines.append(f"N = {N:>8d}  ngp_mixture_sample + copy + numpy  {th[0]:9.2f} ms  [{th[1]:.2f}, {th[2]:.2f}]"
                         f"   ratio {th[0] / td[0]:.1f}")
            q_dev, q_host = device()["q"], host()[0]
            lines.append(f"              largest |q_device - q_host| / |q_host| over the real-valued targets: "
                         f"{np.nanmax(np.abs(q_dev - q_host) / np.abs(q_host)):.2e}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

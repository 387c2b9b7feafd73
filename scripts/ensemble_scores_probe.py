"""Times the path scores (ngp_ensemble_scores) at N = 20,000 paths x m = 32 dates with the default
windows (every single date plus the whole horizon, log scale) against the chunked numpy fallback
(autogp.host_ensemble_scores) in the same session, and prints both with the largest relative
difference of a term.

Device figure: median of `--reps` timed calls after `--warmup` untimed ones, with the min-max
spread; wall time including validation and every copy.  The numpy fallback takes minutes at this
size: it is timed once (`--host-n` scores fewer paths on the host and scales by (N / host_n)^2,
said so in the output; 0 leaves the host out).

    python scripts/ensemble_scores_probe.py [--n 20000] [--m 32] [--host-n 20000]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--host-n", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    ge.build()
    from nowcastautogp_amd import _lib, autogp
    rng = np.random.default_rng(1)
    x = np.exp(5.0 + 0.3 * rng.standard_normal((a.n, a.m)) + 0.05 * np.arange(a.m))
    y = np.exp(5.0 + 0.05 * np.arange(a.m))
    win = [(j, j) for j in range(a.m)] + [(0, a.m - 1)]
    ctx = _lib.Context(0)
    for _ in range(a.warmup):
        ctx.ensemble_scores(x, y, win, 1, 0.0, True)
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        dev = ctx.ensemble_scores(x, y, win, 1, 0.0, True)
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    print(f"ngp_ensemble_scores N={a.n} m={a.m} W={len(win)}: median {np.median(ts):.2f} ms "
          f"(min {ts.min():.2f}, max {ts.max():.2f}, {a.reps} calls)")
    if a.host_n > 0:
        hn = min(a.host_n, a.n)
        t0 = time.perf_counter()
        host = autogp.host_ensemble_scores(x[:hn], y, win, 1, 0.0, True)
        th = time.perf_counter() - t0
        if hn == a.n:
            diff = max(float(np.max(np.abs(dev[k] - host[k]) / np.abs(host[k]))) for k in ("term_obs", "term_pair"))
            print(f"numpy fallback N={hn}: {th:.1f} s (one call); largest relative difference of a term {diff:.2e}")
        else:
            print(f"numpy fallback N={hn}: {th:.1f} s (one call), scaled by (N / host_n)^2 to N={a.n}: "
                  f"{th * (a.n / hn) ** 2:.1f} s")


if __name__ == "__main__":
    main()

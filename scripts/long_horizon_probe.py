"""Times ONE ngp_factor_predict_long query against the pairwise path (autogp.predict_in_blocks over
ngp_factor_nowcast) on a daily grid over a year, with and without sigma:

    python scripts/long_horizon_probe.py [--reps 5] [--out FILE.json]

Shapes: (P = 64, n = 2,047, m = 365) and (P = 24, n = 208, m = 365).  Per shape it prints the wall
time of both paths (median of --reps after one warm-up call), the number of pairwise queries and the
columns they sweep through L, and from the library's profile (class chol_col_thin = 6, the solve)
the solve's device time, its rate against the measured fp64 matrix peak and the HBM bytes the
launch accounts for.  A tool, not a test."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from nowcastautogp_amd import _lib, autogp
    from nowcastautogp_amd.synthetic import make_workload
    ctx = _lib.Context(0)
    ctx.set_combining(False)
    peak = ctx.microbench_mfma_f64()
    res = dict(mfma_f64_peak_tflops=peak, shapes=[])
    for P, n, m in ((64, 2047, 365), (24, 208, 365)):
        w = make_workload("C1", n=n, P=P, D=1, d=1, m=4)
        t_new = w.t[-1] + (w.t[1] - w.t[0]) * np.arange(1, m + 1)
        f = ctx.factor(w.programs, w.t, w.y)
        blocks = autogp.horizon_blocks(n, 0, m)
        nq = len(blocks) * (len(blocks) - 1) // 2
        cols = sum((blocks[i][1] - blocks[i][0]) + (blocks[j][1] - blocks[j][0]) + n % 64 + 1
                   for i in range(len(blocks)) for j in range(i + 1, len(blocks)))

        def pairwise():
            def call(ts):
                mu, sg, _, info = f.predict(ts)
                return mu, sg, info, None
            return autogp.predict_in_blocks(call, t_new, blocks)

        row = dict(P=P, n=n, m=m, pairwise_queries=nq, pairwise_columns=cols,
                   long_columns=1 + n % 64 + m,
                   pairwise_ms=median_ms(pairwise, a.reps),
                   long_sigma_ms=median_ms(lambda: f.predict_long(t_new), a.reps),
                   long_var_ms=median_ms(lambda: f.predict_long(t_new, want_sigma=False), a.reps))
        mu_p, sg_p = pairwise()[:2]
        mu_l, _, sg_l, _ = f.predict_long(t_new)
        row["max_rel_diff_mu"] = float(np.max(np.abs(mu_l[:, 0] - mu_p)) / np.max(np.abs(mu_p)))
        row["max_rel_diff_sigma"] = float(np.max(np.abs(sg_l - sg_p)) / np.max(np.abs(sg_p)))
        ctx.profile_enable(True)
        ctx.profile_reset()
        f.predict_long(t_new, want_sigma=False)
        prof = ctx.profile_get()
        ctx.profile_enable(False)
        row["profile_var_only"] = prof
        s = prof.get("chol_col_thin")
        if s and s["ms"] > 0:
            row["solve_ms"] = s["ms"]
            row["solve_tflops"] = s["flops"] / s["ms"] * 1e-9
            row["solve_fraction_of_mfma_peak"] = row["solve_tflops"] / peak
            row["solve_algorithmic_gbytes"] = s["bytes"] * 1e-9
            row["solve_algorithmic_gbs"] = s["bytes"] / s["ms"] * 1e-6
        f.close()
        res["shapes"].append(row)
        print(json.dumps(row))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

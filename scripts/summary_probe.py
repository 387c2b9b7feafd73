"""Times the exact forecast summaries (ngp_mixture_cdf / _quantiles / _crps) at the headline pool —
64 particles x 200 scenarios = 12,800 components — with m = 9 and m = 52 dates and Q = 23 levels,
and at the everyday pool 24 x 40 = 960 components, m = 9.  For the CRPS it reports pair terms per
second next to what the same expression gives on registers only (ngp_microbench_mixture_pairs: no
loads, no LDS) — how far the tile kernel is from its own ceiling.  Next to them the yardstick: the
device work of the first default-mode forecast_with_nowcasts at 64 x 200, n = 2048, m = 9, 20 draws
per scenario (factorisation included — what a user who forecasts once pays for the draws) and of
the repeated call on the resident factor.

Every figure: median of `--reps` timed calls after `--warmup` untimed ones, with the min-max spread.
Wall times include the host pass (validation, date-major restaging) and both copies.

    python scripts/summary_probe.py [--out profiles/r05/forecast_summaries.txt]
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


def pool(C, m, seed):
    rng = np.random.default_rng([seed, C, m])
    mu = 0.3 + 0.25 * rng.standard_normal((C, m))
    var = (0.05 * np.exp(0.7 * rng.standard_normal((C, m)))) ** 2
    w = np.exp(3.0 * rng.standard_normal(C))
    return w / w.sum(), mu, var


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-yardstick", action="store_true")
    a = ap.parse_args()
    ge.build()
    from nowcastautogp_amd import autogp
    from nowcastautogp_amd import nowcast as nc
    eng = autogp.HipEngine(0)
    ctx = eng.ctx
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# summary_probe: warm-up {a.warmup}, {a.reps} timed calls, median [min, max] ms wall")
    ceil = [ctx.microbench_mixture_pairs(4096) for _ in range(5)]
    say(f"pair expression on registers only: {np.median(ceil) / 1e9:.2f} G pairs/s "
        f"[{min(ceil) / 1e9:.2f}, {max(ceil) / 1e9:.2f}] (5 runs)")
    total = {}
    for C, m in ((12800, 9), (12800, 52), (960, 9)):
        w, mu, var = pool(C, m, 1)
        y = w @ mu
        q = timed(lambda: ctx.mixture_quantiles(w, mu, var, HUB), a.warmup, a.reps)
        c = timed(lambda: ctx.mixture_crps(w, mu, var, y), a.warmup, a.reps)
        p = timed(lambda: ctx.mixture_cdf(w, mu, var, y[:, None]), a.warmup, a.reps)
        pairs = m * C * (C - 1) / 2
        say(f"C = {C:6d} m = {m:3d}: quantiles (Q = 23) {q[0]:8.3f} [{q[1]:.3f}, {q[2]:.3f}]   "
            f"CRPS {c[0]:8.3f} [{c[1]:.3f}, {c[2]:.3f}]   PIT {p[0]:7.3f} [{p[1]:.3f}, {p[2]:.3f}]   "
            f"sum {q[0] + c[0] + p[0]:8.3f} ms")
        say(f"    CRPS: {pairs / 1e6:.1f} M pair terms, {pairs / (c[0] * 1e-3) / 1e9:.2f} G pairs/s of wall "
            f"= {100 * pairs / (c[0] * 1e-3) / np.median(ceil):.0f} % of the register-only rate")
        total[(C, m)] = q[0] + c[0] + p[0]
    if not a.skip_yardstick:
        # the device work of the first default-mode forecast_with_nowcasts at the headline size, call
        # by call as the mirror makes them (nowcast._Scenarios, mode "shared"): factorise the 64
        # particles, one nowcast query for the 200 scenarios, normalise the weights, 20 draws per
        # scenario from the device sampler — then the same forecast as exact summaries instead
        from nowcastautogp_amd import _lib
        from nowcastautogp_amd.synthetic import make_workload
        wl = make_workload("C3", n=2048, P=64, D=200, d=2, m=9)
        P, D, m = 64, 200, 9

        def query(fac):
            o = fac.nowcast(wl.t_add, wl.y_add, wl.t_new, True)
            assert not o["info"].any()
            w, _, _ = _lib.weights_normalize_cols(o["logml_full"] - o["logml_base"][:, None])
            return np.ascontiguousarray(w.T), o["mu"], o["sigma"]                # [D, P], [P, D, m], [P, m, m]

        def draws(fac):
            w, mu, sg = query(fac)
            out, _, info = ctx.mixture_sample(w, mu, sg, 20, 12345)
            assert not info.any()
            return out

        def summaries(fac):
            w, mu, sg = query(fac)
            means = np.ascontiguousarray(mu.transpose(1, 0, 2)).reshape(D * P, m)
            var = np.broadcast_to(np.einsum("pjj->pj", sg)[None], (D, P, m)).reshape(D * P, m)
            wp = (w / D).reshape(D * P)
            y = wp @ means
            q, i1 = ctx.mixture_quantiles(wp, means, var, HUB)
            c, i2 = ctx.mixture_crps(wp, means, var, y)
            f, i3 = ctx.mixture_cdf(wp, means, var, y[:, None])
            assert not (i1.any() or i2.any() or i3.any()) and np.isfinite(q).all()
            return q, c, f

        t0 = time.perf_counter()
        fac = ctx.factor(wl.programs, wl.t, wl.y)
        draws(fac)
        first = (time.perf_counter() - t0) * 1e3
        rep = timed(lambda: draws(fac), 1, 7)
        say(f"yardstick, default-mode forecast_with_nowcasts at 64 x 200, n = 2048, m = 9, 20 draws per "
            f"scenario: first call, factorisation included {first:.1f} ms (one run); repeated on the "
            f"resident factor {rep[0]:.2f} [{rep[1]:.2f}, {rep[2]:.2f}] ms")
        sm = timed(lambda: summaries(fac), 1, 7)
        qy = timed(lambda: query(fac), 1, 7)
        say(f"the same forecast as exact summaries (query of the resident factor + quantiles at 23 levels "
            f"+ CRPS + PIT of the 12,800-component pool): {sm[0]:.2f} [{sm[1]:.2f}, {sm[2]:.2f}] ms, of "
            f"which the query {qy[0]:.2f} ms")
        say(f"goal (summaries no dearer than the first call's draws): {sm[0]:.1f} ms against {first:.1f} ms "
            f"-> {'met' if sm[0] <= first else 'MISSED'} ({sm[0] / first:.2f} x); against the repeated "
            f"call {sm[0] / rep[0]:.1f} x")
        fac.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()

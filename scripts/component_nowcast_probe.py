"""Times the decomposition conditioned on nowcasts (ngp_factor_components_nowcast) next to the
nowcast query that sweeps the same number of rows: 64 particles, n = 2049 (32 block columns and a
tail of one), three components per particle and m = 28 dates — 84 component rows — with d = 2
appended points and D = 200 scenarios, against ngp_factor_nowcast with the same d and D and m = 84
on the same factor, and the plain decomposition (ngp_factor_components, d = 0) beside them.  The
sweep through the resident L is common to all; what the decomposition adds is the component fill
and its epilogue, which here also eliminates the appended points and solves every scenario.  The
per-class device times (ngp_profile) say which.

Every figure: median of `--reps` timed calls after `--warmup` untimed ones, with the min-max spread;
wall times include staging and both copies.  `--skip-components` times the two older queries alone:
for a commit that has no ngp_factor_components_nowcast, copy this script into a checkout of it and
run it there with that flag.

    python scripts/component_nowcast_probe.py [--out profiles/components_nowcast.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


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


def ensemble(P, seed=1):
    """P sums of a trend, a season and a smooth rest; every fourth rest is a ChangePoint"""
    from nowcastautogp_amd import gp
    rng = np.random.default_rng(seed)
    out = []
    for p in range(P):
        lin = gp.Linear(rng.uniform(0.2, 0.8), rng.uniform(0.05, 0.2), rng.uniform(0.3, 1.0))
        per = gp.Periodic(rng.uniform(0.8, 1.5), rng.uniform(0.02, 0.2), rng.uniform(0.2, 0.6))
        se = gp.SquaredExponential(rng.uniform(0.05, 0.3), rng.uniform(0.2, 0.5))
        rest = (gp.ChangePoint(se, gp.GammaExponential(0.2, 1.4, 0.3), rng.uniform(0.3, 0.7), 0.05)
                if p % 4 == 3 else se)
        out.append(gp.to_program(gp.Plus(gp.Plus(lin, per), rest)) + (rng.uniform(0.02, 0.1),))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--particles", type=int, default=64)
    ap.add_argument("--n", type=int, default=2049)
    ap.add_argument("--m", type=int, default=28)
    ap.add_argument("--d", type=int, default=2)
    ap.add_argument("--scenarios", type=int, default=200)
    ap.add_argument("--skip-components", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not os.environ.get("NGP_LIB"):
        ge.build()
    from nowcastautogp_amd import _lib
    ctx = _lib.Context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    P, n, m, C, d, D = a.particles, a.n, a.m, 3, a.d, a.scenarios
    progs = ensemble(P)
    rng = np.random.default_rng(2)
    t = np.arange(n) / (n - 1.0)
    y = 0.8 * (t - 0.4) + 0.5 * np.sin(2 * np.pi * t / 0.07) + 0.1 * rng.standard_normal(n)
    t_add = 1.0 + np.arange(1, d + 1) / (n - 1.0)
    y_add = 0.4 + 0.3 * rng.standard_normal((D, d))
    t_comp = t_add[-1] + np.arange(1, m + 1) / (n - 1.0)
    t_ref = t_add[-1] + np.arange(1, C * m + 1) / (n - 1.0)
    say(f"# component_nowcast_probe: {P} particles, n = {n}, d = {d}, D = {D}, C = {C}, m = {m} "
        f"({C * m} swept rows); warm-up {a.warmup}, {a.reps} timed calls, median [min, max] ms wall")
    fac = ctx.factor(progs, t, y)

    def classes(fn):
        ctx.profile_enable(True)
        ctx.profile_reset()
        fn()
        pr = ctx.profile_get()
        ctx.profile_enable(False)
        return ", ".join(f"{k} {v['ms']:.3f} ms / {v['launches']}" for k, v in pr.items() if v["launches"])

    def reference():
        o = fac.nowcast(t_add, y_add, t_ref, noise_on_new=False)
        assert not o["info"].any()

    r = timed(reference, a.warmup, a.reps)
    say(f"ngp_factor_nowcast  d = {d}, D = {D}, m = {C * m}: {r[0]:8.3f} [{r[1]:.3f}, {r[2]:.3f}] ms")
    say(f"    device time by class: {classes(reference)}")
    comps = [_lib.kernel_components(p) for p in progs]
    assert all(len(c) == C for c in comps)

    def plain():
        o = fac.components(comps, t_comp)
        assert not o["info"].any()

    q = timed(plain, a.warmup, a.reps)
    say(f"ngp_factor_components C = {C}, m = {m}: {q[0]:8.3f} [{q[1]:.3f}, {q[2]:.3f}] ms")
    say(f"    device time by class: {classes(plain)}")
    if not a.skip_components:

        def decomposition(want_sigma=True):
            o = fac.components_nowcast(comps, t_add, y_add, t_comp, want_sigma=want_sigma)
            assert not o["info"].any()

        c = timed(decomposition, a.warmup, a.reps)
        v = timed(lambda: decomposition(False), a.warmup, a.reps)
        say(f"ngp_factor_components_nowcast d = {d}, D = {D}, C = {C}, m = {m}: {c[0]:8.3f} [{c[1]:.3f}, {c[2]:.3f}] ms "
            f"(var alone: {v[0]:.3f} [{v[1]:.3f}, {v[2]:.3f}]) = {c[0] / r[0]:.2f} x the reference query")
        say(f"    device time by class: {classes(decomposition)}")
    fac.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()

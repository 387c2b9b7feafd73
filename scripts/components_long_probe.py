"""Times ONE decomposition over a daily grid of a year (ngp_factor_components_long through
autogp.predict_components / nowcast.forecast_components_with_nowcasts with one_query=True) against
the blockwise default of the same two functions (component_blocks over ngp_factor_components /
ngp_factor_components_nowcast), in one run on one device:

    python scripts/components_long_probe.py [--reps 5] [--out profiles/components_long_probe.json]

Shapes: (P = 64, n = 2,047, C = 3, m = 365) and (P = 24, n = 208, C = 3, m = 365), each without
appended points (d = 0) and with d = 7, D = 200.  Every particle is Plus(Plus(Linear, Periodic),
SquaredExponential) with its own parameters, placed in an unfitted model (the decomposition does not
care where the particles came from).  Per case: the wall time of the mirror call, copies and host
assembly included (median [min, max] of --reps calls after one warm-up), the wall time of the bare
library call with and without sigma, the number of block queries of the default path, the worst
difference of the two paths' means and variances, and the library's per-class profile of one call.
With d > 0 both mirror calls include the weight update's own query, which is the same on both
sides.  A tool, not a test."""
import argparse
import datetime as dt
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return dict(median=float(np.median(out)), min=float(np.min(out)), max=float(np.max(out)))


def make_model(autogp, gp, eng, P, n):
    rng = np.random.default_rng(1000 + n)
    ds = [dt.date(2015, 1, 1) + dt.timedelta(days=i) for i in range(n)]
    i = np.arange(n)
    y = 50.0 + 0.01 * i + 5.0 * np.sin(2 * np.pi * i / 365.25) + rng.standard_normal(n)
    model = autogp.GPModel(ds, y, n_particles=P, engine=eng, seed=1)
    model.n_obs = n
    model.particles = [
        autogp.Particle(gp.Plus(gp.Plus(gp.Linear(*rng.uniform(0.1, 0.6, 3)),
                                        gp.Periodic(rng.uniform(0.5, 1.2), rng.uniform(0.1, 0.3), rng.uniform(0.3, 0.8))),
                                gp.SquaredExponential(rng.uniform(0.05, 0.3), rng.uniform(0.2, 0.6))),
                        float(rng.uniform(0.05, 0.15)))
        for _ in range(P)]
    t, yy = model._obs()
    lm, info = eng.logml(model.programs(), t, yy)
    assert not np.any(info), info
    model._logml = np.asarray(lm, dtype=np.float64).copy()
    return model, ds, y


def worst(a, b):
    return float(max(np.max(np.abs(x - y)) / np.max(np.abs(y)) for x, y in zip(a, b)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 5
    import __graft_entry__ as ge
    ge.build()
    from nowcastautogp_amd import autogp, gp
    from nowcastautogp_amd import nowcast as nc
    eng = autogp.HipEngine(0)
    ctx = eng.ctx
    ctx.set_combining(False)
    m, C = 365, 3
    res = dict(reps=a.reps, cases=[])
    for P, n in ((64, 2047), (24, 208)):
        model, ds, y = make_model(autogp, gp, eng, P, n)
        for d, D in ((0, 1), (7, 200)):
            rng = np.random.default_rng(7)
            nd = [ds[-1] + dt.timedelta(days=k + 1) for k in range(d)]
            fd = [ds[-1] + dt.timedelta(days=d + k + 1) for k in range(m)]
            nows = [nc.TData(nd, list(y[-1] + rng.standard_normal(d)), transformation=lambda v: v)
                    for _ in range(D)]
            if d == 0:
                def blockwise():
                    return autogp.predict_components(model, fd)

                def one_query(want_sigma=False):
                    return autogp.predict_components(model, fd, one_query=True, want_sigma=want_sigma)
            else:
                def blockwise():
                    return nc.forecast_components_with_nowcasts(model, nows, fd, split="plus")

                def one_query(want_sigma=False):
                    return nc.forecast_components_with_nowcasts(model, nows, fd, split="plus",
                                                                one_query=True, want_sigma=want_sigma)
            blocks = autogp.component_blocks(n, C, m, d)
            row = dict(P=P, n=n, C=C, m=m, d=d, D=D, block_queries=len(blocks),
                       blockwise_ms=timed_ms(blockwise, a.reps),
                       one_query_ms=timed_ms(one_query, a.reps),
                       one_query_sigma_ms=timed_ms(lambda: one_query(True), a.reps))
            ref, got = blockwise(), one_query()
            row["max_rel_diff_means"] = worst(got.means, ref.means)
            row["max_rel_diff_var"] = worst(got.var, ref.var)
            # the bare library call, and its profile
            fac = model._factor()
            parts = autogp.decompose(model, "plus")
            comps = [[gp.to_program(c.tree) + (0.0,) for c in ps] for ps in parts]
            t_new = model.ds_transform.apply(autogp.to_days(fd))
            t_add = model.ds_transform.apply(autogp.to_days(nd)) if d else None
            y_add = np.stack([model.y_transform.apply(np.asarray(w.y, dtype=np.float64)) for w in nows]) if d else None
            row["library_call_ms"] = timed_ms(lambda: fac.components_long(comps, t_new, t_add, y_add), a.reps)
            row["library_call_sigma_ms"] = timed_ms(
                lambda: fac.components_long(comps, t_new, t_add, y_add, want_sigma=True), a.reps)
            ctx.profile_enable(True)
            ctx.profile_reset()
            fac.components_long(comps, t_new, t_add, y_add)
            row["profile_one_call"] = ctx.profile_get()
            ctx.profile_reset()
            fac.components_long(comps, t_new, t_add, y_add, want_sigma=True)
            row["profile_one_call_sigma"] = ctx.profile_get()
            ctx.profile_enable(False)
            res["cases"].append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

"""Times ONE hindcast query (ngp_factor_predict_origins: R forecast origins x m dates from the
resident factor) against the only route there was before it — one factor on the prefix per origin,
each followed by a long query without sigma — in one run on one device:

    python scripts/origins_probe.py [--reps 5] [--out profiles/origins_probe.json]

(a) P = 64, n = 2,047, m = 365 daily dates from the middle of the series on, R = 52 weekly origins
    ending at n: wall time of Factor.predict_origins (copies included; median [min, max] of --reps
    calls after one warm-up), wall time of the R prefix factors + long queries (one pass after a
    warm-up of the first and last origin: it is R factorisations), the ratio, and the worst
    difference between the two.
(b) the pass over the solved panel alone: the same call with every origin inside the main block and
    without the evidence, so that profile class 3 holds that pass, the conditioning block of the tail
    and nothing else; its time against 8 qpad n0 P bytes at the copy rate ngp_microbench_hbm reports
    in the same process, and against the solve (class 6) of the same call.
A tool, not a test."""
import argparse
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


def programs(P, seed=3):
    """Plus(Plus(Linear, Periodic), SquaredExponential), own parameters per particle (RPN)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(P):
        par = np.concatenate([rng.uniform(0.1, 0.6, 3), [rng.uniform(0.5, 1.2), rng.uniform(0.1, 0.3),
                                                         rng.uniform(0.3, 0.8)],
                              [rng.uniform(0.05, 0.3), rng.uniform(0.2, 0.6)]])
        out.append((np.array([2, 5, 6, 3, 6], np.int32), par, float(rng.uniform(0.05, 0.15))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 5
    import __graft_entry__ as ge
    ge.build()
    from nowcastautogp_amd import _lib
    ctx = _lib.Context(0)
    ctx.set_combining(False)
    P, n, m, R = 64, 2047, 365, 52
    n0 = n // 64 * 64
    progs = programs(P)
    t = np.arange(n) / n
    rng = np.random.default_rng(11)
    y = np.sin(2 * np.pi * np.arange(n) / 365.25) + 0.3 * t + 0.2 * rng.standard_normal(n)
    t_new = t[n // 2] + np.arange(m) / n
    cuts = np.arange(n - 7 * (R - 1), n + 1, 7).astype(np.int32)
    assert cuts.size == R and cuts[-1] == n
    res = dict(reps=a.reps, P=P, n=n, m=m, R=R)
    fac = ctx.factor(progs, t, y)

    # (a) the call against R prefix factors, each with its long query
    res["predict_origins_ms"] = timed_ms(lambda: fac.predict_origins(cuts, t_new), a.reps)
    mu, var, lm, info = fac.predict_origins(cuts, t_new)
    assert not info.any()

    def prefix_route(cs):
        out = []
        for c in cs:
            g = ctx.factor(progs, t[:c], y[:c])
            try:
                pm, pv, _, pinfo = g.predict_long(t_new, want_sigma=False)
                plm, _ = g.logml()
            finally:
                g.close()
            assert not pinfo.any()
            out.append((pm[:, 0], pv, plm))
        return out
    prefix_route(cuts[[0, -1]])
    t0 = time.perf_counter()
    ref = prefix_route(cuts)
    res["prefix_factors_ms"] = 1e3 * (time.perf_counter() - t0)
    res["ratio"] = res["prefix_factors_ms"] / res["predict_origins_ms"]["median"]
    res["max_rel_diff_mean"] = float(max(np.max(np.abs(mu[:, r] - ref[r][0])) / np.max(np.abs(ref[r][0])) for r in range(R)))
    res["max_rel_diff_var"] = float(max(np.max(np.abs(var[:, r] - ref[r][1])) / np.max(np.abs(ref[r][1])) for r in range(R)))
    res["max_rel_diff_logml"] = float(max(np.max(np.abs(lm[:, r] - ref[r][2]) / np.abs(ref[r][2])) for r in range(R)))

    # (b) the pass over the panel alone
    write_gbs, copy_gbs = ctx.microbench_hbm()
    inside = cuts[cuts <= n0]
    qpad = (1 + (n - n0) + m + 63) // 64 * 64
    lib = _lib.load()
    mu_b, var_b = np.empty((P, inside.size, m)), np.empty((P, inside.size, m))
    info_b = np.zeros(P, np.int32)

    def bare():
        st = lib.ngp_factor_predict_origins(fac._h, inside.size, _lib.iptr(inside), m, _lib.dptr(t_new), 1,
                                            _lib.dptr(mu_b), _lib.dptr(var_b), None, _lib.iptr(info_b))
        assert st == 0, st
    bare()
    ctx.profile_enable(True)
    prof = []
    for _ in range(a.reps):
        ctx.profile_reset()
        bare()
        prof.append(ctx.profile_get())
    ctx.profile_enable(False)
    names = list(prof[0])
    res["profile_main_block_origins"] = {k: dict(ms_median=float(np.median([p[k]["ms"] for p in prof])),
                                                 ms_min=float(np.min([p[k]["ms"] for p in prof])),
                                                 launches=prof[0][k]["launches"]) for k in names}
    res["origins_inside_main_block"] = int(inside.size)
    res["hbm_write_gbs"], res["hbm_copy_gbs"] = write_gbs, copy_gbs
    res["panel_bytes"] = 8 * qpad * n0 * P
    res["panel_read_ms_at_copy_rate"] = 1e3 * res["panel_bytes"] / (copy_gbs * 1e9)
    fac.close()
    print(json.dumps(res, indent=1), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()

"""Staged jobs that are run again after a job of another shape has used the context.

A staged run takes its working storage (factor slabs, tables, K^-1) from the context's one workspace
and leaves results, logdet and info in the job's arena; a run of a differently shaped job in between
overwrites the workspace, and the re-run has to clear what the first run left.  The sequences of
tests/sanitize/staged_calls.h (value jobs with packed and unpacked results, a mixed-precision job
with refinement, a job without a main block, a resident factor's query, a gradient job on the
general leaf, a small mixed gradient batch with both leaves side by side, a trajectory with and
without a trace) live on ONE context.  Each is run and fetched, then run and fetched again after
another sequence's job, in an order in which no job follows the job it followed before.

The repeat is compared bitwise, info arrays included.  Before this was fixed the same script ran
against the library of the parent commit (NGP_LIB): every repeat was bitwise there too, so equality
is what is asserted.  Success paths only."""
import numpy as np
import pytest

from nowcastautogp_amd import _abi, _lib

pytestmark = pytest.mark.gpu

STAT = ([3, 5, 6], [0.3, 0.8, 0.4, 0.25, 0.5])       # SqExp + Periodic
NONSTAT = ([2, 3, 7], [0.5, 0.1, 0.5, 0.2, 0.7])     # Linear x SqExp
PRIOR = {k: {"mu": 0.0, "sigma": 1.0} for k in ("gamma", "period", "wildcard")}


def _trees(B, stationary, scale=1.0):
    out = []
    for i in range(B):
        ops, par = STAT if stationary(i) else NONSTAT
        par = [scale * p for p in par]
        par[0 if stationary(i) else 3] += 0.01 * i
        out.append((ops, par, 0.02 + 0.01 * i))
    return out


def _series(n, d, D, m, lattice=True):
    i = np.arange(n + d + m, dtype=np.float64)
    if not lattice:
        i = i + 0.3 * np.modf(i * 0.6180339887498949)[0]
    t = i / 128.0
    y = ((np.arange(n) * 37) % 11) / 11.0 - 0.5
    y_add = 0.1 * (np.arange(D * d) % 3).reshape(D, d)
    return t[:n], y, t[n:n + d], y_add, t[n + d:]


def _value(ctx, P, n, d, D, m, precision=_abi.NGP_PREC_F64):
    t, y, t_add, y_add, t_new = _series(n, d, D, m)
    old = ctx.get_spec()
    spec = ctx.get_spec()
    spec.precision = precision          # a staged job keeps the spec it was staged under
    ctx.set_spec(spec)
    job = ctx.stage_nowcast(_trees(P, lambda i: i % 2 == 0), t, y, t_add, y_add, t_new)
    ctx.set_spec(old)

    def run():
        r = job.run().fetch()
        return [r[k] for k in ("logml_base", "logml_full", "mu", "sigma", "info")]
    return run


def _factor(ctx):
    t, y, t_add, y_add, t_new = _series(136, 2, 2, 3)
    f = ctx.factor(_trees(3, lambda i: i % 2 == 0), t, y)

    def run():
        r = f.nowcast(t_add, y_add, t_new)
        return [r[k] for k in ("logml_base", "logml_full", "mu", "sigma", "info")]
    return run


def _grad(ctx, B, n, stationary, lattice, invariant=False):
    t, y = _series(n, 0, 1, 0, lattice)[:2]
    first, moved = (_abi.KernelArray(_trees(B, stationary, s)) for s in (1.0, 1.0625))
    ctx.set_batch_invariant(invariant)   # a small mixed batch then runs its two leaves side by side
    job = ctx.stage_grad(first, t, y)
    ctx.set_batch_invariant(False)
    assert job.info()["side_by_side"] == invariant
    return job, first, moved


def _grad_runs(ctx, *args):
    job, first, moved = _grad(ctx, *args)
    return lambda: [*job.run(first), *job.run(moved)]


def _hmc_runs(ctx, trace):
    job, first, _ = _grad(ctx, 3, 70, lambda i: False, False)
    n_lat = job._ngrad

    def run():
        r = job.hmc(np.zeros(n_lat, dtype=np.uint8), np.full(n_lat, 0.125), np.full(n_lat, 0.25), 2, 0.01, PRIOR,
                    trace=trace)
        return [r[k] for k in sorted(r)]
    return run


def test_staged_jobs_repeat_bitwise_after_a_job_of_another_shape():
    import __graft_entry__ as ge
    ge.build()
    ctx = _lib.Context(0)
    try:
        runs = {
            "value P=3 n=136 m=3": _value(ctx, 3, 136, 2, 2, 3),
            "value P=5 n=136 m=170 (unpacked fetch)": _value(ctx, 5, 136, 2, 2, 170),
            "value P=3 n=128 mixed, refined": _value(ctx, 3, 128, 2, 2, 3, _abi.NGP_PREC_MIXED),
            "value P=3 n=40 (no main block)": _value(ctx, 3, 40, 2, 2, 3),
            "factor P=3 n=136 nowcast": _factor(ctx),
            "gradient B=3 n=70 general leaf": _grad_runs(ctx, 3, 70, lambda i: False, False),
            "gradient B=4 n=260 side by side": _grad_runs(ctx, 4, 260, lambda i: i % 2 == 0, True, True),
            "trajectory B=3 n=70 with a trace": _hmc_runs(ctx, True),
            "trajectory B=3 n=70": _hmc_runs(ctx, False),
        }
        names = list(runs)
        # the second order: no job follows the job it followed in the first
        again = names[::-3] + names[-2::-3] + names[-3::-3]
        assert sorted(again) == sorted(names) and again != names
        first = {n: runs[n]() for n in names}
        second = {n: runs[n]() for n in again}
    finally:
        ctx.close()
    for n in names:
        a = [np.ascontiguousarray(x) for x in first[n]]
        b = [np.ascontiguousarray(x) for x in second[n]]
        worst = max(float(np.max(np.abs(x.astype(np.float64) - y.astype(np.float64)), initial=0.0))
                    for x, y in zip(a, b))
        print(f"{n}: {len(a)} arrays, {sum(x.nbytes for x in a)} bytes, largest difference {worst:.3e}")
        assert all(np.isfinite(x).all() for x in a), f"{n}: a result is not finite"
        assert [x.tobytes() for x in a] == [x.tobytes() for x in b], f"{n}: the repeat differs ({worst:.3e})"

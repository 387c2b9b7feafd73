#!/usr/bin/env python3
"""Results of calls that reach every kernel of ngp_tree_kernels.h and ngp_grad_kernels.h, written to
an .npz: run once per build (NGP_LIB selects the library) and compare the files bit for bit
(scripts/k8_dump.py does the same for the column sweep).  Inputs as in tests/value_cases.py and
tests/test_routes_gpu.py.  Usage: python scripts/route_dump.py OUT.npz"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nowcastautogp_amd import _lib
from nowcastautogp_amd._abi import KernelArray, default_spec, NGP_PREC_MIXED
from nowcastautogp_amd.synthetic import make_workload
from tests.value_cases import ensemble, series

out = {}
VAL = ("logml_base", "logml_full", "mu", "sigma", "info")


def put(tag, r):
    for k in VAL:
        out[f"{tag}_{k}"] = np.asarray(r[k])


def grad(ctx, tag, progs, t, y):
    lm, g, info = ctx.logml_grad_flat(KernelArray(progs), t, y)
    out[f"{tag}_lm"], out[f"{tag}_grad"], out[f"{tag}_info"] = lm, g, info


def value_inputs(n, lattice, B, seed):
    """stationary, chain (Linear / ChangePoint folds) and general trees in one chunk"""
    t, y = series(n + 2, lattice, seed=seed)
    progs = ensemble(seed, [1, 3, 5, 7, 9], B, linear_every=3, cp_every=4)
    t_new = t[-1] + (t[-1] - t[-2]) * np.arange(1, 6)
    return progs, t[:n], y[:n], t[n:], np.tile(y[n:], (3, 1)), t_new


ctx = _lib.Context(0)
for lattice in (True, False):
    tag = "lat" if lattice else "irr"
    progs, t, y, t_add, y_add, t_new = value_inputs(333, lattice, 48, 5)
    # ngp_cov_batch: cov_kernel
    out[f"{tag}_cov"] = ctx.cov_batch(progs[:8], t[:70], t[:50], add_diag=True)
    # unstaged and staged value jobs: fill_kernel (irregular); tables, fill_lattice / fill_single /
    # fill_chain (lattice; the staged fp64 job on a regular series is a Toeplitz job)
    put(f"{tag}_now", ctx.nowcast_batch(progs, t, y, t_add, y_add, t_new))
    job = ctx.stage_nowcast(progs, t, y, t_add, y_add, t_new)
    job.run()
    put(f"{tag}_staged", job.fetch())
    job.close()
    # cached factor: the aux rows only (launch_fill with aux_only)
    f = ctx.factor(progs, t, y)
    out[f"{tag}_factor_logml"], out[f"{tag}_factor_info"] = f.logml()
    put(f"{tag}_factor_now", f.nowcast(t_add, y_add, t_new))
    f.close()
    # gradients: the short-series path, the list kernels, every tree-size bucket up to the general
    # contraction kernel; irregular times run grad_contract_kernel
    for n, B in ((130, 24), (448, 40)):
        tg, yg = series(n, lattice, seed=8)
        grad(ctx, f"{tag}_grad{n}", ensemble(18, [1, 3, 5, 7, 9, 15, 17, 31, 33, 63], B,
                                             linear_every=7, cp_every=11), tg, yg)
# the Toeplitz gradient: stationary trees only, on a regular series
tg, yg = series(448, True, seed=8)
grad(ctx, "toep_grad", ensemble(3, [1, 3, 5, 7], 32), tg, yg)
# the bench ensembles
for ens in ("prior", "fitted"):
    wg = make_workload("C3", n=520, P=64, D=1, d=1, m=9, ensemble=ens)
    grad(ctx, f"c3_{ens}", wg.programs, wg.t, wg.y)
ctx.close()

# mixed precision: the Gram refinement runs kapply_kernel in all four modes, the fill leaves auxX
mctx = _lib.Context(0, default_spec(NGP_PREC_MIXED))
for lattice in (True, False):
    tag = "mixlat" if lattice else "mixirr"
    progs, t, y, t_add, y_add, t_new = value_inputs(700, lattice, 24, 6)
    put(tag, mctx.nowcast_batch(progs, t, y, t_add, y_add, t_new))
mctx.close()

np.savez(sys.argv[1], **out)
print("wrote", sys.argv[1], len(out), "arrays; info all zero:",
      all(not v.any() for k, v in out.items() if k.endswith("info")))

"""The tile rule of NGP_PREC_MIXED restated on the host (TEST INFRASTRUCTURE ONLY; plain numpy, no
device code is read at run time).  DESIGN.md section 4.8, include/ngp.h ``ngp_spec::mixed_tau``.

What the device does, and what is restated here:

  maxima     every finished 64 x 64 tile of L (main rows) and of W = X L^-T (aux rows, in the
             job's order: tail of n mod 64 observations | appended points | forecast dates | y')
             records its largest magnitude, rounded UP to fp32.  Here: numpy's fp64 Cholesky of the
             oracle's covariance.  The device's maxima come from its own (mixed) factor and differ
             from these in the last digits, hence the count of BORDERLINE products below.
  schedule   block columns go in pairs (``col_pair_offset`` / ``col_step`` of ngp_plan.h): an odd
             count of at least 3 sends column 0 alone (FULL step) and pairs from column 1.  The fat
             step of pair (j, j + 1) has the row tiles j + 1 .. nb0 - 1 and then the aux tiles;
             a workgroup takes two consecutive ones (rt0, rt1; an odd count leaves the last
             workgroup with one tile) and classifies the k-tiles 0 .. j - 1.
  rule       k-tile kt of a workgroup runs in fp32 iff
                 max(tm[j, kt], tm[j + 1, kt]) * max(tm[rt0, kt], tm[rt1, kt]) <= lim,
                 lim = mixed_tau / (64 * 2^-24) * (noise + jitter)
             — the maxima of the PAIRS of tiles a workgroup multiplies, which is what the header
             states ("max|A tiles| max|B tiles|"); it is stricter than a rule per single tile.
  counts     a workgroup adds 2 * min(2, ntiles - tile0) (its wave tiles) per k-tile to the item's
             fp32 or fp64 count; ``frac_f32`` = n32 / (n32 + n64).  FULL and thin steps, the
             diagonal tiles and the epilogue are fp64 and count nothing.

``emulate`` runs the same blocked factorisation with fp32-rounded operands (one k-tile per fp32
accumulation, sums in fp64) on the products its own running maxima select, and returns log det.
"""
from __future__ import annotations

import numpy as np
from scipy.linalg import cholesky, solve_triangular

from oracle import oracle_np
from tests.blocked_model import NB

BORDER_REL = 1e-5          # a product is borderline when |ta tb / lim - 1| is below this
U24 = 5.9604644775390625e-08   # 2^-24


def f32_up(x):
    """fp64 -> fp32 rounded towards +inf (the device's __double2float_ru), for x >= 0"""
    x = np.asarray(x, np.float64)
    f = x.astype(np.float32)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def limit(noise, mixed_tau, jitter):
    """right-hand side of the rule for products of maxima: c32 (noise + jitter)"""
    return mixed_tau / (64.0 * U24) * (noise + jitter)


# ---- schedule (ngp_plan.h) ---------------------------------------------------------------------
def col_pair_offset(nb0):
    return 1 if (nb0 >= 3 and nb0 % 2 == 1) else 0


def col_step(nb0, jj):
    """'fat' / 'thin' / 'full' for block column jj"""
    o = col_pair_offset(nb0)
    if jj >= o and (jj - o) % 2 == 0 and jj + 1 < nb0:
        return "fat"
    return "thin" if (jj >= o and (jj - o) % 2 == 1) else "full"


def fat_workgroups(nb0, naux_tiles, j):
    """(rt0, rt1, weight) of every workgroup of the fat step of pair (j, j + 1): indices into the
    maxima table (main row tiles 0 .. nb0 - 1, aux tiles nb0 ..)"""
    nmain = nb0 - 1 - j
    ntiles = nmain + naux_tiles

    def rt(tile):
        return j + 1 + tile if tile < nmain else nb0 + (tile - nmain)

    return [(rt(t0), rt(min(t0 + 1, ntiles - 1)), 2 * min(2, ntiles - t0)) for t0 in range(0, ntiles, 2)]


def mixed_eligible(nb0):
    return 2 <= nb0 <= 129


# ---- maxima ----------------------------------------------------------------------------------------
def aux_rows(program, t, y, t_new, spec=None, t_add=()):
    """(n0, X): the aux rows as the job lays them out — k(tail and appended dates, t0), k(forecast
    dates, t0), y' — before the solve"""
    t, y = np.asarray(t, float), np.asarray(y, float)
    n0 = (t.size // NB) * NB
    ta = np.concatenate([t[n0:], np.asarray(t_add, float)])
    t0 = t[:n0]
    X = np.vstack([oracle_np.cov(program, ta, t0, False, spec),
                   oracle_np.cov(program, np.asarray(t_new, float), t0, False, spec), y[None, :n0]])
    return n0, X


def factor_and_aux(program, t, y, t_new, spec=None, t_add=()):
    """L of the main block (fp64, LAPACK) and W = X L^-T, W padded with zero rows to whole tiles"""
    n0, X = aux_rows(program, t, y, t_new, spec, t_add)
    K = oracle_np.cov(program, np.asarray(t, float)[:n0], np.asarray(t, float)[:n0], True, spec)
    L = cholesky(K, lower=True, check_finite=False, overwrite_a=True)
    W = solve_triangular(L, X.T, lower=True, check_finite=False).T
    pad = -W.shape[0] % NB
    return L, np.vstack([W, np.zeros((pad, n0))])


def tile_maxima(L, W):
    """tm[row tile, column tile] (fp32, rounded up): main row tiles, then the aux tiles.  Tiles on and
    above the block diagonal are never read by a fat step and are left at their (meaningless) value."""
    A = np.abs(np.vstack([L, W]))
    nb0 = L.shape[0] // NB
    return f32_up(A.reshape(A.shape[0] // NB, NB, nb0, NB).max(axis=(1, 3)))


# ---- rule and counts ---------------------------------------------------------------------------------
def classify(tm, lim, nb0, naux_tiles, j, second_tile=True, scale=1.0):
    """per workgroup of fat step j: (weight, fp32 mask over k-tiles 0 .. j - 1, borderline mask).
    second_tile=False / scale != 1 are deliberate MISTAKES (the second tile of each pair is ignored /
    every maximum is scaled), for checking that the counts can tell."""
    out = []
    tm = tm.astype(np.float64) * scale
    for rt0, rt1, w in fat_workgroups(nb0, naux_tiles, j):
        ta = np.maximum(tm[j, :j], tm[j + 1, :j]) if second_tile else tm[j, :j]
        tb = np.maximum(tm[rt0, :j], tm[rt1, :j]) if second_tile else tm[rt0, :j]
        prod = ta * tb
        out.append((w, prod <= lim, np.abs(prod / lim - 1.0) < BORDER_REL))
    return out


def counts(tm, lim, nb0, naux_tiles, **mistake):
    """(n32, n64, borderline): weighted tile products of one item over all its fat steps"""
    n32 = n64 = nbd = 0
    if not mixed_eligible(nb0):
        return 0, 0, 0
    for j in range(nb0):
        if col_step(nb0, j) != "fat":
            continue
        for w, m32, bd in classify(tm, lim, nb0, naux_tiles, j, **mistake):
            n32 += w * int(m32.sum())
            n64 += w * int((~m32).sum())
            nbd += w * int(bd.sum())
    return n32, n64, nbd


def item_counts(program, t, y, t_new, mixed_tau, jitter, spec=None, t_add=(), **mistake):
    """the model of one item: dict(n32, n64, borderline, frac)"""
    L, W = factor_and_aux(program, t, y, t_new, spec, t_add)
    nb0, nat = L.shape[0] // NB, W.shape[0] // NB
    tm = tile_maxima(L, W)
    n32, n64, nbd = counts(tm, limit(program[2], mixed_tau, jitter), nb0, nat, **mistake)
    return dict(n32=n32, n64=n64, borderline=nbd, frac=n32 / (n32 + n64) if n32 + n64 else 0.0, tm=tm)


# ---- the blocked factorisation with fp32 tile products -------------------------------------------------
def _prod(A, B, f32):
    if not f32:
        return A @ B.T
    return (A.astype(np.float32) @ B.astype(np.float32).T).astype(np.float64)


def emulate(program, t, y, t_new, mixed_tau, jitter, spec=None, every=False, t_add=()):
    """log det of the main block's covariance from the device's schedule: fat steps accumulate
    k-tiles 0 .. j - 1 into columns j and j + 1 (the diagonal tile (j + 1, j + 1) included: it is the
    sibling wave's tile of the first row tile), in fp32 where the workgroup's rule says so
    (every=True: everywhere), thin steps add k-tile j in fp64, diagonal tiles (j, j) of fat columns
    and FULL columns are fp64.  Returns (log det, n32, n64)."""
    n0, X = aux_rows(program, t, y, t_new, spec, t_add)
    t0 = np.asarray(t, float)[:n0]
    K = oracle_np.cov(program, t0, t0, True, spec)
    pad = -X.shape[0] % NB
    M = np.vstack([K, X, np.zeros((pad, n0))])      # rows: main tiles, then aux tiles
    nb0, nrt = n0 // NB, M.shape[0] // NB
    nat = nrt - nb0
    lim = limit(program[2], mixed_tau, jitter)
    Lm = np.zeros_like(M)
    tm = np.zeros((nrt, nb0), np.float32)
    sl = lambda i: slice(i * NB, (i + 1) * NB)
    logdet, n32, n64 = 0.0, 0, 0

    def finish(j, S):
        """column j from the accumulated S[rt] (rt >= j): diagonal factor, panel solve, maxima"""
        nonlocal logdet
        Ljj = np.linalg.cholesky(M[sl(j), sl(j)] - S[j])
        Lm[sl(j), sl(j)] = Ljj
        logdet += 2.0 * np.log(np.diag(Ljj)).sum()
        for r in range(j + 1, nrt):
            Lm[sl(r), sl(j)] = solve_triangular(Ljj, (M[sl(r), sl(j)] - S[r]).T, lower=True).T
            tm[r, j] = f32_up(np.abs(Lm[sl(r), sl(j)]).max())

    def full64(j, rows):
        return {r: Lm[sl(r), :j * NB] @ Lm[sl(j), :j * NB].T for r in rows}

    j = 0
    while j < nb0:
        if col_step(nb0, j) != "fat":
            finish(j, full64(j, range(j, nrt)))
            j += 1
            continue
        Sj = full64(j, [j])                                   # diag tile (j, j): fp64 (diag_ahead)
        Sj1 = {}
        for (rt0, rt1, w), (_, m32, _) in zip(fat_workgroups(nb0, nat, j), classify(tm, lim, nb0, nat, j)):
            if every:
                m32 = np.ones(j, bool)
            n32 += w * int(m32.sum())
            n64 += w * int((~m32).sum())
            for r in sorted({rt0, rt1}):
                a = np.zeros((NB, NB))
                b = np.zeros((NB, NB))
                for kt in range(j):
                    a += _prod(Lm[sl(r), sl(kt)], Lm[sl(j), sl(kt)], m32[kt])
                    b += _prod(Lm[sl(r), sl(kt)], Lm[sl(j + 1), sl(kt)], m32[kt])
                Sj[r], Sj1[r] = a, b
        finish(j, Sj)
        for r in Sj1:                                         # thin step: k-tile j, fp64
            Sj1[r] += Lm[sl(r), sl(j)] @ Lm[sl(j + 1), sl(j)].T
        finish(j + 1, Sj1)
        j += 2
    return logdet, n32, n64

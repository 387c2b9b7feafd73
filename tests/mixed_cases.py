"""The inputs of the mixed-precision tile tests (tests/test_mixed_model_cpu.py proves on the host
that they can fail; tests/test_mixed_tiles_gpu.py runs them on the device).

Dates are a regular grid on [0, 1], so every length scale below is a share of the span.  Squared
exponentials with length scales of 0.02 .. 0.04 put the decay of the tile maxima inside the block
grid at every size used here: tiles next to the block diagonal are O(1), tiles a few block columns
away are below the rule's limit.  The observations are a smooth signal plus noise of the size the
items' noise variances claim, so that the y' row of W = X L^-T stays O(1).
"""
from __future__ import annotations

import numpy as np

from nowcastautogp_amd import gp

TOL_MIXED = 1e-6           # SURVEY.md section 8d (C5), as in tests/test_mixed_gpu.py
M_NEW = 5                  # forecast dates (tests/test_fat_epilogue_gpu.py)
BORDER_SHARE = 0.005       # cap on the borderline weight of an item: a condition on the cases
FRAC_LO, FRAC_HI = 0.2, 0.95

KINDS = ("se", "se+per", "cp", "se2")


def item(kind, rng, noise, period):
    """one program (ops, params, noise) of the given kind with parameters of its own"""
    f = np.exp(0.15 * rng.standard_normal(6))
    ls = lambda lo, hi: float(lo + (hi - lo) * rng.uniform())
    if kind == "se":            # maxima decay away from the block diagonal
        tree = gp.SquaredExponential(ls(0.02, 0.04), 1.5 * f[0])
    elif kind == "se2":
        tree = gp.Plus(gp.SquaredExponential(ls(0.02, 0.03), 2.0 * f[0]), gp.SquaredExponential(ls(0.03, 0.04), 0.5 * f[1]))
    elif kind == "se+per":      # a peaked periodic term: maxima come back at multiples of the period
        tree = gp.Plus(gp.SquaredExponential(ls(0.02, 0.032), 1.2 * f[0]), gp.Periodic(0.1 * f[1], period * f[2], 0.8 * f[3]))
    elif kind == "cp":          # amplitude steps up along the series: so do the maxima
        tree = gp.ChangePoint(gp.SquaredExponential(ls(0.02, 0.04), 0.4 * f[0]), gp.SquaredExponential(ls(0.02, 0.04), 2.5 * f[1]),
                              0.45 * f[2], 0.05)
    elif kind == "fp64":        # tiny noise, and the exponential term's factor decays by e^-1/4 over the whole
        # series (a Periodic alone is of low rank: past its rank the tiles of L drop to sqrt(noise))
        tree = gp.Plus(gp.Periodic(1.0 * f[0], 0.23 * f[1], 1.5), gp.GammaExponential(2.0 * f[2], 1.0, 1.5))
    elif kind == "fp32":        # a weak signal under loud noise: (nearly) every product in fp32
        tree = gp.SquaredExponential(ls(0.02, 0.04), 0.02 * f[0])
    # ---- the sensitive items: length scales of a block column and more, so that the products of a fat
    # step are O(1) against pivots of the size of the noise; under the rule they run in fp64 ----
    elif kind == "long":
        tree = gp.SquaredExponential(ls(0.18, 0.22), (6.0 if noise > 5e-6 else 3.0) * f[0] ** 0.3)
    elif kind == "long+per":
        tree = gp.Plus(gp.SquaredExponential(ls(0.18, 0.22), 3.6 * f[0] ** 0.3), gp.Periodic(1.0 * f[1], 0.5 * f[2], 0.3))
    elif kind == "long-cp":
        tree = gp.ChangePoint(gp.SquaredExponential(ls(0.18, 0.22), 3.6 * f[0] ** 0.3),
                              gp.SquaredExponential(ls(0.18, 0.22), 4.5 * f[1] ** 0.3), 0.5 * f[2], 0.05)
    else:
        raise ValueError(kind)
    return gp.to_program(tree) + (float(noise),)


def batch(n, B, noises=(1e-5, 3e-6, 1e-4, 1e-6), period=1.6, extremes=False, m=M_NEW, seed=0, kinds=KINDS,
          smooth=False):
    """(programs, kinds, t, y, t_new): B items on n dates, kinds and noises cycling; extremes: the
    last two items are the all-fp64 and the nearly all-fp32 one"""
    rng = np.random.Generator(np.random.PCG64(7919 * n + 31 * B + seed))
    progs, names = [], []
    for b in range(B):
        kind, nz = kinds[b % len(kinds)], noises[(b // len(kinds) + b) % len(noises)]
        if extremes and b == B - 2:
            kind, nz = "fp64", 1e-7
        if extremes and b == B - 1:
            kind, nz = "fp32", 1.0
        progs.append(item(kind, rng, nz, period))
        names.append(kind)
    t = np.arange(n) / (n - 1.0)
    if smooth:      # what a length scale of 0.2 can follow
        y = 1.5 * np.sin(5.0 * t) + 0.8 * np.cos(11.0 * t + 1.0) + 3e-3 * rng.standard_normal(n)
    else:
        y = np.sin(40.0 * t) + 0.6 * np.cos(95.0 * t + 1.0) + 0.3 * t + 3e-3 * rng.standard_normal(n)
    t_new = 1.0 + np.arange(1, m + 1) / (n - 1.0)
    return progs, names, t, y, t_new


# ---- counting cases: name -> keyword arguments of batch() ---------------------------------------------
# n0 = 128: one pair, no k-tile; 192: column 0 is FULL, the fat step of pair (1, 2) has k-tile 0 only,
# next to the block diagonal: both count no fp32 product (frac_f32 = 0)
COUNT_ZERO = {f"n{n}_B{B}": dict(n=n, B=B) for n in (128, 192) for B in (3, 17)}
COUNT_CASES = {f"n{n}_B{B}": dict(n=n, B=B) for n in (256, 448, 257, 320 + 17) for B in (3, 17)}
COUNT_CASES.update({
    # three aux tiles (tail 49 + 100 forecast dates + y' = 150 rows)
    "n497_aux150": dict(n=448 + 49, B=3, m=100),
    # two aux tiles: the only way to an odd tile count (the main row tiles of a fat step are always
    # odd in number), i.e. to a last workgroup with ONE tile and weight 2
    "n497_aux100": dict(n=448 + 49, B=3, m=50),
    # two re-rankings (after block columns 8 and 24); the extremes make the ranking a real permutation
    "n2176_B17": dict(n=64 * 34, B=17, period=0.47, extremes=True),
    # odd k-tile counts above 64: the high mask word with odd nkt
    "n4288_B2": dict(n=64 * 67, B=2, period=0.47, seed=1),
    # the largest eligible series, 129 block columns
    "n8319_B2": dict(n=8319, B=2, period=0.47),
})
LARGE = ("n4288_B2", "n8319_B2")     # too long for long double: judged against oracle_np and the fp64 job
REFUSED = dict(n=8320, B=2, period=0.47)    # the first series that runs fp64 whatever the spec says

# ---- accuracy cases: the sensitive items ------------------------------------------------------------------
ACC_KINDS = ("long", "long+per", "long-cp", "se")
ACC_CASES = {f"n{n}": dict(n=n, B=4, noises=(1e-5, 1e-6, 3e-6, 1e-4), seed=1, kinds=ACC_KINDS, smooth=True)
             for n in (256, 448, 512 + 9)}
SENSITIVE_NOISE = 1e-5     # items up to this noise must break when every product runs in fp32


# ---- the model's answers, once per run (the CPU and the GPU tests share them) ------------------------------
ALL_COUNT = {**COUNT_ZERO, **COUNT_CASES}
MIXED_TAU, JITTER = 1e-6, 1e-5     # default_spec(NGP_PREC_MIXED); tests/test_mixed_model_cpu.py checks that they are
_MODEL = {}


def model(kwargs):
    """per item of batch(**kwargs): dict(n32, n64, borderline, frac, tm) of tests/mixed_model.py"""
    from tests import mixed_model
    key = repr(sorted(kwargs.items()))
    if key not in _MODEL:
        progs, _, t, y, t_new = batch(**kwargs)
        _MODEL[key] = [mixed_model.item_counts(p, t, y, t_new, MIXED_TAU, JITTER) for p in progs]
    return _MODEL[key]


def count_error(frac, m):
    """how far the device's frac_f32 is from the model's counts, in weighted tile products, and the
    allowance: the model's borderline weight plus half a product for the rounding of the ratio"""
    return abs(frac * (m["n32"] + m["n64"]) - m["n32"]), m["borderline"] + 0.5

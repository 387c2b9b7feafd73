"""The 16-row grid of the one-launch gradient job, in one table.

A gradient job of at most 256 points is factorised by chol_small_kernel (small_inverse_column
inside it) and finished by grad_kinv_small_kernel (csrc/ngp_small_kernels.h).  Those kernels are cut
along 16-row blocks: for a series of n points their schedule depends on
  nbe = ceil(n / 16)          16-blocks that hold data, 1 .. 16
  rho = n - 16 (nbe - 1)      real rows of the last of them, 1 .. 16
(small_plan deals block column j of L^-1 to a wave per nbe; a column runs nbe - j unrolled stages
against a ring of SM_RING L blocks; the K^-1 k-loop walks [16 a, 16 nbe) in chunks of 64 and zeroes
what it re-reads past the end; logdet and quad stop at n, alpha sums to 16 nbe).  The rows:
  n16k | n16k+1   k = 1 .. 15: the SAME series with one more point — every nbe at rho = 16 and every
                  nbe from 2 on at rho = 1; k = 4, 8, 12 also cross a 64-edge (n0 grows)
  n255 | n256     nbe = 16 at rho = 15 | 16
  n1, n5          the smallest job ngp_grad_stage accepts (it refuses n <= 0 only,
                  csrc/ngp_host_grad.h), and one inside the first block; both from mid-series dates
  n9, n89, n153, n217    rho = 9
  n97_irr, n241_irr      dates off any lattice: the direct fill, no tables, no Toeplitz candidates
  n208_rows       every item its own observation row, Y [9, n] (every other row: one shared y)
  n208_c1e-08, n208_c1, n208_c1e+08   the sampled items with K scaled by c and y by sqrt(c): the
                  condition number stays, the pivots move sixteen decades (scale_program below)
  sweep_n368 | 369, 400 | 401, 432 | 433   the same K^-1 kernel behind the column sweep
                  (nb0 = 6, 7; nbe = 23 .. 28), two sampled items
Nine items (trees of 3, 5, 1 operators; every 4th a Linear chain, the 7th a ChangePoint tree), three
judged: the first stationary, the first Linear, the first ChangePoint.  tests/test_small_grad_gpu.py
runs the rows on the device against tests/hp_reference.py; tests/test_small_grad_cases_cpu.py admits
every judged (row, item) with the fp64 oracle at a quarter of the tolerance, compares the restated
geometry below with the compiled csrc/ngp_plan.h, and shows that a model of the device algebra
(tests/small_grad_model.py) passes the judge and that seven wrong versions of it fail.
Nothing here imports the GPU.
"""
import functools
from dataclasses import dataclass

import numpy as np

from tests.geometry_cases import kind
from tests.value_cases import ensemble, series

TB, NB = 16, 64
B = 9
# (3, 5, 1), not (1, 3, 5): the ChangePoint item of a batch of 9 is item 6 (cp_every = 7), and
# ``ensemble`` gives a ChangePoint only to a tree of at least 3 operators (geometry_cases.VALUE_SIZES)
SIZES = (3, 5, 1)
LINEAR_EVERY, CP_EVERY = 4, 7
# The rule of geometry_cases.ITEM_SEED: the first seed from 41 on with which every judged (row, item)
# is admissible (tests/test_small_grad_cases_cpu.py): the fp64 oracle passes the judgement of the GPU
# file at a quarter of the tolerance, and every reference has info 0, tol_factor 1 and a condition
# number within the floor.  41 is admissible.
ITEM_SEED = 41
JITTER = 1e-5                      # the default spec's
SCALES = (1e-8, 1.0, 1e8)


# ---- the geometry, restated -------------------------------------------------------------------------
def nbe(n):
    return (n + TB - 1) // TB


def rho(n):
    return n - TB * (nbe(n) - 1)


def n0(n):
    return (n + NB - 1) // NB * NB


def inv_len(nbe_, j):
    """stages + 1 of block column j of L^-1 (small_inverse_column: len = nbe - j; W_jj = M_j, then
    len - 1 stages of 1, 2, ... products)"""
    return nbe_ - j


def kinv_chunks(nbe_, a):
    """(64-chunks of the k-loop of a K^-1 block in block row a, live 16-groups of the last chunk)"""
    groups = nbe_ - a
    return (groups + 3) // 4, (groups - 1) % 4 + 1


def kinv_remainder(nbe_, a):
    return (TB * nbe_ - TB * a) % NB


SM_WAVES = 8
SM_RING = 6


def colwave(nbe_):
    """the wave of every block column of L^-1 (small_plan, csrc/ngp_plan.h): longest first, each to
    the wave whose SIMD (waves w and w + 4 share one) carries least, of its two waves the lighter"""
    load = [0] * SM_WAVES
    out = []
    for j in range(nbe_):
        best = 0
        for w in range(1, SM_WAVES):
            sb = load[best % 4] + load[best % 4 + 4]
            sw = load[w % 4] + load[w % 4 + 4]
            if sw < sb or (sw == sb and load[w] < load[best]):
                best = w
        load[best] += (nbe_ - j) * (nbe_ - j - 1) // 2 + 1
        out.append(best)
    return out


def small_plan(n):
    """(nbe, ident, nsweeps, kinds of the sweeps, colwave) of a gradient job of n <= 256 points: the
    main sweep carries y' beside the main block, the inverse phase follows"""
    return nbe(n), 1, 2, (1, 2), colwave(nbe(n))


# ---- items ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def items():
    return tuple(ensemble(ITEM_SEED, list(SIZES), B, True, LINEAR_EVERY, CP_EVERY))


def sample():
    """the first stationary, the first Linear and the first ChangePoint item"""
    kinds = [kind(p) for p in items()]
    return [kinds.index(k) for k in ("stationary", "linear", "changepoint")]


# amplitude parameters of a leaf, by op (Constant: its value; Linear (c, bias, amp): bias and amp;
# the stationary leaves: the last parameter)
_NPAR = {1: 1, 2: 3, 3: 2, 4: 3, 5: 3, 6: 0, 7: 0, 8: 2}
_AMP = {1: (0,), 2: (1, 2), 3: (1,), 4: (2,), 5: (2,)}


def scale_program(program, c):
    """the item whose covariance is c K + c (noise + jitter) I: the noise times c and every
    amplitude parameter times c — of a product's factors the LEFT one only (both would give c^2),
    of a sum and of a ChangePoint both sides.  (The jitter goes with it: scaled_spec.)"""
    ops, params, noise = program
    params = np.array(params, float)
    stack, pi = [], 0                  # per subtree: the parameter indices that scale it
    for op in (int(o) for o in ops):
        if op <= 5:
            stack.append([pi + a for a in _AMP[op]])
        else:
            r, l = stack.pop(), stack.pop()
            stack.append(l if op == 7 else l + r)
        pi += _NPAR[op]
    (idx,) = stack
    params[idx] *= c
    return np.asarray(ops, np.int32), params, float(noise) * c


def scaled_spec(c):
    """the scale rows run with the jitter scaled by c (not with jitter 0): the matrix of the row c is
    exactly c times the matrix of the row 1, the default jitter included"""
    return dict(jitter=JITTER * c)


# ---- rows -------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class SmallCase:
    n: int
    series_n: int              # the series the first n points are taken from
    seed: int
    lattice: bool = True
    per_item_y: bool = False
    c: float = 1.0             # scale rows
    scaled: bool = False
    judged: tuple = ()         # () : sample()
    first: int = 0             # the row's first point in its series

    def data(self):
        """(t, y): n points of the row's series, from the first on unless the row says otherwise; the
        two sides of a pair share their series"""
        t, y = series(self.series_n, self.lattice, self.seed)
        t, y = t[self.first:self.first + self.n].copy(), y[self.first:self.first + self.n].copy()
        if self.scaled:
            y = y * np.sqrt(self.c)
        if self.per_item_y:
            rng = np.random.default_rng(self.seed + 77)
            return t, y[None, :] + 0.05 * rng.standard_normal((B, self.n))
        return t, y

    def y_of(self, i):
        y = self.data()[1]
        return y[i] if self.per_item_y else y

    def progs(self):
        if self.scaled:
            s = sample()
            return [scale_program(p, self.c) if i in s else p for i, p in enumerate(items())]
        return list(items())

    def spec(self):
        """None: the default spec"""
        return scaled_spec(self.c) if self.scaled else None

    def sample(self):
        return list(self.judged) if self.judged else sample()


ROWS = {}
PAIRS = []                         # (n = 16 k, one more point)
for _k in range(1, 16):
    for _n in (16 * _k, 16 * _k + 1):
        ROWS[f"n{_n}"] = SmallCase(_n, 16 * _k + 1, seed=100 + _k)
    PAIRS.append((f"n{16 * _k}", f"n{16 * _k + 1}"))
ROWS["n255"] = SmallCase(255, 256, seed=116)
ROWS["n256"] = SmallCase(256, 256, seed=116)
PAIRS.append(("n255", "n256"))
# the two smallest rows take their points from the MIDDLE of a 17-point series (t = 0.5; 0.375 ..
# 0.625): at t = 0 every ChangePoint location of the generator (0.3 .. 0.7, scale 0.05) is at least six
# scales away, 1 - sigmoid has lost its digits in fp64 and no seed is admissible
ROWS["n1"] = SmallCase(1, 17, seed=117, first=8)
ROWS["n5"] = SmallCase(5, 17, seed=117, first=6)
for _k in (0, 5, 9, 13):
    ROWS[f"n{16 * _k + 9}"] = SmallCase(16 * _k + 9, 16 * _k + 9, seed=120 + _k)
for _n in (97, 241):
    ROWS[f"n{_n}_irr"] = SmallCase(_n, _n, seed=100 + _n // 16, lattice=False)
ROWS["n208_rows"] = SmallCase(208, 208, seed=140, per_item_y=True)
for _c in SCALES:
    ROWS[f"n208_c{_c:g}"] = SmallCase(208, 208, seed=141, c=_c, scaled=True)
SCALE_ROWS = [f"n208_c{_c:g}" for _c in SCALES]

# the K^-1 kernel behind the column sweep (n > 256, up to 448 points and 512 items): the Linear and
# the ChangePoint item — general trees, which take the general leaf alone as in the batch (a
# stationary tree alone on a regular series goes to the Toeplitz leaf and never meets this kernel)
SWEEP = {}
SWEEP_PAIRS = []
for _n in (368, 400, 432):
    for _m in (_n, _n + 1):
        SWEEP[f"sweep_n{_m}"] = SmallCase(_m, _n + 1, seed=150 + _n // 16, judged=tuple(sample()[1:]))
    SWEEP_PAIRS.append((f"sweep_n{_n}", f"sweep_n{_n + 1}"))

ALL = {**ROWS, **SWEEP}

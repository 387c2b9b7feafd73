"""The geometry grid of the column sweep: block counts and 16-row edges, in one table.

The route tests (tests/value_cases.py, tests/test_routes_gpu.py) straddle the switches a BATCH SIZE
throws.  The rows here straddle what the SERIES throws (csrc/ngp_col_kernels.h, ngp_grad_kernels.h,
ngp_plan.h): how many 64-wide block columns it has — pairing from column 0 or 1, the first
diag-ahead tile that is joined, the four-wave tile, split-k — and where its last rows fall inside a
64 x 64 tile: a fat or thin step works on ONE 16-row group of a tile that holds at most 16 real
rows, the K^-1 kernel stops its k-loop at ceil16(n).  tests/test_geometry_gpu.py runs the rows on
the device against tests/hp_reference.py; tests/test_geometry_cases_cpu.py admits every judged
triple with the fp64 oracles at a quarter of the tolerance, checks the restated schedule below
against the compiled csrc/ngp_plan.h, and shows that wrong kernels of these kinds fail the judge.
Nothing here imports the GPU.

Value rows (ngp_nowcast_batch, 9 items: one past a multiple of 8; stationary, Linear and
ChangePoint items in one batch, so K' synthesised in the epilogue sits next to K' read from HBM);
naux = n % 64 + d + m + 1:
  blocks_nb{6..12}[_irr]  n = 64 nb0 + 33, naux = 39: one partial aux tile, three real 16-row groups
  aux16_nb{k} | aux17_nb{k}   n = 64 k + 10 | 11, naux = 16 | 17: the one aux tile at the nit = 1 edge
  aux80_nb{k} | aux81_nb{k}   n = 64 k + 63, m = 15 | 16, naux = 80 | 81: the SECOND aux tile at it
Gradient rows (a staged gradient job, 9 items, trees of 1, 3, 5 operators, every 4th a Linear chain):
  n = 64 k + r: the main block is padded to nb0 = k + 1 block columns with identity rows and the
  last row tile holds r real rows; r | r + 1 is the SAME series with one more point.
"""
import functools
from dataclasses import dataclass

from tests.value_cases import Case, ensemble, series, tree  # noqa: F401  (tree: re-exported)

NB, TB = 64, 16
B = 9
SIZES = (1, 3, 5)
# the value rows cycle through the same tree sizes from 3 on: the ChangePoint item of a 9-item batch
# is item 6 (cp_every = 7), and ``ensemble`` gives a ChangePoint only to a tree of at least 3
# operators — in the order (1, 3, 5) item 6 would be a single leaf and the batch would hold none
VALUE_SIZES = (3, 5, 1)
LINEAR_EVERY, CP_EVERY = 4, 7
# The items' seed is the first from 41 on with which every sampled (case, item, date set) is
# admissible for BOTH judgements of the GPU file (tests/test_geometry_cases_cpu.py): the fp64 oracle
# against long double at a quarter of the tolerance, and two fp64 evaluations in different
# summation orders (the LAPACK oracle, the blocked model) against each other at a quarter of
# tol(FLOOR_RT, cond).  41, 42 and 43 fail the second on the on_f dates: a low-noise item there has
# |mu| above a hundred sqrt(s_aa), and with seed 41 the two CPU evaluations already differ by 1.10
# of the whole bound — a device run against the item alone across a change of summation order
# (split-k, the diagonal kernel's form) could not be held to it.
ITEM_SEED = 44
BIG_B = 513                       # > SPLITK_MAX_ITEMS: split-k off by size


# ---- value rows ---------------------------------------------------------------------------------------
def _v(n, m=4, seed=1, lattice=True):
    return Case(n=n, B=B, d=1, D=2, m=m, lattice=lattice, seed=seed, item_seed=ITEM_SEED, sizes=VALUE_SIZES,
                linear_every=LINEAR_EVERY, cp_every=CP_EVERY, per_size=False)


VALUE = {}
for _nb in range(6, 13):
    VALUE[f"blocks_nb{_nb}"] = _v(64 * _nb + 33, seed=30 + _nb)
    if _nb in (6, 9, 11):
        VALUE[f"blocks_nb{_nb}_irr"] = _v(64 * _nb + 33, seed=30 + _nb, lattice=False)
AUX_PAIRS = []                    # (at most 16 real rows in the aux tile at the edge, one more)
for _k in (2, 3, 8, 9):
    VALUE[f"aux16_nb{_k}"] = _v(64 * _k + 10, seed=50 + _k)
    VALUE[f"aux17_nb{_k}"] = _v(64 * _k + 11, seed=50 + _k)
    AUX_PAIRS.append((f"aux16_nb{_k}", f"aux17_nb{_k}", 0))
for _k in (3, 8):
    VALUE[f"aux80_nb{_k}"] = _v(64 * _k + 63, m=15, seed=60 + _k)
    VALUE[f"aux81_nb{_k}"] = _v(64 * _k + 63, m=16, seed=60 + _k)
    AUX_PAIRS.append((f"aux80_nb{_k}", f"aux81_nb{_k}", 1))


def value_geometry(case):
    """(nb0, naux) of a value job (stage_general, csrc/ngp_api.hip)"""
    return case.n // NB, case.n % NB + case.d + case.m + 1


def kind(program):
    ops = [int(o) for o in program[0]]
    return "changepoint" if 8 in ops else "linear" if 2 in ops else "stationary"


def value_sample(case):
    """the first stationary, the first Linear and the first ChangePoint item"""
    kinds = [kind(p) for p in case.progs()]
    return [kinds.index(k) for k in ("stationary", "linear", "changepoint")]


@functools.lru_cache(maxsize=None)
def _filler():
    return tuple(ensemble(977, list(VALUE_SIZES), BIG_B - B, True, LINEAR_EVERY, CP_EVERY))


def value_big_batch(case):
    """the case's 9 items as the prefix of a 513-item batch (the other 504 are only company)"""
    return case.progs() + list(_filler())


# ---- gradient rows ------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GradCase:
    k: int                 # full 64-blocks
    r: int                 # real rows of the last row tile
    seed: int

    @property
    def n(self):
        return NB * self.k + self.r

    @property
    def nb0(self):
        return (self.n + NB - 1) // NB

    def data(self):
        """the first n points of the pair's series of 64 k + (r | 1) points: the two sides of a
        pair r | r + 1 differ by the last point alone"""
        t, y = series(NB * self.k + (self.r | 1), True, self.seed)
        return t[:self.n].copy(), y[:self.n].copy()

    def progs(self):
        return list(_grad_items())

    def sample(self):
        """one stationary item, one Linear chain"""
        kinds = [kind(p) for p in self.progs()]
        return [kinds.index("stationary"), kinds.index("linear")]

    def stationary(self):
        return [i for i, p in enumerate(self.progs()) if kind(p) == "stationary"]


@functools.lru_cache(maxsize=None)
def _grad_items():
    return tuple(ensemble(43, list(SIZES), B, linear_every=LINEAR_EVERY))


GRAD = {}
GRAD_PAIRS = []
for _k in (4, 5, 8, 9):
    for _r in (16, 17):
        GRAD[f"grad_n{64 * _k + _r}"] = GradCase(_k, _r, seed=70 + _k)
    GRAD_PAIRS.append((f"grad_n{64 * _k + 16}", f"grad_n{64 * _k + 17}"))
for _k in (4, 8):
    for _r in (32, 33, 48, 49):
        GRAD[f"grad_n{64 * _k + _r}"] = GradCase(_k, _r, seed=70 + _k)
    GRAD_PAIRS += [(f"grad_n{64 * _k + _r}", f"grad_n{64 * _k + _r + 1}") for _r in (32, 48)]


# ---- the kernels' row shortcuts, restated --------------------------------------------------------------
def aux_tile_groups(naux, tile):
    """16-row groups a fat or thin step works on in aux tile ``tile`` of a value job: one when the
    tile holds at most 16 real rows, else all four (csrc/ngp_col_kernels.h, nit)"""
    return 1 if naux - NB * tile <= TB else 4


def last_row_tile_groups(n):
    """the same for the padded last row tile of a gradient job of n points"""
    n0 = (n + NB - 1) // NB * NB
    return 1 if n - (n0 - NB) <= TB else 4


def kinv_kend(n):
    """where grad_kinv_lds_kernel's k-loop stops (csrc/ngp_grad_kernels.h): the 16-chunk that
    holds the last real column"""
    n0 = (n + NB - 1) // NB * NB
    return min(n0, (n + TB - 1) // TB * TB)


# ---- the block-column schedule, restated (csrc/ngp_plan.h) ---------------------------------------------
COL_FULL, COL_FAT, COL_THIN = 0, 1, 2
DIAG_AHEAD_SPLIT_K = 512
SPLITK_MIN_NB = KINV_LDS_MIN_NB = 8
SMALL_ITEMS = 512                 # SPLITK_MAX_ITEMS, DIAG_WAVE_MAX_ITEMS, KINV_SMALL_MAX_ITEMS
SM_MAX_NB = 4
KINV_SMALL, KINV_WAVE, KINV_LDS = 0, 1, 2


def col_pair_offset(nb0):
    return 1 if nb0 >= 3 and nb0 % 2 else 0


def col_step(nb0, jj):
    """(mode, k0_col, k0_diag, ahead, join) of block column jj"""
    o = col_pair_offset(nb0)
    fat = jj >= o and (jj - o) % 2 == 0 and jj + 1 < nb0
    thin = jj >= o and (jj - o) % 2 == 1
    mode = COL_FAT if fat else COL_THIN if thin else COL_FULL
    k0_col = (jj - 1) * NB if thin else 0
    k0_diag = (jj - 1) * NB if thin else (jj - 2) * NB if jj - o >= 2 else 0
    ahead = fat and jj + 2 < nb0 and jj > 0
    join = (jj - o) % 2 == 0 and jj - 2 >= max(o, 1)
    return mode, k0_col, k0_diag, ahead, join


def diag_ahead_waves(jj):
    """waves of the diag-ahead tile the fat step jj launches (the tile (jj + 2, jj + 2))"""
    return 4 if jj * NB >= DIAG_AHEAD_SPLIT_K else 1


def splitk_eligible(nb0, bc, invariant):
    """a value chunk that is neither mixed precision nor half of a two-lane sweep"""
    return bc <= SMALL_ITEMS and nb0 >= SPLITK_MIN_NB and not invariant


def diag_wave(bc, invariant):
    return not invariant and bc <= SMALL_ITEMS


def kinv_route(nb0, bc, invariant):
    """of a gradient chunk with the short path on (small_job: up to SM_MAX_NB block columns and
    SM_MAX_ITEMS items, or any batch under ngp_set_batch_invariant)"""
    small_job = nb0 <= SM_MAX_NB and (bc <= 4096 or invariant)
    lds = nb0 >= KINV_LDS_MIN_NB
    if small_job or (not lds and bc <= SMALL_ITEMS and not invariant):
        return KINV_SMALL
    return KINV_LDS if lds else KINV_WAVE

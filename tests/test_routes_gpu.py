"""Route switch points of the gradient schedule, tested from both sides.

The same item is factorised and differentiated by different kernels, in different summation
orders, depending on the batch size, the series length, the tree size and the dates (DESIGN.md,
include/ngp.h).  For every switch the SAME items run just below and just above the threshold, and
on both sides
  1. sampled items agree with the extended-precision reference (tests/hp_reference.py)
     componentwise: every gradient component against its own scale s_i;
  2. sampled items agree with the same item evaluated in a call of its own;
  3. the two sides agree with each other to rounding,
and, with ngp_set_batch_invariant on, the two sides give the same bits.

Tree sizes: a tree of L leaves has 2L - 1 operators, so the bucket edges (1, 3, 7, 15, 31 operators,
grad_bucket in ngp_plan.h) are straddled with 1|3, 3|5, 7|9, 15|17, 31|33 and 63 operators.
"""
import contextlib

import numpy as np
import pytest

from nowcastautogp_amd import _lib
from nowcastautogp_amd._abi import KernelArray
from tests import hp_reference as hr
from tests.util import TOL_LOGML, check, check_components, tol
from tests.value_cases import ensemble, series, tree

pytestmark = pytest.mark.gpu

# componentwise floors (relative to each component's scale s_i; condition-aware above them)
FLOOR_REF = 1e-10       # against the extended-precision reference
FLOOR_RT = 1e-11        # against the item alone / the other side of a threshold (rounding)


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    c = _lib.Context(0)
    c.set_combining(False)
    yield c
    c.close()


# ---- items: tests/value_cases.py holds the generators (shared with the value-path tests) -----------
# ---- the three comparisons ------------------------------------------------------------------------
def _run(ctx, progs, t, y, profile=False):
    """one staged gradient job over the items (its run gives the one-shot call's bits,
    include/ngp.h): (logml, gradients, kernel-class profile of the run, ngp_grad_job_info)"""
    ka = KernelArray(progs)
    job = ctx.stage_grad(ka, t, y)
    try:
        if profile:
            ctx.profile_enable(True)
            ctx.profile_reset()
        lm, g, info = job.run()
        prof = ctx.profile_get() if profile else None
        if profile:
            ctx.profile_enable(False)
        layout = job.info()
    finally:
        job.close()
    assert not info.any(), np.nonzero(info)
    off = np.concatenate([[0], np.cumsum(ka._npar + 1)])
    return lm, [g[off[b]:off[b + 1]] for b in range(len(progs))], prof, layout


@contextlib.contextmanager
def general_leaf_only(ctx):
    """structured storage off: no item takes the Toeplitz leaf, so the whole batch is ONE general
    chunk and the per-chunk switches see the batch size itself"""
    ctx.set_structured_storage(False)
    try:
        yield
    finally:
        ctx.set_structured_storage(True)


def one_general_chunk(B, layout):
    assert layout["general_items"] == B and layout["general_chunk"] == B, (B, layout)
    assert layout["toeplitz_items"] == 0, (B, layout)


def _sample(progs, B, extra=()):
    """first, last, one item of every op count, the given extra items"""
    seen, idx = set(), {0, B - 1, *extra}
    for i in range(B):
        k = len(progs[i][0])
        if k not in seen:
            seen.add(k)
            idx.add(i)
    return sorted(i for i in idx if i < B)


def judge(ctx, row, progs, t, y, sides, extra=(), profile_check=None, layout_check=None):
    """the items progs[:B] for every B in sides: reference, alone, other side; profile_check /
    layout_check(B, ...) assert the route each side took"""
    res = {}
    for B in sides:
        lm, g, prof, layout = _run(ctx, progs[:B], t, y, profile=profile_check is not None)
        res[B] = (lm, g)
        if profile_check is not None:
            profile_check(B, prof)
        if layout_check is not None:
            layout_check(B, layout)
    Bmin = min(sides)
    for i in _sample(progs, Bmin, extra):
        r = hr.evaluate(progs[i], t, y)
        assert r.info == 0
        lm_a, g_a, _, _ = _run(ctx, [progs[i]], t, y)
        for B in sides:
            lm, g = res[B]
            c = (row, B, i, len(progs[i][0]))
            check(f"routes {row}: logml vs reference", lm[i], float(r.logml), TOL_LOGML, r.cond, ctx=c)
            check_components(f"routes {row}: gradient vs reference", g[i], r.grad, r.scale, FLOOR_REF,
                             r.cond, ctx=c, factor=r.tol_factor)
            assert abs(lm[i] - lm_a[0]) <= tol(1e-12, r.cond) * abs(lm_a[0]), c
            check_components(f"routes {row}: gradient vs item alone", g[i], g_a[0], r.scale, FLOOR_RT,
                             r.cond, ctx=c)
        for B in sides[1:]:
            check_components(f"routes {row}: gradient, one side vs the other", res[B][1][i],
                             res[sides[0]][1][i], r.scale, FLOOR_RT, r.cond, ctx=(row, B, i))
            assert abs(res[B][0][i] - res[sides[0]][0][i]) <= tol(1e-12, r.cond) * abs(lm_a[0])
    return res


def invariant_bits(ctx, progs, t, y, sides, extra=()):
    """batch-invariant mode: every item below the smaller side gets the same bits on both sides,
    and the sampled items the same bits as in a call of their own"""
    Bmin = min(sides)
    ctx.set_batch_invariant(True)
    try:
        out = [_run(ctx, progs[:B], t, y) for B in sides]
        alone = {i: _run(ctx, [progs[i]], t, y) for i in _sample(progs, Bmin, extra)}
    finally:
        ctx.set_batch_invariant(False)
    for lm, g, _, _ in out[1:]:
        assert np.array_equal(lm[:Bmin], out[0][0][:Bmin])
        for i in range(Bmin):
            assert np.array_equal(g[i], out[0][1][i]), i
    for i, (lm_a, g_a, _, _) in alone.items():
        assert lm_a[0] == out[0][0][i] and np.array_equal(g_a[0], out[0][1][i]), i


# ---- the rows -------------------------------------------------------------------------------------
SMALL_SIZES = [1, 3, 5, 7, 9]


@pytest.mark.parametrize("lattice", [True, False], ids=["lattice", "irregular"])
def test_one_launch_path_4096_vs_4097_items(ctx, lattice):
    """chol_small_kernel up to SM_MAX_ITEMS (4,096) items of a series of at most 256 points, the
    column sweep above; stationary and general trees mixed.  On lattice dates the batch above the
    threshold is split: its stationary trees go to the Toeplitz leaf (column sweep, class 0), and
    its other items, 820 of them, stay on the one-launch general leaf."""
    t, y = series(200, lattice, seed=1)
    progs = ensemble(11, SMALL_SIZES, 4097, linear_every=5)

    def prof(B, p):
        if B <= 4096:
            assert p.get("chol_small", {}).get("launches", 0) > 0, p
        elif lattice:
            assert p["chol_col"]["launches"] > 0 and p["chol_small"]["launches"] > 0, p
        else:
            assert "chol_small" not in p, p
    judge(ctx, "one-launch 4096|4097", progs, t, y, [4096, 4097], extra=(1, 4094), profile_check=prof)
    invariant_bits(ctx, progs, t, y, [4096, 4097])


@pytest.mark.parametrize("n", [127, 128])
def test_toeplitz_leaf_from_128_points_at_4097_items(ctx, n):
    """stationary trees on a regular series: the Toeplitz gradient leaf from 128 points on (above
    the one-launch path's batch size); the same item alone takes the one-launch general leaf"""
    t, y = series(n, True, seed=2)
    progs = ensemble(12, [1, 3, 5, 7], 4097)

    def prof(B, p):
        if n >= 128:
            assert "chol_col_grad" not in p and p["chol_col"]["launches"] > 0, p
        else:
            assert p["chol_col_grad"]["launches"] > 0, p

    def layout(B, lay):
        assert lay["toeplitz_items"] == (B if n >= 128 else 0), lay
    judge(ctx, f"toeplitz n={n} @4097", progs, t, y, [4097], extra=(2048,), profile_check=prof,
          layout_check=layout)
    invariant_bits(ctx, progs, t, y, [4097], extra=(2048,))


def test_toeplitz_leaf_16_vs_17_leaves_and_a_linear_leaf(ctx):
    """a mixed batch split into its two leaves: stationary trees of 16 leaves (31 operators) take the
    Toeplitz leaf (class chol_col), 17 leaves (33) and a Linear leaf the general one (class
    chol_col_grad); both halves sampled, and compared with the batch run on the general leaf alone.
    Trees of 3 and 15 operators fill the Toeplitz leaf's other buckets."""
    t, y = series(300, True, seed=3)
    progs = ensemble(13, [31, 33, 3, 15], 300, linear_every=7)
    toep = [i for i, p in enumerate(progs) if len(p[0]) <= 31 and not np.isin(p[0], (2, 8)).any()]
    assert any(len(progs[i][0]) == 31 for i in toep)

    def layout(B, lay):
        assert lay["toeplitz_items"] == len(toep) and lay["general_items"] == B - len(toep), lay

    def prof(B, p):
        assert p["chol_col"]["launches"] > 0 and p["chol_col_grad"]["launches"] > 0, p
    sample = (0, 1, 2, 6, 13)
    judge(ctx, "toeplitz leaves 16|17", progs, t, y, [300], extra=sample, profile_check=prof,
          layout_check=layout)
    with general_leaf_only(ctx):
        _, g_g, p_g, lay_g = _run(ctx, progs, t, y, profile=True)
    one_general_chunk(300, lay_g)
    assert "chol_col" not in p_g and p_g["chol_col_grad"]["launches"] > 0, p_g
    _, g, _, _ = _run(ctx, progs, t, y)
    for i in sample + (299,):
        r = hr.evaluate(progs[i], t, y)
        check_components("routes toeplitz leaves 16|17: Toeplitz vs general leaf", g[i], g_g[i], r.scale,
                         FLOOR_RT, r.cond, ctx=i)
    invariant_bits(ctx, progs, t, y, [300], extra=sample)


# the rows at n = 448 share their items (a prefix of one ensemble on one series): the reference of
# an item is computed once for all of them.  Those rows run on the general leaf alone: on lattice
# dates a batch of 256 items or more would give its stationary trees to the Toeplitz leaf, and the
# per-chunk switches would see the two leaves' sizes instead of the batch size.
def items448(B):
    return ensemble(14, SMALL_SIZES, 2341, linear_every=5)[:B]


@pytest.mark.parametrize("n", [448, 449])
def test_kinv_split_k_and_diag_512_vs_513_items(ctx, n):
    """K^-1: grad_kinv_small (nb0 = 7, <= 512 items) / grad_kinv_kernel (nb0 = 7, 513 items: alpha
    on the side stream) / grad_kinv_lds_kernel (nb0 = 8); split-k fat steps, chol_diag_wave_kernel
    and early diag-ahead up to 512 items in the chunk"""
    t, y = series(n, True, seed=4)
    progs = items448(513)
    with general_leaf_only(ctx):
        judge(ctx, f"kinv/split-k n={n} 512|513", progs, t, y, [512, 513], extra=(256,),
              layout_check=one_general_chunk)
        invariant_bits(ctx, progs, t, y, [512, 513], extra=(256,))


def test_two_lanes_63_vs_64_items(ctx):
    """two lanes for 64..512 items of a series of at least 24 block columns: n = 1472 (nb0 = 23)
    and 1473 (nb0 = 24), 63 and 64 items"""
    for n in (1472, 1473):
        t, y = series(n, True, seed=5)
        progs = ensemble(15, [1, 3, 5], 64, linear_every=4)
        judge(ctx, f"two lanes n={n} 63|64", progs, t, y, [63, 64], extra=(31, 32),
              layout_check=one_general_chunk)
        invariant_bits(ctx, progs, t, y, [63, 64], extra=(31, 32))


# n = 448: nb0 = 7, ntri = 28 — ntri * Bc straddles 1024 (36 | 37), 2048 (73 | 74), 65536 (2340 | 2341)
@pytest.mark.parametrize("sides", [(36, 37), (73, 74)], ids=["1024", "2048"])
def test_contraction_split(ctx, sides):
    t, y = series(448, True, seed=4)
    progs = items448(max(sides))
    with general_leaf_only(ctx):
        judge(ctx, f"contraction split {sides[0]}|{sides[1]}", progs, t, y, list(sides),
              layout_check=one_general_chunk)
        invariant_bits(ctx, progs, t, y, list(sides))


@pytest.mark.parametrize("big", [False, True], ids=["no-big-tree", "with-63-op-tree"])
def test_contraction_four_tiles_per_workgroup(ctx, big):
    """four tiles per workgroup from ntri * Bc >= 65536 in one chunk (28 x 2340 = 65,520 against
    28 x 2341 = 65,548), only when no tree of the chunk has more than 31 operators"""
    t, y = series(448, True, seed=4)
    progs = items448(2341)
    if big:
        progs[1] = tree(np.random.default_rng(99), 63)
    with general_leaf_only(ctx):
        judge(ctx, f"four tiles {'with' if big else 'without'} >31 ops 2340|2341", progs, t, y,
              [2340, 2341], layout_check=one_general_chunk)
        invariant_bits(ctx, progs, t, y, [2340, 2341])


@pytest.mark.parametrize("B", [160, 600])
@pytest.mark.parametrize("lattice", [True, False], ids=["lattice", "irregular"])
def test_tree_size_buckets(ctx, lattice, B):
    """trees of 1, 3, 5, 7, 9, 15, 17, 31, 33 and 63 operators in ONE general chunk: every bucket of
    the contraction, its edges, and the main / side stream alternation (<= 512 items)"""
    t, y = series(448, lattice, seed=8)
    progs = ensemble(18, [1, 3, 5, 7, 9, 15, 17, 31, 33, 63], B, linear_every=7, cp_every=11)
    with general_leaf_only(ctx):
        judge(ctx, f"buckets {'lattice' if lattice else 'irregular'} B={B}", progs, t, y, [B],
              layout_check=one_general_chunk)
        invariant_bits(ctx, progs, t, y, [B])

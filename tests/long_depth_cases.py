"""The long-horizon queries on DEEP factors: the cases and the judgement shared by
tests/test_long_depth_cpu.py (which holds the fp64 oracle to the same judgement at a quarter of the
tolerance) and tests/test_long_depth_gpu.py (which judges the device) — TEST INFRASTRUCTURE ONLY.

Programs, ``series``, ``query`` and the spacing H = 1/200 are those of tests/sample_long_cases.py.
From n = 1000 on particle 1 (Linear + SqExp, noise 4e-3: cond 1.8e6 at n = 1100, 50 eps cond = 2e-8)
is the same tree with noise 4e-2 (cond 1.8e5), so that every long-double-judged case stays within
the floor (50 eps cond <= 1e-8); at n = 2110 the reference is fp64 LAPACK (tol_factor 2) and that
particle (cond 1.4e6) is judged condition-aware, reported through tests.util.RECORDS.

Depth.  n0 = 64 (n // 64) is the main block, nb0 = n0 / 64 its block columns, n - n0 the tail:

    n      n0    nb0  tail
    192    192    3    0     the first block column the solve has never reached
    257    256    4    1
    577    576    9    1
    1090   1088   17   2     n0 > LORG_TERMS = 1024; n + d <= hp_reference.HP_MAX_N for d <= 10
    2110   2048   32   62    headline depth

The judgement is componentwise (tests.util.check_components): mu on sqrt(s_aa), var and sigma on
sqrt(s_aa s_bb) with s the REFERENCE's predictive variances, logml relative; floors TOL_PRED and
TOL_LOGML, cond and tol_factor the reference's.  At m = 4096 the m x m long double array is out of
reach: mu and var are judged in full, sigma on ROWS (tests/long_reference.py nowcast_rows).

Parts of a decomposition carry no observation noise, so a part's own posterior variance is no
floor-bounded yardstick; they are judged on the scale of the part OBSERVED WITH the particle's noise,
s_(c,a) = sigma_(ca,ca) + noise + jitter — with one part this is the s_aa of the particle's forecast.

Agreement with ngp_factor_nowcast (where the horizon also fits beside the factor) is judged as
value_cases.judge_against_run does: FLOOR_RT, condition-aware, on the same scales.  That tolerance,
50 eps cond of sqrt(s_aa), is fair only to a particle whose mean is as well determined as cond says.
Particle 2 (the ChangePoint tree, noise 5e-3) is not: the series has a trend its Periodic branch cannot
follow, alpha is large, and every fp64 evaluation of its mean is 0.15 .. 2.2 of that tolerance from
long double (the fp64 oracle 2.2 at n = 2110, where the long double mean was computed once by hand:
oracle 3.7e-9, predict_long 2.2e-9, ngp_factor_nowcast 1.9e-9 of sqrt(s_aa)).  By the rule of
tests/test_date_cases_cpu.py a case the oracle cannot pass at a quarter is replaced, not loosened: the
agreement test runs, in particle 2's place, value_cases.FILL_OTHER[0] (Linear * SqExp + Linear * Periodic,
noise 5e-3: a general tree filled through the stack, which follows the trend; the oracle is then at
most 0.04 of a quarter — raising particle 2's noise tenfold only brought it to 2.3 of a quarter); the
judgement against the reference above keeps the original particle.

R64_*: the worst error / tolerance of the fp64 oracle under this judgement, per family, measured by
tests/test_long_depth_cpu.py (which requires every single one to stay below 1/4).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from tests import component_nowcast_reference as cnr
from tests import hp_reference as hr
from tests import long_reference as lr
from tests import sample_long_cases as lc
from tests import value_cases as vc
from tests.util import TOL_LOGML, TOL_PRED, check_components, tol

H, P = lc.H, lc.P
series, query = lc.series, lc.query
DEEP_FROM = 1000
DEEP_LINEAR = (np.array(vc.FILL_CHAIN[0][0], np.int32), np.array(vc.FILL_CHAIN[0][1], float), 4e-2)
ROWS = (0, 63, 64, 2047, 2048, 4032, 4095)

# worst error / tolerance of the fp64 oracle (tests/test_long_depth_cpu.py prints and pins them)
R64_PREDICT = 0.1663        # mu, n = 2110, d = 0, m = 300, particle 2 (cond 1.0e5)
R64_ORIGINS = 0.1304
R64_COMPONENTS = 0.02335
R64_AGREE = 0.01852          # of the agreement tolerance (FLOOR_RT, condition-aware), ``agree_programs``


def programs(n):
    return list(lc.PROGRAMS) if n < DEEP_FROM else [lc.PROGRAMS[0], DEEP_LINEAR, lc.PROGRAMS[2]]


AGREE_THIRD = (np.array(vc.FILL_OTHER[0][0], np.int32), np.array(vc.FILL_OTHER[0][1], float), vc.FILL_OTHER[0][2])


def agree_programs(n):
    """``programs(n)`` with AGREE_THIRD in particle 2's place (module docstring)"""
    return programs(n)[:2] + [AGREE_THIRD]


def irregular_series(n):
    """n sorted uniform dates over the span of ``series(n)``, no two within 1e-4 of the span"""
    rng = np.random.default_rng(300 + n)
    u = np.sort(rng.uniform(0.0, 1.0, n)) + np.arange(n) * 1e-4
    t = (u - u[0]) / (u[-1] - u[0]) * ((n - 1) * H)
    return t, np.sin(9.0 * t) + 0.3 * t + 0.1 * rng.standard_normal(n)


def per_item_rows(y):
    return np.stack([y, 0.5 * y + 0.1, -y])


# ---- predict_long ----------------------------------------------------------------------------------
@dataclass(frozen=True)
class Long:
    n: int
    d: int
    D: int
    m: int
    sigma: bool = True
    data: str = "lattice"        # "irregular": sorted uniform dates; "per_item": one y row per particle

    @property
    def id(self):
        return f"n{self.n}-d{self.d}-m{self.m}-{'sigma' if self.sigma else 'lean'}-{self.data}"

    def inputs(self):
        """t [n], y [n] or [P, n], t_add [d], y_add [D, d], t_new [m]"""
        t, y, t_add, y_add, t_new = query(self.n, self.d, self.D, self.m)
        if self.data == "irregular":
            y_last = y[-1]
            t, y = irregular_series(self.n)
            t_add = t[-1] + H * np.arange(1, self.d + 1)
            t_new = t[-1] + H * (self.d + np.arange(1, self.m + 1))
            y_add = y_add - y_last + y[-1] if self.d else y_add
        elif self.data == "per_item":
            y = per_item_rows(y)
        return t, y, t_add, y_add, t_new

    def fits_nowcast(self):
        return self.m <= 192 - self.n % 64 - self.d - 1


DEPTH = [
    Long(192, 0, 1, 65), Long(192, 3, 2, 300), Long(257, 0, 1, 300), Long(257, 3, 2, 1),
    Long(577, 0, 1, 1), Long(577, 3, 2, 65), Long(1090, 0, 1, 65), Long(1090, 3, 2, 300),
    Long(2110, 0, 1, 300), Long(2110, 3, 2, 65),
    Long(257, 3, 2, 1000),
    Long(1090, 0, 1, 1000, sigma=False),      # the fill wraps: 1088 x 1024 > 2^20
    Long(257, 3, 2, 4096, sigma=False),
    Long(64, 0, 1, 4096),                     # the small and the sigma kernel wrap: m^2 = 2^24
]
# the conditioning block: c = tail + d = 88 | 89 either side of LONG_COND_LDS; c = 163: three tile
# columns of S (ct = c / 64 + 1 = 3), with and without sigma; a deep factor beside a large block
COND_BLOCK = [
    Long(191, 25, 2, 65), Long(191, 26, 2, 65), Long(191, 100, 2, 65), Long(191, 100, 2, 65, sigma=False),
    Long(257, 100, 2, 65),
]
INPUT_PATHS = [Long(577, 3, 2, 65, data="irregular"), Long(577, 3, 2, 65, data="per_item")]
LONGS = DEPTH + COND_BLOCK + INPUT_PATHS
BITS_LONG = Long(1090, 3, 2, 300)


def _row(y, p):
    return y if y.ndim == 1 else y[p]


def long_reference(case, p):
    """the long double reference of particle p: hr.nowcast, at m = 4096 lr.nowcast_rows on ROWS"""
    t, y, t_add, y_add, t_new = case.inputs()
    prog = programs(case.n)[p]
    if case.m == 4096:
        return lr.nowcast_rows(prog, t, _row(y, p), t_add, y_add, t_new, ROWS)
    return hr.nowcast(prog, t, _row(y, p), t_add, y_add, t_new)


AGREE = [c for c in LONGS if c.fits_nowcast()]


def agree_reference(case, p):
    t, y, t_add, y_add, t_new = case.inputs()
    return hr.nowcast(agree_programs(case.n)[p], t, _row(y, p), t_add, y_add, t_new)


def judge_agreement(what, mu, var, sigma, other_mu, other_sigma, r, ctx=None, frac=1.0, record=True):
    """one evaluation of a particle against another, as value_cases.judge_against_run: FLOOR_RT,
    condition-aware, on the scales of the reference ``r``; returns the worst error / tolerance"""
    d, dd = hr.pred_scales(r.sigma)
    k = _Cond(r.cond)
    other_sigma = np.asarray(other_sigma, float)
    w = [_judge(f"{what}: mu", mu, other_mu, d[None, :], vc.FLOOR_RT, k, ctx, frac, record),
         _judge(f"{what}: var", var, np.diag(other_sigma), d * d, vc.FLOOR_RT, k, ctx, frac, record)]
    if sigma is not None:
        w.append(_judge(f"{what}: sigma", sigma, other_sigma, dd, vc.FLOOR_RT, k, ctx, frac, record))
    return max(w)


def _judge(what, got, ref, scale, floor, r, ctx, frac, record):
    """check_components, returning error / tolerance (printed before the assertion)"""
    f = r.tol_factor * frac
    got, ref, scale = (np.asarray(a, float) for a in (got, ref, scale))
    assert got.shape == ref.shape, (what, ctx, got.shape, ref.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(got == ref, 0.0, np.abs(got - ref) / scale)
    ratio = float(np.max(e)) / (tol(floor, r.cond) * f)
    if record:
        print(f"{what} {ctx}: error / tolerance = {ratio:.3f} (cond {r.cond:.2e})")
    check_components(what, got, ref, scale, floor, r.cond, ctx=ctx, factor=f, record=record)
    return ratio


def judge_long(what, mu, var, sigma, r, ctx=None, frac=1.0, record=True):
    """mu [D, m], var [m], sigma [m, m] or None of ONE particle against its reference ``r``
    (hr.NowcastRef or lr.RowsRef); returns the worst error / tolerance"""
    assert r.info == 0, ctx
    rows = getattr(r, "rows", None)
    var_ref = np.asarray(r.var if rows is not None else np.diag(r.sigma), float)
    d = np.sqrt(np.abs(var_ref))
    w = [_judge(f"{what}: mu", mu, r.mu, d[None, :], TOL_PRED, r, ctx, frac, record),
         _judge(f"{what}: var", var, var_ref, d * d, TOL_PRED, r, ctx, frac, record)]
    if sigma is not None and rows is None:
        w.append(_judge(f"{what}: sigma", sigma, r.sigma, np.outer(d, d), TOL_PRED, r, ctx, frac, record))
    elif sigma is not None:
        w.append(_judge(f"{what}: sigma rows", np.asarray(sigma)[rows], r.sigma_rows,
                        d[rows][:, None] * d[None, :], TOL_PRED, r, ctx, frac, record))
    return max(w)


# ---- predict_origins --------------------------------------------------------------------------------
def n0_of(n):
    return n // 64 * 64


def cuts_of(n, kind="edges"):
    """edges: 1, 63, 64, 65, 128, 129; five consecutive cuts inside tile 5 nb0 / 8 of the main block
    (from n = 577 on at least two cut-free tiles lie before it and two behind it, before the cuts at
    the end of the main block; the four tiles of n = 257 leave no room for that); 1023, 1024, 1025
    where they exist; n0 - 1, n0, n0 + 1 and n.
    half: the edges and a run of five, all <= n0 / 2 — the walk ends before the last tile.
    all1024: every cut 1 .. 1024."""
    n0 = n0_of(n)
    if kind == "all1024":
        return list(range(1, 1025))
    nb0 = n0 // 64
    mid = 64 * (5 * nb0 // 8) + 30
    if kind == "half":
        mid = 64 * (5 * nb0 // 16) + 30
        return sorted({1, 63, 64, 65, 128, 129, *range(mid, mid + 5), n0 // 2})
    cuts = {1, 63, 64, 65, 128, 129, *range(mid, mid + 5), n0 - 1, n0, n0 + 1, n}
    if n > 1025:
        cuts |= {1023, 1024, 1025}
    return sorted(c for c in cuts if 1 <= c <= n)


def origin_dates(n, m, t=None):
    """from eight observations before the end of the series on (tests/test_predict_origins_gpu.py)"""
    t = series(n)[0] if t is None else t
    return t[-1] + H * (np.arange(m) - 8)


@dataclass(frozen=True)
class Origins:
    n: int
    kind: str
    m: int
    data: str = "lattice"

    @property
    def id(self):
        return f"n{self.n}-{self.kind}-m{self.m}-{self.data}"

    def inputs(self):
        """t [n], y [n] or [P, n], cuts [R], t_new [m]"""
        t, y = irregular_series(self.n) if self.data == "irregular" else series(self.n)
        if self.data == "per_item":
            y = per_item_rows(y)
        return t, y, cuts_of(self.n, self.kind), origin_dates(self.n, self.m, t)


ORIGINS = [
    Origins(257, "edges", 65), Origins(577, "edges", 300), Origins(577, "half", 17),
    Origins(1090, "edges", 65), Origins(1090, "all1024", 17), Origins(2110, "edges", 17),
    Origins(577, "edges", 17, data="irregular"), Origins(577, "edges", 17, data="per_item"),
]
BITS_ORIGINS = Origins(1090, "edges", 65)


def origins_reference(case, p):
    t, y, cuts, t_new = case.inputs()
    return lr.origins(programs(case.n)[p], t, _row(y, p), cuts, t_new)


def judge_origins(what, mu, var, lm, r, ctx=None, frac=1.0, record=True):
    """mu [R, m], var [R, m], logml [R] of ONE particle against lr.origins"""
    assert r.info == 0, ctx
    s = np.abs(np.asarray(r.var, float))
    lm_ref = np.asarray(r.logml, float)
    return max(_judge(f"{what}: mu", mu, r.mu, np.sqrt(s), TOL_PRED, r, ctx, frac, record),
               _judge(f"{what}: var", var, r.var, s, TOL_PRED, r, ctx, frac, record),
               _judge(f"{what}: logml", lm, lm_ref, np.abs(lm_ref), TOL_LOGML, r, ctx, frac, record))


# ---- components_long ---------------------------------------------------------------------------------
COMPONENTS = [(577, 3, 2, 65), (1090, 3, 2, 65)]


def cut(prog, parts):
    """``prog`` as 1, 2 or 3 programs that sum to it (tests/test_components_long_gpu.py)"""
    from tests.test_components_long_gpu import cut as cut_
    return cut_(prog, parts)


@functools.lru_cache(maxsize=None)
def comps_of(n):
    """COMPS[n % 3] of tests/test_components_long_gpu.py, on this n's programs: 1 + (p + n) % 3 parts"""
    return [cut(prog, 1 + (p + n) % 3) for p, prog in enumerate(programs(n))]


def components_reference(case, p):
    n, d, D, m = case
    t, y, t_add, y_add, t_new = query(n, d, D, m)
    return cnr.evaluate(programs(n)[p], comps_of(n)[p], t, y, t_add, y_add, t_new)


class _Cond:
    def __init__(self, cond):
        self.cond, self.tol_factor = cond, 1.0


def judge_components(what, mu, cross, sigma, r, prog, ctx=None, frac=1.0, record=True):
    """mu [C, D, m], cross [C, C, m], sigma [C m, C m] of ONE particle against cnr.evaluate"""
    assert r.info == 0, ctx
    C, D, m = np.asarray(r.mu).shape
    ref = np.asarray(r.sigma, float)
    d = np.sqrt(np.abs(np.diag(ref)) + prog[2] + 1e-5)              # [C m]
    k = _Cond(r.cond)
    same = np.einsum("ajbj->abj", ref.reshape(C, m, C, m))
    dd = np.einsum("ajbj->abj", np.outer(d, d).reshape(C, m, C, m))
    return max(_judge(f"{what}: mu", mu, r.mu, d.reshape(C, 1, m), TOL_PRED, k, ctx, frac, record),
               _judge(f"{what}: cross", cross, same, dd, TOL_PRED, k, ctx, frac, record),
               _judge(f"{what}: sigma", sigma, ref, np.outer(d, d), TOL_PRED, k, ctx, frac, record))

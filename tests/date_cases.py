"""Date layouts: ONE weekly series and ONE ensemble of small trees, written down in the date
conventions a caller may pass — in the style of tests/value_cases.py.

tests/test_date_layouts_gpu.py runs the layouts through the HIP kernels; tests/test_date_cases_cpu.py
runs the same sampled (layout, item, forecast-date set) triples through the plain fp64 oracle at a
quarter of the tolerance, and checks with the extended-precision reference that every affine layout
describes the same GP.

The underlying problem lives on the index grid k = 0 .. N - 1, N = 2 (n + d) + 1, and trains on every
second index as ``value_cases.Case.data`` does (an unobserved week in every gap; the main block keeps
a constant stride of two lattice steps).  A layout maps the index to a date, t = a u + b with
u = k / (N - 1) the ``unit`` date, and the tree parameters go with it (positions:
tests/hp_reference.py ``_leaf``):

    SE, GammaExponential lengthscale      x a       (a > 0 in every layout)
    Periodic period                       x a       (its lengthscale divides sin^2: dimensionless)
    Linear location, ChangePoint location a x + b
    ChangePoint width                     x a
    Linear amplitude                      / a^2     (it multiplies (t - c)(t' - c): a slope squared)

so logml, predictive means and covariances are those of ``unit`` and a gradient component is the
``unit`` one divided by d theta' / d theta (``Problem.pscale``).

Layouts (``LAYOUTS``):
  unit            k / (N - 1), the control
  days_over_last  7 k / (7 (N - 1)): day counts over the last one (the same bits as ``unit``: a
                  correctly rounded quotient of the same rational)
  raw_days        19000 + 7 k (exact)
  decimal_years   2020 + k / 52
  shift100, shift1e4   100 + k / (N - 1), 1e4 + k / (N - 1)
  negative        -1 + 0.3 k / (N - 1)
  descending      ``unit`` with t, y, t_add, y_add and t_new reversed (``Problem.restore`` puts the
                  outputs back in ``unit`` order)
  permuted        ``unit`` under a fixed permutation of the n training points: on the lattice but not
                  regular — tables without structured storage and without the Toeplitz leaf
  backcast        ``unit`` with the forecast dates BEFORE the first training date (tmin comes from
                  t_new); its date sets are ``before`` (even indices) and ``before_odd``
  sparse_lo, sparse_hi   n + d dates drawn from a fine lattice of Q steps, Q = 16 (n + d + m) + 4096
                  - 8: the table-cost refusal of detect_lattice (csrc/ngp_plan.h) counts the dates of
                  the call, so the SAME training data is accepted with m forecast dates (lo) and
                  refused with m - 1 (hi: the lo set without its second-to-last date).  Every set
                  ends in one anchor date at fine index Q, which fixes the span; the two sides are
                  compared on the dates they share.  Gradient jobs see the n training dates alone.
  nudged_<e>      ``unit`` with one interior training date moved by e = 1, 8, 64 ulp of its value or
                  1e-12, 1e-10, 1e-8 of the span: either side of the acceptance (residuals within
                  2.5 eps span of each other; 1 ulp of a date near 0.5 is half an eps of the span,
                  8 ulp are four) and of the 1e-9 span snapping inside the Euclid loop.  The reference
                  sees the date as given.

Sizes: n = 321 (nb0 = 5, tail 1: column sweep, structured storage, Toeplitz leaf) and n = 130
(nb0 = 2, tail 2: the one-launch kernel too); B = 12 items — pure stationary trees of 1, 3 and 7
operators, item 10 with a Linear leaf, item 11 with a ChangePoint; d = 2, D = 2, m = 6.
"""
import functools
from dataclasses import dataclass

import numpy as np

from tests import hp_reference as hr
from tests import value_cases as vc

NS = (321, 130)
B, D_ADD, D_SCEN, M = 12, 2, 2, 6
SIZES = (1, 3, 7)
LINEAR_ITEM, CP_ITEM = 10, 11
DATE_SETS = ("beyond", "between", "on_f")
NUDGES = {"1ulp": ("ulp", 1), "8ulp": ("ulp", 8), "64ulp": ("ulp", 64),
          "1e-12": ("span", 1e-12), "1e-10": ("span", 1e-10), "1e-8": ("span", 1e-8)}
AFFINE = ("days_over_last", "raw_days", "decimal_years", "shift100", "shift1e4", "negative")
LAYOUTS = ("unit",) + AFFINE + ("descending", "permuted", "backcast", "sparse_lo", "sparse_hi") + \
    tuple(f"nudged_{e}" for e in NUDGES)
# what detect_lattice must still recognise (route guards), and the nudges it refuses by its rule:
# 8 ulp of a date near 0.5 are 4 eps span > 2.5, and so is everything larger; 1 ulp may go either way
GUARDED = ("unit", "days_over_last", "raw_days", "descending")
NUDGES_REFUSED = ("nudged_8ulp", "nudged_64ulp", "nudged_1e-12", "nudged_1e-10", "nudged_1e-8")


def _index_date(name, k, N):
    k = np.asarray(k, dtype=float)
    if name == "days_over_last":
        return (7.0 * k) / (7.0 * (N - 1))
    if name == "raw_days":
        return 19000.0 + 7.0 * k
    if name == "decimal_years":
        return 2020.0 + k / 52.0
    if name == "shift100":
        return 100.0 + k / (N - 1)
    if name == "shift1e4":
        return 1e4 + k / (N - 1)
    if name == "negative":
        return -1.0 + 0.3 * k / (N - 1)
    return k / (N - 1)


def affine_of(name, N):
    """(a, b) of t = a u + b"""
    return {"raw_days": (7.0 * (N - 1), 19000.0), "decimal_years": ((N - 1) / 52.0, 2020.0),
            "shift100": (1.0, 100.0), "shift1e4": (1.0, 1e4), "negative": (0.3, -1.0)}.get(name, (1.0, 0.0))


_NPAR = {1: 1, 2: 3, 3: 2, 4: 3, 5: 3, 6: 0, 7: 0, 8: 2}


def map_program(prog, a, b):
    """the program of the same GP on dates a u + b, and d theta' / d theta of every parameter
    (noise last)"""
    assert a > 0
    ops, par, nz = prog
    out, sc, p = np.array(par, float), np.ones(len(par) + 1), 0
    for op in (int(o) for o in ops):
        if op == 2:
            out[p], sc[p] = a * par[p] + b, a
            out[p + 2], sc[p + 2] = par[p + 2] / (a * a), 1.0 / (a * a)
        elif op in (3, 4):
            out[p], sc[p] = a * par[p], a
        elif op == 5:
            out[p + 1], sc[p + 1] = a * par[p + 1], a
        elif op == 8:
            out[p], sc[p] = a * par[p] + b, a
            out[p + 1], sc[p + 1] = a * par[p + 1], a
        p += _NPAR[op]
    assert p == len(par)
    return (np.asarray(ops, np.int32), out, float(nz)), sc


@functools.lru_cache(maxsize=None)
def unit_programs(n):
    """the ensemble on ``unit`` dates: items 0 .. 9 stationary trees of 1, 3, 7 operators, item 10
    with a Linear leaf, item 11 with a ChangePoint; noise chosen as value_cases does"""
    progs = vc._items(41, SIZES, B, n, LINEAR_ITEM + 1, CP_ITEM + 1, True)
    assert 2 in progs[LINEAR_ITEM][0] and 8 in progs[CP_ITEM][0]
    for i in range(LINEAR_ITEM):
        assert not np.isin(progs[i][0], (2, 8)).any()
    return progs


def sample(n):
    """one pure stationary tree (of the seven-operator ones with a Periodic leaf — the leaf with the
    shortest scale, a period down to 0.05 of the span — the one with the least noise), the Linear and
    the ChangePoint tree"""
    progs = unit_programs(n)
    stat = [i for i in range(LINEAR_ITEM) if len(progs[i][0]) == 7 and 5 in progs[i][0]]
    return (min(stat, key=lambda i: progs[i][2]), LINEAR_ITEM, CP_ITEM)


def stationary_items():
    return list(range(LINEAR_ITEM))


@dataclass
class Problem:
    name: str
    n: int
    a: float
    b: float
    progs: list
    pscale: list
    t: np.ndarray
    y: np.ndarray
    t_add: np.ndarray
    y_add: np.ndarray
    sets: dict          # {set name: (t_new, noise_on_new)}
    reverse: bool = False

    def restore(self, out):
        """outputs of one item in the order of the ``unit`` layout"""
        if not self.reverse:
            return out
        o = dict(out)
        o["mu"] = np.asarray(out["mu"])[..., ::-1]
        o["sigma"] = np.asarray(out["sigma"])[::-1, ::-1]
        return o


def _values(u, seed, N):
    """observations of the series at unit dates u (the function of value_cases.series)"""
    rng = np.random.default_rng(seed)
    return np.sin(2 * np.pi * u * 3) + 0.5 * u + 0.1 * rng.standard_normal(N)


def _sparse(n, hi):
    d, m = D_ADD, M
    nt = n + d
    Q = 16 * (nt + m) + 4096 - 8
    assert 16 * (nt + m - 1) + 4096 < Q <= 16 * (nt + m) + 4096
    Qt = Q - 48
    rng = np.random.default_rng(97 + n)
    v = np.sort(rng.choice(Qt - (nt - 1) + 1, nt, replace=False)) + np.arange(nt)   # gaps >= 2
    v[0], v[-1] = 0, Qt
    assert np.all(np.diff(v) >= 2) and np.gcd.reduce(v) == 1
    date = lambda q: np.asarray(q, float) / Qt
    y_all = _values(date(v), 5, nt)
    rng2 = np.random.default_rng(36)
    y_add = y_all[n:][None, :] + 0.1 * rng2.standard_normal((D_SCEN, d))
    gaps = np.unique(np.round(np.linspace(0, nt - 2, m - 1)).astype(int))
    obs = np.unique(np.round(np.linspace(0, nt - 1, m - 1)).astype(int))
    sets = {"beyond": (np.concatenate([Qt + 8 * np.arange(1, m), [Q]]), True),
            "between": (np.concatenate([v[gaps] + 1, [Q]]), True),
            "on_f": (np.concatenate([v[obs], [Q]]), False)}
    keep = [0, 1, 2, 3, 5] if hi else list(range(m))
    return v, date, y_all, y_add, {k: (date(q[keep]), non) for k, (q, non) in sets.items()}


SPARSE_SHARED = ([0, 1, 2, 3, 5], [0, 1, 2, 3, 4])   # lo columns, hi columns of the dates both hold


@functools.lru_cache(maxsize=None)
def problem(name, n):
    assert name in LAYOUTS and n in NS
    d, m = D_ADD, M
    nt = n + d
    N = 2 * nt + 1
    base = list(unit_programs(n))
    if name.startswith("sparse"):
        v, date, y_all, y_add, sets = _sparse(n, name == "sparse_hi")
        tt = date(v)
        return Problem(name, n, 1.0, 0.0, base, [np.ones(len(p[1]) + 1) for p in base], tt[:n], y_all[:n],
                       tt[n:], y_add, sets)
    a, b = affine_of(name, N)
    mapped = [map_program(p, a, b) for p in base]
    progs, pscale = [p for p, _ in mapped], [s for _, s in mapped]
    date = lambda k: _index_date(name, k, N)
    ya = _values(np.arange(N) / (N - 1), 3, N)
    tr = 2 * np.arange(nt)
    rng = np.random.default_rng(34)
    t, y, t_add = date(tr[:n]), ya[tr[:n]], date(tr[n:])
    y_add = ya[tr[n:]][None, :] + 0.1 * rng.standard_normal((D_SCEN, d))
    gaps = np.unique(np.round(np.linspace(0, nt - 2, m)).astype(int))
    obs = np.unique(np.round(np.linspace(0, nt - 1, m)).astype(int))
    assert gaps.size == m and obs.size == m
    if name == "backcast":
        sets = {"before": (date(-2.0 * np.arange(1, m + 1)), True),
                "before_odd": (date(-(2.0 * np.arange(1, m + 1) - 1)), True)}
    else:
        sets = {"beyond": (date(2 * (nt - 1) + 2 * np.arange(1, m + 1)), True),
                "between": (date(2 * gaps + 1), True),
                "on_f": (date(2 * obs), False)}
    reverse = name == "descending"
    if reverse:
        t, y, t_add, y_add = t[::-1].copy(), y[::-1].copy(), t_add[::-1].copy(), y_add[:, ::-1].copy()
        sets = {k: (tn[::-1].copy(), non) for k, (tn, non) in sets.items()}
    if name == "permuted":
        perm = np.random.default_rng(58).permutation(n)
        t, y = t[perm], y[perm]
    if name.startswith("nudged_"):
        kind, e = NUDGES[name[7:]]
        j = n // 2 + 3
        t = t.copy()
        t[j] += e * (np.spacing(t[j]) if kind == "ulp" else 1.0)      # (the span of ``unit`` is 1)
    return Problem(name, n, a, b, progs, pscale, t, y, t_add, y_add, sets, reverse)


def reference(name, n, i, set_name):
    p = problem(name, n)
    t_new, non = p.sets[set_name]
    return hr.nowcast(p.progs[i], p.t, p.y, p.t_add, p.y_add, t_new, None, noise_on_new=non)

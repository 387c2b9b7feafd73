"""The cases of the sampler tests and the judgement both of them make, in one table.

tests/test_sampler_gpu.py runs these cases through ``ngp_mixture_sample`` / ``_indep``;
tests/test_sampler_reference_cpu.py admits them (cond <= 1e9, pick margins above 2^-40, nothing
skipped), measures the fp64 oracle on them (R64 below) and shows that the judgement rejects every
deliberately wrong variant of the reference on one of them.

A case is the shared form's input; every case with S > 1 also has an independent form
(``Case.indep``): mixture s takes component k's mean mu[k][s] and the covariance of component
(k + s) mod P — a different matrix at every (s, k), so info and the factor read with the wrong
stride show — and seeds[0] is the case's own seed, the others are distinct.

Judgement, per draw and coordinate (``judge``): comp exactly; the deviation x_i - mu_{k,i} against
the reference's (L z)_i on the scale s_i = sqrt(sigma_ii) max(1, |z|_inf), the size of the terms it
is summed from, within ``tests.util.tol(FLOOR, cond(sigma_k))``.
"""
import functools
from dataclasses import dataclass

import numpy as np

from tests import grammar_cases as gc
from tests import hp_reference as hr
from tests import sampler_reference as sr
from tests import value_cases as vc
from tests.util import check_components

LD = hr.LD
COND_MAX = 1e9
# the fp64 oracle against the reference over this table (test_sampler_reference_cpu.py measures it
# and asserts that this is what it finds); the GPU floor is four times that (tests/sampler_reference.py)
R64 = 2.82e-12
FLOOR = 4 * R64
PIVOT_MARGIN = 1e-6          # of the largest diagonal entry: the reference's pivots clear it on both sides


@dataclass(frozen=True, eq=False)
class Case:
    name: str
    w: np.ndarray            # [S, P]
    mu: np.ndarray           # [P, S, m]
    sigma: np.ndarray        # [P, m, m]
    draws: int
    seed: int
    ties: tuple = ()         # (s, d) built to have u == acc_i exactly: exempt from the margin rule
    bad: tuple = ()          # (component, first failing row) of matrices made indefinite

    @property
    def shape(self):
        return self.w.shape[1], self.w.shape[0], self.mu.shape[2], self.draws      # P, S, m, draws

    def indep(self):
        """(w, mu [S, P, m], sigma [S, P, m, m], seeds) or None when S = 1"""
        P, S, m, _ = self.shape
        if S == 1:
            return None
        mu = np.ascontiguousarray(self.mu.transpose(1, 0, 2))
        sigma = np.stack([np.roll(self.sigma, -s, axis=0) for s in range(S)])
        seeds = [self.seed] + [self.seed ^ (0x9E3779B97F4A7C15 * s & (2 ** 64 - 1)) for s in range(1, S)]
        return self.w, mu, sigma, seeds


# ---- covariances ------------------------------------------------------------------------------------
def smooth_sigma(rng, P, m):
    """SE covariances on m regular dates plus noise (cond up to about 3e5): the shape cases"""
    t = np.arange(m) / max(m - 1, 1)
    d2 = (t[:, None] - t[None, :]) ** 2
    out = []
    for _ in range(P):
        ell, amp, noise = rng.uniform(0.05, 0.5), rng.uniform(0.3, 1.5), np.exp(rng.uniform(np.log(1e-3), np.log(1e-1)))
        out.append(amp * np.exp(-0.5 * d2 / ell ** 2) + noise * np.eye(m))
    return np.stack(out)


def _zoo(name):
    return gc.PROGRAMS[gc.NAMES.index(name)]


# long-lengthscale SE, SE x Periodic, a ChangePoint tree of the grammar zoo
SE_LONG = (np.array([3], np.int32), np.array([0.8, 1.0]))
SE_PER = (np.array([3, 5, 7], np.int32), np.array([0.6, 1.0, 0.9, 0.25, 0.8]))
REAL_TREES = (SE_LONG, SE_PER, _zoo("cp_both_general")[:2])
REAL_N, REAL_D, REAL_SCEN = 100, 2, 3
NOISE_ENDS = (vc.noise_floor(REAL_N), 1e-1)
# the group without noise on the forecast dates: the covariance of f plus the default jitter, which
# alone separates a smooth tree's from singular
F_TREES = ("se_long", "se_x_per", "cp_both_general", "se", "plus_C_GE", "per_third")
JITTER = 1e-5


@functools.lru_cache(maxsize=None)
def real_predictive(m, noise_on_new=True):
    """(mu [P, S, m], sigma [P, m, m], names) from hp_reference.nowcast, rounded to fp64: n = 100
    training dates, d = 2 appended with 3 scenarios, m forecast dates after the last one; with the
    noise on them (noise_on_new) or the variance of f alone plus JITTER"""
    t_all, y_all = vc.series(2 * (REAL_N + REAL_D) + 1, True, seed=61)
    tr = np.arange(REAL_N + REAL_D) * 2
    t, y, t_add = t_all[tr[:REAL_N]], y_all[tr[:REAL_N]], t_all[tr[REAL_N:]]
    rng = np.random.default_rng(62)
    y_add = y_all[tr[REAL_N:]][None, :] + 0.1 * rng.standard_normal((REAL_SCEN, REAL_D))
    t_new = t_all[-1] + (t_all[2] - t_all[0]) * np.arange(1, m + 1)
    if noise_on_new:
        progs = [(ops, par, nz) for nz in NOISE_ENDS for ops, par in REAL_TREES]
        names = [f"{k}@{nz:g}" for nz in NOISE_ENDS for k in ("se_long", "se_x_per", "cp_both_general")]
    else:
        named = dict(se_long=SE_LONG + (NOISE_ENDS[0],), se_x_per=SE_PER + (NOISE_ENDS[0],))
        progs = [named[k] if k in named else _zoo(k) for k in F_TREES]
        names = list(F_TREES)
    mu, sigma = [], []
    for p in progs:
        r = hr.nowcast(p, t, y, t_add, y_add, t_new, None, noise_on_new=noise_on_new)
        assert r.info == 0
        mu.append(np.asarray(r.mu, np.float64))
        sg = r.sigma if noise_on_new else r.sigma + LD(JITTER) * np.eye(m, dtype=LD)
        sigma.append(np.asarray(sg, np.float64))
    return np.stack(mu), np.stack(sigma), tuple(names)


@functools.lru_cache(maxsize=None)
def f_group():
    """the noise_on_new = False candidates whose long-double cond is at most COND_MAX"""
    mu, sigma, names = real_predictive(60, False)
    keep = []
    for k in range(len(names)):
        L, info = hr.cholesky_ld(sigma[k].astype(LD))
        if info == 0 and sr.cond_ld(sigma[k], L) <= COND_MAX:
            keep.append(k)
    return mu[keep], sigma[keep], tuple(names[k] for k in keep)


# ---- weight rows -----------------------------------------------------------------------------------------
def tie_row(seed, s, draws, tail):
    """a weight row [u*, 1/4, rest, *tail] whose fp64 running sum ends at 1 - 2^-6, u* the uniform of
    the first draw d* of (seed, scenario s) in (0.2, 0.45): below 1/2 it is an fp64 number, so
    u == acc_0 holds exactly for everybody and strict `<` sends draw d* on to component 1; some
    other draw has u above the final sum and takes the fallback.  -> (row, d*)"""
    ref = sr.REFERENCE
    r = ref.words(seed, s, draws, 0)
    u = ref.uniform(r[:, 0], r[:, 1])
    d = int(np.flatnonzero((u > 0.2) & (u < 0.45))[0])
    ustar = float(u[d])
    assert LD(ustar) == u[d]
    row = np.array([ustar, 0.25, 0.0] + list(tail))
    row[2] = (1.0 - 2.0 ** -6) - (ustar + 0.25)
    assert np.add.accumulate(row)[-1] < 1.0 - 2.0 ** -7 and np.any(u > 1.0 - 2.0 ** -6)
    return row, d


# ---- the table ------------------------------------------------------------------------------------------
def _seed(m, draws):
    return 0x0123456789ABCDEF + 1000 * m + draws


def _shape_case(name, P, S, m, draws, w=None, ties=()):
    rng = np.random.default_rng([P, S, m, draws])
    w = rng.dirichlet(np.ones(P), size=S) if w is None else np.asarray(w, float)
    return Case(name, w, rng.standard_normal((P, S, m)), smooth_sigma(rng, P, m), draws,
                _seed(m, draws), ties=ties)


def _indefinite(sigma, k):
    """sigma with c e_k e_k' subtracted (k 1-based): the pivot at row k becomes -0.1 sigma_kk"""
    _, info, piv = hr.cholesky_ld(sigma.astype(LD), pivots=True)
    assert info == 0
    out = sigma.copy()
    out[k - 1, k - 1] -= float(piv[k - 1]) + 0.1 * sigma[k - 1, k - 1]
    return out


def _pivot_case(m):
    mu, sigma, _ = real_predictive(m)
    sigma = sigma.copy()
    bad = ((1, 1), (2, 17), (4, 18), (5, m))
    for comp, k in bad:
        sigma[comp] = _indefinite(sigma[comp], k)
    rng = np.random.default_rng(700 + m)
    return Case(f"pivots_m{m}", rng.dirichlet(np.ones(6), size=REAL_SCEN), mu, sigma, 64, 0xBADC0FFEE + m, bad=bad)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # horizon: odd m, one and two trips of the 256-thread trailing update (17, 18), NGP_MAX_AUX
    for m in (1, 2, 3, 16, 17, 18, 63, 64, 65, 191, 192):
        out.append(_shape_case(f"m{m}", 3, 2, m, 5))
    # S x draws around one workgroup of 256 draws; idx / draws and idx % draws
    for S, draws in ((1, 255), (1, 256), (1, 257), (3, 85), (2, 128), (3, 86), (3, 1)):
        out.append(_shape_case(f"S{S}_draws{draws}", 2, S, 3, draws))
    # P and S: the two layouts of mu differ only when S != P and both exceed 1
    out.append(_shape_case("P1_S3", 1, 3, 5, 40))
    out.append(_shape_case("P5_S3", 5, 3, 6, 40))
    rng = np.random.default_rng(1500)
    w = np.zeros((2, 1500))
    for s in range(2):
        on = rng.choice(1500, 40, replace=False)
        w[s, on] = rng.dirichlet(np.ones(40))
    out.append(_shape_case("P1500_sparse", 1500, 2, 4, 64, w=w))
    # weight rows: zeros first, in the middle, last; one-hot
    out.append(_shape_case("zero_weights", 5, 4, 4, 64,
                           w=[[0, 0, .25, .5, .25], [.5, 0, 0, .25, .25], [.25, .5, .25, 0, 0], [0, 0, 0, 1, 0]]))
    # the fallback: running sums that end at 1 - 2^-6, last weight positive | zeros last
    r0, d0 = tie_row(_seed(4, 250), 0, 250, (0.0, 0.0))  # zeros last: the contract picks P - 1 = 4
    r1, d1 = tie_row(_seed(4, 250), 1, 250, ())
    out.append(_shape_case("fallback", 5, 2, 4, 250, w=[r0, [r1[0], r1[1], 0.0, 0.0, r1[2]]],
                           ties=((0, d0), (1, d1))))
    # real predictive covariances: noise at both ends of value_cases' range
    for m in (60, 192):
        mu, sigma, _ = real_predictive(m)
        rng = np.random.default_rng(600 + m)
        out.append(Case(f"real_m{m}", rng.dirichlet(np.ones(6), size=REAL_SCEN), mu, sigma, 64, 0xC0FFEE + m))
    mu, sigma, names = f_group()
    rng = np.random.default_rng(660)
    out.append(Case("real_f_m60", rng.dirichlet(np.ones(len(names)), size=REAL_SCEN), mu, sigma, 64, 0xF00D))
    # pivot reports: real covariances made indefinite at row k
    out += [_pivot_case(64), _pivot_case(192)]
    assert len({c.name for c in out}) == len(out)
    return {c.name: c for c in out}


NAMES = ("m1", "m2", "m3", "m16", "m17", "m18", "m63", "m64", "m65", "m191", "m192",
         "S1_draws255", "S1_draws256", "S1_draws257", "S3_draws85", "S2_draws128", "S3_draws86",
         "S3_draws1", "P1_S3", "P5_S3", "P1500_sparse", "zero_weights", "fallback", "real_m60",
         "real_m192", "real_f_m60", "pivots_m64", "pivots_m192")
INDEP_NAMES = tuple(n for n in NAMES if not n.startswith("S1_"))


@functools.lru_cache(maxsize=None)
def reference(name, indep=False):
    c = cases()[name]
    if indep:
        w, mu, sigma, seeds = c.indep()
        return sr.sample_indep(w, mu, sigma, c.draws, seeds)
    return sr.sample(c.w, c.mu, c.sigma, c.draws, c.seed)


# ---- the judgement ----------------------------------------------------------------------------------------
def scaled_errors(x, ref, mu, sigma):
    """e [S, draws, m] = |(x - mu_k) - (L z)| / (sqrt(sigma_ii) max(1, |z|_inf)) and cond [S, draws] of
    every draw's component, NaN where its component failed; mu, sigma in the form of ``ref``"""
    S, draws, m = ref.x.shape
    e, cond = np.full((S, draws, m), np.nan), np.full((S, draws), np.nan)
    zmax = np.maximum(1.0, np.max(np.abs(ref.z), axis=2).astype(np.float64))
    for s in range(S):
        for k in np.unique(ref.comp[s]):
            info = ref.info[s, k] if ref.indep else ref.info[k]
            if info:
                continue
            sel = ref.comp[s] == k
            mk = (mu[s, k] if ref.indep else mu[k, s]).astype(LD)
            sg = sigma[s, k] if ref.indep else sigma[k]
            diff = (np.asarray(x[s][sel]).astype(LD) - mk[None, :]) - ref.dev[s, sel]
            e[s, sel] = (np.abs(diff) / (np.sqrt(np.diag(sg))[None, :] * zmax[s, sel, None])).astype(np.float64)
            cond[s, sel] = ref.cond[s, k] if ref.indep else ref.cond[k]
    return e, cond


def judge(what, x, comp, ref, mu, sigma, floor=FLOOR, record=True):
    """comp exactly; every draw of a healthy component within tol(floor, cond_k) componentwise and
    free of NaN; -> the worst scaled error"""
    if comp is not None:
        assert np.array_equal(comp, ref.comp), (what, np.flatnonzero(np.asarray(comp) != ref.comp)[:8])
    e, cond = scaled_errors(x, ref, mu, sigma)
    healthy = np.isfinite(cond)
    assert not np.isnan(np.asarray(x, np.float64)[healthy]).any(), what
    for c in np.unique(cond[healthy]):
        sel = healthy & (cond == c)
        check_components(what, e[sel], np.zeros_like(e[sel]), 1.0, floor, c, ctx=what, record=record)
    return float(np.max(e[healthy])) if healthy.any() else 0.0

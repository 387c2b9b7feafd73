"""The host side of the additive decomposition (include/ngp.h), without a
GPU: the slicing of ngp_kernel_components on hand-written trees, the long double restatement
tests/component_reference.py against the identities it must satisfy, the classification of parts,
the grouped marginals (a particle that lacks a group is a point mass at 0) and the argument errors
that return before anything touches a device."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
from nowcastautogp_amd import _lib, autogp, gp
from nowcastautogp_amd._abi import KernelArray
from oracle import oracle_np
from tests import component_reference as cr
from tests import hp_reference as hr

NGP_ERR_ARG, NGP_ERR_PROGRAM = -1, -2

LIN = gp.Linear(0.3, 0.1, 0.8)
PER = gp.Periodic(1.2, 0.2, 0.4)
SE = gp.SquaredExponential(0.15, 0.3)
GE = gp.GammaExponential(0.3, 1.5, 0.2)
CON = gp.Constant(0.25)
CP = gp.ChangePoint(gp.Plus(SE, CON), PER, 0.5, 0.1)

# (tree, the components it must give)
TREES = {
    "leaf": (PER, [PER]),
    "left-deep": (gp.Plus(gp.Plus(LIN, PER), SE), [LIN, PER, SE]),
    "right-deep": (gp.Plus(LIN, gp.Plus(PER, SE)), [LIN, PER, SE]),
    "plus under times": (gp.Times(gp.Plus(LIN, PER), SE), [gp.Times(gp.Plus(LIN, PER), SE)]),
    "changepoint and periodic": (gp.Plus(gp.ChangePoint(SE, GE, 0.4, 0.2), PER),
                                 [gp.ChangePoint(SE, GE, 0.4, 0.2), PER]),
    "plus below a changepoint": (CP, [CP]),
    "mixed": (gp.Plus(gp.Plus(CON, gp.Times(gp.Plus(LIN, CON), PER)), gp.Plus(CP, GE)),
              [CON, gp.Times(gp.Plus(LIN, CON), PER), CP, GE]),
}


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return _lib.load()


def prog(tree, noise=0.07):
    return gp.to_program(tree) + (noise,)


@pytest.mark.parametrize("name", sorted(TREES))
def test_slicing_of_hand_written_trees(lib, name):
    tree, want = TREES[name]
    got = _lib.kernel_components(prog(tree))
    assert len(got) == len(want)
    for (ops, params, noise), w in zip(got, want):
        w_ops, w_par = gp.to_program(w)
        assert np.array_equal(ops, w_ops) and np.array_equal(params, w_par) and noise == 0.07
        assert _lib.kernel_check((ops, params, noise)) == 0        # a component is a valid program
    # the restatement in the test helper slices the same way
    ref = cr.components(prog(tree))
    assert len(ref) == len(got)
    for a, b in zip(ref, got):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", sorted(TREES))
def test_slices_joined_by_plus_reproduce_the_covariance(lib, name):
    tree, _ = TREES[name]
    parts = _lib.kernel_components(prog(tree))
    rng = np.random.default_rng(7)
    t1, t2 = np.sort(rng.uniform(0, 1.2, 23)), np.sort(rng.uniform(0, 1.2, 17))
    K = oracle_np.cov(prog(tree), t1, t2)
    total = sum(oracle_np.cov(p, t1, t2) for p in parts)
    assert np.max(np.abs(total - K)) <= 1e-15 * np.max(np.abs(K))
    ops = np.concatenate([p[0] for p in parts] + [np.full(len(parts) - 1, gp.PLUS, np.int32)])
    joined = (ops.astype(np.int32), np.concatenate([p[1] for p in parts]), 0.07)
    assert _lib.kernel_check(joined) == 0
    Kj = oracle_np.cov(joined, t1, t2)
    assert np.max(np.abs(Kj - K)) <= 1e-15 * np.max(np.abs(K))


def test_kernel_components_argument_errors(lib):
    ka = KernelArray([prog(TREES["mixed"][0])])
    cnt = C.c_int32(-7)
    assert lib.ngp_kernel_components(None, C.byref(cnt), None, None, None, None) == NGP_ERR_ARG
    assert lib.ngp_kernel_components(C.byref(ka.arr[0]), None, None, None, None, None) == NGP_ERR_ARG
    assert lib.ngp_kernel_components(C.byref(ka.arr[0]), C.byref(cnt), None, None, None, None) == 0
    assert cnt.value == 4                                   # the count alone
    bad = KernelArray([(np.array([2, 6], np.int32), np.array([0.1, 0.2, 0.3]), 0.1)])
    assert lib.ngp_kernel_components(C.byref(bad.arr[0]), C.byref(cnt), None, None, None, None) == NGP_ERR_PROGRAM


def test_factor_components_rejects_a_null_factor_before_the_device(lib):
    """the only argument error that can be reached without a factor, hence without a GPU; the others
    are in tests/test_components_gpu.py and in tests/sanitize/components_stress.cpp (mock runtime)"""
    ka = KernelArray([prog(PER)])
    one = np.array([1], np.int32)
    buf = np.zeros(4)
    st = lib.ngp_factor_components(None, one.ctypes.data_as(C.POINTER(C.c_int32)), ka.arr, 1,
                                   buf.ctypes.data_as(C.POINTER(C.c_double)),
                                   buf.ctypes.data_as(C.POINTER(C.c_double)), None, None, None)
    assert st == NGP_ERR_ARG


@pytest.mark.parametrize("name", ["left-deep", "mixed", "changepoint and periodic", "leaf"])
def test_the_reference_satisfies_the_three_identities(name):
    """sum_c mu_c = mu, sum_cc' Sigma_cc' = Sigma (the noise-free predictive of tests/hp_reference.py),
    every Sigma_cc positive semi-definite — in long double, to its own rounding"""
    tree, _ = TREES[name]
    p = prog(tree)
    comps = cr.components(p)
    n, m = 45, 6
    rng = np.random.default_rng(3)
    t = np.sort(rng.uniform(0, 1, n))
    y = np.sin(7 * t) + 0.1 * rng.standard_normal(n)
    t_new = 1.0 + 0.03 * np.arange(1, m + 1)
    r = cr.evaluate(p, comps, t, y, t_new)
    full = hr.evaluate(p, t, y, grad=False, t_new=t_new, noise_on_new=False)
    assert r.info == 0 and full.info == 0
    C_ = len(comps)
    bound = 1e3 * hr.EPS_LD * r.cond
    mu_sum = r.mu.sum(axis=0)
    assert float(np.max(np.abs(mu_sum - full.mu)) / np.max(np.abs(full.mu))) < bound
    sg_sum = r.sigma.reshape(C_, m, C_, m).sum(axis=(0, 2))
    assert float(np.max(np.abs(sg_sum - full.sigma)) / np.max(np.abs(full.sigma))) < bound
    for c in range(C_):
        ev = np.linalg.eigvalsh(r.sigma[c * m:(c + 1) * m, c * m:(c + 1) * m].astype(float))
        assert ev[0] > -1e-12 * ev[-1]
    assert np.array_equal(r.sigma, r.sigma.T)


def test_kind_of_a_component():
    kinds = {
        "trend": [LIN, gp.Times(LIN, PER), gp.ChangePoint(LIN, SE, 0.5, 0.1), gp.Times(gp.Plus(LIN, CON), PER)],
        "seasonal": [PER, gp.Times(PER, SE), gp.ChangePoint(PER, CON, 0.5, 0.1)],
        "other": [SE, CON, GE, gp.Times(SE, GE), gp.ChangePoint(SE, GE, 0.5, 0.1)],
    }
    for kind, trees in kinds.items():
        for tr in trees:
            assert autogp.component_kind(gp.to_program(tr)[0]) == kind, (kind, str(tr))


class _Stub:
    """what decompose reads of a model"""

    def __init__(self, trees):
        self._p = [prog(t) for t in trees]

    def programs(self):
        return self._p


def test_decompose_labels_and_kinds(lib):
    parts = autogp.decompose(_Stub([TREES["left-deep"][0], TREES["plus under times"][0], CP]))
    assert [[c.kind for c in ps] for ps in parts] == [["trend", "seasonal", "other"], ["trend"], ["seasonal"]]
    assert parts[0][1].label == str(PER) and str(parts[0][1].tree) == str(PER)
    assert parts[2][0].label.startswith("ChangePoint(Plus(")


def _forecast(m=4):
    """three particles by hand: (trend, seasonal), (seasonal, seasonal, other), (trend) — the third
    has no seasonal part"""
    rng = np.random.default_rng(5)
    kinds = [["trend", "seasonal"], ["seasonal", "seasonal", "other"], ["trend"]]
    means, sigma, var = [], [], []
    for ks in kinds:
        k = len(ks) * m
        A = rng.standard_normal((k, k))
        S = A @ A.T / k + 0.1 * np.eye(k)
        means.append(rng.standard_normal((len(ks), m)))
        sigma.append(S)
        var.append(np.diag(S).reshape(len(ks), m).copy())
    w = np.array([0.5, 0.3, 0.2])
    labels = [[f"k{p}{c}" for c in range(len(ks))] for p, ks in enumerate(kinds)]
    return autogp.ComponentForecast(means, sigma, var, w, kinds, labels, 2.5), m


def test_grouped_sums_the_blocks_of_a_group():
    fc, m = _forecast()
    g = fc.grouped()
    assert list(g) == ["trend", "seasonal", "other"]
    sea = g["seasonal"]
    # particle 1 has two seasonal parts: their means add, and so do all four covariance blocks
    S = fc.sigma[1].reshape(3, m, 3, m)
    want_var = np.array([S[0, j, 0, j] + S[1, j, 1, j] + 2 * S[0, j, 1, j] for j in range(m)])
    assert np.allclose(sea.means[1], fc.means[1][0] + fc.means[1][1], rtol=0, atol=1e-15)
    assert np.allclose(sea.variances[1], want_var, rtol=1e-14, atol=0)
    assert np.allclose(sea.means[0], fc.means[0][1]) and np.allclose(sea.variances[0], fc.var[0][1])
    with pytest.raises(ValueError):
        fc.grouped(by="colour")
    assert list(fc.grouped(by="label")) == ["k00", "k01", "k10", "k11", "k12", "k20"]


def test_a_particle_without_the_group_is_a_point_mass_at_zero():
    fc, m = _forecast()
    sea = fc.grouped()["seasonal"]
    assert isinstance(sea, autogp.AtomMixtureMarginals) and isinstance(sea, autogp.MixtureMarginals)
    assert abs(sea.atom - 0.2) < 1e-15 and np.allclose(sea.weights, [0.625, 0.375])
    rest = autogp.MixtureMarginals(sea.means, sea.variances, sea.weights)
    # cdf: the rest scaled, with a step of 0.2 at zero
    x = np.array([-0.5, -1e-9, 0.0, 0.7])
    F, Fr = sea.cdf(x), rest.cdf(x)
    assert np.allclose(F, 0.8 * Fr + 0.2 * (x >= 0), rtol=0, atol=1e-15)
    assert np.allclose(sea.mean(), 0.8 * rest.mean())
    # quantiles invert that cdf: F(q-) <= p <= F(q), and the levels inside the step give exactly 0
    probs = np.array([0.01, 0.2, 0.45, 0.5, 0.55, 0.8, 0.99])
    q = sea.quantile(probs)
    assert q.shape == (m, probs.size) and np.all(np.diff(q, axis=1) >= 0)
    F0 = 0.8 * rest.cdf(np.zeros(m))
    for j in range(m):
        for k, p in enumerate(probs):
            if F0[j] <= p <= F0[j] + 0.2:
                assert q[j, k] == 0.0
            else:
                assert q[j, k] != 0.0 and (q[j, k] < 0) == (p < F0[j])
                xj = np.zeros(m)
                xj[j] = q[j, k]
                assert abs(sea.cdf(xj)[j] - p) < 1e-12
    # crps against the definition by quadrature-free Monte Carlo is too loose; check its two limits
    # instead: without weight on the third particle the atom vanishes and the class is the plain one
    fc.weights = np.array([0.6, 0.4, 0.0])
    plain = fc.grouped()["seasonal"]
    assert type(plain) is autogp.MixtureMarginals
    y = np.array([0.3, -0.2, 0.0, 1.1])
    fc.weights = np.array([0.6, 0.4, 1e-300])
    tiny = fc.grouped()["seasonal"]
    assert isinstance(tiny, autogp.AtomMixtureMarginals)
    assert np.allclose(tiny.crps(y), plain.crps(y), rtol=1e-12, atol=0)
    # and a mixture that is almost all atom scores like the constant 0: CRPS -> |y|
    fc.weights = np.array([1e-9, 1e-9, 1.0])
    assert np.allclose(fc.grouped()["seasonal"].crps(y), np.abs(y), rtol=0, atol=1e-7)


def test_component_blocks_share_the_aux_rows():
    assert autogp.component_blocks(130, 3, 63) is None                 # 2 + 1 + 189 = 192
    assert autogp.component_blocks(130, 3, 64) == [(0, 63), (63, 64)]
    assert autogp.component_blocks(127, 4, 70) == [(0, 32), (32, 64), (64, 70)]
    with pytest.raises(ValueError):
        autogp.component_blocks(127, 129, 1)


def test_crps_with_an_atom_against_its_definition():
    """CRPS = integral of (F(x) - 1[x >= y])^2 dx, by quadrature on the mixture's own cdf (step at 0
    included), at an atom of 0.2 — neither of the two limits: a wrong cross term between the atom
    and the continuous rest would show here"""
    from scipy.integrate import quad
    fc, m = _forecast()
    sea = fc.grouped()["seasonal"]
    assert abs(sea.atom - 0.2) < 1e-15
    y = np.array([0.3, -0.2, 0.0, 1.1])
    got = sea.crps(y)
    w, mu, var = sea.weights, sea.means, sea.variances
    import math
    for j in range(m):
        def F(x):
            cont = sum(wc * 0.5 * math.erfc(-(x - mu[c, j]) / math.sqrt(2 * var[c, j]))
                       for c, wc in enumerate(w))
            return 0.8 * cont + (0.2 if x >= 0 else 0.0)
        span = 12 * float(np.sqrt(var[:, j].max())) + float(np.abs(mu[:, j]).max()) + abs(y[j])
        cuts = sorted({-span, 0.0, float(y[j]), span})
        want = sum(quad(lambda x: (F(x) - (1.0 if x >= y[j] else 0.0)) ** 2, a, b,
                        epsabs=1e-12, epsrel=1e-12, limit=200)[0]
                   for a, b in zip(cuts[:-1], cuts[1:]) if b > a)
        assert abs(got[j] - want) < 1e-9, (j, got[j], want)

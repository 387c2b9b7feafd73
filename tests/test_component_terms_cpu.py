"""The host side of the sum-of-products terms and of the decomposition conditioned on nowcasts
(include/ngp.h), without a GPU: ngp_kernel_terms on the grammar zoo of
tests/grammar_cases.py under every split and both cp_form values, counts and order on hand-written
trees, its NGP_ERR_TOO_LARGE returns, the long double restatement
tests/component_nowcast_reference.py against the identities it must satisfy, decompose(split=...)
with its fallback, the argument errors that return before anything touches a device, and the host
code of ngp_factor_components_nowcast under ThreadSanitizer and AddressSanitizer + UBSan on the
mock runtime (tests/sanitize/components_nowcast_stress.cpp, a stand-alone program)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from nowcastautogp_amd import _lib, autogp, gp
from nowcastautogp_amd import nowcast as nc
from nowcastautogp_amd._abi import NGP_MAX_OPS, KernelArray, dptr, iptr
from oracle import oracle_np
from tests import component_nowcast_reference as cnr
from tests import grammar_cases as gc
from tests import hp_reference as hr
from tests.test_host_sanitizers import HIPCC, build

NGP_ERR_ARG, NGP_ERR_PROGRAM, NGP_ERR_TOO_LARGE = -1, -2, -3
SPLITS = (0, 1, 2, 3)

LIN = gp.Linear(0.3, 0.1, 0.8)
PER = gp.Periodic(1.2, 0.2, 0.4)
SE = gp.SquaredExponential(0.15, 0.3)
GE = gp.GammaExponential(0.3, 1.5, 0.2)
CON = gp.Constant(0.25)
Z = gp.Constant(0.0)


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return _lib.load()


def prog(tree, noise=0.07):
    return gp.to_program(tree) + (noise,)


def same_programs(got, want):
    assert len(got) == len(want)
    for (o1, p1, n1), (o2, p2, n2) in zip(got, want):
        assert np.array_equal(o1, o2) and np.array_equal(p1, p2) and n1 == n2


# ---- the grammar zoo ---------------------------------------------------------------------------------
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("i", range(len(gc.ZOO)), ids=gc.NAMES)
def test_terms_of_the_zoo_are_programs_that_sum_to_the_tree(lib, i, split):
    """every term passes ngp_kernel_check; sum_terms k_term(s, t) = k(s, t) on the zoo's own dates under
    both cp_form values, scale sum_terms max |K_term|, bound: the cov bound of
    tests/test_grammar_cases_cpu.py (8 x 4.41e-15) times the number of terms"""
    p = gc.PROGRAMS[i]
    terms = _lib.kernel_terms(p, split)
    same_programs(terms, cnr.terms(p, split))             # the library against the restatement
    for tm in terms:
        assert _lib.kernel_check(tm) == 0
        assert len(tm[0]) <= len(p[0]) and len(tm[1]) <= len(p[1])
    t1, t2, _ = gc.cov_dates()
    bound = 8.0 * gc.COV_WORST_FP64 * len(terms)
    for cp_form in (0, 1):
        spec = dict(se_form=0, periodic_form=0, cp_form=cp_form, jitter=1e-5)
        K = oracle_np.cov(p, t1, t2, False, spec)
        Kt = [oracle_np.cov(tm, t1, t2, False, spec) for tm in terms]
        scale = sum(float(np.max(np.abs(k))) for k in Kt)
        err = float(np.max(np.abs(sum(Kt) - K))) / scale
        assert err < bound, (gc.NAMES[i], split, cp_form, len(terms), err, bound)


@pytest.mark.parametrize("i", range(len(gc.ZOO)), ids=gc.NAMES)
def test_split_zero_is_ngp_kernel_components(lib, i):
    same_programs(_lib.kernel_terms(gc.PROGRAMS[i], 0), _lib.kernel_components(gc.PROGRAMS[i]))


# ---- counts and order --------------------------------------------------------------------------------
def CPT(l, r):
    return gp.ChangePoint(l, r, 0.5, 0.1)


HAND = {
    "CP(a+b, c)": (CPT(gp.Plus(LIN, PER), SE), 1, [CPT(LIN, Z), CPT(PER, Z), CPT(Z, SE)]),
    "CP(a+b, c) unsplit": (CPT(gp.Plus(LIN, PER), SE), 2, [CPT(gp.Plus(LIN, PER), SE)]),
    "(a+b)(c+d)": (gp.Times(gp.Plus(LIN, PER), gp.Plus(SE, CON)), 2,
                   [gp.Times(LIN, SE), gp.Times(LIN, CON), gp.Times(PER, SE), gp.Times(PER, CON)]),
    "(a+b)(c+d) unsplit": (gp.Times(gp.Plus(LIN, PER), gp.Plus(SE, CON)), 1,
                           [gp.Times(gp.Plus(LIN, PER), gp.Plus(SE, CON))]),
    "CP under Times": (gp.Times(CPT(gp.Plus(LIN, PER), SE), gp.Plus(GE, CON)), 3,
                       [gp.Times(CPT(LIN, Z), GE), gp.Times(CPT(LIN, Z), CON), gp.Times(CPT(PER, Z), GE),
                        gp.Times(CPT(PER, Z), CON), gp.Times(CPT(Z, SE), GE), gp.Times(CPT(Z, SE), CON)]),
    "CP under an unsplit Times": (gp.Plus(gp.Times(CPT(LIN, SE), PER), CON), 1,
                                  [gp.Times(CPT(LIN, SE), PER), CON]),
    "nested CP": (CPT(CPT(LIN, PER), gp.Plus(SE, GE)), 1,
                  [CPT(CPT(LIN, Z), Z), CPT(CPT(Z, PER), Z), CPT(Z, SE), CPT(Z, GE)]),
    "sum at the root": (gp.Plus(gp.Plus(LIN, CPT(PER, SE)), GE), 1, [LIN, CPT(PER, Z), CPT(Z, SE), GE]),
}


@pytest.mark.parametrize("name", list(HAND))
def test_counts_and_order_of_hand_written_trees(lib, name):
    tree, split, want = HAND[name]
    got = _lib.kernel_terms(prog(tree), split)
    same_programs(got, [prog(w) for w in want])
    # the second parameter of a windowed term's ChangePoint is the tree's own
    assert [str(gp.from_program(o, p)) for o, p, _ in got] == [str(w) for w in want]


# ---- NGP_ERR_TOO_LARGE ------------------------------------------------------------------------------
def raw_terms(lib, p, split, max_terms, ops_cap, par_cap, n_index=64):
    ka = KernelArray([p])
    cnt = C.c_int32(-7)
    idx = [np.zeros(n_index, np.int32) for _ in range(4)]
    ops, par = np.zeros(max(ops_cap, 1), np.int32), np.zeros(max(par_cap, 1))
    st = lib.ngp_kernel_terms(C.byref(ka.arr[0]), split, max_terms, C.byref(cnt), *(iptr(a) for a in idx),
                              iptr(ops), ops_cap, dptr(par), par_cap)
    return st, int(cnt.value)


def test_too_large_returns_with_the_count_set(lib):
    p = prog(HAND["(a+b)(c+d)"][0])            # 4 terms of 3 ops; 5 + 4 + 5 + 4 = 18 parameters
    assert raw_terms(lib, p, 2, 4, 12, 18) == (0, 4)
    assert raw_terms(lib, p, 2, 3, 12, 18) == (NGP_ERR_TOO_LARGE, 4)      # max_terms exceeded
    assert raw_terms(lib, p, 2, 4, 11, 18) == (NGP_ERR_TOO_LARGE, 4)      # ops short by one
    assert raw_terms(lib, p, 2, 4, 12, 17) == (NGP_ERR_TOO_LARGE, 4)      # parameters short by one
    # the count alone: NULL buffers
    ka = KernelArray([p])
    cnt = C.c_int32(-7)
    assert lib.ngp_kernel_terms(C.byref(ka.arr[0]), 2, 100, C.byref(cnt), None, None, None, None, None, 0,
                                None, 0) == 0 and cnt.value == 4
    assert lib.ngp_kernel_terms(C.byref(ka.arr[0]), 2, 3, C.byref(cnt), None, None, None, None, None, 0,
                                None, 0) == NGP_ERR_TOO_LARGE and cnt.value == 4
    # a term past NGP_MAX_OPS: a product of 33 leaves (65 ops) beside a leaf — two terms, the first
    # is no valid program
    chain = SE
    for _ in range(32):
        chain = gp.Times(chain, SE)
    big = prog(gp.Plus(chain, PER))
    assert len(big[0]) == NGP_MAX_OPS + 3
    assert raw_terms(lib, big, 0, 8, 200, 200) == (NGP_ERR_TOO_LARGE, 2)
    # ... while a long SUM has terms that fit
    total = SE
    for _ in range(40):
        total = gp.Plus(total, SE)
    st, cnt_ = raw_terms(lib, prog(total), 0, 64, 200, 200)
    assert (st, cnt_) == (0, 41)
    # a product of 30 sums: 2^30 terms of 59 ops each, each a valid program.  Known to be more
    # than the buffers hold before a single term is built (nothing near 2^30 terms is allocated)
    wide = gp.Plus(SE, SE)
    for _ in range(29):
        wide = gp.Times(wide, gp.Plus(SE, SE))
    assert raw_terms(lib, prog(wide), 2, 2**31 - 1, 4096, 4096) == (NGP_ERR_TOO_LARGE, 2**30)
    # a term past NGP_MAX_OPS is said with the count alone, too
    ka = KernelArray([big])
    assert lib.ngp_kernel_terms(C.byref(ka.arr[0]), 0, 8, C.byref(cnt), None, None, None, None, None, 0,
                                None, 0) == NGP_ERR_TOO_LARGE and cnt.value == 2


def test_argument_errors(lib):
    p = prog(LIN)
    ka = KernelArray([p])
    cnt = C.c_int32(0)
    call = lambda k, split, mt, c: lib.ngp_kernel_terms(k, split, mt, c, None, None, None, None, None, 0, None, 0)
    assert call(None, 0, 1, C.byref(cnt)) == NGP_ERR_ARG
    assert call(C.byref(ka.arr[0]), 0, 1, None) == NGP_ERR_ARG
    assert call(C.byref(ka.arr[0]), 4, 1, C.byref(cnt)) == NGP_ERR_ARG
    assert call(C.byref(ka.arr[0]), -1, 1, C.byref(cnt)) == NGP_ERR_ARG
    assert call(C.byref(ka.arr[0]), 0, -1, C.byref(cnt)) == NGP_ERR_ARG
    bad = KernelArray([(np.array([6], np.int32), np.zeros(0), 0.0)])      # a Plus without operands
    assert call(C.byref(bad.arr[0]), 0, 1, C.byref(cnt)) == NGP_ERR_PROGRAM
    # ngp_factor_components_nowcast: the only argument error that can be reached without a factor
    one, buf = np.ones(1, np.int32), np.zeros(4)
    st = lib.ngp_factor_components_nowcast(None, 1, dptr(buf), 1, dptr(buf), iptr(one), ka.arr, 1, dptr(buf),
                                           None, dptr(buf), None, None, None)
    assert st == NGP_ERR_ARG


# ---- the long double restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("name,d,D", [("CP(a+b, c)", 3, 4), ("(a+b)(c+d)", 1, 1), ("CP under Times", 3, 2),
                                      ("sum at the root", 0, 1)])
def test_the_reference_satisfies_the_three_identities(name, d, D):
    """per scenario sum_c mu_c,s = mu_s, sum_cc' Sigma_cc' = Sigma, logml agrees (the noise-free nowcast
    predictive of tests/hp_reference.py), every Sigma_cc positive semi-definite — in long double"""
    tree, split, _ = HAND[name]
    p = prog(tree)
    comps = cnr.terms(p, split)
    n, m = 45, 6
    rng = np.random.default_rng(3)
    t = np.sort(rng.uniform(0, 1, n))
    y = np.sin(7 * t) + 0.1 * rng.standard_normal(n)
    t_add = 1.0 + 0.01 * np.arange(1, d + 1)
    y_add = rng.standard_normal((D, d)) if d else np.zeros((1, 0))
    t_new = 1.05 + 0.03 * np.arange(1, m + 1)
    r = cnr.evaluate(p, comps, t, y, t_add, y_add, t_new)
    full = hr.nowcast(p, t, y, t_add, y_add, t_new, noise_on_new=False)
    assert r.info == 0 and full.info == 0
    C_ = len(comps)
    bound = 1e3 * hr.EPS_LD * r.cond
    assert r.mu.shape == (C_, D, m)
    assert float(np.max(np.abs(r.mu.sum(axis=0) - full.mu)) / np.max(np.abs(full.mu))) < bound
    sg_sum = r.sigma.reshape(C_, m, C_, m).sum(axis=(0, 2))
    assert float(np.max(np.abs(sg_sum - full.sigma)) / np.max(np.abs(full.sigma))) < bound
    assert float(np.max(np.abs((r.logml_full - full.logml_full) / full.logml_full))) < bound
    for c in range(C_):
        ev = np.linalg.eigvalsh(r.sigma[c * m:(c + 1) * m, c * m:(c + 1) * m].astype(float))
        assert ev[0] > -1e-12 * max(ev[-1], 1e-300)
    assert np.array_equal(r.sigma, r.sigma.T)


# ---- the Python layers -----------------------------------------------------------------------------
class _Stub:
    """what decompose reads of a model"""

    def __init__(self, trees, n=130):
        self._p, self._n = [prog(t) for t in trees], n

    def programs(self):
        return self._p

    def _obs(self):
        return np.zeros(self._n), np.zeros(self._n)


def test_decompose_kinds_labels_and_the_split_used(lib):
    cp = CPT(gp.Plus(LIN, PER), SE)
    prod = gp.Times(gp.Plus(LIN, CON), gp.Plus(PER, SE))
    stub = _Stub([cp, prod, gp.Plus(LIN, PER)])
    plus = autogp.decompose(stub)
    assert [len(ps) for ps in plus] == [1, 1, 2] and all(c.split == "plus" for ps in plus for c in ps)
    assert plus[0][0].label == str(cp)                                    # the default is unchanged
    chp = autogp.decompose(stub, "changepoint")
    assert [[c.kind for c in ps] for ps in chp] == [["trend", "seasonal", "other"], ["trend"], ["trend", "seasonal"]]
    assert chp[0][0].label == f"{LIN} [before 0.5]" and chp[0][2].label == f"{SE} [after 0.5]"
    assert str(chp[0][2].tree) == str(CPT(Z, SE))
    assert all(c.split == "changepoint" for ps in chp for c in ps)
    prd = autogp.decompose(stub, "products")
    assert [[c.kind for c in ps] for ps in prd][1] == ["trend", "trend", "seasonal", "other"]
    assert prd[1][3].label == f"Times({CON}, {SE})" and prd[1][0].split == "products"
    nested = autogp.decompose(_Stub([gp.Times(CPT(LIN, PER), SE)]), "products")[0]
    assert [c.label for c in nested] == [f"Times({LIN} [before 0.5], {SE})", f"Times({PER} [after 0.5], {SE})"]
    with pytest.raises(ValueError):
        autogp.decompose(stub, "sums")


def test_a_particle_with_too_many_terms_falls_back_to_the_next_weaker_split(lib):
    cp = CPT(gp.Plus(LIN, PER), SE)                                       # 3 windowed terms
    prod = gp.Times(gp.Plus(gp.Plus(LIN, CON), PER), gp.Plus(PER, SE))    # 6 products
    both = gp.Plus(CPT(LIN, SE), gp.Times(gp.Plus(LIN, CON), gp.Plus(PER, SE)))   # 2 | 3 | 6
    stub = _Stub([cp, prod, both])
    got = autogp.decompose(stub, "products", max_terms=5)
    assert [(len(ps), ps[0].split) for ps in got] == [(3, "products"), (1, "changepoint"), (3, "changepoint")]
    got = autogp.decompose(stub, "products", max_terms=2)
    assert [(len(ps), ps[0].split) for ps in got] == [(1, "plus"), (1, "changepoint"), (2, "plus")]
    # the default limit: what leaves a row for one forecast date beside the factor, 192 - (n mod 64) - 2
    wide = gp.Times(balanced_sum(12), balanced_sum(12))                   # 144 products
    assert len(autogp.decompose(_Stub([wide], n=128), "products")[0]) == 144
    one = autogp.decompose(_Stub([wide], n=128 + 50), "products")[0]       # 140 rows are left
    assert len(one) == 1 and one[0].split == "changepoint"


def balanced_sum(k):
    leaves = [gp.SquaredExponential(0.1 + 0.01 * i, 0.3) for i in range(k)]
    while len(leaves) > 1:
        leaves = [gp.Plus(a, b) for a, b in zip(leaves[::2], leaves[1::2])] + (leaves[-1:] if len(leaves) % 2 else [])
    return leaves[0]


def test_component_blocks_count_the_appended_points():
    assert autogp.component_blocks(130, 3, 63) is None                    # 2 + 1 + 189 = 192
    assert autogp.component_blocks(130, 3, 63, 2) == [(0, 62), (62, 63)]  # 2 + 2 + 1 + 186 <= 192
    assert autogp.component_blocks(130, 3, 62, 2) is None


def test_the_cpu_engine_has_no_resident_factor():
    import datetime as dt

    from tests.engine_oracle import OracleEngine
    n = 30
    ds = [dt.date(2020, 1, 5) + dt.timedelta(days=7 * i) for i in range(n)]
    y = 10.0 + np.sin(np.arange(n) / 3.0)
    model = autogp.GPModel(ds, y, n_particles=2, seed=3, engine=OracleEngine())
    new = [ds[-1] + dt.timedelta(days=7 * (i + 1)) for i in range(4)]
    with pytest.raises(RuntimeError, match="needs the engine's resident factor"):
        autogp.predict_components(model, new[2:])
    nows = [nc.TData(new[:2], [10.0, 10.5], transformation=lambda v: v)]
    with pytest.raises(RuntimeError, match="needs the engine's resident factor"):
        nc.forecast_components_with_nowcasts(model, nows, new[2:])


# ---- the host code under sanitizers (a stand-alone program on the mock runtime) -------------------------
@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
@pytest.mark.parametrize("tag,flags,env", [
    ("tsan", ["-fsanitize=thread"], {"TSAN_OPTIONS": "halt_on_error=0 report_signal_unsafe=0"}),
    ("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
     {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"}),
])
def test_components_nowcast_under_sanitizers(tmp_path, tag, flags, env):
    exe = build(str(tmp_path), flags, tag, "components_nowcast_stress")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env={**os.environ, **env})
    report = out.stdout[-3000:] + out.stderr[-6000:]
    assert "ThreadSanitizer" not in out.stderr, report
    assert "AddressSanitizer" not in out.stderr and "LeakSanitizer" not in out.stderr, report
    assert "runtime error" not in out.stderr, report
    assert out.returncode == 0, report
    assert "0 failures" in out.stdout, report

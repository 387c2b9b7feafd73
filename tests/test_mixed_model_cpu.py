"""tests/mixed_model.py and the cases of tests/mixed_cases.py, judged on the host: the cases must be
able to fail.  For the accuracy cases the emulated factorisation that follows the rule stays within
TOL_MIXED / 100 of the fp64 log det (relative to logml) and the one with every fat-step product in
fp32 is off by more than 100 TOL_MIXED on every sensitive item (noise <= 1e-5; measured here:
1.2e-4 .. 8.5e-3); for the counting cases the model's fp32 share lies strictly inside (0, 1) and
next to no product sits on the rule's threshold, so a device count can be compared exactly."""
import numpy as np
import pytest

from nowcastautogp_amd._abi import NGP_PREC_MIXED, default_spec
from oracle import oracle_np
from tests import mixed_cases as mc
from tests import mixed_model as mm


def test_the_restated_constants_are_the_librarys():
    sp = default_spec(NGP_PREC_MIXED)
    assert (sp.mixed_tau, sp.jitter) == (mc.MIXED_TAU, mc.JITTER)
    assert mc.TOL_MIXED == 1e-6


def test_round_up_to_fp32():
    x = np.array([0.0, 1.0, 1.0 + 2.0 ** -30, 0.1, 3e-39, 1e-300])
    f = mm.f32_up(x)
    assert f.dtype == np.float32 and (f.astype(np.float64) >= x).all()
    assert (np.nextafter(f, np.float32(-np.inf)).astype(np.float64)[1:] < x[1:]).all()
    assert f[1] == 1.0 and f[2] == np.nextafter(np.float32(1), np.float32(2))


def test_schedule():
    """col_pair_offset / col_step of ngp_plan.h and the fat kernel's tile pairing"""
    assert [mm.col_step(4, j) for j in range(4)] == ["fat", "thin", "fat", "thin"]
    assert [mm.col_step(3, j) for j in range(3)] == ["full", "fat", "thin"]
    assert [mm.col_step(2, j) for j in range(2)] == ["fat", "thin"]
    assert mm.col_step(1, 0) == "full"
    # nb0 = 7, one aux tile, pair (3, 4): row tiles 4, 5, 6 and aux tile 7 in two workgroups
    assert mm.fat_workgroups(7, 1, 3) == [(4, 5, 4), (6, 7, 4)]
    # two aux tiles: five tiles, the last workgroup has one (its second index repeats, weight 2)
    assert mm.fat_workgroups(7, 2, 3) == [(4, 5, 4), (6, 7, 4), (8, 8, 2)]
    assert mm.fat_workgroups(2, 1, 0) == [(1, 2, 4)]
    # the main row tiles of a fat step are always odd in number
    assert all((nb0 - 1 - j) % 2 == 1 for nb0 in range(2, 130) for j in range(nb0) if mm.col_step(nb0, j) == "fat")
    assert mm.mixed_eligible(129) and not mm.mixed_eligible(130) and not mm.mixed_eligible(1)


def test_aux_rows_follow_the_jobs_order():
    """tail | forecast dates | y', the rows of tests/blocked_model.py's X"""
    progs, _, t, y, t_new = mc.batch(**mc.COUNT_CASES["n497_aux150"])
    n0, X = mm.aux_rows(progs[0], t, y, t_new)
    assert n0 == 448 and X.shape == (49 + 100 + 1, 448)
    assert np.array_equal(X[:49], oracle_np.cov(progs[0], t[448:], t[:448]))
    assert np.array_equal(X[49:149], oracle_np.cov(progs[0], t_new, t[:448])) and np.array_equal(X[149], y[:448])
    L, W = mm.factor_and_aux(progs[0], t, y, t_new)
    assert W.shape == (192, 448) and not W[150:].any()
    assert np.allclose(W[:150] @ L.T, X, rtol=0, atol=1e-9 * np.abs(X).max())


@pytest.mark.parametrize("name", list(mc.COUNT_ZERO))
def test_the_shortest_series_count_no_fp32_product(name):
    for m in mc.model(mc.COUNT_ZERO[name]):
        assert m["n32"] == 0 and m["borderline"] == 0
        assert (m["n64"] == 0) == (mc.COUNT_ZERO[name]["n"] == 128)


@pytest.mark.parametrize("name", list(mc.COUNT_CASES))
def test_counting_cases_are_mixed_and_off_the_threshold(name):
    kw = mc.COUNT_CASES[name]
    kinds = mc.batch(**kw)[1]
    for b, (m, kind) in enumerate(zip(mc.model(kw), kinds)):
        tot = m["n32"] + m["n64"]
        print(name, b, kind, "frac %.4f" % m["frac"], "of", tot, "borderline", m["borderline"])
        assert tot > 0
        assert m["borderline"] <= mc.BORDER_SHARE * tot, (name, b)
        if kind == "fp64":
            assert m["frac"] == 0.0
        elif kind == "fp32":
            assert m["frac"] > 0.99
        else:
            assert mc.FRAC_LO <= m["frac"] <= mc.FRAC_HI, (name, b, kind, m["frac"])


def test_the_counts_tell_wrong_maxima_from_right_ones():
    """the mistakes of the issue (second tile of a pair ignored, maxima off by 4) move the count of
    every mixed item of the 34-column case by far more than the allowance"""
    kw = mc.COUNT_CASES["n2176_B17"]
    progs, kinds, t, y, t_new = mc.batch(**kw)
    for mistake in (dict(second_tile=False), dict(scale=4.0), dict(scale=0.25)):
        for p, m, kind in zip(progs, mc.model(kw), kinds):
            n32 = mm.counts(m["tm"], mm.limit(p[2], mc.MIXED_TAU, mc.JITTER), 34, 1, **mistake)[0]
            if kind not in ("fp64", "fp32"):
                assert abs(n32 - m["n32"]) > 10 * (m["borderline"] + 0.5), (mistake, kind)


def _acc(name):
    kw = mc.ACC_CASES[name]
    progs, kinds, t, y, t_new = mc.batch(**kw)
    n0 = (t.size // mm.NB) * mm.NB
    for b, p in enumerate(progs):
        K = oracle_np.cov(p, t[:n0], t[:n0], True)
        ld = 2.0 * np.log(np.diag(np.linalg.cholesky(K))).sum()
        lm = oracle_np.logml(p, t, y)[0]
        cond = np.linalg.cond(oracle_np.cov(p, t, t, True))
        yield b, p, kinds[b], ld, lm, cond, (t, y, t_new)


@pytest.mark.parametrize("name", list(mc.ACC_CASES))
def test_accuracy_cases_can_fail(name):
    for b, p, kind, ld, lm, cond, (t, y, t_new) in _acc(name):
        assert 1e-6 <= p[2] <= 1e-4 and cond <= 1e8, (name, b, cond)
        rule, n32, n64 = mm.emulate(p, t, y, t_new, mc.MIXED_TAU, mc.JITTER)
        e_rule = 0.5 * abs(rule - ld) / abs(lm)
        try:
            every = mm.emulate(p, t, y, t_new, mc.MIXED_TAU, mc.JITTER, every=True)[0]
            e_every = 0.5 * abs(every - ld) / abs(lm)
        except np.linalg.LinAlgError:      # a pivot went negative: as wrong as it gets
            e_every = np.inf
        print(name, b, kind, "noise %g cond %.1e rule %.1e every-fp32 %.1e (%.0f x TOL)" %
              (p[2], cond, e_rule, e_every, e_every / mc.TOL_MIXED))
        assert e_rule <= mc.TOL_MIXED / 100, (name, b, e_rule)
        assert (p[2] <= mc.SENSITIVE_NOISE) == (kind != "se")
        if p[2] <= mc.SENSITIVE_NOISE:
            assert e_every > 100 * mc.TOL_MIXED, (name, b, e_every)


def test_emulation_counts_what_the_model_counts():
    """emulate classifies from the maxima of its own factor, the model from numpy's: same counts
    wherever nothing is borderline"""
    kw = mc.COUNT_CASES["n448_B3"]
    progs, _, t, y, t_new = mc.batch(**kw)
    for p, m in zip(progs, mc.model(kw)):
        _, n32, n64 = mm.emulate(p, t, y, t_new, mc.MIXED_TAU, mc.JITTER)
        assert (n32, n64) == (m["n32"], m["n64"])

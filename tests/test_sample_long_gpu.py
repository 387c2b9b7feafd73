"""ngp_factor_sample_long on the device: paths of a horizon beyond the short sampler's 192 dates,
drawn from the sigma the long query leaves on the device.

The contract is ``tests/sampler_reference.py`` (long double) fed with the moments
``Factor.predict_long`` returns on the device for the same query: the component of every path
exactly, every coordinate within ``tests.util.tol(4 r64_long, cond(sigma_k))`` under the measure of
tests/test_sampler_gpu.py, |(x - mu_k)_i - (L z)_i| / (sqrt(sigma_ii) max(1, |z|_inf)).  r64_long is
the fp64 oracle's own worst error under that measure on these cases, found on the CPU by
tests/test_sample_long_cpu.py; the factor 4 is the margin tests/test_sampler_gpu.py grants for
summation order and the last bits of log, cos and sin.  Cases, weights and seeds:
tests/sample_long_cases.py.
"""
import numpy as np
import pytest

from nowcastautogp_amd import _lib, autogp
from nowcastautogp_amd import nowcast as nc
from tests import mirror_contracts as mc
from tests import sample_long_cases as lc
from tests import sampler_cases as sc
from tests import sampler_reference as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    c = _lib.Context(0)
    c.set_combining(False)
    yield c
    c.close()


_FACTORS = {}


def factor(ctx, n, programs=None):
    key = (n, None if programs is None else id(programs))
    if key not in _FACTORS:
        t, y = lc.series(n)
        _FACTORS[key] = ctx.factor(lc.PROGRAMS if programs is None else programs, t, y)
    return _FACTORS[key]


def ask(ctx, case, noise_on_new=True, draws=None, w=None, **kw):
    n, d, D, m, dr = case
    _, _, t_add, y_add, t_new = lc.query(n, d, D, m)
    return factor(ctx, n).sample_long(t_new, lc.weights(D) if w is None else w, dr if draws is None else draws,
                                      lc.seed_of(case), t_add, y_add, noise_on_new, **kw)


def device_moments(ctx, case, noise_on_new=True):
    n, d, D, m, _ = case
    _, _, t_add, y_add, t_new = lc.query(n, d, D, m)
    mu, var, sg, info = factor(ctx, n).predict_long(t_new, t_add, y_add, noise_on_new)
    assert not info.any()
    return mu, var, sg


def judge_case(ctx, case, noise_on_new=True, w=None):
    n, d, D, m, draws = case
    w = lc.weights(D) if w is None else w
    mu, var, sg = device_moments(ctx, case, noise_on_new)
    ref = sr.sample(w, mu, sg, draws, lc.seed_of(case))
    assert ref.margin.min() > sr.PICK_MARGIN
    assert not ref.info[w.max(axis=0) > 0].any()
    out, comp, info, cinfo, mu_s, var_s = ask(ctx, case, noise_on_new, w=w, want_moments=True)
    assert out.shape == (D, draws, m) and comp.shape == (D, draws)
    assert not info.any() and not cinfo.any()
    assert np.array_equal(mu_s, mu) and np.array_equal(var_s, var)      # the long query's bits
    worst = sc.judge(f"sample_long vs reference {case}", out, comp, ref, mu, sg, floor=lc.FLOOR)
    print(f"sample_long {case} noise={noise_on_new}: worst {worst:.3e} (floor {lc.FLOOR:.3e})")
    return out, comp, mu, sg


@pytest.mark.parametrize("case", lc.TABLE, ids=str)
def test_against_the_contract(ctx, case):
    n, d, D, m, draws = case
    out, comp, mu, sg = judge_case(ctx, case)
    counts = np.bincount(comp.ravel(), minlength=lc.P)
    assert counts[1] == 0
    if D == 3 and draws == 70:
        assert 15 <= counts[2] <= 17 and counts[0] > 2 * 64
    if m <= 192:
        # the short sampler on the same device moments: same picks, same tolerance
        x, comp_s, info_s = ctx.mixture_sample(lc.weights(D), mu, sg, draws, lc.seed_of(case))
        assert not info_s.any() and np.array_equal(comp_s, comp)
        ref = sr.sample(lc.weights(D), mu, sg, draws, lc.seed_of(case))
        sc.judge(f"short sampler on the long query's moments {case}", x, comp_s, ref, mu, sg, floor=lc.FLOOR)


def test_without_noise_on_the_dates(ctx):
    """all the weight on particle 0, the one whose noise-free sigma the reference factorises
    (tests/sample_long_cases.py); the others are not factorised and report nothing"""
    D = lc.NOISE_FREE[2]
    judge_case(ctx, lc.NOISE_FREE, noise_on_new=False, w=lc.weights_noise_free(D))


def test_fewer_draws_are_the_first_of_more_and_calls_repeat(ctx):
    case = (191, 3, 3, 300, 70)
    a = ask(ctx, case)
    b = ask(ctx, case)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    few = ask(ctx, case, draws=17)
    assert np.array_equal(few[0], a[0][:, :17]) and np.array_equal(few[1], a[1][:, :17])
    assert np.array_equal(few[2], a[2]) and np.array_equal(few[3], a[3])


@pytest.mark.parametrize("case", [(191, 3, 3, 300, 70), (64, 0, 1, 129, 70)], ids=str)
def test_particles_do_not_depend_on_their_neighbours(ctx, case):
    """P = 3 in one chunk against three single-particle factors asked with the same seed: the picks
    are the stream's, so the one-hot call draws path (s, d) from its only particle with the same
    normals — on the paths the particle owns in the joint call the bits are equal."""
    n, d, D, m, draws = case
    t, y, t_add, y_add, t_new = lc.query(n, d, D, m)
    out, comp, _, _ = ask(ctx, case)
    for k in (0, 2):
        single = ctx.factor([lc.PROGRAMS[k]], t, y)
        o1, c1, i1, ci1 = single.sample_long(t_new, np.ones((D, 1)), draws, lc.seed_of(case), t_add, y_add)
        single.close()
        assert not i1.any() and not ci1.any() and not c1.any()
        own = comp == k
        assert own.any() and np.array_equal(o1[own], out[own])


def test_a_failed_particle_keeps_its_failure_to_itself(ctx):
    """the recipe of test_predict_long_gpu.test_the_conditioning_block_reports_its_pivot: the
    appended point of particle 1 repeats the last training date under a negative noise, so its
    conditioning block reports a pivot; the paths picked from it are NaN, the others finite"""
    from tests import value_cases as vc
    from tests.test_pivot_info_gpu import failing_case, reference_k
    n, d, m, draws = 130, 3, 200, 35
    k_ref = reference_k("duplicate", n, n + 1, d)
    bad, t, t_add = failing_case("duplicate", n, n + 1, d)
    _, y = vc.series(n, True, seed=41)
    good = list(vc._items(31, vc.SIZES, 3, n, 5, 7, True))
    y_add = np.random.default_rng(5).standard_normal((2, d))
    t_new = t[-1] + (d + 1 + np.arange(m)) / (n - 1)
    w = np.array([[0.4, 0.3, 0.3], [0.2, 0.5, 0.3]])
    f = ctx.factor([good[0], bad, good[2]], t, y)
    try:
        out, comp, info, cinfo = f.sample_long(t_new, w, draws, 12345, t_add, y_add)
    finally:
        f.close()
    assert info[1] == k_ref and info[0] == 0 and info[2] == 0 and not cinfo.any()
    lost = comp == 1
    assert lost.any() and (~lost).any()
    assert np.isnan(out[lost]).all() and np.isfinite(out[~lost]).all()


def test_a_particle_without_weight_is_not_factorised(ctx):
    case = (64, 3, 3, 65, 70)
    out, comp, info, cinfo = ask(ctx, case)
    assert cinfo[1] == 0 and not (comp == 1).any() and np.isfinite(out).all()


# ---- the mirror -------------------------------------------------------------------------------------
class Counter:
    def __init__(self):
        self.calls = []


def counted(monkeypatch):
    cnt = Counter()
    for name in ("sample_long", "predict_long", "nowcast"):
        orig = getattr(_lib.Factor, name)

        def wrap(self, *a, _orig=orig, _name=name, **k):
            size = np.size(a[0]) if _name != "nowcast" else np.size(a[2])
            cnt.calls.append((_name, int(size)))
            return _orig(self, *a, **k)
        monkeypatch.setattr(_lib.Factor, name, wrap)
    return cnt


def scenarios():
    ident = lambda v: v  # noqa: E731
    return [nc.TData(mc.days(20, 22), v, transformation=ident) for v in ([111.0, 112.0], [109.0, 113.0])]


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge
    ge.build()
    e = autogp.HipEngine(0)
    yield e
    e.ctx.close()


def test_mirror_draws_a_long_horizon_in_one_device_call(eng, monkeypatch):
    model = mc.fitted(eng, seed=5, n_particles=3)
    dates = mc.days(22, 322)
    cnt = counted(monkeypatch)
    x = nc.forecast_with_nowcasts(model.clone(), scenarios(), dates, 3, device_paths=True)
    assert cnt.calls == [("nowcast", 0), ("sample_long", 300)]
    assert x.shape == (300, 6) and np.isfinite(x).all()
    targets = [(kind, 0, 299) for kind in sorted(autogp.TARGET_KINDS)[:2]]
    tg = nc.forecast_targets_with_nowcasts(model.clone(), scenarios(), dates, targets, 3, device_paths=True,
                                           want_values=True)
    tgs = autogp._target_tuples(targets, 300)
    ref = autogp.path_functionals(np.ascontiguousarray(x.T), tgs)
    for i in range(len(tgs)):
        np.testing.assert_array_equal(tg.values(i), ref[i])
    cnt.calls.clear()
    nc.forecast_with_nowcasts(model.clone(), scenarios(), dates, 3)      # the default: as before
    assert cnt.calls == [("nowcast", 0), ("predict_long", 300)]

"""ngp_mixture_sample / ngp_mixture_sample_indep (small_chol_kernel + mixture_sample_kernel) against
the long-double reference of tests/sampler_reference.py, draw by draw and coordinate by coordinate,
on the case table of tests/sampler_cases.py: every loop and index boundary of the two kernels, the
weight rows that reach the fallback, real predictive covariances (cond up to 2.4e6) and matrices
made indefinite at a chosen row.

Judgement (sampler_cases.judge): comp exactly; x_i - mu_{k,i} against the reference's (L z)_i on
the scale sqrt(sigma_ii) max(1, |z|_inf), within tests.util.tol(FLOOR, cond(sigma_k)).  FLOOR is
4 r64, r64 = 2.82e-12 the fp64 oracle's worst error under the same measure, found on the CPU by
tests/test_sampler_reference_cpu.py — which also asserts that no case has anything to skip and
that the judgement rejects eight deliberately wrong samplers.  Unconditionally: a repeated call
gives the same bits, seed + 1 gives other draws, and no draw of a component with info == 0 is NaN.
"""
import numpy as np
import pytest

from nowcastautogp_amd import _lib
from tests import sampler_cases as sc

pytestmark = pytest.mark.gpu

NGP_ERR_TOO_LARGE = -3
WORST = {}           # case -> worst scaled error of the device, against FLOOR (printed at the end)


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    c = _lib.Context(0)
    yield c
    c.close()
    if WORST:
        name = max(WORST, key=WORST.get)
        print(f"\nsampler: worst scaled error of the device {WORST[name]:.3e} at {name} "
              f"(floor {sc.FLOOR:.3e}, r64 {sc.R64:.3e}) over {len(WORST)} runs")


def run(ctx, c, indep, seed_shift=0, **kw):
    if indep:
        w, mu, sigma, seeds = c.indep()
        return ctx.mixture_sample_indep(w, mu, sigma, c.draws, [s + seed_shift for s in seeds], **kw)
    return ctx.mixture_sample(c.w, c.mu, c.sigma, c.draws, c.seed + seed_shift, **kw)


def check_case(ctx, name, indep):
    c, ref = sc.cases()[name], sc.reference(name, indep)
    mu, sigma = (c.indep()[1:3] if indep else (c.mu, c.sigma))
    x, comp, info = run(ctx, c, indep)
    assert np.array_equal(info, ref.info), (name, indep, info, ref.info)
    what = f"sampler ({'independent' if indep else 'shared'}) vs reference"
    WORST[(name, indep)] = sc.judge(what, x, comp, ref, mu, sigma)
    again, comp2, info2 = run(ctx, c, indep)
    assert np.array_equal(x, again, equal_nan=True) and np.array_equal(comp, comp2) and np.array_equal(info, info2)
    other, _, _ = run(ctx, c, indep, seed_shift=1)
    assert not np.array_equal(x, other, equal_nan=True), (name, indep)
    return x, comp, info


@pytest.mark.parametrize("name", sc.NAMES)
def test_shared_form_against_the_reference(ctx, name):
    check_case(ctx, name, False)


@pytest.mark.parametrize("name", sc.INDEP_NAMES)
def test_independent_form_against_the_reference(ctx, name):
    """judged against the reference's independent form directly (test_lockstep_gpu.py compares it
    with S separate device calls)"""
    check_case(ctx, name, True)


@pytest.mark.parametrize("indep", [False, True], ids=["shared", "independent"])
def test_the_horizon_limit(ctx, indep):
    """m = NGP_MAX_AUX = 192 is a case of the table; 193 is NGP_ERR_TOO_LARGE in both forms"""
    m = 193
    w, mu, sigma = np.full((2, 2), 0.5), np.zeros((2, 2, m)), np.stack([np.eye(m)] * 2)
    with pytest.raises(_lib.NgpError) as e:
        if indep:
            ctx.mixture_sample_indep(w, mu, np.stack([sigma] * 2), 3, [1, 2])
        else:
            ctx.mixture_sample(w, mu, sigma, 3, 1)
    assert e.value.status == NGP_ERR_TOO_LARGE


@pytest.mark.parametrize("indep", [False, True], ids=["shared", "independent"])
@pytest.mark.parametrize("name", ["P5_S3", "pivots_m64"])
def test_optional_outputs_may_be_null(ctx, name, indep):
    """comp = NULL, info = NULL, both: the draws are the bits of the call that asks for them"""
    c = sc.cases()[name]
    x, comp, info = run(ctx, c, indep)
    for want_comp, want_info in ((False, True), (True, False), (False, False)):
        x2, comp2, info2 = run(ctx, c, indep, want_comp=want_comp, want_info=want_info)
        assert np.array_equal(x, x2, equal_nan=True)
        assert (comp2 is None) if not want_comp else np.array_equal(comp, comp2)
        assert (info2 is None) if not want_info else np.array_equal(info, info2)


@pytest.mark.parametrize("m", [64, 192])
def test_pivot_reports_equal_the_long_double_first_failing_row(ctx, m):
    """real predictive covariances with c e_k e_k' subtracted at k = 1, 17, 18, m (components 1, 2,
    4, 5): info is the long-double first failing row — the margins of the reference's own pivots
    and that both healthy components are drawn from are asserted in test_sampler_reference_cpu.py —
    healthy components report 0 and their draws meet the judgement (check_case); the independent
    form reports [S x P]"""
    name = f"pivots_m{m}"
    c = sc.cases()[name]
    _, _, info = check_case(ctx, name, False)
    want = np.zeros(6, np.int32)
    for k_comp, k in c.bad:
        want[k_comp] = k
    assert np.array_equal(info, want), (info, want)
    _, _, info_i = check_case(ctx, name, True)
    assert info_i.shape == (c.shape[1], 6)
    for s in range(c.shape[1]):
        assert np.array_equal(info_i[s], np.roll(want, -s)), (s, info_i[s])

"""NGP_PREC_MIXED: the fp32 / fp64 choice of every fat-step tile product against the host model
(tests/mixed_model.py), on the cases tests/test_mixed_model_cpu.py has shown able to fail.

Counting: ``frac_f32`` of every item against the model's weighted counts, allowing the model's
borderline products (at most 0.5 % of an item's, a condition on the cases) plus half a product.  The
tile maxima (four epilogues write them), the pairing of tiles into workgroups, both words of the
ballot masks, the weights of a workgroup with one tile and the per-item counters under the
re-ranked dispatch order all have to be right for the counts to agree.

Accuracy: items whose fat-step products are O(1) against pivots of the size of the noise.  With the
default spec they must meet TOL_MIXED against the long-double reference with info == 0; forced to
fp32 everywhere (mixed_tau = 1e30, no refinement) the items with noise <= 1e-5 must miss it tenfold,
otherwise the case has stopped testing the rule.  Measured on an MI355X, logml error of the forced
run over TOL_MIXED (items with noise 1e-5, 1e-6, 3e-6): n = 256: 73, 486, 37; n = 448: 3,042, 5,441,
434; n = 521: 989, 3,048, 1,856 (the host emulation gave 120 .. 8,500).  Under the rule the same
items are within 4.7e-12 (logml), 1.2e-11 (mean) and 1.4e-10 (variances) of long double.

The two long series (64 * 67 and 8,319 points) are beyond the long-double reference: they are
judged against oracle_np (fp64 LAPACK) and the device's own fp64 job, at TOL_MIXED.
"""
import numpy as np
import pytest

from nowcastautogp_amd import _lib
from nowcastautogp_amd._abi import NGP_PREC_MIXED, default_spec
from oracle import oracle_np
from tests import hp_reference as hp
from tests import mixed_cases as mc
from tests.util import nerr

pytestmark = pytest.mark.gpu

TOL_MIXED = mc.TOL_MIXED


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    c = _lib.Context(0)
    c.set_short_series_path(False)     # n0 <= 256 on the column sweep whatever the precision
    yield c
    c.close()


def _run(ctx, spec, progs, t, y, t_new):
    ctx.set_spec(spec)
    try:
        job = ctx.stage_predict(progs, t, y, t_new)
        job.run()
        out = job.fetch()
        out.update(job.mixed_stats())
        job.close()
    finally:
        ctx.set_spec(default_spec())
    return out


_ORACLE = {}


def oracle(name):
    """oracle_np's predictive of every item of a large case, once per module"""
    if name not in _ORACLE:
        progs, _, t, y, t_new = mc.batch(**mc.COUNT_CASES[name])
        _ORACLE[name] = [oracle_np.predict(p, t, y, t_new) for p in progs]
    return _ORACLE[name]


def check_counts(name, kw, frac):
    for b, m in enumerate(mc.model(kw)):
        err, allowed = mc.count_error(frac[b], m)
        print(name, b, "frac_f32 %.6f model %.6f of %d, off by %.3f (allowed %.1f)" %
              (frac[b], m["frac"], m["n32"] + m["n64"], err, allowed))
        assert err <= allowed, (name, b, frac[b], m["n32"], m["n64"], m["borderline"])
        if m["n32"] == 0:
            assert frac[b] == 0.0, (name, b)


@pytest.mark.parametrize("name", list(mc.ALL_COUNT))
def test_fp32_share_matches_the_host_model(ctx, name):
    kw = mc.ALL_COUNT[name]
    progs, _, t, y, t_new = mc.batch(**kw)
    mix = _run(ctx, default_spec(NGP_PREC_MIXED), progs, t, y, t_new)
    print(name, "info", mix["info"].tolist(), "refine_steps", mix["refine_steps"].tolist())
    print(name, "frac_f32", [float(f) for f in mix["frac_f32"]])
    assert (mix["info"] <= 0).all(), mix["info"]        # no pivot failure
    check_counts(name, kw, mix["frac_f32"])
    if name in mc.COUNT_ZERO:
        assert (mix["frac_f32"] == 0).all()
    if name in mc.LARGE:
        ref64 = _run(ctx, default_spec(), progs, t, y, t_new)
        assert not mix["info"].any() and not ref64["info"].any(), (mix["info"], ref64["info"])
        for b, (mu, sg, lm, info) in enumerate(oracle(name)):
            assert info == 0
            for ref_lm, ref_mu, ref_var, where in ((lm, mu, np.diag(sg), "oracle_np"),
                                                   (ref64["logml_full"][b, 0], ref64["mu"][b, 0],
                                                    np.diag(ref64["sigma"][b]), "fp64 job")):
                e = (nerr(mix["logml_full"][b, 0], ref_lm), nerr(mix["mu"][b, 0], ref_mu),
                     nerr(np.diag(mix["sigma"][b]), ref_var))
                print(name, b, "against", where, "logml %.2e mean %.2e variance %.2e" % e)
                assert max(e) < TOL_MIXED, (name, b, where, e)


def test_the_first_refused_series_runs_the_fp64_schedule(ctx):
    """n = 8,320 is 130 block columns: one more than the two ballot masks classify"""
    progs, _, t, y, t_new = mc.batch(**mc.REFUSED)
    mix = _run(ctx, default_spec(NGP_PREC_MIXED), progs, t, y, t_new)
    ref = _run(ctx, default_spec(), progs, t, y, t_new)
    assert not mix["info"].any() and not ref["info"].any()
    assert (mix["frac_f32"] == 0).all() and (mix["refine_steps"] == 0).all()
    assert np.array_equal(mix["logml_full"], ref["logml_full"])
    assert np.array_equal(mix["mu"], ref["mu"]) and np.array_equal(mix["sigma"], ref["sigma"])


@pytest.mark.parametrize("name", list(mc.ACC_CASES))
def test_sensitive_items_meet_the_tolerance_only_under_the_rule(ctx, name):
    progs, kinds, t, y, t_new = mc.batch(**mc.ACC_CASES[name])
    refs = [hp.evaluate(p, t, y, grad=False, t_new=t_new) for p in progs]
    assert all(r.info == 0 and r.tol_factor == 1.0 and r.cond <= 1e8 for r in refs)
    mix = _run(ctx, default_spec(NGP_PREC_MIXED), progs, t, y, t_new)
    print(name, "info", mix["info"].tolist(), "refine_steps", mix["refine_steps"].tolist(),
          "frac_f32", [float(f) for f in mix["frac_f32"]])
    errs = [(nerr(mix["logml_full"][b, 0], float(r.logml)), nerr(mix["mu"][b, 0], np.asarray(r.mu, float)),
             nerr(np.diag(mix["sigma"][b]), np.diag(np.asarray(r.sigma, float)))) for b, r in enumerate(refs)]
    for b, e in enumerate(errs):
        print(name, b, kinds[b], "noise %g: logml %.2e mean %.2e variance %.2e" % ((progs[b][2],) + e))
    forced = default_spec(NGP_PREC_MIXED)
    forced.mixed_tau, forced.refine_max = 1e30, 0
    f32 = _run(ctx, forced, progs, t, y, t_new)
    ferr = []
    for b, r in enumerate(refs):
        e = nerr(f32["logml_full"][b, 0], float(r.logml))
        ferr.append(e if np.isfinite(e) and f32["info"][b] == 0 else np.inf)   # a lost pivot: as wrong as it gets
        print(name, b, kinds[b], "every product in fp32: frac %.3f info %d logml error %.2e = %.0f x TOL_MIXED" %
              (f32["frac_f32"][b], f32["info"][b], ferr[b], ferr[b] / TOL_MIXED))
    assert (mix["info"] == 0).all(), mix["info"]
    for b, e in enumerate(errs):
        assert max(e) < TOL_MIXED, (name, b, kinds[b], e)
    for b, p in enumerate(progs):
        if p[2] <= mc.SENSITIVE_NOISE:
            assert ferr[b] > 10 * TOL_MIXED, (name, b, kinds[b], ferr[b])

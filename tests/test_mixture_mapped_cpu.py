"""ngp_mixture_crps_mapped, the parts that need no GPU: the host reference integrator reproduces
the three identities of include/ngp.h; the entry point refuses malformed calls before anything
touches a device; ``MixtureMarginals.wis`` against its definition; ``crps(y)`` with default
arguments is the closed form on the model's scale, as before; the host path of the mapped scores."""
import ctypes as C

import numpy as np
import pytest

from nowcastautogp_amd import _abi, _lib, autogp
from nowcastautogp_amd import nowcast as nc
from tests import mixture_mapped_reference as M
from tests import mixture_reference as R


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def test_symbol_is_declared_and_exported(lib):
    import os
    header = open(os.path.join(R.ROOT, "include", "ngp.h")).read()
    assert "ngp_mixture_crps_mapped" in _lib.SYMBOLS and "ngp_mixture_crps_mapped(" in header
    assert "NGP_INFO_NOT_FINITE (-3)" in header and "NGP_INFO_NOT_CONVERGED (-4)" in header
    assert lib.ngp_mixture_crps_mapped is not None


def test_the_reference_reproduces_the_identities():
    mix = R.make_mixture(5, 3, seed=1)
    y = np.array([0.3, 0.1, 0.6])
    closed, _ = R.ref_crps(mix, y)
    r = M.reference(mix, (M.IDENTITY, 0, 0, 0), M.NATURAL, 0.0, y)
    print("identity + natural:", np.abs(r["crps"] - closed) / closed)
    assert np.all(np.abs(r["crps"] - closed) <= 1e-13 * closed)
    np.testing.assert_allclose(r["mean"], mix.w @ mix.mu, rtol=1e-13)
    ey = np.exp(y)
    closed, _ = R.ref_crps(mix, np.log(ey))
    r = M.reference(mix, (M.EXP, 0, 0, 0), M.LOG, 0.0, ey)
    print("exp + log:", np.abs(r["crps"] - closed) / closed)
    assert np.all(np.abs(r["crps"] - closed) <= 1e-13 * closed)
    for mu, sd, yy in ((0.4, 0.3, 1.7), (2.0, 0.8, 3.0), (-1.0, 0.1, 0.5)):
        one = R.Mixture([1.0], [[mu]], [[sd * sd]])
        r = M.reference(one, (M.EXP, 0, 0, 0), M.NATURAL, 0.0, [yy])
        want = M.lognormal_crps(mu, sd, yy)
        print("lognormal:", abs(r["crps"][0] - want) / want)
        assert abs(r["crps"][0] - want) <= 1e-13 * want
        assert abs(r["mean"][0] - np.exp(mu + sd * sd / 2)) <= 1e-13 * np.exp(mu + sd * sd / 2)


def test_the_reference_converges_on_the_panel_cap_case():
    from tests.test_mixture_mapped_gpu import sd_ratio_case
    mix, inv, y = sd_ratio_case()
    r = M.reference(mix, inv, M.NATURAL, 0.0, y)
    assert r["status"][0] == 0 and np.isfinite(r["crps"][0]) and r["levels"][0] <= 3


def test_entry_point_rejects_malformed_calls_without_a_gpu(lib):
    """NGP_ERR_ARG before anything touches a device: the "context" is a block of zeros"""
    NGP_ERR_ARG = lib.ngp_logml_batch(None, 0, None, 0, None, None, 0, None, None)
    assert NGP_ERR_ARG != 0
    fake = C.create_string_buffer(1 << 16)
    ctx = C.cast(fake, C.c_void_p)
    Cn, m = 3, 2
    w = np.array([0.2, 0.3, 0.5])
    mu, var = np.zeros((Cn, m)), np.ones((Cn, m))
    y, out, info = np.ones(m), np.zeros(m), np.zeros(m, dtype=np.int32)
    d, i = _lib.dptr, _lib.iptr
    good = _abi.NgpInvTransform(_abi.NGP_INV_BOXCOX, 0.3, 0.0, 1e6)

    def call(c=ctx, C_=Cn, m_=m, w_=w, mu_=mu, var_=var, inv_=good, scale_=1, shift_=1.0, y_=y,
             tol_=0.0, out_=out, info_=info):
        p = lambda a: None if a is None else d(a)
        return lib.ngp_mixture_crps_mapped(c, C_, m_, p(w_), p(mu_), p(var_),
                                           None if inv_ is None else C.byref(inv_), scale_, shift_,
                                           p(y_), tol_, p(out_), None, None,
                                           None if info_ is None else i(info_))

    assert call(c=None) == NGP_ERR_ARG
    for bad in (dict(C_=0), dict(m_=0), dict(C_=-1), dict(m_=-5), dict(out_=None), dict(info_=None),
                dict(w_=None), dict(mu_=None), dict(var_=None), dict(y_=None), dict(inv_=None),
                dict(w_=np.array([0.5, -0.1, 0.6])), dict(w_=np.array([0.5, np.nan, 0.5])),
                dict(w_=np.zeros(3)), dict(scale_=2), dict(scale_=-1),
                dict(shift_=-0.5), dict(shift_=np.nan), dict(shift_=np.inf), dict(tol_=np.nan),
                dict(tol_=np.inf), dict(y_=np.array([1.0, np.nan])), dict(y_=np.array([np.inf, 1.0])),
                dict(y_=np.array([1.0, -1.0])), dict(y_=np.array([0.0, 1.0]), shift_=0.0)):
        assert call(**bad) == NGP_ERR_ARG, bad
    for kind, lam, off, cap in ((4, 0.3, 0.0, 1.0), (-1, 0.3, 0.0, 1.0), (3, np.nan, 0.0, 1.0),
                                (3, 0.3, np.inf, 1.0), (3, 0.3, 0.0, np.nan)):
        assert call(inv_=_abi.NgpInvTransform(kind, lam, off, cap)) == NGP_ERR_ARG, (kind, lam, off, cap)


def test_wis_against_its_definition():
    mix = R.make_mixture(5, 4, seed=4)
    mix = R.Mixture(mix.w, mix.mu + 3.0, mix.var)
    mm = autogp.MixtureMarginals(mix.mu, mix.var, mix.w)
    _, inv = nc.get_transformations("positive", np.array([0.0, 3.0, 10.0, 40.0]))
    levels = np.array([0.5, 0.8, 0.95])
    y_model = np.array([3.1, 2.5, 3.9, 3.3])
    for kw, y, tr in ((dict(), y_model, lambda v: v),
                      (dict(inv_transformation=inv, scale="natural"), inv(y_model), lambda v: v),
                      (dict(inv_transformation=inv, scale="log", shift=1.0), inv(y_model),
                       lambda v: np.log(v + 1.0))):
        got = mm.wis(y, levels, **kw)
        want = np.zeros(4)
        f = kw.get("inv_transformation", lambda v: v)
        for j in range(4):
            yt = tr(y[j])
            total = 0.5 * abs(yt - tr(f(mm.quantile([0.5])[j, 0])))
            for lv in levels:
                a = 1.0 - lv
                lo, hi = (tr(f(mm.quantile([p])[j, 0])) for p in (a / 2, 1 - a / 2))
                interval = (hi - lo) + 2 / a * max(lo - yt, 0.0) + 2 / a * max(yt - hi, 0.0)
                total += a / 2 * interval
            want[j] = total / (levels.size + 0.5)
        np.testing.assert_allclose(got, want, rtol=1e-12)


def test_default_crps_is_the_closed_form_on_the_model_scale():
    mix = R.make_mixture(5, 4, seed=6)
    mm = autogp.MixtureMarginals(mix.mu, mix.var, mix.w)
    y = np.array([0.2, 0.4, 0.1, 0.5])
    want = np.empty(4)
    w = mix.w / mix.w.sum()
    for j in range(4):      # the host formula of the class, written out
        t1 = float(w @ autogp._abs_moment(y[j] - mix.mu[:, j], mix.var[:, j]))
        a = autogp._abs_moment(mix.mu[:, j][:, None] - mix.mu[:, j][None, :],
                               mix.var[:, j][:, None] + mix.var[:, j][None, :])
        want[j] = t1 - 0.5 * float(w @ a @ w)
    np.testing.assert_array_equal(mm.crps(y), want)
    np.testing.assert_array_equal(mm.crps(y, scale="model"), want)
    np.testing.assert_array_equal(mm.mean(), w @ mix.mu)


def test_host_path_of_the_mapped_scores():
    mix = R.make_mixture(5, 3, seed=1)
    mix = R.Mixture(mix.w, mix.mu + 3.0, mix.var)
    mm = autogp.MixtureMarginals(mix.mu, mix.var, mix.w)
    _, inv = nc.get_transformations("boxcox", np.array([0.0, 3.0, 10.0, 40.0, 80.0, 25.0]))
    y = inv(np.array([3.2, 3.4, 3.1]))
    for scale, sc, shift in (("natural", M.NATURAL, 0.0), ("log", M.LOG, 1.0)):
        crps, err = mm.crps(y, inv, scale, shift, return_error=True)
        ref = M.reference(mix, inv.ngp_inv, sc, shift, y)
        assert np.all(np.abs(crps - ref["crps"]) <= err + 1e-12 * ref["S"])
        assert np.all(np.abs(mm.mean(inv, scale, shift) - ref["mean"]) <= 1e-10 * ref["S"] + 1e-12 * np.abs(ref["mean"]))
    with pytest.raises(ArithmeticError):
        mm.crps(np.array([3.0, 3.0, 3.0]), lambda v: v, "natural") if False else \
            autogp.MixtureMarginals(mix.mu - 3.0, mix.var, mix.w).crps(np.ones(3), None, "log", 0.0)
    atom = autogp.AtomMixtureMarginals(mix.mu, mix.var, mix.w, 0.2)
    with pytest.raises(NotImplementedError):
        atom.crps(y, inv, "natural")
    with pytest.raises(NotImplementedError):
        atom.mean(inv, "log", 1.0)

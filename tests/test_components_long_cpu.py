"""ngp_factor_components_long without a GPU: the symbol, its refusals before a device is touched, and
ComponentForecast.grouped() reading the same-date covariances (``cross``) instead of a full sigma."""
import inspect
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
from nowcastautogp_amd import _abi, _lib, autogp
from nowcastautogp_amd import nowcast as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NGP_ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return _lib.load()


def test_symbol_is_bound_and_declared(lib):
    hdr = open(os.path.join(ROOT, "include", "ngp.h")).read()
    assert "ngp_factor_components_long" in _lib.SYMBOLS
    assert re.search(r"\bngp_status\s+ngp_factor_components_long\s*\(", hdr)
    assert hasattr(lib, "ngp_factor_components_long")
    assert hasattr(_lib.Factor, "components_long")
    for fn in (autogp.predict_components, nc.forecast_components_with_nowcasts):
        par = inspect.signature(fn).parameters
        assert par["one_query"].default is False and par["want_sigma"].default is False


def test_null_and_empty_arguments_are_refused_without_a_device(lib):
    """a null factor is NGP_ERR_ARG whatever else is passed, and so is every other null or empty
    argument beside it: nothing here has a context, so nothing can have touched a device"""
    one = np.ones(4)
    cnt, info = np.ones(1, np.int32), np.zeros(1, np.int32)
    ka = _abi.KernelArray([(np.array([3], np.int32), np.array([0.2, 0.5]), 0.0)])
    p, ip, cp = _abi.dptr(one), _lib.iptr(info), _lib.iptr(cnt)
    call = lib.ngp_factor_components_long
    assert call(None, 0, None, 1, None, cp, ka.arr, 4, p, p, p, None, ip) == NGP_ERR_ARG
    assert call(None, 0, None, 1, None, None, None, 0, None, None, None, None, None) == NGP_ERR_ARG
    assert call(None, 0, None, 1, None, None, ka.arr, 4, p, p, p, p, ip) == NGP_ERR_ARG
    assert call(None, 0, None, 1, None, cp, None, 4, p, p, p, p, ip) == NGP_ERR_ARG
    assert call(None, 0, None, 1, None, cp, ka.arr, 4, p, None, p, p, ip) == NGP_ERR_ARG
    assert call(None, 0, None, 1, None, cp, ka.arr, 4, p, p, None, p, ip) == NGP_ERR_ARG
    assert call(None, 0, None, 1, None, cp, ka.arr, 0, p, p, p, p, ip) == NGP_ERR_ARG
    assert call(None, -1, p, 1, p, cp, ka.arr, 4, p, p, p, p, ip) == NGP_ERR_ARG


def synthetic(rng, counts, kinds, m):
    """per particle a random joint covariance of its parts and the same-date entries cut from it"""
    means, sigma, var, cross = [], [], [], []
    for C in counts:
        a = rng.standard_normal((C * m, C * m + 3))
        s = a @ a.T
        means.append(rng.standard_normal((C, m)))
        sigma.append(s)
        var.append(np.diag(s).reshape(C, m).copy())
        cross.append(np.ascontiguousarray(np.einsum("ajbj->abj", s.reshape(C, m, C, m))))
    w = rng.uniform(0.5, 1.5, len(counts))
    labels = [[f"part {c}" for c in range(C)] for C in counts]
    full = autogp.ComponentForecast(means, sigma, var, w / w.sum(), kinds, labels, 1.5)
    lean = autogp.ComponentForecast(means, [None] * len(counts), var, w / w.sum(), kinds, labels, 1.5,
                                    cross=cross)
    return full, lean


@pytest.mark.parametrize("by", ["kind", "label"])
def test_grouped_from_cross_is_grouped_from_sigma(by):
    """three particles of 3, 1 and 2 parts; the second has no seasonal part and the second and third
    no third label: those groups carry an atom at 0"""
    kinds = [["trend", "seasonal", "seasonal"], ["trend"], ["seasonal", "trend"]]
    full, lean = synthetic(np.random.default_rng(5), [3, 1, 2], kinds, 7)
    assert full.cross is None and lean.sigma == [None] * 3
    a, b = full.grouped(by), lean.grouped(by)
    assert list(a) == list(b) and len(a) >= 2
    atoms = 0
    for name in a:
        assert type(a[name]) is type(b[name])
        np.testing.assert_array_equal(a[name].means, b[name].means)
        np.testing.assert_array_equal(a[name].variances, b[name].variances)
        np.testing.assert_array_equal(a[name].weights, b[name].weights)
        if isinstance(a[name], autogp.AtomMixtureMarginals):
            assert a[name].atom == b[name].atom
            atoms += 1
    assert atoms >= 1

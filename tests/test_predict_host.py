"""Prediction / goodness-of-fit entry points, the parts that need no GPU: the ABI names, argument validation in front of
the device, and the defaults of the fitter keywords (the numpy path runs unchanged unless asked otherwise)."""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from pyneapple_amd import _lib, api

NEW = ["pnx_nnls_fit_stats_f64", "pnx_nnls_solve_peaks_stats_f64", "pnx_curvefit_predict_f64"]


def test_new_functions_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "pnx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW:
        assert re.search(r"^PNX_API\s+int\s+" + name + r"\s*\(", text, flags=re.M), f"{name} is not declared in include/pnx.h"
        assert name in exported, f"{name} is not exported by the library"
        assert name in _lib.ABI_SYMBOLS
    # the chained entry point takes every argument of pnx_nnls_solve_peaks_f64, in its order, then ss_res
    lib = _lib.load()
    assert list(lib.pnx_nnls_solve_peaks_stats_f64.argtypes[:-1]) == list(lib.pnx_nnls_solve_peaks_f64.argtypes)


def test_library_refuses_bad_predict_arguments_without_a_device():
    import ctypes as C

    lib = _lib.load()
    one = np.zeros(400)
    o = api.make_opts("bi_reduced", 16)
    call = lambda n_x, pred, ss, y=None, opts=o: lib.pnx_curvefit_predict_f64(C.byref(opts), 1, n_x, _lib.ptr(one), _lib.ptr(one), None, y,
                                                                              pred, ss, 0, 0, None)
    assert call(129, _lib.ptr(one), None) == -1 and "n_x" in _lib.last_error()
    assert call(0, _lib.ptr(one), None) == -1
    assert call(16, None, None) == -1 and "both NULL" in _lib.last_error()
    assert call(16, None, _lib.ptr(one)) == -1 and "needs the signal" in _lib.last_error()
    bad = api.make_opts("bi_reduced", 16)
    bad.n_free = 2
    assert call(16, _lib.ptr(one), None, opts=bad) == -1 and "n_free" in _lib.last_error()
    # n_b is not read: an opts struct made for another b-value count (even an invalid one) is accepted up to the device query
    odd = api.make_opts("bi_reduced", 16)
    odd.n_b = 0
    rc = call(16, _lib.ptr(one), None, opts=odd)
    assert rc in (0, -3), _lib.last_error()
    assert lib.pnx_nnls_fit_stats_f64(None, 1, _lib.ptr(one), _lib.ptr(one), _lib.ptr(one), None, 0, 0, None) == -1
    assert lib.pnx_nnls_solve_peaks_stats_f64(None, 1, _lib.ptr(one), 0, _lib.ptr(one), 0.1, 0, 0.5, 8, None, None, None, 0, None, None, None,
                                              _lib.ptr(one), None, None, 0, None, None) == -1


def test_predict_validates_before_touching_the_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_lib, "require_device", no_device)
    monkeypatch.setattr(api, "load", no_device)
    x = np.linspace(0, 1000, 16)
    p = np.ones((3, 10))
    with pytest.raises(ValueError, match="1 .. 128"):
        api.predict("bi_reduced", np.linspace(0, 1, 129), p)
    with pytest.raises(ValueError, match="1-D"):
        api.predict("bi_reduced", np.zeros((2, 4)), p)
    with pytest.raises(ValueError, match="nothing to compute"):
        api.predict("bi_reduced", x, p, want_pred=False)
    with pytest.raises(ValueError, match=r"expected \(3, n_vox\)"):
        api.predict("bi_reduced", x, np.ones((2, 10)))
    with pytest.raises(ValueError, match=r"expected \(2, n_vox\)"):  # one parameter fixed: two free rows
        api.predict("bi_reduced", x, p, fixed_idx=[1], fixed_vals=[0.01])
    with pytest.raises(ValueError, match=r"expected \(4, n_vox\)"):  # T1 is one more parameter
        api.predict("bi_reduced", x, p, t1_mode=1, tr=3000.0)
    with pytest.raises(ValueError, match="y has shape"):
        api.predict("bi_reduced", x, p, y=np.zeros((10, 15)))
    with pytest.raises(ValueError, match="fixed_vals has the wrong shape"):
        api.predict("bi_reduced", x, np.ones((2, 10)), fixed_idx=[1], fixed_vals=np.ones((1, 9)))
    with pytest.raises(ValueError, match="unknown model"):
        api.predict("quad", x, p)


def test_fit_stats_validates_before_touching_the_device(monkeypatch):
    plan = api.NnlsPlan.__new__(api.NnlsPlan)  # no device: the shape checks come first
    plan.n_meas, plan.n_bins, plan.device, plan._h = 16, 50, 0, None
    monkeypatch.setattr(api, "load", lambda: (_ for _ in ()).throw(AssertionError("the device was touched")))
    with pytest.raises(ValueError, match="coeff has shape"):
        plan.fit_stats(np.zeros((4, 16)), np.zeros((4, 49)))
    with pytest.raises(ValueError, match="signal has shape"):
        plan.fit_stats(np.zeros((4, 15)), np.zeros((4, 50)))
    with pytest.raises(ValueError, match="signal has shape"):
        plan.fit_stats(np.zeros((5, 16)), np.zeros((4, 50)))
    with pytest.raises(ValueError, match="nothing to compute"):
        plan.fit_stats(None, np.zeros((4, 50)))
    assert api.NNLSPlan is api.NnlsPlan


class _StubLib:
    """Records which entry point a call went through; answers success and leaves the outputs as they are."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append(name)
            return 0

        return fn


def test_fit_peaks_default_takes_the_old_entry_point(monkeypatch):
    from pyneapple_amd.models import NNLSModel
    from pyneapple_amd.solvers import HipNNLSSolver

    stub = _StubLib()
    monkeypatch.setattr(api, "load", lambda: stub)
    monkeypatch.setattr(_lib, "require_device", lambda: None)
    monkeypatch.setattr(api, "row_ss_tot", lambda y, device=0: np.ones(len(y)))
    b = np.linspace(0, 1000, 16)
    y = np.ones((5, 16))
    s = HipNNLSSolver(model=NNLSModel(d_range=(1e-4, 0.1), n_bins=50), reg_order=2, mu=0.02)
    monkeypatch.setattr(s, "get_regularization_matrix", lambda: np.zeros((50, 50)))
    s.fit_peaks(b, y)
    assert "pnx_nnls_solve_peaks_f64" in stub.calls and "pnx_nnls_solve_peaks_stats_f64" not in stub.calls
    assert "r_squared" not in s.diagnostics_
    stub.calls.clear()
    s.fit_peaks(b, y, r_squared=True)
    assert "pnx_nnls_solve_peaks_stats_f64" in stub.calls and "pnx_nnls_solve_peaks_f64" not in stub.calls
    assert s.diagnostics_["r_squared"].shape == (5,) and s.diagnostics_["ss_res"].shape == (5,)


class _FakeNnlsSolver:
    """What _assemble reads of a fitted HIP NNLS solver."""

    reg_order = 2
    device = 0

    def __init__(self, model, coeffs):
        self.model = model
        self.params_ = {"coefficients": coeffs}
        self.diagnostics_ = {"status": np.ones(len(coeffs), np.int8), "residual": np.zeros(len(coeffs))}
        self.pixel_results_ = None


def test_pixelwise_fitter_defaults_take_the_numpy_path(monkeypatch):
    from pyneapple_amd.fitters import HipPixelWiseFitter
    from pyneapple_amd.models import NNLSModel

    def no_device(*a, **k):
        raise AssertionError("the default path called into the device statistics")

    for name in ("predict", "row_ss_tot", "NnlsPlan"):
        monkeypatch.setattr(api, name, no_device)
    rng = np.random.default_rng(0)
    model = NNLSModel(d_range=(1e-4, 0.1), n_bins=50)
    b = np.linspace(0, 1000, 16)
    coeffs = rng.uniform(0, 1, (6, 50))
    pixels = coeffs @ np.asarray(model.get_basis(b)).T + rng.normal(0, 0.1, (6, 16))
    f = HipPixelWiseFitter(_FakeNnlsSolver(model, coeffs))
    assert f.device_stats is False
    f.image_shape, f.pixel_indices = (6, 1, 1, 16), np.argwhere(np.ones((6, 1, 1), bool))
    f.fitted_params_ = {"coefficients": coeffs}
    r = f._assemble(b, pixels, 0.0)
    pred = coeffs @ np.asarray(model.get_basis(b)).T
    ss_res = ((pixels - pred) ** 2).sum(axis=1)
    ss_tot = ((pixels - pixels.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)
    np.testing.assert_allclose(r.r_squared, 1 - ss_res / ss_tot, rtol=1e-12)
    np.testing.assert_array_equal(f.predict(b), pred.reshape(6, 1, 1, 16))
    # and the keyword routes all three reductions to the device
    g = HipPixelWiseFitter(_FakeNnlsSolver(model, coeffs), device_stats=True)
    assert g.device_stats is True
    g.image_shape, g.pixel_indices, g.fitted_params_ = f.image_shape, f.pixel_indices, f.fitted_params_
    with pytest.raises(AssertionError, match="device statistics"):
        g._assemble(b, pixels, 0.0)
    with pytest.raises(AssertionError, match="device statistics"):
        g.predict(b, on_device=True)

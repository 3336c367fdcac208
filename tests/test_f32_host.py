"""The fp32-arithmetic curve fit (pnx_curvefit_fast_f32, precision="float32") without a GPU: the symbol, its argument
validation, the keyword rules of the solver plugin, and no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import ROOT

from pyneapple_amd import _lib, api, synth
from pyneapple_amd.models import BiExpModel, MonoExpModel, TriExpModel
from pyneapple_amd.solvers import HipCurveFitSolver


def test_fast_f32_is_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "pnx.h")).read()
    assert re.search(r"^PNX_API int pnx_curvefit_fast_f32\s*\(", text, flags=re.M)
    assert "pnx_curvefit_fast_f32" in _lib.ABI_SYMBOLS
    assert hasattr(_lib.load(), "pnx_curvefit_fast_f32")
    # exactly the argument list of pnx_curvefit_batch_f32
    args = lambda name: re.sub(r"\s+", " ", re.search(name + r"\s*\((.*?)\);", text, flags=re.S).group(1))
    assert args("pnx_curvefit_fast_f32") == args("pnx_curvefit_batch_f32")


def _call(o, fixed=None, sigma=None):
    one = np.zeros(8, np.float32)
    if sigma is not None:
        o.sigma = sigma.ctypes.data
    return _lib.load().pnx_curvefit_fast_f32(C.byref(o), 1, _lib.ptr(one), _lib.ptr(one), _lib.ptr(one), _lib.ptr(one), _lib.ptr(one),
                                             _lib.ptr(fixed), _lib.ptr(one), None, None, None, None, 0, 0, None)


def test_argument_validation_needs_no_gpu():
    o = api.make_opts("tri_reduced", 32, jac="analytic")
    o.n_free = 3  # inconsistent with the model
    assert _call(o) == -1 and "n_free" in _lib.last_error()
    assert _call(api.make_opts("tri_reduced", 32, jac="fd")) == -2 and "PNX_JAC_ANALYTIC" in _lib.last_error()
    assert _call(api.make_opts("bi_reduced", 24, fixed_idx=[1], jac="analytic"), fixed=np.zeros(8, np.float32)) == -2
    assert "fixed parameters" in _lib.last_error()
    assert _call(api.make_opts("mono", 16, jac="analytic", t1_mode=1, tr=3000.0)) == -2 and "T1" in _lib.last_error()
    sg = np.ones(16)
    assert _call(api.make_opts("mono", 16, jac="analytic"), sigma=sg) == -2 and "sigma" in _lib.last_error()
    o = api.make_opts("mono", 16, jac="analytic")
    o.queue_order = 8  # any non-NULL value: refused before it is looked at
    assert _call(o) == -2 and "queue_order" in _lib.last_error()


def _kw(model_key="tri_reduced", model=None):
    names, p0, lo, hi = synth.shared_arrays(model_key)
    return dict(model=model or TriExpModel(), max_iter=250, tol=1e-8, p0=dict(zip(names, p0)),
                bounds={n: (l, h) for n, l, h in zip(names, lo, hi)})


def test_solver_keyword_rules():
    s = HipCurveFitSolver(**_kw())
    assert s.precision == "float64" and s.jacobian_mode == "fd" and s.io_dtype is np.float64
    s = HipCurveFitSolver(precision="float32", **_kw())
    assert s.precision == "float32" and s.jacobian_mode == "analytic" and s.io_dtype is np.float32
    assert HipCurveFitSolver(precision="float32", jacobian="analytic", n_gpus=2, **_kw()).n_gpus == 2
    with pytest.raises(ValueError, match="analytic"):
        HipCurveFitSolver(precision="float32", jacobian="fd", **_kw())
    with pytest.raises(ValueError, match="precision"):
        HipCurveFitSolver(precision="float16", **_kw())
    with pytest.raises(ValueError, match="sigma"):
        HipCurveFitSolver(precision="float32", sigma=0.1, **_kw())
    t1 = _kw("mono", MonoExpModel(fit_t1=True, repetition_time=3000.0))
    t1["p0"]["T1"], t1["bounds"]["T1"] = 1000.0, (100.0, 5000.0)
    assert HipCurveFitSolver(**t1).precision == "float64"  # a valid fp64 configuration ...
    with pytest.raises(ValueError, match="T1 / STEAM"):  # ... that the fp32 path is not built for
        HipCurveFitSolver(precision="float32", **t1)
    bi = BiExpModel(fixed_params={"D1": 0.01})
    names = list(bi.param_names)
    with pytest.raises(ValueError, match="fixed parameters"):
        HipCurveFitSolver(precision="float32", model=bi, max_iter=250, tol=1e-8, p0={n: 0.1 for n in names},
                          bounds={n: (0.0, 1.0) for n in names})
    # per-pixel fixed parameters are only known at fit(): refused there, before any device is touched
    b, y, _ = synth.make_numpy("tri_reduced", 4, 32)
    with pytest.raises(ValueError, match="fixed parameters"):
        HipCurveFitSolver(precision="float32", **_kw()).fit(b, y, pixel_fixed_params={"D1": np.full(4, 0.05)})


def test_api_precision_rules():
    b, y, _ = synth.make_numpy("mono", 4, 16)
    _, p0, lo, hi = synth.shared_arrays("mono")
    with pytest.raises(ValueError, match="precision"):
        api.curvefit("mono", b, y, p0, lo, hi, precision="half")
    with pytest.raises(ValueError, match="analytic"):
        api.curvefit("mono", b, y, p0, lo, hi, precision="float32", jac="fd")
    with pytest.raises(ValueError, match="sigma"):
        api.curvefit("mono", b, y, p0, lo, hi, precision="float32", sigma=0.1)


def test_ideal_fitter_refuses_an_fp32_solver():
    from pyneapple_amd.ideal import HipIDEALFitter

    with pytest.raises(ValueError, match="float32"):
        HipIDEALFitter(HipCurveFitSolver(precision="float32", **_kw()), dim_steps=[[1, 1], [4, 4]],
                       step_tol={n: 0.5 for n in synth.P0["tri_reduced"]})


def test_no_cpu_fallback_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is visible here")
    b, y, _ = synth.make_numpy("tri_reduced", 4, 32)
    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    with pytest.raises(_lib.PnxError):
        api.curvefit("tri_reduced", b, y, p0, lo, hi, precision="float32")
    with pytest.raises(_lib.PnxError):
        HipCurveFitSolver(precision="float32", **_kw()).fit(b, y)

"""The exponential-peeling fit (pnx_peel_f64 / _f32, HipPeelSolver, HipCurveFitSolver(p0_peel=...)), the parts that need no GPU:
the ABI symbols, their refusals in front of any device work, the Python-side refusals, the entry point, thresholds -> masks, the
agreement of the reference's two forms on the parity signals, and the host-side argument checks under AddressSanitizer / UBSan (a
stand-alone program, tests/host_stub/peel_args_stub.cpp)."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT
from peel_reference import STAGES, parity_case, reference, signals, stage_masks

from pyneapple_amd import _lib, api
from pyneapple_amd.models import BiExpModel, MonoExpModel, TriExpModel
from pyneapple_amd.solvers import HipConstrainedCurveFitSolver, HipCurveFitSolver, HipPeelSolver

NAMES = ("pnx_peel_f64", "pnx_peel_f32")
TRI_S0 = api.MODEL_IDS["tri_s0"]


def _use(K, n_b):
    use = np.zeros((K, max(n_b, 0)), np.uint8)
    for i in range(max(n_b, 0)):
        use[i % K, i] = 1
    return use


def _call(fn="pnx_peel_f64", model=TRI_S0, n_b=8, b=True, use=True, weighting=1, clip=0, lo=None, hi=None, fallback=None, y=True,
          params=True, mem=0):
    dt = np.float32 if fn.endswith("f32") else np.float64
    bv = (np.arange(max(n_b, 1)) * 50.0).astype(dt) if b is True else b
    uv = _use(3, n_b) if use is True else use
    yv, pv = np.ones(128, dt), np.zeros(6, dt)
    keep = [bv, uv, lo, hi, fallback, yv, pv]  # alive across the call
    rc = getattr(_lib.load(), fn)(model, 1, n_b, _lib.ptr(bv), _lib.ptr(uv), weighting, clip, _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(fallback),
                                  _lib.ptr(yv) if y else None, _lib.ptr(pv) if params else None, None, None, None, mem, 0, None)
    del keep
    return rc


def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnx.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout.split()
    for name in NAMES:
        assert re.search(r"PNX_API\s+int\s+" + name + r"\s*\(", text)
        assert name in _lib.ABI_SYMBOLS
        fn = getattr(_lib.load(), name)
        assert len(fn.argtypes) == 18 and fn.restype is C.c_int
        assert name in out


@pytest.mark.parametrize("fn", NAMES)
def test_abi_refusals_need_no_device(fn):
    """Every refusal comes back -1 with its argument named, before a device is touched: this runs on a machine without one."""
    dt = np.float32 if fn.endswith("f32") else np.float64
    err = _lib.last_error
    for model in (-1, 7):
        assert _call(fn, model=model) == -1 and "model" in err()
    for n_b in (-1, 0, 5, 129):  # three exponentials need six b-values
        assert _call(fn, n_b=n_b) == -1 and "n_b" in err()
    assert _call(fn, model=api.MODEL_IDS["bi_s0"], n_b=3, use=_use(2, 3)) == -1 and "n_b" in err()
    assert _call(fn, model=api.MODEL_IDS["mono"], n_b=1, use=_use(1, 1)) == -1 and "n_b" in err()
    assert _call(fn, b=None) == -1 and "b is NULL" in err()
    assert _call(fn, use=None) == -1 and "use is NULL" in err()
    assert _call(fn, y=False) == -1 and "y is NULL" in err()
    assert _call(fn, params=False) == -1 and "params is NULL" in err()
    for bad in (np.nan, np.inf):
        b = (np.arange(8) * 50.0).astype(dt)
        b[5] = bad
        assert _call(fn, b=b) == -1 and "b[5]" in err()
    for w in (-1, 2):
        assert _call(fn, weighting=w) == -1 and "weighting" in err()
    for k in range(3):
        use = _use(3, 8)
        use[k] = 0
        assert _call(fn, use=use) == -1 and f"use row {k}" in err()
        use[k, 3] = 1
        assert _call(fn, use=use) == -1 and f"use row {k}" in err()
        use[k, 6] = 1
        b = (np.arange(8) * 50.0).astype(dt)
        b[6] = b[3]
        assert _call(fn, b=b, use=use) == -1 and "distinct" in err() and f"row {k}" in err()
    lo, hi = np.full(6, 1e-5, dt), np.full(6, 5000.0, dt)
    assert _call(fn, clip=1) == -1 and "lo" in err()
    assert _call(fn, clip=1, lo=lo) == -1 and "hi" in err()
    bad_hi = hi.copy()
    bad_hi[5] = lo[5]
    assert _call(fn, clip=1, lo=lo, hi=bad_hi) == -1 and "lo[5]" in err()
    for mem in (-1, 2):
        assert _call(fn, mem=mem) == -1 and "mem" in err()
    if _lib.device_count() == 0:  # fully valid calls stop at the device, and only there
        assert _call(fn) == -3
        assert _call(fn, weighting=0, clip=1, lo=lo, hi=hi, fallback=np.ones(6, dt), mem=1) == -3
        assert _call(fn, n_b=6) == -3 and _call(fn, n_b=128) == -3
        assert _call(fn, model=api.MODEL_IDS["mono"], n_b=2, use=_use(1, 2)) == -3


def test_thresholds_build_the_masks():
    b = np.array([0.0, 10.0, 30.0, 100.0, 250.0, 800.0])
    assert api.peel_masks(b, "tri_s0", [30, 250]).tolist() == [[0, 0, 0, 0, 1, 1], [0, 0, 1, 1, 0, 0], [1, 1, 0, 0, 0, 0]]
    assert api.peel_masks(b, "bi_full", [100]).tolist() == [[0, 0, 0, 1, 1, 1], [1, 1, 1, 0, 0, 0]]
    assert api.peel_masks(b, "mono", None).tolist() == [[1] * 6] and api.peel_masks(b, "mono", []).dtype == np.uint8
    for model, bad in (("tri_s0", [250, 30]), ("tri_s0", [30]), ("bi_s0", [30, 250]), ("bi_s0", None), ("mono", [10]), ("bi_s0", [np.nan])):
        with pytest.raises(ValueError, match="b_thresholds"):
            api.peel_masks(b, model, bad)
    # the reference's helper restates the rule on its own
    for model, t in (("tri_s0", [30, 250]), ("bi_s0", [150])):
        bb = np.geomspace(1, 1200, 24)
        assert np.array_equal(api.peel_masks(bb, model, t).astype(bool), stage_masks(bb, STAGES[model]))


def test_api_argument_rules():
    b, y = np.linspace(0, 800, 8), np.ones((2, 8))
    args = lambda **kw: api._peel_args(b, 8, np.float64, kw.pop("model", "bi_s0"), kw.pop("masks", None), kw.pop("b_thresholds", None),
                                       kw.pop("weighting", "signal2"), kw.pop("clip", None), kw.pop("fallback", None))
    with pytest.raises(ValueError, match="model"):
        args(model="quad")
    with pytest.raises(ValueError, match="masks .* or b_thresholds"):
        args()
    with pytest.raises(ValueError, match="masks .* or b_thresholds"):
        args(masks=np.ones((2, 8)), b_thresholds=[100])
    with pytest.raises(ValueError, match="masks has shape"):
        args(masks=np.ones((3, 8)))
    with pytest.raises(ValueError, match="weighting"):
        args(b_thresholds=[100], weighting="signal")
    with pytest.raises(ValueError, match="clip"):
        args(b_thresholds=[100], clip=([0, 0, 0], [1, 1, 1]))
    with pytest.raises(ValueError, match="fallback"):
        args(b_thresholds=[100], fallback=[1, 2, 3])
    bb, use, w, lo, hi, fb = args(b_thresholds=[300], weighting="none", clip=([0] * 4, [1] * 4), fallback=[0.5] * 4)
    assert use.dtype == np.uint8 and use.shape == (2, 8) and w == 0 and lo.shape == hi.shape == fb.shape == (4,)
    assert args(model="mono")[1].tolist() == [[1] * 8]  # one exponential: every b-value without being told


def test_peel_solver_rules():
    with pytest.raises(ValueError, match="T1"):
        HipPeelSolver(BiExpModel(fit_s0=True, fit_t1=True, repetition_time=3000.0), b_thresholds=[150])
    with pytest.raises(ValueError, match="fixed"):
        HipPeelSolver(BiExpModel(fit_s0=True, fixed_params={"D2": 1e-3}), b_thresholds=[150])
    with pytest.raises(ValueError, match="b_thresholds"):
        HipPeelSolver(BiExpModel(fit_s0=True))
    with pytest.raises(ValueError, match="b_thresholds"):
        HipPeelSolver(TriExpModel(fit_s0=True), b_thresholds=[150])
    with pytest.raises(ValueError, match="weighting"):
        HipPeelSolver(BiExpModel(fit_s0=True), b_thresholds=[150], weighting="signal")
    with pytest.raises(ValueError, match="Missing"):
        HipPeelSolver(BiExpModel(fit_s0=True), b_thresholds=[150], p0={"f1": 0.2})
    with pytest.raises(ValueError, match="Missing"):
        HipPeelSolver(BiExpModel(fit_s0=True), b_thresholds=[150], bounds={"f1": (0.0, 1.0)})
    with pytest.raises(ValueError, match="io_dtype"):
        HipPeelSolver(BiExpModel(fit_s0=True), b_thresholds=[150], io_dtype="float16")
    s = HipPeelSolver(BiExpModel(fit_s0=True), b_thresholds=[150])
    assert (s.max_iter, s.tol, s.p0, s.bounds, s.b_thresholds, s.weighting, s.device, s.io_dtype) == \
        (250, 1e-8, None, None, [150.0], "signal2", 0, np.float64)
    assert s.params_ == {} and s.diagnostics_ == {} and len(s.pixel_results_) == 0
    with pytest.raises(ValueError, match="pixel_fixed_params"):
        s.fit(np.linspace(0, 800, 8), np.ones((2, 8)), pixel_fixed_params={"D2": np.full(2, 1e-3)})
    with pytest.raises(ValueError, match="xdata"):  # shapes are checked before the device is looked for
        s.fit(np.linspace(0, 800, 8), np.ones((2, 7)))
    # what the TOML loader and the reference's solver arguments bring along is accepted; one exponential needs no threshold
    t = HipPeelSolver(MonoExpModel(), 100, 1e-6, weighting="none", device=1, io_dtype="float32", method="trf", multi_threading=True,
                      verbose=True, n_pools=4)
    assert (t.b_thresholds, t.weighting, t.device, t.io_dtype, t.verbose) == (None, "none", 1, np.float32, True)


P0 = {"f1": 0.2, "D1": 0.05, "D2": 1e-3, "S0": 1000.0}
BOUNDS = {"f1": (0.0, 1.0), "D1": (5e-3, 0.5), "D2": (1e-5, 5e-3), "S0": (1.0, 5000.0)}
PEEL = {"b_thresholds": [150.0], "weighting": "signal2"}


def _curvefit(model=None, **kw):
    return HipCurveFitSolver(model or BiExpModel(fit_s0=True), 250, 1e-8, p0=P0, bounds=BOUNDS, **kw)


def test_p0_peel_refusals_name_their_argument():
    s = _curvefit(p0_peel=PEEL)
    assert s.p0_peel == PEEL and _curvefit().p0_peel is None
    assert _curvefit(p0_peel={"b_thresholds": [150]}).p0_peel == PEEL  # the default weighting
    with pytest.raises(ValueError, match="p0_peel and p0_grid"):
        _curvefit(p0_peel=PEEL, p0_grid={"D1": [0.02, 0.05]})
    with pytest.raises(ValueError, match="p0_peel.*fixed"):
        _curvefit(BiExpModel(fit_s0=True, fixed_params={"D2": 1e-3}), p0_peel=PEEL)
    with pytest.raises(ValueError, match="p0_peel.*T1"):
        HipCurveFitSolver(BiExpModel(fit_s0=True, fit_t1=True, repetition_time=3000.0), 250, 1e-8, p0=dict(P0, T1=1000.0),
                          bounds=dict(BOUNDS, T1=(100.0, 5000.0)), p0_peel=PEEL)
    with pytest.raises(ValueError, match="p0_peel.*float64"):
        _curvefit(p0_peel=PEEL, precision="float32")
    with pytest.raises(ValueError, match="p0_peel.*float64"):
        _curvefit(p0_peel=PEEL, io_dtype="float32")
    with pytest.raises(ValueError, match="p0_peel.*b_thresholds"):
        _curvefit(p0_peel={"b_thresholds": [30, 250]})
    with pytest.raises(ValueError, match="p0_peel.*weighting"):
        _curvefit(p0_peel={"b_thresholds": [150], "weighting": "w"})
    with pytest.raises(ValueError, match="p0_peel must be a dict"):
        _curvefit(p0_peel={"b_thresholds": [150], "n_reweight": 1})
    tri = TriExpModel(fit_s0=True)
    names = api.MODEL_PARAM_NAMES["tri_s0"]
    with pytest.raises(ValueError, match="p0_peel.*HipConstrainedCurveFitSolver"):
        HipConstrainedCurveFitSolver(tri, p0={n: 0.1 for n in names}, bounds={n: (0.0, 1.0) for n in names},
                                     p0_peel={"b_thresholds": [30, 250]})
    # what only fit() can see
    b, y = np.linspace(0, 800, 8), np.ones((3, 8))
    with pytest.raises(ValueError, match="p0_peel.*per-voxel p0"):
        s.fit(b, y, p0=np.tile(np.array([P0[n] for n in P0])[:, None], (1, 3)))
    with pytest.raises(ValueError, match="p0_peel.*pixel_fixed_params"):
        s.fit(b, y, pixel_fixed_params={"D2": np.full(3, 1e-3)})
    lo = np.tile(np.array([BOUNDS[n][0] for n in P0])[:, None], (1, 3))
    hi = np.tile(np.array([BOUNDS[n][1] for n in P0])[:, None], (1, 3))
    with pytest.raises(ValueError, match="p0_peel.*shared bounds"):
        s.fit(b, y, bounds=(lo, hi))


def test_entry_point_line():
    text = open(os.path.join(ROOT, "pyproject.toml")).read()
    group = text.split('[project.entry-points."pyneapple.solvers"]')[1].split("[")[0]
    assert re.search(r'^hip_peel = "pyneapple_amd\.solvers:HipPeelSolver"$', group, flags=re.M)
    mod, cls = "pyneapple_amd.solvers:HipPeelSolver".split(":")
    assert getattr(__import__(mod, fromlist=[cls]), cls) is HipPeelSolver


def test_no_cpu_fallback_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is visible here")
    b, y = np.linspace(0, 800, 8), np.ones((4, 8))
    with pytest.raises(_lib.PnxError):
        api.peel(b, y, "bi_s0", b_thresholds=[150])
    with pytest.raises(_lib.PnxError):
        HipPeelSolver(BiExpModel(fit_s0=True), b_thresholds=[150]).fit(b, y)


# What the two numpy forms of the reference differ by on the parity signals (0.05 % noise), measured where this file was written:
# weighting 1 up to 2e-13 on the parameters at 16 b-values and beyond, weighting 0 up to 4e-9 (the logarithm of a small residual
# amplifies rounding).  The bars below are ten times those figures: a reference whose forms drift apart is caught here, before the
# GPU tests take a hundred times their difference as their bar.
@pytest.mark.parametrize("model,n_b", [("mono", 24), ("bi_s0", 16), ("bi_s0", 24), ("bi_s0", 128), ("tri_s0", 16), ("tri_s0", 24),
                                       ("tri_s0", 128), ("bi_s0", 4), ("bi_s0", 5), ("tri_s0", 6), ("tri_s0", 7)])
def test_reference_forms_agree_on_the_parity_signals(model, n_b):
    for weighting, bar in ((1, 2e-12), (0, 4e-8)):
        b, y, masks, lsq, d = parity_case(model, 129, n_b, weighting)  # asserts completeness and equal n_used itself
        print(f"peel reference forms {model} n_b={n_b} weighting={weighting}: params {d['params']:.2e} ss_res {d['ss_res']:.2e}")
        assert (lsq["status"] == 1).all() and (lsq["n_used"] >= 2).all() and lsq["n_used"].shape == (STAGES[model], 129)
        assert d["params"] <= bar, d
        assert np.isfinite(lsq["params"]).all() and np.isfinite(lsq["ss_res"]).all()


def test_reference_failure_rules():
    b, y, masks = signals("bi_s0", 6, 12, seed=1)
    y = y.copy()
    M = masks.any(axis=0)
    assert M.all()
    y[1, 3] = np.nan                      # inside M
    y[2, masks[1]] = 1e-3                 # far below the slow extrapolation: no positive residual
    for form in ("centred", "lstsq"):
        r = reference("bi_s0", b, y, masks, form=form)
        assert r["status"].tolist() == [1, -2, 0, 1, 1, 1]
        assert r["n_used"][:, 1].tolist() == [0, 0] and r["n_used"][0, 2] == masks[0].sum() and r["n_used"][1, 2] < 2
        assert np.isnan(r["params"][:, [1, 2]]).all() and np.isnan(r["ss_res"][[1, 2]]).all()
        f = reference("bi_s0", b, y, masks, fallback=[0.2, 0.05, 1e-3, 900.0], form=form)
        assert f["params"][:, 1].tolist() == f["params"][:, 2].tolist() == [0.2, 0.05, 1e-3, 900.0] and np.isnan(f["ss_res"][[1, 2]]).all()
        assert np.array_equal(f["params"][:, [0, 3, 4, 5]], r["params"][:, [0, 3, 4, 5]])


def test_argument_checks_are_clean_under_sanitizers(tmp_path):
    """pnx_peel_args.hpp (free of HIP types) under AddressSanitizer and UBSan, as a stand-alone program run directly: every refusal
    and a valid argument set for every layout and both storage types, on exact-size heap arrays."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "peel_args_stub")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "pyneapple_amd", "csrc"), os.path.join(ROOT, "tests", "host_stub", "peel_args_stub.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode and any(s in b.stderr for s in ("cannot find -lasan", "cannot find -lubsan")):
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-6000:]
    assert r.returncode == 0 and "peel args stub ok" in r.stdout, out[-4000:]

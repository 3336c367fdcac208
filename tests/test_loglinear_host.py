"""The log-linear mono-exponential fit (pnx_loglinear_f64 / _f32, HipLogLinearSolver), the parts that need no GPU: the ABI symbols,
their refusals in front of any device work, the solver's rules, the entry point, the segmented fitter's hand-over of the whole
image plus a b-value mask, and the host-side argument checks under AddressSanitizer / UBSan (a stand-alone program,
tests/host_stub/loglin_args_stub.cpp)."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT

from pyneapple_amd import _lib, api
from pyneapple_amd.models import BiExpModel, MonoExpModel
from pyneapple_amd.segmented import HipSegmentedFitter
from pyneapple_amd.solvers import HipLogLinearSolver

NAMES = ("pnx_loglinear_f64", "pnx_loglinear_f32")


def _call(fn="pnx_loglinear_f64", n_b=8, b=True, use=None, weighting=1, n_reweight=0, clip=0, lo=None, hi=None, y=True, params=True, mem=0):
    dt = np.float32 if fn.endswith("f32") else np.float64
    bv = (np.arange(max(n_b, 1)) * 50.0).astype(dt) if b is True else b
    yv, pv = np.ones(128, dt), np.zeros(2, dt)
    keep = [bv, use, lo, hi, yv, pv]  # alive across the call
    rc = getattr(_lib.load(), fn)(1, n_b, _lib.ptr(bv), _lib.ptr(use), weighting, n_reweight, clip, _lib.ptr(lo), _lib.ptr(hi),
                                  _lib.ptr(yv) if y else None, _lib.ptr(pv) if params else None, None, None, None, None, mem, 0, None)
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
    # the library's exports are the header's functions and nothing else
    declared = set(re.findall(r"PNX_API\s+int\s+(pnx_[a-z0-9_]+)\s*\(", text))
    exported = {s for s in out if s.startswith("pnx_")}
    assert exported == declared == set(_lib.ABI_SYMBOLS)


@pytest.mark.parametrize("fn", NAMES)
def test_abi_refusals_need_no_device(fn):
    """Every refusal comes back -1 with its argument named, before a device is touched: this runs on a machine without one."""
    dt = np.float32 if fn.endswith("f32") else np.float64
    err = _lib.last_error
    for n_b in (-1, 0, 1, 129):
        assert _call(fn, n_b=n_b) == -1 and "n_b" in err()
    assert _call(fn, b=None) == -1 and "b is NULL" in err()
    assert _call(fn, y=False) == -1 and "y is NULL" in err()
    assert _call(fn, params=False) == -1 and "params is NULL" in err()
    for bad in (np.nan, np.inf):
        b = (np.arange(8) * 50.0).astype(dt)
        b[5] = bad
        assert _call(fn, b=b) == -1 and "b[5]" in err()
    for w in (-1, 2):
        assert _call(fn, weighting=w) == -1 and "weighting" in err()
    for r in (-1, 9):
        assert _call(fn, n_reweight=r) == -1 and "n_reweight" in err()
    one = np.zeros(8, np.uint8)
    one[3] = 1
    assert _call(fn, use=one) == -1 and "use" in err()
    assert _call(fn, use=np.zeros(8, np.uint8)) == -1 and "use" in err()
    two = one.copy()
    two[6] = 1
    b = (np.arange(8) * 50.0).astype(dt)
    b[6] = b[3]
    assert _call(fn, b=b, use=two) == -1 and "distinct" in err()
    assert _call(fn, b=np.full(8, 100.0, dt)) == -1 and "distinct" in err()
    lo, hi = np.array([1.0, 1e-5], dt), np.array([5000.0, 0.1], dt)
    assert _call(fn, clip=1) == -1 and "lo" in err()
    assert _call(fn, clip=1, lo=lo) == -1 and "hi" in err()
    assert _call(fn, clip=1, lo=lo, hi=np.array([5000.0, 1e-5], dt)) == -1 and "lo[1]" in err()
    assert _call(fn, clip=1, lo=np.array([6000.0, 1e-5], dt), hi=hi) == -1 and "lo[0]" in err()
    for mem in (-1, 2):
        assert _call(fn, mem=mem) == -1 and "mem" in err()
    if _lib.device_count() == 0:  # fully valid calls stop at the device, and only there
        assert _call(fn) == -3
        assert _call(fn, use=two, weighting=0, n_reweight=8, clip=1, lo=lo, hi=hi, mem=1) == -3
        assert _call(fn, n_b=2) == -3 and _call(fn, n_b=128) == -3


def test_solver_rules():
    with pytest.raises(ValueError, match="BiExpModel"):
        HipLogLinearSolver(BiExpModel())
    with pytest.raises(ValueError, match="MonoExpModel.*fixed"):
        HipLogLinearSolver(MonoExpModel(fixed_params={"S0": 1000.0}))
    with pytest.raises(ValueError, match="T1"):
        HipLogLinearSolver(MonoExpModel(fit_t1=True, repetition_time=3000.0))
    with pytest.raises(ValueError, match="bounds"):
        HipLogLinearSolver(MonoExpModel(), clip=True)
    with pytest.raises(ValueError, match="weighting"):
        HipLogLinearSolver(MonoExpModel(), weighting="signal")
    with pytest.raises(ValueError, match="n_reweight"):
        HipLogLinearSolver(MonoExpModel(), n_reweight=9)
    with pytest.raises(ValueError, match="Missing"):
        HipLogLinearSolver(MonoExpModel(), p0={"S0": 1000.0})
    with pytest.raises(ValueError, match="Missing"):
        HipLogLinearSolver(MonoExpModel(), clip=True, bounds={"D": (1e-5, 0.1)})
    s = HipLogLinearSolver(MonoExpModel())
    with pytest.raises(ValueError, match="pixel_fixed_params"):
        s.fit(np.linspace(0, 800, 8), np.ones((2, 8)), pixel_fixed_params={"D": np.full(2, 1e-3)})
    with pytest.raises(ValueError, match="xdata"):  # shapes are checked before the device is looked for
        s.fit(np.linspace(0, 800, 8), np.ones((2, 7)))


def test_defaults_of_a_plainly_constructed_solver():
    s = HipLogLinearSolver(MonoExpModel())
    assert (s.max_iter, s.tol, s.p0, s.bounds, s.weighting, s.n_reweight, s.clip, s.device, s.io_dtype) == \
        (250, 1e-8, None, None, "signal2", 0, False, 0, np.float64)
    assert s.supports_bvalue_mask is True and HipLogLinearSolver.supports_bvalue_mask is True
    assert s.params_ == {} and s.diagnostics_ == {} and len(s.pixel_results_) == 0
    # what the TOML loader and the reference's solver arguments bring along is accepted
    t = HipLogLinearSolver(MonoExpModel(), 100, 1e-6, p0={"S0": 900.0, "D": 1e-3}, bounds={"S0": (1.0, 5e3), "D": (1e-5, 0.1)},
                           weighting="none", n_reweight=2, clip=True, device=1, io_dtype="float32", method="trf", multi_threading=True,
                           verbose=True, n_pools=4)
    assert (t.weighting, t.n_reweight, t.clip, t.device, t.io_dtype, t.verbose) == ("none", 2, True, 1, np.float32, True)


def test_entry_point_line():
    text = open(os.path.join(ROOT, "pyproject.toml")).read()
    group = text.split('[project.entry-points."pyneapple.solvers"]')[1].split("[")[0]
    assert re.search(r'^hip_loglinear = "pyneapple_amd\.solvers:HipLogLinearSolver"$', group, flags=re.M)
    mod, cls = "pyneapple_amd.solvers:HipLogLinearSolver".split(":")
    assert getattr(__import__(mod, fromlist=[cls]), cls) is HipLogLinearSolver


def test_no_cpu_fallback_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is visible here")
    b, y = np.linspace(0, 800, 8), np.ones((4, 8))
    with pytest.raises(_lib.PnxError):
        api.loglinear(b, y)
    with pytest.raises(_lib.PnxError):
        HipLogLinearSolver(MonoExpModel()).fit(b, y)


class _FakeSolver:
    """Records what the fitter hands it and answers with constants."""

    def __init__(self, model, with_mask):
        self.model = model
        if with_mask:
            self.supports_bvalue_mask = True
        self.calls = []
        self.params_, self.diagnostics_, self.pixel_results_ = {}, {}, None

    def fit(self, xdata, ydata, pixel_fixed_params=None, **kw):
        self.calls.append(dict(xdata=np.array(xdata), shape=ydata.shape, ydata=np.array(ydata), kw=kw))
        self.params_ = {n: np.full(ydata.shape[0], 1.0 if n == "S0" else 0.5 if n.startswith("f") else 1e-3) for n in self.model.param_names}
        return self


def test_segmented_fitter_hands_a_masking_solver_the_whole_image():
    b = np.array([0.0, 50.0, 100.0, 200.0, 400.0, 600.0, 800.0])
    rng = np.random.default_rng(5)
    image = rng.uniform(0.5, 1.5, (3, 2, 2, b.size))
    keep = b >= 200
    # a step-1 solver that takes a mask: the full last axis plus the mask, no slicing
    s1, s2 = _FakeSolver(MonoExpModel(), True), _FakeSolver(BiExpModel(), False)
    f = HipSegmentedFitter(s1, s2, step1_bvalue_range=(200, None)).fit(b, image)
    (c1,), (c2,) = s1.calls, s2.calls
    assert c1["shape"] == (12, b.size) and np.array_equal(c1["xdata"], b)
    assert np.array_equal(np.asarray(c1["kw"]["bvalue_mask"], bool), keep)
    assert np.array_equal(c1["ydata"], image.reshape(-1, b.size))
    assert c2["shape"] == (12, b.size) and "bvalue_mask" not in c2["kw"]  # step 2 fits every b-value, as before
    assert set(f.step1_params_) == {"S0", "D"} and f.results_ is not None
    # R^2 of step 1 runs over the masked-in measurements: the constant answer S0 = 1, D = 1e-3 against the kept columns
    rows = image.reshape(-1, b.size)[:, keep]
    ss_res = ((rows - np.exp(-b[keep] * 1e-3)) ** 2).sum(axis=1)
    ss_tot = ((rows - rows.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)
    np.testing.assert_allclose(f.step1_result_.r_squared, 1.0 - ss_res / ss_tot, rtol=1e-12)
    # a step-1 solver without the attribute: the sliced image and the sliced b-values, as before
    o1, o2 = _FakeSolver(MonoExpModel(), False), _FakeSolver(BiExpModel(), False)
    HipSegmentedFitter(o1, o2, step1_bvalue_range=(200, None)).fit(b, image)
    (d1,) = o1.calls
    assert d1["shape"] == (12, int(keep.sum())) and np.array_equal(d1["xdata"], b[keep]) and "bvalue_mask" not in d1["kw"]
    assert np.array_equal(d1["ydata"], image.reshape(-1, b.size)[:, keep])
    # the >= 3 b-values rule holds on both paths
    for solver in (_FakeSolver(MonoExpModel(), True), _FakeSolver(MonoExpModel(), False)):
        with pytest.raises(ValueError, match="at least 3"):
            HipSegmentedFitter(solver, _FakeSolver(BiExpModel(), False), step1_bvalue_range=(600, None)).fit(b, image)


def test_pixelwise_fitter_assembles_a_masked_loglinear_result(monkeypatch):
    """HipPixelWiseFitter on a solver that reports ss_res instead of cost: R^2 from the solver's signal-domain residual and SS_tot
    over the masked-in columns; a failed voxel (status 0, parameters p0) gets the model's residual at p0 over those columns."""
    from pyneapple_amd.fitters import HipPixelWiseFitter

    b = np.array([0.0, 100.0, 200.0, 400.0, 800.0])
    keep = b >= 100
    rng = np.random.default_rng(2)
    rows = 1000.0 * np.exp(-b * 1.2e-3) * (1 + 0.01 * rng.standard_normal((6, b.size)))
    want = dict(params=np.stack([np.full(6, 1000.0), np.full(6, 1.2e-3)]), pcov=np.full((6, 2, 2), 1.0), status=np.ones(6, np.int8),
                n_used=np.full(6, 4, np.int32), ss_res=np.arange(6) + 1.0)
    want["status"][4] = 0
    want["params"][:, 4] = np.nan
    want["ss_res"][4] = np.nan
    seen = {}

    def fake(bb, y, **kw):
        seen.update(kw, b=bb, y=y)
        return {k: v.copy() for k, v in want.items()}

    monkeypatch.setattr(api, "loglinear", fake)
    s = HipLogLinearSolver(MonoExpModel(), p0={"S0": 900.0, "D": 1e-3})
    f = HipPixelWiseFitter(s).fit(b, rows.reshape(6, 1, 1, b.size), bvalue_mask=keep)
    assert seen["y"].shape == (6, b.size) and np.array_equal(seen["bvalue_mask"], keep) and seen["clip"] is None
    assert (s.params_["S0"][4], s.params_["D"][4]) == (900.0, 1e-3) and s.params_["S0"][0] == 1000.0
    assert [r.success for r in s.pixel_results_] == [True, True, True, True, False, True]
    assert "usable" in s.pixel_results_[4].message and s.pixel_results_[0].message is None
    assert set(s.diagnostics_) == {"pcov", "n_pixels", "status", "n_used", "ss_res"}
    sub = rows[:, keep]
    ss_tot = ((sub - sub.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)
    ss_res = want["ss_res"].copy()
    ss_res[4] = ((900.0 * np.exp(-b[keep] * 1e-3) - sub[4]) ** 2).sum()
    np.testing.assert_allclose(f.results_.r_squared, 1.0 - ss_res / ss_tot, rtol=1e-12)
    assert list(f.results_.success) == [True, True, True, True, False, True]


def test_argument_checks_are_clean_under_sanitizers(tmp_path):
    """pnx_loglin_args.hpp (free of HIP types) under AddressSanitizer and UBSan, as a stand-alone program run directly: every
    refusal and a valid argument set for both storage types, on exact-size heap arrays."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "loglin_args_stub")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "pyneapple_amd", "csrc"), os.path.join(ROOT, "tests", "host_stub", "loglin_args_stub.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode and any(s in b.stderr for s in ("cannot find -lasan", "cannot find -lubsan")):
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-6000:]
    assert r.returncode == 0 and "loglin args stub ok" in r.stdout, out[-4000:]

"""The dictionary search for per-voxel start values, the parts that need no GPU: the ABI symbol, its refusals in front of any
device work, the solver's p0_grid rules, and the host-side argument checks under AddressSanitizer / UBSan (a stand-alone
program, tests/host_stub/grid_args_stub.cpp)."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT

from pyneapple_amd import _lib, api, synth
from pyneapple_amd.models import BiExpModel, MonoExpModel, TriExpModel
from pyneapple_amd.solvers import HipConstrainedCurveFitSolver, HipCurveFitSolver

NAME = "pnx_curvefit_grid_start_f64"


def _call(o, n_atoms=4, atoms=None, lo=None, hi=None, project=0, p0_out=True, fixed=None):
    n = o.n_free
    atoms = np.full((n, max(n_atoms, 1)), 0.5) if atoms is None else np.ascontiguousarray(atoms, float)
    lo = np.zeros(n) if lo is None else np.asarray(lo, float)
    hi = np.ones(n) if hi is None else np.asarray(hi, float)
    b, y, out = np.zeros(128), np.ones(128), np.zeros(8)
    return _lib.load().pnx_curvefit_grid_start_f64(C.byref(o), 1, _lib.ptr(b), _lib.ptr(y), n_atoms, _lib.ptr(atoms), fixed, _lib.ptr(lo),
                                                   _lib.ptr(hi), project, _lib.ptr(out) if p0_out else None, None, None, 0, 0, None)


def test_symbol_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnx.h")).read(), flags=re.S)
    assert re.search(r"PNX_API\s+int\s+" + NAME + r"\s*\(", text)
    assert NAME in _lib.ABI_SYMBOLS
    fn = getattr(_lib.load(), NAME)
    assert len(fn.argtypes) == 16 and fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NAME in out.split()


def test_abi_refusals_need_no_device():
    """Every refusal comes back from the library before a device is touched: this runs on a machine without one."""
    mk = api.make_opts
    for n_atoms in (0, 4097):
        assert _call(mk("bi_reduced", 32), n_atoms=n_atoms) == -1 and "n_atoms" in _lib.last_error()
    o = mk("bi_reduced", 32)
    o.n_b = 129
    assert _call(o) == -1 and "n_b" in _lib.last_error()
    assert _call(mk("bi_reduced", 32), p0_out=False) == -1 and "NULL" in _lib.last_error()
    assert _call(mk("bi_reduced", 32), project=1) == -1 and "S0" in _lib.last_error()
    for model in ("bi_full", "tri_reduced", "tri_full"):
        assert _call(mk(model, 32), project=1) == -1 and "S0" in _lib.last_error()
    # S0 exists but is fixed: nothing to project
    assert _call(mk("bi_s0", 32, fixed_idx=[3], jac="analytic"), project=1, fixed=_lib.ptr(np.ones(1))) == -1 and "S0" in _lib.last_error()
    atoms = np.full((3, 4), 0.5)
    atoms[1, 2] = 1.5
    assert _call(mk("bi_reduced", 32), atoms=atoms) == -1
    assert "atom 2" in _lib.last_error() and "parameter 1" in _lib.last_error()
    atoms[1, 2] = np.nan
    assert _call(mk("bi_reduced", 32), atoms=atoms) == -1 and "atom 2" in _lib.last_error()
    assert _call(mk("bi_reduced", 32, per_voxel=True)) == -2 and "per_voxel_p0_bounds" in _lib.last_error()
    assert _call(mk("bi_reduced", 32, fixed_idx=[1], fixed_per_voxel=True, jac="analytic"), fixed=_lib.ptr(np.ones(1))) == -2
    assert "fixed_per_voxel" in _lib.last_error()
    o = mk("bi_reduced", 32)
    o.queue_order = np.zeros(4, np.int32).ctypes.data
    assert _call(o) == -2 and "queue_order" in _lib.last_error()
    o = mk("tri_reduced", 32)
    o.n_free = 3  # inconsistent with the model, as pnx_curvefit_batch_f64 reports it
    assert _call(o) == -1 and "n_free" in _lib.last_error()
    # the Jacobian mode is not looked at: FD with a fixed parameter is the fit's refusal, not the search's
    if _lib.device_count() == 0:
        assert _call(mk("bi_reduced", 32, fixed_idx=[1], jac="analytic"), fixed=_lib.ptr(np.ones(1))) == -3  # valid: stops at the device


def _tri():
    names, p0, lo, hi = synth.shared_arrays("tri_reduced")
    return dict(p0=dict(zip(names, map(float, p0))), bounds={n: (float(a), float(b)) for n, a, b in zip(names, lo, hi)})


def _solver(model=None, **kw):
    return HipCurveFitSolver(model or TriExpModel(), 250, 1e-8, **{**_tri(), **kw})


def test_solver_builds_the_cartesian_product_in_parameter_order():
    s = _solver(p0_grid={"D3": [1e-3, 5e-4, 2e-4], "f1": [0.1, 0.2]})  # the dict's own order does not matter
    assert s._p0_atoms.shape == (5, 6) and s._p0_atoms.flags.c_contiguous
    # model.param_names order [f1, D1, f2, D2, D3], the last parameter fastest; unnamed parameters take the scalar p0
    want = [[f1, 0.05, 0.3, 0.005, d3] for f1 in (0.1, 0.2) for d3 in (1e-3, 5e-4, 2e-4)]
    np.testing.assert_array_equal(s._p0_atoms.T, np.array(want))
    assert s.p0_grid == {"D3": [1e-3, 5e-4, 2e-4], "f1": [0.1, 0.2]}
    one = _solver(p0_grid={"D1": 0.1})  # a scalar is a sequence of one
    assert one._p0_atoms.shape == (5, 1)


def test_solver_refuses_bad_grids():
    with pytest.raises(ValueError, match="4097 atoms"):
        _solver(p0_grid={"f1": np.linspace(0.1, 0.9, 17), "f2": np.linspace(0.1, 0.9, 241)})
    assert _solver(p0_grid={"f1": np.linspace(0.1, 0.9, 16), "f2": np.linspace(0.1, 0.9, 256)})._p0_atoms.shape == (5, 4096)
    with pytest.raises(ValueError, match="f3"):
        _solver(p0_grid={"f3": [0.1]})
    with pytest.raises(ValueError, match="D3"):
        _solver(model=TriExpModel(fixed_params={"D3": 1e-3}), p0_grid={"D3": [1e-3]})  # fixed: not a fitted parameter
    with pytest.raises(ValueError, match="outside the bounds"):
        _solver(p0_grid={"D2": [0.005, 0.02]})  # bounds of D2: (2e-3, 0.01)
    with pytest.raises(ValueError, match="outside the bounds"):
        _solver(p0_grid={"D2": [float("nan")]})
    with pytest.raises(ValueError, match="dict"):
        _solver(p0_grid=[0.1, 0.2])
    with pytest.raises(ValueError, match="float64"):
        _solver(p0_grid={"f1": [0.1]}, precision="float32")
    with pytest.raises(ValueError, match="float64"):
        _solver(p0_grid={"f1": [0.1]}, io_dtype="float32")
    with pytest.raises(ValueError, match="p0_grid"):
        _solver(p0_grid_project=True)
    for kw in (dict(p0_grid={"f1": [0.1]}), dict(p0_grid={"f1": [0.1]}, fraction_constraint=False)):
        with pytest.raises(ValueError, match="constraint"):
            HipConstrainedCurveFitSolver(TriExpModel(), **_tri(), **kw)


def test_projection_default_follows_the_model():
    t = _tri()
    s0 = dict(p0={**t["p0"], "S0": 900.0}, bounds={**t["bounds"], "S0": (1.0, 5000.0)})
    assert _solver(p0_grid={"f1": [0.1]}).p0_grid_project is False
    assert HipCurveFitSolver(TriExpModel(fit_s0=True), 250, 1e-8, **s0, p0_grid={"f1": [0.1]}).p0_grid_project is True
    assert HipCurveFitSolver(TriExpModel(fit_s0=True), 250, 1e-8, **s0, p0_grid={"f1": [0.1]}, p0_grid_project=False).p0_grid_project is False
    bi = dict(p0={"f1": 0.2, "D1": 0.01, "D2": 0.001, "S0": 900.0}, bounds={"f1": (0, 1), "D1": (1e-3, 0.1), "D2": (1e-5, 5e-3), "S0": (1.0, 5000.0)})
    assert HipCurveFitSolver(BiExpModel(fit_s0=True), 250, 1e-8, **bi, p0_grid={"D1": [0.01, 0.05]}).p0_grid_project is True
    fixed = HipCurveFitSolver(BiExpModel(fit_s0=True, fixed_params={"S0": 900.0}), 250, 1e-8, p0={k: v for k, v in bi["p0"].items() if k != "S0"},
                              bounds={k: v for k, v in bi["bounds"].items() if k != "S0"}, p0_grid={"D1": [0.01, 0.05]})
    assert fixed.p0_grid_project is False  # S0 exists but is not free
    mono = dict(p0={"S0": 1000.0, "D": 1e-3}, bounds={"S0": (1.0, 5000.0), "D": (1e-5, 0.1)})
    assert HipCurveFitSolver(MonoExpModel(), 250, 1e-8, **mono, p0_grid={"D": [1e-3, 2e-3]}).p0_grid_project is True
    with pytest.raises(ValueError, match="S0"):
        _solver(p0_grid={"f1": [0.1]}, p0_grid_project=True)


def test_fit_refuses_per_pixel_fixed_parameters_and_per_voxel_bounds():
    s = _solver(p0_grid={"f1": [0.1, 0.2]})
    b, y = np.linspace(0, 1200, 32), np.ones((2, 32))
    with pytest.raises(ValueError, match="per-pixel fixed"):
        s.fit(b, y, pixel_fixed_params={"D3": np.full(2, 1e-3)})
    names, p0, lo, hi = synth.shared_arrays("tri_reduced")
    with pytest.raises(ValueError, match="shared bounds"):
        s.fit(b, y, bounds=(np.repeat(lo[:, None], 2, 1), np.repeat(hi[:, None], 2, 1)))


def test_a_solver_without_p0_grid_is_constructed_as_before():
    s = _solver()
    assert s.p0_grid is None and s._p0_atoms is None and s.p0_grid_project is False
    assert (s.precision, s.io_dtype, s.jacobian_mode, s.xtol, s.gtol, s.sigma) == ("float64", np.float64, "fd", 1e-8, 1e-8, None)
    assert _solver(p0_grid=None)._p0_atoms is None
    with pytest.raises(ValueError, match="p0_grid, p0_grid_project"):
        _solver(no_such_argument=1)  # the supported list names the two new keys
    f = _solver(precision="float32")  # still constructible without a grid
    assert f.precision == "float32" and f._p0_atoms is None


def test_no_cpu_fallback_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is visible here")
    b, y, _ = synth.make_numpy("tri_reduced", 4, 32)
    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    with pytest.raises(_lib.PnxError):
        api.grid_start("tri_reduced", b, y, p0[:, None], lo, hi)
    with pytest.raises(_lib.PnxError):
        _solver(p0_grid={"f1": [0.1, 0.2]}).fit(b, y)


def test_argument_checks_are_clean_under_sanitizers(tmp_path):
    """pnx_grid_args.hpp (free of HIP types) under AddressSanitizer and UBSan, as a stand-alone program: the bounds check reads
    exactly n_free * n_atoms atoms, and the slab sizing stays inside the LDS budget for every n_b."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "grid_args_stub")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "pyneapple_amd", "csrc"), os.path.join(ROOT, "tests", "host_stub", "grid_args_stub.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode and any(s in b.stderr for s in ("cannot find -lasan", "cannot find -lubsan")):
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-6000:]
    assert r.returncode == 0 and "grid args stub ok" in r.stdout, out[-4000:]

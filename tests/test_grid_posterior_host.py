"""The Bayesian grid posterior (pnx_curvefit_grid_posterior_f64, api.grid_posterior, HipBayesGridSolver), the parts that need no
GPU: the host-side argument checks under AddressSanitizer / UBSan (a stand-alone program,
tests/host_stub/grid_posterior_args_stub.cpp), the ABI's refusals in front of any device work, the solver's construction rules,
the atoms of p0_grid after the refactor, and the numpy oracle itself against a brute-force posterior."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT
from grid_posterior_reference import reference
from grid_start_reference import signals

from pyneapple_amd import _lib, api, synth
from pyneapple_amd.models import BiExpModel, TriExpModel
from pyneapple_amd.solvers import HipBayesGridSolver, HipCurveFitSolver

NAME = "pnx_curvefit_grid_posterior_f64"


# ---- the argument checks as a stand-alone program under the sanitizers
@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("stub") / "grid_posterior_args_stub")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "pyneapple_amd", "csrc"), os.path.join(ROOT, "tests", "host_stub", "grid_posterior_args_stub.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode and any(s in b.stderr for s in ("cannot find -lasan", "cannot find -lubsan")):
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-4000:]
    return exe


def _run_stub(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-6000:]
    assert r.returncode == 0, out[-4000:]
    return r.stdout


def test_argument_checks_are_clean_under_sanitizers(stub):
    """Every invalid argument refused by name, the valid edges accepted (all but one prior at -inf, noise_sd = 0, 1 and 4096 atoms),
    the normaliser and the centres right, the slab inside the LDS budget for every (n_b, n_free)."""
    assert "grid posterior args stub ok" in _run_stub(stub)


@pytest.mark.parametrize("n_b,n_free", [(1, 1), (16, 5), (32, 5), (32, 8), (64, 3), (65, 6), (128, 8)])
def test_python_slab_width_is_the_kernels(stub, n_b, n_free):
    assert int(_run_stub(stub, n_b, n_free)) == api.grid_posterior_slab_atoms(n_b, n_free)


# ---- the ABI without a device
def _call(o, n_atoms=4, atoms=None, log_prior=None, noise_sd=0.0, project=0, mean=True):
    n = o.n_free
    atoms = np.full((n, max(n_atoms, 1)), 0.5) if atoms is None else np.ascontiguousarray(atoms, float)
    lo, hi = np.zeros(n), np.ones(n)
    b, y, out = np.zeros(128), np.ones(128), np.zeros(8)
    lp = None if log_prior is None else np.ascontiguousarray(log_prior, float)
    return _lib.load().pnx_curvefit_grid_posterior_f64(C.byref(o), 1, _lib.ptr(b), _lib.ptr(y), n_atoms, _lib.ptr(atoms), None, _lib.ptr(lo),
                                                       _lib.ptr(hi), project, _lib.ptr(lp), noise_sd, _lib.ptr(out) if mean else None, None, None,
                                                       None, None, None, 0, 0, None)


def test_symbol_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnx.h")).read(), flags=re.S)
    assert re.search(r"PNX_API\s+int\s+" + NAME + r"\s*\(", text)
    assert NAME in _lib.ABI_SYMBOLS
    fn = getattr(_lib.load(), NAME)
    assert len(fn.argtypes) == 21 and fn.restype is C.c_int
    assert _lib.load().pnx_version() == 2


def test_abi_refusals_need_no_device():
    mk = api.make_opts
    for bad in (-1.0, float("nan"), float("inf")):
        assert _call(mk("bi_reduced", 32), noise_sd=bad) == -1 and "noise_sd" in _lib.last_error()
    for prior in ([0.0, np.nan, 0.0, 0.0], [0.0, np.inf, 0.0, 0.0], [-np.inf] * 4):
        assert _call(mk("bi_reduced", 32), log_prior=prior) == -1 and "log_prior" in _lib.last_error()
    assert _call(mk("bi_reduced", 32), mean=False) == -1 and "mean" in _lib.last_error()
    for n_atoms in (0, 4097):
        assert _call(mk("bi_reduced", 32), n_atoms=n_atoms) == -1 and "n_atoms" in _lib.last_error()
    assert _call(mk("bi_reduced", 32), project=1) == -1 and "S0" in _lib.last_error()
    atoms = np.full((3, 4), 0.5)
    atoms[1, 2] = 1.5
    assert _call(mk("bi_reduced", 32), atoms=atoms) == -1 and "atom 2" in _lib.last_error()
    assert _call(mk("bi_reduced", 32, per_voxel=True)) == -2 and "per_voxel_p0_bounds" in _lib.last_error()
    o = mk("bi_reduced", 32)
    o.queue_order = np.zeros(4, np.int32).ctypes.data
    assert _call(o) == -2 and "queue_order" in _lib.last_error()
    if _lib.device_count() == 0:  # valid calls stop at the device
        assert _call(mk("bi_reduced", 32), log_prior=[-np.inf, -np.inf, -1.0, -np.inf]) == -3
        assert _call(mk("bi_s0", 32), project=1, noise_sd=0.02) == -3


def test_no_cpu_fallback_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is visible here")
    b, y, _ = synth.make_numpy("tri_reduced", 4, 32)
    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    with pytest.raises(_lib.PnxError):
        api.grid_posterior("tri_reduced", b, y, p0[:, None], lo, hi)
    with pytest.raises(_lib.PnxError):
        _solver(grid={"f1": [0.1, 0.2]}).fit(b, y)


def test_api_refuses_a_wrong_prior_length_and_per_voxel_fixed_maps(monkeypatch):
    monkeypatch.setattr(_lib, "require_device", lambda: None)
    b, y, _ = synth.make_numpy("tri_reduced", 4, 32)
    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    with pytest.raises(ValueError, match="log_prior"):
        api.grid_posterior("tri_reduced", b, y, p0[:, None], lo, hi, log_prior=np.zeros(2))
    with pytest.raises(ValueError, match="per-voxel fixed"):
        api.grid_posterior("tri_reduced", b, y, p0[[0, 1, 2, 4], None], lo[[0, 1, 2, 4]], hi[[0, 1, 2, 4]], fixed_idx=[3], fixed_vals=np.ones((1, 4)))


# ---- the solver's construction rules
def _tri():
    names, p0, lo, hi = synth.shared_arrays("tri_reduced")
    return dict(p0=dict(zip(names, map(float, p0))), bounds={n: (float(a), float(b)) for n, a, b in zip(names, lo, hi)})


def _solver(model=None, **kw):
    return HipBayesGridSolver(model or TriExpModel(), **{**_tri(), **kw})


def test_solver_grid_rules_are_p0_grids():
    s = _solver(grid={"D3": [1e-3, 5e-4, 2e-4], "f1": [0.1, 0.2]})
    c = HipCurveFitSolver(TriExpModel(), 250, 1e-8, **_tri(), p0_grid={"D3": [1e-3, 5e-4, 2e-4], "f1": [0.1, 0.2]})
    assert s._atoms.tobytes() == c._p0_atoms.tobytes() and s._atoms.shape == (5, 6)
    assert s.grid == c.p0_grid and s.project is False and s.noise_sd == 0.0 and s.log_prior is None
    grids = [({"f1": np.linspace(0.1, 0.9, 17), "f2": np.linspace(0.1, 0.9, 241)}, "4097 atoms"), ({"f3": [0.1]}, "f3"),
             ({"D2": [0.005, 0.02]}, "outside the bounds"), ({"D2": [float("nan")]}, "outside the bounds"), ([0.1, 0.2], "dict")]
    for grid, text in grids:  # the same refusal, worded alike, from both classes
        with pytest.raises(ValueError, match=text) as e1:
            _solver(grid=grid)
        with pytest.raises(ValueError, match=text) as e2:
            HipCurveFitSolver(TriExpModel(), 250, 1e-8, **_tri(), p0_grid=grid)
        assert str(e1.value).replace("grid", "p0_grid", 1) == str(e2.value)
    assert _solver(grid={"f1": np.linspace(0.1, 0.9, 16), "f2": np.linspace(0.1, 0.9, 256)})._atoms.shape == (5, 4096)
    with pytest.raises(ValueError, match="D3"):
        _solver(model=TriExpModel(fixed_params={"D3": 1e-3}), grid={"D3": [1e-3]})
    with pytest.raises(ValueError, match="grid is required"):
        HipBayesGridSolver(TriExpModel(), **_tri())
    with pytest.raises(ValueError, match="D3"):  # not in the grid, not in p0
        HipBayesGridSolver(TriExpModel(), {"f1": [0.1]}, p0={k: v for k, v in _tri()["p0"].items() if k != "D3"}, bounds=_tri()["bounds"])
    # the TOML loader's call: max_iter, tol, p0 by keyword, the reference's other keys ignored
    t = HipBayesGridSolver(TriExpModel(), {"f1": [0.1, 0.2]}, max_iter=100, tol=1e-6, **_tri(), method="trf", multi_threading=True, verbose=True)
    assert t._atoms.shape == (5, 2) and t.solver_kwargs == {"method": "trf", "multi_threading": True}


def test_solver_prior_noise_and_projection_rules():
    with pytest.raises(ValueError, match="log_prior"):
        _solver(grid={"f1": [0.1, 0.2]}, log_prior=np.zeros(3))
    with pytest.raises(ValueError, match="log_prior"):
        _solver(grid={"f1": [0.1, 0.2]}, log_prior=[-np.inf, -np.inf])
    with pytest.raises(ValueError, match="log_prior"):
        _solver(grid={"f1": [0.1, 0.2]}, log_prior=[0.0, np.nan])
    assert _solver(grid={"f1": [0.1, 0.2]}, log_prior=[0.0, -np.inf]).log_prior.tolist() == [0.0, -np.inf]
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="noise_sd"):
            _solver(grid={"f1": [0.1]}, noise_sd=bad)
    assert _solver(grid={"f1": [0.1]}, noise_sd=0.03).noise_sd == 0.03
    with pytest.raises(ValueError, match="S0"):
        _solver(grid={"f1": [0.1]}, project=True)
    bi = dict(p0={"f1": 0.2, "D1": 0.01, "D2": 0.001, "S0": 900.0}, bounds={"f1": (0, 1), "D1": (1e-3, 0.1), "D2": (1e-5, 5e-3), "S0": (1.0, 5000.0)})
    assert HipBayesGridSolver(BiExpModel(fit_s0=True), {"D1": [0.01, 0.05]}, **bi).project is True
    assert HipBayesGridSolver(BiExpModel(fit_s0=True), {"D1": [0.01, 0.05]}, **bi, project=False).project is False


def test_solver_refuses_what_the_kernel_does_not_take():
    for kw in (dict(io_dtype="float32"), dict(precision="float32")):
        with pytest.raises(ValueError, match="float64"):
            _solver(grid={"f1": [0.1]}, **kw)
    s = _solver(grid={"f1": [0.1, 0.2]})
    with pytest.raises(ValueError, match="per-pixel fixed"):
        s.fit(np.linspace(0, 1200, 32), np.ones((2, 32)), pixel_fixed_params={"D3": np.full(2, 1e-3)})
    with pytest.raises(ValueError, match="sigma"):
        _solver(grid={"f1": [0.1]}, sigma=np.ones((4, 4)))


def test_entry_point_is_registered():
    text = open(os.path.join(ROOT, "pyproject.toml")).read()
    group = text.split('[project.entry-points."pyneapple.solvers"]', 1)[1].split("\n[", 1)[0]
    assert re.search(r'^hip_bayes_grid = "pyneapple_amd\.solvers:HipBayesGridSolver"$', group, flags=re.M)
    mod, cls = "pyneapple_amd.solvers:HipBayesGridSolver".split(":")
    assert getattr(__import__(mod, fromlist=[cls]), cls) is HipBayesGridSolver


def test_p0_grid_builds_the_atoms_it_built_before_the_refactor():
    s = HipCurveFitSolver(BiExpModel(), 250, 1e-8, p0={"f1": 0.25, "D1": 0.05, "D2": 1e-3},
                          bounds={"f1": (0.0, 1.0), "D1": (1e-3, 0.5), "D2": (1e-5, 5e-3)}, p0_grid={"D2": [2e-3, 5e-4], "f1": [0.1, 0.3, 0.5]})
    want = np.array([[0.1, 0.1, 0.3, 0.3, 0.5, 0.5], [0.05] * 6, [2e-3, 5e-4, 2e-3, 5e-4, 2e-3, 5e-4]])
    assert s._p0_atoms.dtype == np.float64 and s._p0_atoms.flags.c_contiguous and s._p0_atoms.tobytes() == want.tobytes()
    assert s.p0_grid == {"D2": [2e-3, 5e-4], "f1": [0.1, 0.3, 0.5]} and s.p0_grid_project is False


# ---- the oracle itself
@pytest.mark.parametrize("noise_sd", [0.0, 0.05])
def test_reference_against_a_brute_force_posterior(noise_sd):
    """4 voxels, 5 atoms, a non-uniform prior: the helper's outputs are the three-line textbook posterior."""
    rng = np.random.default_rng(5)
    b = np.array([0.0, 50.0, 200.0, 800.0])
    atoms = np.stack([rng.uniform(0.1, 0.4, 5), rng.uniform(0.02, 0.1, 5), rng.uniform(5e-4, 2e-3, 5)])
    truth = np.stack([rng.uniform(0.1, 0.4, 4), rng.uniform(0.02, 0.1, 4), rng.uniform(5e-4, 2e-3, 4)])
    y = signals("bi_reduced", b, truth) * (1 + 0.03 * rng.standard_normal((4, 4)))
    lp = np.log(rng.uniform(0.1, 1.0, 5))
    ref = reference("bi_reduced", b, y, atoms, np.zeros(3), np.ones(3), log_prior=lp, noise_sd=noise_sd)
    c = 0.5 * ((y[:, None, :] - signals("bi_reduced", b, atoms)[None]) ** 2).sum(axis=2)
    like = np.exp(-c / noise_sd ** 2) if noise_sd else c ** (-len(b) / 2)
    post = like * np.exp(lp)
    W = post / post.sum(axis=1, keepdims=True)
    np.testing.assert_allclose(ref["mean"], W @ atoms.T, rtol=1e-12)
    np.testing.assert_allclose(ref["var"], W @ (atoms.T ** 2) - (W @ atoms.T) ** 2, rtol=1e-9, atol=1e-18)
    np.testing.assert_allclose(ref["log_evidence"], np.log(post.sum(axis=1) / np.exp(lp).sum()), rtol=1e-12)
    np.testing.assert_allclose(ref["ess"], 1 / (W ** 2).sum(axis=1), rtol=1e-12)
    assert (ref["map_atom"] == post.argmax(axis=1)).all() and ref["finite"].all()
    assert (ref["eps"] <= 1e-6).all() and (ref["bound_mean"] > 0).all()

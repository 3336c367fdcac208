"""The variable-projection dictionary fit (pnx_curvefit_varpro_f64, api.varpro, HipVarProSolver, p0_varpro), the parts that need no
GPU: the host-side argument checks under AddressSanitizer / UBSan (a stand-alone program, tests/host_stub/varpro_args_stub.cpp),
the ABI's refusals in front of any device work, the slab sizing, the solvers' construction rules, the entry-point line, and the
numpy oracle itself against a brute-force bounded least squares and against the expanded form the kernel evaluates."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT
from varpro_reference import FREE, REDUCED, RATES, accept, case_atoms as _atoms, case_box as _box, case_signals as _noisy, columns, reference

from pyneapple_amd import _lib, api
from pyneapple_amd.models import BiExpModel, MonoExpModel, TriExpModel
from pyneapple_amd.solvers import HipConstrainedCurveFitSolver, HipCurveFitSolver, HipVarProSolver

NAME = "pnx_curvefit_varpro_f64"


# ---- the argument checks as a stand-alone program under the sanitizers
@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("stub") / "varpro_args_stub")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "pyneapple_amd", "csrc"), os.path.join(ROOT, "tests", "host_stub", "varpro_args_stub.cpp"), "-o", exe]
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
    """Every refusal by name, the valid edges accepted (1 and 4096 atoms, every layout, fixed rates and T1), the layout tables
    right, the slab inside the LDS budget for every (n_b, K) with sixteen atoms at 128 b-values and three compartments."""
    assert "varpro args stub ok" in _run_stub(stub)


@pytest.mark.parametrize("n_b,k", [(2, 1), (16, 1), (32, 2), (32, 3), (33, 3), (64, 2), (65, 3), (128, 1), (128, 3)])
def test_python_slab_width_is_the_kernels(stub, n_b, k):
    assert int(_run_stub(stub, n_b, k)) == api.varpro_slab_atoms(n_b, k)


# ---- the ABI without a device
def _call(o, nl=None, lo=None, hi=None, fb=None, fixed=None, n_atoms=None, p_out=True):
    n = o.n_free
    nl = np.array([[0.1, 0.2], [0.01, 0.02], [0.001, 0.002]]) if nl is None else np.ascontiguousarray(nl, float)
    lo = np.zeros(n) if lo is None else np.ascontiguousarray(lo, float)
    hi = np.ones(n) if hi is None else np.ascontiguousarray(hi, float)
    fb = np.full(n, 0.5) if fb is None else np.ascontiguousarray(fb, float)
    fixed = None if fixed is None else np.ascontiguousarray(fixed, float)
    b, y, out = np.zeros(128), np.ones(128), np.zeros(8)
    return _lib.load().pnx_curvefit_varpro_f64(C.byref(o), 1, _lib.ptr(b), _lib.ptr(y), nl.shape[1] if n_atoms is None else n_atoms, _lib.ptr(nl),
                                               _lib.ptr(fixed), _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(fb), _lib.ptr(out) if p_out else None, None,
                                               None, None, 0, 0, None)


def test_symbol_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnx.h")).read(), flags=re.S)
    assert re.search(r"PNX_API\s+int\s+" + NAME + r"\s*\(", text)
    assert NAME in _lib.ABI_SYMBOLS
    fn = getattr(_lib.load(), NAME)
    assert len(fn.argtypes) == 17 and fn.restype is C.c_int


def test_every_refusal_by_message():
    mk = api.make_opts
    tri = lambda **kw: mk("tri_s0", 32, jac="analytic", **kw)
    assert _call(tri(per_voxel=True)) == -2 and "per_voxel_p0_bounds" in _lib.last_error()
    o = mk("tri_s0", 32, fixed_idx=[1], fixed_per_voxel=True, jac="analytic")
    assert _call(o, nl=np.ones((2, 2)) * [[0.01], [0.001]], fixed=[0.1]) == -2 and "fixed_per_voxel" in _lib.last_error()
    o = tri()
    o.queue_order = np.zeros(4, np.int32).ctypes.data
    assert _call(o) == -2 and "queue_order" in _lib.last_error()
    for idx, word in ((0, "fraction"), (5, "S0")):  # a fixed fraction, a fixed S0
        assert _call(mk("tri_s0", 32, fixed_idx=[idx], jac="analytic"), fixed=[0.3]) == -2 and word in _lib.last_error() and "fixed" in _lib.last_error()
    for n_atoms in (0, 4097):
        assert _call(tri(), n_atoms=n_atoms) == -1 and "n_atoms" in _lib.last_error()
    assert _call(tri(), nl=[[0.1, 0.2], [0.01, 0.2], [0.001, 0.002]]) == -1 and "atom 1" in _lib.last_error() and "equal rates" in _lib.last_error()
    # a fixed rate takes part in the comparison
    assert _call(mk("tri_s0", 32, fixed_idx=[4], jac="analytic"), nl=[[0.1, 0.2], [0.01, 0.002]], fixed=[0.002]) == -1 and "equal rates" in _lib.last_error()
    assert _call(tri(), nl=[[0.1, 1.5], [0.01, 0.02], [0.001, 0.002]]) == -1 and "atom 1" in _lib.last_error() and "outside its bounds" in _lib.last_error()
    lo = np.zeros(6)
    lo[5] = -1.0
    assert _call(tri(), lo=lo) == -1 and "lo_S0" in _lib.last_error()
    assert _call(mk("mono", 32, jac="analytic"), nl=[[0.1, 0.2]], lo=[-1.0, 0.0]) == -1 and "lo_S0" in _lib.last_error()
    assert _call(mk("tri_s0", 3, jac="analytic")) == -1 and "n_b=3" in _lib.last_error()
    assert _call(mk("mono", 1, jac="analytic"), nl=[[0.1, 0.2]]) == -1 and "n_b=1" in _lib.last_error()
    fb = np.full(6, 0.5)
    fb[2] = 1.5
    assert _call(tri(), fb=fb) == -1 and "fallback[2]" in _lib.last_error()
    assert _call(tri(), p_out=False) == -1 and "NULL" in _lib.last_error()
    if _lib.device_count() == 0:  # valid calls stop at the device
        assert _call(tri()) == -3
        assert _call(mk("tri_reduced", 32, fixed_idx=[4, 5], t1_mode=1, tr=3000.0, jac="analytic"), nl=[[0.1, 0.2], [0.01, 0.02]], fixed=[0.001, 0.9]) == -3


def test_no_cpu_fallback_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is visible here")
    with pytest.raises(_lib.PnxError):
        api.varpro("bi_reduced", np.linspace(0, 1000, 8), np.ones((2, 8)), [[0.1], [0.001]], np.zeros(3), np.ones(3), np.full(3, 0.5))
    with pytest.raises(_lib.PnxError):
        _solver().fit(np.linspace(0, 1000, 8), np.ones((2, 8)))


def test_api_shape_rules(monkeypatch):
    monkeypatch.setattr(_lib, "require_device", lambda: None)
    b, y = np.linspace(0, 1000, 8), np.ones((2, 8))
    with pytest.raises(ValueError, match="2 free non-linear"):
        api.varpro("bi_reduced", b, y, [[0.1]], np.zeros(3), np.ones(3), np.full(3, 0.5))
    with pytest.raises(ValueError, match="per-voxel fixed"):
        api.varpro("bi_reduced", b, y, [[0.1]], np.zeros(2), np.ones(2), np.full(2, 0.5), fixed_idx=[2], fixed_vals=np.ones((1, 2)))
    with pytest.raises(ValueError, match="fallback"):
        api.varpro("bi_reduced", b, y, [[0.1], [0.001]], np.zeros(3), np.ones(3), np.full(2, 0.5))


# ---- the solvers' construction rules
BOUNDS = {"f1": (0.0, 1.0), "D1": (1e-4, 0.5), "f2": (0.0, 1.0), "D2": (1e-4, 0.5), "D3": (1e-5, 0.5), "S0": (0.0, 10.0)}
P0 = {"f1": 0.2, "D1": 0.1, "f2": 0.3, "D2": 0.01, "D3": 0.001, "S0": 1.0}


def _solver(model=None, rates=None, **kw):
    kw = {"p0": P0, "bounds": BOUNDS, **kw}
    return HipVarProSolver(model or TriExpModel(fit_s0=True), {n: RATES for n in ("D1", "D2", "D3")} if rates is None else rates, **kw)


def test_solver_builds_the_ordered_atoms():
    s = _solver()
    assert s._nl_atoms.shape == (3, 56) and s._nl_names == ["D1", "D2", "D3"] and s.ordered is True
    assert (s._nl_atoms[0] > s._nl_atoms[1]).all() and (s._nl_atoms[1] > s._nl_atoms[2]).all()
    assert s._nl_atoms.dtype == np.float64 and s._nl_atoms.flags.c_contiguous
    assert _solver(ordered=False, rates={"D1": [0.1, 0.2], "D3": [1e-3]})._nl_atoms.tolist() == [[0.1, 0.2], [0.01, 0.01], [1e-3, 1e-3]]
    r19 = list(np.geomspace(1e-3, 0.3, 19))
    assert _solver(rates={"D1": r19, "D2": r19, "D3": r19})._nl_atoms.shape == (3, 969)
    # a fixed rate takes part in the ordering; T1 is one more axis
    s = _solver(model=TriExpModel(fit_s0=True, fixed_params={"D3": 1e-3}), rates={"D1": RATES, "D2": RATES})
    assert s._nl_names == ["D1", "D2"] and (s._nl_atoms[1] > 1e-3).all() and (s._nl_atoms[0] > s._nl_atoms[1]).all()
    s = HipVarProSolver(MonoExpModel(fit_t1=True, repetition_time=3000.0), {"D": [1e-3, 2e-3], "T1": [800.0, 1200.0, 1600.0]},
                        p0={"S0": 1.0, "D": 1e-3, "T1": 1000.0}, bounds={"S0": (0.0, 10.0), "D": (1e-4, 0.1), "T1": (100.0, 5000.0)})
    assert s._nl_atoms.shape == (2, 6) and s._nl_names == ["D", "T1"]
    # the TOML loader's call: max_iter, tol by keyword, the reference's other keys ignored
    t = HipVarProSolver(TriExpModel(fit_s0=True), {"D1": [0.1, 0.2]}, max_iter=100, tol=1e-6, p0=P0, bounds=BOUNDS, method="trf", multi_threading=True)
    assert t._nl_atoms.shape == (3, 2) and t.solver_kwargs == {"method": "trf", "multi_threading": True}


def test_solver_refusals():
    with pytest.raises(ValueError, match="rates is required"):
        HipVarProSolver(TriExpModel(fit_s0=True), p0=P0, bounds=BOUNDS)
    with pytest.raises(ValueError, match="bounds is required"):
        HipVarProSolver(TriExpModel(fit_s0=True), {"D1": [0.1]}, p0=P0)
    for rates, text in (([0.1], "dict"), ({"f1": [0.1]}, "closed form"), ({"D1": [0.9]}, "outside the bounds"), ({"D1": [float("nan")]}, "outside the bounds"),
                        ({"D1": [0.01], "D2": [0.01, 0.02]}, "leaves no atom"), ({n: np.geomspace(1e-3, 0.3, 40) for n in ("D1", "D2", "D3")}, "atoms, more than")):
        with pytest.raises(ValueError, match=text):
            _solver(rates=rates)
    with pytest.raises(ValueError, match="D3"):  # not in rates, not in p0
        _solver(rates={"D1": [0.1]}, p0={k: v for k, v in P0.items() if k != "D3"}, fallback=P0)
    with pytest.raises(ValueError, match="fallback"):
        _solver(p0=None)
    with pytest.raises(ValueError, match=r"fallback\['f1'\]"):
        _solver(fallback={**P0, "f1": 1.5})
    with pytest.raises(ValueError, match="lower bound of S0"):
        _solver(bounds={**BOUNDS, "S0": (-1.0, 10.0)})
    with pytest.raises(ValueError, match="fixed fraction"):
        _solver(model=TriExpModel(fit_s0=True, fixed_params={"f2": 0.3}))
    for kw in (dict(io_dtype="float32"), dict(precision="float32")):
        with pytest.raises(ValueError, match="float64"):
            _solver(**kw)
    with pytest.raises(ValueError, match="sigma"):
        _solver(sigma=np.ones((4, 4)))
    with pytest.raises(ValueError, match="per-pixel fixed"):
        _solver().fit(np.linspace(0, 1000, 32), np.ones((2, 32)), pixel_fixed_params={"D3": np.full(2, 1e-3)})
    assert _solver(fallback={**P0, "f1": 0.7}).fallback["f1"] == 0.7


def test_p0_varpro_construction_rules():
    mk = lambda **kw: HipCurveFitSolver(TriExpModel(fit_s0=True), 250, 1e-8, p0=P0, bounds=BOUNDS, **kw)
    rates = {n: RATES for n in ("D1", "D2", "D3")}
    s = mk(p0_varpro={"rates": rates})
    assert s._varpro_nl_atoms.tobytes() == _solver()._nl_atoms.tobytes() and s.p0_varpro["ordered"] is True
    assert mk().p0_varpro is None and mk()._varpro_nl_atoms is None  # opt-in
    assert mk(p0_varpro={"rates": {"D1": [0.1, 0.2]}, "ordered": False})._varpro_nl_atoms.shape == (3, 2)
    with pytest.raises(ValueError, match="give one of them"):
        mk(p0_varpro={"rates": rates}, p0_grid={"f1": [0.1, 0.2]})
    with pytest.raises(ValueError, match="give one of them"):
        mk(p0_varpro={"rates": rates}, p0_peel={"b_thresholds": [50.0, 300.0]})
    for bad in ([0.1], {"ordered": True}, {"rates": rates, "other": 1}):
        with pytest.raises(ValueError, match="'rates'"):
            mk(p0_varpro=bad)
    with pytest.raises(ValueError, match="float64"):
        mk(p0_varpro={"rates": rates}, io_dtype="float32")
    with pytest.raises(ValueError, match="HipConstrainedCurveFitSolver"):
        HipConstrainedCurveFitSolver(TriExpModel(fit_s0=True), P0, BOUNDS, p0_varpro={"rates": rates})
    b, y = np.linspace(0, 1000, 32), np.ones((2, 32))
    with pytest.raises(ValueError, match="per-voxel p0"):
        s.fit(b, y, p0=np.ones((6, 2)))
    with pytest.raises(ValueError, match="per-pixel fixed"):
        s.fit(b, y, pixel_fixed_params={"D3": np.full(2, 1e-3)})


def test_entry_point_is_registered():
    text = open(os.path.join(ROOT, "pyproject.toml")).read()
    group = text.split('[project.entry-points."pyneapple.solvers"]', 1)[1].split("\n[", 1)[0]
    assert re.search(r'^hip_varpro = "pyneapple_amd\.solvers:HipVarProSolver"$', group, flags=re.M)
    mod, cls = "pyneapple_amd.solvers:HipVarProSolver".split(":")
    assert getattr(__import__(mod, fromlist=[cls]), cls) is HipVarProSolver


# ---- the oracle itself
@pytest.mark.parametrize("model", ["mono", "bi_full", "tri_s0", "tri_reduced"])
def test_reference_against_brute_force_bounded_least_squares(model):
    """A handful of voxels: where no clip is active the reference's amplitudes are the bounded least-squares optimum; where one is,
    its point is feasible, costs no less than the optimum, and for K = 1 it IS the optimum."""
    from scipy.optimize import lsq_linear

    b, y = _noisy(model, 6)
    atoms = _atoms(model)[:, ::3]
    for narrow in (False, True):
        lo, hi = _box(model, narrow)
        ref = reference(model, b, y, atoms, lo, hi, noisy=True)
        Phi, _ = columns(model, b, atoms)
        if ref["cls"] != FREE:
            continue  # the free classes are a plain box problem in the amplitudes
        for v in range(len(y)):
            for g in range(atoms.shape[1]):
                opt = lsq_linear(Phi[g], y[v], bounds=(lo[ref["lin_rows"]], hi[ref["lin_rows"]]), tol=1e-14, method="bvls")
                assert ref["c"][v, g] >= opt.cost - 1e-12
                if ref["K"] == 1 or not ref["clipped"][v, g]:
                    assert abs(ref["c"][v, g] - opt.cost) <= 1e-10 and np.allclose(ref["lin"][v, g], opt.x, atol=1e-8)
    assert narrow and ref["clipped"].any()


def _expanded(model, b, y, atoms, lo, hi):
    """The kernel's arithmetic in numpy: c = Phi^T y, the stored inverse, the clip, the expanded cost, the argmin."""
    ref = reference(model, b, y, atoms, lo, hi)
    Phi, _ = columns(model, b, atoms)
    K, cls, rows = ref["K"], ref["cls"], ref["lin_rows"]
    llo, lhi = lo[rows], hi[rows]
    n_vox, G = len(y), atoms.shape[1]
    cost, lin, clp = np.empty((n_vox, G)), np.empty((n_vox, G, len(rows))), np.empty((n_vox, G), bool)
    from varpro_reference import _clip_map

    for g in range(G):
        P = Phi[g]
        M, c = P.T @ P, P.T @ y.T
        if cls == REDUCED:
            D = P[:, :K - 1] - P[:, K - 1:]
            ah = np.linalg.inv(D.T @ D) @ ((c[:K - 1] - c[K - 1:]) - (D.T @ P[:, K - 1])[:, None])
        else:
            ah = np.linalg.inv(M) @ c
        ap, rep, clp[:, g], _ = _clip_map(cls, K, ah, llo, lhi)
        cost[:, g] = 0.5 * (y * y).sum(axis=1) - (c * ap).sum(axis=0) + 0.5 * (ap * (M @ ap)).sum(axis=0)
        lin[:, g] = rep.T
    best = cost.argmin(axis=1).astype(np.int32)
    v = np.arange(n_vox)
    params = np.empty((len(lo), n_vox))
    params[ref["nl_rows"]] = atoms[:, best]
    params[rows] = lin[v, best].T
    return ref, dict(params=params, atom=best, cost=cost[v, best], clipped=clp[v, best].astype(np.int8))


@pytest.mark.parametrize("model", sorted(api.MODEL_IDS))
@pytest.mark.parametrize("narrow", [False, True])
def test_the_expanded_form_meets_the_bound(model, narrow):
    """The acceptance the GPU tests apply, applied to a numpy restatement of the kernel's arithmetic: the bound holds, and the
    condition that keeps it honest (tol <= 1e-3 of the smallest cost) holds on the noisy inputs the GPU tests use."""
    b, y = _noisy(model, 40)
    atoms = _atoms(model)
    lo, hi = _box(model, narrow)
    ref, got = _expanded(model, b, y, atoms, lo, hi)
    reference(model, b, y, atoms, lo, hi, noisy=True)
    assert ref["kappa"].max() <= 1.3e4 * 1.01  # the 56 / 28 / 8 atoms of the shared list; the per-compartment lists: 520
    accept(ref, got, atoms)

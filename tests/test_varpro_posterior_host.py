"""The posterior over the variable-projection dictionary (pnx_curvefit_varpro_posterior_f64, api.varpro_posterior,
HipBayesVarProSolver), the parts that need no GPU: the host-side argument checks under AddressSanitizer / UBSan (a stand-alone
program, tests/host_stub/varpro_posterior_args_stub.cpp), the ABI's refusals in front of any device work, the slab sizing, the
solver's construction rules, the entry-point line, and the numpy oracle itself -- against a brute-force dense posterior and against
the expanded form the kernel evaluates, on the inputs the GPU tests use (so the oracle's preconditions are checked here)."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT
from varpro_posterior_reference import accept, apart_atoms, reference, wide_box
from varpro_reference import REDUCED, _clip_map, case_atoms, case_box, case_signals, columns

from pyneapple_amd import _lib, api
from pyneapple_amd.models import MonoExpModel, TriExpModel
from pyneapple_amd.solvers import HipBayesVarProSolver

NAME = "pnx_curvefit_varpro_posterior_f64"
NOISE_SD = 0.02  # the additive noise of varpro_reference.case_signals


# ---- the argument checks as a stand-alone program under the sanitizers
@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("stub") / "varpro_posterior_args_stub")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "pyneapple_amd", "csrc"), os.path.join(ROOT, "tests", "host_stub", "varpro_posterior_args_stub.cpp"), "-o", exe]
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
    """Every refusal by name (the variable projection's and the three new arguments'), the valid edges accepted, the normaliser, the
    centres and the amplitude bound A right, the slab inside the LDS budget for every (n_b, K)."""
    assert "varpro posterior args stub ok" in _run_stub(stub)


@pytest.mark.parametrize("n_b,k", [(2, 1), (16, 1), (32, 2), (32, 3), (33, 3), (64, 2), (65, 3), (128, 1), (128, 3)])
def test_python_slab_width_is_the_kernels(stub, n_b, k):
    assert int(_run_stub(stub, n_b, k)) == api.varpro_posterior_slab_atoms(n_b, k)


# ---- the ABI without a device
def _call(o, nl=None, lo=None, hi=None, fixed=None, n_atoms=None, lp=None, noise_sd=0.0, marg=1, mean=True):
    n = o.n_free
    nl = np.array([[0.1, 0.2], [0.01, 0.02], [0.001, 0.002]]) if nl is None else np.ascontiguousarray(nl, float)
    lo = np.zeros(n) if lo is None else np.ascontiguousarray(lo, float)
    hi = np.ones(n) if hi is None else np.ascontiguousarray(hi, float)
    fixed = None if fixed is None else np.ascontiguousarray(fixed, float)
    lp = None if lp is None else np.ascontiguousarray(lp, float)
    b, y, out = np.zeros(128), np.ones(128), np.zeros(8)
    return getattr(_lib.load(), NAME)(C.byref(o), 1, _lib.ptr(b), _lib.ptr(y), nl.shape[1] if n_atoms is None else n_atoms, _lib.ptr(nl),
                                      _lib.ptr(fixed), _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(lp), noise_sd, marg, _lib.ptr(out) if mean else None,
                                      None, None, None, None, None, None, 0, 0, None)


def test_symbol_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnx.h")).read(), flags=re.S)
    assert re.search(r"PNX_API\s+int\s+" + NAME + r"\s*\(", text)
    assert NAME in _lib.ABI_SYMBOLS
    fn = getattr(_lib.load(), NAME)
    dp, vp = C.c_void_p, C.c_void_p
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.POINTER(_lib.CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, dp, C.c_double, C.c_int, dp, dp, vp, dp,
                                 dp, dp, dp, C.c_int, C.c_int, vp]
    args = re.search(NAME + r"\s*\((.*?)\);", text, flags=re.S).group(1)
    assert len(args.split(",")) == len(fn.argtypes) == 22


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
    assert _call(tri(), nl=[[0.1, 1.5], [0.01, 0.02], [0.001, 0.002]]) == -1 and "atom 1" in _lib.last_error() and "outside its bounds" in _lib.last_error()
    lo = np.zeros(6)
    lo[5] = -1.0
    assert _call(tri(), lo=lo) == -1 and "lo_S0" in _lib.last_error()
    assert _call(mk("tri_s0", 3, jac="analytic")) == -1 and "n_b=3" in _lib.last_error()
    assert _call(tri(), mean=False) == -1 and "mean" in _lib.last_error()
    for bad in (-0.5, float("nan"), float("inf")):
        assert _call(tri(), noise_sd=bad) == -1 and "noise_sd" in _lib.last_error()
    for bad in (-1, 2):
        assert _call(tri(), marg=bad) == -1 and "marginal_amplitudes" in _lib.last_error()
    assert _call(tri(), lp=[0.0, float("nan")]) == -1 and "log_prior[1]" in _lib.last_error()
    assert _call(tri(), lp=[float("inf"), 0.0]) == -1 and "log_prior[0]" in _lib.last_error()
    assert _call(tri(), lp=[-np.inf, -np.inf]) == -1 and "excludes every atom" in _lib.last_error()
    if _lib.device_count() == 0:  # valid calls stop at the device
        assert _call(tri()) == -3
        assert _call(tri(), lp=[-np.inf, -1.0], noise_sd=0.02, marg=0) == -3


def test_no_cpu_fallback_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is visible here")
    with pytest.raises(_lib.PnxError):
        api.varpro_posterior("bi_reduced", np.linspace(0, 1000, 8), np.ones((2, 8)), [[0.1], [0.001]], np.zeros(3), np.ones(3))
    with pytest.raises(_lib.PnxError):
        _solver().fit(np.linspace(0, 1000, 8), np.ones((2, 8)))


def test_api_shape_rules(monkeypatch):
    monkeypatch.setattr(_lib, "require_device", lambda: None)
    b, y = np.linspace(0, 1000, 8), np.ones((2, 8))
    with pytest.raises(ValueError, match="2 free non-linear"):
        api.varpro_posterior("bi_reduced", b, y, [[0.1]], np.zeros(3), np.ones(3))
    with pytest.raises(ValueError, match="per-voxel fixed"):
        api.varpro_posterior("bi_reduced", b, y, [[0.1]], np.zeros(2), np.ones(2), fixed_idx=[2], fixed_vals=np.ones((1, 2)))
    with pytest.raises(ValueError, match="log_prior has shape"):
        api.varpro_posterior("bi_reduced", b, y, [[0.1], [0.001]], np.zeros(3), np.ones(3), log_prior=np.zeros(2))


# ---- the solver's construction rules
BOUNDS = {"f1": (0.0, 1.0), "D1": (1e-4, 0.5), "f2": (0.0, 1.0), "D2": (1e-4, 0.5), "D3": (1e-5, 0.5), "S0": (0.0, 10.0)}
P0 = {"f1": 0.2, "D1": 0.1, "f2": 0.3, "D2": 0.01, "D3": 0.001, "S0": 1.0}
RATES = list(np.geomspace(3e-4, 0.3, 8))


def _solver(model=None, rates=None, **kw):
    kw = {"p0": P0, "bounds": BOUNDS, **kw}
    return HipBayesVarProSolver(model or TriExpModel(fit_s0=True), {n: RATES for n in ("D1", "D2", "D3")} if rates is None else rates, **kw)


def test_solver_builds_the_atoms_of_the_variable_projection():
    from pyneapple_amd.solvers import HipVarProSolver

    s = _solver()
    assert s._nl_atoms.shape == (3, 56) and s._nl_names == ["D1", "D2", "D3"] and s.ordered is True
    assert s._nl_atoms.tobytes() == HipVarProSolver(TriExpModel(fit_s0=True), {n: RATES for n in ("D1", "D2", "D3")}, p0=P0, bounds=BOUNDS)._nl_atoms.tobytes()
    assert s.noise_sd == 0.0 and s.log_prior is None and s.marginal_amplitudes is True
    t = _solver(noise_sd=0.02, log_prior=np.zeros(2), marginal_amplitudes=False, sigma=2.0, ordered=False, rates={"D1": [0.1, 0.2]})
    assert t.noise_sd == 0.02 and t.marginal_amplitudes is False and t.sigma.shape == (1,) and t._nl_atoms.shape == (3, 2)
    s = HipBayesVarProSolver(MonoExpModel(fit_t1=True, repetition_time=3000.0), {"D": [1e-3, 2e-3], "T1": [800.0, 1200.0, 1600.0]},
                             p0={"S0": 1.0, "D": 1e-3, "T1": 1000.0}, bounds={"S0": (0.0, 10.0), "D": (1e-4, 0.1), "T1": (100.0, 5000.0)})
    assert s._nl_atoms.shape == (2, 6) and s._nl_names == ["D", "T1"]
    # the TOML loader's call: max_iter, tol by keyword, the reference's other keys ignored
    t = HipBayesVarProSolver(TriExpModel(fit_s0=True), {"D1": [0.1, 0.2]}, max_iter=100, tol=1e-6, p0=P0, bounds=BOUNDS, method="trf", multi_threading=True)
    assert t._nl_atoms.shape == (3, 2) and t.solver_kwargs == {"method": "trf", "multi_threading": True}


def test_solver_refusals():
    with pytest.raises(ValueError, match="rates is required"):
        HipBayesVarProSolver(TriExpModel(fit_s0=True), p0=P0, bounds=BOUNDS)
    with pytest.raises(ValueError, match="bounds is required"):
        HipBayesVarProSolver(TriExpModel(fit_s0=True), {"D1": [0.1]}, p0=P0)
    for rates, text in (([0.1], "dict"), ({"f1": [0.1]}, "closed form"), ({"D1": [0.9]}, "outside the bounds"),
                        ({"D1": [0.01], "D2": [0.01, 0.02]}, "leaves no atom"), ({n: np.geomspace(1e-3, 0.3, 40) for n in ("D1", "D2", "D3")}, "atoms, more than")):
        with pytest.raises(ValueError, match=text):
            _solver(rates=rates)
    with pytest.raises(ValueError, match="lower bound of S0"):
        _solver(bounds={**BOUNDS, "S0": (-1.0, 10.0)})
    with pytest.raises(ValueError, match="fixed fraction"):
        _solver(model=TriExpModel(fit_s0=True, fixed_params={"f2": 0.3}))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="noise_sd"):
            _solver(noise_sd=bad)
    with pytest.raises(ValueError, match="56 atoms"):
        _solver(log_prior=np.zeros(55))
    for lp in (np.full(56, -np.inf), np.r_[np.nan, np.zeros(55)], np.r_[np.inf, np.zeros(55)]):
        with pytest.raises(ValueError, match="finite or -inf"):
            _solver(log_prior=lp)
    for kw in (dict(io_dtype="float32"), dict(precision="float32")):
        with pytest.raises(ValueError, match="float64"):
            _solver(**kw)
    with pytest.raises(ValueError, match="sigma"):
        _solver(sigma=np.ones((4, 4)))
    with pytest.raises(ValueError, match="per-pixel fixed"):
        _solver().fit(np.linspace(0, 1000, 32), np.ones((2, 32)), pixel_fixed_params={"D3": np.full(2, 1e-3)})


def test_entry_point_is_registered():
    text = open(os.path.join(ROOT, "pyproject.toml")).read()
    group = text.split('[project.entry-points."pyneapple.solvers"]', 1)[1].split("\n[", 1)[0]
    assert re.search(r'^hip_bayes_varpro = "pyneapple_amd\.solvers:HipBayesVarProSolver"$', group, flags=re.M)
    mod, cls = "pyneapple_amd.solvers:HipBayesVarProSolver".split(":")
    assert getattr(__import__(mod, fromlist=[cls]), cls) is HipBayesVarProSolver


# ---- the oracle itself
@pytest.mark.parametrize("model", ["mono", "bi_s0", "bi_reduced"])
@pytest.mark.parametrize("noise_sd", [0.0, NOISE_SD])
@pytest.mark.parametrize("marginal", [False, True])
def test_reference_against_a_brute_force_dense_posterior(model, noise_sd, marginal):
    """Three voxels, the wide box (no clip is active, asserted): amplitudes by the normal equations, the evidence by
    scipy.special.logsumexp, the weights and the centred moments in extended precision."""
    from scipy.special import logsumexp

    b, y = case_signals(model, 3)
    atoms = case_atoms(model)
    lo, hi = case_box(model)
    for i, n in enumerate(api.MODEL_PARAM_NAMES[model]):  # a box no amplitude reaches, at the wrong-basin atoms either
        if n.startswith("f"):
            lo[i], hi[i] = -100.0, 100.0
        if n == "S0":
            hi[i] = 100.0
    rng = np.random.default_rng(5)
    lp = np.log(rng.uniform(0.1, 1.0, atoms.shape[1]))
    lp[1] = -np.inf
    ref = reference(model, b, y, atoms, lo, hi, log_prior=lp, noise_sd=noise_sd, marginal=marginal)
    Phi, _ = columns(model, b, atoms)
    K, cls = ref["K"], ref["cls"]
    G, n_b = atoms.shape[1], len(b)
    n_lin = len(ref["lin_rows"])
    ell = np.empty((3, G))
    theta = np.empty((3, len(lo), G), np.longdouble)
    for g in range(G):
        P = Phi[g]
        if cls == REDUCED:
            A, rhs = P[:, :K - 1] - P[:, K - 1:], y.T - P[:, K - 1:]
        else:
            A, rhs = P, y.T
        N = A.T @ A
        ah = np.linalg.solve(N, A.T @ rhs)  # (n_lin, 3)
        r = rhs - A @ ah
        cost = 0.5 * (r * r).sum(axis=0)
        rep = ah.copy()
        if cls not in (0, REDUCED) and K > 1:  # S0 class: (f_1 .. f_{K-1}, S0)
            rep = np.vstack([ah[:K - 1] / ah.sum(axis=0), ah.sum(axis=0)[None]])
        assert ((rep >= lo[ref["lin_rows"], None]) & (rep <= hi[ref["lin_rows"], None])).all(), "a clip would be active"
        occam = -0.5 * np.log(np.linalg.det(N)) if marginal else 0.0
        ell[:, g] = lp[g] + occam - (cost / noise_sd ** 2 if noise_sd > 0 else 0.5 * (n_b - n_lin) * np.log(cost))
        theta[:, ref["lin_rows"], g] = rep.T
        theta[:, ref["nl_rows"], g] = atoms[:, g]
    L = logsumexp(ell, axis=1)
    W = np.exp(ell - L[:, None]).astype(np.longdouble)
    mean = (W[:, None, :] * theta).sum(axis=2)
    var = (W[:, None, :] * (theta - mean[:, :, None]) ** 2).sum(axis=2)
    assert not ref["clipped_mass"].any() and ref["W"][:, 1].max() == 0.0
    np.testing.assert_allclose(ref["log_evidence"], L - logsumexp(lp), rtol=0, atol=1e-9)
    np.testing.assert_allclose(ref["mean"], mean.astype(float), rtol=1e-9)
    np.testing.assert_allclose(ref["var"], var.astype(float), rtol=1e-5, atol=1e-22)
    np.testing.assert_allclose(ref["ess"], (1 / (W * W).sum(axis=1)).astype(float), rtol=1e-9)
    assert (ref["map_atom"] == ell.argmax(axis=1)).all()


def expanded(model, b, y, atoms, lo, hi, log_prior=None, noise_sd=0.0, marginal=True, **kw):
    """The kernel's arithmetic in numpy: c = Phi^T y, the stored inverse, the clip, the expanded cost, log det N by cofactors of the
    Gram matrix, the floor; then the weights and moments by the textbook formulas."""
    from varpro_posterior_reference import amp_l1

    ref = reference(model, b, y, atoms, lo, hi, log_prior=log_prior, noise_sd=noise_sd, marginal=marginal, **kw)
    Phi, w = columns(model, b, atoms, kw.get("fixed_idx", ()), kw.get("fixed_vals"), kw.get("sigma"), kw.get("t1_mode", 0), kw.get("tr", 0.0), kw.get("tm", 0.0))
    K, cls, rows = ref["K"], ref["cls"], ref["lin_rows"]
    llo, lhi = lo[rows], hi[rows]
    yw = y * w
    n_vox, G, n_b = len(y), atoms.shape[1], len(b)
    lp = np.zeros(G) if log_prior is None else np.asarray(log_prior, float)
    ell, clp = np.full((n_vox, G), -np.inf), np.zeros((n_vox, G), bool)
    theta = np.zeros((n_vox, len(lo), G))
    yy = (yw * yw).sum(axis=1)
    floor = 4 * n_b * 2.0 ** -52 * (yy + amp_l1(cls, K, llo, lhi) ** 2 * (Phi * Phi).sum(axis=1).max())
    for g in range(G):
        if lp[g] == -np.inf:
            continue
        P = Phi[g]
        M, c = P.T @ P, P.T @ yw.T
        if cls == REDUCED:
            D = P[:, :K - 1] - P[:, K - 1:]
            N = D.T @ D
            ah = np.linalg.inv(N) @ ((c[:K - 1] - c[K - 1:]) - (D.T @ P[:, K - 1])[:, None])
        else:
            N = M
            ah = np.linalg.inv(M) @ c
        ap, rep, clp[:, g], _ = _clip_map(cls, K, ah, llo, lhi)
        cost = 0.5 * yy - (c * ap).sum(axis=0) + 0.5 * (ap * (M @ ap)).sum(axis=0)
        lw = lp[g] - (0.5 * np.log(np.linalg.det(N)) if marginal else 0.0)
        ell[:, g] = lw - (cost / noise_sd ** 2 if noise_sd > 0 else 0.5 * (n_b - len(rows)) * np.log(np.maximum(cost, floor)))
        theta[:, rows, g] = rep.T
        theta[:, ref["nl_rows"], g] = atoms[:, g]
    m = ell.max(axis=1)
    wg = np.exp(ell - m[:, None])
    s = wg.sum(axis=1)
    W = wg / s[:, None]
    adm = lp > -np.inf
    centre = np.zeros(len(lo))  # the kernel accumulates a non-linear row about the mid-range of its admissible atoms
    centre[ref["nl_rows"]] = atoms[:, adm].min(axis=1) + 0.5 * (atoms[:, adm].max(axis=1) - atoms[:, adm].min(axis=1))
    mean = centre + (W[:, None, :] * (theta - centre[None, :, None])).sum(axis=2)
    var = (W[:, None, :] * (theta - mean[:, :, None]) ** 2).sum(axis=2)
    best = ell.argmax(axis=1).astype(np.int32)
    lpa = lp[lp > -np.inf]
    got = dict(mean=np.ascontiguousarray(mean.T), sd=np.ascontiguousarray(np.sqrt(var).T), map_atom=best,
               map_p=np.ascontiguousarray(theta[np.arange(n_vox), :, best].T), log_evidence=m + np.log(s) - (np.log(np.exp(lpa - lpa.max()).sum()) + lpa.max()),
               ess=1 / (W * W).sum(axis=1), clipped_mass=np.minimum((W * clp).sum(axis=1), 1.0))
    return ref, got


# the eps cap of a case: the reference's default of 1e-6 in the wide box (wide_box: no clip is active at any pair).  The narrow box
# makes a clip active at nearly every pair, and the first-order clip term of the variable projection's tol (4 |grad| L d_a) then
# dominates: an explicit looser cap, 1e-3, there only.  tests/test_gpu_varpro_posterior.py applies the same rule.
def max_eps(narrow):
    return 1e-3 if narrow else 1e-6


@pytest.mark.parametrize("model", sorted(api.MODEL_IDS))
@pytest.mark.parametrize("narrow", [False, True])
def test_the_expanded_form_meets_the_bound(model, narrow):
    """The acceptance the GPU tests apply, applied to a numpy restatement of the kernel's arithmetic on the GPU tests' own inputs:
    the bounds hold, and so do the reference's preconditions (eps_v under its cap, no voxel on the cancellation floor)."""
    b, y = case_signals(model, 40)
    atoms = case_atoms(model)
    lo, hi = case_box(model, True) if narrow else wide_box(model)
    for noise_sd in (0.0, NOISE_SD):
        for marginal in (False, True):
            ref, got = expanded(model, b, y, atoms, lo, hi, noise_sd=noise_sd, marginal=marginal, max_eps=max_eps(narrow))
            print(model, narrow, noise_sd, marginal, f"eps <= {ref['eps'].max():.3g}, median ess {np.median(ref['ess']):.3g}")
            accept(ref, got, atoms)
            assert ref["clipped_mass"].mean() > 0.5 if narrow else not ref["clipped_mass"].any()


def _gpu_cases():
    """(id, model, b, y, atoms, lo, hi, narrow, keywords) of the inputs tests/test_gpu_varpro_posterior.py compares against the reference: the
    largest of each axis and every case with inputs of its own."""
    from grid_start_reference import signals

    for model in sorted(api.MODEL_IDS):
        b, y = case_signals(model, 130)
        yield f"layout-{model}-wide", model, b, y, case_atoms(model), *wide_box(model), False, {}
        yield f"layout-{model}-narrow", model, b, y, case_atoms(model), *case_box(model, True), True, {}
    b, y = case_signals("tri_s0", 1000)
    yield "voxels-1000", "tri_s0", b, y, case_atoms("tri_s0"), *wide_box("tri_s0"), False, {}
    b, y = case_signals("mono", 70001, n_b=5)
    yield "voxels-70001", "mono", b, y, case_atoms("mono"), *wide_box("mono"), False, {}
    b, y = case_signals("tri_reduced", 50)
    for n in (1, 15, 47, 64):
        yield f"atoms-{n}", "tri_reduced", b, y, case_atoms("tri_reduced")[:, :n], *wide_box("tri_reduced"), False, {}
    b, y = case_signals("mono", 40, n_b=4)
    yield "atoms-4096", "mono", b, y, np.geomspace(3e-4, 0.3, 4096)[None], *wide_box("mono"), False, {}
    for model, n_b in (("mono", 2), ("mono", 4), ("mono", 5), ("tri_s0", 31), ("tri_s0", 33), ("tri_s0", 64), ("tri_s0", 65), ("tri_s0", 128), ("bi_full", 128)):
        b, y = case_signals(model, 150, n_b=n_b)
        yield f"b-{model}-{n_b}", model, b, y, case_atoms(model), *wide_box(model), False, {}
    b, y = case_signals("bi_s0", 100)
    yield "sigma", "bi_s0", b, y, apart_atoms("bi_s0"), *wide_box("bi_s0"), False, dict(sigma=np.linspace(0.5, 2.0, 32))
    b, y = case_signals("tri_s0", 100)
    lo, hi = wide_box("tri_s0")
    free = [0, 1, 2, 3, 5]
    yield "fixed-rate", "tri_s0", b, y, case_atoms("tri_s0")[:2, ::4], lo[free], hi[free], False, dict(fixed_idx=[4], fixed_vals=np.array([6e-4]))
    d = np.geomspace(3e-4, 0.03, 8)
    for t1_mode, fixed in ((1, True), (2, True), (1, False)):
        rng = np.random.default_rng(11)
        b = np.linspace(0.0, 1000.0, 32)
        kw = dict(t1_mode=t1_mode, tr=3000.0, tm=20.0 if t1_mode == 2 else 0.0)
        truth = np.stack([rng.uniform(0.8, 1.2, 90), rng.uniform(1e-3, 3e-3, 90), np.full(90, 1000.0) if fixed else rng.uniform(700.0, 1500.0, 90)])
        y = signals("mono", b, truth, **kw) + 0.02 * rng.standard_normal((90, 32))
        if fixed:
            yield f"t1-{t1_mode}-fixed", "mono", b, y, d[None], np.array([0.0, 1e-5]), np.array([10.0, 0.5]), False, dict(fixed_idx=[2], fixed_vals=np.array([1000.0]), **kw)
        else:
            atoms = np.ascontiguousarray(np.array([(a, t) for a in d for t in (600.0, 1000.0, 1600.0)]).T)
            yield "t1-axis", "mono", b, y, atoms, np.array([0.0, 1e-5, 100.0]), np.array([10.0, 0.5, 5000.0]), False, kw
    for model in ("tri_s0", "tri_reduced"):
        b, y = case_signals(model, 65)
        yield f"one-atom-{model}", model, b, y, np.ascontiguousarray(case_atoms(model)[:, 21][:, None]), *wide_box(model), False, {}
    for model in ("bi_reduced", "tri_s0"):
        b, y = case_signals(model, 70)
        yield f"n70-{model}", model, b, y, case_atoms(model), *wide_box(model), False, {}
    b, y = case_signals("tri_s0", 200)
    yield "plugin", "tri_s0", b, y, case_atoms("tri_s0"), *wide_box("tri_s0"), False, {}


_GPU_CASES = {c[0]: c[1:] for c in _gpu_cases()}


@pytest.mark.parametrize("case", sorted(_GPU_CASES))
def test_reference_preconditions_of_the_gpu_cases(case):
    """The reference alone, on the CPU: eps_v <= 1e-6 on every voxel of every wide-box case and no clip at any pair there; the
    explicit 1e-3 only in the narrow box; no voxel on the cancellation floor (asserted inside `reference`)."""
    model, b, y, atoms, lo, hi, narrow, kw = _GPU_CASES[case]
    for noise_sd in (0.0, NOISE_SD):
        for marginal in (False, True):
            ref = reference(model, b, y, atoms, lo, hi, noise_sd=noise_sd, marginal=marginal, max_eps=max_eps(narrow), **kw)
            print(case, noise_sd, marginal, f"eps <= {ref['eps'].max():.3g}")
            assert narrow or not ref["clipped_mass"].any()

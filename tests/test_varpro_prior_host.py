"""The empirical-Bayes prior over the variable-projection dictionary (pnx_curvefit_varpro_prior_em_f64, api.varpro_prior_em,
HipBayesVarProSolver's empirical_prior), the parts that need no GPU: the host-side argument checks, start prior, stopping rule and
slab sizing under AddressSanitizer / UBSan (a stand-alone program, tests/host_stub/varpro_prior_args_stub.cpp; nothing is
preloaded), the ABI's refusals in front of any device work, what a call without voxels reports, the solver's construction rules,
the reference's preconditions on the inputs of every GPU case, and the numpy EM on a case worked by hand."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT
from varpro_prior_cases import cases, ref_kw
from varpro_prior_reference import em, em_step, likelihoods, normalise, population, reference_gain

from pyneapple_amd import _lib, api
from pyneapple_amd.models import BiExpModel
from pyneapple_amd.solvers import HipBayesGridSolver, HipBayesVarProSolver

NAME = "pnx_curvefit_varpro_prior_em_f64"


# ---- the argument checks as a stand-alone program under the sanitizers
@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("stub") / "varpro_prior_args_stub")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "pyneapple_amd", "csrc"), os.path.join(ROOT, "tests", "host_stub", "varpro_prior_args_stub.cpp"), "-o", exe]
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
    assert "varpro prior args stub ok" in _run_stub(stub)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("n_b", [1, 8, 16, 32, 33, 64, 128])
def test_python_slab_width_is_the_kernels(stub, n_b, k):
    assert int(_run_stub(stub, n_b, k)) == api.varpro_prior_slab_atoms(n_b, k) <= api.varpro_posterior_slab_atoms(n_b, k)


# ---- the ABI without a device
def _call(o, n_vox=1, n_atoms=2, nl=None, log_prior=None, noise_sd=0.0, amplitudes=1, n_iter=3, pseudo_count=0.0, rel_tol=0.0, out=True,
          lo=None, fixed=None):
    n = o.n_free
    nl = np.array([[0.1, 0.2], [0.01, 0.02], [0.001, 0.002]]) if nl is None else np.ascontiguousarray(nl, float)
    lo = np.zeros(n) if lo is None else np.ascontiguousarray(lo, float)
    hi = np.ones(n)
    fixed = None if fixed is None else np.ascontiguousarray(fixed, float)
    b, y = np.zeros(128), np.ones(128)
    res = dict(log_prior=np.full(max(n_atoms, 1), 9.0), loglik=np.full(max(min(n_iter, 1000), 0) + 1, 9.0), done=C.c_int(-7), n_eff=C.c_int64(-7))
    lp = None if log_prior is None else np.ascontiguousarray(log_prior, float)
    rc = getattr(_lib.load(), NAME)(C.byref(o), n_vox, _lib.ptr(b), _lib.ptr(y), n_atoms, _lib.ptr(nl), _lib.ptr(fixed), _lib.ptr(lo),
                                    _lib.ptr(hi), _lib.ptr(lp), noise_sd, amplitudes, n_iter, pseudo_count, rel_tol,
                                    _lib.ptr(res["log_prior"]) if out else None, _lib.ptr(res["loglik"]), C.byref(res["done"]),
                                    C.byref(res["n_eff"]), 0, 0, None)
    return rc, res


def tri():
    return api.make_opts("tri_s0", 32, jac="analytic")


def test_symbol_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnx.h")).read(), flags=re.S)
    assert re.search(r"PNX_API\s+int\s+" + NAME + r"\s*\(", text)
    assert NAME in _lib.ABI_SYMBOLS
    fn = getattr(_lib.load(), NAME)
    assert len(fn.argtypes) == 22 and fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NAME in [ln.split()[-1] for ln in out.splitlines() if ln.strip()]


def test_abi_refusals_need_no_device():
    for bad in (0, 1001):
        assert _call(tri(), n_iter=bad)[0] == -1 and "n_iter" in _lib.last_error() and "varpro prior" in _lib.last_error()
    for bad in (-1.0, float("nan"), float("inf")):
        assert _call(tri(), pseudo_count=bad)[0] == -1 and "pseudo_count" in _lib.last_error()
        assert _call(tri(), rel_tol=bad)[0] == -1 and "rel_tol" in _lib.last_error()
        assert _call(tri(), noise_sd=bad)[0] == -1 and "noise_sd" in _lib.last_error()
    assert _call(tri(), out=False)[0] == -1 and "log_prior_out" in _lib.last_error()
    assert _call(tri(), log_prior=[-np.inf, -np.inf])[0] == -1 and "log_prior excludes every atom" in _lib.last_error()
    assert _call(tri(), log_prior=[0.0, np.nan])[0] == -1 and "log_prior" in _lib.last_error()
    assert _call(tri(), amplitudes=2)[0] == -1 and "marginal_amplitudes=2" in _lib.last_error()
    # the posterior's own refusals, through varpro_check_args unchanged
    for idx, word in ((0, "fraction"), (5, "S0")):  # a fixed fraction, a fixed S0
        o = api.make_opts("tri_s0", 32, fixed_idx=[idx], jac="analytic")
        assert _call(o, fixed=[0.3])[0] == -2 and word in _lib.last_error() and "fixed" in _lib.last_error()
    lo = np.zeros(6)
    lo[5] = -1e-300
    assert _call(tri(), lo=lo)[0] == -1 and "lo_S0" in _lib.last_error()
    for n_atoms in (0, 4097):
        assert _call(tri(), n_atoms=n_atoms)[0] == -1 and "n_atoms" in _lib.last_error()
    assert _call(tri(), nl=[[0.1, 0.2], [0.01, 0.2], [0.001, 0.002]])[0] == -1 and "equal rates" in _lib.last_error()
    assert _call(api.make_opts("tri_s0", 32, per_voxel=True, jac="analytic"))[0] == -2 and "per_voxel_p0_bounds" in _lib.last_error()
    rc, res = _call(tri(), n_iter=0)  # a refused call writes nothing
    assert rc == -1 and (res["log_prior"] == 9.0).all() and (res["loglik"] == 9.0).all() and res["done"].value == -7
    if _lib.device_count() == 0:  # valid calls stop at the device
        assert _call(tri(), log_prior=[-np.inf, -1.0])[0] == -3
        assert _call(tri(), amplitudes=0, noise_sd=0.02, pseudo_count=0.5, rel_tol=1e-6)[0] == -3


def test_a_call_without_voxels_returns_the_normalised_start():
    """n_vox = 0 needs no device: PNX_OK, the start prior normalised (-inf kept), done = 0, n_eff = 0, loglik[0] = 0, NaN behind."""
    nl = np.array([[0.1, 0.2, 0.3, 0.4], [0.01, 0.02, 0.03, 0.04], [0.001, 0.002, 0.003, 0.004]])
    lp = np.array([np.log(3.0) + 5.0, -np.inf, 5.0, -np.inf])
    rc, res = _call(tri(), n_vox=0, n_atoms=4, nl=nl, log_prior=lp, n_iter=3)
    assert rc == 0 and res["done"].value == 0 and res["n_eff"].value == 0
    np.testing.assert_allclose(res["log_prior"][[0, 2]], np.log([0.75, 0.25]), rtol=0, atol=1e-15)
    assert (res["log_prior"][[1, 3]] == -np.inf).all()
    assert res["loglik"][0] == 0.0 and np.isnan(res["loglik"][1:]).all()
    rc, res = _call(tri(), n_vox=0, n_iter=1)
    assert rc == 0 and res["log_prior"].tobytes() == normalise(None, 2).tobytes()


# ---- the solver's construction rules
def _solver(**kw):
    bounds = {"f1": (0.0, 1.0), "D1": (1e-5, 0.5), "D2": (1e-5, 0.5), "S0": (0.0, 10.0)}
    return HipBayesVarProSolver(BiExpModel(fit_s0=True), rates={"D1": [0.1, 0.05], "D2": [0.002, 0.001]}, bounds=bounds, **kw)


def test_solver_option_rules_are_the_grid_solvers():
    assert _solver().empirical_prior is None and _solver(empirical_prior=False).empirical_prior is None
    assert _solver(empirical_prior=True).empirical_prior == {"n_iter": 20, "pseudo_count": 0.0, "rel_tol": 1e-6, "max_voxels": None}
    assert _solver(empirical_prior={"n_iter": 3, "max_voxels": 100}).empirical_prior == {"n_iter": 3, "pseudo_count": 0.0, "rel_tol": 1e-6,
                                                                                          "max_voxels": 100}
    assert HipBayesVarProSolver._empirical_prior_options.__func__ is HipBayesGridSolver._empirical_prior_options.__func__
    for bad, word in (({"n_iter": 0}, "n_iter"), ({"n_iter": 1001}, "n_iter"), ({"n_iter": 2.5}, "n_iter"), ({"pseudo_count": -1}, "pseudo_count"),
                      ({"rel_tol": float("nan")}, "rel_tol"), ({"max_voxels": 0}, "max_voxels"), ({"steps": 3}, "unknown keys"), ("yes", "must be None")):
        with pytest.raises(ValueError, match=word):
            _solver(empirical_prior=bad)
        with pytest.raises(ValueError) as grid:  # the same message from the grid solver's own rule
            HipBayesGridSolver._empirical_prior_options(bad)
        with pytest.raises(ValueError) as vp:
            HipBayesVarProSolver._empirical_prior_options(bad)
        assert str(grid.value) == str(vp.value)


# ---- the inputs of the GPU cases, chosen on the CPU
@pytest.mark.parametrize("name", sorted(cases()))
def test_reference_preconditions_of_the_gpu_cases(name):
    """The reference alone on the inputs of every one-update GPU case: eps_v <= 1e-6 in wide_box, the explicit 1e-3 for the
    narrow-box case only (varpro_posterior_reference.reference asserts it), and a finite one-step result."""
    c = cases()[name]
    assert c["max_eps"] == (1e-3 if name == "narrow-box" else 1e-6)
    l0, eps0, fin = likelihoods(c["model"], c["b"], c["y"], c["atoms"], c["lo"], c["hi"], **ref_kw(c))
    assert fin.all() and (eps0 <= c["max_eps"]).all()
    lp0 = normalise(c["kw"].get("log_prior"), c["atoms"].shape[1])
    S, lp1, ll = em_step(l0, lp0, fin)
    assert np.isfinite(ll) and abs(S.sum() - len(l0)) <= 1e-9 * len(l0) and (lp1[np.isinf(lp0)] == -np.inf).all()


def test_reference_gain_on_the_narrow_population():
    """What tests/test_gpu_varpro_prior.py::test_it_earns_its_keep holds the library to: numpy alone, seed 0, 1000 voxels, 5 % noise,
    30 updates.  learned / uniform of the median |error| of the posterior mean: f1 0.564, D1 0.833, D2 0.655 with the noise known,
    0.604, 0.838, 0.681 marginalised -- a fraction and a rate below 0.9 in both modes."""
    for noise_sd, want in ((0.05, [0.564, 0.833, 0.655]), (0.0, [0.604, 0.838, 0.681])):
        ratio, _, _ = reference_gain(1000, 0, noise_sd)
        np.testing.assert_allclose(ratio, want, atol=2e-3)
        assert ratio[0] < 0.9 and ratio[2] < 0.9
    assert population(5)[3].shape == (2, 91)


# ---- worked by hand
def test_two_voxels_two_atoms_by_hand():
    """l = [[0, log 3], [log 3, 0]] under the uniform start: L_v = log(0.5 + 1.5) = log 2, W = [[1/4, 3/4], [3/4, 1/4]], S = [1, 1],
    pi = [1/2, 1/2].  With the first voxel alone: S = [1/4, 3/4], and a pseudo-count of 1/2 gives pi = [(1/4 + 1/2) / 2, (3/4 + 1/2) / 2].
    An atom at -inf stays there and the other takes everything."""
    l0 = np.log(np.array([[1.0, 3.0], [3.0, 1.0]]))
    fin = np.array([True, True])
    S, lp, ll = em_step(l0, normalise(None, 2), fin)
    np.testing.assert_allclose(S, [1.0, 1.0], atol=1e-15)
    np.testing.assert_allclose(lp, np.log([0.5, 0.5]), atol=1e-15)
    assert abs(ll - 2 * np.log(2.0)) < 1e-15
    S, lp, ll = em_step(l0, normalise(None, 2), np.array([True, False]), alpha=0.5)
    np.testing.assert_allclose(S, [0.25, 0.75], atol=1e-15)
    np.testing.assert_allclose(np.exp(lp), [0.375, 0.625], atol=1e-15)
    S, lp, ll = em_step(l0, normalise([0.0, -np.inf], 2), fin)
    assert S.tolist() == [2.0, 0.0] and lp[0] == 0.0 and lp[1] == -np.inf and abs(ll - np.log(3.0)) < 1e-15
    lp2, trace = em(l0, normalise(None, 2), fin, 0.0, 2)  # the symmetric case is a fixed point: the trace is flat
    np.testing.assert_allclose(lp2, np.log([0.5, 0.5]), atol=1e-15)
    assert trace.shape == (3,) and np.ptp(trace) < 1e-15

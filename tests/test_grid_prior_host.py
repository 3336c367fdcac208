"""The empirical-Bayes prior over the grid (pnx_curvefit_grid_prior_em_f64, api.grid_prior_em, HipBayesGridSolver's
empirical_prior), the parts that need no GPU: the host-side argument checks, start prior, stopping rule and slab sizing under
AddressSanitizer / UBSan (a stand-alone program, tests/host_stub/grid_prior_args_stub.cpp), the ABI's refusals in front of any
device work, what a call without voxels reports, the solver's construction rules, and the numpy EM itself on a case worked by hand."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT
from grid_prior_reference import em, em_step, normalise, step_bounds

from pyneapple_amd import _lib, api, synth
from pyneapple_amd.models import BiExpModel, TriExpModel
from pyneapple_amd.solvers import HipBayesGridSolver

NAME = "pnx_curvefit_grid_prior_em_f64"


# ---- the argument checks as a stand-alone program under the sanitizers
@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("stub") / "grid_prior_args_stub")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "pyneapple_amd", "csrc"), os.path.join(ROOT, "tests", "host_stub", "grid_prior_args_stub.cpp"), "-o", exe]
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
    """Every invalid argument refused by name (the EM's four and the posterior's), the edges accepted, the start prior normalised
    with its -inf entries kept, the stopping rule, the NaN tail of the trace, the slab inside the LDS budget for every n_b."""
    assert "grid prior args stub ok" in _run_stub(stub)


@pytest.mark.parametrize("n_b", [1, 8, 16, 32, 33, 64, 128])
def test_python_slab_width_is_the_kernels(stub, n_b):
    assert int(_run_stub(stub, n_b)) == api.grid_prior_slab_atoms(n_b)


# ---- the ABI without a device
def _call(o, n_vox=1, n_atoms=4, atoms=None, log_prior=None, noise_sd=0.0, project=0, n_iter=3, pseudo_count=0.0, rel_tol=0.0, out=True):
    n = o.n_free
    atoms = np.full((n, max(n_atoms, 1)), 0.5) if atoms is None else np.ascontiguousarray(atoms, float)
    lo, hi = np.zeros(n), np.ones(n)
    b, y = np.zeros(128), np.ones(128)
    res = dict(log_prior=np.full(max(n_atoms, 1), 9.0), loglik=np.full(max(min(n_iter, 1000), 0) + 1, 9.0), done=C.c_int(-7), n_eff=C.c_int64(-7))
    lp = None if log_prior is None else np.ascontiguousarray(log_prior, float)
    rc = _lib.load().pnx_curvefit_grid_prior_em_f64(C.byref(o), n_vox, _lib.ptr(b), _lib.ptr(y), n_atoms, _lib.ptr(atoms), None, _lib.ptr(lo),
                                                    _lib.ptr(hi), project, _lib.ptr(lp), noise_sd, n_iter, pseudo_count, rel_tol,
                                                    _lib.ptr(res["log_prior"]) if out else None, _lib.ptr(res["loglik"]),
                                                    C.byref(res["done"]), C.byref(res["n_eff"]), 0, 0, None)
    return rc, res


def test_symbol_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnx.h")).read(), flags=re.S)
    assert re.search(r"PNX_API\s+int\s+" + NAME + r"\s*\(", text)
    assert NAME in _lib.ABI_SYMBOLS
    fn = getattr(_lib.load(), NAME)
    assert len(fn.argtypes) == 22 and fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NAME in [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    assert _lib.load().pnx_version() == 2


def test_abi_refusals_need_no_device():
    mk = api.make_opts
    for bad in (0, -1, 1001):
        assert _call(mk("bi_reduced", 32), n_iter=bad)[0] == -1 and "n_iter" in _lib.last_error()
    for bad in (-1.0, float("nan"), float("inf")):
        assert _call(mk("bi_reduced", 32), pseudo_count=bad)[0] == -1 and "pseudo_count" in _lib.last_error()
        assert _call(mk("bi_reduced", 32), rel_tol=bad)[0] == -1 and "rel_tol" in _lib.last_error()
        assert _call(mk("bi_reduced", 32), noise_sd=bad)[0] == -1 and "noise_sd" in _lib.last_error()
    assert _call(mk("bi_reduced", 32), out=False)[0] == -1 and "log_prior_out" in _lib.last_error()
    for prior in ([0.0, np.nan, 0.0, 0.0], [0.0, np.inf, 0.0, 0.0], [-np.inf] * 4):
        assert _call(mk("bi_reduced", 32), log_prior=prior)[0] == -1 and "log_prior" in _lib.last_error()
    for n_atoms in (0, 4097):
        assert _call(mk("bi_reduced", 32), n_atoms=n_atoms)[0] == -1 and "n_atoms" in _lib.last_error()
    assert _call(mk("bi_reduced", 32), project=1)[0] == -1 and "S0" in _lib.last_error()
    atoms = np.full((3, 4), 0.5)
    atoms[1, 2] = 1.5
    assert _call(mk("bi_reduced", 32), atoms=atoms)[0] == -1 and "atom 2" in _lib.last_error()
    assert _call(mk("bi_reduced", 32, per_voxel=True))[0] == -2 and "per_voxel_p0_bounds" in _lib.last_error()
    o = mk("bi_reduced", 32)
    o.queue_order = np.zeros(4, np.int32).ctypes.data
    assert _call(o)[0] == -2 and "queue_order" in _lib.last_error()
    rc, res = _call(mk("bi_reduced", 32), n_iter=0)  # a refused call writes nothing
    assert rc == -1 and (res["log_prior"] == 9.0).all() and (res["loglik"] == 9.0).all() and res["done"].value == -7
    if _lib.device_count() == 0:  # valid calls stop at the device
        assert _call(mk("bi_reduced", 32), log_prior=[-np.inf, -np.inf, -1.0, -np.inf])[0] == -3
        assert _call(mk("bi_s0", 32), project=1, noise_sd=0.02, pseudo_count=0.5, rel_tol=1e-6)[0] == -3


def test_a_call_without_voxels_returns_the_normalised_start():
    """n_vox = 0 needs no device: PNX_OK, the start prior normalised (-inf kept), done = 0, n_eff = 0, loglik[0] = 0, NaN behind."""
    lp = np.array([np.log(3.0) + 5.0, -np.inf, 5.0, -np.inf])
    rc, res = _call(api.make_opts("bi_reduced", 32), n_vox=0, log_prior=lp, n_iter=3)
    assert rc == 0 and res["done"].value == 0 and res["n_eff"].value == 0
    np.testing.assert_allclose(res["log_prior"][[0, 2]], np.log([0.75, 0.25]), rtol=0, atol=1e-15)
    assert (res["log_prior"][[1, 3]] == -np.inf).all()
    assert res["log_prior"].tobytes() == normalise(lp, 4).tobytes()
    assert res["loglik"][0] == 0.0 and np.isnan(res["loglik"][1:]).all()
    rc, res = _call(api.make_opts("bi_reduced", 32), n_vox=0, n_atoms=4, n_iter=1)
    assert rc == 0 and (res["log_prior"] == -np.log(4.0)).all()


def test_no_cpu_fallback_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is visible here")
    b, y, _ = synth.make_numpy("tri_reduced", 4, 32)
    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    with pytest.raises(_lib.PnxError):
        api.grid_prior_em("tri_reduced", b, y, p0[:, None], lo, hi)
    with pytest.raises(_lib.PnxError):
        _solver(grid={"f1": [0.1, 0.2]}, empirical_prior=True).fit(b, y)


def test_api_refuses_a_wrong_prior_length_and_per_voxel_fixed_maps(monkeypatch):
    monkeypatch.setattr(_lib, "require_device", lambda: None)
    b, y, _ = synth.make_numpy("tri_reduced", 4, 32)
    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    with pytest.raises(ValueError, match="log_prior"):
        api.grid_prior_em("tri_reduced", b, y, p0[:, None], lo, hi, log_prior=np.zeros(2))
    with pytest.raises(ValueError, match="per-voxel fixed"):
        api.grid_prior_em("tri_reduced", b, y, p0[[0, 1, 2, 4], None], lo[[0, 1, 2, 4]], hi[[0, 1, 2, 4]], fixed_idx=[3], fixed_vals=np.ones((1, 4)))
    with pytest.raises(_lib.PnxError, match="n_iter"):
        api.grid_prior_em("tri_reduced", b, y, p0[:, None], lo, hi, n_iter=10 ** 9)


# ---- the solver's construction rules
def _tri():
    names, p0, lo, hi = synth.shared_arrays("tri_reduced")
    return dict(p0=dict(zip(names, map(float, p0))), bounds={n: (float(a), float(b)) for n, a, b in zip(names, lo, hi)})


def _solver(model=None, **kw):
    return HipBayesGridSolver(model or TriExpModel(), **{**_tri(), **kw})


def test_solver_empirical_prior_rules():
    defaults = {"n_iter": 20, "pseudo_count": 0.0, "rel_tol": 1e-6, "max_voxels": None}
    for off in (None, False):
        assert _solver(grid={"f1": [0.1, 0.2]}, empirical_prior=off).empirical_prior is None
    assert _solver(grid={"f1": [0.1, 0.2]}).empirical_prior is None
    assert _solver(grid={"f1": [0.1, 0.2]}, empirical_prior=True).empirical_prior == defaults
    assert _solver(grid={"f1": [0.1, 0.2]}, empirical_prior={}).empirical_prior == defaults
    # the TOML loader's call: a table arrives as a plain dict, integers where the file holds integers
    s = _solver(grid={"f1": [0.1, 0.2]}, max_iter=100, tol=1e-6, method="trf", empirical_prior={"n_iter": 5, "pseudo_count": 1, "max_voxels": 4096})
    assert s.empirical_prior == {"n_iter": 5, "pseudo_count": 1.0, "rel_tol": 1e-6, "max_voxels": 4096}
    assert isinstance(s.empirical_prior["pseudo_count"], float) and s.solver_kwargs == {"method": "trf"}
    with pytest.raises(ValueError, match=r"unknown keys \['iterations', 'tol'\]"):
        _solver(grid={"f1": [0.1]}, empirical_prior={"iterations": 5, "tol": 1.0, "n_iter": 3})
    bad = [{"n_iter": 0}, {"n_iter": 1001}, {"n_iter": 2.5}, {"n_iter": True}, {"pseudo_count": -1.0}, {"pseudo_count": float("nan")},
           {"rel_tol": -1e-9}, {"rel_tol": float("inf")}, {"max_voxels": 0}, {"max_voxels": 1.5}]
    for value in bad:
        with pytest.raises(ValueError, match=next(iter(value))):
            _solver(grid={"f1": [0.1]}, empirical_prior=value)
    for value in ("yes", 3, [("n_iter", 3)]):
        with pytest.raises(ValueError, match="empirical_prior"):
            _solver(grid={"f1": [0.1]}, empirical_prior=value)
    # the learned prior never replaces the caller's
    lp = np.array([0.0, -1.0])
    s = _solver(grid={"f1": [0.1, 0.2]}, log_prior=lp, empirical_prior=True)
    assert s.log_prior.tolist() == lp.tolist()
    doc = HipBayesGridSolver.__doc__
    assert "empirical_prior" in doc and "37 voxels" in doc and "very voxels it is applied to" in doc
    bi = dict(p0={"f1": 0.2, "D1": 0.01, "D2": 0.001, "S0": 900.0}, bounds={"f1": (0, 1), "D1": (1e-3, 0.1), "D2": (1e-5, 5e-3), "S0": (1.0, 5000.0)})
    assert HipBayesGridSolver(BiExpModel(fit_s0=True), {"D1": [0.01, 0.05]}, **bi, empirical_prior={"n_iter": 2}).project is True


def test_entry_point_is_unchanged():
    text = open(os.path.join(ROOT, "pyproject.toml")).read()
    group = text.split('[project.entry-points."pyneapple.solvers"]', 1)[1].split("\n[", 1)[0]
    assert re.search(r'^hip_bayes_grid = "pyneapple_amd\.solvers:HipBayesGridSolver"$', group, flags=re.M) and "prior" not in group


# ---- the numpy EM itself, worked by hand
def test_reference_em_on_three_atoms_and_four_voxels():
    """Likelihoods P[v, g] = [[4,1,1],[4,1,1],[1,4,1],[1,1,1]], uniform start.  Update 1: W = P / row sums (6, 6, 6, 3), so
    S = (11/6, 8/6, 5/6), pi = (11, 8, 5) / 24, log-likelihood 3 log 2.  Update 2 from that pi: row sums of pi P are 57/24, 57/24,
    48/24, 1, so S = (2 * 44/57 + 11/48 + 11/24, 2 * 8/57 + 32/48 + 8/24, 2 * 5/57 + 5/48 + 5/24) and the log-likelihood is
    2 log(57/24) + log 2."""
    P = np.array([[4.0, 1, 1], [4, 1, 1], [1, 4, 1], [1, 1, 1]])
    l0, fin = np.log(P), np.ones(4, bool)
    lp0 = normalise(None, 3)
    S, lp1, ll0 = em_step(l0, lp0, fin)
    np.testing.assert_allclose(S, [11 / 6, 8 / 6, 5 / 6], rtol=1e-14)
    np.testing.assert_allclose(np.exp(lp1), np.array([11, 8, 5]) / 24, rtol=1e-14)
    assert ll0 == pytest.approx(3 * np.log(2.0), rel=1e-14)  # sum_g P / 3 = 2, 2, 2, 1
    S2, lp2, ll1 = em_step(l0, lp1, fin)
    want = np.array([2 * 44 / 57 + 11 / 48 + 11 / 24, 2 * 8 / 57 + 32 / 48 + 8 / 24, 2 * 5 / 57 + 5 / 48 + 5 / 24])
    np.testing.assert_allclose(S2, want, rtol=1e-14)
    np.testing.assert_allclose(np.exp(lp2), want / 4, rtol=1e-14)
    assert ll1 == pytest.approx(2 * np.log(57 / 24) + np.log(2.0), rel=1e-14) and ll1 > ll0
    lp, trace = em(l0, lp0, fin, n_iter=2)
    assert lp.tobytes() == lp2.tobytes() and trace.shape == (3,) and trace[0] == ll0 and trace[1] == ll1 and trace[2] >= trace[1]
    assert abs(np.exp(lp).sum() - 1) < 1e-15
    # an excluded atom stays excluded and takes no weight; a non-finite voxel takes no part; the pseudo-count enters both sums
    lpx = normalise(np.array([0.0, -np.inf, 0.0]), 3)
    fin3 = np.array([True, True, False, True])
    bad = l0.copy()
    bad[2] = np.nan
    S, lp1, ll = em_step(bad, lpx, fin3, alpha=0.5)
    np.testing.assert_allclose(S, [0.8 + 0.8 + 0.5, 0.0, 0.2 + 0.2 + 0.5], rtol=1e-14)
    np.testing.assert_allclose(np.exp(lp1), [(2.1 + 0.5) / 4, 0.0, (0.9 + 0.5) / 4], rtol=1e-14)
    assert lp1[1] == -np.inf and ll == pytest.approx(2 * np.log(2.5) + 0.0, rel=1e-14)
    # no finite voxel: the prior stays, the log-likelihood is the empty sum
    S, same, ll = em_step(bad, lpx, np.zeros(4, bool))
    assert same.tobytes() == lpx.tobytes() and ll == 0.0 and (S == 0).all()
    bd = step_bounds(l0, lp0, np.full(4, 1e-12), fin, np.array([11 / 6, 8 / 6, 5 / 6]))
    assert 2e-12 < bd["rel"] < 3e-12 and bd["lp"] == pytest.approx(bd["rel"], rel=1e-6) and bd["loglik"] > 4e-12

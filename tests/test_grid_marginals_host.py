"""The marginals of the grid posterior (pnx_curvefit_grid_marginals_f64, api.grid_marginals, HipBayesGridSolver's marginals), the
parts that need no GPU: the host-side argument checks, the table of bin indices and the choice of the instantiation under
AddressSanitizer / UBSan (a stand-alone program, tests/host_stub/grid_marginal_args_stub.cpp), the ABI's refusals in front of any
device work, the solver's option rules, the np.unique derivation of the binning, and the numpy reference against a brute-force loop."""
from __future__ import annotations

import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT
from grid_marginal_reference import marginals, quantile_bins, weights

from pyneapple_amd import _lib, api, synth
from pyneapple_amd.models import BiExpModel, TriExpModel
from pyneapple_amd.solvers import HipBayesGridSolver

NAME = "pnx_curvefit_grid_marginals_f64"


# ---- the argument checks as a stand-alone program under the sanitizers
@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("stub") / "grid_marginal_args_stub")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "pyneapple_amd", "csrc"), os.path.join(ROOT, "tests", "host_stub", "grid_marginal_args_stub.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode and any(s in b.stderr for s in ("cannot find -lasan", "cannot find -lubsan")):
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-4000:]
    return exe


def test_argument_checks_are_clean_under_sanitizers(stub):
    """Every refusal by name -- B = 0 and 129, a bin out of range, an atom off its bin's value, values that do not ascend, S0 bins
    under projection, a level at 0 or 1, n_q = 9, NULL outputs, the posterior's own -- the edges accepted, the table of global
    bin indices with its -1 padding, 2 / 4 / 8 chunks, the table inside the slab for every n_b."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    r = subprocess.run([stub], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-6000:]
    assert r.returncode == 0, out[-4000:]
    assert "grid marginal args stub ok" in r.stdout


# ---- the ABI without a device
def _call(o, atoms, n_bins, bin_of, bin_value, probs=(0.5,), n_vox=1, project=0, noise_sd=0.0, marginal=True, quantile=True, n_q=None):
    n = o.n_free
    atoms = np.ascontiguousarray(atoms, float)
    lo, hi = np.zeros(n), np.ones(n)
    b, y = np.zeros(128), np.ones(128)
    n_bins, bin_of = np.ascontiguousarray(n_bins, np.int32), np.ascontiguousarray(bin_of, np.int32)
    bin_value, probs = np.ascontiguousarray(bin_value, float), np.ascontiguousarray(probs, float)
    res = dict(marginal=np.full((max(int(n_bins.sum()), 1), max(n_vox, 1)), 9.0), quantile=np.full((8, n, max(n_vox, 1)), 9.0),
               log_evidence=np.full(max(n_vox, 1), 9.0))
    rc = _lib.load().pnx_curvefit_grid_marginals_f64(C.byref(o), n_vox, _lib.ptr(b), _lib.ptr(y), atoms.shape[1], _lib.ptr(atoms), None,
                                                     _lib.ptr(lo), _lib.ptr(hi), project, None, noise_sd, _lib.ptr(n_bins), _lib.ptr(bin_of),
                                                     _lib.ptr(bin_value), len(probs) if n_q is None else n_q, _lib.ptr(probs),
                                                     _lib.ptr(res["marginal"]) if marginal else None,
                                                     _lib.ptr(res["quantile"]) if quantile else None, _lib.ptr(res["log_evidence"]), 0, 0, None)
    return rc, res


def _grid():
    """Three parameters on a 2 x 1 x 3 grid inside (0, 1): (atoms (n, 6), n_bins, bin_of, bin_value)."""
    cols = list(itertools.product([0.25, 0.75], [0.5], [0.2, 0.4, 0.6]))
    atoms = np.ascontiguousarray(np.array(cols).T)
    return (atoms, *api.grid_marginal_bins(atoms))


def test_symbol_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnx.h")).read(), flags=re.S)
    assert re.search(r"PNX_API\s+int\s+" + NAME + r"\s*\(", text)
    assert NAME in _lib.ABI_SYMBOLS
    fn = getattr(_lib.load(), NAME)
    assert len(fn.argtypes) == 23 and fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NAME in [ln.split()[-1] for ln in out.splitlines() if ln.strip()]


def test_abi_refusals_need_no_device():
    mk = lambda: api.make_opts("bi_reduced", 32)
    atoms, n_bins, bin_of, bin_value = _grid()
    err = lambda **kw: (_call(mk(), **{**dict(atoms=atoms, n_bins=n_bins, bin_of=bin_of, bin_value=bin_value), **kw})[0], _lib.last_error())
    rc, msg = err(n_bins=[0, 0, 0], bin_value=[0.5])
    assert rc == -1 and "sum n_bins = 0" in msg
    rc, msg = err(n_bins=[2, 1, 126], bin_value=np.linspace(0.1, 0.9, 129))
    assert rc == -1 and "129" in msg
    bad = bin_of.copy()
    bad[2, 4] = 3
    rc, msg = err(bin_of=bad)
    assert rc == -1 and "bin_of[2, 4]=3" in msg
    off = bin_value.copy()
    off[4] = 0.41
    rc, msg = err(bin_value=off)
    assert rc == -1 and "atom" in msg and "bin_value[4]" in msg
    desc = bin_value.copy()
    desc[[3, 4]] = desc[[4, 3]]
    rc, msg = err(bin_value=desc)
    assert rc == -1 and "ascending" in msg
    for p in (0.0, 1.0, float("nan")):
        rc, msg = err(probs=[0.5, p])
        assert rc == -1 and "probs[1]" in msg
    rc, msg = err(probs=[0.5] * 9)
    assert rc == -1 and "n_q=9" in msg
    rc, msg = err(marginal=False)
    assert rc == -1 and "marginal is NULL" in msg
    rc, msg = err(quantile=False)
    assert rc == -1 and "quantile is NULL" in msg
    rc, msg = err(noise_sd=-1.0)
    assert rc == -1 and "noise_sd" in msg
    # S0 bins under projection
    cols = list(itertools.product([0.25, 0.75], [0.5], [0.2, 0.4], [0.3, 0.6]))
    a4 = np.ascontiguousarray(np.array(cols).T)
    nb4, of4, val4 = api.grid_marginal_bins(a4)
    rc, _ = _call(api.make_opts("bi_s0", 32), a4, nb4, of4, val4, project=1)
    assert rc == -1 and "S0" in _lib.last_error() and "n_bins[3]=2" in _lib.last_error()
    rc, res = _call(mk(), atoms, n_bins, bin_of, bin_value, probs=[1.0])  # a refused call writes nothing
    assert rc == -1 and (res["marginal"] == 9.0).all() and (res["quantile"] == 9.0).all() and (res["log_evidence"] == 9.0).all()
    assert _call(mk(), atoms, n_bins, bin_of, bin_value, n_vox=0)[0] == 0  # no voxels: nothing to do, no device needed
    if _lib.device_count() == 0:  # valid calls stop at the device
        assert _call(mk(), atoms, n_bins, bin_of, bin_value)[0] == -3
        nb4, of4, val4 = api.grid_marginal_bins(a4, skip_rows=(3,))
        assert _call(api.make_opts("bi_s0", 32), a4, nb4, of4, val4, project=1, probs=(), quantile=False)[0] == -3


def test_no_cpu_fallback_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is visible here")
    b, y, _ = synth.make_numpy("tri_reduced", 4, 32)
    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    with pytest.raises(_lib.PnxError):
        api.grid_marginals("tri_reduced", b, y, p0[:, None], lo, hi)
    with pytest.raises(_lib.PnxError):
        _solver(grid={"f1": [0.1, 0.2]}, marginals=True).fit(b, y)


def test_api_refuses_a_malformed_binning(monkeypatch):
    monkeypatch.setattr(_lib, "require_device", lambda: None)
    b, y, _ = synth.make_numpy("tri_reduced", 4, 32)
    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    with pytest.raises(ValueError, match="bins must be"):
        api.grid_marginals("tri_reduced", b, y, p0[:, None], lo, hi, bins=(np.ones(4, np.int32), np.zeros((5, 1), np.int32), np.zeros(4)))
    with pytest.raises(ValueError, match="bins must be"):
        api.grid_marginals("tri_reduced", b, y, p0[:, None], lo, hi, bins=(np.ones(5, np.int32), np.zeros((5, 1), np.int32), np.zeros(4)))
    with pytest.raises(_lib.PnxError, match="n_q=9"):
        api.grid_marginals("tri_reduced", b, y, p0[:, None], lo, hi, quantiles=[0.5] * 9)


# ---- the solver's option rules
def _tri():
    names, p0, lo, hi = synth.shared_arrays("tri_reduced")
    return dict(p0=dict(zip(names, map(float, p0))), bounds={n: (float(a), float(b)) for n, a, b in zip(names, lo, hi)})


def _solver(model=None, **kw):
    return HipBayesGridSolver(model or TriExpModel(), **{**_tri(), **kw})


def test_solver_marginals_rules():
    default = {"quantiles": (0.025, 0.5, 0.975)}
    for off in (None, False):
        assert _solver(grid={"f1": [0.1, 0.2]}, marginals=off).marginals is None
    assert _solver(grid={"f1": [0.1, 0.2]}).marginals is None
    assert _solver(grid={"f1": [0.1, 0.2]}, marginals=True).marginals == default
    assert _solver(grid={"f1": [0.1, 0.2]}, marginals={}).marginals == default
    # the TOML loader's call: a table arrives as a plain dict, beside the arguments it always passes
    s = _solver(grid={"f1": [0.1, 0.2]}, max_iter=100, tol=1e-6, method="trf", marginals={"quantiles": [0.1, 0.9]})
    assert s.marginals == {"quantiles": (0.1, 0.9)} and s.solver_kwargs == {"method": "trf"}
    assert _solver(grid={"f1": [0.1]}, marginals={"quantiles": []}).marginals == {"quantiles": ()}
    assert _solver(grid={"f1": [0.1]}, marginals={"quantiles": 0.5}).marginals == {"quantiles": (0.5,)}
    with pytest.raises(ValueError, match=r"unknown keys \['levels', 'probs'\]"):
        _solver(grid={"f1": [0.1]}, marginals={"probs": [0.5], "levels": 1, "quantiles": [0.5]})
    for bad in ([0.0], [1.0], [0.5, -0.1], [float("nan")], [0.5] * 9, ["median"], "lots"):
        with pytest.raises(ValueError, match="quantiles"):
            _solver(grid={"f1": [0.1]}, marginals={"quantiles": bad})
    for value in ("yes", 3, [("quantiles", [0.5])]):
        with pytest.raises(ValueError, match="marginals"):
            _solver(grid={"f1": [0.1]}, marginals=value)
    # together with the learned prior; neither touches the other's options
    s = _solver(grid={"f1": [0.1, 0.2]}, empirical_prior={"n_iter": 3}, marginals=True)
    assert s.empirical_prior["n_iter"] == 3 and s.marginals == default
    doc = HipBayesGridSolver.__doc__
    assert "marginals" in doc and "[Fitting.solver.marginals]" in doc and "interpolated" in doc
    bi = dict(p0={"f1": 0.2, "D1": 0.01, "D2": 0.001, "S0": 900.0}, bounds={"f1": (0, 1), "D1": (1e-3, 0.1), "D2": (1e-5, 5e-3), "S0": (1.0, 5000.0)})
    assert HipBayesGridSolver(BiExpModel(fit_s0=True), {"D1": [0.01, 0.05]}, **bi, marginals=True).project is True


# ---- the binning derived from the atoms
def test_bins_of_a_cartesian_grid():
    grid = [[0.3, 0.1, 0.2], [5.0], [1e-3, 4e-3]]  # not sorted: itertools.product keeps the caller's order, the bins ascend
    atoms = np.array(list(itertools.product(*grid))).T
    n_bins, bin_of, bin_value = api.grid_marginal_bins(atoms)
    assert n_bins.dtype == np.int32 and bin_of.dtype == np.int32 and bin_value.dtype == np.float64
    assert n_bins.tolist() == [3, 1, 2] and bin_value.tolist() == [0.1, 0.2, 0.3, 5.0, 1e-3, 4e-3]
    assert bin_of[0].tolist() == [2, 2, 0, 0, 1, 1] and bin_of[1].tolist() == [0] * 6 and bin_of[2].tolist() == [0, 1] * 3
    off = np.concatenate([[0], np.cumsum(n_bins)])
    for k in range(3):
        assert (bin_value[off[k] + bin_of[k]] == atoms[k]).all()
    # a skipped row (the projected S0) has no bins and no values
    n_bins, bin_of, bin_value = api.grid_marginal_bins(atoms, skip_rows=(1,))
    assert n_bins.tolist() == [3, 0, 2] and bin_value.tolist() == [0.1, 0.2, 0.3, 1e-3, 4e-3] and (bin_of[1] == 0).all()


def test_bins_of_a_non_cartesian_atom_list():
    rng = np.random.default_rng(5)
    atoms = np.stack([rng.choice([0.1, 0.2, 0.7], 17), rng.uniform(0, 1, 17), np.full(17, 2.0)])
    atoms[1, 3] = atoms[1, 11]  # one repeated value among otherwise distinct ones
    n_bins, bin_of, bin_value = api.grid_marginal_bins(atoms)
    assert n_bins.tolist() == [len(set(atoms[0])), 16, 1] and bin_value.size == n_bins.sum()
    off = np.concatenate([[0], np.cumsum(n_bins)])
    for k in range(3):
        seg = bin_value[off[k]:off[k + 1]]
        assert (np.diff(seg) > 0).all() and (seg[bin_of[k]] == atoms[k]).all() and set(bin_of[k]) == set(range(n_bins[k]))
    assert bin_of[1, 3] == bin_of[1, 11]
    with pytest.raises(ValueError, match="n_free, n_atoms"):
        api.grid_marginal_bins(np.zeros(4))


# ---- the numpy reference against a brute-force loop
def test_reference_on_a_tiny_case():
    """Two voxels, five atoms (one excluded), two parameters with 2 and 3 bins: every sum written out by hand."""
    ell = np.log(np.array([[1.0, 2.0, 3.0, 0.0, 4.0], [5.0, 1.0, 1.0, 0.0, 3.0]]), where=[True, True, True, False, True],
                 out=np.full((2, 5), -np.inf))
    n_bins, bin_of = [2, 3], np.array([[0, 1, 0, 1, 1], [2, 0, 0, 1, 2]])
    W = weights(ell)
    np.testing.assert_allclose(W, np.array([[1, 2, 3, 0, 4], [5, 1, 1, 0, 3]]) / 10.0, rtol=1e-15)
    assert (W[:, 3] == 0).all()
    got = marginals(W, n_bins, bin_of)
    want = np.zeros((2, 5))
    for v in range(2):
        off = 0
        for k in range(2):
            for g in range(5):
                want[v, off + bin_of[k, g]] += W[v, g]
            off += n_bins[k]
    np.testing.assert_allclose(got, want, rtol=1e-15)
    np.testing.assert_allclose(got, [[0.4, 0.6, 0.5, 0.0, 0.5], [0.6, 0.4, 0.2, 0.0, 0.8]], rtol=1e-15)
    assert (got[:, 3] == 0).all()  # the bin only the excluded atom occupies: exactly 0
    # quantiles: the first bin whose running sum reaches the level; the last bin when none does
    cdf = np.cumsum(got[:, 2:], axis=1)  # [[0.5, 0.5, 1.0], [0.2, 0.2, 1.0]]
    q = quantile_bins(cdf, [0.1, 0.5, 0.6])
    assert q.tolist() == [[0, 0], [0, 2], [2, 2]]
    assert quantile_bins(np.array([[0.25, 0.5]]), [0.75]).tolist() == [[1]]

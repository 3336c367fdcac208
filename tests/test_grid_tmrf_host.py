"""The edge-preserving (Student-t) neighbourhood prior of the grid posterior (pnx_curvefit_grid_neighbour_wfield_f64,
pnx_curvefit_grid_posterior_wfield_f64, pnx_curvefit_grid_posterior_tmrf_f64; api.grid_neighbour_wfield / grid_posterior_wfield /
grid_posterior_tmrf; HipBayesGridSolver's spatial_prior keys "potential" and "dof"), the parts that need no GPU:
the numpy reference (its free energy never decreases, its Gaussian limit, a weight worked by hand), the solver's options, the
ABI's refusals in front of any device work, the symbols, and the host-side checks under AddressSanitizer / UBSan as a stand-alone
program (tests/host_stub/grid_tmrf_args_stub.cpp)."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT
import grid_mrf_reference as R
import grid_tmrf_reference as T
from grid_posterior_reference import reference as posterior_reference

from pyneapple_amd import _lib, api, synth
from pyneapple_amd.models import BiExpModel, TriExpModel
from pyneapple_amd.solvers import HipBayesGridSolver, HipBayesVarProSolver

GATHER, FIELD, DRIVER = ("pnx_curvefit_grid_neighbour_wfield_f64", "pnx_curvefit_grid_posterior_wfield_f64",
                         "pnx_curvefit_grid_posterior_tmrf_f64")


# ---- the numpy reference
@pytest.fixture(scope="module")
def small_phantom():
    ph = R.phantom(seed=0, noise=0.05, H=12, W=12)
    order, nb, start = R.colour_sort(ph["nb"], ph["colours"])
    return ph, order, nb, start


def _lam(ph, strength):
    return strength / (ph["atoms"].max(axis=1) - ph["atoms"].min(axis=1)) ** 2


def _monotone(F):
    F = np.array(F)
    assert (np.diff(F) >= -1e-9 * np.abs(F[1:])).all(), np.diff(F)
    return F


@pytest.mark.parametrize("strength", [1.0, 64.0])
@pytest.mark.parametrize("dof", [0.5, 4.0])
def test_reference_free_energy_never_decreases(small_phantom, strength, dof):
    """After the refresh of a colour's edge weights and after the colour's update: 1 + 4 sweeps x 2 colours x 2 values."""
    ph, order, nb, start = small_phantom
    _, delta, F = T.tmrf("bi_reduced", ph["b"], ph["y"][order], ph["atoms"], ph["lo"], ph["hi"], nb, start, _lam(ph, strength), dof, 4,
                         noise_sd=0.05, trace_free_energy=True)
    F = _monotone(F)
    assert F.size == 1 + 4 * 2 * 2 and len(delta) == 4
    assert F[-1] > F[0] and delta[-1] < delta[0]


def test_reference_free_energy_never_decreases_with_four_colours():
    ph = R.phantom(seed=0, noise=0.05, H=12, W=12)
    nb8, col = api.grid_neighbours(np.ones((12, 12), bool), 8)
    order, nb, start = R.colour_sort(nb8, col)
    assert len(start) == 5 and nb.shape[1] == 8
    _, delta, F = T.tmrf("bi_reduced", ph["b"], ph["y"][order], ph["atoms"], ph["lo"], ph["hi"], nb, start, _lam(ph, 64.0), 4.0, 3,
                         noise_sd=0.05, trace_free_energy=True)
    F = _monotone(F)
    assert F.size == 1 + 3 * 4 * 2 and F[-1] > F[0]


def test_reference_gaussian_limit(small_phantom):
    """dof = 1e300: nu + K and nu + s both round to nu for every s below half an ulp of 1e300 (5e283), so w is exactly 1, the
    weighted sums are the Gaussian gather's sums term for term and W_v = n_v: the derived bound is zero, the bytes are the same."""
    ph, order, nb, start = small_phantom
    y, lam = ph["y"][order], _lam(ph, 64.0)
    args = ("bi_reduced", ph["b"], y, ph["atoms"], ph["lo"], ph["hi"], nb, start, lam)
    st, delta, _ = T.tmrf(*args, 1e300, 3, noise_sd=0.05)
    ref, delta_ref, _ = R.mrf(*args, 3, noise_sd=0.05)
    for key in ("mean", "var", "log_evidence", "ess", "map_atom"):
        assert np.asarray(st[key]).tobytes() == np.asarray(ref[key]).tobytes(), key
    assert delta == delta_ref and (st["field_w"] == st["field_n"]).all() and st["field_n"].max() == 4
    finite = T.tmrf(*args, 4.0, 3, noise_sd=0.05)[0]  # and a finite dof is another answer
    assert np.abs(finite["mean"] - ref["mean"]).max() > 0


def test_reference_without_a_precision_is_the_plain_posterior(small_phantom):
    ph, order, nb, start = small_phantom
    y = ph["y"][order]
    st, delta, _ = T.tmrf("bi_reduced", ph["b"], y, ph["atoms"], ph["lo"], ph["hi"], nb, start, np.zeros(3), 4.0, 3, noise_sd=0.05)
    ref = posterior_reference("bi_reduced", ph["b"], y, ph["atoms"], ph["lo"], ph["hi"], noise_sd=0.05)
    for key in ("mean", "var", "log_evidence", "ess", "map_atom"):
        assert np.asarray(st[key]).tobytes() == np.asarray(ref[key]).tobytes(), key
    assert delta == [0.0, 0.0, 0.0]


def test_reference_weight_of_a_three_voxel_chain():
    """0 - 1 - 2, two rows, the second without a precision (K = 1): the formula typed out."""
    nb = np.array([[1, -1], [0, 2], [1, -1]], np.int32)
    mean = np.array([[1.0, 1.5, 4.0], [10.0, 20.0, 30.0]])
    sd = np.array([[0.5, 0.25, 1.0], [3.0, 3.0, 3.0]])
    centre, lam, nu = np.array([2.0, 5.0]), np.array([2.0, 0.0]), 4.0
    g = T.gather(nb, mean, sd, centre, lam, nu)
    s01 = 2.0 * (0.5 * 0.5 + 0.25 * 0.25 + (1.0 - 1.5) * (1.0 - 1.5))
    s12 = 2.0 * (0.25 * 0.25 + 1.0 * 1.0 + (1.5 - 4.0) * (1.5 - 4.0))
    w01, w12 = (nu + 1) / (nu + s01), (nu + 1) / (nu + s12)
    assert g["edge"].tolist() == [[w01, 0.0], [w01, w12], [w12, 0.0]]
    assert g["w"].tolist() == [w01, w01 + w12, w12] and g["n"].tolist() == [1, 2, 1]
    assert g["q"][0].tolist() == [2.0 * (w01 * (1.5 - 2.0)), 2.0 * (w01 * (1.0 - 2.0) + w12 * (4.0 - 2.0)), 2.0 * (w12 * (1.5 - 2.0))]
    assert (g["q"][1] == 0.0).all() and w12 < 0.5 < w01  # the edge with the jump counts for less
    lam2 = np.array([2.0, 0.01])  # both rows (K = 2)
    g2 = T.gather(nb, mean, sd, centre, lam2, nu)
    assert g2["edge"][0, 0] == (nu + 2) / (nu + (s01 + 0.01 * (3.0 * 3.0 + 3.0 * 3.0 + (10.0 - 20.0) * (10.0 - 20.0))))
    part = T.gather(nb, mean, sd, centre, lam, nu, first=1, count=2)  # a range is the same numbers
    assert part["q"].tobytes() == g["q"][:, 1:].tobytes() and part["w"].tolist() == g["w"][1:].tolist()
    mean[:, 1] = np.nan  # a non-finite voxel: nothing for itself, absent for its neighbours
    g3 = T.gather(nb, mean, sd, centre, lam, nu)
    assert g3["n"].tolist() == [0, 0, 0] and (g3["w"] == 0).all() and (g3["q"] == 0).all() and (g3["edge"] == 0).all()


# ---- the solver's options
def _tri():
    names, p0, lo, hi = synth.shared_arrays("tri_reduced")
    return dict(p0=dict(zip(names, map(float, p0))), bounds={n: (float(a), float(b)) for n, a, b in zip(names, lo, hi)})


def _solver(**kw):
    return HipBayesGridSolver(TriExpModel(), **{**_tri(), **kw})


def test_solver_potential_options():
    g = {"f1": [0.1, 0.2, 0.3], "D1": [0.01, 0.02]}
    names = list(TriExpModel().param_names)
    four = {"strength": {n: 4.0 for n in names}, "n_sweeps": 4, "tol": 0.0, "connectivity": 6}
    s = _solver(grid=g, spatial_prior={"strength": 4})  # without the new keys: the same four-key dict, the Gaussian path
    assert s.spatial_prior == four and s.spatial_potential == "gaussian" and s.spatial_dof is None
    s = _solver(grid=g, spatial_prior={"strength": 4, "potential": "gaussian"})
    assert s.spatial_prior == four and s.spatial_potential == "gaussian" and s.spatial_dof is None
    given = {"strength": 4, "potential": "student_t", "dof": 4}
    s = _solver(grid=g, spatial_prior=given)
    assert s.spatial_prior == four and s.spatial_potential == "student_t" and s.spatial_dof == 4.0 and s.needs_neighbours
    assert given == {"strength": 4, "potential": "student_t", "dof": 4}  # the caller's dict is not changed
    assert _solver(grid=g).spatial_potential == "gaussian" and _solver(grid=g).spatial_dof is None
    for bad in (None, 0, -1.0, np.nan, np.inf, "4", True):
        with pytest.raises(ValueError, match="potential 'student_t' needs a finite dof > 0"):
            _solver(grid=g, spatial_prior={"strength": 4, "potential": "student_t", "dof": bad})
    with pytest.raises(ValueError, match="potential 'student_t' needs a finite dof > 0"):
        _solver(grid=g, spatial_prior={"strength": 4, "potential": "student_t"})
    with pytest.raises(ValueError, match="dof=4.0 is given with potential 'gaussian'"):
        _solver(grid=g, spatial_prior={"strength": 4, "dof": 4.0})
    with pytest.raises(ValueError, match="potential must be 'gaussian' or 'student_t', got 'huber'"):
        _solver(grid=g, spatial_prior={"strength": 4, "potential": "huber"})
    with pytest.raises(ValueError, match=r"unknown keys \['nu'\]"):
        _solver(grid=g, spatial_prior={"strength": 4, "potential": "student_t", "dof": 4, "nu": 1})
    with pytest.raises(ValueError, match="needs a strength"):
        _solver(grid=g, spatial_prior={"potential": "student_t", "dof": 4})
    t = {"strength": 1, "potential": "student_t", "dof": 4}
    for kw in ({"empirical_prior": {"per_label": True}}, {"log_prior": np.zeros((2, 6))}):
        with pytest.raises(ValueError, match="spatial_prior is not built with per-label priors"):
            _solver(grid=g, spatial_prior=t, **kw)
    with pytest.raises(ValueError, match="spatial_prior is not built with marginals"):
        _solver(grid=g, spatial_prior=t, marginals=True)
    doc = HipBayesGridSolver.__doc__
    assert "student_t" in doc and "spatial_edge_weight" in doc and "dof" in doc


def test_varpro_solver_still_refuses_the_keys():
    rates = {"D1": list(np.geomspace(0.01, 0.2, 5)), "D2": list(np.geomspace(3e-4, 5e-3, 5))}
    bounds = {"f1": (0.0, 1.0), "D1": (1e-5, 0.5), "D2": (1e-5, 0.5), "S0": (0.0, 10.0)}
    assert HipBayesVarProSolver(BiExpModel(fit_s0=True), rates, bounds=bounds, spatial_prior={"strength": 4}).needs_neighbours
    with pytest.raises(ValueError, match=r"unknown keys \['potential'\]"):
        HipBayesVarProSolver(BiExpModel(fit_s0=True), rates, bounds=bounds, spatial_prior={"strength": 4, "potential": "student_t"})
    with pytest.raises(ValueError, match=r"unknown keys \['dof'\]"):
        HipBayesVarProSolver(BiExpModel(fit_s0=True), rates, bounds=bounds, spatial_prior={"strength": 4, "dof": 4})


def test_no_cpu_fallback_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is visible here")
    b, y, _ = synth.make_numpy("tri_reduced", 4, 32)
    nb, col = api.grid_neighbours(np.ones((2, 2), bool), 4)
    with pytest.raises(_lib.PnxError):
        _solver(grid={"f1": [0.1, 0.2]}, spatial_prior={"strength": 4, "potential": "student_t", "dof": 4}).fit(b, y, neighbours=nb, colours=col)


# ---- the ABI without a device
def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnx.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    for name, n_args in ((GATHER, 19), (FIELD, 27), (DRIVER, 33)):
        assert re.search(r"PNX_API\s+int\s+" + name + r"\s*\(", text) and name in _lib.ABI_SYMBOLS and name in exported
        fn = getattr(_lib.load(), name)
        assert len(fn.argtypes) == n_args and fn.restype is C.c_int
    for name in ("grid_neighbour_wfield", "grid_posterior_wfield", "grid_posterior_tmrf"):
        assert callable(getattr(api, name))


def _driver_call(dof=4.0, sd=True, n_nb=4, n_sweeps=2, precision=(1.0, 0, 0, 0), n_vox=6, start=(0, 3, 6)):
    o = api.make_opts("bi_s0", 16)
    n = o.n_free
    atoms, lo, hi, b, y = np.full((n, 4), 0.5), np.zeros(n), np.ones(n), np.zeros(16), np.ones((max(n_vox, 1), 16))
    table = np.full((max(n_vox, 1), max(min(n_nb, 8), 1)), -1, np.int32)
    cs, pr = np.asarray(start, np.int64), np.asarray(precision, float)
    res = dict(mean=np.full((n, max(n_vox, 1)), 9.0), sd=np.full((n, max(n_vox, 1)), 9.0), w=np.full(max(n_vox, 1), 9.0),
               delta=np.full(max(min(n_sweeps, 100), 1), 9.0), done=C.c_int(-7))
    rc = _lib.load().pnx_curvefit_grid_posterior_tmrf_f64(C.byref(o), n_vox, _lib.ptr(b), _lib.ptr(y), 4, _lib.ptr(atoms), None, _lib.ptr(lo),
                                                          _lib.ptr(hi), 0, None, 0.0, n_nb, _lib.ptr(table), 2, _lib.ptr(cs), _lib.ptr(pr), dof,
                                                          n_sweeps, 0.0, _lib.ptr(res["mean"]), _lib.ptr(res["sd"]) if sd else None, None, None,
                                                          None, None, _lib.ptr(res["w"]), None, _lib.ptr(res["delta"]), C.byref(res["done"]), 0,
                                                          0, None)
    return rc, res


def test_driver_refusals_need_no_device():
    err = _lib.last_error
    for bad in (0.0, -1.0, np.nan, np.inf):
        rc, res = _driver_call(dof=bad)
        assert rc == -1 and "dof" in err() and "finite and > 0" in err()
        assert (res["mean"] == 9.0).all() and (res["w"] == 9.0).all() and (res["delta"] == 9.0).all() and res["done"].value == -7
    assert _driver_call(sd=False)[0] == -1 and "sd is NULL" in err()
    assert _driver_call(n_nb=9)[0] == -1 and "n_nb" in err()  # and everything the Gaussian driver refuses
    assert _driver_call(n_sweeps=101)[0] == -1 and "n_sweeps" in err()
    assert _driver_call(start=(0, 3, 5))[0] == -1 and "from 0 to n_vox" in err()
    assert _driver_call(precision=(0, -1.0, 0, 0))[0] == -1 and "precision[1]" in err()
    rc, res = _driver_call(n_vox=0, start=(0, 0, 0))
    assert rc == 0 and res["done"].value == 0 and np.isnan(res["delta"][:2]).all()
    if _lib.device_count() == 0:  # a valid call stops at the device
        assert _driver_call()[0] == -3


def test_field_and_gather_refusals_need_no_device():
    err = _lib.last_error
    lib = _lib.load()
    o = api.make_opts("bi_reduced", 16)
    n = o.n_free
    atoms, lo, hi, b, y = np.full((n, 4), 0.5), np.zeros(n), np.ones(n), np.zeros(16), np.ones((6, 16))
    q, w, fn, mean, sd, pr = np.zeros((n, 6)), np.zeros(6), np.zeros(6, np.int32), np.zeros((n, 6)), np.zeros((n, 6)), np.zeros(n)

    def field(first=0, count=6, mem=1, field_w=w):
        return lib.pnx_curvefit_grid_posterior_wfield_f64(C.byref(o), 6, _lib.ptr(b), _lib.ptr(y), 4, _lib.ptr(atoms), None, _lib.ptr(lo),
                                                          _lib.ptr(hi), 0, None, 0.0, first, count, _lib.ptr(q), _lib.ptr(field_w), _lib.ptr(pr),
                                                          _lib.ptr(mean), None, None, None, None, None, None, mem, 0, None)

    assert field(mem=0) == -1 and "PNX_MEM_DEVICE" in err()
    assert field(5, 2) == -1 and "range" in err()
    assert field(field_w=None) == -1 and "field_w is NULL" in err()
    nb, centre = np.full((6, 4), -1, np.int32), np.zeros(n)

    def gather(dof=4.0, sd=sd, field_w=w, n_nb=4, count=6):
        return lib.pnx_curvefit_grid_neighbour_wfield_f64(6, 0, count, n, n_nb, _lib.ptr(nb), _lib.ptr(mean), _lib.ptr(sd), _lib.ptr(centre),
                                                          _lib.ptr(pr), dof, _lib.ptr(q), _lib.ptr(field_w), _lib.ptr(fn), None, None, 0, 0, None)

    for bad in (0.0, -2.0, np.nan, np.inf):
        assert gather(dof=bad) == -1 and "dof" in err()
    assert gather(sd=None) == -1 and "sd and field_w" in err()
    assert gather(field_w=None) == -1 and "sd and field_w" in err()
    assert gather(n_nb=9) == -1 and "n_nb" in err()
    assert gather(count=0) == 0  # an empty range is no work
    if _lib.device_count() == 0:
        assert gather() == -3 and field() == -3


# ---- the host-side checks under the sanitizers, as a stand-alone program
@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("stub") / "grid_tmrf_args_stub")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "pyneapple_amd", "csrc"), os.path.join(ROOT, "tests", "host_stub", "grid_tmrf_args_stub.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode and any(s in b.stderr for s in ("cannot find -lasan", "cannot find -lubsan")):
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-4000:]
    return exe


def test_argument_checks_are_clean_under_sanitizers(stub):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    r = subprocess.run([stub], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-6000:]
    assert r.returncode == 0 and "grid tmrf args stub ok" in r.stdout, out[-4000:]

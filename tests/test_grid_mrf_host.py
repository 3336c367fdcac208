"""The neighbourhood (MRF) prior of the grid posterior (pnx_curvefit_grid_neighbour_field_f64, pnx_curvefit_grid_posterior_field_f64,
pnx_curvefit_grid_posterior_mrf_f64, api.grid_neighbours / grid_neighbour_field / grid_posterior_field / grid_posterior_mrf,
HipBayesGridSolver's spatial_prior), the parts that need no GPU: the host-side checks, r_g, ranges, report and slab sizing under
AddressSanitizer / UBSan (a stand-alone program, tests/host_stub/grid_mrf_args_stub.cpp), the ABI's refusals in front of any device
work, api.grid_neighbours worked by hand, the solver's option parsing, the colour sort and its way back, the fitter's hand-over,
and the numpy reference: its free energy never decreases, and strength 0 is the plain posterior."""
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
from grid_posterior_reference import reference as posterior_reference

from pyneapple_amd import _lib, api, synth
from pyneapple_amd.fitters import HipPixelWiseFitter
from pyneapple_amd.models import TriExpModel
from pyneapple_amd.solvers import HipBayesGridSolver

GATHER, FIELD, MRF = ("pnx_curvefit_grid_neighbour_field_f64", "pnx_curvefit_grid_posterior_field_f64", "pnx_curvefit_grid_posterior_mrf_f64")


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("stub") / "grid_mrf_args_stub")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "pyneapple_amd", "csrc"), os.path.join(ROOT, "tests", "host_stub", "grid_mrf_args_stub.cpp"), "-o", exe]
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
    """Every refusal of the three calls by its message, r_g, the ranges and centres, the delta scales, the report, and the slab inside
    64 KB for every n_b 1..128 x n_free 1..8."""
    assert "grid mrf args stub ok" in _run_stub(stub)


@pytest.mark.parametrize("n_b", [1, 32, 33, 128])
def test_slab_python_agrees(stub, n_b):
    kpad = (n_b + 3) & ~3
    for n_free in (1, 3, 6, 8):
        w = api.grid_mrf_slab_atoms(n_b, n_free)
        assert int(_run_stub(stub, n_b, n_free)) == w
        assert w >= 16 and w % 16 == 0 and (kpad * (w if w & 16 else w + 16) + (4 + n_free) * w + 8) * 8 <= 64 * 1024
        assert w <= api.grid_posterior_slab_atoms(n_b, n_free)


# ---- the ABI without a device
def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnx.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    for name, n_args in ((GATHER, 15), (FIELD, 27), (MRF, 30)):
        assert re.search(r"PNX_API\s+int\s+" + name + r"\s*\(", text) and name in _lib.ABI_SYMBOLS and name in exported
        fn = getattr(_lib.load(), name)
        assert len(fn.argtypes) == n_args and fn.restype is C.c_int
    for name in ("grid_neighbours", "grid_neighbour_field", "grid_posterior_field", "grid_posterior_mrf", "grid_mrf_centre"):
        assert callable(getattr(api, name))
    header = open(os.path.join(ROOT, "include", "pnx.h")).read()
    assert "LOCAL NORMALISER" in header and "not a model evidence" in header


def _mrf_call(o=None, n_vox=6, n_atoms=4, n_nb=4, n_colours=2, start=(0, 3, 6), precision=None, n_sweeps=2, tol=0.0, project=0, out=True,
              noise_sd=0.0, nb=True, mem=0):
    o = o or api.make_opts("bi_s0", 16)
    n = o.n_free
    atoms = np.full((n, max(n_atoms, 1)), 0.5)
    lo, hi = np.zeros(n), np.ones(n)
    b, y = np.zeros(16), np.ones((max(n_vox, 1), 16))
    table = np.full((max(n_vox, 1), max(min(n_nb, 8), 1)), -1, np.int32)
    cs = None if start is None else np.asarray(start, np.int64)
    pr = np.zeros(n) if precision is None else np.asarray(precision, float)
    res = dict(mean=np.full((n, max(n_vox, 1)), 9.0), delta=np.full(max(min(n_sweeps, 100), 1), 9.0), done=C.c_int(-7))
    rc = _lib.load().pnx_curvefit_grid_posterior_mrf_f64(C.byref(o), n_vox, _lib.ptr(b), _lib.ptr(y), n_atoms, _lib.ptr(atoms), None, _lib.ptr(lo),
                                                         _lib.ptr(hi), project, None, noise_sd, n_nb, _lib.ptr(table) if nb else None, n_colours,
                                                         _lib.ptr(cs), _lib.ptr(pr) if precision is not False else None, n_sweeps, tol,
                                                         _lib.ptr(res["mean"]) if out else None, None, None, None, None, None,
                                                         _lib.ptr(res["delta"]), C.byref(res["done"]), mem, 0, None)
    return rc, res


def test_driver_refusals_need_no_device():
    err = _lib.last_error
    assert _mrf_call(noise_sd=-1.0)[0] == -1 and "noise_sd" in err()  # the posterior's own, first
    assert _mrf_call(n_atoms=0)[0] == -1 and "n_atoms" in err()
    assert _mrf_call(out=False)[0] == -1 and "mean" in err()
    assert _mrf_call(api.make_opts("bi_s0", 16, per_voxel=True))[0] == -2 and "per_voxel_p0_bounds" in err()
    for bad in (0, 9):
        assert _mrf_call(n_nb=bad)[0] == -1 and "n_nb" in err() and "[1,8]" in err()
        assert _mrf_call(n_colours=bad)[0] == -1 and "n_colours" in err() and "[1,8]" in err()
    for bad in (-1, 101):
        assert _mrf_call(n_sweeps=bad)[0] == -1 and "n_sweeps" in err() and "[0,100]" in err()
    for bad in (-1.0, np.nan, np.inf):
        assert _mrf_call(tol=bad)[0] == -1 and "tol" in err()
    assert _mrf_call(nb=False)[0] == -1 and "neighbours is NULL" in err()
    assert _mrf_call(start=None)[0] == -1 and "colour_start is NULL" in err()
    for bad in ((1, 3, 6), (0, 3, 5), (0, 3, 7)):
        assert _mrf_call(start=bad)[0] == -1 and "from 0 to n_vox" in err()
    assert _mrf_call(n_colours=3, start=(0, 4, 3, 6))[0] == -1 and "not ascending at colour 1" in err()
    assert _mrf_call(precision=False)[0] == -1 and "precision is NULL" in err()
    for bad in (-1.0, np.nan, np.inf):
        assert _mrf_call(precision=[0, bad, 0, 0])[0] == -1 and "precision[1]" in err()
    assert _mrf_call(precision=[0, 0, 0, 1.0], project=1)[0] == -1 and "projected S0" in err()
    rc, res = _mrf_call(n_nb=9)  # a refused call writes nothing
    assert rc == -1 and (res["mean"] == 9.0).all() and (res["delta"] == 9.0).all() and res["done"].value == -7
    rc, res = _mrf_call(n_vox=0, start=(0, 0, 0))  # no voxels: nothing to do, every delta NaN
    assert rc == 0 and res["done"].value == 0 and np.isnan(res["delta"][:2]).all()
    if _lib.device_count() == 0:  # valid calls stop at the device
        assert _mrf_call(precision=[1.0, 0, 0, 0])[0] == -3
        assert _mrf_call(n_colours=3, start=(0, 3, 3, 6), n_sweeps=0)[0] == -3


def test_field_and_gather_refusals_need_no_device():
    err = _lib.last_error
    lib = _lib.load()
    o = api.make_opts("bi_reduced", 16)
    n = o.n_free
    atoms, lo, hi, b, y = np.full((n, 4), 0.5), np.zeros(n), np.ones(n), np.zeros(16), np.ones((6, 16))
    q, fn, mean, pr = np.zeros((n, 6)), np.zeros(6, np.int32), np.zeros((n, 6)), np.zeros(n)

    def field(first=0, count=6, mem=1, precision=pr, out=mean):
        return lib.pnx_curvefit_grid_posterior_field_f64(C.byref(o), 6, _lib.ptr(b), _lib.ptr(y), 4, _lib.ptr(atoms), None, _lib.ptr(lo),
                                                         _lib.ptr(hi), 0, None, 0.0, first, count, _lib.ptr(q), _lib.ptr(fn), _lib.ptr(precision),
                                                         _lib.ptr(out), None, None, None, None, None, None, mem, 0, None)

    assert field(mem=0) == -1 and "PNX_MEM_DEVICE" in err()
    assert field(out=None) == -1 and "mean" in err()
    for first, count in ((-1, 2), (0, 7), (5, 2), (7, 0), (0, -1)):
        assert field(first, count) == -1 and "range" in err()
    assert field(precision=np.array([0.0, -1.0, 0.0])) == -1 and "precision[1]" in err()
    assert field(precision=None) == -1 and "precision is NULL" in err()
    nb, centre = np.full((6, 4), -1, np.int32), np.zeros(n)

    def gather(n_vox=6, first=0, count=6, n_free=n, n_nb=4, centre=centre, precision=pr):
        return lib.pnx_curvefit_grid_neighbour_field_f64(n_vox, first, count, n_free, n_nb, _lib.ptr(nb), _lib.ptr(mean), _lib.ptr(centre),
                                                         _lib.ptr(precision), _lib.ptr(q), _lib.ptr(fn), None, 0, 0, None)

    for bad in (0, 9):
        assert gather(n_free=bad) == -1 and "n_free" in err()
        assert gather(n_nb=bad) == -1 and "n_nb" in err()
    assert gather(first=4, count=3) == -1 and "range" in err()
    assert gather(n_vox=2 ** 31) == -1 and "n_vox" in err()
    assert gather(precision=np.array([0.0, np.nan, 0.0])) == -1 and "precision[1]" in err()
    assert gather(centre=np.array([0.0, 0.0, np.inf])) == -1 and "centre[2]" in err()
    assert gather(count=0) == 0  # an empty range is no work
    if _lib.device_count() == 0:
        assert gather() == -3 and field() == -3


# ---- api.grid_neighbours, worked by hand
def test_grid_neighbours_on_a_3x3x2_mask_with_a_hole():
    mask = np.ones((3, 3, 2), bool)
    mask[1, 1, 0] = False  # the hole
    mask[2, 2, 1] = False
    n = int(mask.sum())
    idx = -np.ones(mask.shape, int)
    idx[mask] = np.arange(n)
    for conn, n_nb, n_col in ((4, 4, 2), (8, 8, 4), (6, 6, 2)):
        nb, col = api.grid_neighbours(mask, conn)
        assert nb.shape == (n, n_nb) and nb.dtype == np.int32 and col.shape == (n,) and col.dtype == np.int32
        assert ((nb >= -1) & (nb < n)).all() and set(col.tolist()) <= set(range(n_col))
        edges = {(v, int(u)) for v in range(n) for u in nb[v] if u >= 0}
        assert all((u, v) in edges for v, u in edges), "the table is not symmetric"
        assert all(col[v] != col[u] for v, u in edges), "an edge inside a colour"
        assert all(len({int(u) for u in nb[v] if u >= 0}) == (nb[v] >= 0).sum() for v in range(n))
    nb4, col4 = api.grid_neighbours(mask, 4)
    c = idx[0, 0, 0]  # a corner of slice 0: +x and +y only, slots (-x, +x, -y, +y); no neighbour across slices
    assert nb4[c].tolist() == [-1, idx[1, 0, 0], -1, idx[0, 1, 0]] and col4[c] == 0
    e = idx[1, 0, 0]  # beside the hole: +y is absent
    assert nb4[e].tolist() == [idx[0, 0, 0], idx[2, 0, 0], -1, -1] and col4[e] == 1
    nb6, col6 = api.grid_neighbours(mask, 6)
    m = idx[1, 1, 1]  # above the hole: -z is absent
    assert nb6[m].tolist() == [idx[0, 1, 1], idx[2, 1, 1], idx[1, 0, 1], idx[1, 2, 1], -1, -1] and col6[m] == 1
    assert nb6[c].tolist() == [-1, idx[1, 0, 0], -1, idx[0, 1, 0], -1, idx[0, 0, 1]]
    nb8, col8 = api.grid_neighbours(mask, 8)
    assert nb8[c].tolist() == [-1, idx[1, 0, 0], -1, idx[0, 1, 0], -1, -1, -1, -1]  # the diagonal (1, 1, 0) is the hole
    assert nb8[idx[0, 0, 1]].tolist()[4:] == [-1, -1, -1, idx[1, 1, 1]] and col8[idx[1, 1, 1]] == 3
    nb2, col2 = api.grid_neighbours(mask[:, :, 1], 4)  # a 2-D mask is one slice
    assert nb2.shape == (8, 4) and col2.tolist() == [(i + j) & 1 for i in range(3) for j in range(3) if (i, j) != (2, 2)]
    with pytest.raises(ValueError, match="connectivity must be 4, 8"):
        api.grid_neighbours(mask, 5)
    with pytest.raises(ValueError, match="2-D or 3-D"):
        api.grid_neighbours(np.ones(4, bool), 4)


# ---- the solver
def _tri():
    names, p0, lo, hi = synth.shared_arrays("tri_reduced")
    return dict(p0=dict(zip(names, map(float, p0))), bounds={n: (float(a), float(b)) for n, a, b in zip(names, lo, hi)})


def _solver(**kw):
    return HipBayesGridSolver(TriExpModel(), **{**_tri(), **kw})


def test_solver_spatial_prior_options():
    g = {"f1": [0.1, 0.2, 0.3], "D1": [0.01, 0.02]}
    names = list(TriExpModel().param_names)
    assert _solver(grid=g).spatial_prior is None and not _solver(grid=g).needs_neighbours
    assert _solver(grid=g, spatial_prior=False).spatial_prior is None
    s = _solver(grid=g, spatial_prior={"strength": 4})
    assert s.needs_neighbours and s.spatial_prior == {"strength": {n: 4.0 for n in names}, "n_sweeps": 4, "tol": 0.0, "connectivity": 6}
    s = _solver(grid=g, spatial_prior={"strength": {"f1": 8.0}, "n_sweeps": 2, "tol": 1e-3, "connectivity": 4})
    assert s.spatial_prior["strength"] == {n: (8.0 if n == "f1" else 0.0) for n in names} and s.spatial_prior["connectivity"] == 4
    pr = s.spatial_precision()
    assert pr[names.index("f1")] == 8.0 / (0.3 - 0.1) ** 2 and (np.delete(pr, names.index("f1")) == 0).all()
    pr = _solver(grid=g, spatial_prior={"strength": 1.0}).spatial_precision()
    assert pr[names.index("D1")] == 1.0 / (0.02 - 0.01) ** 2 and pr[names.index("D2")] == 0.0  # a one-value axis has no precision
    lp = np.zeros(6)
    lp[4:] = -np.inf  # f1 = 0.3 excluded: the range shrinks to the admitted atoms
    assert _solver(grid=g, spatial_prior={"strength": 1.0}).spatial_precision(lp)[names.index("f1")] == pytest.approx(1.0 / 0.1 ** 2, rel=1e-12)
    with pytest.raises(ValueError, match=r"unknown keys \['strenght'\]"):
        _solver(grid=g, spatial_prior={"strenght": 1})
    with pytest.raises(ValueError, match="needs a strength"):
        _solver(grid=g, spatial_prior={"n_sweeps": 2})
    for bad in (-1.0, np.nan, "4", True):
        with pytest.raises(ValueError, match="strength of .* must be finite and >= 0"):
            _solver(grid=g, spatial_prior={"strength": bad})
    with pytest.raises(ValueError, match=r"unknown parameters \['f9'\]"):
        _solver(grid=g, spatial_prior={"strength": {"f9": 1.0}})
    for bad in (-1, 101, 2.5):
        with pytest.raises(ValueError, match="n_sweeps must be an integer"):
            _solver(grid=g, spatial_prior={"strength": 1, "n_sweeps": bad})
    with pytest.raises(ValueError, match="tol must be finite"):
        _solver(grid=g, spatial_prior={"strength": 1, "tol": -1})
    with pytest.raises(ValueError, match="connectivity must be 4, 8"):
        _solver(grid=g, spatial_prior={"strength": 1, "connectivity": 26})
    with pytest.raises(ValueError, match="must be None or a dict"):
        _solver(grid=g, spatial_prior=True)
    for kw in ({"empirical_prior": {"per_label": True}}, {"log_prior": np.zeros((2, 6))}):
        with pytest.raises(ValueError, match="spatial_prior is not built with per-label priors"):
            _solver(grid=g, spatial_prior={"strength": 1}, **kw)
    with pytest.raises(ValueError, match="spatial_prior is not built with marginals"):
        _solver(grid=g, spatial_prior={"strength": 1}, marginals=True)
    assert _solver(grid=g, spatial_prior={"strength": 1}, empirical_prior=True).empirical_prior  # the single learned table is allowed
    doc = HipBayesGridSolver.__doc__
    assert "spatial_prior" in doc and "spatial_delta" in doc and "over-smooths" in doc


def test_colour_sort_round_trip():
    mask = np.ones((4, 3, 2), bool)
    mask[1, 1, 0] = mask[3, 0, 1] = False
    for conn in (4, 6, 8):
        nb, col = api.grid_neighbours(mask, conn)
        n = nb.shape[0]
        order, snb, start = HipBayesGridSolver.colour_sort(nb, col, n)
        o2, snb2, start2 = R.colour_sort(nb, col)
        assert (order == o2).all() and snb.tobytes() == snb2.tobytes() and (start == start2).all()
        assert snb.dtype == np.int32 and start.dtype == np.int64 and start[0] == 0 and start[-1] == n and (np.diff(start) >= 0).all()
        assert (np.diff(col[order]) >= 0).all()
        for c in range(len(start) - 1):  # no neighbour inside a voxel's own colour range
            rows = snb[start[c]:start[c + 1]]
            assert not ((rows >= start[c]) & (rows < start[c + 1])).any()
        # the edges are the caller's: voxel order[i] is voxel i of the call
        assert all({int(order[u]) for u in snb[i] if u >= 0} == {int(u) for u in nb[order[i]] if u >= 0} for i in range(n))
        back = np.empty(n, np.int64)
        back[order] = np.arange(n)
        vals = np.arange(n) * 10.0
        assert (vals[order][back] == vals).all()  # the way back
    with pytest.raises(ValueError, match="neighbours must be"):
        HipBayesGridSolver.colour_sort(np.zeros((3, 9), np.int32), np.zeros(3, np.int32), 3)
    with pytest.raises(ValueError, match="colours must be 3 integers"):
        HipBayesGridSolver.colour_sort(np.zeros((3, 4), np.int32), np.full(3, 8), 3)
    with pytest.raises(ValueError, match=r"indices in \[-1, 3\)"):
        HipBayesGridSolver.colour_sort(np.full((3, 4), 3, np.int32), np.zeros(3, np.int32), 3)


def test_fit_asks_for_neighbours_and_the_fitter_hands_them_over(monkeypatch):
    b, y, _ = synth.make_numpy("tri_reduced", 8, 32)
    s = _solver(grid={"f1": [0.1, 0.2]}, spatial_prior={"strength": 4, "connectivity": 4})
    with pytest.raises(ValueError, match="neighbours .* and colours .* are required"):
        s.fit(b, y)
    seen = {}

    def fake_fit(xdata, ydata, pixel_fixed_params=None, neighbours=None, colours=None, **kw):
        seen.update(nb=neighbours, col=colours, n=ydata.shape[0])
        raise RuntimeError("stop here")

    monkeypatch.setattr(s, "fit", fake_fit)
    seg = np.array([1, 1, 0, 1, 1, 1, 1, 0]).reshape(2, 2, 2)
    with pytest.raises(RuntimeError, match="stop here"):
        HipPixelWiseFitter(s).fit(b, y.reshape(2, 2, 2, 32), segmentation=seg)
    nb, col = api.grid_neighbours(seg != 0, 4)
    assert seen["n"] == 6 and seen["nb"].tobytes() == nb.tobytes() and seen["col"].tobytes() == col.tobytes()
    with pytest.raises(RuntimeError, match="stop here"):  # without a segmentation every voxel is inside
        HipPixelWiseFitter(s).fit(b, y.reshape(2, 2, 2, 32))
    assert seen["n"] == 8 and seen["nb"].tobytes() == api.grid_neighbours(np.ones((2, 2, 2), bool), 4)[0].tobytes()
    plain = _solver(grid={"f1": [0.1, 0.2]})
    monkeypatch.setattr(plain, "fit", lambda xdata, ydata, pixel_fixed_params=None, **kw: seen.update(kw=kw) or (_ for _ in ()).throw(RuntimeError("plain")))
    with pytest.raises(RuntimeError, match="plain"):
        HipPixelWiseFitter(plain).fit(b, y.reshape(2, 2, 2, 32), segmentation=seg)
    assert seen["kw"] == {}  # every other solver's call is untouched


def test_no_cpu_fallback_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is visible here")
    b, y, _ = synth.make_numpy("tri_reduced", 4, 32)
    nb, col = api.grid_neighbours(np.ones((2, 2), bool), 4)
    with pytest.raises(_lib.PnxError):
        _solver(grid={"f1": [0.1, 0.2]}, spatial_prior={"strength": 4}).fit(b, y, neighbours=nb, colours=col)


# ---- the numpy reference
@pytest.fixture(scope="module")
def small_phantom():
    ph = R.phantom(seed=0, noise=0.05, H=12, W=12)
    order, nb, start = R.colour_sort(ph["nb"], ph["colours"])
    return ph, order, nb, start


@pytest.mark.parametrize("strength", [1.0, 64.0])
def test_reference_free_energy_never_decreases(small_phantom, strength):
    ph, order, nb, start = small_phantom
    lam = strength / (ph["atoms"].max(axis=1) - ph["atoms"].min(axis=1)) ** 2
    _, delta, F = R.mrf("bi_reduced", ph["b"], ph["y"][order], ph["atoms"], ph["lo"], ph["hi"], nb, start, lam, 4, noise_sd=0.05,
                        trace_free_energy=True)
    F = np.array(F)
    assert F.size == 1 + 4 * 2 and len(delta) == 4
    assert (np.diff(F) >= -1e-9 * np.abs(F[1:])).all(), np.diff(F)
    assert F[-1] > F[0] and delta[-1] < delta[0]


def test_reference_at_strength_zero_is_the_plain_posterior(small_phantom):
    ph, order, nb, start = small_phantom
    y = ph["y"][order]
    st, delta, _ = R.mrf("bi_reduced", ph["b"], y, ph["atoms"], ph["lo"], ph["hi"], nb, start, np.zeros(3), 3, noise_sd=0.05)
    ref = posterior_reference("bi_reduced", ph["b"], y, ph["atoms"], ph["lo"], ph["hi"], noise_sd=0.05)
    for key in ("mean", "var", "log_evidence", "ess", "map_atom"):
        assert np.asarray(st[key]).tobytes() == np.asarray(ref[key]).tobytes(), key
    assert delta == [0.0, 0.0, 0.0]


def test_reference_gather_sums_in_slot_order():
    mean = np.array([[1.0, 2.0, np.nan, 4.0], [10.0, 20.0, np.nan, 40.0]])
    nb = np.array([[1, 2, 3], [-1, 0, -1], [0, 1, 3], [7, -5, 0]], np.int32)  # 2 is a non-finite voxel; 7 and -5 are out of range
    q, n = R.gather(nb, mean, np.array([0.5, 5.0]), np.array([2.0, 0.0]))
    assert n.tolist() == [2, 1, 3, 1]
    assert q[0].tolist() == [2.0 * ((2.0 - 0.5) + (4.0 - 0.5)), 2.0 * 0.5, 2.0 * (((1.0 - 0.5) + (2.0 - 0.5)) + (4.0 - 0.5)), 2.0 * 0.5]
    assert (q[1] == 0.0).all()
    q2, n2 = R.gather(nb, mean, np.array([0.5, 5.0]), np.array([2.0, 0.0]), first=1, count=2)
    assert q2.tobytes() == q[:, 1:3].tobytes() and n2.tolist() == [1, 3]

"""The grid posterior under a Rician likelihood on the device (pnx_curvefit_grid_posterior_rician_f64, pnx_log_i0e_f64;
api.grid_posterior_rician / log_i0e; HipBayesGridSolver(noise_model="rician")) against the numpy reference of
tests/grid_rician_reference.py inside that reference's own bounds, on the cases of tests/grid_rician_cases.py."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT
import grid_rician_cases as K
import grid_rician_reference as R

from pyneapple_amd import _lib, api
from pyneapple_amd.models import BiExpModel
from pyneapple_amd.solvers import HipBayesGridSolver

pytestmark = pytest.mark.gpu
U = 2.0 ** -52
KEYS = ("mean", "sd", "map_p", "map_atom", "log_evidence", "ess")


def _call(c, y=None, **over):
    kw = dict(noise_sd=c["noise_sd"], log_prior=c["log_prior"], **c["kw"])
    kw.update(over)
    return api.grid_posterior_rician(c["model"], c["b"], c["y"] if y is None else y, c["atoms"], c["lo"], c["hi"], **kw)


def _same(a, b, cols=slice(None)):
    return all(np.asarray(a[k])[..., cols].tobytes() == np.asarray(b[k])[..., cols].tobytes() for k in KEYS)


# ---- log I0e per element
@pytest.fixture(scope="module")
def host_h(tmp_path_factory):
    """log_i0e of the z list from the host program (g++, no contraction): the same header the kernel compiles."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("bessel")
    exe = str(d / "bessel_stub")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "pyneapple_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_stub", "bessel_stub.cpp"), "-o", exe], check=True, timeout=300)
    z = K.z_list()
    z.tofile(str(d / "z.bin"))
    subprocess.run([exe, str(d / "z.bin"), str(d / "h.bin")], check=True, timeout=60)
    return z, np.fromfile(str(d / "h.bin"))


def test_log_i0e_on_the_device(host_h):
    """Inside E_h of the reference h (SciPy up to 1e3, the asymptotic series in longdouble beyond).  Bytes: the three polynomial
    pieces (z < 8) are chains of explicit fma and one multiplication, so they are asserted EQUAL to the host program's bytes; the last
    piece calls `log`, where the device's and glibc's may differ in the last place -- there the two are asserted within 2 units."""
    z, hh = host_h
    got = api.log_i0e(z)
    ref = R.reference_h(z)
    den = np.maximum(np.abs(ref), 1.0)
    err = np.abs(got - ref) / (U * den)
    print("log_i0e on the device: largest error", err.max(), "units of 2^-52 max(|h|, 1); bound", R.E_H)
    assert np.isfinite(got).all() and got[0] == 0.0 and (got <= 0).all()
    assert err.max() <= R.E_H
    poly = z < 8.0
    assert got[poly].tobytes() == hh[poly].tobytes()
    assert (np.abs(got[~poly] - hh[~poly]) <= 2 * U * den[~poly]).all()
    bad = api.log_i0e(np.array([np.nan, -1.0, -5e-324, -np.inf, 1.0]))
    assert np.isnan(bad[:4]).all() and abs(bad[4] - R.log_i0e(1.0)) <= R.E_H * U


def test_log_i0e_on_device_tensors():
    import torch

    z = np.array([0.0, 0.5, 3.0, 7.0, 1e5])
    zt = torch.from_numpy(z).cuda()
    out = torch.full_like(zt, 9.0)
    api.log_i0e(zt, out=out)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == api.log_i0e(z).tobytes()


# ---- the posterior against the reference
@pytest.fixture(scope="module")
def refs():
    return {}


@pytest.mark.parametrize("name", list(K.CASES))
def test_posterior_inside_the_reference_bounds(name, refs):
    c = K.build(name)
    ref = R.rician_posterior(c["model"], c["b"], c["y"], c["atoms"], c["lo"], c["hi"], c["noise_sd"], log_prior=c["log_prior"], **c["kw"])
    got = _call(c)
    q = R.accept(ref, got, c["atoms"])
    print(name, "largest error / bound:", {k: f"{v:.3g}" for k, v in q.items()})
    if c["log_prior"] is not None:
        assert (c["log_prior"][got["map_atom"]] > -np.inf).all()


# ---- signals at the edges
def test_signals_at_the_edges():
    c = K.build("bi_reduced_15")
    y = np.repeat(c["y"], 3, axis=0)[:32].copy()  # two strips of 16
    sd = c["noise_sd"]
    y[1] = 0.0                       # an all-zero row
    y[2, 2] = 0.0                    # a zero entry beside finite ones
    y[5] = [1e-3 * sd, 1e3 * sd, 0.3, 1e-3 * sd, 1e3 * sd]  # small-z and large-z paths in one sum
    good = _call(c, y=y)
    ref = R.rician_posterior(c["model"], c["b"], y, c["atoms"], c["lo"], c["hi"], sd, max_eps=1e-4)
    R.accept(ref, good, c["atoms"])
    for v in (1, 2):
        assert good["log_evidence"][v] == -np.inf and np.isfinite(good["mean"][:, v]).all() and np.isfinite(good["sd"][:, v]).all()
        assert np.isfinite(good["ess"][v]) and good["map_atom"][v] >= 0
    assert np.isfinite(good["log_evidence"][5])
    for v, bad_value in ((3, np.nan), (7, np.inf), (20, -0.25)):  # each beside finite neighbours in its strip of 16
        yb = y.copy()
        yb[v, 1] = bad_value
        got = _call(c, y=yb)
        assert got["map_atom"][v] == -1
        for k in ("mean", "sd", "map_p"):
            assert np.isnan(got[k][:, v]).all()
        assert np.isnan(got["log_evidence"][v]) and np.isnan(got["ess"][v])
        others = np.array([i for i in range(32) if i != v])
        assert _same(got, good, others), f"a bad voxel ({bad_value}) moved its neighbours"


# ---- bytes
def test_bytes_between_calls_memories_and_beside_the_gaussian_call():
    import torch

    c = K.build("tri_reduced_prior_slab")
    g_args = (c["model"], c["b"], c["y"], c["atoms"], c["lo"], c["hi"])
    gauss_before = api.grid_posterior(*g_args, noise_sd=c["noise_sd"], log_prior=c["log_prior"])
    a, b2 = _call(c), _call(c)
    assert _same(a, b2)
    gauss_after = api.grid_posterior(*g_args, noise_sd=c["noise_sd"], log_prior=c["log_prior"])
    assert _same(gauss_before, gauss_after)
    assert not _same(a, gauss_before)  # and the likelihood is another one
    n, n_vox = c["atoms"].shape[0], len(c["y"])
    o = api.make_opts(c["model"], len(c["b"]), jac="analytic")
    yt = torch.from_numpy(c["y"]).cuda()
    t = dict(mean=torch.full((n, n_vox), 9.0, dtype=torch.float64, device="cuda"), sd=torch.full((n, n_vox), 9.0, dtype=torch.float64, device="cuda"),
             map_p=torch.full((n, n_vox), 9.0, dtype=torch.float64, device="cuda"), map_atom=torch.full((n_vox,), 9, dtype=torch.int32, device="cuda"),
             log_evidence=torch.full((n_vox,), 9.0, dtype=torch.float64, device="cuda"), ess=torch.full((n_vox,), 9.0, dtype=torch.float64, device="cuda"))
    api.grid_posterior_rician_device(o, n_vox, c["b"], yt, c["atoms"], None, c["lo"], c["hi"], c["log_prior"], c["noise_sd"], t["mean"], t["sd"],
                                     t["map_atom"], t["map_p"], t["log_evidence"], t["ess"], 0)
    torch.cuda.synchronize()
    assert _same({k: v.cpu().numpy() for k, v in t.items()}, a)
    # optional outputs: NULL leaves nothing written, the mean is the same bytes
    m2 = torch.full((n, n_vox), 9.0, dtype=torch.float64, device="cuda")
    api.grid_posterior_rician_device(o, n_vox, c["b"], yt, c["atoms"], None, c["lo"], c["hi"], c["log_prior"], c["noise_sd"], m2, None, None, None,
                                     None, None, 0)
    torch.cuda.synchronize()
    assert m2.cpu().numpy().tobytes() == a["mean"].tobytes()
    sentinel = {k: np.full_like(a[k], 9) for k in KEYS}
    lib = _lib.load()
    rc = lib.pnx_curvefit_grid_posterior_rician_f64(C.byref(o), n_vox, _lib.ptr(c["b"]), _lib.ptr(c["y"]), c["atoms"].shape[1], _lib.ptr(c["atoms"]),
                                                    None, _lib.ptr(c["lo"]), _lib.ptr(c["hi"]), _lib.ptr(c["log_prior"]), c["noise_sd"],
                                                    _lib.ptr(sentinel["mean"]), None, None, None, None, None, 0, 0, None)
    assert rc == 0 and sentinel["mean"].tobytes() == a["mean"].tobytes()
    for k in KEYS[1:]:
        assert (sentinel[k] == 9).all(), k


# ---- refusals that leave the device usable
def test_refusals_leave_the_device_usable():
    c = K.build("bi_reduced_15")
    good = _call(c)
    for bad in (0.0, -0.05, np.nan, np.inf):
        with pytest.raises(_lib.PnxError, match="noise_sd"):
            _call(c, noise_sd=bad)
    with pytest.raises(_lib.PnxError, match="sigma is not built") as e:
        _call(c, sigma=np.ones(len(c["b"])))
    assert e.value.args[0].startswith("pnx error -2")
    atoms = c["atoms"].copy()
    atoms[1, 3] = c["hi"][1] * 2
    with pytest.raises(_lib.PnxError, match="atom 3, free parameter 1"):
        api.grid_posterior_rician(c["model"], c["b"], c["y"], atoms, c["lo"], c["hi"], noise_sd=c["noise_sd"])
    # no layout is refused for scratch: all six forms of the kernel are built without it
    assert _same(_call(c), good)


# ---- the solver, end to end
def test_solver_end_to_end_under_the_pixelwise_fitter():
    """The asserted cell of the worth table (test_grid_rician_host.py): noise 0.10, b up to 2500, the slow rate D2.  The 400 voxels as
    a 20 x 20 x 1 image; the segmentation leaves a border row, a border column and three inner pixels out."""
    from grid_posterior_reference import reference as gauss_reference

    from pyneapple_amd.fitters import HipPixelWiseFitter

    sd, b_max = 0.10, 2500.0
    p = K.worth_population(sd, b_max)
    names = ("f1", "D1", "D2")
    bounds = {n: K.WORTH_BOUNDS[n] for n in names}
    grid = {n: list(K.WORTH_GRID[n]) for n in names}
    img = p["y"].reshape(20, 20, 1, 32)
    seg = np.ones((20, 20, 1), int)
    seg[0, :, 0] = 0
    seg[:, 19, 0] = 0
    for x, y in ((3, 4), (10, 10), (17, 2)):
        seg[x, y, 0] = 0
    sel = (seg > 0).reshape(-1)
    px, truth = img[seg > 0], p["truth"][:, sel]
    assert px.shape == (358, 32) and px.tobytes() == np.ascontiguousarray(p["y"][sel]).tobytes()
    ric = HipBayesGridSolver(BiExpModel(), grid, bounds=bounds, noise_sd=sd, noise_model="rician")
    gau = HipBayesGridSolver(BiExpModel(), grid, bounds=bounds, noise_sd=sd)
    assert not ric.needs_labels and not ric.needs_neighbours
    fr = HipPixelWiseFitter(ric).fit(p["b"], img, segmentation=seg)
    fg = HipPixelWiseFitter(gau).fit(p["b"], img, segmentation=seg)
    assert fr.results_ is not None and fg.results_ is not None
    assert ric.diagnostics_["noise_model"] == "rician" and "noise_model" not in gau.diagnostics_ and ric.diagnostics_["n_pixels"] == 358
    assert set(ric.diagnostics_) == {"posterior_sd", "map", "map_atom", "log_evidence", "ess", "n_pixels", "noise_model"}
    assert ric._atoms.tobytes() == p["atoms"].tobytes()
    direct = api.grid_posterior_rician("bi_reduced", p["b"], px, p["atoms"], p["lo"], p["hi"], noise_sd=sd)
    for i, n in enumerate(names):
        assert np.asarray(ric.params_[n]).tobytes() == direct["mean"][i].tobytes()
        assert ric.diagnostics_["posterior_sd"][n].tobytes() == direct["sd"][i].tobytes()
    assert ric.diagnostics_["map_atom"].tobytes() == direct["map_atom"].tobytes()
    assert all(r.success for r in ric.pixel_results_)
    ref = R.rician_posterior("bi_reduced", p["b"], px, p["atoms"], p["lo"], p["hi"], sd)
    R.accept(ref, direct, p["atoms"])
    err = lambda m: np.median(np.abs(m - truth[2]))
    ratio = err(np.asarray(ric.params_["D2"])) / err(np.asarray(gau.params_["D2"]))
    gref = gauss_reference("bi_reduced", p["b"], px, p["atoms"], p["lo"], p["hi"], noise_sd=sd)
    ratio_ref = err(ref["mean"][:, 2]) / err(gref["mean"][:, 2])
    # a median of |error| moves by at most the largest bound on a mean: to first order the ratio a / b moves by (da + ratio db) / b;
    # twice that covers the second order
    slack = 2 * (ref["bound_mean"][:, 2].max() + ratio_ref * gref["bound_mean"][:, 2].max()) / err(gref["mean"][:, 2])
    print("worth of D2 at noise 0.10, b <= 2500, 358 masked pixels: device", ratio, "reference", ratio_ref, "slack", slack)
    assert abs(ratio - ratio_ref) <= slack and ratio <= K.WORTH_ASSERTED_RATIO

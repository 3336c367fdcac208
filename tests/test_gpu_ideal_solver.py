"""HipIDEALFitter honours its solver on the GPU: the constraint f1 + f2 <= 1 of a HipConstrainedCurveFitSolver and the sigma /
absolute_sigma of a HipCurveFitSolver hold at every level of the pyramid, on the device-resident path and on the host path.

Pyramid 4 x 4 -> 8 x 8 -> 16 x 16, two slices (512 voxels at the last level), 16 b-values; signals from the g13 recipe
(tests/ideal_reference.py `volume`: f3 = 0 on even voxels, U(0, 0.05) on odd ones, 2 % noise, seed 11).  Every pyramid is fitted
once per module and shared, read-only."""
from __future__ import annotations

import functools
import types

import numpy as np
import pytest
from conftest import pcov_norm_err

import ideal_reference as R
from pyneapple_amd import synth

pytestmark = pytest.mark.gpu

NAMES, P0, LO, HI = synth.shared_arrays("tri_reduced")
I_F1, I_F2 = NAMES.index("f1"), NAMES.index("f2")
TOLS = {"wide": {n: 0.5 for n in NAMES}, "narrow": {n: 0.01 if n in ("f1", "f2") else 0.5 for n in NAMES}}
SIGMA = np.linspace(0.02, 0.06, R.N_B)  # one standard deviation per b-value, two to six times the noise at b = 0
VOLUMES = {"g13": {}, "interior": dict(f3=(0.3, 0.35), f1=(0.2, 0.4))}  # "interior": f3 >= 0.3 everywhere, f2 in (0.25, 0.5)


@functools.lru_cache(maxsize=None)
def _volume(name):
    b, img = R.volume(**VOLUMES[name])
    img.setflags(write=False)
    return b, img


def _solver(kind):
    from pyneapple_amd.models import TriExpModel
    from pyneapple_amd.solvers import HipConstrainedCurveFitSolver, HipCurveFitSolver

    kw = dict(model=TriExpModel(), max_iter=250, tol=1e-8, p0=dict(zip(NAMES, map(float, P0))),
              bounds={n: (float(a), float(c)) for n, a, c in zip(NAMES, LO, HI)})
    if kind == "constrained":
        return HipConstrainedCurveFitSolver(**kw)
    return HipCurveFitSolver(**kw, **(dict(sigma=SIGMA, absolute_sigma=True) if kind == "sigma" else {}))


@functools.lru_cache(maxsize=None)
def _pyramid(kind, resident, tol="wide", vol="g13"):
    """One fitted pyramid: kind "box" | "constrained" | "sigma", device resident or host path."""
    from pyneapple_amd.ideal import HipIDEALFitter

    b, img = _volume(vol)
    s = _solver(kind)
    f = HipIDEALFitter(s, np.array(R.DIM_STEPS), TOLS[tol], device_resident=resident)
    f.fit(b, img)
    assert [p.shape for p in f.step_params] == [(4, 4, 2, 5), (8, 8, 2, 5), (16, 16, 2, 5)]
    for a in f.step_params:
        a.setflags(write=False)
    return types.SimpleNamespace(step_params=f.step_params, level_stats=list(f.level_stats_), diagnostics=dict(s.diagnostics_),
                                 params={k: np.asarray(v) for k, v in s.params_.items()}, pixel_indices=f.pixel_indices)


def _fsum(pmap):
    return pmap[..., I_F1] + pmap[..., I_F2]


# ---- 1. the kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_px", [1, 63, 64, 65, 257])
def test_projection_kernel_is_the_numpy_statement_bit_for_bit(gpu, n_px):
    """pnx_ideal_bounds_simplex_f64 against tests/ideal_reference.py: the same fp64 operations in the same order and no
    transcendental, so every byte agrees; block edges of the 256-lane launch and a second block (257).  Fraction sums from
    U(0.8, 1.1); the other rows partly outside their bounds (step 1 clips them).  Second set of bounds: fractions in other rows,
    f1 bounded below at 0.45 so that the second clip acts."""
    import torch

    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    rng = np.random.default_rng(1000 + n_px)
    tol = np.array([0.5, 0.2, 0.01, 0.3, 0.4])
    for lo, hi, i1, i2 in ((LO, HI, I_F1, I_F2), (np.array([1e-3, 0.0, 2e-3, 0.45, 1e-5]), np.array([0.1, 0.9, 0.01, 1.0, 2e-3]), 3, 1)):
        pmap = rng.uniform(0.5 * lo, 1.2 * hi, (n_px, 5))
        total = rng.uniform(0.8, 1.1, n_px)
        pmap[:, i1] = total * rng.uniform(0.3, 0.7, n_px)
        pmap[:, i2] = total - pmap[:, i1]
        want = R.ideal_bounds_simplex(pmap, lo, hi, tol, i1, i2)
        plain_np = R.ideal_bounds(pmap, lo, hi, tol)
        over = R.project(pmap, lo, hi, i1, i2)[1]
        m = torch.from_numpy(pmap).to(dev)
        got = [torch.full((5, n_px), np.nan, dtype=torch.float64, device=dev) for _ in range(3)]
        plain = [torch.full((5, n_px), np.nan, dtype=torch.float64, device=dev) for _ in range(3)]
        gpu.ideal_bounds_simplex_device(m, n_px, lo, hi, tol, i1, i2, *got, 0, st)
        gpu.ideal_bounds_device(m, n_px, lo, hi, tol, *plain, 0, st)
        torch.cuda.synchronize(dev)
        for key, g, p, w, wp in zip(("p0", "lower", "upper"), got, plain, want, plain_np):
            g, p = g.cpu().numpy(), p.cpu().numpy()
            assert g.tobytes() == w.tobytes(), (key, n_px, np.flatnonzero((g != w).any(axis=0)))
            assert p.tobytes() == wp.tobytes(), key  # the restatement of the plain kernel is held to it as well
            assert g[:, ~over].tobytes() == p[:, ~over].tobytes(), key
        if n_px >= 63:
            assert over.any() and not over.all()
            g0 = got[0].cpu().numpy()
            assert (g0[i1] + g0[i2] <= 1.0 + 2.0 ** -52)[over & (g0[i1] > lo[i1]) & (g0[i2] > lo[i2])].all()


# ---- 2. the constraint is applied -----------------------------------------------------------------------------------------
def test_constraint_holds_at_every_level(gpu):
    """Guard: the box-only HipCurveFitSolver through the device-resident pyramid leaves 153 of the 512 converged voxels of the
    last level with f1 + f2 > 1 (measured on an MI355X; 2 of 32 and 24 of 128 at the levels before).  With
    HipConstrainedCurveFitSolver every converged voxel of every level is feasible (measured: 2, 24 and 153 face voxels, all
    certified); a face voxel's f2 is written as 1 - f1, so no slack beyond the fp64 sum."""
    box = _pyramid("box", True)
    ok = box.diagnostics["status"] > 0
    viol = ok & (box.params["f1"] + box.params["f2"] > 1.0)
    print(f"\nbox-only pyramid: {int(viol.sum())} of {int(ok.sum())} converged voxels of the last level have f1 + f2 > 1; "
          f"per level in the maps: {[int((_fsum(p) > 1.0).sum()) for p in box.step_params]}")
    assert viol.sum() >= 1
    assert all("n_face" not in s and "feasible_frac" not in s for s in box.level_stats)

    con = _pyramid("constrained", True)
    print(f"constrained pyramid: {[(s['n_pixels'], s['n_face'], s['feasible_frac'], s['converged_frac'], s['n_bad_bounds']) for s in con.level_stats]}")
    assert len(con.level_stats) == 3
    for s, pmap in zip(con.level_stats, con.step_params):
        assert s["feasible_frac"] == 1.0
        # the level's map holds every voxel: at most the voxels that did not converge (sentinel: their start values) may be outside
        n_failed = s["n_pixels"] - int(round(s["converged_frac"] * s["n_pixels"]))
        assert int((_fsum(pmap) > 1.0).sum()) <= n_failed
    assert sum(s["n_face"] for s in con.level_stats) >= 1
    dg = con.diagnostics
    n = dg["n_pixels"]
    assert n == 512 and dg["lambda"].shape == (n,) and dg["lambda"].dtype == np.float64
    assert dg["face"].shape == (n,) and dg["face"].dtype == np.int8
    assert ((dg["face"] != 0) == (dg["lambda"] != 0)).all()          # lambda is 0 off the face, the multiplier (or NaN) on it
    assert int((dg["face"] != 0).sum()) == con.level_stats[-1]["n_face"] >= 1
    good = dg["status"] > 0
    assert (con.params["f1"] + con.params["f2"] <= 1.0)[good].all()
    on = good & (dg["face"] != 0)
    assert (con.params["f2"][on] == 1.0 - con.params["f1"][on]).all() and np.isnan(dg["pcov"][dg["face"] != 0]).all()


# ---- 3. no empty windows --------------------------------------------------------------------------------------------------
def test_narrow_fraction_windows_are_never_empty(gpu):
    """step_tol = 0.01 for both fractions: a window [p (1 - 0.01), p (1 + 0.01)] around an interpolated start with f1 + f2 > 1.0102
    holds no feasible point, the face problem's intersected bounds are empty and the fit ends with status -1.  The projection
    puts the start on the face first, so no voxel of any level ends that way.  Measured on an MI355X with the projection taken
    out (pnx_ideal_bounds_f64 in its place): 0, 1 and 2 voxels of the three levels end with status -1 on this volume; with it,
    none (6 and 33 face voxels at the second and third level)."""
    for resident in (True, False):
        con = _pyramid("constrained", resident, "narrow")
        st = con.diagnostics["status"]
        print(f"\nnarrow windows, device_resident={resident}: status counts of the last level "
              f"{ {int(k): int((st == k).sum()) for k in np.unique(st)} }, levels "
              f"{[(s['n_face'], s['n_bad_bounds'], s['feasible_frac']) for s in con.level_stats]}")
        assert (st != -1).all()
        for s in con.level_stats:  # the device path counts status -1 at every level
            assert s["n_bad_bounds"] == 0 and s["feasible_frac"] == 1.0


# ---- 4. device path = host path -------------------------------------------------------------------------------------------
def _assert_same_pyramid(dev, host, label):
    """The device-vs-host bar of tests/test_ideal.py::test_device_resident_pyramid_equals_host_pyramid."""
    worst = [float(np.max(np.abs(c - a) / np.maximum(np.abs(a), 1e-300))) for a, c in zip(host.step_params, dev.step_params)]
    print(f"\n[{label}] device against host path: largest relative difference per level {['%.2e' % w for w in worst]}, status differs on "
          f"{int((dev.diagnostics['status'] != host.diagnostics['status']).sum())} voxels")
    for a, c in zip(host.step_params, dev.step_params):
        assert a.shape == c.shape
        np.testing.assert_allclose(c, a, rtol=1e-6, atol=1e-12)
    np.testing.assert_array_equal(dev.pixel_indices, host.pixel_indices)
    for k in NAMES:
        np.testing.assert_allclose(dev.params[k], host.params[k], rtol=1e-6)
    np.testing.assert_array_equal(dev.diagnostics["status"], host.diagnostics["status"])
    assert dev.diagnostics["pcov"].shape == host.diagnostics["pcov"].shape


def test_constrained_device_path_equals_host_path(gpu):
    """For the HIP constrained solver the host loop resizes with the device loop's kernel (pnx_resize2d_f64 on host arrays), so
    both loops hand pnx_curvefit_simplex_f64 the same bytes: measured on an MI355X, the maps of all three levels are identical.
    With numpy's resize in the host loop the figures were 0, 4.9e-7 and 1.9e-2 (4 of 512 voxels of the last level beyond the bar):
    the 5e-16 between the two summation orders became 4.9e-7 in the box-only phase of one second-level voxel with D3 on its upper
    bound, and the third level, started from windows 5.8e-7 apart, stopped elsewhere in the flat D3 valley.  The bar is the one
    of tests/test_ideal.py."""
    dev, host = _pyramid("constrained", True), _pyramid("constrained", False)
    _assert_same_pyramid(dev, host, "constrained")
    np.testing.assert_array_equal(dev.diagnostics["face"], host.diagnostics["face"])
    assert (dev.diagnostics["face"] != 0).any()


def test_sigma_device_path_equals_host_path_and_is_in_force(gpu):
    dev, host, unweighted = _pyramid("sigma", True), _pyramid("sigma", False), _pyramid("box", True)
    _assert_same_pyramid(dev, host, "sigma")
    # the weights arrived: beyond the same bar the weighted pyramid is another one
    far = ~np.isclose(dev.step_params[-1], unweighted.step_params[-1], rtol=1e-6, atol=1e-12)
    print(f"sigma against unweighted: {int(far.any(axis=-1).sum())} of 512 voxels differ beyond the bar")
    assert far.any()
    # absolute_sigma=True arrived as well: without it the device path's covariance would carry the factor 2 cost / (n_b - n_params)
    # (curve_fit's reduced chi-square), which is far from 1 here (guard), while the two paths' covariances agree much closer
    pd, ph = dev.diagnostics["pcov"], host.diagnostics["pcov"]
    ok = (dev.diagnostics["status"] > 0) & np.isfinite(pd).all(axis=(1, 2)) & np.isfinite(ph).all(axis=(1, 2))
    s_sq = 2.0 * dev.diagnostics["cost"][ok] / (R.N_B - len(NAMES))
    err = pcov_norm_err(pd[ok], ph[ok])
    print(f"absolute_sigma: {int(ok.sum())} voxels with a finite covariance, median |reduced chi-square - 1| {np.median(np.abs(s_sq - 1)):.3f}, "
          f"device against host covariance (normalised): median {np.median(err):.2e}, max {err.max():.2e}")
    assert ok.sum() >= 256 and np.median(np.abs(s_sq - 1)) > 0.25
    assert np.median(err) < 1e-3


# ---- 5. nothing moved for others ------------------------------------------------------------------------------------------
def test_interior_volume_is_the_plain_solvers_pyramid(gpu):
    """f3 >= 0.3 everywhere: no level has a violator, so the constrained solver's pyramid is the plain solver's byte for byte."""
    box, con = _pyramid("box", True, "wide", "interior"), _pyramid("constrained", True, "wide", "interior")
    assert [s["n_face"] for s in con.level_stats] == [0, 0, 0] and [s["feasible_frac"] for s in con.level_stats] == [1.0, 1.0, 1.0]
    for a, c in zip(box.step_params, con.step_params):
        assert a.tobytes() == c.tobytes()
    for key in ("status", "nfev", "cost", "pcov"):
        assert np.ascontiguousarray(box.diagnostics[key]).tobytes() == np.ascontiguousarray(con.diagnostics[key]).tobytes(), key
    assert (con.diagnostics["face"] == 0).all() and (con.diagnostics["lambda"] == 0).all()


def test_sigma_leaves_the_unweighted_sweep_out(gpu):
    sig, box = _pyramid("sigma", True), _pyramid("box", True)
    assert all("cost_p0_mean" not in s and "not_worse_than_p0_frac" not in s for s in sig.level_stats)
    assert all("cost_p0_mean" in s for s in box.level_stats[1:]) and "cost_p0_mean" not in box.level_stats[0]
    assert all(s["converged_frac"] > 0.9 for s in sig.level_stats)

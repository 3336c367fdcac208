"""The per-voxel fine grid on the device (pnx_curvefit_grid_refine_f64; api.grid_refine; HipBayesGridSolver(refine=...); DESIGN.md
4.1u) against the numpy reference of tests/grid_refine_reference.py inside that reference's own bounds, on the cases of
tests/grid_refine_cases.py."""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np
import pytest
import grid_refine_cases as K
import grid_refine_reference as R
from grid_posterior_reference import reference as coarse_reference

from pyneapple_amd import _lib, api
from pyneapple_amd.models import BiExpModel
from pyneapple_amd.solvers import HipBayesGridSolver

pytestmark = pytest.mark.gpu
KEYS = ("mean", "sd", "map_p", "edge_mass", "ess", "log_norm")


def _call(c, **over):
    a = dict(c)
    a.update(over)
    return api.grid_refine(a["model"], a["b"], a["y"], a["lo"], a["hi"], a["n_points"], a["centre"], a["half_width"], **K.call_kwargs(a))


def _same(a, b, cols=slice(None)):
    return all(np.asarray(a[k])[..., cols].tobytes() == np.asarray(b[k])[..., cols].tobytes() for k in KEYS)


@pytest.mark.parametrize("name", list(K.CASES))
def test_inside_the_reference_bounds(name):
    """Every output of every voxel inside the bounds tests/grid_refine_reference.py derives; the same bytes from a second call."""
    c = K.build(name)
    ref = K.reference_of(c)
    got = _call(c)
    R.accept(ref, got)
    assert _same(got, _call(c))


def test_one_point_everywhere_is_the_clipped_centre():
    c = K.build("bi_reduced_one_point")
    c["centre"][1, 2], c["centre"][2, 4] = 0.5, -1.0  # outside the bounds: clipped
    got = _call(c)
    clipped = np.clip(c["centre"], c["lo"][:, None], c["hi"][:, None])
    assert got["mean"].tobytes() == clipped.tobytes() and got["map_p"].tobytes() == clipped.tobytes()
    assert (got["sd"] == 0).all() and (got["edge_mass"] == 0).all() and (got["ess"] == 1).all() and (got["log_norm"] < 0).all()


def test_boxes_cut_by_bounds_bad_voxels_and_their_neighbours():
    c, info = K.edge_case()
    ref = K.reference_of(c)
    assert sorted(np.flatnonzero(~ref["finite"])) == info["nan"] and ref["n_atoms"][info["single"]] == 25 == ref["n_atoms"][info["zero_width"]]
    assert ref["n_admitted"][info["straddle"]] == 75
    got = _call(c)
    R.accept(ref, got)
    assert got["map_p"][1, info["cut"]] <= c["hi"][1] and got["mean"][1, info["cut"]] <= c["hi"][1]
    assert got["mean"][2, info["single"]] == c["lo"][2] and got["sd"][2, info["single"]] == 0 and got["edge_mass"][2, info["single"]] == 0
    assert got["mean"][0, info["zero_width"]] == c["centre"][0, info["zero_width"]] and got["sd"][0, info["zero_width"]] == 0
    assert got["mean"][0, info["straddle"]] <= 1.0 and got["map_p"][0, info["straddle"]] <= 1.0
    # the neighbours of the bad voxels are untouched: the same bytes as in a launch without the oddities
    clean = K.build("bi_reduced_125")
    clean["y"], clean["centre"], clean["half_width"] = clean["y"][:17], np.ascontiguousarray(clean["centre"][:, :17]), np.ascontiguousarray(clean["half_width"][:, :17])
    clean["hi"] = c["hi"]
    plain = _call(clean)
    untouched = [v for v in range(17) if v not in info["nan"] + [info["cut"], info["single"], info["zero_width"], info["straddle"]]]
    assert _same(got, plain, untouched)


def test_host_and_device_memory_give_the_same_bytes():
    import torch

    c = K.build("bi_reduced_125")
    host = _call(c)
    n, n_vox = c["centre"].shape
    dev = torch.device("cuda", 0)
    up = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev).contiguous()
    y, ce, hw = up(c["y"]), up(c["centre"]), up(c["half_width"])
    out = {k: torch.full((n, n_vox), 7.0, dtype=torch.float64, device=dev) for k in ("mean", "sd", "map_p", "edge_mass")}
    out.update({k: torch.full((n_vox,), 7.0, dtype=torch.float64, device=dev) for k in ("ess", "log_norm")})
    o = api.make_opts(c["model"], len(c["b"]), c["fixed_idx"], jac="analytic")
    api.grid_refine_device(o, n_vox, c["b"], y, c["fixed_vals"], c["lo"], c["hi"], c["project"], c["noise_sd"], c["n_points"], ce, hw,
                           out["mean"], out["sd"], out["map_p"], out["ess"], out["log_norm"], out["edge_mass"], 0)
    torch.cuda.synchronize()
    assert _same(host, {k: v.cpu().numpy() for k, v in out.items()})


def test_a_fine_grid_that_coincides_with_a_coarse_grid():
    """The 27 coarse atoms of one block as the box, a uniform prior, one box for all voxels: the coarse call's mean, sd, ess and
    log_evidence (= L - log 27 = log_norm) within the sum of both references' bounds."""
    axes = K.COINCIDE_AXES
    atoms = np.ascontiguousarray(np.array(list(itertools.product(*axes))).T)
    rng = np.random.default_rng(3)
    truth = np.stack([rng.uniform(ax[0], ax[-1], 40) for ax in axes])
    b = np.linspace(0.0, 800.0, 32)
    y = truth[0][:, None] * np.exp(-b[None] * truth[1][:, None]) + (1 - truth[0])[:, None] * np.exp(-b[None] * truth[2][:, None])
    y = y + rng.normal(0.0, 0.02, y.shape)
    lo, hi = np.zeros(3), np.ones(3)
    centre = np.repeat(np.array([0.5 * (ax[0] + ax[-1]) for ax in axes])[:, None], 40, axis=1)
    half = np.repeat(np.array([0.5 * (ax[-1] - ax[0]) for ax in axes])[:, None], 40, axis=1)
    npts = np.array([3, 3, 3], np.int32)
    for noise_sd in (0.02, 0.0):
        fine = api.grid_refine("bi_reduced", b, y, lo, hi, npts, centre, half, noise_sd=noise_sd)
        coarse = api.grid_posterior("bi_reduced", b, y, atoms, lo, hi, noise_sd=noise_sd)
        rf = R.reference("bi_reduced", b, y, lo, hi, npts, centre, half, noise_sd=noise_sd)
        rc = coarse_reference("bi_reduced", b, y, atoms, lo, hi, noise_sd=noise_sd)
        assert all(rf["atoms"][v].tobytes() == atoms.tobytes() for v in range(40))
        assert (np.abs(fine["mean"] - coarse["mean"]) <= (rf["bound_mean"] + rc["bound_mean"]).T).all()
        assert (np.abs(fine["sd"] ** 2 - coarse["sd"] ** 2) <= (rf["bound_var"] + rc["bound_var"]).T).all()
        assert (np.abs(fine["ess"] - coarse["ess"]) <= rf["bound_ess"] + rc["bound_ess"]).all()
        assert (np.abs(fine["log_norm"] - coarse["log_evidence"]) <= rf["bound_log_norm"] + rc["bound_log_evidence"]).all()
        assert (fine["map_p"] == coarse["map_p"]).mean() > 0.9


def test_refusals_leave_the_device_usable():
    c = K.build("bi_reduced_one_b")
    before = _call(c)
    with pytest.raises(_lib.PnxError, match="sigma is not built"):
        api.grid_refine(c["model"], c["b"], c["y"], c["lo"], c["hi"], c["n_points"], c["centre"], c["half_width"], noise_sd=0.02, sigma=0.1)
    with pytest.raises(_lib.PnxError, match="more than 4096"):
        t = K.build("tri_reduced_3125")
        _call(t, n_points=np.array([9, 9, 9, 9, 1], np.int32))
    with pytest.raises(_lib.PnxError, match=r"n_points\[1\]=10"):
        _call(c, n_points=np.array([2, 10, 1], np.int32))
    assert _same(before, _call(c))


def _worth_ratios(levels_out, truth):
    med = lambda m: np.median(np.abs(m - truth), axis=1)
    return med(levels_out[-1]["mean"]) / med(levels_out[0]["mean"])


@pytest.mark.parametrize("noise", K.WORTH_NOISE)
def test_worth_on_the_device_is_the_references(noise):
    """The device reproduces the reference's ratios of the worth table to 10 digits (both chains start from the numpy coarse
    posterior, so only the fine levels differ)."""
    p = K.worth_population(noise)
    run = lambda model, b, y, lo, hi, npts, centre, hw, noise_sd: api.grid_refine(model, b, y, lo, hi, npts, np.ascontiguousarray(centre),
                                                                                  np.ascontiguousarray(hw), noise_sd=noise_sd)
    for lv in K.WORTH_LEVELS:
        ref = R.refine_levels("bi_reduced", p["b"], p["y"], K.WORTH_LO, K.WORTH_HI, K.WORTH_AXES, noise, points=5, levels=lv)
        dev = R.refine_levels("bi_reduced", p["b"], p["y"], K.WORTH_LO, K.WORTH_HI, K.WORTH_AXES, noise, points=5, levels=lv, run=run)
        rr, rd = _worth_ratios(ref, p["truth"]), _worth_ratios(dev, p["truth"])
        print(f"noise {noise} levels {lv}: refined / coarse (f1, D1, D2) device {rd} reference {rr}")
        np.testing.assert_allclose(rd, rr, rtol=1e-10, atol=0)


def test_solver_through_the_pixelwise_fitter_with_two_levels():
    from pyneapple_amd.fitters import HipPixelWiseFitter

    noise = 0.01
    p = K.worth_population(noise)
    names = ("f1", "D1", "D2")
    grid = {n: list(ax) for n, ax in zip(names, K.WORTH_AXES)}
    bounds = {n: (float(K.WORTH_LO[i]), float(K.WORTH_HI[i])) for i, n in enumerate(names)}
    img = p["y"].reshape(20, 20, 1, 32).copy()
    img[2, 3, 0, 5] = np.nan
    seg = np.ones((20, 20, 1), int)
    seg[0, :, 0] = 0
    px = img[seg > 0]
    truth = p["truth"][:, (seg > 0).reshape(-1)]
    fine = HipBayesGridSolver(BiExpModel(), grid, bounds=bounds, noise_sd=noise, refine={"points": 5, "levels": 2})
    coarse = HipBayesGridSolver(BiExpModel(), grid, bounds=bounds, noise_sd=noise)
    HipPixelWiseFitter(fine).fit(p["b"], img, segmentation=seg)
    HipPixelWiseFitter(coarse).fit(p["b"], img, segmentation=seg)
    d = fine.diagnostics_
    assert d["refine_levels"] == 2 and d["n_pixels"] == 380 and set(d["refine_edge_mass"]) == set(names) and d["refine_ess"].shape == (380,)
    assert d["ess"].tobytes() == coarse.diagnostics_["ess"].tobytes() and d["log_evidence"].tobytes() == coarse.diagnostics_["log_evidence"].tobytes()
    assert d["map_atom"].tobytes() == coarse.diagnostics_["map_atom"].tobytes()
    bad = int(np.flatnonzero(np.isnan(px).any(axis=1))[0])
    ok = np.ones(380, bool)
    ok[bad] = False
    success = [r.success for r in fine.pixel_results_]
    assert not success[bad] and sum(success) == 379
    # the chain by hand: the coarse call, then two api.grid_refine calls with the solver's half-widths
    lo, hi = K.WORTH_LO, K.WORTH_HI
    mean, sd = np.stack([np.asarray(coarse.params_[n]) for n in names]), np.stack([coarse.diagnostics_["posterior_sd"][n] for n in names])
    cell = np.stack([HipBayesGridSolver.coarse_cell(ax, mean[k]) for k, ax in enumerate(K.WORTH_AXES)])
    npts = np.array([5, 5, 5], np.int32)
    for _ in range(2):
        half = np.maximum(1.0 * cell, 2.0 * sd)
        res = api.grid_refine("bi_reduced", p["b"], px, lo, hi, npts, np.ascontiguousarray(mean), half, noise_sd=noise)
        cell = (np.minimum(hi[:, None], mean + half) - np.maximum(lo[:, None], mean - half)) / 4
        mean, sd = res["mean"], res["sd"]
    for i, n in enumerate(names):
        assert np.asarray(fine.params_[n]).tobytes() == mean[i].tobytes() and d["posterior_sd"][n].tobytes() == sd[i].tobytes()
        assert d["map"][n].tobytes() == res["map_p"][i].tobytes() and d["refine_edge_mass"][n].tobytes() == res["edge_mass"][i].tobytes()
        assert np.isnan(np.asarray(fine.params_[n])[bad])
    err = lambda s, k: np.median(np.abs(np.asarray(s.params_[names[k]])[ok] - truth[k][ok]))
    for k in range(3):  # the worth at 1 % noise, two levels: every parameter gains (reference: 0.21, 0.45, 0.20)
        ratio = err(fine, k) / err(coarse, k)
        print(names[k], "refined / coarse on the masked image:", ratio)
        assert ratio <= K.WORTH_MEASURED[(0.01, 2)][k] + 0.1


def test_a_cost_that_overflows_weighs_nothing_and_poisons_nothing():
    """A finite but enormous signal under known noise: every cost is +inf, every l is -inf.  The voxel reports equal weights (pnx.h),
    not NaN, and its neighbours keep their bytes."""
    c = K.build("bi_reduced_one_b")
    plain = _call(c)
    c["y"] = c["y"].copy()
    c["y"][3] = 1e200
    got = _call(c)
    others = [v for v in range(17) if v != 3]
    assert _same(got, plain, others)
    assert got["log_norm"][3] == -np.inf and got["ess"][3] == 6.0
    ref = K.reference_of(K.build("bi_reduced_one_b"))
    atoms = ref["atoms"][3]
    np.testing.assert_allclose(got["mean"][:, 3], atoms.mean(axis=1), rtol=1e-14)
    np.testing.assert_allclose(got["sd"][:, 3], atoms.std(axis=1), rtol=1e-12, atol=1e-18)
    assert got["map_p"][:, 3].tobytes() == np.ascontiguousarray(atoms[:, 0]).tobytes()
    np.testing.assert_allclose(got["edge_mass"][:, 3], [1.0, 2.0 / 3.0, 0.0], rtol=1e-14)

"""pnx_curvefit_grid_posterior_f64 on the device against tests/grid_posterior_reference.py: tile edges along every axis, all
layouts, projection, weights / fixed parameters / T1, both noise modes, priors, the online log-sum-exp at its extremes, the exact
cases, invariances, non-finite signals, host against device memory, and HipBayesGridSolver end to end.

Acceptance per voxel (grid_posterior_reference.accept, derivation in DESIGN.md 4.1g): the library's l_g differs from the
reference's by at most eps_v (the cancellation bound of the expanded cost, pushed through -c / noise_sd^2 or -(nu / 2) log c, plus
the rounding of l itself), the normalised weights then move by e^{+-2 eps_v}, a weighted sum of G terms adds gamma = 4 (G + 16)
2^-52; mean, sd^2, log_evidence and ess are held to the resulting bounds, the MAP atom to l_ref[map] >= max l_ref - 2 eps_v, map_p
to a bit-for-bit copy.  Oracle-compared cases satisfy eps_v <= 1e-6 on every voxel (asserted by the reference); no voxel is left out.

The largest error-to-bound ratios observed are recorded in DESIGN.md 4.1g."""
from __future__ import annotations

import numpy as np
import pytest
from grid_posterior_reference import accept, reference
from grid_start_reference import reference as grid_reference
from grid_start_reference import s0_row, signals

from pyneapple_amd import api, synth
from pyneapple_amd.fitters import HipPixelWiseFitter
from pyneapple_amd.models import BiExpModel
from pyneapple_amd.solvers import HipBayesGridSolver

pytestmark = pytest.mark.gpu

BOUNDS = {"f1": (0.0, 1.0), "f2": (0.0, 1.0), "f3": (0.0, 1.0), "D": (1e-5, 0.1), "D1": (0.01, 0.5), "D2": (2e-3, 0.01), "D3": (1e-5, 2e-3),
          "S0": (0.5, 2.0), "T1": (500.0, 3000.0)}
TRUTH = {**BOUNDS, "f1": (0.05, 0.4), "f2": (0.05, 0.4), "f3": (0.05, 0.4), "S0": (0.6, 1.8)}
NOISE_SD = 0.05  # the known-noise mode of the cases below: signals of order 1 with 2 % noise, so the posterior spreads over atoms


def _names(model, t1_mode=0, fixed_idx=()):
    names = api.MODEL_PARAM_NAMES[model] + (["T1"] if t1_mode else [])
    return [n for i, n in enumerate(names) if i not in fixed_idx]


def _case(model, n_vox, n_atoms, n_b, seed=0, noise=0.02, **kw):
    """(b, y, atoms, lo, hi): atoms uniform inside the bounds, signals of uniform truth values (no atom coincides with one) with
    additive Gaussian noise of sd 0.02 on signals of order 1: min_g c_g ~ n_b noise^2 / 2 stays far above the cancellation floor
    (multiplicative noise would not: a fast mono-exponential decay is zero, noise and all, beyond b = 0)."""
    rng = np.random.default_rng(1000 * seed + 7 * n_vox + 3 * n_atoms + n_b)
    names = _names(model, kw.get("t1_mode", 0), kw.get("fixed_idx", ()))
    lo = np.array([BOUNDS[n][0] for n in names])
    hi = np.array([BOUNDS[n][1] for n in names])
    atoms = np.ascontiguousarray(rng.uniform(lo[:, None], hi[:, None], (len(names), n_atoms)))
    truth = np.stack([rng.uniform(*TRUTH[n], n_vox) for n in names])
    b = synth.bvalues(n_b)
    y = signals(model, b, truth, **{k: v for k, v in kw.items() if k in ("fixed_idx", "fixed_vals", "t1_mode", "tr", "tm")})
    y = np.ascontiguousarray(y + noise * rng.standard_normal(y.shape))
    return b, y, atoms, lo, hi


def _check(gpu, model, b, y, atoms, lo, hi, project=False, noise_sd=0.0, log_prior=None, max_eps=1e-6, **kw):
    got = gpu.grid_posterior(model, b, y, atoms, lo, hi, project_amplitude=project, noise_sd=noise_sd, log_prior=log_prior, **kw)
    ref = reference(model, b, y, atoms, lo, hi, project=project, noise_sd=noise_sd, log_prior=log_prior, max_eps=max_eps, **kw)
    accept(ref, got, atoms)
    return got, ref


def _both_modes(gpu, model, *case, **kw):
    _check(gpu, model, *case, noise_sd=0.0, **kw)
    return _check(gpu, model, *case, noise_sd=NOISE_SD, **kw)


# ---- tile edges: each axis' edge values crossed with one mid value of the others
@pytest.mark.parametrize("n_vox", [1, 15, 16, 17, 33])
def test_voxel_axis(gpu, n_vox):
    _both_modes(gpu, "tri_reduced", *_case("tri_reduced", n_vox, 33, 16))


@pytest.mark.parametrize("n_atoms", [1, 15, 16, 17])
def test_atom_axis(gpu, n_atoms):
    _both_modes(gpu, "tri_reduced", *_case("tri_reduced", 65, n_atoms, 16))


@pytest.mark.parametrize("n_b", [2, 3, 4, 5, 32, 33, 64, 65, 128])  # 33 and up take the larger instantiation
def test_b_axis(gpu, n_b):
    _both_modes(gpu, "tri_reduced", *_case("tri_reduced", 65, 33, n_b))


@pytest.mark.parametrize("delta", [0, 1])
def test_slab_capacity_at_32_b_values(gpu, delta):
    """One slab resident in LDS at exactly the capacity, two slabs reloaded per pass one atom above it; the capacity follows from
    n_free (api.grid_posterior_slab_atoms: 3 + n_free values per atom beside the 32 of its dictionary row)."""
    cap = api.grid_posterior_slab_atoms(32, 5)
    assert cap % 16 == 0 and 16 < cap < 256 and api.grid_posterior_slab_atoms(32, 8) <= cap
    _both_modes(gpu, "tri_reduced", *_case("tri_reduced", 65, cap + delta, 32))


def test_dictionary_at_the_cap(gpu):
    _both_modes(gpu, "bi_reduced", *_case("bi_reduced", 64, 4096, 16))


@pytest.mark.parametrize("n_b,n_atoms", [(8, 17), (128, 49)])
def test_more_voxels_than_one_pass_of_the_grid(gpu, n_b, n_atoms):
    """A block owns 64 voxels per pass and the grid is capped at two blocks per CU: 40 000 voxels send every block round its loop
    again -- with the one-slab dictionary resident in LDS (17 atoms) and with two slabs reloaded (49 atoms at 128 b-values)."""
    assert (n_atoms > api.grid_posterior_slab_atoms(n_b, 3)) == (n_b == 128)
    _check(gpu, "bi_reduced", *_case("bi_reduced", 40000, n_atoms, n_b), noise_sd=NOISE_SD if n_b == 8 else 0.0)


# ---- configurations
@pytest.mark.parametrize("model", sorted(api.MODEL_IDS))
def test_every_layout(gpu, model):
    _both_modes(gpu, model, *_case(model, 65, 33, 16))


@pytest.mark.parametrize("model", api.PROJECT_MODELS)
@pytest.mark.parametrize("project", [False, True])
def test_projection_on_and_off(gpu, model, project):
    """Projected: the S0 row of mean / sd / map_p is the posterior of the clipped amplitude a_g(v), whatever the atoms' S0 row holds;
    voxels whose amplitude clips at either bound are among the cases."""
    b, y, atoms, lo, hi = _case(model, 96, 33, 16)
    y[:16] *= 0.05
    y[80:] *= 100.0
    if project:
        atoms[s0_row(model)] = np.linspace(0.5, 2.0, atoms.shape[1])  # ignored
        got, _ = _check(gpu, model, b, y, atoms, lo, hi, project=True)
        row = s0_row(model)
        assert (got["mean"][row, :16] == 0.5).all() and (got["sd"][row, :16] == 0.0).all()  # every atom clips at lo_S0: exact
        top = got["mean"][row, 80:]  # an atom with f1 + f2 > 1 has a row that changes sign and need not clip at hi_S0
        assert ((top > 1.5) & (top <= 2.0)).all() and (got["sd"][row, 80:][top == 2.0] == 0.0).all()
        mid = got["mean"][row, 16:80]
        assert ((mid > 0.5) & (mid < 2.0)).mean() > 0.5
    # signals 100 times an atom's amplitude make |l| ~ 1e8 with a known noise_sd: outside eps_v <= 1e-6, so both modes run on the rest
    _both_modes(gpu, model, b, y[16:80], atoms, lo, hi, project=project)


def test_sigma(gpu):
    sigma = np.linspace(0.5, 3.0, 16)
    _both_modes(gpu, "tri_reduced", *_case("tri_reduced", 65, 33, 16), sigma=sigma)
    _both_modes(gpu, "tri_s0", *_case("tri_s0", 65, 33, 16), project=True, sigma=sigma)


def test_shared_fixed_parameter(gpu):
    kw = dict(fixed_idx=[1], fixed_vals=np.array([0.07]))  # D1 of [f1, D1, D2, S0]
    case = _case("bi_s0", 65, 33, 16, **kw)
    assert case[2].shape[0] == 3
    _both_modes(gpu, "bi_s0", *case, **kw)
    _both_modes(gpu, "bi_s0", *case, project=True, **kw)


@pytest.mark.parametrize("t1_mode", [1, 2])
def test_t1_factor_on_mono(gpu, t1_mode):
    kw = dict(t1_mode=t1_mode, tr=3000.0, tm=30.0 if t1_mode == 2 else 0.0)
    _both_modes(gpu, "mono", *_case("mono", 65, 33, 16, **kw), project=True, **kw)


@pytest.mark.parametrize("excluded", [0.0, 1 / 3])
def test_log_prior(gpu, excluded):
    b, y, atoms, lo, hi = _case("tri_s0", 65, 100, 16)
    rng = np.random.default_rng(3)
    lp = np.log(rng.uniform(0.01, 1.0, 100)) + 2.5  # not normalised: the library normalises
    lp[rng.random(100) < excluded] = -np.inf
    assert bool(excluded) == bool(np.isinf(lp).any())
    for project in (False, True):
        got, _ = _both_modes(gpu, "tri_s0", b, y, atoms, lo, hi, project=project, log_prior=lp)
        assert np.isfinite(lp[got["map_atom"]]).all()


# ---- the online log-sum-exp
@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_maximum_moves_at_every_tile_or_never(gpu, order):
    """Atoms sorted by their likelihood for voxel 0 (every voxel carries the same truth, own noise): ascending, the running maximum
    moves with every tile and every sum is rescaled each time; descending, never."""
    b, y, atoms, lo, hi = _case("bi_reduced", 33, 200, 16)
    y = np.repeat(y[:1], 33, axis=0) * (1 + 0.005 * np.random.default_rng(4).standard_normal((33, 16)))
    c = grid_reference("bi_reduced", b, y[:1], atoms, lo, hi)["c"][0]
    o = np.argsort(c)[::-1] if order == "ascending" else np.argsort(c)
    got, ref = _both_modes(gpu, "bi_reduced", b, y, np.ascontiguousarray(atoms[:, o]), lo, hi)
    assert got["map_atom"][0] == (199 if order == "ascending" else 0)


def test_a_tiny_noise_sd_puts_the_posterior_on_the_map_atom(gpu):
    """noise_sd = 1e-3 on signals of order 1: l spreads over more than 1e5 and every weight but the MAP atom's underflows.
    Everything is finite; where the reference's own ess is 1 the mean is the MAP atom and ess is 1, each to its bound."""
    b, y, atoms, lo, hi = _case("tri_reduced", 65, 257, 16)
    got, ref = _check(gpu, "tri_reduced", b, y, atoms, lo, hi, noise_sd=1e-3)
    assert (ref["l"].max(axis=1) - ref["l"].min(axis=1)).min() > 1e5
    for key in ("mean", "sd", "map_p", "log_evidence", "ess"):
        assert np.isfinite(got[key]).all()
    sharp = ref["ess"] - 1 < 1e-13
    assert sharp.mean() > 0.9
    assert (np.abs(got["mean"] - got["map_p"])[:, sharp] <= ref["bound_mean"].T[:, sharp]).all()
    assert (np.abs(got["ess"] - 1)[sharp] <= ref["bound_ess"][sharp] + 1e-13).all()
    assert (got["sd"][:, sharp] ** 2 <= ref["bound_var"].T[:, sharp]).all()


def test_a_huge_noise_sd_returns_the_prior(gpu):
    b, y, atoms, lo, hi = _case("tri_reduced", 65, 100, 16)
    lp = np.log(np.random.default_rng(6).uniform(0.05, 1.0, 100))
    got, ref = _check(gpu, "tri_reduced", b, y, atoms, lo, hi, noise_sd=1e9, log_prior=lp)
    prior = np.exp(lp) / np.exp(lp).sum()
    R = atoms.max(axis=1) - atoms.min(axis=1)
    assert (np.abs(got["mean"] - (atoms @ prior)[:, None]) <= ref["bound_mean"].T + 1e-15 * R[:, None]).all()
    assert (np.abs(got["log_evidence"]) <= ref["bound_log_evidence"] + 1e-15).all()  # the evidence of pure prior: log 1
    np.testing.assert_allclose(got["ess"], 1 / (prior ** 2).sum(), rtol=1e-12)


# ---- exact cases
@pytest.mark.parametrize("model,project", [("tri_reduced", False), ("tri_s0", True)])
@pytest.mark.parametrize("noise_sd", [0.0, NOISE_SD])
def test_a_dictionary_of_one_atom(gpu, model, project, noise_sd):
    b, y, atoms, lo, hi = _case(model, 65, 1, 16)
    lp = np.array([-1.25])
    got, ref = _check(gpu, model, b, y, atoms, lo, hi, project=project, noise_sd=noise_sd, log_prior=lp)
    rows = [k for k in range(atoms.shape[0]) if k != ref["s0_row"]]
    assert (got["mean"][rows].view(np.uint64) == np.repeat(atoms[rows], 65, axis=1).view(np.uint64)).all()
    assert got["mean"].tobytes() == got["map_p"].tobytes()  # the projected S0 row too: the one amplitude
    assert (got["sd"] == 0.0).all() and (got["ess"] == 1.0).all() and (got["map_atom"] == 0).all()
    assert (np.abs(got["log_evidence"] - (ref["l"][:, 0] - lp[0])) <= ref["bound_log_evidence"]).all()


def test_a_noise_free_voxel_that_equals_an_atom(gpu):
    """Marginalised mode on the cancellation floor: c_j is rounding noise, the floor makes l_j finite and the largest by far."""
    b, _, atoms, lo, hi = _case("tri_reduced", 8, 40, 16)  # random atoms: well separated
    j = np.array([0, 5, 16, 17, 31, 32, 38, 39])
    y = signals("tri_reduced", b, atoms[:, j])
    got = gpu.grid_posterior("tri_reduced", b, y, atoms, lo, hi)
    for key in ("mean", "sd", "map_p", "log_evidence", "ess"):
        assert np.isfinite(got[key]).all()
    assert (got["map_atom"] == j).all() and (got["ess"] < 1.0 + 1e-6).all()


# ---- invariances (no oracle): each within twice the bound
def _close(a, b, bound):
    assert (np.abs(a - b) <= 2 * bound).all(), float((np.abs(a - b) / bound).max())


@pytest.mark.parametrize("noise_sd", [0.0, NOISE_SD])
def test_permuting_the_atoms_changes_nothing(gpu, noise_sd):
    b, y, atoms, lo, hi = _case("tri_s0", 65, 300, 16)
    rng = np.random.default_rng(8)
    lp = np.log(rng.uniform(0.05, 1.0, 300))
    perm = rng.permutation(300)
    one = gpu.grid_posterior("tri_s0", b, y, atoms, lo, hi, log_prior=lp, noise_sd=noise_sd, project_amplitude=True)
    two = gpu.grid_posterior("tri_s0", b, y, np.ascontiguousarray(atoms[:, perm]), lo, hi, log_prior=lp[perm], noise_sd=noise_sd, project_amplitude=True)
    ref = reference("tri_s0", b, y, atoms, lo, hi, log_prior=lp, noise_sd=noise_sd, project=True)
    _close(one["mean"].T, two["mean"].T, ref["bound_mean"])
    _close(one["sd"].T ** 2, two["sd"].T ** 2, ref["bound_var"])
    _close(one["log_evidence"], two["log_evidence"], ref["bound_log_evidence"])
    _close(one["ess"], two["ess"], ref["bound_ess"])
    assert (perm[two["map_atom"]] == one["map_atom"]).all()


@pytest.mark.parametrize("noise_sd", [0.0, NOISE_SD])
def test_doubling_the_dictionary_doubles_ess(gpu, noise_sd):
    b, y, atoms, lo, hi = _case("tri_reduced", 65, 300, 16)
    one = gpu.grid_posterior("tri_reduced", b, y, atoms, lo, hi, noise_sd=noise_sd)
    two = gpu.grid_posterior("tri_reduced", b, y, np.ascontiguousarray(np.tile(atoms, 2)), lo, hi, noise_sd=noise_sd)
    ref = reference("tri_reduced", b, y, np.tile(atoms, 2), lo, hi, noise_sd=noise_sd)
    _close(one["mean"].T, two["mean"].T, ref["bound_mean"])
    _close(one["sd"].T ** 2, two["sd"].T ** 2, ref["bound_var"])
    _close(one["log_evidence"], two["log_evidence"], ref["bound_log_evidence"])
    _close(2 * one["ess"], two["ess"], ref["bound_ess"])
    assert (one["map_atom"] == two["map_atom"]).all()  # the lower of the two copies


# ---- further checks
@pytest.mark.parametrize("project", [False, True])
def test_non_finite_voxels_do_not_touch_their_neighbours(gpu, project):
    model = "tri_s0" if project else "tri_reduced"
    b, y, atoms, lo, hi = _case(model, 64, 33, 16)
    clean = gpu.grid_posterior(model, b, y, atoms, lo, hi, project_amplitude=project)
    bad = y.copy()
    bad[3, 5] = np.nan
    bad[21, 0] = np.inf
    bad[40, 15] = -np.inf
    got, _ = _check(gpu, model, b, bad, atoms, lo, hi, project=project)  # accept() checks the NaN / -1 rows
    where = np.array([3, 21, 40])
    assert (got["map_atom"][where] == -1).all() and np.isnan(got["mean"][:, where]).all() and np.isnan(got["ess"][where]).all()
    rest = np.setdiff1d(np.arange(64), where)  # the other voxels of the same 16-voxel tiles: identical bytes
    for key in got:
        assert np.ascontiguousarray(got[key][..., rest]).tobytes() == np.ascontiguousarray(clean[key][..., rest]).tobytes(), key


@pytest.mark.parametrize("project", [False, True])
def test_map_atom_is_grid_starts_best_under_a_uniform_prior(gpu, project):
    b, y, atoms, lo, hi = _case("bi_s0", 500, 257, 16)
    for noise_sd in (0.0, NOISE_SD):
        got = gpu.grid_posterior("bi_s0", b, y, atoms, lo, hi, project_amplitude=project, noise_sd=noise_sd)
        gs = gpu.grid_start("bi_s0", b, y, atoms, lo, hi, project_amplitude=project)
        ref = grid_reference("bi_s0", b, y, atoms, lo, hi, project=project)
        two = np.sort(ref["c"], axis=1)[:, :2]
        clear = two[:, 1] - two[:, 0] > 2 * ref["tol"]
        assert clear.mean() > 0.99 and (got["map_atom"][clear] == gs["best"][clear]).all()
        assert np.ascontiguousarray(got["map_p"][:, clear]).tobytes() == np.ascontiguousarray(gs["p0"][:, clear]).tobytes()


def test_host_and_device_memory_return_the_same_bytes(gpu):
    import torch

    n_vox = 1000
    b, y, atoms, lo, hi = _case("tri_s0", n_vox, 257, 32)
    lp = np.log(np.random.default_rng(9).uniform(0.05, 1.0, 257))
    host = gpu.grid_posterior("tri_s0", b, y, atoms, lo, hi, project_amplitude=True, log_prior=lp, noise_sd=NOISE_SD)
    dev = torch.device("cuda", 0)
    yd = torch.from_numpy(y).to(dev)
    f = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    out = dict(mean=f(6, n_vox), sd=f(6, n_vox), map_atom=torch.empty(n_vox, dtype=torch.int32, device=dev), map_p=f(6, n_vox),
               log_evidence=f(n_vox), ess=f(n_vox))
    o = api.make_opts("tri_s0", 32, jac="analytic")
    stream = torch.cuda.current_stream(dev).cuda_stream
    api.grid_posterior_device(o, n_vox, b, yd, atoms, None, lo, hi, True, lp, NOISE_SD, out["mean"], out["sd"], out["map_atom"], out["map_p"],
                              out["log_evidence"], out["ess"], 0, stream)
    torch.cuda.synchronize()
    for key, t in out.items():
        assert host[key].tobytes() == t.cpu().numpy().tobytes(), key
    mean = f(6, n_vox).zero_()  # every output but the mean is optional
    api.grid_posterior_device(o, n_vox, b, yd, atoms, None, lo, hi, True, lp, NOISE_SD, mean, None, None, None, None, None, 0, stream)
    torch.cuda.synchronize()
    assert host["mean"].tobytes() == mean.cpu().numpy().tobytes()


def test_solver_under_the_pixelwise_fitter(gpu):
    rng = np.random.default_rng(10)
    b = synth.bvalues(16)
    truth = np.stack([rng.uniform(*TRUTH[n], 64) for n in ("f1", "D1", "D2", "S0")])
    img = (signals("bi_s0", b, truth) * 900.0 * (1 + 0.02 * rng.standard_normal((64, 16)))).reshape(8, 8, 1, 16)
    seg = np.zeros((8, 8, 1), int)
    seg[1:7, 2:8] = 1
    img[3, 3, 0, 2] = np.nan
    bounds = {"f1": (0.0, 1.0), "D1": (0.01, 0.5), "D2": (2e-3, 0.01), "S0": (100.0, 5000.0)}
    grid = {"f1": np.linspace(0.05, 0.45, 9), "D1": np.geomspace(0.012, 0.4, 8), "D2": np.linspace(2.5e-3, 9e-3, 7)}
    s = HipBayesGridSolver(BiExpModel(fit_s0=True), grid, p0={"S0": 900.0}, bounds=bounds, noise_sd=20.0)
    assert s.project is True and s._atoms.shape == (4, 504)
    fitter = HipPixelWiseFitter(s).fit(b, img, segmentation=seg)
    px = img[seg > 0]
    names = ["f1", "D1", "D2", "S0"]
    want = gpu.grid_posterior("bi_s0", b, px, s._atoms, np.array([bounds[n][0] for n in names]), np.array([bounds[n][1] for n in names]),
                              noise_sd=20.0, project_amplitude=True)
    for i, n in enumerate(names):
        assert np.asarray(s.params_[n]).tobytes() == want["mean"][i].tobytes()
        assert s.diagnostics_["posterior_sd"][n].tobytes() == want["sd"][i].tobytes() and s.diagnostics_["map"][n].shape == (36,)
    assert set(s.diagnostics_) == {"posterior_sd", "map", "map_atom", "log_evidence", "ess", "n_pixels"} and s.diagnostics_["n_pixels"] == 36
    assert s.diagnostics_["log_evidence"].shape == (36,) and s.diagnostics_["ess"].shape == (36,)
    ok = np.array([r.success for r in s.pixel_results_])
    assert ok.sum() == 35 and "NaN" in s.pixel_results_[int(np.flatnonzero(~ok)[0])].message
    assert (np.abs(np.asarray(s.params_["S0"])[ok] / 900.0 - truth[3].reshape(8, 8, 1)[seg > 0][ok]) < 0.2).all()
    assert fitter.results_ is not None

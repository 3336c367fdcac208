"""pnx_curvefit_varpro_posterior_f64 on the GPU against the numpy restatement (tests/varpro_posterior_reference.py): every axis of
the kernel (voxels, atoms, b-values, layouts), both boxes, both noise modes, both amplitude weights, sigma / fixed rates / T1,
priors, the one-atom dictionary, the argmin, the grid posterior as a second independent kernel, non-finite voxels, host against
device memory and the plugin class.

Acceptance per voxel (varpro_posterior_reference.accept, derivation in DESIGN.md 4.1i): every output of every case on every voxel
within its derived bound; the reference asserts its own preconditions (eps_v under the case's cap, no voxel on the cancellation
floor), which tests/test_varpro_posterior_host.py also runs on the CPU for the inputs used here."""
from __future__ import annotations

import numpy as np
import pytest
from grid_posterior_reference import reference as grid_posterior_reference
from grid_start_reference import signals
from varpro_posterior_reference import accept, apart_atoms, reference, wide_box
from varpro_reference import RATES, case_atoms, case_box, case_signals
from varpro_reference import reference as varpro_reference

from pyneapple_amd import api
from pyneapple_amd.models import TriExpModel
from pyneapple_amd.solvers import HipBayesVarProSolver

pytestmark = pytest.mark.gpu

NOISE_SD = 0.02  # the additive noise of case_signals: the known-noise mode of the cases below


def max_eps(narrow=False):
    """The eps cap of a case: the reference's default of 1e-6 in the wide box, where no clip is active (wide_box: asserted per case by
    test_varpro_posterior_host.py on the CPU); 1e-3, passed explicitly, in the narrow box only, where a clip is active at nearly every
    pair and the first-order clip term of the variable projection's tol dominates."""
    return 1e-3 if narrow else 1e-6


def _check(gpu, model, b, y, atoms, lo, hi, noise_sd=0.0, marginal=True, log_prior=None, narrow=False, **kw):
    got = gpu.varpro_posterior(model, b, y, atoms, lo, hi, log_prior=log_prior, noise_sd=noise_sd, marginal_amplitudes=marginal, **kw)
    ref = reference(model, b, y, atoms, lo, hi, log_prior=log_prior, noise_sd=noise_sd, marginal=marginal, max_eps=max_eps(narrow), **kw)
    accept(ref, got, atoms)
    return got, ref


def _both_modes(gpu, model, *case, **kw):
    _check(gpu, model, *case, noise_sd=0.0, **kw)
    return _check(gpu, model, *case, noise_sd=NOISE_SD, **kw)


# one pass of a block is 64 voxels (four waves, one strip of 16 each)
@pytest.mark.parametrize("n_vox", [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1000])
def test_voxel_axis(gpu, n_vox):
    b, y = case_signals("tri_s0", n_vox)
    _both_modes(gpu, "tri_s0", b, y, case_atoms("tri_s0"), *wide_box("tri_s0"))


def test_more_voxels_than_one_pass_of_the_grid(gpu):
    """The grid is capped at two blocks per CU: 70 001 voxels give every block of a 256-CU card a second pass."""
    b, y = case_signals("mono", 70001, n_b=5)
    _check(gpu, "mono", b, y, case_atoms("mono"), *wide_box("mono"))


@pytest.mark.parametrize("delta", [1 - 48, 15 - 48, 16 - 48, 17 - 48, -1, 0, 1, 16])
def test_atom_axis(gpu, delta):
    """1, 15, 16, 17 atoms and W - 1, W, W + 1, W + 16 around the slab width W of the tri-exponential layouts at 32 b-values."""
    W = api.varpro_posterior_slab_atoms(32, 3)
    assert W == 48
    b, y = case_signals("tri_reduced", 50)
    _both_modes(gpu, "tri_reduced", b, y, case_atoms("tri_reduced")[:, :W + delta], *wide_box("tri_reduced"))


def test_dictionary_at_the_cap(gpu):
    b, y = case_signals("mono", 40, n_b=4)
    _both_modes(gpu, "mono", b, y, np.geomspace(3e-4, 0.3, 4096)[None], *wide_box("mono"))


@pytest.mark.parametrize("model,n_b", [("mono", 2), ("mono", 4), ("mono", 5), ("tri_s0", 31), ("tri_s0", 32), ("tri_s0", 33), ("tri_s0", 64),
                                       ("tri_s0", 65), ("tri_s0", 128), ("bi_full", 128)])
def test_b_axis(gpu, model, n_b):
    b, y = case_signals(model, 150, n_b=n_b)
    _both_modes(gpu, model, b, y, case_atoms(model), *wide_box(model))


@pytest.mark.parametrize("model", sorted(api.MODEL_IDS))
@pytest.mark.parametrize("narrow", [False, True])
@pytest.mark.parametrize("noise_sd", [0.0, NOISE_SD])
@pytest.mark.parametrize("marginal", [False, True])
def test_every_layout_box_noise_mode_and_weight(gpu, model, narrow, noise_sd, marginal):
    """narrow: the truth lies outside the box of the fractions and of S0, so the clips of every class are active and clipped_mass
    (accepted against the reference like every output) is most of the posterior.  wide: no clip at any pair, clipped_mass is 0."""
    b, y = case_signals(model, 130)
    lo, hi = case_box(model, True) if narrow else wide_box(model)
    got, ref = _check(gpu, model, b, y, case_atoms(model), lo, hi, noise_sd=noise_sd, marginal=marginal, narrow=narrow)
    if narrow:
        assert got["clipped_mass"].mean() > 0.5
        rows = ref["lin_rows"]
        assert ((got["mean"][rows] >= lo[rows, None] - 1e-12) & (got["mean"][rows] <= hi[rows, None] + 1e-12)).all()  # a convex combination
    else:
        assert not ref["clipped_mass"].any() and not got["clipped_mass"].any()


def test_sigma(gpu):
    """The signals and sigma of test_gpu_varpro.py's case, on the pairs of rates that are not neighbours (apart_atoms says why)."""
    b, y = case_signals("bi_s0", 100)
    _both_modes(gpu, "bi_s0", b, y, apart_atoms("bi_s0"), *wide_box("bi_s0"), sigma=np.linspace(0.5, 2.0, 32))


def test_shared_fixed_rate(gpu):
    b, y = case_signals("tri_s0", 100)
    lo, hi = wide_box("tri_s0")
    free = [0, 1, 2, 3, 5]
    _both_modes(gpu, "tri_s0", b, y, case_atoms("tri_s0")[:2, ::4], lo[free], hi[free], fixed_idx=[4], fixed_vals=np.array([6e-4]))


@pytest.mark.parametrize("t1_mode,fixed", [(1, True), (2, True), (1, False)])
def test_t1_fixed_and_as_a_grid_axis(gpu, t1_mode, fixed):
    rng = np.random.default_rng(11)
    b = np.linspace(0.0, 1000.0, 32)
    kw = dict(t1_mode=t1_mode, tr=3000.0, tm=20.0 if t1_mode == 2 else 0.0)
    truth = np.stack([rng.uniform(0.8, 1.2, 90), rng.uniform(1e-3, 3e-3, 90), np.full(90, 1000.0) if fixed else rng.uniform(700.0, 1500.0, 90)])
    y = signals("mono", b, truth, **kw) + 0.02 * rng.standard_normal((90, 32))
    d = np.geomspace(3e-4, 0.03, 8)
    if fixed:
        _both_modes(gpu, "mono", b, y, d[None], np.array([0.0, 1e-5]), np.array([10.0, 0.5]), fixed_idx=[2], fixed_vals=np.array([1000.0]), **kw)
    else:
        atoms = np.ascontiguousarray(np.array([(a, t) for a in d for t in (600.0, 1000.0, 1600.0)]).T)
        _both_modes(gpu, "mono", b, y, atoms, np.array([0.0, 1e-5, 100.0]), np.array([10.0, 0.5, 5000.0]), **kw)


def test_log_prior_with_excluded_atoms(gpu):
    b, y = case_signals("tri_s0", 65)
    atoms = case_atoms("tri_s0")
    rng = np.random.default_rng(3)
    lp = np.log(rng.uniform(0.01, 1.0, 64)) + 2.5  # not normalised: the library normalises
    lp[rng.random(64) < 1 / 3] = -np.inf
    assert np.isinf(lp).any()
    got, ref = _both_modes(gpu, "tri_s0", b, y, atoms, *wide_box("tri_s0"), log_prior=lp)
    assert np.isfinite(lp[got["map_atom"]]).all() and (ref["W"][:, np.isinf(lp)] == 0).all()


@pytest.mark.parametrize("noise_sd", [0.0, NOISE_SD])
def test_all_atoms_but_one_excluded(gpu, noise_sd):
    b, y = case_signals("tri_s0", 65)
    atoms = case_atoms("tri_s0")
    lo, hi = wide_box("tri_s0")
    lp = np.full(64, -np.inf)
    lp[37] = -0.5
    got, ref = _check(gpu, "tri_s0", b, y, atoms, lo, hi, noise_sd=noise_sd, log_prior=lp)
    assert (got["map_atom"] == 37).all() and (got["ess"] == 1.0).all() and (got["sd"] == 0.0).all()
    assert got["mean"].tobytes() == got["map_p"].tobytes()
    assert (got["mean"][ref["nl_rows"]].view(np.uint64) == np.repeat(atoms[:, 37:38], 65, axis=1).view(np.uint64)).all()


@pytest.mark.parametrize("model", ["mono", "tri_s0", "tri_reduced"])
@pytest.mark.parametrize("noise_sd", [0.0, NOISE_SD])
def test_a_dictionary_of_one_atom(gpu, model, noise_sd):
    b, y = case_signals(model, 65)
    atoms = np.ascontiguousarray(case_atoms(model)[:, 21 % case_atoms(model).shape[1]][:, None])
    lo, hi = wide_box(model)
    got, ref = _check(gpu, model, b, y, atoms, lo, hi, noise_sd=noise_sd)
    vp = gpu.varpro(model, b, y, atoms, lo, hi, lo + 0.25 * (hi - lo))
    assert (np.abs(got["mean"][ref["lin_rows"]].T - vp["params"][ref["lin_rows"]].T) <= 2 * ref["param_bound"][:, 0]).all()
    assert got["mean"][ref["nl_rows"]].tobytes() == vp["params"][ref["nl_rows"]].tobytes()
    assert (got["sd"] == 0.0).all() and (got["ess"] == 1.0).all() and (got["map_atom"] == 0).all()
    assert (got["clipped_mass"] == vp["clipped"]).all()


@pytest.mark.parametrize("model", ["bi_s0", "tri_s0"])
def test_map_atom_is_the_argmin_under_a_uniform_prior(gpu, model):
    """marginal_amplitudes = 0, known noise, uniform prior: l is a decreasing function of the cost alone."""
    b, y = case_signals(model, 300)
    atoms = case_atoms(model)
    lo, hi = case_box(model)
    got = gpu.varpro_posterior(model, b, y, atoms, lo, hi, noise_sd=NOISE_SD, marginal_amplitudes=False)
    vp = gpu.varpro(model, b, y, atoms, lo, hi, lo + 0.25 * (hi - lo))
    ref = varpro_reference(model, b, y, atoms, lo, hi)
    v = np.arange(300)
    assert (np.abs(ref["c"][v, got["map_atom"]] - ref["c"][v, vp["atom"]]) <= ref["tol"]).all()
    same = got["map_atom"] == vp["atom"]
    assert same.mean() > 0.95
    np.testing.assert_allclose(got["map_p"][:, same], vp["params"][:, same], rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("noise_sd", [0.0, NOISE_SD])
def test_mono_agrees_with_the_projected_grid_posterior(gpu, noise_sd):
    """Two independent kernels: on mono the profile weight is the grid posterior's with a projected amplitude.  The allowed
    difference is the sum of the two references' bounds."""
    b, y = case_signals("mono", 300)
    lo, hi = wide_box("mono")
    d = np.array(RATES)
    got, ref = _check(gpu, "mono", b, y, d[None], lo, hi, noise_sd=noise_sd, marginal=False)
    full = np.stack([np.ones(8), d])
    gp = gpu.grid_posterior("mono", b, y, full, lo, hi, project_amplitude=True, noise_sd=noise_sd)
    gref = grid_posterior_reference("mono", b, y, full, lo, hi, project=True, noise_sd=noise_sd)
    assert (np.abs(got["mean"] - gp["mean"]).T <= ref["bound_mean"] + gref["bound_mean"]).all()
    assert (np.abs(got["sd"] ** 2 - gp["sd"] ** 2).T <= ref["bound_var"] + gref["bound_var"]).all()
    assert (np.abs(got["log_evidence"] - gp["log_evidence"]) <= ref["bound_log_evidence"] + gref["bound_log_evidence"]).all()
    assert (np.abs(got["ess"] - gp["ess"]) <= ref["bound_ess"] + gref["bound_ess"]).all()


@pytest.mark.parametrize("model", ["bi_reduced", "tri_s0"])
def test_non_finite_voxels_leave_their_neighbours_bit_identical(gpu, model):
    b, y = case_signals(model, 70)
    atoms = case_atoms(model)
    lo, hi = wide_box(model)
    clean = gpu.varpro_posterior(model, b, y, atoms, lo, hi)
    bad = y.copy()
    bad[3, 5], bad[16, 0], bad[33, 31], bad[69, 7] = np.nan, np.inf, -np.inf, np.nan
    got, _ = _check(gpu, model, b, bad, atoms, lo, hi)  # accept() checks the NaN / -1 rows
    where = np.array([3, 16, 33, 69])
    assert (got["map_atom"][where] == -1).all() and np.isnan(got["mean"][:, where]).all() and np.isnan(got["clipped_mass"][where]).all()
    rest = np.setdiff1d(np.arange(70), where)
    for key in got:
        assert np.ascontiguousarray(got[key][..., rest]).tobytes() == np.ascontiguousarray(clean[key][..., rest]).tobytes(), key


@pytest.mark.parametrize("n_vox,chunk", [(1000, None), (2500, 1024)])  # 2500 voxels in chunks of 1024: three pieces through the ring
def test_host_and_device_memory_return_the_same_bytes(gpu, monkeypatch, n_vox, chunk):
    import torch

    if chunk:
        monkeypatch.setenv("PNX_HOST_CHUNK", str(chunk))
    b, y = case_signals("tri_s0", n_vox)
    atoms = case_atoms("tri_s0")
    lo, hi = case_box("tri_s0")
    lp = np.log(np.random.default_rng(9).uniform(0.05, 1.0, 64))
    host = gpu.varpro_posterior("tri_s0", b, y, atoms, lo, hi, log_prior=lp, noise_sd=NOISE_SD)
    dev = torch.device("cuda", 0)
    yd = torch.from_numpy(y).to(dev)
    f = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    out = dict(mean=f(6, n_vox), sd=f(6, n_vox), map_atom=torch.empty(n_vox, dtype=torch.int32, device=dev), map_p=f(6, n_vox),
               log_evidence=f(n_vox), ess=f(n_vox), clipped_mass=f(n_vox))
    o = api.make_opts("tri_s0", 32, jac="analytic")
    st = torch.cuda.current_stream(dev).cuda_stream
    api.varpro_posterior_device(o, n_vox, b, yd, atoms, None, lo, hi, lp, NOISE_SD, True, out["mean"], out["sd"], out["map_atom"], out["map_p"],
                                out["log_evidence"], out["ess"], out["clipped_mass"], 0, st)
    torch.cuda.synchronize()
    for key, t in out.items():
        assert host[key].tobytes() == t.cpu().numpy().tobytes(), key
    mean = f(6, n_vox).zero_()  # every output but the mean is optional
    api.varpro_posterior_device(o, n_vox, b, yd, atoms, None, lo, hi, lp, NOISE_SD, True, mean, None, None, None, None, None, None, 0, st)
    torch.cuda.synchronize()
    assert host["mean"].tobytes() == mean.cpu().numpy().tobytes()


# ---- through the plugin interface
BOUNDS = {"f1": (-40.0, 40.0), "D1": (1e-5, 0.5), "f2": (-40.0, 40.0), "D2": (1e-5, 0.5), "D3": (1e-5, 0.5), "S0": (0.0, 10.0)}  # wide_box
P0 = {"f1": 0.2, "D1": 0.1, "f2": 0.3, "D2": 0.01, "D3": 0.001, "S0": 1.0}
TRI = {"D1": list(np.geomspace(0.04, 0.3, 4)), "D2": list(np.geomspace(4e-3, 0.02, 4)), "D3": list(np.geomspace(3e-4, 1.5e-3, 4))}
NAMES = api.MODEL_PARAM_NAMES["tri_s0"]


def test_hip_bayes_varpro_through_the_plugin_interface(gpu):
    b, y = case_signals("tri_s0", 200)
    y[7, 3] = np.nan
    s = HipBayesVarProSolver(TriExpModel(fit_s0=True), TRI, max_iter=250, tol=1e-8, p0=P0, bounds=BOUNDS, noise_sd=NOISE_SD).fit(b, y)
    assert s._nl_atoms.tobytes() == case_atoms("tri_s0").tobytes()
    lo, hi = (np.array([BOUNDS[n][i] for n in NAMES]) for i in (0, 1))
    got, _ = _check(gpu, "tri_s0", b, y, s._nl_atoms, lo, hi, noise_sd=NOISE_SD)
    assert np.stack([s.params_[n] for n in NAMES]).tobytes() == got["mean"].tobytes()
    assert set(s.diagnostics_) == {"posterior_sd", "map", "map_atom", "log_evidence", "ess", "clipped_mass", "n_pixels"} and s.diagnostics_["n_pixels"] == 200
    for i, n in enumerate(NAMES):
        assert s.diagnostics_["posterior_sd"][n].tobytes() == got["sd"][i].tobytes() and s.diagnostics_["map"][n].tobytes() == got["map_p"][i].tobytes()
    for key in ("map_atom", "log_evidence", "ess", "clipped_mass"):
        assert s.diagnostics_[key].tobytes() == got[key].tobytes()
    ok = [r.success for r in s.pixel_results_]
    assert ok.count(False) == 1 and not ok[7] and s.diagnostics_["map_atom"][7] == -1 and np.isnan(s.params_["f1"][7])

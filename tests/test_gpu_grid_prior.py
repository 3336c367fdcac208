"""pnx_curvefit_grid_prior_em_f64 on the device against tests/grid_prior_reference.py (numpy EM on the posterior reference's l_g):
one update at the tile edges of every axis, three updates, a long run checked step by step, the properties of an EM, what the
learned prior is worth, and HipBayesGridSolver's empirical_prior end to end.

Acceptance of one update (grid_prior_reference.step_bounds, derivation in DESIGN.md 4.1j): the library's l_g differs from the
reference's by at most eps_v, so a normalised weight moves by e^{+-2 eps_v}; sums over G atoms and N voxels add gamma_G and gamma_N;
log_prior after the update is held to log1p of that, the log-likelihood to the sum of the posterior's log-evidence bounds.  After
t <= 3 updates the bound against an all-numpy run is (2^t - 1) single-step bounds; a long run is checked one step at a time against
the library's own previous prior.  Oracle-compared cases satisfy eps_v <= 1e-6 on every voxel (asserted by the reference).

The largest error-to-bound ratios observed are recorded in DESIGN.md 4.1j."""
from __future__ import annotations

import functools

import numpy as np
import pytest
from grid_posterior_reference import U
from grid_prior_reference import accept_step, em_step, likelihoods, normalise, population, step_bounds
from grid_start_reference import signals

from pyneapple_amd import api, synth
from pyneapple_amd.models import BiExpModel
from pyneapple_amd.solvers import HipBayesGridSolver

pytestmark = pytest.mark.gpu

BOUNDS = {"f1": (0.0, 1.0), "f2": (0.0, 1.0), "f3": (0.0, 1.0), "D": (1e-5, 0.1), "D1": (0.01, 0.5), "D2": (2e-3, 0.01), "D3": (1e-5, 2e-3),
          "S0": (0.5, 2.0)}
TRUTH = {**BOUNDS, "f1": (0.05, 0.4), "f2": (0.05, 0.4), "f3": (0.05, 0.4), "S0": (0.6, 1.8)}
NOISE_SD = 0.05  # the known-noise mode: signals of order 1 with 2 % noise, so the weights spread over atoms


def _case(model, n_vox, n_atoms, n_b, seed=0, noise=0.02):
    """(b, y, atoms, lo, hi): atoms uniform inside the bounds, signals of uniform truth values with additive Gaussian noise."""
    rng = np.random.default_rng(1000 * seed + 7 * n_vox + 3 * n_atoms + n_b)
    names = api.MODEL_PARAM_NAMES[model]
    lo = np.array([BOUNDS[n][0] for n in names])
    hi = np.array([BOUNDS[n][1] for n in names])
    atoms = np.ascontiguousarray(rng.uniform(lo[:, None], hi[:, None], (len(names), n_atoms)))
    truth = np.stack([rng.uniform(*TRUTH[n], n_vox) for n in names])
    b = synth.bvalues(n_b)
    y = signals(model, b, truth)
    return b, np.ascontiguousarray(y + noise * rng.standard_normal(y.shape)), atoms, lo, hi


def _accept(got, l0, eps0, fin, lp0, alpha, steps):
    """The result of `steps` updates (rel_tol = 0) against the all-numpy run from the same normalised start lp0."""
    n = int(fin.sum())
    assert got["n_eff"] == n and got["n_iter"] == steps and got["loglik"].shape == (steps + 1,) and got["log_prior"].dtype == np.float64
    lp, drift, worst = lp0, 0.0, 0.0  # drift: how far the library's prior may be from numpy's before update t
    for t in range(steps + 1):
        S, lp_next, ll = em_step(l0, lp, fin, alpha)
        bd = step_bounds(l0, lp, eps0, fin, S)
        bound = bd["loglik"] + n * drift  # a prior moved by eta moves every L_v by at most eta
        err = abs(got["loglik"][t] - ll)
        print(f"loglik[{t}] = {got['loglik'][t]!r}: error {err:.3g}, bound {bound:.3g}")
        assert err <= bound, f"loglik[{t}]: error is {err / bound:.3g} x its bound"
        worst = max(worst, err / bound)
        if t < steps:
            drift = 2 * drift + bd["lp"]
            last = (lp_next, S, bd["lp"])
            lp = lp_next
    q = accept_step(got["log_prior"], lp0, last[0], last[1], n, drift, alpha)
    print(f"log_prior: error / bound = {q:.3g} after {steps} update(s); loglik worst {worst:.3g}")
    return q


def _run(gpu, model, case, steps=1, project=False, noise_sd=0.0, log_prior=None, alpha=0.0, **kw):
    b, y, atoms, lo, hi = case
    got = gpu.grid_prior_em(model, b, y, atoms, lo, hi, log_prior=log_prior, noise_sd=noise_sd, n_iter=steps, pseudo_count=alpha, rel_tol=0.0,
                            project_amplitude=project, **kw)
    l0, eps0, fin = likelihoods(model, b, y, atoms, lo, hi, noise_sd=noise_sd, project=project, **kw)
    _accept(got, l0, eps0, fin, normalise(log_prior, atoms.shape[1]), alpha, steps)
    return got


def _both_modes(gpu, model, case, **kw):
    _run(gpu, model, case, noise_sd=0.0, **kw)
    return _run(gpu, model, case, noise_sd=NOISE_SD, **kw)


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


PROJ = [("tri_reduced", False), ("bi_s0", True)]  # both instantiations of the amplitude projection


# ---- one update against numpy: tile edges of each axis crossed with a mid value of the others
@pytest.mark.parametrize("model,project", PROJ)
@pytest.mark.parametrize("n_vox", [1, 15, 16, 17, 65])
def test_one_step_voxel_axis(gpu, n_vox, model, project):
    _both_modes(gpu, model, _case(model, n_vox, 33, 16), project=project)


@pytest.mark.parametrize("model,project", PROJ)
def test_one_step_more_voxel_groups_than_blocks(gpu, model, project):
    """2 x CUs blocks of 64 voxels and 69 voxels more: the first blocks go round their loop twice, the last group is partly filled."""
    n_vox = 2 * _cus() * 64 + 69
    _run(gpu, model, _case(model, n_vox, 48, 8), project=project, noise_sd=NOISE_SD if project else 0.0)


@pytest.mark.parametrize("model,project", PROJ)
@pytest.mark.parametrize("n_atoms", [1, 15, 16, 17, "posterior slab + 16", "slab + 16"])
def test_one_step_atom_axis(gpu, n_atoms, model, project):
    """The last two: two slabs with the second partly filled -- 16 atoms past the posterior kernel's slab and past this kernel's own
    (api.grid_prior_slab_atoms: at 32 b-values it is wider than the posterior's)."""
    n_free = len(api.MODEL_PARAM_NAMES[model])
    if n_atoms == "posterior slab + 16":
        n_atoms = api.grid_posterior_slab_atoms(32, n_free) + 16
    elif n_atoms == "slab + 16":
        n_atoms = api.grid_prior_slab_atoms(32) + 16
        assert n_atoms >= api.grid_posterior_slab_atoms(32, n_free) + 16  # equal at four free parameters, wider above
    _both_modes(gpu, model, _case(model, 65, n_atoms, 32), project=project)


@pytest.mark.parametrize("n_b", [1, 4, 5, 32, 33, 128])  # 33 and up take the larger instantiation; 1 and 5 pad the k-steps
def test_one_step_b_axis(gpu, n_b):
    _both_modes(gpu, "tri_reduced", _case("tri_reduced", 65, 33, n_b))


@pytest.mark.parametrize("n_b", [5, 33])
def test_one_step_b_axis_projected(gpu, n_b):
    _both_modes(gpu, "bi_s0", _case("bi_s0", 65, 33, n_b), project=True)


def test_one_step_mono_projected(gpu):
    _both_modes(gpu, "mono", _case("mono", 65, 33, 16), project=True)


def test_one_step_sigma_vector(gpu):
    sigma = np.linspace(0.5, 3.0, 16)
    _both_modes(gpu, "tri_reduced", _case("tri_reduced", 65, 33, 16), sigma=sigma)
    _both_modes(gpu, "bi_s0", _case("bi_s0", 65, 33, 16), project=True, sigma=sigma)


@pytest.mark.parametrize("model,project", PROJ)
def test_one_step_excluded_atoms_stay_excluded(gpu, model, project):
    rng = np.random.default_rng(3)
    lp = np.log(rng.uniform(0.01, 1.0, 100)) + 2.5  # not normalised: the library normalises
    lp[rng.random(100) < 1 / 3] = -np.inf
    for alpha in (0.0, 0.25):
        got = _both_modes(gpu, model, _case(model, 65, 100, 16), project=project, log_prior=lp, alpha=alpha)
        assert np.isinf(got["log_prior"][np.isinf(lp)]).all()
        if alpha:  # without a pseudo-count a far atom's weight sum may underflow to 0 in the known-noise mode
            assert np.isfinite(got["log_prior"][np.isfinite(lp)]).all()


@pytest.mark.parametrize("model,project", PROJ)
def test_one_step_non_finite_voxels_take_no_part(gpu, model, project):
    """A NaN and an Inf voxel in the middle of a strip: not counted, and the result is that of the reference without them."""
    b, y, atoms, lo, hi = _case(model, 64, 33, 16)
    y[21, 5] = np.nan
    y[38, 0] = np.inf
    got = _both_modes(gpu, model, (b, y, atoms, lo, hi), project=project)
    assert got["n_eff"] == 62 and np.isfinite(got["loglik"]).all()
    none = gpu.grid_prior_em(model, b, np.full((5, 16), np.nan), atoms, lo, hi, n_iter=3, project_amplitude=project)
    assert none["n_eff"] == 0 and none["n_iter"] == 0 and none["loglik"][0] == 0.0 and np.isnan(none["loglik"][1:]).all()
    assert none["log_prior"].tobytes() == normalise(None, 33).tobytes()


# ---- more than one update
@pytest.mark.parametrize("model,project", PROJ)
def test_three_steps_against_numpy(gpu, model, project):
    _both_modes(gpu, model, _case(model, 300, 100, 16), steps=3, project=project)


@functools.lru_cache(maxsize=None)
def _population():
    return population(1000, seed=0)


@pytest.mark.parametrize("noise_sd", [0.0, 0.05])
def test_step_consistency_over_a_long_run(gpu, noise_sd):
    """The library is deterministic: its 20-update run repeats its 19-update run bit for bit and adds one update, which numpy
    reproduces from the 19-update prior within the single-step bound."""
    b, y, _, _, atoms, lo, hi = _population()
    kw = dict(noise_sd=noise_sd, project_amplitude=True, rel_tol=0.0)
    r19 = gpu.grid_prior_em("bi_s0", b, y, atoms, lo, hi, n_iter=19, **kw)
    r20 = gpu.grid_prior_em("bi_s0", b, y, atoms, lo, hi, n_iter=20, **kw)
    assert r19["n_iter"] == 19 and r20["n_iter"] == 20
    assert r19["loglik"][:19].tobytes() == r20["loglik"][:19].tobytes()
    assert r19["loglik"][19] == r20["loglik"][19]  # under the same prior, by the same pass
    l0, eps0, fin = likelihoods("bi_s0", b, y, atoms, lo, hi, noise_sd=noise_sd, project=True)
    S, lp_next, ll = em_step(l0, r19["log_prior"], fin)
    bd = step_bounds(l0, r19["log_prior"], eps0, fin, S)
    q = accept_step(r20["log_prior"], r19["log_prior"], lp_next, S, 1000, bd["lp"])
    print(f"update 20 from the library's update 19: error / bound = {q:.3g}")
    assert abs(r19["loglik"][19] - ll) <= bd["loglik"]


# ---- properties of an EM, on 1000 voxels
@pytest.mark.parametrize("noise_sd", [0.0, 0.05])
def test_properties_of_thirty_updates(gpu, noise_sd):
    import torch

    b, y, _, _, atoms, lo, hi = _population()
    G, n = atoms.shape[1], 1000
    kw = dict(noise_sd=noise_sd, project_amplitude=True, n_iter=30, pseudo_count=0.0, rel_tol=0.0)
    one = gpu.grid_prior_em("bi_s0", b, y, atoms, lo, hi, **kw)
    lp = one["log_prior"]
    assert one["n_iter"] == 30 and one["n_eff"] == n and np.isfinite(one["loglik"]).all()
    adm = lp > -np.inf
    gamma_g = 4 * (G + 16) * U
    total = np.log(np.exp(lp[adm] - lp[adm].max()).sum()) + lp[adm].max()
    assert abs(total) <= gamma_g, total  # the reported prior sums to 1 over its finite entries
    # the derived bound on a sum of L_v under this prior
    l0, eps0, fin = likelihoods("bi_s0", b, y, atoms, lo, hi, noise_sd=noise_sd, project=True)
    S, _, ll = em_step(l0, lp, fin)
    bound = step_bounds(l0, lp, eps0, fin, S)["loglik"]
    steps = np.diff(one["loglik"])
    print(f"loglik {one['loglik'][0]:.6f} -> {one['loglik'][-1]:.6f}, smallest step {steps.min():.3g}, bound {bound:.3g}")
    assert (steps >= -2 * bound).all() and one["loglik"][-1] > one["loglik"][0] + 1.0
    assert abs(one["loglik"][30] - ll) <= bound
    post = gpu.grid_posterior("bi_s0", b, y, atoms, lo, hi, log_prior=lp, noise_sd=noise_sd, project_amplitude=True)
    assert abs(post["log_evidence"].sum() - one["loglik"][30]) <= bound
    # reproducible, and the same from device memory
    two = gpu.grid_prior_em("bi_s0", b, y, atoms, lo, hi, **kw)
    assert one["log_prior"].tobytes() == two["log_prior"].tobytes() and one["loglik"].tobytes() == two["loglik"].tobytes()
    dev = torch.device("cuda", 0)
    yd = torch.from_numpy(y).to(dev)
    o = api.make_opts("bi_s0", len(b), jac="analytic")
    three = api.grid_prior_em_device(o, n, b, yd, atoms, None, lo, hi, True, None, noise_sd, 30, 0.0, 0.0, 0, torch.cuda.current_stream(dev).cuda_stream)
    assert one["log_prior"].tobytes() == three["log_prior"].tobytes() and one["loglik"].tobytes() == three["loglik"].tobytes()
    assert three["n_iter"] == 30 and three["n_eff"] == n


def test_duplicating_the_voxels_changes_nothing(gpu):
    b, y, _, _, atoms, lo, hi = _population()
    kw = dict(noise_sd=0.05, project_amplitude=True, n_iter=1, rel_tol=0.0)
    one = gpu.grid_prior_em("bi_s0", b, y, atoms, lo, hi, **kw)
    two = gpu.grid_prior_em("bi_s0", b, np.ascontiguousarray(np.tile(y, (2, 1))), atoms, lo, hi, **kw)
    assert two["n_eff"] == 2000
    l0, eps0, fin = likelihoods("bi_s0", b, np.tile(y, (2, 1)), atoms, lo, hi, noise_sd=0.05, project=True)
    lp0 = normalise(None, atoms.shape[1])
    S, lp_next, _ = em_step(l0, lp0, fin)
    bd = step_bounds(l0, lp0, eps0, fin, S)
    accept_step(two["log_prior"], lp0, one["log_prior"], S, 2000, bd["lp"])
    assert abs(two["loglik"][0] - 2 * one["loglik"][0]) <= bd["loglik"]


@pytest.mark.parametrize("noise_sd", [0.0, 0.05])
def test_pseudo_count_keeps_every_admissible_atom(gpu, noise_sd):
    b, y, _, _, atoms, lo, hi = _population()
    lp = np.zeros(atoms.shape[1])
    lp[::7] = -np.inf
    got = _run(gpu, "bi_s0", (b, y, atoms, lo, hi), project=True, noise_sd=noise_sd, log_prior=lp, alpha=0.5)
    assert (np.isinf(got["log_prior"]) == np.isinf(lp)).all()
    n_adm = int(np.isfinite(lp).sum())
    assert (got["log_prior"][np.isfinite(lp)] >= np.log(0.5 / (1000 + 0.5 * n_adm)) - 1e-12).all()
    long = gpu.grid_prior_em("bi_s0", b, y, atoms, lo, hi, log_prior=lp, noise_sd=noise_sd, project_amplitude=True, n_iter=30, pseudo_count=0.5, rel_tol=0.0)
    assert (np.isinf(long["log_prior"]) == np.isinf(lp)).all()


def test_rel_tol_stops_the_run(gpu):
    b, y, _, _, atoms, lo, hi = _population()
    got = gpu.grid_prior_em("bi_s0", b, y, atoms, lo, hi, noise_sd=0.05, project_amplitude=True, n_iter=6, rel_tol=1.0)
    assert got["n_iter"] == 1 and np.isfinite(got["loglik"][:2]).all() and np.isnan(got["loglik"][2:]).all() and got["loglik"].shape == (7,)
    one = gpu.grid_prior_em("bi_s0", b, y, atoms, lo, hi, noise_sd=0.05, project_amplitude=True, n_iter=1, rel_tol=0.0)
    assert one["log_prior"].tobytes() == got["log_prior"].tobytes() and one["loglik"].tobytes() == got["loglik"][:2].tobytes()
    loose = gpu.grid_prior_em("bi_s0", b, y, atoms, lo, hi, noise_sd=0.05, project_amplitude=True, n_iter=200, rel_tol=1e-4)
    assert 1 < loose["n_iter"] < 200
    ll, d = loose["loglik"], loose["n_iter"]
    assert ll[d] - ll[d - 1] <= 1e-4 * abs(ll[d]) and (np.diff(ll[:d]) > 1e-4 * np.abs(ll[1:d])).all()


# ---- what it is worth
@pytest.mark.parametrize("noise_sd", [0.0, 0.05])
def test_it_earns_its_keep(gpu, noise_sd):
    """1000 voxels of a narrow population at 5 % noise, a grid over far wider ranges: under the prior learned in 30 updates the
    median absolute errors of f1 and D1 are at most 0.75 of those under the uniform prior (the numpy reference gives 0.57 and
    0.46 marginalised, 0.54 and 0.42 with the noise known)."""
    b, y, truth, _, atoms, lo, hi = _population()
    kw = dict(noise_sd=noise_sd, project_amplitude=True)
    learned = gpu.grid_prior_em("bi_s0", b, y, atoms, lo, hi, n_iter=30, rel_tol=0.0, **kw)
    flat = gpu.grid_posterior("bi_s0", b, y, atoms, lo, hi, **kw)["mean"]
    post = gpu.grid_posterior("bi_s0", b, y, atoms, lo, hi, log_prior=learned["log_prior"], **kw)["mean"]
    err = lambda mean: np.median(np.abs(mean[:3] - truth[:3]), axis=1)
    ratio = err(post) / err(flat)
    print("median abs error uniform", err(flat), "learned", err(post), "ratio", ratio)
    assert ratio[0] <= 0.75 and ratio[1] <= 0.75


# ---- through the plugin
def test_through_the_solver(gpu):
    b, y, _, grid, atoms, lo, hi = _population()
    names = ["f1", "D1", "D2", "S0"]
    bounds = {n: (float(lo[i]), float(hi[i])) for i, n in enumerate(names)}
    mk = lambda **kw: HipBayesGridSolver(BiExpModel(fit_s0=True), grid, p0={"S0": 1.0}, bounds=bounds, noise_sd=0.05, **kw)
    s = mk(empirical_prior={"n_iter": 5})
    assert s.project is True and s._atoms.tobytes() == atoms.tobytes()
    s.fit(b, y)
    em5 = gpu.grid_prior_em("bi_s0", b, y, atoms, lo, hi, noise_sd=0.05, project_amplitude=True, n_iter=5, pseudo_count=0.0, rel_tol=1e-6)
    want = gpu.grid_posterior("bi_s0", b, y, atoms, lo, hi, noise_sd=0.05, project_amplitude=True, log_prior=em5["log_prior"])
    d = s.diagnostics_
    assert set(d) == {"posterior_sd", "map", "map_atom", "log_evidence", "ess", "n_pixels", "log_prior", "prior_loglik", "prior_n_iter", "prior_n_voxels"}
    assert d["log_prior"].tobytes() == em5["log_prior"].tobytes() and d["prior_loglik"].tobytes() == em5["loglik"].tobytes()
    assert d["prior_n_iter"] == em5["n_iter"] and d["prior_n_voxels"] == 1000 and d["log_prior"].shape == (384,) and s.log_prior is None
    for i, n in enumerate(names):
        assert np.asarray(s.params_[n]).tobytes() == want["mean"][i].tobytes() and d["posterior_sd"][n].tobytes() == want["sd"][i].tobytes()
    assert d["log_evidence"].tobytes() == want["log_evidence"].tobytes()
    # max_voxels: the evenly strided subset ydata[::ceil(n / max_voxels)], here every fourth voxel
    sub = mk(empirical_prior={"n_iter": 5, "max_voxels": 300}).fit(b, y)
    em_sub = gpu.grid_prior_em("bi_s0", b, y[::4], atoms, lo, hi, noise_sd=0.05, project_amplitude=True, n_iter=5)
    assert sub.diagnostics_["prior_n_voxels"] == 250 and sub.diagnostics_["log_prior"].tobytes() == em_sub["log_prior"].tobytes()
    assert len(sub.params_["f1"]) == 1000
    # a start prior is the EM's start; off is today's posterior, bit for bit
    lp = np.zeros(384)
    lp[:48] = -np.inf
    st = mk(log_prior=lp, empirical_prior=True).fit(b, y)
    em_st = gpu.grid_prior_em("bi_s0", b, y, atoms, lo, hi, noise_sd=0.05, project_amplitude=True, log_prior=lp)
    assert st.diagnostics_["log_prior"].tobytes() == em_st["log_prior"].tobytes() and np.isinf(st.diagnostics_["log_prior"][:48]).all()
    off = mk(empirical_prior=None).fit(b, y)
    plain = gpu.grid_posterior("bi_s0", b, y, atoms, lo, hi, noise_sd=0.05, project_amplitude=True)
    assert set(off.diagnostics_) == {"posterior_sd", "map", "map_atom", "log_evidence", "ess", "n_pixels"}
    for i, n in enumerate(names):
        assert np.asarray(off.params_[n]).tobytes() == plain["mean"][i].tobytes()

"""pnx_curvefit_grid_marginals_f64 on the device against tests/grid_marginal_reference.py (numpy, on the posterior reference's
l_g): the marginal of every free parameter and the quantiles from it at the tile edges of every axis -- voxels, atoms, b-values and
bins --, excluded atoms, non-finite voxels, the properties that tie it to the posterior, reproducibility, and HipBayesGridSolver's
`marginals` end to end.

Acceptance (grid_marginal_reference.accept; derived as in DESIGN.md 4.1j, not measured): the library's l_g is within eps_v of the
reference's, so a normalised weight moves by e^{+-2 eps_v}, and a sum over at most G atoms in any order adds gamma_G =
4 (G + 16) 2^-52:  |marginal - ref| <= (expm1(2 eps_v) + gamma_G) ref + 1e-300 per bin, |sum_j marginal - 1| within the same bound,
and a quantile's bin j* is accepted when cdf_ref[j*] + D >= p and cdf_ref[j* - 1] - D < p with D the summed bounds of the bins up
to there.  No voxel is excluded.  Oracle-compared cases satisfy eps_v <= 1e-6 on every voxel (asserted by the reference).

The largest error-to-bound ratio observed is recorded in DESIGN.md 4.1k."""
from __future__ import annotations

import functools

import numpy as np
import pytest
from grid_marginal_reference import accept, reference
from grid_posterior_reference import U
from grid_prior_reference import population
from grid_start_reference import signals

from pyneapple_amd import api, synth
from pyneapple_amd.models import BiExpModel
from pyneapple_amd.solvers import HipBayesGridSolver

pytestmark = pytest.mark.gpu

BOUNDS = {"f1": (0.0, 1.0), "f2": (0.0, 1.0), "f3": (0.0, 1.0), "D": (1e-5, 0.1), "D1": (0.01, 0.5), "D2": (2e-3, 0.01), "D3": (1e-5, 2e-3),
          "S0": (0.5, 2.0)}
TRUTH = {**BOUNDS, "f1": (0.05, 0.4), "f2": (0.05, 0.4), "f3": (0.05, 0.4), "S0": (0.6, 1.8)}
NOISE_SD = 0.05  # the known-noise mode: signals of order 1 with 2 % noise, so the weights spread over atoms
PROBS = (0.025, 0.5, 0.975)
PROJ = [("tri_reduced", False), ("bi_s0", True)]  # both instantiations of the amplitude projection
MID = {"tri_reduced": (4, 3, 0, 5, 2), "bi_s0": (4, 3, 5, 0)}  # B = 14 and 12, a parameter without a marginal in the middle / at S0


@functools.lru_cache(maxsize=None)
def _case(model, n_vox, n_atoms, n_b, n_bins=None, seed=0, noise=0.02):
    """(b, y, atoms, lo, hi, (n_bins, bin_of, bin_value)): parameter k takes n_bins[k] evenly spaced values inside its bounds and
    every atom a random one of them (a non-Cartesian atom list: some bins stay empty); a parameter without bins takes uniform
    values; signals of uniform truth values with additive Gaussian noise."""
    n_bins = MID[model] if n_bins is None else n_bins
    rng = np.random.default_rng(1000 * seed + 7 * n_vox + 3 * n_atoms + n_b + 11 * sum(n_bins))
    names = api.MODEL_PARAM_NAMES[model]
    lo = np.array([BOUNDS[n][0] for n in names])
    hi = np.array([BOUNDS[n][1] for n in names])
    atoms = np.ascontiguousarray(rng.uniform(lo[:, None], hi[:, None], (len(names), n_atoms)))
    bin_of = np.zeros((len(names), n_atoms), np.int32)
    values = []
    for k, nb in enumerate(n_bins):
        if nb:
            val = lo[k] + (hi[k] - lo[k]) * (np.arange(nb) + 1.0) / (nb + 1.0)
            bin_of[k] = rng.integers(0, nb, n_atoms)
            atoms[k] = val[bin_of[k]]
            values.append(val)
    truth = np.stack([rng.uniform(*TRUTH[n], n_vox) for n in names])
    b = synth.bvalues(n_b)
    y = signals(model, b, truth)
    y = np.ascontiguousarray(y + noise * rng.standard_normal(y.shape))
    return b, y, atoms, lo, hi, (np.array(n_bins, np.int32), bin_of, np.concatenate(values))


def _run(gpu, model, case, project=False, noise_sd=0.0, log_prior=None, probs=PROBS, **kw):
    b, y, atoms, lo, hi, bins = case
    got = gpu.grid_marginals(model, b, y, atoms, lo, hi, log_prior=log_prior, noise_sd=noise_sd, bins=bins, quantiles=probs,
                             project_amplitude=project, **kw)
    ref = reference(model, b, y, atoms, lo, hi, *bins, probs=probs, log_prior=log_prior, noise_sd=noise_sd, project=project, **kw)
    worst = accept(ref, got, bins[0], bins[2], probs)
    print(f"{model} n_vox={len(y)} G={atoms.shape[1]} n_b={len(b)} B={int(bins[0].sum())} noise_sd={noise_sd}: error / bound = {worst:.3g}")
    return got, ref


def _both_modes(gpu, model, case, **kw):
    _run(gpu, model, case, noise_sd=0.0, **kw)
    return _run(gpu, model, case, noise_sd=NOISE_SD, **kw)


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- against numpy: tile edges of each axis crossed with mid values of the others
@pytest.mark.parametrize("model,project", PROJ)
@pytest.mark.parametrize("n_vox", [1, 15, 16, 17, 65])
def test_voxel_axis(gpu, n_vox, model, project):
    _both_modes(gpu, model, _case(model, n_vox, 33, 16), project=project)


@pytest.mark.parametrize("model,project", PROJ)
def test_more_voxel_groups_than_blocks(gpu, model, project):
    """2 x CUs blocks of 64 voxels and 69 voxels more: the first blocks go round their loop twice, the last group is partly filled."""
    n_vox = 2 * _cus() * 64 + 69
    _run(gpu, model, _case(model, n_vox, 48, 8), project=project, noise_sd=NOISE_SD if project else 0.0)


@pytest.mark.parametrize("model,project", PROJ)
@pytest.mark.parametrize("n_atoms", [1, 15, 16, 17, "slab + 16"])
def test_atom_axis(gpu, n_atoms, model, project):
    """The last: two slabs, the second partly filled (api.grid_prior_slab_atoms: the slab of both passes)."""
    if n_atoms == "slab + 16":
        n_atoms = api.grid_prior_slab_atoms(32) + 16
    _both_modes(gpu, model, _case(model, 65, n_atoms, 32), project=project)


@pytest.mark.parametrize("n_b", [1, 4, 5, 32, 33, 64, 65, 128])  # 33 and up take the larger instantiation; 1, 5 and 65 pad the k-steps
def test_b_axis(gpu, n_b):
    _both_modes(gpu, "tri_reduced", _case("tri_reduced", 65, 33, n_b))


@pytest.mark.parametrize("n_b", [4, 5, 32, 33, 65, 128])
def test_b_axis_projected(gpu, n_b):
    _both_modes(gpu, "bi_s0", _case("bi_s0", 65, 33, n_b), project=True)


BINS = {  # label -> n_bins for tri_reduced (5 free parameters) and bi_s0 (3 and the projected S0)
    "B=1": ((0, 0, 1, 0, 0), (0, 1, 0, 0)),
    "B=16": ((16, 0, 0, 0, 0), (0, 0, 16, 0)),
    "B=17, a second chunk": ((9, 8, 0, 0, 0), (16, 1, 0, 0)),
    "B=33, a third chunk and the next instantiation": ((11, 11, 11, 0, 0), (11, 11, 11, 0)),
    "B=65, the widest instantiation": ((13, 13, 13, 13, 13), (30, 5, 30, 0)),
    "B=128, the cap": ((26, 26, 26, 25, 25), (43, 43, 42, 0)),
    "a parameter astride a chunk boundary": ((10, 10, 0, 0, 0), (0, 12, 10, 0)),
    "n_bins = 0 in the middle": ((5, 0, 7, 0, 3), (5, 0, 7, 0)),
}


@pytest.mark.parametrize("k,model,project", [(0, "tri_reduced", False), (1, "bi_s0", True)])
@pytest.mark.parametrize("label", list(BINS))
def test_bin_axis(gpu, label, k, model, project):
    n_bins = BINS[label][k]
    _both_modes(gpu, model, _case(model, 65, 300 if sum(n_bins) > 64 else 100, 16, n_bins), project=project)


def test_sigma_vector(gpu):
    sigma = np.linspace(0.5, 3.0, 16)
    _both_modes(gpu, "tri_reduced", _case("tri_reduced", 65, 33, 16), sigma=sigma)
    _both_modes(gpu, "bi_s0", _case("bi_s0", 65, 33, 16), project=True, sigma=sigma)


@pytest.mark.parametrize("model,project", PROJ)
def test_excluded_atoms_weigh_exactly_nothing(gpu, model, project):
    """A third of the atoms at log_prior = -inf, among them every atom of bin 0 of the first parameter: that bin is exactly 0.0."""
    case = _case(model, 65, 100, 16)
    bin_of = case[5][1]
    rng = np.random.default_rng(3)
    lp = np.log(rng.uniform(0.01, 1.0, 100)) + 2.5  # not normalised
    lp[rng.random(100) < 1 / 3] = -np.inf
    lp[bin_of[0] == 0] = -np.inf
    assert (bin_of[0] == 0).any() and np.isfinite(lp).sum() > 20
    for noise_sd in (0.0, NOISE_SD):
        got, ref = _run(gpu, model, case, project=project, noise_sd=noise_sd, log_prior=lp)
        assert (got["marginal"][0][0] == 0.0).all() and not np.signbit(got["marginal"][0][0]).any()
        assert (got["marginal"][0][1:].sum(axis=0) > 0.99).all()


@pytest.mark.parametrize("model,project", PROJ)
def test_a_non_finite_voxel_between_finite_ones(gpu, model, project):
    """A NaN and an Inf voxel in the middle of a strip: NaN in every output of theirs, their neighbours as the reference has them."""
    b, y, atoms, lo, hi, bins = _case(model, 64, 33, 16)
    y = y.copy()
    y[21, 5] = np.nan
    y[38, 0] = np.inf
    got, ref = _both_modes(gpu, model, (b, y, atoms, lo, hi, bins), project=project)
    assert (~ref["finite"]).sum() == 2 and np.isnan(got["log_evidence"][[21, 38]]).all() and np.isfinite(got["log_evidence"][[20, 22, 37, 39]]).all()
    for k in got["marginal"]:
        assert np.isnan(got["marginal"][k][:, [21, 38]]).all() and np.isnan(got["quantiles"][k][:, [21, 38]]).all()


# ---- what ties it to the posterior
@pytest.mark.parametrize("model,project", PROJ)
@pytest.mark.parametrize("noise_sd", [0.0, NOISE_SD])
def test_first_moment_and_evidence_are_the_posteriors(gpu, model, project, noise_sd):
    """sum_j marginal_k[j] value_j is grid_posterior's mean[k] within the sum of the two bounds; log_evidence within its bound."""
    case = _case(model, 65, 100, 16, tuple(7 if n else 0 for n in MID[model]))
    b, y, atoms, lo, hi, bins = case
    got, ref = _run(gpu, model, case, project=project, noise_sd=noise_sd)
    post = gpu.grid_posterior(model, b, y, atoms, lo, hi, noise_sd=noise_sd, project_amplitude=project)
    err = np.abs(got["log_evidence"] - post["log_evidence"])
    assert (err <= ref["bound_log_evidence"]).all(), (err / ref["bound_log_evidence"]).max()
    off = np.concatenate([[0], np.cumsum(bins[0])])
    for k, m in got["marginal"].items():
        first = got["values"][k] @ m
        bound = ref["post"]["bound_mean"][:, k] + ref["bound"][:, off[k]:off[k + 1]] @ np.abs(got["values"][k])
        err = np.abs(first - post["mean"][k])
        print(f"parameter {k}: first moment against the posterior's mean, error / bound = {(err / bound).max():.3g}")
        assert (err <= bound).all()


def test_reproducible_and_the_same_from_device_memory(gpu):
    """Two calls return the same bytes; so does the call on device tensors; so does a call on a part of the voxels: a voxel's sums
    depend on the order of the atoms only."""
    import torch

    for model, project, n_b in (("tri_reduced", False, 33), ("bi_s0", True, 16)):
        b, y, atoms, lo, hi, bins = _case(model, 1000, 100, n_b)
        kw = dict(noise_sd=NOISE_SD, bins=bins, quantiles=PROBS, project_amplitude=project)
        one = gpu.grid_marginals(model, b, y, atoms, lo, hi, **kw)
        two = gpu.grid_marginals(model, b, y, atoms, lo, hi, **kw)
        part = gpu.grid_marginals(model, b, y[:83], atoms, lo, hi, **kw)
        dev = torch.device("cuda", 0)
        n, B = len(y), int(bins[0].sum())
        yd = torch.from_numpy(y).to(dev)
        md = torch.full((B, n), 7.0, dtype=torch.float64, device=dev)
        qd = torch.full((len(PROBS), atoms.shape[0], n), 7.0, dtype=torch.float64, device=dev)
        ed = torch.full((n,), 7.0, dtype=torch.float64, device=dev)
        o = api.make_opts(model, len(b), jac="analytic")
        three = api.grid_marginals_device(o, n, b, yd, atoms, None, lo, hi, project, None, NOISE_SD, *bins, PROBS, md, qd, ed, 0,
                                          torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        assert one["log_evidence"].tobytes() == two["log_evidence"].tobytes() == ed.cpu().numpy().tobytes()
        assert one["log_evidence"][:83].tobytes() == part["log_evidence"].tobytes()
        assert sorted(three["marginal"]) == sorted(one["marginal"])
        for k in one["marginal"]:
            assert one["marginal"][k].tobytes() == two["marginal"][k].tobytes() == three["marginal"][k].cpu().numpy().tobytes()
            assert one["quantiles"][k].tobytes() == two["quantiles"][k].tobytes() == three["quantiles"][k].cpu().contiguous().numpy().tobytes()
            assert np.ascontiguousarray(one["marginal"][k][:, :83]).tobytes() == part["marginal"][k].tobytes()
            assert np.ascontiguousarray(one["quantiles"][k][:, :83]).tobytes() == part["quantiles"][k].tobytes()
        none = [k for k, nb in enumerate(bins[0]) if not nb]
        assert torch.isnan(qd[:, none]).all()  # a parameter without a marginal: NaN quantiles


def test_the_median_of_two_equal_atoms_is_the_lower_value(gpu):
    """Symmetric by construction: the mono-exponential model at the single b-value 0, where both atoms (S0 = 1, two values of D)
    predict exactly 1 and the signal is exactly 1, so both l_g are exactly 0 and the weights are equal.  The level 0.5 is reached at
    the first bin -- its weight exp(-log 2) is 0.5 -- and the lower value is reported; 0.6 is reached at the second."""
    atoms = np.array([[1.0, 1.0], [0.05, 0.01]])  # the higher D first: the bins ascend, not the atoms
    lo, hi = np.array([0.5, 1e-5]), np.array([2.0, 0.1])
    y = np.ones((17, 1))
    got = gpu.grid_marginals("mono", np.zeros(1), y, atoms, lo, hi, noise_sd=0.5, quantiles=[0.5, 0.6, 0.4])
    assert got["values"][1].tolist() == [0.01, 0.05] and got["values"][0].tolist() == [1.0]
    assert (np.abs(got["marginal"][0] - 1.0) <= 4 * U).all()
    assert (np.abs(got["marginal"][1] - 0.5) <= 2 * U).all() and (got["marginal"][1][0] == got["marginal"][1][1]).all()
    assert (got["quantiles"][1][0] == 0.01).all() and (got["quantiles"][1][1] == 0.05).all() and (got["quantiles"][1][2] == 0.01).all()
    assert (np.abs(got["log_evidence"]) <= 2 * U).all()  # L = log 2, less the log 2 of the uniform prior's normaliser


# ---- through the plugin
@functools.lru_cache(maxsize=None)
def _population():
    return population(1000, seed=0)


def test_through_the_solver(gpu):
    b, y, _, grid, atoms, lo, hi = _population()
    names = ["f1", "D1", "D2", "S0"]
    bounds = {n: (float(lo[i]), float(hi[i])) for i, n in enumerate(names)}
    mk = lambda **kw: HipBayesGridSolver(BiExpModel(fit_s0=True), grid, p0={"S0": 1.0}, bounds=bounds, noise_sd=0.05, **kw)
    today = {"posterior_sd", "map", "map_atom", "log_evidence", "ess", "n_pixels"}
    s = mk(marginals={"quantiles": [0.05, 0.5, 0.95, 0.99]}).fit(b, y)
    d = s.diagnostics_
    assert set(d) == today | {"marginal", "marginal_values", "quantiles", "quantile_probs"}
    assert s.project is True and list(d["marginal"]) == ["f1", "D1", "D2"] == list(d["marginal_values"]) == list(d["quantiles"])  # no S0
    want = gpu.grid_marginals("bi_s0", b, y, atoms, lo, hi, noise_sd=0.05, project_amplitude=True, quantiles=[0.05, 0.5, 0.95, 0.99])
    assert d["quantile_probs"].tolist() == [0.05, 0.5, 0.95, 0.99]
    for k, n in enumerate(names[:3]):
        assert d["marginal"][n].shape == (len(grid[n]), 1000) and d["quantiles"][n].shape == (4, 1000)
        assert d["marginal_values"][n].tobytes() == np.sort(np.asarray(grid[n], float)).tobytes()
        assert d["marginal"][n].tobytes() == want["marginal"][k].tobytes() and d["quantiles"][n].tobytes() == want["quantiles"][k].tobytes()
        assert (np.diff(d["quantiles"][n], axis=0) >= 0).all()  # the levels ascend, so do their quantiles
        assert np.isin(d["quantiles"][n], grid[n]).all()
    # True: the three default levels; the posterior itself is untouched
    t = mk(marginals=True).fit(b, y)
    assert t.diagnostics_["quantile_probs"].tolist() == [0.025, 0.5, 0.975] and t.diagnostics_["quantiles"]["D1"].shape == (3, 1000)
    off = mk(marginals=None).fit(b, y)
    assert set(off.diagnostics_) == today
    for n in names:
        assert np.asarray(off.params_[n]).tobytes() == np.asarray(s.params_[n]).tobytes() == np.asarray(t.params_[n]).tobytes()
    assert off.diagnostics_["log_evidence"].tobytes() == d["log_evidence"].tobytes()
    # with the learned prior: the marginals are taken under the learned table
    e = mk(empirical_prior={"n_iter": 5}, marginals=True).fit(b, y)
    assert set(e.diagnostics_) == today | {"marginal", "marginal_values", "quantiles", "quantile_probs", "log_prior", "prior_loglik",
                                           "prior_n_iter", "prior_n_voxels"}
    under = gpu.grid_marginals("bi_s0", b, y, atoms, lo, hi, noise_sd=0.05, project_amplitude=True, log_prior=e.diagnostics_["log_prior"])
    for k, n in enumerate(names[:3]):
        assert e.diagnostics_["marginal"][n].tobytes() == under["marginal"][k].tobytes()
        assert e.diagnostics_["marginal"][n].tobytes() != t.diagnostics_["marginal"][n].tobytes()

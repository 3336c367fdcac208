"""pnx_curvefit_varpro_marginals_f64 on the GPU against the numpy restatement (tests/varpro_marginal_reference.py): every axis of the
kernel (voxels, atoms, b-values, bins), every layout in both noise modes and with both amplitude weights, a free T1 with bins, a
sigma vector, the running maximum (excluded tiles in front and in the middle, the best atom last so that every tile rescales, far
atoms that underflow to exactly 0), exact zeros, non-finite voxels, the narrow box, the posterior's own mean and evidence as a
second kernel, bit identity (two calls, host against device memory, a prefix of the voxels), the median of two equal weights and
the plugin class.  The inputs are tests/varpro_marginal_cases.py's, by name.

Acceptance per voxel (varpro_marginal_reference.accept, derivation there and in DESIGN.md 4.1l): every bin of every case on every
voxel within (expm1(2 eps_v) + 3 gamma_G) ref + 1e-300, the bins of a parameter summing to 1 within the same relative bound, bins
without an admissible atom exactly 0, every quantile a bin the reference's running sum can cross the level at, log geo_mean and
log_evidence within their bounds.  The reference asserts its own preconditions (eps_v <= 1e-6; 1e-3, explicit, in the narrow box
only), which tests/test_varpro_marginals_host.py also runs on the CPU for the inputs used here.

Largest error-to-bound ratios measured on an MI355X: DESIGN.md 4.1l."""
from __future__ import annotations

import numpy as np
import pytest
from varpro_marginal_cases import NOISE_SD, call_kw, cases, ref_kw
from varpro_marginal_reference import U, accept, reference
from varpro_posterior_reference import wide_box
from varpro_reference import case_atoms, case_signals

from pyneapple_amd import api
from pyneapple_amd.models import TriExpModel
from pyneapple_amd.solvers import HipBayesVarProSolver

pytestmark = pytest.mark.gpu

PROBS = (0.025, 0.5, 0.975)
CASES = cases()


def _bins(case):
    o = api.make_opts(case["model"], len(case["b"]), case["kw"].get("fixed_idx", ()), t1_mode=case["kw"].get("t1_mode", 0))
    return api._varpro_marginal_bins(o, case["model"], case["atoms"], None)


def _run(gpu, case, y=None, probs=PROBS):
    return gpu.varpro_marginals(case["model"], case["b"], case["y"] if y is None else y, case["atoms"], case["lo"], case["hi"], quantiles=probs,
                                **call_kw(case))


def _check(gpu, case, y=None, probs=PROBS):
    n_bins, bin_of, bin_value = _bins(case)
    got = _run(gpu, case, y, probs)
    ref = reference(case["model"], case["b"], case["y"] if y is None else y, case["atoms"], case["lo"], case["hi"], n_bins, bin_of, bin_value,
                    probs=probs, **ref_kw(case))
    accept(ref, got, n_bins, bin_value, probs)
    return got, ref


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_against_the_reference(gpu, name):
    got, ref = _check(gpu, CASES[name])
    if name == "first-tile-excluded":  # D1's first grid value holds excluded atoms only: exactly 0.0, not a rounded residue
        assert ref["empty"][0] and (got["marginal"][1][0] == 0.0).all() and not np.signbit(got["marginal"][1][0]).any()
    if name == "far-atoms-underflow":
        assert ((got["marginal"][1] == 0.0) & ~ref["empty"][:, None]).any()
    if name == "narrow-box":
        assert ref["post"]["clipped_mass"].mean() > 0.5


def test_non_finite_voxels_leave_their_neighbours_bit_identical(gpu):
    case = CASES["layout-tri_s0-a"]
    clean = _run(gpu, case)
    bad = case["y"].copy()
    bad[3, 5], bad[16, 0], bad[33, 31], bad[69, 7] = np.nan, np.inf, -np.inf, np.nan
    got, ref = _check(gpu, case, y=bad)  # accept() checks the NaN rows
    where = np.array([3, 16, 33, 69])
    assert (~ref["finite"]).nonzero()[0].tolist() == where.tolist()
    rest = np.setdiff1d(np.arange(70), where)
    assert np.isnan(got["log_evidence"][where]).all() and got["log_evidence"][rest].tobytes() == clean["log_evidence"][rest].tobytes()
    for key in ("marginal", "quantiles", "geo_mean"):
        for k in got[key]:
            assert np.isnan(got[key][k][..., where]).all(), key
            assert np.ascontiguousarray(got[key][k][..., rest]).tobytes() == np.ascontiguousarray(clean[key][k][..., rest]).tobytes(), key


@pytest.mark.parametrize("name", ["layout-tri_s0-a", "layout-bi_reduced-b", "free-t1", "sigma"])
def test_mean_and_evidence_agree_with_the_posterior_kernel(gpu, name):
    """Two kernels over the same weights: sum_j marginal_k[j] value_j is the posterior mean of a rate, and log_evidence is the
    posterior's.  The allowed difference is the sum of the two references' bounds (the mean's: the bins' bounds times |value_j|,
    plus the rounding of a sum of n_bins terms)."""
    case = CASES[name]
    got, ref = _check(gpu, case)
    post = gpu.varpro_posterior(case["model"], case["b"], case["y"], case["atoms"], case["lo"], case["hi"], **call_kw(case))
    n_bins, _, bin_value = _bins(case)
    off = np.concatenate([[0], np.cumsum(n_bins)])
    for k, m in got["marginal"].items():
        val = bin_value[off[k]:off[k + 1]]
        bound = ref["post"]["bound_mean"][:, k] + (ref["bound"][:, off[k]:off[k + 1]] * np.abs(val)).sum(axis=1) + 4 * (len(val) + 16) * U * np.abs(val).max()
        assert (np.abs(val @ m - post["mean"][k]) <= bound).all(), f"parameter {k}"
    assert (np.abs(got["log_evidence"] - post["log_evidence"]) <= ref["bound_log_evidence"] + ref["post"]["bound_log_evidence"]).all()


def test_two_calls_host_and_device_memory_and_a_prefix_return_the_same_bytes(gpu):
    import torch

    n_vox = 1000
    b, y = case_signals("tri_s0", n_vox)
    atoms = case_atoms("tri_s0")
    lo, hi = wide_box("tri_s0")
    lp = np.log(np.random.default_rng(9).uniform(0.05, 1.0, 64))
    kw = dict(log_prior=lp, noise_sd=NOISE_SD)
    host = gpu.varpro_marginals("tri_s0", b, y, atoms, lo, hi, quantiles=PROBS, **kw)
    again = gpu.varpro_marginals("tri_s0", b, y, atoms, lo, hi, quantiles=PROBS, **kw)
    part = gpu.varpro_marginals("tri_s0", b, y[:83], atoms, lo, hi, quantiles=PROBS, **kw)
    o = api.make_opts("tri_s0", 32, jac="analytic")
    n_bins, bin_of, bin_value = api._varpro_marginal_bins(o, "tri_s0", atoms, None)
    dev = torch.device("cuda", 0)
    yd = torch.from_numpy(y).to(dev)
    f = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    marginal, quantile, geo, logev = f(int(n_bins.sum()), n_vox), f(3, 6, n_vox), f(6, n_vox), f(n_vox)
    st = torch.cuda.current_stream(dev).cuda_stream
    res = api.varpro_marginals_device(o, n_vox, b, yd, atoms, None, lo, hi, lp, NOISE_SD, True, n_bins, bin_of, bin_value, PROBS, marginal,
                                      quantile, geo, logev, 0, st)
    torch.cuda.synchronize()
    assert host["log_evidence"].tobytes() == again["log_evidence"].tobytes() == logev.cpu().numpy().tobytes()
    assert host["log_evidence"][:83].tobytes() == part["log_evidence"].tobytes()
    assert sorted(res["marginal"]) == sorted(host["marginal"]) == [1, 3, 4]
    for key in ("marginal", "quantiles", "geo_mean"):
        for k in host[key]:
            h = np.ascontiguousarray(host[key][k])
            assert h.tobytes() == np.ascontiguousarray(again[key][k]).tobytes(), key
            assert h.tobytes() == res[key][k].cpu().numpy().tobytes(), key
            assert np.ascontiguousarray(h[..., :83]).tobytes() == np.ascontiguousarray(part[key][k]).tobytes(), key
    only = f(int(n_bins.sum()), n_vox).zero_()  # every output but the marginal is optional
    api.varpro_marginals_device(o, n_vox, b, yd, atoms, None, lo, hi, lp, NOISE_SD, True, n_bins, bin_of, bin_value, (), only, None, None, None, 0, st)
    torch.cuda.synchronize()
    assert only.cpu().numpy().tobytes() == marginal.cpu().numpy().tobytes()


def test_the_median_of_two_equal_weights_is_the_lower_value(gpu):
    """mono with a free T1 (t1_mode 1: the factor 1 - exp(-TR / T1)) at TR = 3000 and T1 = 1 or 2: exp(-1500) is 0, the factor of both
    atoms is exactly 1, their columns and so their weights are the same bits: each T1 bin holds exactly 0.5, and the running sum
    reaches the level 0.5 at the first."""
    b, y = case_signals("mono", 33)
    atoms = np.array([[2e-3, 2e-3], [1.0, 2.0]])
    lo, hi = np.array([0.0, 1e-5, 0.5]), np.array([10.0, 0.5, 5000.0])
    got = gpu.varpro_marginals("mono", b, y, atoms, lo, hi, quantiles=(0.5, 0.5000000001), t1_mode=1, tr=3000.0)
    assert (got["marginal"][2] == 0.5).all() and (got["marginal"][1] == 1.0).all()
    assert (got["quantiles"][2][0] == 1.0).all() and (got["quantiles"][2][1] == 2.0).all()
    assert (got["quantiles"][1] == 2e-3).all()
    # exp(log v): the rounding of the logarithm (|log 2e-3| = 6.2 times 2^-53) and an ulp or two of exp and of the host's log
    np.testing.assert_allclose(got["geo_mean"][1], 2e-3, rtol=16 * U)
    np.testing.assert_allclose(got["geo_mean"][2], np.sqrt(2.0), rtol=16 * U)


# ---- through the plugin interface
BOUNDS = {"f1": (-40.0, 40.0), "D1": (1e-5, 0.5), "f2": (-40.0, 40.0), "D2": (1e-5, 0.5), "D3": (1e-5, 0.5), "S0": (0.0, 10.0)}  # wide_box
P0 = {"f1": 0.2, "D1": 0.1, "f2": 0.3, "D2": 0.01, "D3": 0.001, "S0": 1.0}
TRI = {"D1": list(np.geomspace(0.04, 0.3, 4)), "D2": list(np.geomspace(4e-3, 0.02, 4)), "D3": list(np.geomspace(3e-4, 1.5e-3, 4))}
NAMES = api.MODEL_PARAM_NAMES["tri_s0"]


def test_hip_bayes_varpro_marginals_through_the_plugin_interface(gpu):
    b, y = case_signals("tri_s0", 200)
    y[7, 3] = np.nan
    mk = lambda **kw: HipBayesVarProSolver(TriExpModel(fit_s0=True), TRI, max_iter=250, tol=1e-8, p0=P0, bounds=BOUNDS, noise_sd=NOISE_SD, **kw)
    plain, s = mk().fit(b, y), mk(marginals={"quantiles": [0.1, 0.9]}).fit(b, y)
    lo, hi = (np.array([BOUNDS[n][i] for n in NAMES]) for i in (0, 1))
    got = gpu.varpro_marginals("tri_s0", b, y, s._nl_atoms, lo, hi, noise_sd=NOISE_SD, quantiles=(0.1, 0.9))
    extra = {"marginal", "marginal_values", "quantiles", "quantile_probs", "geo_mean"}
    assert set(s.diagnostics_) == set(plain.diagnostics_) | extra and not extra & set(plain.diagnostics_)
    for n in NAMES:  # what the solver reported before is the same bytes
        assert np.asarray(s.params_[n]).tobytes() == np.asarray(plain.params_[n]).tobytes()
    assert s.diagnostics_["log_evidence"].tobytes() == plain.diagnostics_["log_evidence"].tobytes()
    assert s.diagnostics_["quantile_probs"].tolist() == [0.1, 0.9]
    for key, mine in (("marginal", "marginal"), ("marginal_values", "values"), ("quantiles", "quantiles"), ("geo_mean", "geo_mean")):
        assert sorted(s.diagnostics_[key]) == ["D1", "D2", "D3"]
        for k, n in ((1, "D1"), (3, "D2"), (4, "D3")):
            assert np.ascontiguousarray(s.diagnostics_[key][n]).tobytes() == np.ascontiguousarray(got[mine][k]).tobytes(), key
    assert np.isnan(s.diagnostics_["geo_mean"]["D1"][7]) and np.isnan(s.diagnostics_["marginal"]["D2"][:, 7]).all()
    q = s.diagnostics_["quantiles"]["D1"]
    fin = np.arange(200) != 7
    assert (q[0, fin] <= q[1, fin]).all() and (s.diagnostics_["geo_mean"]["D1"][fin] <= s.params_["D1"][fin] * (1 + 1e-12)).all()  # AM >= GM

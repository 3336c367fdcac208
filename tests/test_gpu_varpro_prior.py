"""pnx_curvefit_varpro_prior_em_f64 on the device against tests/varpro_prior_reference.py (the numpy EM of
tests/grid_prior_reference.py on the variable-projection posterior reference's l_g): one update at the tile edges of every axis
(the inputs: tests/varpro_prior_cases.py, whose preconditions tests/test_varpro_prior_host.py checks on the CPU), inadmissible
atoms, voxels that take no part, three updates, a long run checked step by step, the properties of an EM, what the learned prior
is worth, and HipBayesVarProSolver's empirical_prior end to end.

Acceptance of one update (grid_prior_reference.step_bounds with varpro_posterior_reference's eps_v, derivation in DESIGN.md 4.1m):
the library's l_g differs from the reference's by at most eps_v, so a normalised weight moves by e^{+-2 eps_v}; sums over G atoms
and N voxels add gamma_G and gamma_N; log_prior after the update is held to log1p of that, the log-likelihood to the sum of the
posterior's log-evidence bounds.  After t <= 3 updates the bound against an all-numpy run is (2^t - 1) single-step bounds; a long
run is checked one step at a time against the library's own previous prior.

n_b = K + 1 at K = 2, 3 is left out for 4.1l's reason (tests/varpro_prior_cases.py states it).  The largest error-to-bound ratios
observed are recorded in DESIGN.md 4.1m."""
from __future__ import annotations

import functools

import numpy as np
import pytest
from grid_posterior_reference import U
from varpro_prior_cases import call_kw, cases, ref_kw
from varpro_prior_reference import accept_step, em_step, likelihoods, normalise, population, step_bounds
from varpro_reference import case_signals

from pyneapple_amd import api
from pyneapple_amd.models import BiExpModel
from pyneapple_amd.solvers import HipBayesVarProSolver

pytestmark = pytest.mark.gpu

CASES = cases()


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
            last = (lp_next, S)
            lp = lp_next
    q = accept_step(got["log_prior"], lp0, last[0], last[1], n, drift, alpha)
    print(f"log_prior: error / bound = {q:.3g} after {steps} update(s); loglik worst {worst:.3g}")
    return q


def _run(gpu, c, steps=1, alpha=0.0):
    got = gpu.varpro_prior_em(c["model"], c["b"], c["y"], c["atoms"], c["lo"], c["hi"], n_iter=steps, pseudo_count=alpha, rel_tol=0.0, **call_kw(c))
    l0, eps0, fin = likelihoods(c["model"], c["b"], c["y"], c["atoms"], c["lo"], c["hi"], **ref_kw(c))
    lp0 = normalise(c["kw"].get("log_prior"), c["atoms"].shape[1])
    _accept(got, l0, eps0, fin, lp0, alpha, steps)
    lp = got["log_prior"]
    adm = lp > -np.inf
    total = np.log(np.exp(lp[adm] - lp[adm].max()).sum()) + lp[adm].max()
    # the table sums to 1 over its finite entries: every S_g is within `rel` of the exact sum of exact weights, which sum to n
    rel = step_bounds(l0, lp0, eps0, fin, em_step(l0, lp0, fin, alpha)[0])["lp"]
    assert abs(total) <= 2 ** steps * rel + 4 * (len(lp) + 16) * U, total
    assert (lp[np.isinf(lp0)] == -np.inf).all()
    return got


# ---- one update against numpy: the voxel, atom and b axes, the seven layouts, both noise modes, both amplitude weights, a sigma
# vector, a free T1, excluded tiles, the narrow box
@pytest.mark.parametrize("name", sorted(CASES))
def test_one_update(gpu, name):
    _run(gpu, CASES[name])


def test_excluded_atoms_with_a_pseudo_count(gpu):
    for name in ("first-tile-excluded", "middle-tile-excluded"):
        c = CASES[name]
        got = _run(gpu, c, alpha=0.25)
        assert (np.isinf(got["log_prior"]) == np.isinf(c["kw"]["log_prior"])).all()


def _singular_case(marginal):
    """bi_s0, 32 b-values from 0 to 1000, the 28 pairs of the case dictionary and two atoms whose rates (60, 40) and (90, 70) differ
    but whose columns are both exactly (1, 0, 0, ...): exp(-32 D) underflows to 0.  N is exactly singular: the variable projection's
    a_hat = 0 atoms."""
    from varpro_posterior_reference import wide_box
    from varpro_reference import case_atoms

    b, y = case_signals("bi_s0", 70)
    lo, hi = wide_box("bi_s0")
    hi[[1, 2]] = 100.0
    good = case_atoms("bi_s0")
    atoms = np.ascontiguousarray(np.concatenate([good[:, :5], [[60.0], [40.0]], good[:, 5:], [[90.0], [70.0]]], axis=1))
    return dict(model="bi_s0", b=b, y=y, atoms=atoms, lo=lo, hi=hi, noise_sd=0.0, marginal=marginal, max_eps=1e-6, kw={}), [5, 29], good


def test_an_atom_with_a_singular_n_is_inadmissible_when_the_amplitudes_are_marginalised(gpu):
    c, sing, good = _singular_case(True)
    got = gpu.varpro_prior_em(c["model"], c["b"], c["y"], c["atoms"], c["lo"], c["hi"], n_iter=1, rel_tol=0.0, pseudo_count=0.5, **call_kw(c))
    lp = got["log_prior"]
    rest = np.setdiff1d(np.arange(30), sing)
    assert (lp[sing] == -np.inf).all() and np.isfinite(lp[rest]).all() and got["n_eff"] == 70
    assert abs(np.exp(lp[rest]).sum() - 1.0) <= 1e-12
    # the reference on the dictionary without them, from the start the library used: uniform over all 30 atoms, n_adm = 28
    l0, eps0, fin = likelihoods(c["model"], c["b"], c["y"], good, c["lo"], c["hi"], **ref_kw(c))
    lp0 = np.full(28, -np.log(30.0))
    S, lp_next, ll = em_step(l0, lp0, fin, 0.5)
    bd = step_bounds(l0, lp0, eps0, fin, S)
    accept_step(lp[rest], lp0, lp_next, S, 70, bd["lp"], 0.5)
    assert abs(got["loglik"][0] - ll) <= bd["loglik"]
    # with the profile weight the same atoms are admissible: a_hat = 0, a finite cost, a finite weight
    c0, _, _ = _singular_case(False)
    got0 = gpu.varpro_prior_em(c0["model"], c0["b"], c0["y"], c0["atoms"], c0["lo"], c0["hi"], n_iter=1, rel_tol=0.0, pseudo_count=0.5, **call_kw(c0))
    assert np.isfinite(got0["log_prior"]).all() and abs(np.exp(got0["log_prior"]).sum() - 1.0) <= 1e-12
    assert (got0["log_prior"] >= np.log(0.5 / (70 + 0.5 * 30)) - 1e-12).all()


def test_non_finite_voxels_take_no_part(gpu):
    """A NaN and an Inf voxel in the middle of a strip: not counted, and the result is the reference's without them.  At the end of
    the array (same launch grid, the same lanes for everyone else) the table is bit-identical to the run without them."""
    c = dict(CASES["voxels-65"])
    y = np.ascontiguousarray(c["y"][:64]).copy()
    y[21, 5] = np.nan
    y[38, 0] = np.inf
    c["y"] = y
    got = _run(gpu, c)
    assert got["n_eff"] == 62 and np.isfinite(got["loglik"]).all()
    tail = np.ascontiguousarray(CASES["voxels-65"]["y"][:64]).copy()
    tail[62] = np.nan
    tail[63, 3] = -np.inf
    a = dict(model=c["model"], b=c["b"], nl_atoms=c["atoms"], lo=c["lo"], hi=c["hi"], n_iter=3, rel_tol=0.0, **call_kw(c))
    with_them = gpu.varpro_prior_em(y=tail, **a)
    without = gpu.varpro_prior_em(y=np.ascontiguousarray(tail[:62]), **a)
    assert with_them["n_eff"] == without["n_eff"] == 62
    assert with_them["log_prior"].tobytes() == without["log_prior"].tobytes() and with_them["loglik"].tobytes() == without["loglik"].tobytes()
    none = gpu.varpro_prior_em(y=np.full((5, 32), np.nan), **a)
    assert none["n_eff"] == 0 and none["n_iter"] == 0 and none["loglik"][0] == 0.0 and np.isnan(none["loglik"][1:]).all()
    assert none["log_prior"].tobytes() == normalise(None, c["atoms"].shape[1]).tobytes()


# ---- more than one update
@pytest.mark.parametrize("noise_sd", [0.0, 0.02])
def test_three_updates_against_numpy(gpu, noise_sd):
    from varpro_marginal_cases import _case

    _run(gpu, _case("tri_s0", 300, noise_sd=noise_sd), steps=3)
    _run(gpu, _case("bi_reduced", 300, noise_sd=noise_sd, marginal=False), steps=3)


@functools.lru_cache(maxsize=None)
def _population():
    """varpro_prior_reference.population (seed 0, 1000 voxels, 91 atoms) and its box with the fraction in [-40, 40]: no pair clips,
    so eps_v stays under 1e-6 (2e-8; in the [0, 1] box 1.2e-6 with the noise marginalised) and the derived bounds apply."""
    b, y, truth, atoms, lo, hi = population(1000, seed=0)
    wlo, whi = lo.copy(), hi.copy()
    wlo[0], whi[0] = -40.0, 40.0
    return b, y, truth, atoms, lo, hi, wlo, whi


@pytest.mark.parametrize("noise_sd", [0.0, 0.05])
def test_step_consistency_and_properties_of_a_long_run(gpu, noise_sd):
    """The library is deterministic: its 20-update run repeats its 19-update run bit for bit and adds one update, which numpy
    reproduces from the 19-update table within the single-step bound.  loglik never falls by more than its bound, and loglik[done]
    is the sum of the posterior's log_evidence under the returned table."""
    import torch

    b, y, _, atoms, _, _, lo, hi = _population()
    kw = dict(noise_sd=noise_sd, rel_tol=0.0)
    r19 = gpu.varpro_prior_em("bi_s0", b, y, atoms, lo, hi, n_iter=19, **kw)
    r20 = gpu.varpro_prior_em("bi_s0", b, y, atoms, lo, hi, n_iter=20, **kw)
    assert r19["n_iter"] == 19 and r20["n_iter"] == 20 and r20["n_eff"] == 1000
    assert r19["loglik"][:20].tobytes() == r20["loglik"][:20].tobytes()
    l0, eps0, fin = likelihoods("bi_s0", b, y, atoms, lo, hi, noise_sd=noise_sd)
    S, lp_next, ll = em_step(l0, r19["log_prior"], fin)
    bd = step_bounds(l0, r19["log_prior"], eps0, fin, S)
    q = accept_step(r20["log_prior"], r19["log_prior"], lp_next, S, 1000, bd["lp"])
    print(f"update 20 from the library's update 19: error / bound = {q:.3g}")
    assert abs(r19["loglik"][19] - ll) <= bd["loglik"]
    S20, _, ll20 = em_step(l0, r20["log_prior"], fin)
    bound = step_bounds(l0, r20["log_prior"], eps0, fin, S20)["loglik"]
    steps = np.diff(r20["loglik"])
    print(f"loglik {r20['loglik'][0]:.6f} -> {r20['loglik'][-1]:.6f}, smallest step {steps.min():.3g}, bound {bound:.3g}")
    assert (steps >= -2 * bound).all() and r20["loglik"][-1] > r20["loglik"][0] + 1.0
    assert abs(r20["loglik"][20] - ll20) <= bound
    post = gpu.varpro_posterior("bi_s0", b, y, atoms, lo, hi, log_prior=r20["log_prior"], noise_sd=noise_sd)
    assert abs(post["log_evidence"].sum() - r20["loglik"][20]) <= 2 * bound  # the two kernels' bounds
    # reproducible, and the same from device memory
    two = gpu.varpro_prior_em("bi_s0", b, y, atoms, lo, hi, n_iter=20, **kw)
    assert r20["log_prior"].tobytes() == two["log_prior"].tobytes() and r20["loglik"].tobytes() == two["loglik"].tobytes()
    dev = torch.device("cuda", 0)
    yd = torch.from_numpy(y).to(dev)
    o = api.make_opts("bi_s0", len(b), jac="analytic")
    three = api.varpro_prior_em_device(o, 1000, b, yd, atoms, None, lo, hi, None, noise_sd, True, 20, 0.0, 0.0, 0,
                                       torch.cuda.current_stream(dev).cuda_stream)
    assert r20["log_prior"].tobytes() == three["log_prior"].tobytes() and r20["loglik"].tobytes() == three["loglik"].tobytes()
    assert three["n_iter"] == 20 and three["n_eff"] == 1000


def test_duplicating_the_voxels_changes_the_table_within_the_bound(gpu):
    b, y, _, atoms, _, _, lo, hi = _population()
    kw = dict(noise_sd=0.05, n_iter=1, rel_tol=0.0)
    one = gpu.varpro_prior_em("bi_s0", b, y, atoms, lo, hi, **kw)
    y2 = np.ascontiguousarray(np.tile(y, (2, 1)))
    two = gpu.varpro_prior_em("bi_s0", b, y2, atoms, lo, hi, **kw)
    assert two["n_eff"] == 2000
    l0, eps0, fin = likelihoods("bi_s0", b, y2, atoms, lo, hi, noise_sd=0.05)
    lp0 = normalise(None, atoms.shape[1])
    S, lp_next, _ = em_step(l0, lp0, fin)
    bd = step_bounds(l0, lp0, eps0, fin, S)
    accept_step(two["log_prior"], lp0, lp_next, S, 2000, bd["lp"])
    accept_step(two["log_prior"], lp0, one["log_prior"], S, 2000, 2 * bd["lp"])  # both runs within one bound of the reference
    assert abs(two["loglik"][0] - 2 * one["loglik"][0]) <= bd["loglik"]


@pytest.mark.parametrize("noise_sd", [0.0, 0.05])
def test_pseudo_count_keeps_every_admissible_atom(gpu, noise_sd):
    b, y, _, atoms, _, _, lo, hi = _population()
    G = atoms.shape[1]
    lp = np.zeros(G)
    lp[::7] = -np.inf
    n_adm = int(np.isfinite(lp).sum())
    for n_iter in (1, 30):
        got = gpu.varpro_prior_em("bi_s0", b, y, atoms, lo, hi, log_prior=lp, noise_sd=noise_sd, n_iter=n_iter, pseudo_count=0.5, rel_tol=0.0)
        assert (np.isinf(got["log_prior"]) == np.isinf(lp)).all()
        assert (got["log_prior"][np.isfinite(lp)] >= np.log(0.5 / (1000 + 0.5 * n_adm)) - 1e-12).all()


def test_rel_tol_stops_the_run(gpu):
    b, y, _, atoms, _, _, lo, hi = _population()
    got = gpu.varpro_prior_em("bi_s0", b, y, atoms, lo, hi, noise_sd=0.05, n_iter=6, rel_tol=1.0)
    assert got["n_iter"] == 1 and np.isfinite(got["loglik"][:2]).all() and np.isnan(got["loglik"][2:]).all() and got["loglik"].shape == (7,)
    one = gpu.varpro_prior_em("bi_s0", b, y, atoms, lo, hi, noise_sd=0.05, n_iter=1, rel_tol=0.0)
    assert one["log_prior"].tobytes() == got["log_prior"].tobytes() and one["loglik"].tobytes() == got["loglik"][:2].tobytes()
    loose = gpu.varpro_prior_em("bi_s0", b, y, atoms, lo, hi, noise_sd=0.05, n_iter=200, rel_tol=1e-4)
    assert 1 < loose["n_iter"] < 200
    ll, d = loose["loglik"], loose["n_iter"]
    assert ll[d] - ll[d - 1] <= 1e-4 * abs(ll[d]) and (np.diff(ll[:d]) > 1e-4 * np.abs(ll[1:d])).all()


# ---- what it is worth
@pytest.mark.parametrize("noise_sd,ref_f1,ref_d2", [(0.05, 0.564, 0.655), (0.0, 0.604, 0.681)])
def test_it_earns_its_keep(gpu, noise_sd, ref_f1, ref_d2):
    """1000 voxels of a population narrower than the dictionary (varpro_prior_reference.population, seed 0, 5 % noise; 91 pairs of 14
    rates over three decades): the ratio learned / uniform of the median |error| of the posterior mean after 30 updates.  numpy
    alone (varpro_prior_reference.reference_gain, seed 0; tests/test_varpro_prior_host.py pins it) reaches 0.564 for f1 and 0.655
    for D2 with the noise known, 0.604 and 0.681 marginalised (D1: 0.83, 0.84).  The library must reach the midpoint between the
    reference's ratio and 1: the margin covers the posterior's documented bound and nothing else, the midpoint keeps the test from
    passing on no gain."""
    b, y, truth, atoms, lo, hi, _, _ = _population()
    kw = dict(noise_sd=noise_sd)
    learned = gpu.varpro_prior_em("bi_s0", b, y, atoms, lo, hi, n_iter=30, rel_tol=0.0, **kw)
    flat = gpu.varpro_posterior("bi_s0", b, y, atoms, lo, hi, **kw)["mean"]
    post = gpu.varpro_posterior("bi_s0", b, y, atoms, lo, hi, log_prior=learned["log_prior"], **kw)["mean"]
    err = lambda mean: np.median(np.abs(mean[:3] - truth[:3]), axis=1)
    ratio = err(post) / err(flat)
    print("median abs error uniform", err(flat), "learned", err(post), "ratio", ratio)
    assert ratio[0] <= 0.5 * (ref_f1 + 1.0) and ratio[2] <= 0.5 * (ref_d2 + 1.0)


# ---- through the plugin
def test_through_the_solver(gpu):
    b, y, _, atoms, lo, hi, _, _ = _population()
    names = ["f1", "D1", "D2", "S0"]
    bounds = {n: (float(lo[i]), float(hi[i])) for i, n in enumerate(names)}
    rates = np.geomspace(3e-4, 0.3, 14)
    mk = lambda **kw: HipBayesVarProSolver(BiExpModel(fit_s0=True), rates={"D1": rates, "D2": rates}, bounds=bounds, noise_sd=0.05, **kw)
    s = mk(empirical_prior={"n_iter": 3, "max_voxels": 300}, marginals=True)
    assert s._nl_atoms.shape == (2, 91) and sorted(map(tuple, s._nl_atoms.T)) == sorted(map(tuple, atoms.T))
    nl = s._nl_atoms
    s.fit(b, y)
    em3 = gpu.varpro_prior_em("bi_s0", b, y[::4], nl, lo, hi, noise_sd=0.05, n_iter=3, pseudo_count=0.0, rel_tol=1e-6)
    d = s.diagnostics_
    assert set(d) == {"posterior_sd", "map", "map_atom", "log_evidence", "ess", "clipped_mass", "n_pixels", "log_prior", "prior_loglik",
                      "prior_n_iter", "prior_n_voxels", "marginal", "marginal_values", "quantiles", "quantile_probs", "geo_mean"}
    assert d["prior_n_voxels"] == 250 and d["prior_n_iter"] == em3["n_iter"] and d["log_prior"].shape == (91,) and s.log_prior is None
    assert d["log_prior"].tobytes() == em3["log_prior"].tobytes() and d["prior_loglik"].tobytes() == em3["loglik"].tobytes()
    want = gpu.varpro_posterior("bi_s0", b, y, nl, lo, hi, noise_sd=0.05, log_prior=em3["log_prior"])
    for i, n in enumerate(names):
        assert np.asarray(s.params_[n]).tobytes() == want["mean"][i].tobytes() and d["posterior_sd"][n].tobytes() == want["sd"][i].tobytes()
    mg = gpu.varpro_marginals("bi_s0", b, y, nl, lo, hi, noise_sd=0.05, log_prior=em3["log_prior"])
    for k, n in ((1, "D1"), (2, "D2")):
        assert d["marginal"][n].tobytes() == mg["marginal"][k].tobytes() and d["quantiles"][n].tobytes() == mg["quantiles"][k].tobytes()
        assert d["geo_mean"][n].tobytes() == mg["geo_mean"][k].tobytes()
    # a start prior is the EM's start; off is the plain posterior, bit for bit
    lp = np.zeros(91)
    lp[:16] = -np.inf
    st = mk(log_prior=lp, empirical_prior=True).fit(b, y)
    em_st = gpu.varpro_prior_em("bi_s0", b, y, nl, lo, hi, noise_sd=0.05, log_prior=lp)
    assert st.diagnostics_["log_prior"].tobytes() == em_st["log_prior"].tobytes() and np.isinf(st.diagnostics_["log_prior"][:16]).all()
    off = mk(empirical_prior=None).fit(b, y)
    plain = gpu.varpro_posterior("bi_s0", b, y, nl, lo, hi, noise_sd=0.05)
    assert set(off.diagnostics_) == {"posterior_sd", "map", "map_atom", "log_evidence", "ess", "clipped_mass", "n_pixels"}
    for i, n in enumerate(names):
        assert np.asarray(off.params_[n]).tobytes() == plain["mean"][i].tobytes()

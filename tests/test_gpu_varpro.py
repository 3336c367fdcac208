"""pnx_curvefit_varpro_f64 on the GPU against the numpy restatement (tests/varpro_reference.py): every axis of the kernel (voxels,
atoms, b-values, layouts), sigma / fixed rates / T1, exact recovery, ties, clips, non-finite voxels, host against device memory,
the plugin class and p0_varpro.  Noisy cases assert the condition that keeps the bound honest (tol <= 1e-3 of the smallest cost)."""
from __future__ import annotations

import numpy as np
import pytest
from grid_start_reference import signals
from varpro_reference import RATES, accept, case_atoms, case_box, case_signals, reference

from pyneapple_amd import api
from pyneapple_amd.models import TriExpModel
from pyneapple_amd.solvers import HipCurveFitSolver, HipVarProSolver

pytestmark = pytest.mark.gpu


def _fallback(lo, hi):
    return lo + 0.25 * (hi - lo)


def _run_and_accept(gpu, model, b, y, atoms, lo, hi, noisy=True, **kw):
    fb = _fallback(lo, hi)
    got = gpu.varpro(model, b, y, atoms, lo, hi, fb, **kw)
    ref = reference(model, b, y, atoms, lo, hi, noisy=noisy, **kw)
    print(f"{model}: kappa <= {ref['kappa'].max():.3g}, tol / min cost <= {(ref['tol'][ref['finite']] / ref['c'][ref['finite']].min(axis=1)).max():.3g}")
    accept(ref, got, atoms, fb)
    return ref, got


# one pass of a block is 128 voxels (four waves, two strips of 16 each) up to 64 b-values
@pytest.mark.parametrize("n_vox", [1, 15, 16, 17, 127, 128, 129, 1000])
def test_voxel_axis(gpu, n_vox):
    b, y = case_signals("tri_s0", n_vox)
    _run_and_accept(gpu, "tri_s0", b, y, case_atoms("tri_s0"), *case_box("tri_s0"))


def test_more_voxels_than_one_pass_of_the_grid(gpu):
    """The grid is capped at two blocks per CU: 70 000 voxels give every block of a 256-CU card a second pass."""
    b, y = case_signals("mono", 70001, n_b=5)
    _run_and_accept(gpu, "mono", b, y, case_atoms("mono"), *case_box("mono"))


# a slab of the tri-exponential layouts holds 48 atoms at 32 b-values
@pytest.mark.parametrize("n_atoms", [1, 15, 16, 17, 47, 48, 49, 64])
def test_atom_axis(gpu, n_atoms):
    assert api.varpro_slab_atoms(32, 3) == 48
    b, y = case_signals("tri_reduced", 50)
    _run_and_accept(gpu, "tri_reduced", b, y, case_atoms("tri_reduced")[:, :n_atoms], *case_box("tri_reduced"))


def test_dictionary_at_the_cap(gpu):
    b, y = case_signals("mono", 40, n_b=4)
    _run_and_accept(gpu, "mono", b, y, np.geomspace(3e-4, 0.3, 4096)[None], *case_box("mono"))


@pytest.mark.parametrize("model,n_b", [("mono", 2), ("mono", 4), ("mono", 5), ("tri_s0", 31), ("tri_s0", 32), ("tri_s0", 33), ("tri_s0", 64),
                                       ("tri_s0", 65), ("tri_s0", 128), ("bi_full", 128)])
def test_b_axis(gpu, model, n_b):
    b, y = case_signals(model, 150, n_b=n_b)
    _run_and_accept(gpu, model, b, y, case_atoms(model), *case_box(model))


@pytest.mark.parametrize("model", sorted(api.MODEL_IDS))
@pytest.mark.parametrize("narrow", [False, True])
def test_every_layout_and_its_clips(gpu, model, narrow):
    """narrow: the truth lies outside the box of the fractions and of S0, so the clips of every class are active."""
    b, y = case_signals(model, 130)
    ref, got = _run_and_accept(gpu, model, b, y, case_atoms(model), *case_box(model, narrow))
    if narrow:  # accept() has compared the flag with the reference voxel by voxel; most truths lie outside the narrowed box
        assert got["clipped"].mean() > 0.5
        lo, hi = case_box(model, narrow)
        assert ((got["params"] >= lo[:, None]) & (got["params"] <= hi[:, None])).all()
    else:
        assert not got["clipped"].all()


def test_sigma(gpu):
    b, y = case_signals("bi_s0", 100)
    sigma = np.linspace(0.5, 2.0, 32)
    _run_and_accept(gpu, "bi_s0", b, y, case_atoms("bi_s0"), *case_box("bi_s0"), sigma=sigma)


def test_shared_fixed_rate(gpu):
    b, y = case_signals("tri_s0", 100)
    lo, hi = case_box("tri_s0")
    free = [0, 1, 2, 3, 5]
    _run_and_accept(gpu, "tri_s0", b, y, case_atoms("tri_s0")[:2, ::4], lo[free], hi[free], fixed_idx=[4], fixed_vals=np.array([6e-4]))


@pytest.mark.parametrize("t1_mode,fixed", [(1, True), (2, True), (1, False)])
def test_t1_fixed_and_as_a_grid_axis(gpu, t1_mode, fixed):
    rng = np.random.default_rng(11)
    b = np.linspace(0.0, 1000.0, 32)
    kw = dict(t1_mode=t1_mode, tr=3000.0, tm=20.0 if t1_mode == 2 else 0.0)
    truth = np.stack([rng.uniform(0.8, 1.2, 90), rng.uniform(1e-3, 3e-3, 90), np.full(90, 1000.0) if fixed else rng.uniform(700.0, 1500.0, 90)])
    y = signals("mono", b, truth, **kw) + 0.02 * rng.standard_normal((90, 32))
    d = np.geomspace(3e-4, 0.03, 8)
    if fixed:
        _run_and_accept(gpu, "mono", b, y, d[None], np.array([0.0, 1e-5]), np.array([10.0, 0.5]), fixed_idx=[2], fixed_vals=np.array([1000.0]), **kw)
    else:
        atoms = np.ascontiguousarray(np.array([(a, t) for a in d for t in (600.0, 1000.0, 1600.0)]).T)
        _run_and_accept(gpu, "mono", b, y, atoms, np.array([0.0, 1e-5, 100.0]), np.array([10.0, 0.5, 5000.0]), **kw)


@pytest.mark.parametrize("model", ["mono", "bi_reduced", "tri_s0", "tri_full"])
def test_a_noise_free_voxel_returns_its_atom_and_amplitudes(gpu, model):
    atoms = case_atoms(model)
    names = api.MODEL_PARAM_NAMES[model]
    rng = np.random.default_rng(2)
    pick = rng.integers(0, atoms.shape[1], 60)
    truth = np.empty((len(names), 60))
    truth[[i for i, n in enumerate(names) if n.startswith("D")]] = atoms[:, pick]
    for i, n in enumerate(names):
        if not n.startswith("D"):
            truth[i] = rng.uniform(0.15, 0.4, 60) if n.startswith("f") else rng.uniform(0.8, 1.2, 60)
    b = np.linspace(0.0, 1000.0, 32)
    y = signals(model, b, truth)
    lo, hi = case_box(model)
    got = gpu.varpro(model, b, y, atoms, lo, hi, _fallback(lo, hi))
    accept(reference(model, b, y, atoms, lo, hi), got, atoms)
    assert (got["atom"] == pick).all() and (got["clipped"] == 0).all()
    np.testing.assert_allclose(got["params"], truth, rtol=0, atol=1e-9)
    assert (got["cost"] <= 1e-20 + 4 * 32 * 2.0 ** -52 * (y * y).sum(axis=1) * 50).all()


@pytest.mark.parametrize("n_atoms,first,second", [(33, 7, 20), (33, 2, 32), (64, 5, 60)])
def test_equal_costs_take_the_lower_index(gpu, n_atoms, first, second):
    """Two identical atoms cost the same bit for bit in any lane: the lower index wins, across lanes, tiles and slabs."""
    b, y = case_signals("tri_s0", 40)
    atoms = case_atoms("tri_s0")[:, :n_atoms].copy()
    lo, hi = case_box("tri_s0")
    base = gpu.varpro("tri_s0", b, y, atoms, lo, hi, _fallback(lo, hi))
    v = int(np.flatnonzero(base["atom"] != first)[0]) if (base["atom"] == first).all() else 0
    win = atoms[:, base["atom"][v]].copy()
    atoms[:, first] = win
    atoms[:, second] = win
    got = gpu.varpro("tri_s0", b, y, atoms, lo, hi, _fallback(lo, hi))
    twice = np.isin(got["atom"], (first, second))
    assert twice.any() and (got["atom"][twice] == first).all()
    accept(reference("tri_s0", b, y, atoms, lo, hi), got, atoms)


@pytest.mark.parametrize("model", ["bi_reduced", "tri_s0"])
def test_non_finite_voxels_leave_their_neighbours_bit_identical(gpu, model):
    b, y = case_signals(model, 70)
    atoms = case_atoms(model)
    lo, hi = case_box(model)
    fb = _fallback(lo, hi)
    clean = gpu.varpro(model, b, y, atoms, lo, hi, fb)
    bad = y.copy()
    bad[3, 5], bad[16, 0], bad[33, 31], bad[69, 7] = np.nan, np.inf, -np.inf, np.nan
    got = gpu.varpro(model, b, bad, atoms, lo, hi, fb)
    rest = np.setdiff1d(np.arange(70), [3, 16, 33, 69])
    for key in ("atom", "cost", "clipped"):
        assert got[key][rest].tobytes() == clean[key][rest].tobytes()
    assert np.ascontiguousarray(got["params"][:, rest]).tobytes() == np.ascontiguousarray(clean["params"][:, rest]).tobytes()
    accept(reference(model, b, bad, atoms, lo, hi), got, atoms, fb)


@pytest.mark.parametrize("n_vox,chunk", [(1000, None), (2500, 1024)])  # 2500 voxels in chunks of 1024: three pieces through the ring
def test_host_and_device_memory_return_the_same_bytes(gpu, monkeypatch, n_vox, chunk):
    import torch

    if chunk:
        monkeypatch.setenv("PNX_HOST_CHUNK", str(chunk))
    b, y = case_signals("tri_s0", n_vox)
    atoms = case_atoms("tri_s0")
    lo, hi = case_box("tri_s0")
    fb = _fallback(lo, hi)
    host = gpu.varpro("tri_s0", b, y, atoms, lo, hi, fb)
    dev = torch.device("cuda", 0)
    yd = torch.from_numpy(y).to(dev)
    p = torch.empty((6, n_vox), dtype=torch.float64, device=dev)
    atom = torch.empty(n_vox, dtype=torch.int32, device=dev)
    cost = torch.empty(n_vox, dtype=torch.float64, device=dev)
    clp = torch.empty(n_vox, dtype=torch.int8, device=dev)
    o = api.make_opts("tri_s0", 32, jac="analytic")
    st = torch.cuda.current_stream(dev).cuda_stream
    api.varpro_device(o, n_vox, b, yd, atoms, None, lo, hi, fb, p, atom, cost, clp, 0, st)
    torch.cuda.synchronize()
    for key, t in (("params", p), ("atom", atom), ("cost", cost), ("clipped", clp)):
        assert host[key].tobytes() == t.cpu().numpy().tobytes()
    api.varpro_device(o, n_vox, b, yd, atoms, None, lo, hi, fb, p.zero_(), None, None, None, 0, st)  # the optional outputs
    torch.cuda.synchronize()
    assert host["params"].tobytes() == p.cpu().numpy().tobytes()


def test_mono_agrees_with_the_projected_grid_start(gpu):
    b, y = case_signals("mono", 300)
    lo, hi = case_box("mono")
    d = np.array(RATES)
    ref, got = _run_and_accept(gpu, "mono", b, y, d[None], lo, hi)
    gs = gpu.grid_start("mono", b, y, np.stack([np.ones(8), d]), lo, hi, project_amplitude=True)
    assert (np.abs(gs["cost"] - got["cost"]) <= ref["tol"]).all()
    same = gs["best"] == got["atom"]
    v = np.arange(300)
    assert (np.abs(ref["c"][v, gs["best"]] - ref["c"][v, got["atom"]]) <= ref["tol"]).all()
    np.testing.assert_allclose(gs["p0"][0, same], got["params"][0, same], rtol=1e-12)


# ---- through the plugin interface and as the start of the fit
BOUNDS = {"f1": (0.0, 1.0), "D1": (1e-5, 0.5), "f2": (0.0, 1.0), "D2": (1e-5, 0.5), "D3": (1e-5, 0.5), "S0": (0.0, 10.0)}
P0 = {"f1": 0.2, "D1": 0.1, "f2": 0.3, "D2": 0.01, "D3": 0.001, "S0": 1.0}
TRI = {"D1": list(np.geomspace(0.04, 0.3, 4)), "D2": list(np.geomspace(4e-3, 0.02, 4)), "D3": list(np.geomspace(3e-4, 1.5e-3, 4))}
NAMES = api.MODEL_PARAM_NAMES["tri_s0"]


def test_hip_varpro_through_the_plugin_interface(gpu):
    b, y = case_signals("tri_s0", 200)
    y[7, 3] = np.nan
    s = HipVarProSolver(TriExpModel(fit_s0=True), TRI, max_iter=250, tol=1e-8, p0=P0, bounds=BOUNDS).fit(b, y)
    assert s._nl_atoms.tobytes() == case_atoms("tri_s0").tobytes()
    lo, hi = (np.array([BOUNDS[n][i] for n in NAMES]) for i in (0, 1))
    fb = np.array([P0[n] for n in NAMES])
    got = gpu.varpro("tri_s0", b, y, s._nl_atoms, lo, hi, fb)
    assert np.stack([s.params_[n] for n in NAMES]).tobytes() == got["params"].tobytes()
    assert sorted(s.diagnostics_) == ["atom", "clipped", "cost", "n_pixels"] and s.diagnostics_["n_pixels"] == 200
    for key in ("atom", "cost", "clipped"):
        assert s.diagnostics_[key].tobytes() == got[key].tobytes()
    accept(reference("tri_s0", b, y, s._nl_atoms, lo, hi), got, s._nl_atoms, fb)
    ok = [r.success for r in s.pixel_results_]
    assert ok.count(False) == 1 and not ok[7] and s.diagnostics_["atom"][7] == -1
    assert [s.params_[n][7] for n in NAMES] == [P0[n] for n in NAMES]


def test_p0_varpro_is_the_search_followed_by_the_fit(gpu, monkeypatch):
    b, y = case_signals("tri_s0", 301)
    kw = dict(model=TriExpModel(fit_s0=True), max_iter=250, tol=1e-8, p0=P0, bounds=BOUNDS)
    s = HipCurveFitSolver(**kw, p0_varpro={"rates": TRI}).fit(b, y)
    lo, hi = (np.array([BOUNDS[n][i] for n in NAMES]) for i in (0, 1))
    vp = gpu.varpro("tri_s0", b, y, s._varpro_nl_atoms, lo, hi, np.array([P0[n] for n in NAMES]))
    tile = lambda a: np.ascontiguousarray(np.repeat(a[:, None], len(y), axis=1))
    r = gpu.curvefit("tri_s0", b, y, vp["params"], tile(lo), tile(hi), max_nfev=250, ftol=1e-8, jac="fd")
    assert np.stack([s.params_[n] for n in NAMES]).tobytes() == r["popt"].tobytes()
    for key in ("pcov", "status", "nfev", "cost"):
        assert s.diagnostics_[key].tobytes() == r[key].tobytes()
    for key, src in (("p0_atom", "atom"), ("p0_cost", "cost"), ("p0_clipped", "clipped")):
        assert s.diagnostics_[key].tobytes() == vp[src].tobytes()
    st = s.diagnostics_["status"]
    print("status histogram", {int(k): int((st == k).sum()) for k in np.unique(st)})
    assert (st >= 0).all(), "a VARPRO start was refused by the fit (outside its bounds, or a non-finite residual)"
    # an explicit shared p0 serves the non-finite voxels only; without p0_varpro nothing of it shows
    assert "p0_atom" not in HipCurveFitSolver(**kw).fit(b, y[:20]).diagnostics_
    # sharded with the fit: two shards on one card give the single call's result
    monkeypatch.setenv("PNX_SHARE_DEVICE", "1")
    two = HipCurveFitSolver(**kw, p0_varpro={"rates": TRI}, n_gpus=2).fit(b, y)
    for key in ("pcov", "status", "nfev", "cost", "p0_atom", "p0_cost", "p0_clipped"):
        assert s.diagnostics_[key].tobytes() == two.diagnostics_[key].tobytes()
    for n in NAMES:
        assert np.asarray(s.params_[n]).tobytes() == np.asarray(two.params_[n]).tobytes()

"""pnx_curvefit_grid_start_f64 on the device against tests/grid_start_reference.py: tile edges along every axis, all layouts, the
tie rule, amplitude projection, weights / fixed parameters / T1, non-finite signals, host against device memory, and the solver's
p0_grid end to end.

Acceptance per voxel (grid_start_reference.accept): with c_ref[g] the reference's DIRECT cost of atom g, the library -- which
evaluates the expanded form, two dot products of n_b terms each rounding by at most n_b 2^-53 ||y|| ||s_g|| -- must choose an atom
with c_ref[best] <= min_g c_ref[g] + tol and report |cost - c_ref[best]| <= tol, tol = 4 n_b 2^-52 (||y||^2 + max_g ||s_g||^2)
(weighted norms with sigma); p0_out is a bit-for-bit copy of the atom; no padded atom ever wins."""
from __future__ import annotations

import numpy as np
import pytest
from conftest import load_golden, rel_err
from grid_start_reference import accept, reference, s0_row, signals

from pyneapple_amd import api, synth
from pyneapple_amd.models import TriExpModel
from pyneapple_amd.solvers import HipCurveFitSolver

pytestmark = pytest.mark.gpu

BOUNDS = {"f1": (0.0, 1.0), "f2": (0.0, 1.0), "f3": (0.0, 1.0), "D": (1e-5, 0.1), "D1": (0.01, 0.5), "D2": (2e-3, 0.01), "D3": (1e-5, 2e-3),
          "S0": (0.5, 2.0), "T1": (500.0, 3000.0)}
TRUTH = {**BOUNDS, "f1": (0.05, 0.4), "f2": (0.05, 0.4), "f3": (0.05, 0.4), "S0": (0.6, 1.8)}


def _names(model, t1_mode=0, fixed_idx=()):
    names = api.MODEL_PARAM_NAMES[model] + (["T1"] if t1_mode else [])
    return [n for i, n in enumerate(names) if i not in fixed_idx]


def _case(model, n_vox, n_atoms, n_b, seed=0, noise=0.02, **kw):
    """(b, y, atoms, lo, hi): atoms uniform inside the bounds, signals of uniform truth values with multiplicative noise."""
    rng = np.random.default_rng(1000 * seed + 7 * n_vox + 3 * n_atoms + n_b)
    names = _names(model, kw.get("t1_mode", 0), kw.get("fixed_idx", ()))
    lo = np.array([BOUNDS[n][0] for n in names])
    hi = np.array([BOUNDS[n][1] for n in names])
    atoms = np.ascontiguousarray(rng.uniform(lo[:, None], hi[:, None], (len(names), n_atoms)))
    truth = np.stack([rng.uniform(*TRUTH[n], n_vox) for n in names])
    b = synth.bvalues(n_b)
    y = signals(model, b, truth, **{k: v for k, v in kw.items() if k in ("fixed_idx", "fixed_vals", "t1_mode", "tr", "tm")})
    y = np.ascontiguousarray(y * (1.0 + noise * rng.standard_normal(y.shape)))
    return b, y, atoms, lo, hi


def _run_and_accept(gpu, model, b, y, atoms, lo, hi, project=False, **kw):
    got = gpu.grid_start(model, b, y, atoms, lo, hi, project_amplitude=project, **kw)
    ref = reference(model, b, y, atoms, lo, hi, project=project, **kw)
    accept(ref, got, atoms)
    return got, ref


# ---- tile edges: each axis' edge values crossed with one mid value of the others (mid: 65 voxels, 33 atoms, 16 b-values)
@pytest.mark.parametrize("n_vox", [1, 15, 16, 17, 63, 64, 65, 1000])
def test_voxel_axis(gpu, n_vox):
    _run_and_accept(gpu, "tri_reduced", *_case("tri_reduced", n_vox, 33, 16))


@pytest.mark.parametrize("n_atoms", [1, 15, 16, 17, 33, 257])  # 257 atoms at 16 b-values: two LDS slabs
def test_atom_axis(gpu, n_atoms):
    _run_and_accept(gpu, "tri_reduced", *_case("tri_reduced", 65, n_atoms, 16))


@pytest.mark.parametrize("n_b", [1, 3, 4, 5, 16, 31, 32, 33, 127, 128])  # 33 and 127 take the two larger instantiations
def test_b_axis(gpu, n_b):
    _run_and_accept(gpu, "tri_reduced", *_case("tri_reduced", 65, 33, n_b))


def test_dictionary_at_the_cap(gpu):
    """4096 atoms at 128 b-values: 86 slabs of 48 atoms through LDS, the largest dictionary the call takes."""
    _run_and_accept(gpu, "bi_reduced", *_case("bi_reduced", 65, 4096, 128))


@pytest.mark.parametrize("n_b,n_atoms", [(65, 17), (127, 65)])
def test_more_voxels_than_one_pass_of_the_grid(gpu, n_b, n_atoms):
    """A block owns 128 voxels per pass at more than 64 b-values and the grid is capped at two blocks per CU: 70 000 voxels send
    every block round its loop again -- with the one-slab dictionary resident in LDS (17 atoms) and with two slabs reloaded."""
    _run_and_accept(gpu, "bi_reduced", *_case("bi_reduced", 70000, n_atoms, n_b))


@pytest.mark.parametrize("model", sorted(api.MODEL_IDS))
def test_every_layout(gpu, model):
    _run_and_accept(gpu, model, *_case(model, 65, 33, 16))


# ---- the tie rule
@pytest.mark.parametrize("n_atoms,first,second", [(33, 7, 20), (33, 7, 23), (33, 2, 32), (300, 5, 280), (300, 250, 260)])
def test_equal_costs_take_the_lower_index(gpu, n_atoms, first, second):
    """One atom at two indices -- other lane, same lane in another tile, the last (partial) tile, another slab -- and noise-free
    signals generated from it: both dictionary rows are bit-identical, so are the costs, and the lower index must win."""
    b, _, atoms, lo, hi = _case("tri_reduced", 40, n_atoms, 16)
    atoms[:, second] = atoms[:, first]
    y = np.repeat(signals("tri_reduced", b, atoms[:, [first]]), 40, axis=0) * np.linspace(0.999, 1.001, 40)[:, None]
    got = gpu.grid_start("tri_reduced", b, y, atoms, lo, hi)
    assert (got["best"] == first).all()
    accept(reference("tri_reduced", b, y, atoms, lo, hi), got, atoms)


# ---- amplitude projection
@pytest.mark.parametrize("model", api.PROJECT_MODELS)
def test_projected_amplitude_is_clipped_to_its_bounds(gpu, model):
    """Voxels whose optimal amplitude lies below lo_S0 = 0.5 for every atom, inside for the good ones, and above hi_S0 = 2 for every
    atom.  Signals and rows are positive with s(0) = 1 and ||s||^2 <= 16, so y . s / ||s||^2 lies in [A / 16, 4 A] for a signal of
    amplitude A: A <= 0.09 stays below 0.5 and A >= 60 above 2 whatever the shapes (truth S0 is drawn from (0.6, 1.8))."""
    b, y, atoms, lo, hi = _case(model, 96, 33, 16)
    row = s0_row(model)
    y[:32] *= 0.05
    y[64:] *= 100.0
    atoms[row] = np.linspace(0.5, 2.0, atoms.shape[1])  # ignored by the search
    got, ref = _run_and_accept(gpu, model, b, y, atoms, lo, hi, project=True)
    assert (got["p0"][row, :32] == 0.5).all() and (got["p0"][row, 64:] == 2.0).all()
    mid = got["p0"][row, 32:64]
    assert ((mid > 0.5) & (mid < 2.0)).mean() > 0.5  # the data does exercise the unclipped branch; its values: accept() above
    # without projection the same call takes S0 from the atoms
    plain, _ = _run_and_accept(gpu, model, b, y, atoms, lo, hi, project=False)
    assert (plain["p0"][row] == atoms[row, plain["best"]]).all()


# ---- weights, fixed parameters, T1
def test_sigma(gpu):
    b, y, atoms, lo, hi = _case("tri_reduced", 65, 33, 16)
    sigma = np.linspace(0.5, 3.0, 16)
    _run_and_accept(gpu, "tri_reduced", b, y, atoms, lo, hi, sigma=sigma)
    b, y, atoms, lo, hi = _case("tri_s0", 65, 33, 16)
    _run_and_accept(gpu, "tri_s0", b, y, atoms, lo, hi, project=True, sigma=sigma)


def test_shared_fixed_parameter(gpu):
    kw = dict(fixed_idx=[1], fixed_vals=np.array([0.07]))  # D1 of [f1, D1, D2, S0]
    b, y, atoms, lo, hi = _case("bi_s0", 65, 33, 16, **kw)
    assert atoms.shape[0] == 3
    _run_and_accept(gpu, "bi_s0", b, y, atoms, lo, hi, **kw)
    _run_and_accept(gpu, "bi_s0", b, y, atoms, lo, hi, project=True, **kw)


@pytest.mark.parametrize("t1_mode", [1, 2])
def test_t1_factor_on_mono(gpu, t1_mode):
    kw = dict(t1_mode=t1_mode, tr=3000.0, tm=30.0 if t1_mode == 2 else 0.0)
    b, y, atoms, lo, hi = _case("mono", 65, 33, 16, **kw)
    assert atoms.shape[0] == 3  # [S0, D, T1]
    _run_and_accept(gpu, "mono", b, y, atoms, lo, hi, **kw)
    _run_and_accept(gpu, "mono", b, y, atoms, lo, hi, project=True, **kw)


# ---- non-finite signals
@pytest.mark.parametrize("project", [False, True])
def test_non_finite_voxels_do_not_touch_their_neighbours(gpu, project):
    model = "tri_s0" if project else "tri_reduced"
    b, y, atoms, lo, hi = _case(model, 64, 33, 16)
    clean = gpu.grid_start(model, b, y, atoms, lo, hi, project_amplitude=project)
    bad = y.copy()
    bad[3, 5] = np.nan
    bad[21, 0] = np.inf
    bad[40, 15] = -np.inf
    got = gpu.grid_start(model, b, bad, atoms, lo, hi, project_amplitude=project)
    where = np.array([3, 21, 40])
    assert (got["best"][where] == -1).all() and np.isnan(got["cost"][where]).all()
    assert (got["p0"][:, where] == atoms[:, [0]]).all()
    rest = np.setdiff1d(np.arange(64), where)  # the other voxels of the same 16-voxel tiles: identical bytes
    for key in ("best", "cost"):
        assert got[key][rest].tobytes() == clean[key][rest].tobytes()
    assert np.ascontiguousarray(got["p0"][:, rest]).tobytes() == np.ascontiguousarray(clean["p0"][:, rest]).tobytes()
    accept(reference(model, b, bad, atoms, lo, hi, project=project), got, atoms)


# ---- host path against device path
@pytest.mark.parametrize("n_vox,chunk", [(1000, None), (2500, 1024)])  # 2500 voxels in chunks of 1024: three pieces through the ring
def test_host_and_device_memory_return_the_same_bytes(gpu, monkeypatch, n_vox, chunk):
    import torch

    if chunk:
        monkeypatch.setenv("PNX_HOST_CHUNK", str(chunk))
    b, y, atoms, lo, hi = _case("tri_s0", n_vox, 257, 32)
    host = gpu.grid_start("tri_s0", b, y, atoms, lo, hi, project_amplitude=True)
    dev = torch.device("cuda", 0)
    yd = torch.from_numpy(y).to(dev)
    p0 = torch.empty((6, n_vox), dtype=torch.float64, device=dev)
    best = torch.empty(n_vox, dtype=torch.int32, device=dev)
    cost = torch.empty(n_vox, dtype=torch.float64, device=dev)
    o = api.make_opts("tri_s0", 32, jac="analytic")
    api.grid_start_device(o, n_vox, b, yd, atoms, None, lo, hi, True, p0, best, cost, 0, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert host["p0"].tobytes() == p0.cpu().numpy().tobytes()
    assert host["best"].tobytes() == best.cpu().numpy().tobytes()
    assert host["cost"].tobytes() == cost.cpu().numpy().tobytes()
    # best and cost are optional
    api.grid_start_device(o, n_vox, b, yd, atoms, None, lo, hi, True, p0.zero_(), None, None, 0, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert host["p0"].tobytes() == p0.cpu().numpy().tobytes()


# ---- end to end through the solver
GRID = {"f1": [0.1, 0.3], "D1": [0.03, 0.1], "f2": [0.2, 0.4], "D3": [5e-4, 1.5e-3]}


def test_solver_with_p0_grid_is_the_search_followed_by_the_fit(gpu):
    d = load_golden("g3_tri_reduced")
    names = api.MODEL_PARAM_NAMES["tri_reduced"]
    b, y, p0, lo, hi = d["bvalues"], d["y"], d["p0_vals"], d["lo_vals"], d["hi_vals"]
    kw = dict(model=TriExpModel(), max_iter=int(d["max_iter"]), tol=float(d["tol"]), p0=dict(zip(names, map(float, p0))),
              bounds={n: (float(a), float(c)) for n, a, c in zip(names, lo, hi)})
    s = HipCurveFitSolver(**kw, p0_grid=GRID)
    assert s._p0_atoms.shape == (5, 16)
    s.fit(b, y)
    gs = gpu.grid_start("tri_reduced", b, y, s._p0_atoms, lo, hi)
    accept(reference("tri_reduced", b, y, s._p0_atoms, lo, hi), gs, s._p0_atoms)
    tile = lambda a: np.ascontiguousarray(np.repeat(a[:, None], len(y), axis=1))
    r = gpu.curvefit("tri_reduced", b, y, gs["p0"], tile(lo), tile(hi), max_nfev=int(d["max_iter"]), ftol=float(d["tol"]), jac="fd")
    assert np.stack([s.params_[n] for n in names]).tobytes() == r["popt"].tobytes()
    for key in ("pcov", "status", "nfev", "cost"):
        assert s.diagnostics_[key].tobytes() == r[key].tobytes()
    assert s.diagnostics_["p0_atom"].dtype == np.int32 and (s.diagnostics_["p0_atom"] == gs["best"]).all()
    assert s.diagnostics_["p0_cost"].tobytes() == gs["cost"].tobytes()
    # an explicit p0 wins: the grid is not consulted, the result is the plain fit's
    s.fit(b, y, p0=dict(zip(names, map(float, p0))))
    assert "p0_atom" not in s.diagnostics_
    # the same solver without p0_grid still reproduces the fixture, and so does the explicit-p0 fit above
    plain = HipCurveFitSolver(**kw).fit(b, y)
    assert "p0_atom" not in plain.diagnostics_
    for fit in (plain, s):
        assert ((fit.diagnostics_["status"] > 0) == d["success"]).all()
        assert rel_err(np.stack([fit.params_[n] for n in names]).T, d["popt"]).max() <= 1e-4


def test_solver_shards_the_search_with_the_fit(gpu, monkeypatch):
    """n_gpus = 2 on one card (PNX_SHARE_DEVICE): each shard searches and fits its own voxels; the joined result is the single call's."""
    monkeypatch.setenv("PNX_SHARE_DEVICE", "1")
    b, y, _ = synth.make_numpy("tri_reduced", 301, 32)
    names, p0, lo, hi = synth.shared_arrays("tri_reduced")
    kw = dict(model=TriExpModel(), max_iter=250, tol=1e-8, p0=dict(zip(names, map(float, p0))),
              bounds={n: (float(a), float(c)) for n, a, c in zip(names, lo, hi)}, p0_grid=GRID)
    one, two = HipCurveFitSolver(**kw).fit(b, y), HipCurveFitSolver(**kw, n_gpus=2).fit(b, y)
    for key in ("pcov", "status", "nfev", "cost", "p0_atom", "p0_cost"):
        assert one.diagnostics_[key].tobytes() == two.diagnostics_[key].tobytes()
    for n in names:
        assert np.asarray(one.params_[n]).tobytes() == np.asarray(two.params_[n]).tobytes()

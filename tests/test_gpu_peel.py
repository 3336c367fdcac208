"""pnx_peel_f64 / _f32 on the device against tests/peel_reference.py: tile and row edges for every number of stages, the
mono-exponential case against pnx_loglinear_f64, hand-built rows, an analytic row, clipping, unaligned input, host against device
memory, float32 storage, and HipPeelSolver / HipCurveFitSolver(p0_peel=...) end to end.

The parity bar is measured, not chosen: per compared quantity (parameters, ss_res; peel_reference.differences) the two numpy forms
of the reference -- each stage's line by the centred closed form, or by np.linalg.lstsq on sqrt(w)-scaled rows, each form running
its own chain of stages -- are compared on the test's own inputs, and the device must agree with the lstsq form to
max(1e-12, 100 x that difference): the margin covers a device log / exp that differs from numpy's in the last place.  Every voxel
is compared; the test prints the three figures of each case.  The worst device differences measured on an MI355X over the shapes
below are recorded in DESIGN.md 4.1f."""
from __future__ import annotations

import functools

import numpy as np
import pytest
from conftest import rel_err
from peel_reference import STAGES, differences, model_signal, parity_case, reference, signals

from pyneapple_amd import api
from pyneapple_amd.models import BiExpModel, MonoExpModel, TriExpModel
from pyneapple_amd.solvers import HipCurveFitSolver, HipPeelSolver

pytestmark = pytest.mark.gpu

KEYS = ("params", "status", "n_used", "ss_res")
WCODE = {"none": 0, "signal2": 1}


def _device(b, y, model, want=KEYS, y_dev=None, **kw):
    """api.peel_device on torch tensors -> numpy dict; y_dev: a device tensor to use instead of uploading y."""
    import torch

    dev = torch.device("cuda:0")
    yd = torch.from_numpy(np.ascontiguousarray(y)).to(dev) if y_dev is None else y_dev
    n, dt = yd.shape[0], yd.dtype
    out = dict(params=torch.empty((len(api.MODEL_PARAM_NAMES[model]), n), dtype=dt, device=dev),
               status=torch.empty(n, dtype=torch.int8, device=dev), n_used=torch.empty((STAGES[model], n), dtype=torch.int32, device=dev),
               ss_res=torch.empty(n, dtype=dt, device=dev))
    arg = {k: (v if k in want else None) for k, v in out.items()}
    api.peel_device(b, yd, model, arg["params"], arg["status"], arg["n_used"], arg["ss_res"], 0,
                    stream=torch.cuda.current_stream(dev).cuda_stream, **kw)
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in out.items() if k in want}


def _rows(d, k, idx):
    """voxels idx of result array k (parameters and n_used are parameter-major)"""
    return np.ascontiguousarray(d[k][:, idx] if k in ("params", "n_used") else d[k][idx])


def _same_bytes(a, b, keys=KEYS):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


@functools.lru_cache(maxsize=None)
def _parity_reference(model, n_vox, n_b, weighting):
    """(b, y, masks, lstsq form, per-quantity bar, measured): computed once per case, shared, never modified."""
    b, y, masks, lsq, measured = parity_case(model, n_vox, n_b, WCODE[weighting])
    for a in (b, y, masks, *lsq.values()):
        a.setflags(write=False)
    return b, y, masks, lsq, {k: max(1e-12, 100.0 * v) for k, v in measured.items()}, measured


def _shapes(K):
    # each axis' edge values crossed with one mid value of the other (129 voxels = two full tiles and a lane), and the largest of both
    return [(n, 24) for n in (1, 63, 64, 65, 129, 4161)] + [(129, n_b) for n_b in (2 * K, 2 * K + 1, 16, 33, 128)] + [(4161, 128)]


CASES = [(m, n, n_b) for m in ("mono", "bi_s0", "tri_s0") for n, n_b in _shapes(STAGES[m])] + \
        [(m, 129, 24) for m in ("bi_reduced", "bi_full", "tri_reduced", "tri_full")]


@pytest.mark.parametrize("weighting", ["none", "signal2"])
@pytest.mark.parametrize("model,n_vox,n_b", CASES)
def test_parity_over_tile_and_row_edges(gpu, model, n_vox, n_b, weighting):
    b, y, masks, ref, bar, measured = _parity_reference(model, n_vox, n_b, weighting)
    got = gpu.peel(b, y, model, masks=masks, weighting=weighting)
    assert np.array_equal(got["status"], ref["status"]) and np.array_equal(got["n_used"], ref["n_used"])
    diff = differences(got, ref, y, masks)
    print(f"peel parity {model} n_vox={n_vox} n_b={n_b} {weighting}: "
          + ", ".join(f"{k} gpu {diff[k]:.2e} numpy-forms {measured[k]:.2e} bar {bar[k]:.2e}" for k in diff))
    for k in diff:
        assert diff[k] <= bar[k], (k, diff[k], bar[k])


@pytest.mark.parametrize("weighting", ["none", "signal2"])
def test_one_stage_is_the_loglinear_fit(gpu, weighting):
    b, y, masks, ref, bar, _ = _parity_reference("mono", 129, 24, weighting)
    keep = b >= 100
    peel = gpu.peel(b, y, "mono", masks=keep[None, :], weighting=weighting)
    ll = gpu.loglinear(b, y, bvalue_mask=keep, weighting=weighting, n_reweight=0, want_pcov=False)
    assert np.array_equal(peel["status"], ll["status"]) and np.array_equal(peel["n_used"][0], ll["n_used"])
    d = differences(peel, ll, y, keep[None, :])
    print(f"peel vs loglinear {weighting}: params {d['params']:.2e} ss_res {d['ss_res']:.2e} bar {bar}")
    assert d["params"] <= bar["params"] and d["ss_res"] <= bar["ss_res"]


def test_hand_built_rows_beside_ordinary_neighbours(gpu):
    b, y, masks = signals("bi_s0", 70, 12, seed=3)  # two tiles; the special rows sit in both
    masks = masks.copy()
    masks[1, 1] = False  # b-value 1 belongs to no stage
    slow, fast = np.flatnonzero(masks[0]), np.flatnonzero(masks[1])
    assert slow.size >= 3 and fast.size >= 4 and not masks[:, 1].any()
    clean = gpu.peel(b, y, "bi_s0", masks=masks)
    assert (clean["status"] == 1).all() and (clean["n_used"][0] == slow.size).all()
    bad = y.copy()
    bad[3, fast[2]] = 1e-3        # one fast sample below the slow extrapolation: a negative residual, left out
    bad[9, fast] = 1e-3           # the whole fast segment below it: no positive residual, status 0
    bad[20, slow[1]] = np.nan     # NaN inside M
    bad[21, 1] = np.nan           # NaN outside M: ignored
    bad[22, 1] = -np.inf          # likewise
    bad[66, fast[0]] = np.inf     # inf inside M, second tile
    bad[68, fast[2:]] = 1e-3      # exactly two usable samples in the fast stage
    got = gpu.peel(b, bad, "bi_s0", masks=masks)
    special = [3, 9, 20, 66, 68]
    others = np.setdiff1d(np.arange(70), special)
    for k in KEYS:
        assert _rows(got, k, others).tobytes() == _rows(clean, k, others).tobytes(), k
    assert got["status"][[3, 9, 20, 21, 22, 66, 68]].tolist() == [1, 0, -2, 1, 1, -2, 1]
    assert got["n_used"][:, [3, 9, 20, 66, 68]].tolist() == [[slow.size] * 2 + [0, 0, slow.size], [fast.size - 1, 0, 0, 0, 2]]
    for v in (9, 20, 66):
        assert np.isnan(got["params"][:, v]).all() and np.isnan(got["ss_res"][v])
    ref = reference("bi_s0", b, bad, masks)
    assert np.array_equal(got["status"], ref["status"]) and np.array_equal(got["n_used"], ref["n_used"])
    d = differences(got, ref, bad, masks)
    assert max(d.values()) < 1e-10, d
    # the slow stage of the rows whose fast segment was spoilt is untouched: D2 is the clean call's, bit for bit
    assert got["params"][2, [3, 68]].tobytes() == clean["params"][2, [3, 68]].tobytes()
    # with a fallback the failed rows hold it exactly, their ss_res stays NaN, and nothing else changes
    fb = [0.25, 0.04, 1.5e-3, 900.0]
    for res in (gpu.peel(b, bad, "bi_s0", masks=masks, fallback=fb), _device(b, bad, "bi_s0", masks=masks, fallback=fb)):
        for v in (9, 20, 66):
            assert res["params"][:, v].tolist() == fb and np.isnan(res["ss_res"][v])
        keep = np.setdiff1d(np.arange(70), [9, 20, 66])
        for k in KEYS:
            assert _rows(res, k, keep).tobytes() == _rows(got, k, keep).tobytes(), k
        assert np.array_equal(res["status"], got["status"]) and np.array_equal(res["n_used"], got["n_used"])


def test_analytic_row(gpu):
    """Noise-free bi-exponential with fast D = 0.1 and the slow stage on b >= 200: the fast compartment's share of the tail is
    below exp(-20), so both stages recover their parameters to rtol 1e-6."""
    b = np.array([0.0, 5.0, 10.0, 15.0, 20.0, 30.0, 40.0, 200.0, 400.0, 600.0, 800.0, 1000.0])
    f1, D1, D2, S0 = 0.3, 0.1, 1.2e-3, 1000.0
    y = np.tile(S0 * (f1 * np.exp(-b * D1) + (1 - f1) * np.exp(-b * D2)), (65, 1))
    for weighting in ("signal2", "none"):
        got = gpu.peel(b, y, "bi_s0", b_thresholds=[200.0], weighting=weighting)
        assert (got["status"] == 1).all() and got["n_used"][:, 0].tolist() == [5, 7]
        np.testing.assert_allclose(got["params"], np.tile(np.array([f1, D1, D2, S0])[:, None], (1, 65)), rtol=1e-6)
        assert (got["params"] == got["params"][:, :1]).all() and (got["ss_res"] < 1e-6 * (y[0] ** 2).sum()).all()
    full = gpu.peel(b, y[:1], "bi_full", b_thresholds=[200.0])
    np.testing.assert_allclose(full["params"][:, 0], [f1 * S0, D1, (1 - f1) * S0, D2], rtol=1e-6)


@pytest.mark.parametrize("model", ["bi_s0", "tri_reduced"])
def test_clip_moves_only_the_voxels_outside(gpu, model):
    b, y, masks = signals(model, 130, 24, seed=4)
    free = gpu.peel(b, y, model, masks=masks)
    assert (free["status"] == 1).all()
    names = api.MODEL_PARAM_NAMES[model]
    iD = names.index("D1")
    lo, hi = np.full(len(names), -1e300), np.full(len(names), 1e300)
    lo[iD], hi[-1] = np.median(free["params"][iD]), np.median(free["params"][-1])  # half of D1 below, half of the last one above
    got = gpu.peel(b, y, model, masks=masks, clip=(lo, hi))
    low, high = free["params"][iD] < lo[iD], free["params"][-1] > hi[-1]
    moved = low | high
    assert low.sum() > 10 and high.sum() > 10 and (~moved).sum() > 10
    assert (got["status"][moved] == 2).all() and (got["status"][~moved] == 1).all()
    assert (got["params"][iD][low] == lo[iD]).all() and (got["params"][-1][high] == hi[-1]).all()
    for k in KEYS:  # unclipped voxels: the bytes of the call without clip
        assert _rows(got, k, ~moved).tobytes() == _rows(free, k, ~moved).tobytes(), k
    assert np.array_equal(got["n_used"], free["n_used"])
    pred = np.stack([model_signal(model, got["params"][:, v], b) for v in range(130)])
    np.testing.assert_allclose(got["ss_res"], ((pred - y) ** 2).sum(axis=1), rtol=1e-9)  # at the clipped point
    assert (got["ss_res"][moved] > free["ss_res"][moved]).any()
    ref = reference(model, b, y, masks, clip=(lo, hi))
    assert np.array_equal(got["status"], ref["status"])
    assert max(differences(got, ref, y, masks).values()) < 1e-10


@pytest.mark.parametrize("n_b", [7, 16])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_unaligned_input_gives_identical_bytes(gpu, n_b, dtype):
    import torch

    b, y, masks = signals("tri_s0", 129, n_b, seed=1)
    y = y.astype(dtype)
    dev = torch.device("cuda:0")
    flat = torch.from_numpy(y.reshape(-1)).to(dev)
    buf = torch.empty(flat.numel() + 3, dtype=flat.dtype, device=dev)
    for off in (1, 3) if dtype == "float32" else (1,):  # 8 (4, 12) bytes past a 16-byte boundary
        view = buf[off:off + flat.numel()]
        view.copy_(flat)
        assert view.data_ptr() % 16 != 0 and flat.data_ptr() % 16 == 0
        for kw in (dict(), dict(weighting="none")):
            _same_bytes(_device(b, y, "tri_s0", masks=masks, y_dev=view.view(129, n_b), **kw),
                        _device(b, y, "tri_s0", masks=masks, y_dev=flat.view(129, n_b), **kw))


@pytest.mark.parametrize("n_vox", [129, 4161])
def test_host_arrays_give_the_bytes_of_device_pointers(gpu, n_vox, monkeypatch):
    b, y, masks = signals("tri_s0", n_vox, 16, seed=5)
    y = y.copy()
    y[n_vox // 2, 3] = np.nan
    kw = dict(masks=masks, clip=([0.0, 0.01, 0.0, 1e-3, 1e-4, 1.0], [1.0, 1.0, 1.0, 0.1, 5e-3, 1500.0]), fallback=[0.2, 0.1, 0.3, 0.01, 1e-3, 800.0])
    host = gpu.peel(b, y, "tri_s0", **kw)
    assert host["status"][n_vox // 2] == -2 and (host["status"] == 2).any() and (host["status"] == 1).any()
    _same_bytes(host, _device(b, y, "tri_s0", **kw))
    # optional outputs left out: the others do not change
    _same_bytes(_device(b, y, "tri_s0", want=("params",), **kw), host, keys=("params",))
    _same_bytes(_device(b, y, "tri_s0", want=("params", "n_used"), **kw), host, keys=("params", "n_used"))
    _same_bytes(_device(b, y, "tri_s0", want=("params", "status", "ss_res"), **kw), host, keys=("params", "status", "ss_res"))
    if n_vox == 4161:  # several chunks through the ring (the chunk size is a developer switch, tests/conftest.py opens the gate)
        monkeypatch.setenv("PNX_HOST_CHUNK", "1024")
        _same_bytes(gpu.peel(b, y, "tri_s0", **kw), host)


def test_float32_storage_matches_the_widened_float64_call(gpu):
    b, y, masks = signals("bi_s0", 200, 24, seed=6)
    b32, y32 = b.astype(np.float32), y.astype(np.float32)
    y32[7, 3] = np.nan
    # bounds and fallback that float32 holds exactly
    kw = dict(masks=masks, clip=([0.0, 2.0 ** -6, 2.0 ** -12, 1.0], [1.0, 0.5, 2.0 ** -9, 1024.0]), fallback=[0.25, 0.0625, 2.0 ** -10, 512.0])
    wide = gpu.peel(b32.astype(np.float64), y32.astype(np.float64), "bi_s0", **kw)
    for got in (gpu.peel(b32, y32, "bi_s0", **kw), _device(b32, y32, "bi_s0", **kw)):
        assert got["params"].dtype == got["ss_res"].dtype == np.float32
        assert np.array_equal(got["status"], wide["status"]) and np.array_equal(got["n_used"], wide["n_used"])
        for k in ("params", "ss_res"):  # to float32 rounding of the outputs
            np.testing.assert_allclose(got[k].astype(np.float64), wide[k], rtol=2.0 ** -23, atol=0, equal_nan=True)
        assert got["params"][:, 7].tolist() == kw["fallback"]
    assert (wide["status"] == 2).sum() > 10 and (wide["status"] == 1).sum() > 10 and wide["status"][7] == -2


def test_solver_sentinels_names_and_shapes(gpu):
    b, y, masks = signals("tri_s0", 40, 24, seed=7)
    y = y.copy()
    y[5, masks[2]] = 1e-3  # the fastest segment below the extrapolation of the others
    y[6, 2] = np.nan
    names = api.MODEL_PARAM_NAMES["tri_s0"]
    p0 = dict(zip(names, [0.2, 0.15, 0.3, 0.012, 1.1e-3, 777.0]))
    s = HipPeelSolver(TriExpModel(fit_s0=True), b_thresholds=[30.0, 250.0], p0=p0).fit(b, y)
    raw = gpu.peel(b, y, "tri_s0", b_thresholds=[30.0, 250.0])
    assert list(s.params_) == names and all(s.params_[n].shape == (40,) for n in names)
    assert s.diagnostics_["status"][[5, 6]].tolist() == [0, -2] and (np.delete(s.diagnostics_["status"], [5, 6]) == 1).all()
    for v in (5, 6):
        assert [s.params_[n][v] for n in names] == list(p0.values())
        r = s.pixel_results_[v]
        assert r.success is False and r.covariance is None and list(r.params) == list(p0.values()) and r.message
    ok = np.delete(np.arange(40), [5, 6])
    for i, n in enumerate(names):
        assert np.array_equal(s.params_[n][ok], raw["params"][i][ok])
    assert all(s.pixel_results_[int(v)].success and s.pixel_results_[int(v)].message is None for v in ok)
    assert set(s.diagnostics_) == {"n_pixels", "status", "n_used", "ss_res"} and s.diagnostics_["n_pixels"] == 40
    assert s.diagnostics_["n_used"].shape == (3, 40) and np.isnan(s.diagnostics_["ss_res"][[5, 6]]).all()
    n = HipPeelSolver(TriExpModel(fit_s0=True), b_thresholds=[30.0, 250.0]).fit(b, y)  # without p0: NaN
    assert all(np.isnan(n.params_[k][[5, 6]]).all() for k in names)
    # bounds clip; a single row, as the reference's solvers take it; one exponential needs no threshold; float32 arrays
    bounds = {k: (0.0, 1e4) for k in names}
    bounds["S0"] = (1.0, float(np.median(raw["params"][5][ok])))
    c = HipPeelSolver(TriExpModel(fit_s0=True), b_thresholds=[30.0, 250.0], bounds=bounds).fit(b, y)
    assert (c.diagnostics_["status"] == 2).sum() >= 15 and np.nanmax(c.params_["S0"]) == bounds["S0"][1]
    one = HipPeelSolver(BiExpModel(fit_s0=True), b_thresholds=[150.0]).fit(b, y[0])
    assert list(one.params_) == api.MODEL_PARAM_NAMES["bi_s0"] and all(isinstance(v, list) and len(v) == 1 for v in one.params_.values())
    m = HipPeelSolver(MonoExpModel(), io_dtype="float32").fit(b, y)
    assert m.params_["S0"].dtype == np.float32 and m.diagnostics_["n_used"].shape == (1, 40)


def test_curvefit_starts_from_the_peel(gpu, oracle, monkeypatch):
    rng = np.random.default_rng(11)
    b = np.array([0, 10, 20, 40, 80, 150, 200, 300, 400, 500, 600, 700, 800, 1000, 1200.0])
    shape = (16, 16, 2)
    f1, D1 = rng.uniform(0.15, 0.35, shape), rng.uniform(0.02, 0.08, shape)
    D2, S0 = rng.uniform(8e-4, 2e-3, shape), rng.uniform(500.0, 1500.0, shape)
    e = lambda D: np.exp(-b * D[..., None])
    image = S0[..., None] * (f1[..., None] * e(D1) + (1 - f1[..., None]) * e(D2)) * (1 + 0.005 * rng.standard_normal(shape + (b.size,)))
    y = np.ascontiguousarray(image.reshape(-1, b.size))
    y[17, 4] = np.nan        # the peel cannot use it: the voxel starts from the shared p0 (and the fit refuses it as well)
    # a fast compartment that is gone by b = 10 (2 % under the slow curve from there on): one positive residual in the fast
    # stage, the peel fails, the fit runs from the shared p0
    y[18, 1:5] = 0.98 * (S0 * (1 - f1)).reshape(-1)[18] * np.exp(-b[1:5] * D2.reshape(-1)[18])
    names = api.MODEL_PARAM_NAMES["bi_s0"]
    p0 = {"f1": 0.2, "D1": 0.05, "D2": 1e-3, "S0": 1000.0}
    bounds = {"f1": (0.0, 1.0), "D1": (5e-3, 0.06), "D2": (1e-5, 5e-3), "S0": (1.0, 5000.0)}  # D1 up to 0.08: some peel starts are clipped
    peel = {"b_thresholds": [150.0], "weighting": "signal2"}
    s = HipCurveFitSolver(BiExpModel(fit_s0=True), 250, 1e-8, p0=p0, bounds=bounds, p0_peel=peel).fit(b, y)
    lo, hi = (np.array([bounds[n][k] for n in names]) for k in (0, 1))
    start = gpu.peel(b, y, "bi_s0", b_thresholds=[150.0], clip=(lo, hi), fallback=[p0[n] for n in names])
    assert np.array_equal(s.diagnostics_["p0_status"], start["status"]) and s.diagnostics_["p0_status"].dtype == np.int8
    assert start["status"][[17, 18]].tolist() == [-2, 0] and (start["status"] == 2).sum() > 10 and (start["status"] == 1).sum() > 100
    assert (start["params"][1][start["status"] == 2] == 0.06).any()  # starts that sit exactly on a bound
    tile = lambda a: np.ascontiguousarray(np.repeat(a[:, None], y.shape[0], axis=1))
    direct = gpu.curvefit("bi_s0", b, y, start["params"], tile(lo), tile(hi), max_nfev=250, ftol=1e-8, jac="fd")
    for i, n in enumerate(names):
        assert s.params_[n].tobytes() == direct["popt"][i].tobytes(), n
    for k in ("status", "nfev", "cost", "pcov"):
        assert s.diagnostics_[k].tobytes() == direct[k].tobytes(), k
    assert set(s.diagnostics_) == {"pcov", "n_pixels", "status", "nfev", "cost", "p0_status"}
    ref = oracle.curvefit("bi_s0", b, y, start["params"], tile(lo), tile(hi), max_nfev=250, ftol=1e-8, jac="fd")
    assert np.array_equal(direct["status"] > 0, ref["status"] > 0) and direct["status"][17] == -2
    good = ref["status"] > 0
    assert good.sum() == y.shape[0] - 1
    assert rel_err(direct["popt"][:, good], ref["popt"][:, good]).max() <= 1e-4
    # the plain solver is not touched by the option
    plain = HipCurveFitSolver(BiExpModel(fit_s0=True), 250, 1e-8, p0=p0, bounds=bounds).fit(b, y)
    assert "p0_status" not in plain.diagnostics_
    # two shards on one card give the single call's result
    monkeypatch.setenv("PNX_SHARE_DEVICE", "1")
    two = HipCurveFitSolver(BiExpModel(fit_s0=True), 250, 1e-8, p0=p0, bounds=bounds, p0_peel=peel, n_gpus=2).fit(b, y)
    for n in names:
        assert two.params_[n].tobytes() == s.params_[n].tobytes(), n
    assert np.array_equal(two.diagnostics_["p0_status"], s.diagnostics_["p0_status"])

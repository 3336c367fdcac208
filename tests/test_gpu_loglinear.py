"""pnx_loglinear_f64 / _f32 on the device against tests/loglinear_reference.py: tile and row edges, unaligned input, the b-value
mask, hand-built rows, clipping, host against device memory, float32 storage, and HipLogLinearSolver / HipSegmentedFitter end to end.

The parity bar is measured, not chosen: per compared quantity (parameters, covariance, ss_res; loglinear_reference.differences) the
two numpy forms of the reference -- the centred closed form and np.linalg.lstsq on sqrt(w)-scaled rows -- are compared on the
test's own inputs, and the device must agree with the lstsq form to max(1e-12, 100 x that difference): the margin covers a device
log / exp that differs from numpy's in the last place.  Every voxel is compared; the test prints the three figures of each case.
Worst device differences measured on an MI355X over the shapes below: parameters 2.3e-14, covariance 2.4e-11 at
3 b-values (one degree of freedom; the numpy forms differ by as much) and 5.8e-13 from 5 b-values on, ss_res 6.5e-11 at 3 b-values
and 5.6e-12 otherwise."""
from __future__ import annotations

import functools

import numpy as np
import pytest
from loglinear_reference import differences, reference, signals

from pyneapple_amd import api
from pyneapple_amd.fitters import HipPixelWiseFitter
from pyneapple_amd.models import BiExpModel, MonoExpModel
from pyneapple_amd.segmented import HipSegmentedFitter
from pyneapple_amd.solvers import HipCurveFitSolver, HipLogLinearSolver

pytestmark = pytest.mark.gpu

KEYS = ("params", "pcov", "status", "n_used", "ss_res")
WCODE = {"none": 0, "signal2": 1}


def _device(b, y, bvalue_mask=None, weighting="signal2", n_reweight=0, clip=None, want=KEYS, y_dev=None):
    """api.loglinear_device on torch tensors -> numpy dict; y_dev: a device tensor to use instead of uploading y."""
    import torch

    dev = torch.device("cuda:0")
    yd = torch.from_numpy(np.ascontiguousarray(y)).to(dev) if y_dev is None else y_dev
    n, dt = yd.shape[0], yd.dtype
    out = dict(params=torch.empty((2, n), dtype=dt, device=dev), pcov=torch.empty((n, 2, 2), dtype=dt, device=dev),
               status=torch.empty(n, dtype=torch.int8, device=dev), n_used=torch.empty(n, dtype=torch.int32, device=dev),
               ss_res=torch.empty(n, dtype=dt, device=dev))
    arg = {k: (v if k in want else None) for k, v in out.items()}
    api.loglinear_device(b, yd, arg["params"], arg["pcov"], arg["status"], arg["n_used"], arg["ss_res"], 0, bvalue_mask=bvalue_mask,
                         weighting=weighting, n_reweight=n_reweight, clip=clip, stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in out.items() if k in want}


def _rows(d, k, idx):
    """voxels idx of result array k (the parameters are parameter-major)"""
    return np.ascontiguousarray(d[k][:, idx] if k == "params" else d[k][idx])


def _same_bytes(a, b, keys=KEYS):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


@functools.lru_cache(maxsize=None)
def _parity_reference(n_vox, n_b, weighting, n_reweight):
    """(b, y, lstsq form, per-quantity bar): computed once per shape, shared, never modified."""
    b, y, _, _ = signals(n_vox, n_b)
    cen = reference(b, y, weighting=WCODE[weighting], n_reweight=n_reweight, form="centred")
    lsq = reference(b, y, weighting=WCODE[weighting], n_reweight=n_reweight, form="lstsq")
    assert (cen["status"] == 1).all() and (lsq["status"] == 1).all() and (cen["n_used"] == n_b).all()
    measured = differences(cen, lsq, y)
    for a in (b, y, *lsq.values()):
        a.setflags(write=False)
    return b, y, lsq, {k: max(1e-12, 100.0 * v) for k, v in measured.items()}, measured


# each axis' edge values crossed with one mid value of the other (mid: 129 voxels = two full tiles and a lane, 23 b-values = an odd
# row), and the largest of both
SHAPES = [(n, 23) for n in (1, 63, 64, 65, 129, 4161)] + [(129, n_b) for n_b in (2, 3, 5, 16, 33, 128)] + [(4161, 128)]


@pytest.mark.parametrize("n_reweight", [0, 2])
@pytest.mark.parametrize("weighting", ["none", "signal2"])
@pytest.mark.parametrize("n_vox,n_b", SHAPES)
def test_parity_over_tile_and_row_edges(gpu, n_vox, n_b, weighting, n_reweight):
    b, y, ref, bar, measured = _parity_reference(n_vox, n_b, weighting, n_reweight)
    got = gpu.loglinear(b, y, weighting=weighting, n_reweight=n_reweight)
    assert np.array_equal(got["status"], ref["status"]) and np.array_equal(got["n_used"], ref["n_used"])
    diff = differences(got, ref, y)
    print(f"loglinear parity n_vox={n_vox} n_b={n_b} {weighting} rw={n_reweight}: "
          + ", ".join(f"{k} gpu {diff[k]:.2e} numpy-forms {measured[k]:.2e} bar {bar[k]:.2e}" for k in diff))
    for k in diff:
        assert diff[k] <= bar[k], (k, diff[k], bar[k])
    assert np.isnan(got["pcov"]).all() == (n_b == 2)  # two points: a line without a residual


@pytest.mark.parametrize("n_b", [5, 16])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_unaligned_input_gives_identical_bytes(gpu, n_b, dtype):
    import torch

    b, y, _, _ = signals(129, n_b, seed=1)
    y = y.astype(dtype)
    dev = torch.device("cuda:0")
    flat = torch.from_numpy(y.reshape(-1)).to(dev)
    buf = torch.empty(flat.numel() + 3, dtype=flat.dtype, device=dev)
    for off in (1, 3) if dtype == "float32" else (1,):  # 8 (4, 12) bytes past a 16-byte boundary
        view = buf[off:off + flat.numel()]
        view.copy_(flat)
        assert view.data_ptr() % 16 != 0 and flat.data_ptr() % 16 == 0
        for kw in (dict(), dict(weighting="none", n_reweight=1)):
            _same_bytes(_device(b, y, y_dev=view.view(129, n_b), **kw), _device(b, y, y_dev=flat.view(129, n_b), **kw))


@pytest.mark.parametrize("weighting,n_reweight", [("signal2", 0), ("none", 2)])
def test_mask_equals_the_sliced_call(gpu, weighting, n_reweight):
    b, y, _, _ = signals(200, 23, seed=2)
    keep = b >= 200
    assert 3 <= keep.sum() < b.size
    masked = gpu.loglinear(b, y, bvalue_mask=keep, weighting=weighting, n_reweight=n_reweight)
    sliced = gpu.loglinear(b[keep], np.ascontiguousarray(y[:, keep]), weighting=weighting, n_reweight=n_reweight)
    _same_bytes(masked, sliced)  # ss_res too: both see the same samples
    assert (masked["n_used"] == keep.sum()).all()
    ref = reference(b, y, use=keep, weighting=WCODE[weighting], n_reweight=n_reweight)
    diff = differences(masked, ref, y, use=keep)
    assert max(diff["params"], diff["ss_res"]) < 1e-10 and np.array_equal(masked["status"], ref["status"])


def test_hand_built_rows_beside_ordinary_neighbours(gpu):
    b, y, _, _ = signals(70, 8, seed=3)  # two tiles; the special rows sit in both
    use = np.ones(8, bool)
    use[1] = False
    clean = gpu.loglinear(b, y, bvalue_mask=use)
    bad = y.copy()
    bad[3, 4] = -5.0          # one non-positive sample: left out
    bad[9, 2:] = 0.0          # all but one usable (column 1 is masked out): no line
    bad[9, 0] = 700.0
    bad[20, 5] = np.nan       # NaN inside the mask
    bad[21, 1] = np.nan       # NaN outside the mask: ignored
    bad[22, 1] = -np.inf      # likewise
    bad[66, 6] = np.inf       # inf inside the mask, second tile
    bad[68, :] = -1.0         # exactly two usable samples
    bad[68, 0], bad[68, 7] = 900.0, 300.0
    got = gpu.loglinear(b, bad, bvalue_mask=use)
    special = [3, 9, 20, 66, 68]
    others = np.setdiff1d(np.arange(70), special)
    for k in KEYS:
        assert _rows(got, k, others).tobytes() == _rows(clean, k, others).tobytes(), k
    assert got["status"][[3, 9, 20, 21, 22, 66, 68]].tolist() == [1, 0, -2, 1, 1, -2, 1]
    assert got["n_used"][[3, 9, 20, 66, 68]].tolist() == [6, 1, 0, 0, 2]
    for v in (9, 20, 66):
        assert np.isnan(got["params"][:, v]).all() and np.isnan(got["pcov"][v]).all() and np.isnan(got["ss_res"][v])
    ref = reference(b, bad, use=use)
    assert np.array_equal(got["status"], ref["status"]) and np.array_equal(got["n_used"], ref["n_used"])
    d = differences({k: _rows(got, k, [3]) for k in ("params", "pcov", "ss_res")},
                    {k: _rows(ref, k, [3]) for k in ("params", "pcov", "ss_res")}, bad[[3]], use=use)
    assert max(d.values()) < 1e-10
    # the exact two-point line: D = ln(900 / 300) / (b7 - b0), S0 = 900 exp(b0 D), no covariance; ss_res counts the masked-in
    # non-positive samples too
    D = np.log(900.0 / 300.0) / (b[7] - b[0])
    np.testing.assert_allclose(got["params"][:, 68], [900.0 * np.exp(b[0] * D), D], rtol=1e-13)
    assert np.isnan(got["pcov"][68]).all()
    pred = got["params"][0, 68] * np.exp(-b[use] * got["params"][1, 68])
    np.testing.assert_allclose(got["ss_res"][68], ((pred - bad[68, use]) ** 2).sum(), rtol=1e-12)


def test_clip_moves_only_the_voxels_outside(gpu):
    b, y, S0, D = signals(130, 16, seed=4)
    lo, hi = [100.0, 1e-3], [1500.0, 0.1]  # D in [3e-4, 3e-3] and S0 in [200, 2000]: some of each outside
    free = gpu.loglinear(b, y)
    got = gpu.loglinear(b, y, clip=(lo, hi))
    low_d, high_s = free["params"][1] < lo[1], free["params"][0] > hi[0]
    moved = low_d | high_s
    assert low_d.sum() > 10 and high_s.sum() > 10 and (~moved).sum() > 10
    assert (got["status"][moved] == 2).all() and (got["status"][~moved] == 1).all()
    assert (got["params"][1][low_d] == lo[1]).all() and (got["params"][0][high_s] == hi[0]).all()
    for k in KEYS:  # unclipped voxels: the bytes of the call without clip
        assert _rows(got, k, ~moved).tobytes() == _rows(free, k, ~moved).tobytes(), k
    assert got["pcov"].tobytes() == free["pcov"].tobytes()  # the covariance is left as computed
    pred = got["params"][0][:, None] * np.exp(-b[None, :] * got["params"][1][:, None])
    np.testing.assert_allclose(got["ss_res"][moved], ((pred - y) ** 2).sum(axis=1)[moved], rtol=1e-12)
    ref = reference(b, y, clip=(lo, hi))
    assert np.array_equal(got["status"], ref["status"])
    assert max(differences(got, ref, y).values()) < 1e-10


@pytest.mark.parametrize("n_vox", [129, 4161])
def test_host_arrays_give_the_bytes_of_device_pointers(gpu, n_vox, monkeypatch):
    b, y, _, _ = signals(n_vox, 16, seed=5)
    kw = dict(bvalue_mask=b >= 100, n_reweight=1, clip=([100.0, 1e-3], [1500.0, 0.1]))
    host = gpu.loglinear(b, y, **kw)
    _same_bytes(host, _device(b, y, **kw))
    # optional outputs left out on both paths: the others do not change
    assert gpu.loglinear(b, y, want_pcov=False, **kw)["pcov"] is None
    _same_bytes(gpu.loglinear(b, y, want_pcov=False, **kw), host, keys=("params", "status", "n_used", "ss_res"))
    _same_bytes(_device(b, y, want=("params",), **kw), host, keys=("params",))
    if n_vox == 4161:  # several chunks through the ring (the chunk size is a developer switch, tests/conftest.py opens the gate)
        monkeypatch.setenv("PNX_HOST_CHUNK", "1024")
        _same_bytes(gpu.loglinear(b, y, **kw), host)


def test_float32_storage_matches_the_widened_float64_call(gpu):
    b, y, _, _ = signals(200, 23, seed=6)
    b32, y32 = b.astype(np.float32), y.astype(np.float32)
    y32[7, 3] = np.nan
    y32[8, 2] = -1.0
    kw = dict(bvalue_mask=b >= 50, clip=([100.0, 2.0 ** -10], [1500.0, 0.125]))  # bounds that float32 holds exactly
    wide = gpu.loglinear(b32.astype(np.float64), y32.astype(np.float64), **kw)
    for got in (gpu.loglinear(b32, y32, **kw), _device(b32, y32, **kw)):
        assert got["params"].dtype == got["pcov"].dtype == got["ss_res"].dtype == np.float32
        assert np.array_equal(got["status"], wide["status"]) and np.array_equal(got["n_used"], wide["n_used"])
        for k in ("params", "pcov", "ss_res"):  # to float32 rounding of the outputs
            np.testing.assert_allclose(got[k].astype(np.float64), wide[k], rtol=2.0 ** -23, atol=0, equal_nan=True)
    assert (wide["status"] == 2).sum() > 10 and wide["status"][7] == -2 and wide["n_used"][8] == wide["n_used"][0] - 1


def test_solver_sentinels(gpu):
    b, y, _, _ = signals(40, 8, seed=7)
    y[5, 1:] = 0.0     # one usable sample
    y[6, 2] = np.nan
    p0 = {"S0": 777.0, "D": 1.5e-3}
    s = HipLogLinearSolver(MonoExpModel(), p0=p0).fit(b, y)
    raw = gpu.loglinear(b, y)
    assert s.diagnostics_["status"][[5, 6]].tolist() == [0, -2] and (np.delete(s.diagnostics_["status"], [5, 6]) == 1).all()
    for v in (5, 6):
        assert (s.params_["S0"][v], s.params_["D"][v]) == (777.0, 1.5e-3)
        r = s.pixel_results_[v]
        assert r.success is False and np.isnan(r.covariance).all() and list(r.params) == [777.0, 1.5e-3] and r.message
    ok = np.delete(np.arange(40), [5, 6])
    assert np.array_equal(s.params_["S0"][ok], raw["params"][0][ok]) and np.array_equal(s.params_["D"][ok], raw["params"][1][ok])
    assert all(s.pixel_results_[int(v)].success and s.pixel_results_[int(v)].message is None for v in ok)
    assert set(s.diagnostics_) == {"pcov", "n_pixels", "status", "n_used", "ss_res"} and s.diagnostics_["n_pixels"] == 40
    n = HipLogLinearSolver(MonoExpModel()).fit(b, y)  # without p0: NaN
    assert np.isnan(n.params_["S0"][[5, 6]]).all() and np.isnan(n.params_["D"][[5, 6]]).all()
    one = HipLogLinearSolver(MonoExpModel()).fit(b, y[0])  # a single row, as the reference's solvers take it
    assert one.params_["S0"] == [float(raw["params"][0, 0])] and one.diagnostics_["pcov"].shape == (2, 2)


def test_segmented_fit_with_loglinear_step1(gpu):
    rng = np.random.default_rng(11)
    b = np.array([0, 10, 20, 40, 80, 150, 200, 300, 400, 500, 600, 700, 800, 1000, 1200.0])
    shape = (16, 16, 2)
    f1, D1 = rng.uniform(0.1, 0.3, shape), rng.uniform(0.02, 0.08, shape)
    D2, S0 = rng.uniform(8e-4, 2e-3, shape), rng.uniform(500.0, 1500.0, shape)
    e = lambda D: np.exp(-b * D[..., None])
    image = S0[..., None] * (f1[..., None] * e(D1) + (1 - f1[..., None]) * e(D2)) * (1 + 0.005 * rng.standard_normal(shape + (b.size,)))
    step1 = HipLogLinearSolver(MonoExpModel())
    step2 = HipCurveFitSolver(BiExpModel(fit_s0=True), 250, 1e-8, p0={"f1": 0.2, "D1": 0.05, "D2": 1e-3, "S0": 1000.0},
                              bounds={"f1": (0.0, 1.0), "D1": (5e-3, 0.5), "D2": (1e-5, 5e-3), "S0": (1.0, 5000.0)})
    f = HipSegmentedFitter(step1, step2, step1_bvalue_range=(200, None), fixed_from_step1=["D"], param_mapping={"D": "D2"})
    f.fit(b, image)
    # step-1 maps: a direct call with the same mask on the same rows
    direct = gpu.loglinear(b, image.reshape(-1, b.size), bvalue_mask=b >= 200)
    assert np.array_equal(f.step1_params_["S0"], direct["params"][0]) and np.array_equal(f.step1_params_["D"], direct["params"][1])
    assert f.step1_result_.success.all() and np.nanmin(f.step1_result_.r_squared) > 0.98
    # the tail of a bi-exponential decay is its slow compartment: D2 to a few percent
    assert np.median(np.abs(f.step1_params_["D"] / D2.reshape(-1) - 1)) < 0.05
    # the reference's keys and shapes: step-2 parameters followed by the fixed ones, one value per voxel
    assert list(f.fitted_params_) == ["f1", "D1", "S0", "D2"]
    assert all(np.asarray(v).shape == (512,) for v in f.fitted_params_.values())
    assert np.array_equal(f.fitted_params_["D2"], f.step1_params_["D"])
    assert f.results_.n_pixels == 512 and f.results_.success.mean() > 0.95 and np.nanmedian(f.results_.r_squared) > 0.99
    maps = f.parameter_maps()
    assert set(maps) == {"f1", "D1", "S0", "D2"} and all(m.shape == shape for m in maps.values())
    assert np.median(np.abs(f.fitted_params_["f1"] - f1.reshape(-1))) < 0.05
    # the pixel-wise fitter forwards the mask on its own too
    pw = HipPixelWiseFitter(HipLogLinearSolver(MonoExpModel())).fit(b, image, bvalue_mask=b >= 200)
    assert np.array_equal(pw.fitted_params_["D"], direct["params"][1])

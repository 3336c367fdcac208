"""Which lane of which wave fits a voxel, beside which neighbours, and which row loop of the pass it takes are decided at run
time: by the work queue, by the size of the batch and by the FD steps of the other lanes of the wave.  None of that may show in
a result.  Here a batch on the device-resident path is compared, byte for byte (NaN patterns included), with the same voxels
fitted one or a few per call, where every voxel sits in another lane beside other neighbours: an index that is lost,
handed out twice or fitted from another voxel's signal tile shows as a difference, and so does a row loop that does not compute
the bits of the other one."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODEL = "tri_reduced"
KEYS = ("popt", "pcov", "status", "nfev", "cost")
VOX_AXIS = {"popt": 1, "pcov": 0, "status": 0, "nfev": 0, "cost": 0}
# per-call sizes of the piecewise fits: one voxel per call for small batches, "a few" (either side of a wave) for large ones
SMALL, LARGE = (1,), (1, 3, 7, 33, 61, 64, 65)


def fit(y, b, p0, lo, hi, order=None):
    """One device-resident call; p0 / lo / hi are numpy (n,) arrays (shared) or device tensors (n, n_vox) (per voxel).  Every
    output starts from a sentinel no fit produces, so a voxel that was never written shows."""
    import torch
    from pyneapple_amd import api

    dev = y.device
    m, n_b = y.shape
    pv = not isinstance(p0, np.ndarray)
    n = p0.shape[0]
    out = dict(popt=torch.full((n, m), -7.5, dtype=torch.float64, device=dev),
               pcov=torch.full((m, n, n), -7.5, dtype=torch.float64, device=dev),
               status=torch.full((m,), 99, dtype=torch.int8, device=dev),
               nfev=torch.full((m,), -7, dtype=torch.int32, device=dev),
               cost=torch.full((m,), -7.5, dtype=torch.float64, device=dev))
    opts = api.make_opts(MODEL, n_b, per_voxel=pv, max_nfev=250, ftol=1e-8, jac="fd")
    api.curvefit_device(opts, m, b, y, p0, lo, hi, None, out["popt"], out["pcov"], out["status"], out["nfev"], out["cost"],
                        dev.index or 0, torch.cuda.current_stream().cuda_stream, order=order)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def piecewise(y, b, p0, lo, hi, sizes):
    """The rows of y fitted in consecutive calls of sizes[0], sizes[1], ... voxels (cycling), concatenated."""
    pv = not isinstance(p0, np.ndarray)
    parts, start, k = [], 0, 0
    while start < y.shape[0]:
        stop = min(start + sizes[k % len(sizes)], y.shape[0])
        sub = [a[:, start:stop].contiguous() if pv else a for a in (p0, lo, hi)]
        parts.append(fit(y[start:stop].contiguous(), b, *sub))
        start, k = stop, k + 1
    return {key: np.concatenate([p[key] for p in parts], axis=VOX_AXIS[key]) for key in KEYS}


def assert_same_bytes(got, want, label):
    for key in KEYS:
        a, w = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert a.shape == w.shape and a.dtype == w.dtype, (label, key)
        same = a.view(np.uint8).reshape(a.shape + (-1,)) == w.view(np.uint8).reshape(w.shape + (-1,))
        bad = np.unique(np.argwhere(~same)[:, VOX_AXIS[key]])
        assert bad.size == 0, f"{label}: {key} differs on {bad.size} voxels, first {bad[:8].tolist()}"


def assert_every_voxel_written(r):
    assert (r["status"] != 99).all() and (r["nfev"] != -7).all()
    assert not (r["popt"] == -7.5).any() and not (r["cost"] == -7.5).any() and not (r["pcov"] == -7.5).any()


@pytest.mark.parametrize("n_b", [32, 31])
@pytest.mark.parametrize("n_vox", [1, 63, 64, 65, 577, 4097, 65536 + 1])
def test_batch_equals_its_voxels_fitted_apart(gpu, n_vox, n_b):
    """Sizes either side of a wave, of a block and of the resident grid; 31 b-values add the partial last row block and the odd
    row's signal load.  With and without order=."""
    import torch
    from pyneapple_amd import synth

    dev = torch.device("cuda", 0)
    b, y = synth.make_torch(MODEL, n_vox, n_b, dev, sigma=0.01, seed=100 + n_b)
    _, p0, lo, hi = synth.shared_arrays(MODEL)
    whole = fit(y, b, p0, lo, hi)
    assert_every_voxel_written(whole)
    assert (whole["status"] > 0).mean() >= 0.99
    apart = piecewise(y, b, p0, lo, hi, SMALL if n_vox <= 577 else LARGE)
    assert_same_bytes(whole, apart, f"{n_vox} voxels x {n_b}")
    perm = torch.randperm(n_vox, device=dev, generator=torch.Generator(device=dev).manual_seed(n_vox)).to(torch.int32)
    for order in (perm, torch.arange(n_vox - 1, -1, -1, device=dev, dtype=torch.int32)):
        assert_same_bytes(fit(y, b, p0, lo, hi, order=order), whole, f"{n_vox} voxels x {n_b}, order=")


def per_voxel_arrays(n_vox, dev):
    import torch
    from pyneapple_amd import synth

    _, p0, lo, hi = synth.shared_arrays(MODEL)
    return [torch.from_numpy(np.repeat(a[:, None], n_vox, axis=1)).to(dev).contiguous() for a in (p0, lo, hi)]


@pytest.mark.parametrize("n_vox", [577, 4097])
def test_refused_voxels_are_reported_once_among_fitted_ones(gpu, n_vox):
    """Scattered voxels with lo >= hi (status -1) or p0 outside its bounds (-3) take the early exit of the refill and still consume
    one queue index each: every voxel of the batch is written, the refused ones with p0, zero evaluations and a NaN cost and
    covariance, and all of them as when fitted alone."""
    import torch
    from pyneapple_amd import synth

    dev = torch.device("cuda", 0)
    b, y = synth.make_torch(MODEL, n_vox, 32, dev, sigma=0.01, seed=7)
    p0, lo, hi = per_voxel_arrays(n_vox, dev)
    rng = np.random.default_rng(n_vox)
    kind = rng.choice([0, 1, 3], size=n_vox, p=[0.8, 0.1, 0.1])
    kind[:3] = (1, 3, 1)  # the first indices a wave pulls
    kind[-1] = 3
    bad_bounds = torch.from_numpy(kind == 1).to(dev)
    bad_p0 = torch.from_numpy(kind == 3).to(dev)
    lo[3, bad_bounds] = hi[3, bad_bounds]  # lo == hi for D2
    p0[1, bad_p0] = 0.75                   # D1 above its upper bound of 0.5
    whole = fit(y, b, p0, lo, hi)
    assert_every_voxel_written(whole)
    np.testing.assert_array_equal(whole["status"][kind == 1], -1)
    np.testing.assert_array_equal(whole["status"][kind == 3], -3)
    refused = kind != 0
    assert (whole["status"][~refused] > 0).mean() >= 0.99
    np.testing.assert_array_equal(whole["nfev"][refused], 0)
    assert np.isnan(whole["cost"][refused]).all() and np.isnan(whole["pcov"][refused]).all()
    np.testing.assert_array_equal(whole["popt"][:, refused], p0.cpu().numpy()[:, refused])
    assert_same_bytes(whole, piecewise(y, b, p0, lo, hi, SMALL if n_vox <= 577 else LARGE), f"{n_vox} voxels, refused subset")


@pytest.mark.parametrize("n_b", [32, 31])
def test_fd_factor_out_of_range_in_some_lanes(gpu, n_b):
    """The row pass tests once per pass whether |b dx| < 2e-4 holds for the largest b-value in every lane of the wave and then
    runs a row loop without the per-row test; otherwise the generic loop.  Every seventh voxel starts D1 at 40 (upper bound 100:
    dx = 1.5e-8 * 40, |b dx| = 7e-4 at b = 1200), so its wave takes the generic loop while that voxel is far out, and its
    neighbours change loops during their fit.  Alone, the neighbours never leave the short loop: equality with the voxels fitted
    apart shows that both loops compute the same bits."""
    import torch
    from pyneapple_amd import synth

    dev = torch.device("cuda", 0)
    n_vox = 1500
    b, y = synth.make_torch(MODEL, n_vox, n_b, dev, sigma=0.01, seed=11)
    p0, lo, hi = per_voxel_arrays(n_vox, dev)
    far = torch.arange(n_vox, device=dev) % 7 == 3
    hi[1] = 100.0
    p0[1, far] = 40.0
    assert float(b.max()) * 1.4901161193847656e-08 * 40.0 >= 2e-4 > float(b.max()) * 1.4901161193847656e-08
    whole = fit(y, b, p0, lo, hi)
    assert_every_voxel_written(whole)
    assert_same_bytes(whole, piecewise(y, b, p0, lo, hi, SMALL), f"{n_vox} voxels x {n_b}, some lanes out of range")

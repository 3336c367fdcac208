"""Team mode of the fp64 curve-fit kernel: a wave whose queue has run dry and that has one voxel left evaluates that voxel's
rows one per lane instead of one after the other in the owner's lane.  Which voxels end in a drained wave depends on timing, so
the mode must not show in a single bit.  PNX_CF_TEAM=0 (a test hook, read at every call) keeps the lone lane on the old path:
every case here is fitted twice by the same library, hook off and on, and compared byte for byte, NaN patterns included.  A
batch of 65 voxels puts one voxel alone into the second wave, which is a team from its first evaluation to its last; in every
batch the last survivor of each wave ends as one too."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("popt", "pcov", "status", "nfev", "cost")
VOX_AXIS = {"popt": 1, "pcov": 0, "status": 0, "nfev": 0, "cost": 0}
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "curvefit_team_parent.npz")


def fit(model, y, b, p0, lo, hi, *, team, jac="fd", sigma=None, max_nfev=250):
    """One device-resident call with the team mode on or off; outputs start from sentinels no fit produces."""
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
    opts = api.make_opts(model, n_b, per_voxel=pv, max_nfev=max_nfev, ftol=1e-8, jac=jac, sigma=sigma)
    old = os.environ.pop("PNX_CF_TEAM", None)
    try:
        if not team:
            os.environ["PNX_CF_TEAM"] = "0"
        api.curvefit_device(opts, m, b, y, p0, lo, hi, None, out["popt"], out["pcov"], out["status"], out["nfev"], out["cost"],
                            dev.index or 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        os.environ.pop("PNX_CF_TEAM", None)
        if old is not None:
            os.environ["PNX_CF_TEAM"] = old
    return {k: v.cpu().numpy() for k, v in out.items()}


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


def both(model, y, b, p0, lo, hi, label, **kw):
    off = fit(model, y, b, p0, lo, hi, team=False, **kw)
    on = fit(model, y, b, p0, lo, hi, team=True, **kw)
    assert_every_voxel_written(on)
    assert_same_bytes(on, off, label)
    return on


def resident_grid(capfd):
    """Blocks of a launch that fills the device, from the library's own launch trace."""
    import torch
    from pyneapple_amd import synth

    dev = torch.device("cuda", 0)
    b, y = synth.make_torch("mono", 1 << 17, 8, dev, sigma=0.01, seed=3)
    _, p0, lo, hi = synth.shared_arrays("mono")
    os.environ["PNX_LAUNCH_TRACE"] = "1"
    try:
        capfd.readouterr()
        fit("mono", y, b, p0, lo, hi, team=True)
        err = capfd.readouterr().err
    finally:
        del os.environ["PNX_LAUNCH_TRACE"]
    m = re.search(r"\[pnx launch\] curvefit .* waves=(\d+) .* grid=(\d+)", err)
    assert m, err
    assert int(m.group(1)) == 4
    return int(m.group(2))


def test_batch_sizes_around_a_wave_and_the_resident_grid(gpu, capfd):
    """1, 2, 63, 65 voxels and one more than the resident lanes of the device hold (4 waves x 64 lanes x grid): the benchmark's
    instantiation, hook off against hook on."""
    import torch
    from pyneapple_amd import synth

    dev = torch.device("cuda", 0)
    g = resident_grid(capfd)
    assert 1 <= g <= 4096
    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    big = 4 * 64 * g + 1
    b, yall = synth.make_torch("tri_reduced", big, 32, dev, sigma=0.01, seed=41)
    for n_vox in (1, 2, 63, 65, big):
        r = both("tri_reduced", yall[:n_vox].contiguous(), b, p0, lo, hi, f"{n_vox} voxels")
        assert (r["status"] > 0).mean() >= 0.99 or n_vox < 100


@pytest.mark.parametrize("n_b", [1, 2, 7, 8, 31, 32, 33, 64, 65, 128])
def test_every_row_count_model_jacobian_and_sigma(gpu, n_b):
    """65 voxels (the 65th alone in its wave) for mono, bi reduced and tri reduced, FD and analytic Jacobians, with and without
    sigma, along the b-value axis: odd counts, the partial last block, fewer rows than parameters, more rows than lanes."""
    import torch
    from pyneapple_amd import synth

    dev = torch.device("cuda", 0)
    sig = np.linspace(0.5, 2.0, n_b)
    for model in ("mono", "bi_reduced", "tri_reduced"):
        b, y = synth.make_torch(model, 65, n_b, dev, sigma=0.02, seed=500 + n_b)
        _, p0, lo, hi = synth.shared_arrays(model)
        for jac in ("fd", "analytic"):
            for sigma in (None, sig):
                both(model, y, b, p0, lo, hi, f"{model} n_b={n_b} {jac} sigma={sigma is not None}", jac=jac, sigma=sigma)


def test_long_fits_at_five_per_cent_noise(gpu):
    """4 096 voxels at 5 % noise with up to 250 evaluations: some voxels run to the limit, and their waves finish as teams."""
    import torch
    from pyneapple_amd import synth

    dev = torch.device("cuda", 0)
    b, y = synth.make_torch("tri_reduced", 4096, 32, dev, sigma=0.05, seed=77)
    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    r = both("tri_reduced", y, b, p0, lo, hi, "4096 voxels, 5 % noise", max_nfev=250)
    assert r["nfev"].max() >= 100  # the batch does hold long fits


def test_sentinel_paths_from_a_team(gpu):
    """The lone voxel of the second wave has a non-finite signal value (status -2, detected in its first row pass, which a team
    runs), or a start value outside its bounds (-3, refused before any pass); per-voxel start values and bounds."""
    import torch
    from pyneapple_amd import synth

    dev = torch.device("cuda", 0)
    n_vox = 65
    b, y = synth.make_torch("tri_reduced", n_vox, 32, dev, sigma=0.01, seed=9)
    _, p0s, los, his = synth.shared_arrays("tri_reduced")
    p0, lo, hi = (torch.from_numpy(np.repeat(a[:, None], n_vox, axis=1)).to(dev).contiguous() for a in (p0s, los, his))
    y_nan = y.clone()
    y_nan[64, 17] = float("nan")
    y_nan[3, 0] = float("inf")
    r = both("tri_reduced", y_nan, b, p0, lo, hi, "non-finite signal")
    assert r["status"][64] == -2 and r["status"][3] == -2 and r["nfev"][64] == 0 and np.isnan(r["cost"][64])
    np.testing.assert_array_equal(r["popt"][:, 64], p0s)
    assert (r["status"][np.r_[0:3, 4:64]] > 0).all()
    p0_out = p0.clone()
    p0_out[1, 64] = 0.75  # D1 above its upper bound of 0.5
    r = both("tri_reduced", y, b, p0_out, lo, hi, "p0 outside its bounds")
    assert r["status"][64] == -3 and r["nfev"][64] == 0 and (r["status"][:64] > 0).all()


def test_single_voxel_against_the_oracle(gpu, oracle):
    """One tri-exponential voxel -- a team from the first evaluation on -- against the oracle, under the tolerances of
    test_gpu_curvefit.py (rtol 1e-4 per parameter, cost 1e-5, same evaluation count)."""
    import torch
    from pyneapple_amd import synth

    dev = torch.device("cuda", 0)
    b, y, _ = synth.make_numpy("tri_reduced", 1, 32, sigma=0.01, seed=123)
    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    for jac in ("fd", "analytic"):
        r = both("tri_reduced", torch.from_numpy(y).to(dev), b, p0, lo, hi, f"one voxel {jac}", jac=jac)
        o = oracle.curvefit("tri_reduced", b, y, p0, lo, hi, jac=jac, n_threads=1)
        assert r["status"][0] > 0 and o["status"][0] > 0
        np.testing.assert_allclose(r["popt"], o["popt"], rtol=1e-4)
        np.testing.assert_allclose(r["cost"], o["cost"], rtol=1e-5, atol=1e-300)
        assert r["nfev"][0] == o["nfev"][0]


def golden_case(name):
    """Inputs of the two cases whose results were recorded from the build before the team mode."""
    from pyneapple_amd import synth

    if name == "tri_s0":  # six free parameters: an instantiation that keeps the old loop
        b, y, _ = synth.make_numpy("tri_reduced", 300, 32, sigma=0.01, seed=21)
        _, p0, lo, hi = synth.shared_arrays("tri_reduced")
        return "tri_s0", b, y * 1000.0, np.append(p0, 1000.0), np.append(lo, 1.0), np.append(hi, 5000.0)
    b, y, _ = synth.make_numpy("tri_reduced", 2500, 32, sigma=0.01, seed=22)  # host arrays: the streamed kernel
    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    return "tri_reduced", b, y, p0, lo, hi


def run_golden_case(api, name):
    model, b, y, p0, lo, hi = golden_case(name)
    return api.curvefit(model, b, y, p0, lo, hi, want_pcov=(name == "tri_s0"))


@pytest.mark.parametrize("name", ["tri_s0", "streamed"])
def test_instantiations_without_the_mode_equal_the_parent_build(gpu, monkeypatch, capfd, name):
    """A 6-parameter fit and a streamed host-array call skip the mode but share the rewritten loop: bit for bit the results the
    build before this change gave (tests/golden/curvefit_team_parent.npz, recorded on an MI355X)."""
    if name == "streamed":
        monkeypatch.setenv("PNX_STREAM_GRANULE_SHIFT", "10")
        monkeypatch.setenv("PNX_STREAM_IN_CHUNK", "1024")
        monkeypatch.setenv("PNX_HOST_TRACE", "1")
        capfd.readouterr()
    r = run_golden_case(gpu, name)
    if name == "streamed":
        assert "[pnx stream]" in capfd.readouterr().err
    want = np.load(GOLDEN)
    for k in ("popt", "status", "nfev", "cost") + (("pcov",) if name == "tri_s0" else ()):
        np.testing.assert_array_equal(r[k], want[f"{name}_{k}"], err_msg=k)

"""Prediction and goodness of fit on the device: pnx_nnls_fit_stats_f64, pnx_nnls_solve_peaks_stats_f64,
pnx_curvefit_predict_f64 and the fitter keywords built on them, against numpy restatements of the reference's formulas
(model_functions/multiexp.py:35-241, fitters/base.py:142-186).

Bounds (derived, not tuned):
  * NNLS prediction: every term of B x is non-negative, so |pred - ref| <= gamma_n ref with gamma_n ~ n_bins 1.1e-16 <= 5.7e-14 for
    either summation order: rtol 1e-12.
  * ss_res = sum (y - pred)^2: the same error pushed through the square,
    |ss - ref| <= 2e-12 ||pred||_2 (sqrt(ref) + 1e-12 ||pred||_2).
  * model prediction: 2 ulp per exp plus three roundings per term, with a 100x margin: 1e-13 sum_c |w_c| (w_c the amplitudes,
    times the relaxation factor), which also covers the cancellation when 1 - f1 - f2 < 0.
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import load_golden, many_fixed_cases

pytestmark = pytest.mark.gpu

N_PARAMS = {"mono": 2, "bi_reduced": 3, "bi_s0": 4, "bi_full": 4, "tri_reduced": 5, "tri_s0": 6, "tri_full": 6}
TR, TM = 3000.0, 30.0


def ss_bound(pred, ss_ref):
    npred = np.sqrt((pred ** 2).sum(axis=1))
    return 2e-12 * npred * (np.sqrt(ss_ref) + 1e-12 * npred)


# ---------------------------------------------------------------------------------------------- NNLS stats
def _sparse_spectra(rng, n_vox, n_bins):
    x = np.zeros((n_vox, n_bins))
    for i in range(n_vox):
        k = int(rng.integers(3, 41))
        idx = rng.choice(n_bins, size=min(k, n_bins), replace=False)
        x[i, idx] = rng.uniform(0.0, 1000.0, idx.size)
    return x


@pytest.mark.parametrize("n_bins", [50, 250, 256, 257, 300, 512])
@pytest.mark.parametrize("n_meas", [1, 3, 16, 23, 32, 33, 128])
def test_nnls_fit_stats(gpu, n_meas, n_bins):
    import torch

    rng = np.random.default_rng(1000 * n_meas + n_bins)
    b = np.linspace(0.0, 1000.0, n_meas)
    bins = np.logspace(-4, -0.5, n_bins)
    basis = np.exp(-b[:, None] * bins[None, :])
    plan = gpu.NnlsPlan(basis, None, 0)
    dev = torch.device("cuda", 0)
    try:
        for n_vox in (1, 15, 16, 17, 1000):
            x = _sparse_spectra(rng, n_vox, n_bins)
            ref = x @ basis.T
            y = ref + rng.normal(0.0, 5.0, ref.shape)
            ss_ref = ((y - ref) ** 2).sum(axis=1)
            r = plan.fit_stats(y, x, want_pred=True)
            print(f"n_vox={n_vox} n_meas={n_meas} n_bins={n_bins}: max rel pred err {np.abs(r['pred'] / ref - 1).max():.3e}, "
                  f"max ss err / bound {(np.abs(r['ss_res'] - ss_ref) / ss_bound(ref, ss_ref)).max():.3e}")
            np.testing.assert_allclose(r["pred"], ref, rtol=1e-12, atol=0)
            assert (np.abs(r["ss_res"] - ss_ref) <= ss_bound(ref, ss_ref)).all()
            only = plan.fit_stats(y, x)
            assert only["pred"] is None
            np.testing.assert_array_equal(only["ss_res"], r["ss_res"])
            np.testing.assert_array_equal(plan.fit_stats(None, x, want_pred=True)["pred"], r["pred"])
            d = plan.fit_stats(torch.from_numpy(y).to(dev), torch.from_numpy(x).to(dev), want_pred=True)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(d["pred"].cpu().numpy(), r["pred"])  # host and device pointer modes: bit for bit
            np.testing.assert_array_equal(d["ss_res"].cpu().numpy(), r["ss_res"])
    finally:
        plan.close()


def test_nnls_fit_stats_host_arrays_in_chunks(gpu, monkeypatch):
    """A host-array call larger than a chunk goes through the ring: same bits as the one-chunk call."""
    rng = np.random.default_rng(7)
    b = np.linspace(0.0, 1000.0, 32)
    basis = np.exp(-b[:, None] * np.logspace(-4, -0.5, 250)[None, :])
    x = _sparse_spectra(rng, 5000, 250)
    y = x @ basis.T + rng.normal(0.0, 5.0, (5000, 32))
    plan = gpu.NnlsPlan(basis, None, 0)
    try:
        one = plan.fit_stats(y, x, want_pred=True)
        monkeypatch.setenv("PNX_STATS_HOST_CHUNK", "1024")
        many = plan.fit_stats(y, x, want_pred=True)
    finally:
        plan.close()
    np.testing.assert_array_equal(many["pred"], one["pred"])
    np.testing.assert_array_equal(many["ss_res"], one["ss_res"])


# ---------------------------------------------------------------------------------------------- chained path
def _reg2(n, mu=0.02):
    return (np.diag(np.ones(n - 1), -1) + np.diag(np.full(n, -2.0)) + np.diag(np.ones(n - 1), 1)) * mu


@pytest.mark.parametrize("fixture", ["g9_spectrum_nnls_250_r2_h0p1", "g11_spectrum_nnls_512_r2_h0p1"])
def test_solve_peaks_with_ss_res(gpu, fixture, monkeypatch):
    d = load_golden(fixture)
    bins, spec = d["bins"], np.maximum(d["spectrum"], 0.0)
    rng = np.random.default_rng(3)
    b = np.linspace(0.0, 1000.0, 32)
    basis = np.exp(-b[:, None] * bins[None, :])
    y = spec @ basis.T
    y = y + rng.normal(0.0, 0.002 * np.abs(y).max(), y.shape)
    plan = gpu.NnlsPlan(basis, _reg2(bins.size), 0)
    kw = dict(max_iter=250, height=float(d["height"]), regularized=bool(d["regularized"]), max_peaks=8, cutoffs=d["cutoffs"])
    try:
        plain = plan.solve_peaks(y, bins, **kw)
        full = plan.solve(y, 250)
        for chunk in (str(1 << 20), "1024"):  # one chunk, then the ring (the fixtures have 64 voxels: the ring's smallest chunk holds them)
            monkeypatch.setenv("PNX_NNLS_PEAKS_CHUNK", chunk)
            r = plan.solve_peaks(y, bins, with_ss_res=True, **kw)
            for k in plain:
                if plain[k] is not None:
                    np.testing.assert_array_equal(r[k], plain[k], err_msg=k)
            pred = full["coefficients"] @ basis.T
            ss_ref = ((y - pred) ** 2).sum(axis=1)
            with np.errstate(invalid="ignore"):  # an all-zero spectrum: 0 / 0
                print(fixture, "max ss err / bound", np.nanmax(np.abs(r["ss_res"] - ss_ref) / ss_bound(pred, ss_ref)))
            assert (np.abs(r["ss_res"] - ss_ref) <= ss_bound(pred, ss_ref)).all()
            # not rnorm^2: that one contains the regulariser rows
            assert (r["ss_res"] <= plain["residual"] ** 2 * (1 + 1e-9)).all()
    finally:
        plan.close()


def test_fit_peaks_r_squared(gpu):
    from pyneapple_amd import synth
    from pyneapple_amd.models import NNLSModel
    from pyneapple_amd.solvers import HipNNLSSolver

    b, y, _ = synth.make_numpy("tri_reduced", 300, 32, sigma=0.01, seed=4, scale=1000.0)
    y = np.ascontiguousarray(y, np.float64)
    y[17, :] = 250.0  # a constant signal row: SS_tot = 0
    model = NNLSModel(d_range=(0.0008, 0.5), n_bins=250)
    a = HipNNLSSolver(model=model, reg_order=2, mu=0.02, max_iter=250).fit_peaks(b, y, height=0.1)
    assert "r_squared" not in a.diagnostics_ and "ss_res" not in a.diagnostics_
    f = HipNNLSSolver(model=model, reg_order=2, mu=0.02, max_iter=250).fit_peaks(b, y, height=0.1, r_squared=True)
    for k in ("n_peaks", "d_values", "f_values"):
        np.testing.assert_array_equal(f.params_[k], a.params_[k])
    r2 = f.diagnostics_["r_squared"]
    assert np.isnan(r2[17]) and np.isfinite(np.delete(r2, 17)).all()
    full = HipNNLSSolver(model=model, reg_order=2, mu=0.02, max_iter=250).fit(b, y)
    pred = full.params_["coefficients"] @ np.asarray(model.get_basis(b)).T
    ss_ref = ((y - pred) ** 2).sum(axis=1)
    assert (np.abs(f.diagnostics_["ss_res"] - ss_ref) <= ss_bound(pred, ss_ref)).all()
    ss_tot = ((y - y.mean(axis=1, keepdims=True)) ** 2).sum(axis=1)
    keep = np.arange(300) != 17
    np.testing.assert_allclose(r2[keep], 1.0 - ss_ref[keep] / ss_tot[keep], rtol=0, atol=1e-10)
    assert np.median(r2[keep]) > 0.99


# ---------------------------------------------------------------------------------------------- model predict
def _forward(model, x, P, t1_mode):
    """(pred (n_vox, n_x), sum_c |w_c| * relaxation (n_vox, 1)): the reference's formulas, restated.  P (n_all, n_vox)."""
    e = lambda D: np.exp(-x[None, :] * D[:, None])
    c = lambda v: v[:, None]
    if model == "mono":
        terms = [(c(P[0]), e(P[1]))]
    elif model == "bi_reduced":
        terms = [(c(P[0]), e(P[1])), (c(1 - P[0]), e(P[2]))]
    elif model == "bi_s0":
        terms = [(c(P[3] * P[0]), e(P[1])), (c(P[3] * (1 - P[0])), e(P[2]))]
    elif model == "bi_full":
        terms = [(c(P[0]), e(P[1])), (c(P[2]), e(P[3]))]
    elif model == "tri_reduced":
        terms = [(c(P[0]), e(P[1])), (c(P[2]), e(P[3])), (c(1 - P[0] - P[2]), e(P[4]))]
    elif model == "tri_s0":
        terms = [(c(P[5] * P[0]), e(P[1])), (c(P[5] * P[2]), e(P[3])), (c(P[5] * (1 - P[0] - P[2])), e(P[4]))]
    else:
        terms = [(c(P[0]), e(P[1])), (c(P[2]), e(P[3])), (c(P[4]), e(P[5]))]
    fac = 1.0
    if t1_mode:
        T1 = c(P[N_PARAMS[model]])
        fac = (1 - np.exp(-TR / T1)) * (np.exp(-TM / T1) if t1_mode == 2 else 1.0)
    pred = sum(w * E for w, E in terms) * fac
    return pred, sum(np.abs(w) for w, _ in terms) * np.abs(fac)


def _random_params(rng, model, t1_mode, n_vox):
    names = {"mono": "SD", "bi_reduced": "fDD", "bi_s0": "fDDS", "bi_full": "fDfD", "tri_reduced": "fDfDD", "tri_s0": "fDfDDS",
             "tri_full": "fDfDfD"}[model] + ("T" if t1_mode else "")
    draw = {"f": lambda: rng.uniform(0.0, 0.8, n_vox), "D": lambda: 10 ** rng.uniform(-4, -1, n_vox),
            "S": lambda: rng.uniform(500.0, 1500.0, n_vox), "T": lambda: rng.uniform(500.0, 3000.0, n_vox)}
    return np.stack([draw[ch]() for ch in names])  # f1 + f2 may exceed 1: the cancellation case of the bound


PREDICT_CASES = [(m, t) for m in N_PARAMS for t in (0, 1)] + [("bi_s0", 2)]


@pytest.mark.parametrize("model,t1_mode", PREDICT_CASES)
def test_model_predict(gpu, model, t1_mode):
    import torch

    rng = np.random.default_rng(17 * len(model) + t1_mode)
    dev = torch.device("cuda", 0)
    kw = dict(t1_mode=t1_mode, tr=TR if t1_mode else 0.0, tm=TM if t1_mode == 2 else 0.0)
    n_all = N_PARAMS[model] + (1 if t1_mode else 0)
    for n_x in (1, 5, 23, 32, 128):
        x = np.sort(rng.uniform(0.0, 1200.0, n_x))  # not a fitted b-value set
        for n_vox in (1, 63, 64, 65, 1000):
            P = _random_params(rng, model, t1_mode, n_vox)
            # no fixed parameter / a scalar one / a per-voxel map, in turn
            variant = (n_x + n_vox) % 3
            fixed_idx = [] if variant == 0 else [1]
            free = [i for i in range(n_all) if i not in fixed_idx]
            Pv = P.copy()
            if variant == 1:
                Pv[1] = P[1, 0]
            ref, scale = _forward(model, x, Pv, t1_mode)
            # noise of 1 % of the row's own rms: the ss_res bound is the prediction's error pushed through the square, it
            # presumes a residual that is small against the prediction (as y = B x + noise is for the NNLS cases)
            y = ref + rng.normal(0.0, 0.01, ref.shape) * np.sqrt((ref ** 2).mean(axis=1, keepdims=True))
            ss_ref = ((ref - y) ** 2).sum(axis=1)
            fv = None if variant == 0 else (np.array([Pv[1, 0]]) if variant == 1 else np.ascontiguousarray(Pv[[1]]))
            r = gpu.predict(model, x, np.ascontiguousarray(Pv[free]), fixed_idx=fixed_idx, fixed_vals=fv, y=y, **kw)
            err = np.abs(r["pred"] - ref) / scale
            assert err.max() <= 1e-13, (model, t1_mode, n_x, n_vox, variant, err.max())
            assert (np.abs(r["ss_res"] - ss_ref) <= ss_bound(ref, ss_ref)).all(), (model, n_x, n_vox)
            # want_pred=False leaves a caller's pred buffer alone and gives the same residual
            sentinel = np.full((n_vox, n_x), -7.25)
            out = {"pred": sentinel}
            q = gpu.predict(model, x, np.ascontiguousarray(Pv[free]), fixed_idx=fixed_idx, fixed_vals=fv, y=y, want_pred=False, out=out, **kw)
            assert q["pred"] is None and (sentinel == -7.25).all()
            np.testing.assert_array_equal(q["ss_res"], r["ss_res"])
            # device pointers: same bits
            fvd = torch.from_numpy(fv).to(dev) if variant == 2 else fv
            t = gpu.predict(model, x, torch.from_numpy(np.ascontiguousarray(Pv[free])).to(dev), fixed_idx=fixed_idx, fixed_vals=fvd,
                            y=torch.from_numpy(y).to(dev), **kw)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(t["pred"].cpu().numpy(), r["pred"])
            np.testing.assert_array_equal(t["ss_res"].cpu().numpy(), r["ss_res"])


def test_model_predict_device_buffer_is_not_touched_without_want_pred(gpu):
    """The C entry point with pred = NULL writes ss_res only: a device buffer placed where pred would go keeps its sentinel."""
    import ctypes as C

    import torch

    from pyneapple_amd import _lib

    rng = np.random.default_rng(5)
    dev = torch.device("cuda", 0)
    n_vox, n_x = 130, 23
    x = np.linspace(0.0, 1000.0, n_x)
    P = _random_params(rng, "tri_s0", 0, n_vox)
    ref, _ = _forward("tri_s0", x, P, 0)
    y = ref + rng.normal(0.0, 1.0, ref.shape)
    buf = torch.full((n_vox * n_x + n_vox,), -7.25, dtype=torch.float64, device=dev)
    ss = buf[n_vox * n_x:]
    o = gpu.make_opts("tri_s0", n_x, jac="analytic")
    pd, yd = torch.from_numpy(P).to(dev), torch.from_numpy(y).to(dev)
    torch.cuda.synchronize()
    _lib.check(_lib.load().pnx_curvefit_predict_f64(C.byref(o), n_vox, n_x, _lib.ptr(x), _lib.ptr(pd), None, _lib.ptr(yd), None,
                                                    _lib.ptr(ss), _lib.MEM_DEVICE, 0, None))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:n_vox * n_x] == -7.25).all()
    ss_ref = ((ref - y) ** 2).sum(axis=1)
    assert (np.abs(got[n_vox * n_x:] - ss_ref) <= ss_bound(ref, ss_ref)).all()


def test_model_predict_many_fixed_shapes(gpu):
    """The per-voxel fixed layouts of SegmentedFitter's second step (conftest.many_fixed_cases), scalar and per voxel."""
    for d, model, free, fixed, maps, _ in many_fixed_cases():
        x = np.asarray(d["bvalues"], float)
        n_vox = maps.shape[1]
        rng = np.random.default_rng(n_vox)
        P = _random_params(rng, model, 0, n_vox)
        P[fixed] = maps
        ref, scale = _forward(model, x, P, 0)
        r = gpu.predict(model, x, np.ascontiguousarray(P[free]), fixed_idx=fixed, fixed_vals=np.ascontiguousarray(maps))
        assert (np.abs(r["pred"] - ref) / scale).max() <= 1e-13 and r["ss_res"] is None
        P[fixed] = maps[:, :1]
        ref, scale = _forward(model, x, P, 0)
        r = gpu.predict(model, x, np.ascontiguousarray(P[free]), fixed_idx=fixed, fixed_vals=np.ascontiguousarray(maps[:, 0]))
        assert (np.abs(r["pred"] - ref) / scale).max() <= 1e-13


def test_predict_refuses_more_than_128_x_values_in_the_library(gpu):
    import ctypes as C

    from pyneapple_amd import _lib

    o = gpu.make_opts("mono", 16)
    one = np.zeros(400)
    rc = _lib.load().pnx_curvefit_predict_f64(C.byref(o), 1, 129, _lib.ptr(one), _lib.ptr(one), None, None, _lib.ptr(one), None, 0, 0, None)
    assert rc == -1 and "n_x" in _lib.last_error()


# ---------------------------------------------------------------------------------------------- fitters
def _volume(rng, b):
    f1 = rng.uniform(0.1, 0.5, (16, 16, 2))
    D1 = rng.uniform(0.01, 0.05, (16, 16, 2))
    D2 = rng.uniform(5e-4, 3e-3, (16, 16, 2))
    img = 1000.0 * (f1[..., None] * np.exp(-b * D1[..., None]) + (1 - f1[..., None]) * np.exp(-b * D2[..., None]))
    img += rng.normal(0.0, 2.0, img.shape)
    seg = np.zeros((16, 16, 2), int)
    seg[2:13, 3:15, :] = 1
    return img, seg


def _same_fit(a, b):
    np.testing.assert_array_equal(a.success, b.success)
    for k in a.params:
        np.testing.assert_array_equal(a.params[k], b.params[k])
    if a.residuals is None:
        assert b.residuals is None
    else:
        np.testing.assert_array_equal(a.residuals, b.residuals)
    np.testing.assert_allclose(b.r_squared, a.r_squared, rtol=0, atol=1e-10, equal_nan=True)


@pytest.mark.parametrize("max_iter", [250, 1])
def test_pixelwise_fitter_device_stats_curvefit(gpu, max_iter):
    from pyneapple_amd.fitters import HipPixelWiseFitter
    from pyneapple_amd.models import BiExpModel
    from pyneapple_amd.solvers import HipCurveFitSolver

    rng = np.random.default_rng(11)
    b = np.linspace(0.0, 1000.0, 16)
    img, seg = _volume(rng, b)
    img = img / 1000.0
    mk = lambda: HipCurveFitSolver(model=BiExpModel(), max_iter=max_iter, tol=1e-8, p0={"f1": 0.2, "D1": 0.02, "D2": 0.001},
                                   bounds={"f1": (0.0, 1.0), "D1": (5e-3, 0.5), "D2": (1e-5, 5e-3)})
    ref = HipPixelWiseFitter(mk()).fit(b, img, segmentation=seg)
    dev = HipPixelWiseFitter(mk(), device_stats=True).fit(b, img, segmentation=seg)
    assert dev.device_stats and not ref.device_stats
    if max_iter == 1:  # every voxel returns p0: its R^2 comes from the predict kernel
        assert not ref.results_.success.all() and np.isfinite(dev.results_.r_squared).all()
    else:
        assert ref.results_.success.all()
    _same_fit(ref.results_, dev.results_)
    x = np.linspace(0.0, 800.0, 23)
    p_host, p_dev = ref.predict(x), dev.predict(x, on_device=True)
    assert p_dev.shape == (16, 16, 2, 23) and (p_dev[seg == 0] == 0).all()
    np.testing.assert_allclose(p_dev, p_host, rtol=0, atol=1e-13 * 2.0)  # amplitudes f1 + (1 - f1) <= 1, both sides within 1e-13
    np.testing.assert_array_equal(dev.predict(x), p_host)


def test_pixelwise_fitter_device_stats_nnls(gpu):
    from pyneapple_amd.fitters import HipPixelWiseFitter
    from pyneapple_amd.models import NNLSModel
    from pyneapple_amd.solvers import HipNNLSSolver

    rng = np.random.default_rng(12)
    b = np.linspace(0.0, 1000.0, 16)
    img, seg = _volume(rng, b)
    mk = lambda: HipNNLSSolver(model=NNLSModel(d_range=(1e-4, 0.1), n_bins=50), reg_order=2, mu=0.02)
    ref = HipPixelWiseFitter(mk()).fit(b, img, segmentation=seg)
    dev = HipPixelWiseFitter(mk(), device_stats=True).fit(b, img, segmentation=seg)
    _same_fit(ref.results_, dev.results_)
    assert ref.results_.mean_r_squared > 0.99
    x = np.linspace(0.0, 800.0, 23)
    p_host, p_dev = ref.predict(x), dev.predict(x, on_device=True)
    assert (p_dev[seg == 0] == 0).all()
    np.testing.assert_allclose(p_dev, p_host, rtol=1e-12, atol=0)

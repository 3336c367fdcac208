"""The fp32-arithmetic curve fit (pnx_curvefit_fast_f32) on the GPU.  Its results are not SciPy-parity results; what they owe the
user is a minimum as good as float32 arithmetic allows, and that is defined by tests/golden/f32_yardstick.json: the reference
algorithm (SciPy TRF, fp64 linear algebra) on a float32 model (tools/f32_yardstick.py).  Bars, per fixture, against the recorded
values: cost excess <= 4 x recorded on every successful voxel (the kernel's fast exp, its FMA contraction and its fp32 small
linear algebra each add an error of the order the yardstick already contains), parameter share within 1e-3 >= recorded - 0.05,
success-flag share >= recorded - 0.02.  Every figure is printed before it is asserted (pytest -s shows them)."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import pytest
from conftest import GOLDEN, ROOT, golden_p0_bounds, load_golden

sys.path.insert(0, os.path.join(ROOT, "tools"))
import f32_yardstick as Y  # noqa: E402  (model evaluation in numpy + the yardstick's definitions)

from pyneapple_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
YARD = json.load(open(os.path.join(GOLDEN, "f32_yardstick.json")))["fixtures"]
MARGIN = 4.0


def _fit32(gpu, model, b, y, p0, lo, hi, **kw):
    return gpu.curvefit(model, b, y, p0, lo, hi, precision="float32", **kw)


def _check_fixture(gpu, name):
    d, rec, model = load_golden(name), YARD[name], Y.FIXTURES[name]
    p0, lo, hi = golden_p0_bounds(d)
    r = _fit32(gpu, model, d["bvalues"], d["y"], p0, lo, hi, max_nfev=int(d["max_iter"]), ftol=float(d["tol"]))
    assert r["popt"].dtype == np.float32 and r["pcov"].dtype == np.float32
    ok = r["status"] > 0
    P = r["popt"].T.astype(np.float64)
    ex = Y.cost_excess(model, d["bvalues"], d["y"], P, d["popt"])
    share_p = float(Y.param_within(P, d["popt"]).mean())
    share_s = float((ok == d["success"]).mean())
    print(f"\n[f32 {name}] cost_excess max {ex[ok].max():.4g} (yardstick {rec['cost_excess']:.4g}, bar {MARGIN * rec['cost_excess']:.4g}; "
          f"voxels over the bar {(ex[ok] > MARGIN * rec['cost_excess']).sum()} of {ok.sum()}, median {np.median(ex[ok]):.3g})  "
          f"param_share {share_p:.4f} (yardstick {rec['param_share']:.4f})  success_share {share_s:.4f} (yardstick {rec['success_share']:.4f})  "
          f"nfev mean {r['nfev'].mean():.1f} max {r['nfev'].max()}")
    assert ex[ok].max() <= MARGIN * rec["cost_excess"]
    if rec["param_criterion"]:
        assert share_p >= rec["param_share"] - 0.05
    assert share_s >= rec["success_share"] - 0.02
    if (~ok).any():
        assert np.isnan(r["pcov"][~ok]).all()


@pytest.mark.parametrize("name", sorted(n for n in Y.FIXTURES if not n.startswith("g5_")))
def test_fixtures_against_the_yardstick(gpu, name):
    """Measured on an MI355X (cost excess max / parameter share / success share; yardstick in brackets) -- see DESIGN.md."""
    _check_fixture(gpu, name)


@pytest.mark.parametrize("name", ["g5_bi_pervoxel", "g5_tri_pervoxel"])
def test_per_voxel_start_values_and_bounds(gpu, name):
    _check_fixture(gpu, name)


# ---- smallest shapes where the kernel can go wrong ---------------------------------------------------------------------
_SHAPE_MODELS = {"tri_reduced": "g3_tri_reduced", "mono": "g1_mono_b16"}


def _nb_cases(model):
    n = Y.N_PARAMS[model]
    return sorted({1, n - 1, n, n + 1, 23, 32, 33, 128})


@pytest.mark.parametrize("model,n_b", [(m, nb) for m in _SHAPE_MODELS for nb in _nb_cases(m)])
def test_shapes(gpu, model, n_b):
    n = Y.N_PARAMS[model]
    bar = MARGIN * YARD[_SHAPE_MODELS[model]]["cost_excess"]
    _, p0, lo, hi = synth.shared_arrays(model)
    for n_vox in (1, 63, 64, 65, 257):
        b, y, _ = synth.make_numpy(model, n_vox, n_b, sigma=0.01, seed=1000 + n_vox)
        r = _fit32(gpu, model, b, y, p0, lo, hi)
        st, P = r["status"], r["popt"].T.astype(np.float64)
        assert r["popt"].shape == (n, n_vox) and r["pcov"].shape == (n_vox, n, n) and st.shape == (n_vox,)
        assert np.isin(st, [1, 2, 3, 4, 0, -1, -2, -3, -4]).all()
        ok = st > 0
        lo32, hi32 = lo.astype(np.float32).astype(float), hi.astype(np.float32).astype(float)
        assert ((P[ok] >= lo32) & (P[ok] <= hi32)).all()
        y32 = y.astype(np.float32).astype(float)  # what the kernel was given
        c = Y.cost64(model, b, y32, P)
        c0 = Y.cost64(model, b, y32, np.tile(p0.astype(np.float32).astype(float), (n_vox, 1)))
        assert (c[ok] <= c0[ok] * (1 + 1e-6) + Y.cost_floor(y32)[ok]).all()
        assert (P[~ok] == p0.astype(np.float32)).all() and np.isnan(r["pcov"][~ok]).all()
        if n_b <= n:  # no degrees of freedom: curve_fit fills the covariance with inf
            assert np.isinf(r["pcov"][ok]).all()
        else:
            assert not np.isnan(r["pcov"][ok]).any()
        if n_b >= 2 * n:
            r64 = gpu.curvefit(model, b, y32, p0, lo, hi, jac="analytic")
            both = ok & (r64["status"] > 0)
            ex = Y.cost_excess(model, b, y32, P, r64["popt"].T)
            print(f"\n[f32 shapes {model} n_b={n_b} n_vox={n_vox}] ok {ok.mean():.3f} (fp64 {(r64['status'] > 0).mean():.3f}) "
                  f"cost excess vs fp64 max {ex[both].max() if both.any() else float('nan'):.4g} (bar {bar:.4g})")
            assert ok.mean() >= (r64["status"] > 0).mean() - 0.02
            assert (ex[both] <= bar).all()


def _other_model_case(model, n_vox=65, n_b=24):
    """Signals of the five models synth has no generator for, from its reduced ones: the same curves, re-parameterised."""
    base = "bi_reduced" if model.startswith("bi") else "tri_reduced"
    b, y, _ = synth.make_numpy(base, n_vox, n_b, sigma=0.01, seed=77)
    _, p0, lo, hi = synth.shared_arrays(base)
    p0, lo, hi = list(p0), list(lo), list(hi)
    if model.endswith("_s0"):
        y = 1000.0 * y
        p0, lo, hi = p0 + [900.0], lo + [1.0], hi + [5000.0]
    elif model == "bi_full":  # [f1, D1, f2, D2]
        p0, lo, hi = [p0[0], p0[1], 1 - p0[0], p0[2]], [lo[0], lo[1], 0.0, lo[2]], [hi[0], hi[1], 1.0, hi[2]]
    elif model == "tri_full":  # [f1, D1, f2, D2, f3, D3]
        p0, lo, hi = p0[:4] + [1 - p0[0] - p0[2], p0[4]], lo[:4] + [0.0, lo[4]], hi[:4] + [1.0, hi[4]]
    return b, y, np.array(p0), np.array(lo), np.array(hi)


@pytest.mark.parametrize("model", ["bi_reduced", "bi_s0", "bi_full", "tri_s0", "tri_full"])
def test_other_models(gpu, model):
    b, y, p0, lo, hi = _other_model_case(model)
    y32 = y.astype(np.float32).astype(float)
    r = _fit32(gpu, model, b, y, p0, lo, hi)
    r64 = gpu.curvefit(model, b, y32, p0, lo, hi, jac="analytic")
    ok, P = r["status"] > 0, r["popt"].T.astype(np.float64)
    both = ok & (r64["status"] > 0)
    ex = Y.cost_excess(model, b, y32, P, r64["popt"].T)
    fixture = {"bi_reduced": "g2_bi_reduced", "bi_s0": "g2_bi_s0", "bi_full": "g2_bi_full", "tri_s0": "g3_tri_s0", "tri_full": "g3_tri_full"}[model]
    bar = MARGIN * YARD[fixture]["cost_excess"]
    print(f"\n[f32 {model} 24 x 65] ok {ok.mean():.3f} (fp64 {(r64['status'] > 0).mean():.3f}) cost excess vs fp64 max {ex[both].max():.4g} (bar {bar:.4g})")
    assert ok.mean() >= (r64["status"] > 0).mean() - 0.02 and both.any()
    assert (ex[both] <= bar).all()
    assert ((P[ok] >= lo.astype(np.float32)) & (P[ok] <= hi.astype(np.float32))).all()


# ---- failure sentinels -------------------------------------------------------------------------------------------------
def _assert_sentinel(r, sel, p0, status):
    assert (r["status"][sel] == status).all(), r["status"][sel]
    assert (r["popt"].T[sel] == np.asarray(p0, np.float32)).all()
    assert np.isnan(r["pcov"][sel]).all()


def test_failure_sentinels(gpu):
    b, y, _ = synth.make_numpy("tri_reduced", 130, 32, sigma=0.01, seed=5)
    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    every = np.ones(130, bool)
    _assert_sentinel(_fit32(gpu, "tri_reduced", b, y, p0, lo, hi, max_nfev=1), every, p0, 0)
    bad_hi = hi.copy()
    bad_hi[1] = lo[1]
    _assert_sentinel(_fit32(gpu, "tri_reduced", b, y, p0, lo, bad_hi), every, p0, -1)
    out = p0.copy()
    out[3] = hi[3] * 2
    _assert_sentinel(_fit32(gpu, "tri_reduced", b, y, out, lo, hi), every, out, -3)
    yn = y.copy()
    yn[7, 3] = np.nan
    yn[64, 31] = np.inf
    r = _fit32(gpu, "tri_reduced", b, yn, p0, lo, hi)
    hit = np.zeros(130, bool)
    hit[[7, 64]] = True
    _assert_sentinel(r, hit, p0, -2)
    assert (r["status"][~hit] > 0).mean() > 0.95
    # per-voxel start values: the sentinel is the voxel's own p0
    p0v = np.tile(p0[:, None], (1, 130)) * np.linspace(0.95, 1.05, 130)
    lov, hiv = np.tile(lo[:, None], (1, 130)), np.tile(hi[:, None], (1, 130))
    p0v[0, 11] = 2.0  # outside [0, 1]
    r = _fit32(gpu, "tri_reduced", b, y, p0v, lov, hiv)
    assert r["status"][11] == -3 and (r["popt"][:, 11] == p0v[:, 11].astype(np.float32)).all() and np.isnan(r["pcov"][11]).all()


# ---- same-result equalities --------------------------------------------------------------------------------------------
def test_host_call_equals_device_resident_call(gpu):
    import torch

    from pyneapple_amd import api

    n_vox, n_b = 1000, 32
    b, y, _ = synth.make_numpy("tri_reduced", n_vox, n_b, sigma=0.01, seed=9)
    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    host = _fit32(gpu, "tri_reduced", b, y, p0, lo, hi)
    dev = torch.device("cuda", 0)
    yt = torch.from_numpy(y.astype(np.float32)).to(dev)
    popt = torch.empty((5, n_vox), dtype=torch.float32, device=dev)
    pcov = torch.empty((n_vox, 5, 5), dtype=torch.float32, device=dev)
    status = torch.empty(n_vox, dtype=torch.int8, device=dev)
    nfev = torch.empty(n_vox, dtype=torch.int32, device=dev)
    cost = torch.empty(n_vox, dtype=torch.float32, device=dev)
    o = api.make_opts("tri_reduced", n_b, jac="analytic")
    api.curvefit_device(o, n_vox, b, yt, p0, lo, hi, None, popt, pcov, status, nfev, cost, 0,
                        torch.cuda.current_stream(dev).cuda_stream, precision="float32")
    torch.cuda.synchronize(dev)
    for k, t in (("popt", popt), ("pcov", pcov), ("status", status), ("nfev", nfev), ("cost", cost)):
        np.testing.assert_array_equal(t.cpu().numpy(), host[k], err_msg=k)


def _solver(**extra):
    from pyneapple_amd.models import TriExpModel
    from pyneapple_amd.solvers import HipCurveFitSolver

    names, p0, lo, hi = synth.shared_arrays("tri_reduced")
    return names, HipCurveFitSolver(model=TriExpModel(), max_iter=250, tol=1e-8, p0=dict(zip(names, p0)),
                                    bounds={n: (l, h) for n, l, h in zip(names, lo, hi)}, precision="float32", **extra)


def test_plugin_and_two_shards_equal_one_device(gpu, monkeypatch):
    b, y, _ = synth.make_numpy("tri_reduced", 1001, 32, sigma=0.01, seed=13)
    names, s1 = _solver()
    s1.fit(b, y)
    assert set(s1.params_) == set(names)
    for n in names:
        assert s1.params_[n].dtype == np.float32 and s1.params_[n].shape == (1001,)
    dg = s1.diagnostics_
    assert dg["pcov"].dtype == np.float32 and dg["pcov"].shape == (1001, 5, 5) and dg["n_pixels"] == 1001
    assert dg["status"].shape == (1001,) and dg["nfev"].shape == (1001,) and dg["cost"].dtype == np.float32
    assert len(s1.pixel_results_) == 1001
    rec = s1.pixel_results_[0]
    assert np.asarray(rec.params if hasattr(rec, "params") else rec["params"]).shape == (5,)
    assert (dg["status"] > 0).mean() > 0.95
    monkeypatch.setenv("PNX_SHARE_DEVICE", "1")
    _, s2 = _solver(n_gpus=2)
    s2.fit(b, y)
    for n in names:
        np.testing.assert_array_equal(s2.params_[n], s1.params_[n], err_msg=n)
    for k in ("pcov", "status", "nfev", "cost"):
        np.testing.assert_array_equal(s2.diagnostics_[k], dg[k], err_msg=k)

"""pnx_curvefit_simplex_f64 on the GPU: the constrained fit f1 + f2 <= 1 of the reduced tri-exponential models.

Interior voxels are the box-only fit bit for bit; face voxels are checked against numpy (multiplier, stationarity along the
face) and against the oracle's bi-exponential fit of the same gathered inputs; the g13 fixtures against the reference's SLSQP
solver by cost.  Shapes: every block edge of the streaming kernels (64 voxels per wave) and the b-value counts at which the fit
kernel changes its row blocking (5, 6), an odd count (23, 33), the benchmark's 32 and the maximum 128."""
from __future__ import annotations

import numpy as np
import pytest
from conftest import load_golden

import constrained_reference as R
from pyneapple_amd import synth

pytestmark = pytest.mark.gpu

MAX_NFEV, TOL = 250, 1e-8
FIXTURE = dict(ftol=TOL, xtol=1e-8, gtol=1e-8, jac="fd")          # the reference's settings (SciPy defaults beside tol)
TIGHT = dict(ftol=1e-13, xtol=1e-13, gtol=1e-13, jac="analytic")  # a fit that ends at its minimum, not at a stopping rule


def _same(a, b):  # bit-identical, NaN payloads included
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check(gpu, oracle, model, b, y, p0, lo, hi, res, label="", max_nfev=MAX_NFEV, min_violators=None, fit=None):
    """Every property a result of the constrained fit has, against the box-only fit of the same inputs.  Returns the violators.
    fit: the tolerances and Jacobian mode of the call (TIGHT by default).  Stationarity along the face, |g_f1 - g_f2| <=
    1e-6 (|g_f1| + |g_f2|) + 1e-12, is a statement about a minimum: it is asserted for TIGHT fits and printed for FIXTURE
    ones, where TRF ends at its stopping rules -- measured on g13_tri_constrained_reduced with ftol = gtol = 1e-8:
    |g_f1 - g_f2| up to 1.2e-8 at multipliers of 2e-5 .. 2e-3, 9.5e-9 above the bound, on voxels whose parameters agree with
    the oracle's to 1e-9."""
    fit = fit or TIGHT
    n_vox = len(y)
    box = gpu.curvefit(model, b, y, p0, lo, hi, max_nfev=max_nfev, **fit)
    popt, face, lam = res["popt"], res["face"], res["lambda"]
    viol = (box["status"] > 0) & (box["popt"][0] + box["popt"][2] > 1.0)
    print(f"\n[{label}] {model} n_vox={n_vox} n_b={len(b)}: {int(viol.sum())} violators, face counts "
          f"{[int((face == k).sum()) for k in (0, 1, 2)]}, status<=0: {int((res['status'] <= 0).sum())}")
    if min_violators is not None:
        assert viol.sum() >= min_violators, (int(viol.sum()), min_violators)
    assert ((face > 0) == viol).all()
    inside = face == 0
    for key in ("pcov", "status", "nfev", "cost"):
        assert _same(res[key][inside], box[key][inside]), key
    assert _same(popt[:, inside], box["popt"][:, inside])
    assert (lam[inside] == 0).all()
    # feasibility and bounds, every voxel
    lo_a = lo if lo.ndim == 2 else lo[:, None]
    hi_a = hi if hi.ndim == 2 else hi[:, None]
    assert (popt[0] + popt[2] <= 1.0)[res["status"] > 0].all()
    assert ((popt >= lo_a) & (popt <= hi_a))[:, res["status"] > 0].all()
    on = np.flatnonzero(viol)
    if not len(on):
        return viol
    ok = on[res["status"][on] > 0]
    bad = on[res["status"][on] <= 0]
    assert (face[bad] == 2).all() and np.isnan(lam[bad]).all()
    assert np.isnan(res["pcov"][on]).all()
    assert (res["nfev"][on] >= box["nfev"][on]).all() and (res["nfev"][ok] > box["nfev"][ok]).all()  # both phases
    assert (popt[2, ok] == 1.0 - popt[0, ok]).all()
    assert _same(popt[4, ok], box["popt"][4, ok])
    if not len(ok):
        return viol
    # the multiplier, from the returned parameters
    g1, g2 = R.tri_grad_f(model, b, y[ok], popt[:, ok].T)
    lam_np = -0.5 * (g1 + g2)
    err = np.abs(lam[ok] - lam_np) - (1e-9 + 1e-6 * np.abs(lam_np))
    l0, h0 = R.face_bounds(lo_a, hi_a)
    l0, h0 = np.broadcast_to(l0, (n_vox,))[ok], np.broadcast_to(h0, (n_vox,))[ok]
    # "f1 sits on an intersected bound": TRF keeps its iterates strictly inside the box (SciPy moves a point 1e-10 max(1, |bound|)
    # off a bound) and approaches an active bound from inside, so "on" is within 1e-8 max(1, |bound|) -- a hundred such offsets,
    # the square root of the fp64 epsilon -- with the gradient along the face pointing out of the box (the KKT sign)
    gf = g1 - g2
    near = lambda bd: np.abs(popt[0, ok] - bd) <= 1e-8 * np.maximum(1.0, np.abs(bd))
    at_bound = (near(l0) & (gf >= 0)) | (near(h0) & (gf <= 0))
    stat = np.abs(g1 - g2) - (1e-6 * (np.abs(g1) + np.abs(g2)) + 1e-12)
    print(f"[{label}] lambda range [{lam[ok].min():.3e}, {lam[ok].max():.3e}], worst lambda excess {err.max():.3e}, "
          f"worst stationarity excess off the bounds {stat[~at_bound].max() if (~at_bound).any() else float('nan'):.3e}, "
          f"{int(at_bound.sum())} on an intersected bound, cost {np.nanmin(res['cost'][ok]):.3e}..{np.nanmax(res['cost'][ok]):.3e}")
    assert (err <= 0).all()
    assert ((face[ok] == 1) == (lam[ok] >= 0)).all() and ((face[ok] == 2) == (lam[ok] < 0)).all()
    # cost at the returned point: exp to 1 ulp on both sides, so 1e-9 relative plus the rounding of a residual of ||y||
    c_np = R.tri_cost(model, b, y[ok], popt[:, ok].T)
    assert (np.abs(res["cost"][ok] - c_np) <= 1e-9 * c_np + 1e-18 * (y[ok] ** 2).sum(axis=1)).all()
    # the face fit against the oracle's bi-exponential fit of the same gathered inputs
    rows = R.FACE_ROWS[model]
    f1, f2 = box["popt"][0, on], box["popt"][2, on]
    L0, H0 = R.face_bounds(lo_a, hi_a)
    L0, H0 = np.broadcast_to(L0, (n_vox,))[on], np.broadcast_to(H0, (n_vox,))[on]
    q0 = box["popt"][rows][:, on].copy()
    q0[0] = np.where(L0 < H0, np.clip(f1 / (f1 + f2), L0, H0), f1 / (f1 + f2))
    lo2 = np.ascontiguousarray(np.broadcast_to(lo_a[rows], (len(rows), n_vox))[:, on])
    hi2 = np.ascontiguousarray(np.broadcast_to(hi_a[rows], (len(rows), n_vox))[:, on])
    lo2[0], hi2[0] = L0, H0
    left = max(1, max_nfev - int(box["nfev"][on].min()))
    ref = oracle.curvefit(R.BI_OF_TRI[model], b, y[on], np.ascontiguousarray(q0), lo2, hi2, max_nfev=left, want_pcov=False, **fit)
    good = ref["status"] > 0
    assert (good == (res["status"][on] > 0)).all() and (ref["status"][~good] == res["status"][on][~good]).all()
    rel = np.abs(popt[rows][:, on][:, good] - ref["popt"][:, good]) / np.maximum(np.abs(ref["popt"][:, good]), 1e-300)
    print(f"[{label}] face fit against the oracle: worst relative difference {rel.max() if rel.size else 0.0:.3e}")
    assert (rel <= 1e-4).all()
    # stationarity along the face, asserted last so that everything above has been checked when it misses (module docstring)
    assert fit is FIXTURE or (stat[~at_bound] <= 0).all(), f"|g_f1 - g_f2| exceeds 1e-6 (|g_f1| + |g_f2|) + 1e-12 by up to {stat[~at_bound].max():.3e}"
    return viol


def _fit(gpu, model, b, y, p0, lo, hi, fit=None, **kw):
    return gpu.curvefit_constrained(model, b, y, p0, lo, hi, max_nfev=kw.pop("max_nfev", MAX_NFEV), **(fit or TIGHT), **kw)


# ---- fixtures against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g13_tri_constrained_reduced", "g13_tri_constrained_s0"])
def test_fixture_is_feasible_and_no_worse_than_the_reference(gpu, oracle, name):
    d = load_golden(name)
    model, b, y, p0, lo, hi = str(d["model"]), d["b"], d["y"], d["p0"], d["lo"], d["hi"]
    res = _fit(gpu, model, b, y, p0, lo, hi, FIXTURE, max_nfev=int(d["max_iter"]))
    popt = res["popt"]
    cost = R.tri_cost(model, b, y, popt.T)
    cost_ref = R.tri_cost(model, b, y, d["ref_popt"].T)
    rel = cost / cost_ref - 1.0
    print(f"\n{name}: face counts {[int((res['face'] == k).sum()) for k in (0, 1, 2)]}; cost / reference - 1: max {rel.max():+.3e}, "
          f"median {np.median(rel):+.3e}, min {rel.min():+.3e}; reference more than 10 % worse on {int((rel < -1 / 11).sum())} of "
          f"{len(y)}; reference successes {int(d['ref_success'].sum())}; status > 0 on {int((res['status'] > 0).sum())}")
    assert (popt[0] + popt[2] <= 1.0).all()
    assert ((popt >= lo[:, None]) & (popt <= hi[:, None])).all()
    assert (res["status"][d["ref_success"]] > 0).all()
    assert (cost <= cost_ref * (1 + 1e-5)).all(), np.flatnonzero(cost > cost_ref * (1 + 1e-5))
    viol = check(gpu, oracle, model, b, y, p0, lo, hi, res, name, max_nfev=int(d["max_iter"]), min_violators=10, fit=FIXTURE)
    assert (res["face"][viol] == 1).all()  # the method test (SciPy) certifies every face voxel of the fixtures


# ---- shapes ---------------------------------------------------------------------------------------------------------------
def _signals(n_vox, n_b, f3, seed, noise=0.01, f1=(0.3, 0.6)):
    rng = np.random.default_rng(seed)
    T = synth.TRUTH["tri_reduced"]
    # b = 0 and a geometric grid from 10 to 1200: every compartment is seen at any count.  On a uniform grid of 5 or 6 values the
    # first non-zero b is 240 .. 300, where the fast compartment (D1 >= 0.03) has decayed below 1e-3: f1 and D1 of the face fit
    # are then unidentifiable and any two TRF implementations -- SciPy and the oracle included -- stop at different points
    b = np.concatenate([[0.0], np.geomspace(10.0, 1200.0, n_b - 1)])
    f1 = rng.uniform(*f1, n_vox)
    f2 = 1.0 - f1 - f3
    D1, D2, D3 = (rng.uniform(*T[k], n_vox) for k in ("D1", "D2", "D3"))
    e = lambda D: np.exp(-b[None, :] * D[:, None])
    y = f1[:, None] * e(D1) + f2[:, None] * e(D2) + f3 * e(D3)
    return b, np.ascontiguousarray(y * (1.0 + noise * rng.standard_normal(y.shape)))


@pytest.mark.parametrize("n_b", [5, 6, 23, 32, 33, 128])
@pytest.mark.parametrize("n_vox", [1, 63, 64, 65, 257])
def test_shapes(gpu, oracle, n_vox, n_b):
    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    # case 1: no violator can exist (hi_f1 + hi_f2 < 1): phase 2 is skipped, the whole result is the box-only fit
    b, y = _signals(n_vox, n_b, 0.3, 100 * n_vox + n_b)
    hi1 = hi.copy()
    hi1[[0, 2]] = 0.45
    res = _fit(gpu, "tri_reduced", b, y, p0, lo, hi1)
    box = gpu.curvefit("tri_reduced", b, y, p0, lo, hi1, max_nfev=MAX_NFEV, **TIGHT)
    for key in ("popt", "pcov", "status", "nfev", "cost"):
        assert _same(res[key], box[key]), key
    assert (res["face"] == 0).all() and (res["lambda"] == 0).all()
    # case 2: signals with f3 = -0.1: most box-only minima are infeasible
    b, y = _signals(n_vox, n_b, -0.1, 200 * n_vox + n_b)
    res = _fit(gpu, "tri_reduced", b, y, p0, lo, hi)
    viol = check(gpu, oracle, "tri_reduced", b, y, p0, lo, hi, res, "most")
    assert viol.mean() > 0.5, viol.mean()
    # case 3: exactly one violator, at the last index (per-voxel bounds keep every other voxel below f1 + f2 = 0.9)
    b, y = _signals(n_vox, n_b, 0.3, 300 * n_vox + n_b)
    y[-1] = _signals(1, n_b, -0.1, 7, noise=0.0)[1][0]
    P0, LO, HI = (np.ascontiguousarray(np.repeat(a[:, None], n_vox, axis=1)) for a in (p0, lo, hi1))
    HI[:, -1] = hi
    res = _fit(gpu, "tri_reduced", b, y, P0, LO, HI)
    viol = check(gpu, oracle, "tri_reduced", b, y, P0, LO, HI, res, "last")
    assert viol.sum() == 1 and viol[-1]


@pytest.mark.parametrize("model", ["tri_reduced", "tri_s0"])
def test_per_voxel_bounds_intersect_and_an_empty_intersection_fails(gpu, oracle, model):
    n_vox, n_b = 130, 32
    b, y = _signals(n_vox, n_b, -0.1, 41, f1=(0.45, 0.75))
    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    if model == "tri_s0":
        y, p0, lo, hi = y * 1000.0, np.append(p0, 900.0), np.append(lo, 1.0), np.append(hi, 5000.0)
    P0, LO, HI = (np.ascontiguousarray(np.repeat(a[:, None], n_vox, axis=1)) for a in (p0, lo, hi))
    HI[2] = 0.5  # f2 <= 0.5: on the face f1 >= 0.5
    # voxel 3: lo_f1 = 0.5 and lo_f2 = 0.6 force f1 + f2 >= 1.1, and [max(0.5, 1 - 1), min(1, 1 - 0.6)] is empty
    LO[0, 3], LO[2, 3], HI[2, 3], P0[0, 3], P0[2, 3] = 0.5, 0.6, 1.0, 0.6, 0.7
    res = _fit(gpu, model, b, y, P0, LO, HI)
    viol = check(gpu, oracle, model, b, y, P0, LO, HI, res, "hi_f2=0.5", min_violators=n_vox // 2)
    assert viol[3] and res["status"][3] == -1 and res["face"][3] == 2 and np.isnan(res["lambda"][3])
    assert _same(res["popt"][:, 3], P0[:, 3]) and np.isnan(res["pcov"][3]).all()
    ok = viol & (res["status"] > 0)
    assert (res["popt"][0, ok] >= 0.5).all() and (res["popt"][0, ok] <= 0.5 + 1e-8).any()  # the intersected bound is active somewhere


# ---- same result on every route -------------------------------------------------------------------------------------------
def test_host_call_equals_device_resident_call(gpu):
    import torch

    for name, per_voxel in (("g13_tri_constrained_reduced", False), ("g13_tri_constrained_s0", True)):
        d = load_golden(name)
        model, b, y, p0, lo, hi = str(d["model"]), d["b"], d["y"], d["p0"], d["lo"], d["hi"]
        n_vox, n = len(y), len(p0)
        if per_voxel:
            p0, lo, hi = (np.ascontiguousarray(np.repeat(a[:, None], n_vox, axis=1)) for a in (p0, lo, hi))
        host = _fit(gpu, model, b, y, p0, lo, hi, FIXTURE)
        dev = torch.device("cuda", 0)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        out = dict(popt=e((n, n_vox), torch.float64), pcov=e((n_vox, n, n), torch.float64), status=e(n_vox, torch.int8),
                   nfev=e(n_vox, torch.int32), cost=e(n_vox, torch.float64))
        out["lambda"], out["face"] = e(n_vox, torch.float64), e(n_vox, torch.int8)
        o = gpu.make_opts(model, len(b), per_voxel=per_voxel, max_nfev=MAX_NFEV, ftol=TOL, jac="fd")
        args = (t(p0), t(lo), t(hi)) if per_voxel else (p0, lo, hi)
        gpu.curvefit_constrained_device(o, n_vox, b, t(y), *args, out["popt"], out["pcov"], out["status"], out["nfev"], out["cost"],
                                        out["lambda"], out["face"], 0, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        assert (host["face"] > 0).sum() >= 10
        for key, v in out.items():
            assert _same(host[key], v.cpu().numpy()), (name, key)
        # the optional outputs may be left out: popt and status alone
        p2, s2 = e((n, n_vox), torch.float64), e(n_vox, torch.int8)
        gpu.curvefit_constrained_device(o, n_vox, b, t(y), *args, p2, None, s2, None, None, None, None, 0,
                                        torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        assert _same(host["popt"], p2.cpu().numpy()) and _same(host["status"], s2.cpu().numpy())


def _solver(d, **kw):
    from pyneapple_amd.models import TriExpModel
    from pyneapple_amd.solvers import HipConstrainedCurveFitSolver

    names = [str(n) for n in d["names"]]
    return HipConstrainedCurveFitSolver(model=TriExpModel(fit_s0=str(d["model"]) == "tri_s0"), p0=dict(zip(names, map(float, d["p0"]))),
                                        bounds={n: (float(a), float(c)) for n, a, c in zip(names, d["lo"], d["hi"])},
                                        max_iter=int(d["max_iter"]), tol=float(d["tol"]), **kw)


@pytest.mark.parametrize("name", ["g13_tri_constrained_reduced", "g13_tri_constrained_s0"])
def test_plugin_and_two_shards_equal_one_device(gpu, monkeypatch, name):
    monkeypatch.setenv("PNX_SHARE_DEVICE", "1")
    d = load_golden(name)
    names, n_vox = [str(n) for n in d["names"]], len(d["y"])
    one, two = _solver(d), _solver(d, n_gpus=2)
    one.fit(d["b"], d["y"])
    two.fit(d["b"], d["y"])
    direct = _fit(gpu, str(d["model"]), d["b"], d["y"], d["p0"], d["lo"], d["hi"], FIXTURE, max_nfev=int(d["max_iter"]))
    for s in (one, two):
        assert list(s.params_) == names and all(s.params_[n].shape == (n_vox,) for n in names)
        dg = s.diagnostics_
        assert dg["pcov"].shape == (n_vox, len(names), len(names)) and dg["n_pixels"] == n_vox
        assert dg["lambda"].shape == (n_vox,) and dg["lambda"].dtype == np.float64
        assert dg["face"].shape == (n_vox,) and dg["face"].dtype == np.int8
        assert len(s.pixel_results_) == n_vox and s.pixel_results_[0].params.shape == (len(names),)
        assert [r.success for r in s.pixel_results_[:5]] == list(dg["status"][:5] > 0)
        for i, nm in enumerate(names):
            assert _same(s.params_[nm], direct["popt"][i]), nm
        for key in ("pcov", "status", "nfev", "cost", "lambda", "face"):
            assert _same(dg[key], direct[key]), key
    assert (one.diagnostics_["face"] > 0).sum() >= 10


# ---- sentinels ------------------------------------------------------------------------------------------------------------
def test_sentinels_are_the_parents(gpu):
    d = load_golden("g13_tri_constrained_reduced")
    b, p0, lo, hi = d["b"], d["p0"], d["lo"], d["hi"]
    y = d["y"].copy()
    n_vox = len(y)
    # max_nfev = 1: nobody converges, nobody is a violator
    res = _fit(gpu, "tri_reduced", b, y, p0, lo, hi, FIXTURE, max_nfev=1)
    box = gpu.curvefit("tri_reduced", b, y, p0, lo, hi, max_nfev=1, **FIXTURE)
    assert (res["status"] == 0).all() and (res["face"] == 0).all() and np.isnan(res["pcov"]).all()
    assert (res["popt"] == p0[:, None]).all()
    for key in ("popt", "pcov", "status", "nfev", "cost"):
        assert _same(res[key], box[key]), key
    # a bad bound and a NaN signal, among voxels that do go to the face
    P0, LO, HI = (np.ascontiguousarray(np.repeat(a[:, None], n_vox, axis=1)) for a in (p0, lo, hi))
    LO[1, 5] = HI[1, 5]
    y[9, 3] = np.nan
    res = _fit(gpu, "tri_reduced", b, y, P0, LO, HI, FIXTURE)
    box = gpu.curvefit("tri_reduced", b, y, P0, LO, HI, max_nfev=MAX_NFEV, **FIXTURE)
    assert res["status"][5] == -1 and res["status"][9] == -2 and (res["face"][[5, 9]] == 0).all()
    for v in (5, 9):
        assert _same(res["popt"][:, v], P0[:, v]) and np.isnan(res["pcov"][v]).all()
        for key in ("status", "nfev", "cost", "pcov"):
            assert _same(res[key][v], box[key][v]), key
    assert (res["face"] > 0).sum() >= 10

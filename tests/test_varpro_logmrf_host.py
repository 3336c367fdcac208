"""The log coupling of the neighbourhood (MRF) prior over the variable-projection dictionary (pnx_curvefit_varpro_posterior_logfield_f64,
pnx_curvefit_varpro_posterior_logmrf_f64, api.varpro_posterior_logfield / varpro_posterior_logmrf, HipBayesVarProSolver's
spatial_prior "coupling"), the parts that need no GPU: the symbols, the ABI's refusals in front of any device work,
the solver's option parsing and refusals, and the numpy reference -- all-linear coupling is varpro_mrf_reference exactly, its free
energy never decreases, the eps_v preconditions on the inputs of every GPU case, and the worth of the coupling on the phantom."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import varpro_logmrf_cases as cases
import varpro_logmrf_reference as LR
import varpro_mrf_reference as R
from conftest import ROOT

from pyneapple_amd import _lib, api
from pyneapple_amd.models import BiExpModel, TriExpModel
from pyneapple_amd.solvers import HipBayesGridSolver, HipBayesVarProSolver

FIELD, MRF = "pnx_curvefit_varpro_posterior_logfield_f64", "pnx_curvefit_varpro_posterior_logmrf_f64"


def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnx.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    for name, n_args in ((FIELD, 30), (MRF, 33)):
        assert re.search(r"PNX_API\s+int\s+" + name + r"\s*\(", text) and name in _lib.ABI_SYMBOLS and name in exported
        fn = getattr(_lib.load(), name)
        assert len(fn.argtypes) == n_args and fn.restype is C.c_int
    for name in ("varpro_posterior_logfield", "varpro_posterior_logmrf", "varpro_logmrf_centre", "varpro_logmrf_slab_atoms"):
        assert callable(getattr(api, name))


@pytest.mark.parametrize("k", [1, 2, 3])
def test_slab_holds_the_field_rows(k):
    """k + 1 more rows than the linear field's slab, inside 64 KB, never wider than it."""
    for n_b in (k + 1, 16, 32, 33, 128):
        kpad = (n_b + 3) & ~3
        w = api.varpro_logmrf_slab_atoms(n_b, k)
        assert 16 <= w <= api.varpro_mrf_slab_atoms(n_b, k) and w % 16 == 0
        assert k * kpad * (w if w & 16 else w + 16) + (k * (k + 1) + 2 * (k + 1) + 2) * w + 8 <= 8192


def test_centres_and_ranges_by_hand():
    nl = np.array([[0.02, 0.04, 0.10], [0.001, 0.002, 0.004]])
    nonlin = [False, True, True, False]
    c, r = api.varpro_logmrf_centre(nl, nonlin, [0, 1, 0, 0])
    l = np.log(nl[0])
    assert c.tolist() == [0.0, l.min() + 0.5 * (l.max() - l.min()), 0.001 + 0.5 * (0.004 - 0.001), 0.0]
    assert r.tolist() == [0.0, l.max() - l.min(), 0.004 - 0.001, 0.0]
    assert api.varpro_logmrf_centre(nl, nonlin, [0, 0, 0, 0])[0].tolist() == api.varpro_mrf_centre(nl, nonlin).tolist()
    c2, r2 = api.varpro_logmrf_centre(nl, nonlin, [0, 1, 1, 0], np.array([-np.inf, 0.0, 0.0]))  # over the admissible atoms only
    assert r2[1] == np.log(0.10) - np.log(0.04) and r2[2] == np.log(0.004) - np.log(0.002)
    with pytest.raises(ValueError, match="fraction / S0 row"):
        api.varpro_logmrf_centre(nl, nonlin, [1, 0, 0, 0])
    with pytest.raises(ValueError, match="positive values"):
        api.varpro_logmrf_centre(np.array([[0.0, 0.04, 0.10], [0.001, 0.002, 0.004]]), nonlin, [0, 1, 0, 0])


# ---- the ABI without a device
def _mrf_call(precision=(0, 1.0, 1.0, 0), coupling=(0, 1, 1, 0), nl=None, lp=None, n_nb=4):
    o = api.make_opts("bi_s0", 16)  # f1, D1, D2, S0
    nl = np.array([[0.02, 0.04, 0.08], [0.001, 0.002, 0.003]]) if nl is None else np.asarray(nl, float)
    lo, hi = np.array([0.0, -1.0, -1.0, 0.0]), np.array([1.0, 1.0, 1.0, 10.0])
    b, y = np.linspace(0.0, 800.0, 16), np.ones((6, 16))
    table = np.full((6, max(min(n_nb, 8), 1)), -1, np.int32)
    cs, pr = np.array([0, 3, 6], np.int64), np.asarray(precision, float)
    cp = None if coupling is None else np.asarray(coupling, np.int32)
    res = dict(mean=np.full((4, 6), 9.0), fm=np.full((4, 6), 9.0), delta=np.full(2, 9.0), done=C.c_int(-7))
    rc = _lib.load().pnx_curvefit_varpro_posterior_logmrf_f64(C.byref(o), 6, _lib.ptr(b), _lib.ptr(y), 3, _lib.ptr(nl), None, _lib.ptr(lo),
                                                              _lib.ptr(hi), _lib.ptr(lp), 0.0, 1, n_nb, _lib.ptr(table), 2, _lib.ptr(cs),
                                                              _lib.ptr(pr), _lib.ptr(cp), 2, 0.0, _lib.ptr(res["mean"]), None, None, None, None,
                                                              None, None, _lib.ptr(res["fm"]), _lib.ptr(res["delta"]), C.byref(res["done"]), 0, 0,
                                                              None)
    return rc, res


def test_driver_refusals_need_no_device():
    err = _lib.last_error
    assert _mrf_call(n_nb=9)[0] == -1 and "n_nb" in err()  # the linear driver's own, first
    assert _mrf_call(precision=[1.0, 1.0, 0, 0])[0] == -1 and "fraction / S0 row" in err()
    assert _mrf_call(coupling=None)[0] == -1 and "coupling is NULL" in err()
    assert _mrf_call(coupling=[0, 2, 0, 0])[0] == -1 and "coupling[1]=2 must be 0 (linear) or 1 (log)" in err()
    assert _mrf_call(coupling=[1, 1, 0, 0])[0] == -1 and "coupling[0]=1 on a fraction / S0 row must be 0" in err()
    assert _mrf_call(coupling=[0, 1, 1, 1])[0] == -1 and "coupling[3]=1 on a fraction / S0 row must be 0" in err()
    assert _mrf_call(precision=[0, 0.0, 1.0, 0])[0] == -1 and "coupling[1]=1 with precision[1]=0 must be 0" in err()
    zero = [[0.02, 0.04, 0.08], [0.0, 0.002, 0.003]]
    assert _mrf_call(nl=zero)[0] == -1 and "coupling[2]=1 (log) needs positive values: nl_atoms[1, 0]=0" in err()
    assert _mrf_call(nl=[[0.02, 0.04, 0.08], [-0.001, 0.002, 0.003]])[0] == -1 and "needs positive values" in err()
    rc, res = _mrf_call(nl=zero)  # a refused call writes nothing
    assert rc == -1 and (res["mean"] == 9.0).all() and (res["fm"] == 9.0).all() and (res["delta"] == 9.0).all() and res["done"].value == -7
    if _lib.device_count() == 0:  # valid calls stop at the device: a zero rate on a linear row, or on an excluded atom of a log row
        assert _mrf_call()[0] == -3
        assert _mrf_call(nl=zero, coupling=[0, 1, 0, 0])[0] == -3
        assert _mrf_call(nl=zero, lp=np.array([-np.inf, 0.0, 0.0]))[0] == -3


def test_field_refusals_need_no_device():
    err = _lib.last_error
    o = api.make_opts("bi_s0", 16)
    nl = np.array([[0.02, 0.04, 0.08], [0.0, 0.002, 0.003]])
    lo, hi = np.array([0.0, -1.0, -1.0, 0.0]), np.array([1.0, 1.0, 1.0, 10.0])
    b, y, q, n, mean = np.linspace(0.0, 800.0, 16), np.ones((6, 16)), np.zeros((4, 6)), np.zeros(6, np.int32), np.full((4, 6), 9.0)
    fm = np.full((4, 6), 9.0)

    def call(cp=(0, 1, 0, 0), pr=(0, 1.0, 1.0, 0), mem=1, fmean=True, count=6):
        pr, cp = np.asarray(pr, float), np.asarray(cp, np.int32)
        return _lib.load().pnx_curvefit_varpro_posterior_logfield_f64(C.byref(o), 6, _lib.ptr(b), _lib.ptr(y), 3, _lib.ptr(nl), None, _lib.ptr(lo),
                                                                      _lib.ptr(hi), None, 0.0, 1, 0, count, _lib.ptr(q), _lib.ptr(n), _lib.ptr(pr),
                                                                      _lib.ptr(cp), _lib.ptr(mean), None, None, None, None, None, None,
                                                                      _lib.ptr(fm) if fmean else None, None, mem, 0, None)

    assert call(mem=0) == -1 and "PNX_MEM_DEVICE" in err()
    assert call(count=7) == -1 and "range" in err()
    assert call(fmean=False) == -1 and "field_mean is NULL" in err()
    assert call(cp=(0, 1, 1, 0)) == -1 and "needs positive values: nl_atoms[1, 0]=0" in err()
    assert call(cp=(1, 0, 0, 0)) == -1 and "fraction / S0 row" in err()
    assert call(cp=(0, 1, 0, 0), pr=(0, 0, 1.0, 0)) == -1 and "precision[1]=0" in err()
    assert (mean == 9.0).all() and (fm == 9.0).all()


def test_the_one_layout_without_a_kernel_form_is_refused_by_both_calls():
    """Three compartments with S0 and a free T1 above 32 b-values: PNX_ERR_UNSUPPORTED on the host, by name, nothing written; at 32
    b-values, and without T1 above them, the calls go on to the device."""
    err = _lib.last_error
    nl = np.array([[0.1, 0.2], [0.01, 0.02], [0.001, 0.002], [600.0, 1000.0]])
    lo, hi = np.array([0, 1e-5, 0, 1e-5, 1e-5, 0, 100.0]), np.array([1, 0.5, 1, 0.5, 0.5, 10, 5000.0])
    pr, cp = np.array([0, 1.0, 0, 1.0, 1.0, 0, 1.0]), np.array([0, 1, 0, 1, 1, 0, 0], np.int32)
    table, cs = np.full((6, 4), -1, np.int32), np.array([0, 3, 6], np.int64)

    def calls(n_b, t1=True):
        o = api.make_opts("tri_s0", n_b, t1_mode=1, tr=3000.0) if t1 else api.make_opts("tri_s0", n_b)
        k = 7 if t1 else 6
        b, y, q, n = np.linspace(0.0, 800.0, n_b), np.ones((6, n_b)), np.zeros((k, 6)), np.zeros(6, np.int32)
        mean, fm, delta, done = np.full((k, 6), 9.0), np.full((k, 6), 9.0), np.full(2, 9.0), C.c_int(-7)
        atoms, lo_k, hi_k = np.ascontiguousarray(nl[:k - 3]), lo[:k].copy(), hi[:k].copy()  # named: they must outlive the calls
        a = (C.byref(o), 6, _lib.ptr(b), _lib.ptr(y), 2, _lib.ptr(atoms), None, _lib.ptr(lo_k), _lib.ptr(hi_k), None, 0.0, 1)
        p, c = pr[:k].copy(), cp[:k].copy()
        out = (_lib.ptr(mean), None, None, None, None, None, None, _lib.ptr(fm))
        rc_d = _lib.load().pnx_curvefit_varpro_posterior_logmrf_f64(*a, 4, _lib.ptr(table), 2, _lib.ptr(cs), _lib.ptr(p), _lib.ptr(c), 2, 0.0, *out,
                                                                    _lib.ptr(delta), C.byref(done), 0, 0, None)
        msg_d = err()
        rc_f = _lib.load().pnx_curvefit_varpro_posterior_logfield_f64(*a, 0, 6, _lib.ptr(q), _lib.ptr(n), _lib.ptr(p), _lib.ptr(c), *out, None, 1, 0,
                                                                      None)
        return rc_d, msg_d, rc_f, err(), (mean == 9.0).all() and (fm == 9.0).all() and (delta == 9.0).all() and done.value == -7

    for n_b in (33, 128):
        rc_d, msg_d, rc_f, msg_f, untouched = calls(n_b)
        assert rc_d == rc_f == -2 and untouched, (rc_d, msg_d, rc_f, msg_f)
        for who, msg in (("varpro posterior logmrf", msg_d), ("varpro posterior logfield", msg_f)):
            assert who in msg and f"three compartments with S0 and a free T1 at n_b={n_b} > 32 is not built" in msg
            assert "pnx_curvefit_varpro_posterior_mrf_f64 takes this layout" in msg
    if _lib.device_count() == 0:  # built layouts stop at the device
        assert calls(32)[0] == calls(32)[2] == -3 and calls(33, t1=False)[0] == calls(33, t1=False)[2] == -3


# ---- the solver
RATES = {"D1": list(np.geomspace(0.01, 0.2, 5)), "D2": list(np.geomspace(3e-4, 5e-3, 5))}
BOUNDS = {"f1": (0.0, 1.0), "D1": (1e-5, 0.5), "D2": (1e-5, 0.5), "S0": (0.0, 10.0)}


def _solver(rates=RATES, bounds=BOUNDS, **kw):
    return HipBayesVarProSolver(BiExpModel(fit_s0=True), rates, bounds=bounds, **kw)


def test_solver_coupling_options():
    lin = {"f1": "linear", "D1": "linear", "D2": "linear", "S0": "linear"}
    plain = {"strength": {"f1": 0.0, "D1": 16.0, "D2": 16.0, "S0": 0.0}, "n_sweeps": 4, "tol": 0.0, "connectivity": 6}
    assert _solver().spatial_coupling == lin and _solver(spatial_prior={"strength": 16}).spatial_coupling == lin
    assert _solver(spatial_prior={"strength": 16, "coupling": "linear"}).spatial_coupling == lin
    s = _solver(spatial_prior={"strength": 16, "coupling": "log"})
    assert s.spatial_coupling == {**lin, "D1": "log", "D2": "log"} and s.spatial_prior == plain and s.needs_neighbours
    s2 = _solver(spatial_prior={"strength": 16, "coupling": {"D2": "log"}})
    assert s2.spatial_coupling == {**lin, "D2": "log"}
    # the precision of a log row: strength / (range of log rate)^2; of a linear row as before
    nl = s._nl_atoms
    assert s.spatial_precision().tolist() == [0.0, 16.0 / (np.log(nl[0]).max() - np.log(nl[0]).min()) ** 2,
                                              16.0 / (np.log(nl[1]).max() - np.log(nl[1]).min()) ** 2, 0.0]
    assert s2.spatial_precision()[1] == 16.0 / (nl[0].max() - nl[0].min()) ** 2 and s2.spatial_precision()[2] == s.spatial_precision()[2]
    # refusals, each by its message
    for n in ("f1", "S0"):
        with pytest.raises(ValueError, match=f"coupling of {n} cannot be set: a fraction or S0 is solved in closed form"):
            _solver(spatial_prior={"strength": 16, "coupling": {n: "log"}})
    with pytest.raises(ValueError, match=r"coupling names unknown parameters \['D9'\]"):
        _solver(spatial_prior={"strength": 16, "coupling": {"D9": "log"}})
    with pytest.raises(ValueError, match="coupling of D1 must be 'linear' or 'log', got 'sqrt'"):
        _solver(spatial_prior={"strength": 16, "coupling": "sqrt"})
    with pytest.raises(ValueError, match="coupling of D2 must be 'linear' or 'log', got 1"):
        _solver(spatial_prior={"strength": 16, "coupling": {"D2": 1}})
    with pytest.raises(ValueError, match="coupling must be 'linear', 'log' or"):
        _solver(spatial_prior={"strength": 16, "coupling": 7})
    zero = {"D1": RATES["D1"], "D2": [0.0, 1e-3, 2e-3]}
    wide = {**BOUNDS, "D2": (0.0, 0.5)}
    with pytest.raises(ValueError, match="coupling of D2 is 'log', which needs positive values: its admitted atoms reach 0.0"):
        _solver(rates=zero, bounds=wide, spatial_prior={"strength": 16, "coupling": "log"})
    _solver(rates=zero, bounds=wide, spatial_prior={"strength": 16, "coupling": {"D1": "log"}})  # a zero rate on a linear row is fine
    _solver(rates=zero, bounds=wide, spatial_prior={"strength": 16})
    # the key is this solver's only
    grid = dict(model=TriExpModel(fit_reduced=True), grid={"f1": [0.1, 0.2]}, p0={"D1": 0.05, "f2": 0.2, "D2": 0.005, "D3": 0.001},
                bounds={n: (0.0, 1.0) for n in ("f1", "D1", "f2", "D2", "D3")})
    with pytest.raises(ValueError, match=r"spatial_prior has unknown keys \['coupling'\]"):
        HipBayesGridSolver(spatial_prior={"strength": 1, "coupling": "log"}, **grid)


def test_solver_refuses_the_layout_without_a_kernel_form_before_any_work(monkeypatch):
    """tri-exponential with S0 and a free T1 above 32 b-values under coupling "log": a ValueError from fit, before the prior is learned."""
    for name in ("varpro_prior_em", "varpro_posterior_logmrf", "varpro_posterior_mrf"):
        monkeypatch.setattr(api, name, lambda *a, **k: pytest.fail("reached the device"))
    names = ["f1", "D1", "f2", "D2", "D3", "S0", "T1"]
    model = TriExpModel(fit_s0=True, fit_t1=True, repetition_time=3000.0)
    assert list(model.param_names) == names
    rates = {"D1": [0.05, 0.1], "D2": [0.005, 0.01], "D3": [0.0005, 0.001], "T1": [600.0, 1000.0]}
    bounds = {"f1": (0.0, 1.0), "f2": (0.0, 1.0), "S0": (0.0, 10.0), "D1": (1e-5, 0.5), "D2": (1e-5, 0.5), "D3": (1e-5, 0.5), "T1": (100.0, 5000.0)}
    s = HipBayesVarProSolver(model, rates, bounds=bounds, empirical_prior=True, spatial_prior={"strength": 4.0, "connectivity": 4, "coupling": "log"})
    nb, col = api.grid_neighbours(np.ones((2, 3), bool), 4)
    with pytest.raises(ValueError, match="coupling 'log' is not built for three compartments with S0 and a free T1 above 32 b-values"):
        s.fit(np.linspace(0.0, 800.0, 33), np.ones((6, 33)), neighbours=nb, colours=col)


def test_linear_coupling_stays_on_the_linear_entry_point(monkeypatch):
    seen = []
    monkeypatch.setattr(api, "varpro_posterior_mrf", lambda *a, **k: seen.append("mrf") or (_ for _ in ()).throw(RuntimeError("stop")))
    monkeypatch.setattr(api, "varpro_posterior_logmrf", lambda *a, **k: seen.append("logmrf") or (_ for _ in ()).throw(RuntimeError("stop")))
    nb, col = api.grid_neighbours(np.ones((2, 3), bool), 4)
    b, y = np.linspace(0.0, 800.0, 8), np.ones((6, 8))
    for sp in ({"strength": 4.0, "connectivity": 4}, {"strength": 4.0, "connectivity": 4, "coupling": "linear"},
               {"strength": 4.0, "connectivity": 4, "coupling": {"D1": "log"}}):
        with pytest.raises(RuntimeError, match="stop"):
            _solver(spatial_prior=sp).fit(b, y, neighbours=nb, colours=col)
    assert seen == ["mrf", "mrf", "logmrf"]


# ---- the reference
@pytest.fixture(scope="module")
def small():
    from varpro_mrf_cases import small_phantom

    return small_phantom()


def test_all_linear_coupling_is_the_linear_reference_exactly(small):
    c = small
    base, nl, lp = R.base_posterior(c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], noise_sd=c["noise_sd"])
    lam = R.precision_of(base, nl, lp, 16.0)
    assert LR.precision_of(base, nl, lp, 16.0, LR.coupling_of(base, "linear")).tobytes() == lam.tobytes()
    want, wd, wF = R.mrf(c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], c["nb"], c["start"], lam, 3, trace_free_energy=True,
                         noise_sd=c["noise_sd"])
    got, gd, gF = LR.mrf(c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], c["nb"], c["start"], lam, "linear", 3,
                         trace_free_energy=True, noise_sd=c["noise_sd"])
    for k in ("mean", "var", "log_evidence", "ess", "clipped_mass", "map_atom", "W", "l", "eps", "bound_mean", "bound_var"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert gd == wd and gF == wF and np.array_equal(got["field_mean"], got["mean"]) and np.array_equal(got["bound_field_mean"], got["bound_mean"])


def _monotone(Fs):
    Fs = np.array(Fs)
    return (np.diff(Fs) >= -1e-9 * np.abs(Fs[:-1])).all() and Fs[-1] > Fs[0]


def test_free_energy_never_decreases_on_a_mixed_coupling(small):
    c = small
    base, nl, lp = R.base_posterior(c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], noise_sd=c["noise_sd"])
    cp = np.array([0, 1, 0, 0])  # D1 log, D2 linear
    lam = LR.precision_of(base, nl, lp, 64.0, cp)
    state, delta, Fs = LR.mrf(c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], c["nb"], c["start"], lam, cp, 6,
                              trace_free_energy=True, noise_sd=c["noise_sd"])
    assert len(Fs) == 1 + 6 * 2 and _monotone(Fs), Fs
    assert delta[0] > 0 and delta[-1] < delta[0]
    assert np.array_equal(state["field_mean"][:, 2], state["mean"][:, 2]) and not np.array_equal(state["field_mean"][:, 1], state["mean"][:, 1])


@pytest.fixture(scope="module")
def phantom_runs():
    """phantom(seed=0, noise=0.05): the plain posterior and coupling="log" at strength 64, 6 sweeps; max_eps = 1e-3 as
    profiles/varpro_mrf_probe.py, for its reason: at 5 % noise on 16 b-values the posterior is broad and eps_v exceeds 1e-6."""
    ph = LR.phantom(seed=0, noise=0.05)
    order, snb, start = LR.colour_sort(ph["nb"], ph["colours"])
    y, truth = ph["y"][order], ph["truth"][order]
    args = ("bi_s0", ph["b"], y, ph["nl_atoms"], ph["lo"], ph["hi"])
    base, nl, lp = R.base_posterior(*args, noise_sd=0.05, max_eps=1e-3)
    lam = LR.precision_of(base, nl, lp, 64.0, LR.coupling_of(base, "log"))
    state, delta, Fs = LR.mrf(*args, snb, start, lam, "log", 6, trace_free_energy=True, noise_sd=0.05, max_eps=1e-3)
    return dict(plain=base["mean"], state=state, Fs=Fs, truth=truth)


def worth_ratios(mean, plain, truth):
    """median |error| of the linear posterior mean over the plain posterior's, per parameter."""
    return np.median(np.abs(mean - truth), axis=0) / np.median(np.abs(plain - truth), axis=0)


def test_free_energy_never_decreases_on_the_phantom(phantom_runs):
    assert len(phantom_runs["Fs"]) == 13 and _monotone(phantom_runs["Fs"])


def test_worth_on_the_phantom(phantom_runs):
    """The ratios to plain of the median |error| of f1 / D1 / D2 are each <= 0.8 (0.8: "a real gain"; D1 is the tight one)."""
    r = worth_ratios(phantom_runs["state"]["mean"], phantom_runs["plain"], phantom_runs["truth"])
    print("log coupling, strength 64, 5 % noise: ratio to plain of the median |error| (f1, D1, D2, S0):", r)
    assert (r[:3] <= 0.8).all(), r


@pytest.mark.parametrize("name", sorted(cases.GPU_CASES))
def test_gpu_cases_meet_the_references_preconditions(name):
    """The reference alone on the inputs of every GPU case: eps_v <= 1e-6 with the log field's rounding inside."""
    c = cases.GPU_CASES[name]()
    base, nl, lp = R.base_posterior(c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], **c["kw"])  # max_eps = 1e-6
    cp0 = LR.coupling_of(base, c["coupling"])
    pr = LR.precision_of(base, nl, lp, c["strength"], cp0)
    cp = LR.effective(cp0, pr)
    zero = LR.field_posterior(base, nl, lp, np.zeros((len(c["lo"]), c["y"].shape[0])), np.zeros(c["y"].shape[0], np.int32), pr, cp)
    q, n = LR.gather(cases.table(c["y"].shape[0], 8), np.where(base["finite"][None, :], zero["field_mean"].T, np.nan),
                     LR.centres(base, nl, lp, cp), pr)
    ref = LR.field_posterior(base, nl, lp, q, n, pr, cp)
    fin = base["finite"]
    assert (ref["eps"][fin] <= 1e-6).all() and (ref["eps"][fin] >= base["eps"][fin]).all()
    assert (n == 0).any() and (n == 8).any() and not q[base["lin_rows"]].any()
    assert (np.abs(q[base["nl_rows"]]).max() > 0) == (nl.shape[1] > 1)

"""The neighbourhood (MRF) prior of the posterior over the variable projection's dictionary (pnx_curvefit_varpro_posterior_field_f64,
pnx_curvefit_varpro_posterior_mrf_f64, api.varpro_posterior_field / varpro_posterior_mrf, HipBayesVarProSolver's spatial_prior),
the parts that need no GPU: the host-side checks, r_g, ranges and slab sizing under AddressSanitizer / UBSan (a stand-alone
program, tests/host_stub/varpro_mrf_args_stub.cpp), the ABI's refusals in front of any device work, the solver's option parsing
and refusals, the fitter's hand-over, and the numpy reference: its free energy never decreases, strength 0 is the plain
posterior, its host-computed quantities by hand, and the eps_v preconditions on the inputs of every GPU case."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT
import varpro_mrf_cases as cases
import varpro_mrf_reference as R
from varpro_posterior_reference import reference as posterior_reference

from pyneapple_amd import _lib, api
from pyneapple_amd.fitters import HipPixelWiseFitter
from pyneapple_amd.models import BiExpModel, TriExpModel
from pyneapple_amd.solvers import HipBayesGridSolver, HipBayesVarProSolver

FIELD, MRF = "pnx_curvefit_varpro_posterior_field_f64", "pnx_curvefit_varpro_posterior_mrf_f64"


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("stub") / "varpro_mrf_args_stub")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "pyneapple_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "host_stub", "varpro_mrf_args_stub.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode and any(s in b.stderr for s in ("cannot find -lasan", "cannot find -lubsan")):
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-4000:]
    return exe


def _run_stub(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-6000:]
    assert r.returncode == 0, out[-4000:]
    return r.stdout


def test_argument_checks_are_clean_under_sanitizers(stub):
    """Every refusal of the two calls by its message (a positive precision on a fraction / S0 row among them), r_g over the
    non-linear rows, the ranges and centres, the delta scales, and the slab inside 64 KB for every n_b 1..128 x K 1..3."""
    assert "varpro mrf args stub ok" in _run_stub(stub)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_slab_sizing(stub, k):
    """<= 8192 doubles for K 1-3 x n_b {K + 1, 16, 32, 33, 128}, never wider than the posterior's; Python agrees with the header."""
    for n_b in (k + 1, 16, 32, 33, 128):
        kpad = (n_b + 3) & ~3
        w = api.varpro_mrf_slab_atoms(n_b, k)
        got, post = map(int, _run_stub(stub, n_b, k).split())
        assert got == w and post == api.varpro_posterior_slab_atoms(n_b, k) and w <= post
        assert w >= 16 and w % 16 == 0 and k * kpad * (w if w & 16 else w + 16) + (k * (k + 1) + k + 3) * w + 8 <= 8192


# ---- the ABI without a device
def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnx.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    for name, n_args in ((FIELD, 28), (MRF, 31)):
        assert re.search(r"PNX_API\s+int\s+" + name + r"\s*\(", text) and name in _lib.ABI_SYMBOLS and name in exported
        fn = getattr(_lib.load(), name)
        assert len(fn.argtypes) == n_args and fn.restype is C.c_int
    for name in ("varpro_posterior_field", "varpro_posterior_mrf", "varpro_mrf_centre", "varpro_mrf_slab_atoms"):
        assert callable(getattr(api, name))


def _mrf_call(n_vox=6, n_nb=4, n_colours=2, start=(0, 3, 6), precision=None, n_sweeps=2, tol=0.0, out=True, noise_sd=0.0, nb=True, mem=0,
              marginal=1):
    o = api.make_opts("bi_s0", 16)  # f1, D1, D2, S0
    nl = np.array([[0.02, 0.04, 0.08], [0.001, 0.002, 0.003]])
    lo, hi = np.array([0.0, 1e-4, 1e-4, 0.0]), np.array([1.0, 1.0, 1.0, 10.0])
    b, y = np.linspace(0.0, 800.0, 16), np.ones((max(n_vox, 1), 16))
    table = np.full((max(n_vox, 1), max(min(n_nb, 8), 1)), -1, np.int32)
    cs = None if start is None else np.asarray(start, np.int64)
    pr = np.zeros(4) if precision is None else np.asarray(precision, float)
    res = dict(mean=np.full((4, max(n_vox, 1)), 9.0), delta=np.full(max(min(n_sweeps, 100), 1), 9.0), done=C.c_int(-7))
    rc = _lib.load().pnx_curvefit_varpro_posterior_mrf_f64(C.byref(o), n_vox, _lib.ptr(b), _lib.ptr(y), 3, _lib.ptr(nl), None, _lib.ptr(lo),
                                                           _lib.ptr(hi), None, noise_sd, marginal, n_nb, _lib.ptr(table) if nb else None,
                                                           n_colours, _lib.ptr(cs), _lib.ptr(pr) if precision is not False else None, n_sweeps,
                                                           tol, _lib.ptr(res["mean"]) if out else None, None, None, None, None, None, None,
                                                           _lib.ptr(res["delta"]), C.byref(res["done"]), mem, 0, None)
    return rc, res


def test_driver_refusals_need_no_device():
    err = _lib.last_error
    assert _mrf_call(noise_sd=-1.0)[0] == -1 and "noise_sd" in err()  # the posterior's own, first
    assert _mrf_call(marginal=2)[0] == -1 and "marginal_amplitudes" in err()
    assert _mrf_call(out=False)[0] == -1 and "mean" in err()
    for bad in (0, 9):
        assert _mrf_call(n_nb=bad)[0] == -1 and "n_nb" in err() and "[1,8]" in err()
        assert _mrf_call(n_colours=bad)[0] == -1 and "n_colours" in err() and "[1,8]" in err()
    for bad in (-1, 101):
        assert _mrf_call(n_sweeps=bad)[0] == -1 and "n_sweeps" in err() and "[0,100]" in err()
    for bad in (-1.0, np.nan, np.inf):
        assert _mrf_call(tol=bad)[0] == -1 and "tol" in err()
    assert _mrf_call(nb=False)[0] == -1 and "neighbours is NULL" in err()
    assert _mrf_call(start=None)[0] == -1 and "colour_start is NULL" in err()
    for bad in ((1, 3, 6), (0, 3, 5), (0, 3, 7)):
        assert _mrf_call(start=bad)[0] == -1 and "from 0 to n_vox" in err()
    assert _mrf_call(n_colours=3, start=(0, 4, 3, 6))[0] == -1 and "not ascending at colour 1" in err()
    assert _mrf_call(precision=False)[0] == -1 and "precision is NULL" in err()
    for bad in (-1.0, np.nan, np.inf):
        assert _mrf_call(precision=[0, bad, 0, 0])[0] == -1 and "precision[1]" in err()
    assert _mrf_call(precision=[1.0, 0, 0, 0])[0] == -1 and "precision[0]" in err() and "fraction / S0 row" in err()
    assert _mrf_call(precision=[0, 1.0, 1.0, 0.5])[0] == -1 and "precision[3]" in err() and "fraction / S0 row" in err()
    rc, res = _mrf_call(n_nb=9)  # a refused call writes nothing
    assert rc == -1 and (res["mean"] == 9.0).all() and (res["delta"] == 9.0).all() and res["done"].value == -7
    rc, res = _mrf_call(n_vox=0, start=(0, 0, 0))  # no voxels: nothing to do, every delta NaN
    assert rc == 0 and res["done"].value == 0 and np.isnan(res["delta"][:2]).all()
    if _lib.device_count() == 0:  # valid calls stop at the device
        assert _mrf_call(precision=[0, 1.0, 2.0, 0])[0] == -3
        assert _mrf_call(n_colours=3, start=(0, 3, 3, 6), n_sweeps=0)[0] == -3


def test_field_refusals_need_no_device():
    err = _lib.last_error
    o = api.make_opts("bi_s0", 16)
    nl = np.array([[0.02, 0.04, 0.08], [0.001, 0.002, 0.003]])
    lo, hi = np.array([0.0, 1e-4, 1e-4, 0.0]), np.array([1.0, 1.0, 1.0, 10.0])
    b, y, q, n, mean = np.linspace(0.0, 800.0, 16), np.ones((6, 16)), np.zeros((4, 6)), np.zeros(6, np.int32), np.full((4, 6), 9.0)

    def call(first=0, count=6, pr=(0, 1.0, 1.0, 0), mem=1, fq=True):
        pr = np.asarray(pr, float)
        return _lib.load().pnx_curvefit_varpro_posterior_field_f64(C.byref(o), 6, _lib.ptr(b), _lib.ptr(y), 3, _lib.ptr(nl), None, _lib.ptr(lo),
                                                                   _lib.ptr(hi), None, 0.0, 1, first, count, _lib.ptr(q) if fq else None,
                                                                   _lib.ptr(n), _lib.ptr(pr), _lib.ptr(mean), None, None, None, None, None, None,
                                                                   None, mem, 0, None)

    assert call(mem=0) == -1 and "PNX_MEM_DEVICE" in err()
    for first, count in ((-1, 2), (0, 7), (5, 2), (7, 0), (0, -1)):
        assert call(first, count) == -1 and "range" in err()
    assert call(fq=False) == -1 and "field_q" in err()
    assert call(pr=(0, -1.0, 0, 0)) == -1 and "precision[1]" in err()
    assert call(pr=(0.5, 1.0, 0, 0)) == -1 and "fraction / S0 row" in err()
    assert (mean == 9.0).all()


# ---- the solver
RATES = {"D1": list(np.geomspace(0.01, 0.2, 5)), "D2": list(np.geomspace(3e-4, 5e-3, 5))}
BOUNDS = {"f1": (0.0, 1.0), "D1": (1e-5, 0.5), "D2": (1e-5, 0.5), "S0": (0.0, 10.0)}


def _solver(**kw):
    return HipBayesVarProSolver(BiExpModel(fit_s0=True), RATES, bounds=BOUNDS, **kw)


def test_a_misspelt_option_is_refused_not_swallowed():
    """Before spatial_prior existed on this solver the keyword fell into the ignored reference keywords: no error, no field."""
    with pytest.raises(ValueError, match=r"spatial_prior has unknown keys \['strenght'\]"):
        _solver(spatial_prior={"strenght": 1})
    assert "spatial_prior" not in _solver(spatial_prior={"strength": 1.0}).solver_kwargs


def test_solver_spatial_prior_options():
    names = ["f1", "D1", "D2", "S0"]
    assert _solver().spatial_prior is None and not _solver().needs_neighbours and _solver(spatial_prior=False).spatial_prior is None
    s = _solver(spatial_prior={"strength": 16})
    assert s.needs_neighbours and s.spatial_prior == {"strength": {"f1": 0.0, "D1": 16.0, "D2": 16.0, "S0": 0.0}, "n_sweeps": 4, "tol": 0.0,
                                                      "connectivity": 6}
    s = _solver(spatial_prior={"strength": {"D2": 4.0, "f1": 0}, "n_sweeps": 7, "tol": 1e-3, "connectivity": 4})
    assert s.spatial_prior == {"strength": {"f1": 0.0, "D1": 0.0, "D2": 4.0, "S0": 0.0}, "n_sweeps": 7, "tol": 1e-3, "connectivity": 4}
    # the precision: strength / range^2 of the row over the atoms (ordered: D1 > D2), 0 on a fraction and S0
    pr = _solver(spatial_prior={"strength": 16}).spatial_precision()
    nl = s._nl_atoms
    assert pr.tolist() == [0.0, 16.0 / (nl[0].max() - nl[0].min()) ** 2, 16.0 / (nl[1].max() - nl[1].min()) ** 2, 0.0]
    lp = np.where(nl[0] > 0.05, 0.0, -np.inf)  # under a prior that excludes atoms the range shrinks
    assert _solver(spatial_prior={"strength": 16}).spatial_precision(lp)[1] == 16.0 / (nl[0][nl[0] > 0.05].max() - nl[0][nl[0] > 0.05].min()) ** 2
    one = HipBayesVarProSolver(BiExpModel(fit_s0=True), {"D1": [0.05], "D2": RATES["D2"]}, bounds=BOUNDS, spatial_prior={"strength": 3})
    assert one.spatial_precision()[1] == 0.0 and one.spatial_precision()[2] > 0  # a one-value row
    # a fraction or S0 by name
    for n in ("f1", "S0"):
        with pytest.raises(ValueError, match=f"strength of {n} must be 0: a fraction or S0 is solved in closed form"):
            _solver(spatial_prior={"strength": {n: 1.0}})
    # the grid solver's rules and messages
    grid = dict(model=TriExpModel(fit_reduced=True), grid={"f1": [0.1, 0.2]}, p0={"D1": 0.05, "f2": 0.2, "D2": 0.005, "D3": 0.001},
                bounds={n: (0.0, 1.0) for n in ("f1", "D1", "f2", "D2", "D3")})
    for bad in ({"strength": -1}, {"n_sweeps": 3}, {"strength": 1, "n_sweeps": 101}, {"strength": 1, "tol": -1}, {"strength": 1, "connectivity": 5},
                {"strength": {"D9": 1}}, {"strength": "a"}, 7):
        with pytest.raises(ValueError) as mine:
            _solver(spatial_prior=bad)
        if isinstance(bad, dict) and "D9" in str(bad):
            continue
        with pytest.raises(ValueError) as theirs:
            HipBayesGridSolver(spatial_prior=bad, **grid)
        strip = lambda e: re.sub(r"\[.*?\]|of \w+ ", "", str(e.value))
        assert strip(mine) == strip(theirs), (bad, str(mine.value), str(theirs.value))
    # refused by name
    with pytest.raises(ValueError, match="spatial_prior is not built with per-label priors"):
        _solver(spatial_prior={"strength": 1}, empirical_prior={"per_label": True})
    with pytest.raises(ValueError, match="spatial_prior is not built with per-label priors"):
        _solver(spatial_prior={"strength": 1}, log_prior=np.zeros((2, 25)))
    with pytest.raises(ValueError, match="spatial_prior is not built with marginals"):
        _solver(spatial_prior={"strength": 1}, marginals=True)
    assert _solver(spatial_prior={"strength": 1}, empirical_prior=True).needs_neighbours  # a single learned table is allowed
    assert names == list(BiExpModel(fit_s0=True).param_names)


def test_colour_sort_is_shared_and_round_trips():
    assert HipBayesVarProSolver.colour_sort is HipBayesGridSolver.colour_sort
    rng = np.random.default_rng(0)
    nb, col = api.grid_neighbours(np.ones((4, 5), bool), 4)
    y = rng.normal(size=(20, 3))
    seen = {}

    def run(ys, snb, start):
        seen.update(y=ys, nb=snb, start=start)
        return dict(mean=ys.T.copy(), map_atom=np.arange(20, dtype=np.int32), delta=np.zeros(2), n_sweeps=2, extra=1)

    out = HipBayesVarProSolver.in_colour_order(y, nb, col, np.ones(3), ("mean", "map_atom"), run)
    order, snb, start = R.colour_sort(nb, col)
    assert seen["y"].tobytes() == y[order].tobytes() and seen["nb"].tobytes() == snb.tobytes() and seen["start"].tolist() == start.tolist()
    assert out["mean"].tobytes() == np.ascontiguousarray(y.T).tobytes() and out["map_atom"][order].tolist() == list(range(20))
    assert set(out) == {"mean", "map_atom", "delta", "n_sweeps", "precision"}


def test_fit_asks_for_neighbours_and_the_fitter_hands_them_over(monkeypatch):
    s = _solver(spatial_prior={"strength": 4.0, "connectivity": 4})
    b = np.linspace(0.0, 800.0, 8)
    with pytest.raises(ValueError, match="neighbours .* and colours .* are required with spatial_prior"):
        monkeypatch.setattr(api, "varpro_posterior_mrf", lambda *a, **k: pytest.fail("reached the device"))
        s.fit(b, np.ones((6, 8)))
    seen = {}

    def fake_fit(xdata, ydata, pixel_fixed_params=None, **kw):
        seen.update(kw, n=ydata.shape[0])
        raise RuntimeError("stop here")

    monkeypatch.setattr(s, "fit", fake_fit)
    mask = np.ones((3, 4, 1), int)
    mask[0, 0, 0] = 0
    with pytest.raises(RuntimeError, match="stop here"):
        HipPixelWiseFitter(s).fit(b, np.ones((3, 4, 1, 8)), segmentation=mask)
    nb, col = api.grid_neighbours(mask != 0, 4)
    assert seen["n"] == 11 and seen["neighbours"].tobytes() == nb.tobytes() and seen["colours"].tobytes() == col.tobytes()


# ---- the reference
@pytest.fixture(scope="module")
def small_phantom():
    """6 x 5 voxels of the two-region phantom's kind over the 21 apart pairs of the 8-rate list, 4-neighbourhood, sorted by colour."""
    c = cases.small_phantom()
    return c


@pytest.mark.parametrize("strength", [4.0, 64.0])
def test_reference_free_energy_never_decreases(small_phantom, strength):
    c = small_phantom
    base, nl, lp = R.base_posterior(c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], noise_sd=c["noise_sd"])
    lam = R.precision_of(base, nl, lp, strength)
    assert (lam[base["lin_rows"]] == 0).all() and (lam[base["nl_rows"]] > 0).all()
    state, delta, Fs = R.mrf(c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], c["nb"], c["start"], lam, 4, trace_free_energy=True,
                             noise_sd=c["noise_sd"])
    Fs = np.array(Fs)
    assert len(Fs) == 1 + 4 * 2 and (np.diff(Fs) >= -1e-9 * np.abs(Fs[:-1])).all(), Fs
    assert Fs[-1] > Fs[0] and delta[0] > 0 and delta[-1] < delta[0]


def test_reference_at_strength_zero_is_the_plain_posterior(small_phantom):
    c = small_phantom
    ref = posterior_reference(c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], noise_sd=c["noise_sd"])
    state, delta, _ = R.mrf(c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], c["nb"], c["start"], np.zeros(4), 2, noise_sd=c["noise_sd"])
    for k in ("mean", "var", "log_evidence", "ess", "clipped_mass"):
        assert np.allclose(state[k], ref[k], rtol=1e-12, atol=1e-300), k
    assert (state["map_atom"] == ref["map_atom"]).all() and delta == [0.0, 0.0]


def test_reference_host_quantities_by_hand():
    """r_g, the precision, the ranges and the centres on a dictionary small enough to write down (bi_s0: f1, D1, D2, S0)."""
    nl = np.array([[0.02, 0.04, 0.10], [0.001, 0.002, 0.003]])
    base = dict(lin_rows=[0, 3], nl_rows=[1, 2])
    lp = np.zeros(3)
    assert R.ranges(base, nl, lp).tolist() == [0.0, 0.10 - 0.02, 0.003 - 0.001, 0.0]
    c = R.centres(base, nl, lp)
    assert c.tolist() == [0.0, 0.02 + 0.5 * (0.10 - 0.02), 0.001 + 0.5 * (0.003 - 0.001), 0.0]
    pr = R.precision_of(base, nl, lp, 16.0)
    assert pr.tolist() == [0.0, 16.0 / (0.10 - 0.02) ** 2, 16.0 / (0.003 - 0.001) ** 2, 0.0]
    r = R.r_row(base, nl, c, pr)
    for g in range(3):
        t1, t2 = nl[0, g] - c[1], nl[1, g] - c[2]
        assert r[g] == 0.0 + pr[1] * (t1 * t1) + pr[2] * (t2 * t2)
    lp2 = np.array([-np.inf, 0.0, 0.0])  # over the admissible atoms only
    assert R.ranges(base, nl, lp2)[1] == 0.10 - 0.04 and R.centres(base, nl, lp2)[1] == 0.04 + 0.5 * (0.10 - 0.04)
    one = np.array([[0.05, 0.05, 0.05], [0.001, 0.002, 0.003]])
    assert R.precision_of(base, one, lp, 16.0)[1] == 0.0  # a one-value row
    assert api.varpro_mrf_centre(nl, [False, True, True, False]).tolist() == c.tolist()


@pytest.mark.parametrize("name", sorted(cases.GPU_CASES))
def test_gpu_cases_meet_the_references_preconditions(name):
    """The reference alone on the inputs of every GPU case: varpro_posterior_reference asserts eps_v <= 1e-6 in the wide box and
    that no compared voxel sits on the cancellation floor; with the field's rounding the enlarged eps_v stays under 1e-6 too."""
    c = cases.GPU_CASES[name]()
    base, nl, lp = R.base_posterior(c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], **c["kw"])  # max_eps = 1e-6
    assert not base["clipped_mass"].any()
    pr = R.precision_of(base, nl, lp, c["strength"])
    nb = cases.table(c["y"].shape[0], 8)
    q, n = R.gather(nb, np.where(base["finite"][None, :], base["mean"].T, np.nan), R.centres(base, nl, lp), pr)
    ref = R.field_posterior(base, nl, lp, q, n, pr)
    fin = base["finite"]
    assert (ref["eps"][fin] <= 1e-6).all() and (ref["eps"][fin] >= base["eps"][fin]).all()
    assert (n == 0).any() and (n == 8).any() and not q[base["lin_rows"]].any()
    assert (np.abs(q[base["nl_rows"]]).max() > 0) == (nl.shape[1] > 1)  # one atom: every row holds one value, every precision is 0

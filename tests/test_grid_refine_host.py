"""The per-voxel fine grid (pnx_curvefit_grid_refine_f64; api.grid_refine; HipBayesGridSolver(refine=...)), the
parts that need no GPU: the numpy reference against a brute-force per-voxel posterior, the construction of the fine grid (as a host
program, under sanitizers too), the reference's preconditions on every GPU case, the solver's options and refusals, the ABI's
refusals in front of any device work, and the worth of the refinement on the reference alone."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT
import grid_refine_cases as K
import grid_refine_reference as R
from grid_start_reference import signals

from pyneapple_amd import _lib, api
from pyneapple_amd.models import BiExpModel
from pyneapple_amd.solvers import HipBayesGridSolver

SYMBOL = "pnx_curvefit_grid_refine_f64"
STUB_SRC = os.path.join(ROOT, "tests", "host_stub", "grid_refine_stub.cpp")


def _build_stub(exe, *flags):
    cmd = ["g++", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "pyneapple_amd", "csrc"), STUB_SRC, "-o", exe]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def plain_stub(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("refine") / "grid_refine_stub")
    b = _build_stub(exe, "-O2", "-ffp-contract=off")
    assert b.returncode == 0, b.stderr[-4000:]
    return exe


def test_stub_is_clean_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "grid_refine_stub_san")
    b = _build_stub(exe, "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer")
    if b.returncode and any(s in b.stderr for s in ("cannot find -lasan", "cannot find -lubsan")):
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-6000:]
    assert r.returncode == 0 and "grid refine stub ok" in r.stdout, out[-4000:]


# ---- the fine grid's construction: the header's function against the reference's
@pytest.mark.parametrize("lo,hi,c,h,m", [(0.0, 1.0, 0.9, 0.3, 5), (0.0, 1.0, 0.05, 0.3, 4), (0.0, 1.0, 0.5, 0.3, 1), (0.0, 1.0, 1.7, 0.3, 9),
                                         (0.0, 1.0, 0.4, 0.0, 9), (0.005, 0.2, 0.0613, 0.0177, 9), (0.0001, 0.004, 0.0011, 0.0007, 2)])
def test_axis_of_the_header_is_the_references(plain_stub, lo, hi, c, h, m):
    out = subprocess.run([plain_stub, "axis", repr(lo), repr(hi), repr(c), repr(h), str(m)], capture_output=True, text=True, check=True).stdout
    got = np.array([float(t) for t in out.split()])
    x, a, b = R.axis(lo, hi, c, h, m)
    assert got.shape == x.shape and (got >= lo).all() and (got <= hi).all()
    assert got[0] == x[0] and got[-1] == x[-1]  # the ends are exact; between them fma against two roundings
    np.testing.assert_allclose(got, x, rtol=3 * R.U, atol=0)
    if m == 1 or not min(hi, c + h) > max(lo, c - h):
        assert got.size == 1 and got[0] == min(max(c, lo), hi)


def test_construction_clipping_single_values_and_the_limit():
    c, info = K.edge_case()
    ref = K.reference_of(c)
    at = ref["atoms"]
    assert at[info["cut"]][1].max() == c["hi"][1] and at[info["cut"]][1].min() == 0.19 - 0.03  # cut by the upper bound
    assert ref["n_atoms"][info["single"]] == 25 and (at[info["single"]][2] == c["lo"][2]).all()  # b <= a: the clipped centre
    assert ref["n_atoms"][info["zero_width"]] == 25 and (at[info["zero_width"]][0] == c["centre"][0, info["zero_width"]]).all()
    assert ref["n_admitted"][info["straddle"]] == 75 and (at[info["straddle"]][0][ref["adm"][info["straddle"]]] <= 1.0).all()
    assert sorted(np.flatnonzero(~ref["finite"])) == info["nan"] and ref["n_admitted"][13] == 0 and ref["n_atoms"][13] == 125
    # the first row is the slowest
    v = at[0]
    assert (np.diff(v[0]) >= 0).all() and v[2][0] != v[2][1] and v[0][0] == v[0][24]
    one = K.reference_of(K.build("bi_reduced_one_point"))
    assert (one["n_atoms"] == 1).all() and (one["var"] == 0).all() and (one["ess"] == 1).all()


LAYOUTS = [("bi_reduced", (3, 4, 2), False, 0.03), ("tri_s0", (2, 2, 2, 3, 2, 1), True, 0.0)]


@pytest.mark.parametrize("model,pts,project,noise_sd", LAYOUTS)
def test_reference_against_a_brute_force_posterior(model, pts, project, noise_sd):
    """Per voxel: the atoms one by one through the project's own forward models (tests/grid_start_reference.signals), the textbook
    posterior over them."""
    rng = np.random.default_rng(2)
    names = R.LAYOUT[model]
    n_vox, b = 12, np.array([0.0, 20.0, 60.0, 150.0, 400.0, 800.0])
    truth = np.stack([rng.uniform(*K.RANGES[n], n_vox) for n in names])
    y = signals(model, b, truth) + rng.normal(0, 0.03, (n_vox, len(b)))
    lo, hi = np.array([K.BOUNDS[n][0] for n in names]), np.array([K.BOUNDS[n][1] for n in names])
    centre = truth * rng.uniform(0.9, 1.1, truth.shape)
    half = 0.2 * truth
    ref = R.reference(model, b, y, lo, hi, np.array(pts), centre, half, noise_sd=noise_sd, project=project)
    for v in range(n_vox):
        atoms = ref["atoms"][v].copy()
        S = signals(model, b, atoms)
        if project:
            row = len(names) - 1
            amp = np.clip((S @ y[v]) / (S * S).sum(axis=1), lo[row], hi[row])
            S = S * amp[:, None]
            atoms[row] = amp
        c = 0.5 * ((y[v][None] - S) ** 2).sum(axis=1)
        ll = -c / noise_sd ** 2 if noise_sd > 0 else -0.5 * (len(b) - (1 if project else 0)) * np.log(c)
        post = np.exp(ll - ll.max())
        post /= post.sum()
        np.testing.assert_allclose(ref["mean"][v], atoms @ post, rtol=1e-10)
        np.testing.assert_allclose(ref["var"][v], ((atoms - (atoms @ post)[:, None]) ** 2) @ post, rtol=1e-8, atol=1e-30)
        np.testing.assert_allclose(ref["ess"][v], 1 / (post ** 2).sum(), rtol=1e-10)
        np.testing.assert_allclose(ref["log_norm"][v], np.log(np.mean(np.exp(ll - ll.max()))) + ll.max(), rtol=0, atol=1e-10)
        np.testing.assert_allclose(ref["map_p"][v], atoms[:, ll.argmax()], rtol=1e-12)
    assert ref["finite"].all() and (ref["edge_mass"] >= 0).all() and (ref["edge_mass"] <= 1 + 1e-12).all()
    assert (ref["edge_mass"][:, np.array(pts) == 1] == 0).all() and (ref["edge_mass"][:, np.array(pts) == 2] > 1 - 1e-12).all()


@pytest.mark.parametrize("name", list(K.CASES))
def test_reference_preconditions_hold_on_every_gpu_case(name):
    c = K.build(name)
    ref = K.reference_of(c)
    assert ref["finite"].all() and np.nanmax(ref["eps"]) <= 1e-6 and (ref["margin"] > 1e-9).all()
    assert ref["n_atoms"].max() == int(np.prod(c["n_points"])) <= 4096


def test_cases_cover_the_kernel_paths():
    shapes = [K.CASES[n] for n in K.CASES]
    assert {1, 17, 130} == {s[1] for s in shapes} and {1, 4, 5, 32, 33, 128} == {s[2] for s in shapes}
    assert {s[0] for s in shapes} == set(api.MODEL_PARAM_NAMES)
    atoms = {int(np.prod(s[3])) for s in shapes}
    assert 1 in atoms and 64 in atoms and any(a % 64 and a > 64 for a in atoms) and 3125 in atoms
    assert any(9 in s[3] for s in shapes) and any(s[4] == 0.0 for s in shapes) and any(s[4] > 0 for s in shapes)
    assert any(s[5] for s in shapes) and any(s[6] for s in shapes)
    assert any(s[0].endswith("_s0") and not s[5] for s in shapes)  # S0 on the grid


# ---- worth, on the reference alone
def test_worth_of_the_refinement_on_the_reference():
    """The table of DESIGN.md 4.1u / README, printed whole: median |error| refined / coarse per parameter.  Every cell below 1 is
    asserted at measured + 0.1.  At 5 % noise D1 does NOT gain (0.99 at one level, 1.24 at two): the table says so."""
    for noise in K.WORTH_NOISE:
        p = K.worth_population(noise)
        for lv in K.WORTH_LEVELS:
            out = R.refine_levels("bi_reduced", p["b"], p["y"], K.WORTH_LO, K.WORTH_HI, K.WORTH_AXES, noise, points=5, levels=lv)
            med = lambda m: np.median(np.abs(m - p["truth"]), axis=1)
            ratio = med(out[-1]["mean"]) / med(out[0]["mean"])
            print(f"noise {noise} levels {lv}: refined / coarse (f1, D1, D2) {np.round(ratio, 4)}; median refine_ess "
                  f"{np.median(out[-1]['ess']):.2f}; mean edge_mass {np.round(out[-1]['edge_mass'].mean(axis=1), 3)}")
            for k, measured in enumerate(K.WORTH_MEASURED[(noise, lv)]):
                if measured < 1:
                    assert ratio[k] <= measured + 0.1
    assert all(m < 0.7 for m in K.WORTH_MEASURED[(0.01, 1)]) and K.WORTH_MEASURED[(0.05, 2)][1] > 1


# ---- the solver's options
GRID = {n: list(ax) for n, ax in zip(("f1", "D1", "D2"), K.WORTH_AXES)}
BOUNDS = {n: (float(K.WORTH_LO[i]), float(K.WORTH_HI[i])) for i, n in enumerate(("f1", "D1", "D2"))}


def _bi(**kw):
    return HipBayesGridSolver(BiExpModel(), {n: list(v) for n, v in GRID.items()}, bounds=dict(BOUNDS), **kw)


def test_solver_refine_options():
    assert _bi().refine is None and _bi(refine=None).refine is None and _bi(refine=False).refine is None
    s = _bi(refine=True)
    assert s.refine == {"points": {"f1": 5, "D1": 5, "D2": 5}, "levels": 1, "span": 1.0, "n_sd": 2.0} and list(s.refine_points()) == [5, 5, 5]
    s = _bi(refine={"points": {"D1": 9}, "levels": 3, "span": 0.5, "n_sd": 0})
    assert s.refine["points"] == {"f1": 5, "D1": 9, "D2": 5} and s.refine["levels"] == 3 and s.refine["n_sd"] == 0.0
    one = HipBayesGridSolver(BiExpModel(), {"f1": [0.1, 0.2], "D1": [0.02, 0.05]}, p0={"D2": 0.001}, bounds=dict(BOUNDS), refine=True)
    assert list(one.refine_points()) == [5, 5, 1]  # a one-value axis keeps one value
    for bad, what in (({"pts": 5}, "unknown keys"), ({"points": 0}, "points of f1"), ({"points": 10}, "points of f1"), ({"points": 2.5}, "points of f1"),
                      ({"points": {"D9": 3}}, "unknown parameters"), ({"levels": 0}, "levels"), ({"levels": 4}, "levels"), ({"levels": True}, "levels"),
                      ({"span": -1}, "span"), ({"n_sd": np.nan}, "n_sd"), ({"span": 0, "n_sd": 0}, "span > 0 or n_sd > 0"), (5, "must be None"),
                      ("yes", "must be None")):
        with pytest.raises(ValueError, match=re.escape(what)):
            _bi(refine=bad)
    not_built = "refine is not built with "
    for kw, what in ((dict(noise_sd=0.05, noise_model="rician"), "noise_model='rician'"), (dict(spatial_prior={"strength": 4}), "spatial_prior"),
                     (dict(empirical_prior=True), "empirical_prior"), (dict(marginals=True), "marginals"),
                     (dict(log_prior=np.zeros((2, 64))), "per-label priors"), (dict(log_prior=np.arange(64.0)), "a non-uniform log_prior"),
                     (dict(sigma=0.1), "sigma")):
        with pytest.raises(ValueError, match=re.escape(not_built + what)):
            _bi(refine=True, **kw)
    assert _bi(refine=True, log_prior=np.zeros(64)).refine  # a constant table is the uniform prior
    big = {n: (0.0, 1.0) for n in ("f1", "D1", "f2", "D2", "D3")}
    from pyneapple_amd.models import TriExpModel

    tri = lambda pts: HipBayesGridSolver(TriExpModel(fit_reduced=True), {n: [0.1, 0.2] for n in big}, bounds=big, refine={"points": pts})
    assert list(tri(5).refine_points()) == [5] * 5
    with pytest.raises(ValueError, match="span 7776 atoms"):
        tri(6)
    doc = HipBayesGridSolver.__doc__
    assert "refine" in doc and SYMBOL in doc and "refine_edge_mass" in doc


def test_coarse_cell():
    ax = np.array([0.1, 0.2, 0.4, 0.8])
    got = HipBayesGridSolver.coarse_cell(ax, np.array([0.05, 0.1, 0.15, 0.2, 0.3, 0.5, 0.8, 0.9, np.nan]))
    np.testing.assert_allclose(got[:8], [0.1, 0.1, 0.1, 0.2, 0.2, 0.4, 0.4, 0.4])
    assert np.isnan(got[8]) and (HipBayesGridSolver.coarse_cell(np.array([0.3]), np.array([0.3, 0.1])) == 0).all()
    np.testing.assert_allclose(R.coarse_cell(ax, np.array([0.05, 0.15, 0.3, 0.9])), [0.1, 0.1, 0.2, 0.4])


def test_toml_round_trip():
    try:
        import tomllib
    except ImportError:  # Python 3.10
        import tomli as tomllib
    text = ('[Fitting.solver]\nnoise_sd = 0.05\n[Fitting.solver.grid]\nf1 = [0.1, 0.2]\nD1 = [0.02, 0.04]\nD2 = [0.001]\n'
            '[Fitting.solver.refine]\nlevels = 2\nn_sd = 3.0\n[Fitting.solver.refine.points]\nf1 = 7\n')
    table = tomllib.loads(text)["Fitting"]["solver"]
    s = HipBayesGridSolver(BiExpModel(), max_iter=250, tol=1e-8, bounds=dict(BOUNDS), **table)
    assert s.refine == {"points": {"f1": 7, "D1": 5, "D2": 5}, "levels": 2, "span": 1.0, "n_sd": 3.0} and list(s.refine_points()) == [7, 5, 1]


def test_default_path_is_unchanged(monkeypatch):
    """refine=None calls api.grid_posterior with the arguments it had and nothing else; refine calls it the same way, then
    api.grid_refine once per level with the previous level's mean as the centre."""
    calls = []
    n = 2
    fake = dict(mean=np.full((3, n), 0.25) * np.array([[1.0], [0.1], [0.005]]), sd=np.full((3, n), 0.01), map_p=np.zeros((3, n)),
                map_atom=np.zeros(n, np.int32), log_evidence=np.zeros(n), ess=np.ones(n))
    fine = lambda i: dict(mean=fake["mean"] * (1 + 0.01 * i), sd=fake["sd"] / 2, map_p=np.ones((3, n)), edge_mass=np.zeros((3, n)),
                          ess=np.full(n, 3.0), log_norm=np.zeros(n))
    monkeypatch.setattr(api, "grid_posterior", lambda *a, **k: calls.append(("coarse", a, k)) or fake)
    monkeypatch.setattr(api, "grid_refine", lambda *a, **k: calls.append(("fine", a, k)) or fine(len(calls)))
    b, y = np.linspace(0, 1000, 8), np.ones((n, 8))
    g = _bi(noise_sd=0.05).fit(b, y)
    assert [c[0] for c in calls] == ["coarse"]
    assert set(calls[0][2]) == {"log_prior", "noise_sd", "fixed_idx", "fixed_vals", "sigma", "project_amplitude", "device"} | set(g._kernel_t1)
    assert set(g.diagnostics_) == {"posterior_sd", "map", "map_atom", "log_evidence", "ess", "n_pixels"}
    assert np.asarray(g.params_["f1"]).tobytes() == fake["mean"][0].tobytes()
    del calls[:]
    r = _bi(noise_sd=0.05, refine={"levels": 2}).fit(b, y)
    assert [c[0] for c in calls] == ["coarse", "fine", "fine"] and calls[0][2].keys() == set(g._kernel_t1) | {"log_prior", "noise_sd", "fixed_idx",
                                                                                                              "fixed_vals", "sigma", "project_amplitude", "device"}
    first, second = calls[1][1], calls[2][1]
    assert list(first[5]) == [5, 5, 5] and first[6].tobytes() == fake["mean"].tobytes()
    cell = np.array([0.1, 0.02, 0.0005])  # the coarse gaps of the three axes
    np.testing.assert_allclose(first[7], np.maximum(cell[:, None], 2 * fake["sd"]), rtol=1e-12)
    assert second[6].tobytes() == fine(2)["mean"].tobytes()  # the second level is centred on the first level's mean
    spacing = (np.minimum(K.WORTH_HI[:, None], first[6] + first[7]) - np.maximum(K.WORTH_LO[:, None], first[6] - first[7])) / 4
    np.testing.assert_allclose(second[7], np.maximum(spacing, 2 * fake["sd"] / 2), rtol=1e-12)
    assert calls[1][2]["noise_sd"] == 0.05 and calls[1][2]["project_amplitude"] is False
    d = r.diagnostics_
    assert d["refine_levels"] == 2 and (d["refine_ess"] == 3.0).all() and set(d["refine_edge_mass"]) == {"f1", "D1", "D2"}
    assert (d["ess"] == 1.0).all() and (d["map"]["f1"] == 1.0).all() and np.asarray(r.params_["D1"]).tobytes() == fine(3)["mean"][1].tobytes()
    assert (d["posterior_sd"]["D2"] == 0.005).all()


def test_no_cpu_fallback_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is visible here")
    c = K.build("bi_reduced_one_b")
    with pytest.raises(_lib.PnxError):
        api.grid_refine(c["model"], c["b"], c["y"], c["lo"], c["hi"], c["n_points"], c["centre"], c["half_width"], noise_sd=0.02)
    p = K.worth_population(0.05, n_vox=4)
    with pytest.raises(_lib.PnxError):
        _bi(noise_sd=0.05, refine=True).fit(p["b"], p["y"])


# ---- the ABI without a device
def test_symbol_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnx.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    assert re.search(r"PNX_API\s+int\s+" + SYMBOL + r"\s*\(", text) and SYMBOL in _lib.ABI_SYMBOLS and SYMBOL in exported
    fn = getattr(_lib.load(), SYMBOL)
    assert len(fn.argtypes) == 21 and fn.restype is C.c_int
    assert callable(api.grid_refine) and callable(api.grid_refine_device) and api.GRID_REFINE_MAX_POINTS == 9
    header = open(os.path.join(ROOT, "include", "pnx.h")).read()
    assert "fraction-sum rule" in header and "NOT an evidence" in header and "edge_mass" in header


def _abi_call(noise_sd=0.05, sigma=None, points=(2, 2, 2), mean=True, n_vox=3, t1_mode=0, lo0=0.0):
    o = api.make_opts("bi_reduced", 16, sigma=sigma)
    o.t1_mode = t1_mode
    lo, hi, b, y = np.array([lo0, 0.0, 0.0]), np.ones(3), np.zeros(16), np.ones((max(n_vox, 1), 16))
    centre, hw = np.full((3, max(n_vox, 1)), 0.5), np.full((3, max(n_vox, 1)), 0.1)
    npts = np.array(points, np.int32)
    out = np.full((3, max(n_vox, 1)), 9.0)
    rc = _lib.load().pnx_curvefit_grid_refine_f64(C.byref(o), n_vox, _lib.ptr(b), _lib.ptr(y), None, _lib.ptr(lo), _lib.ptr(hi), 0, noise_sd,
                                                  _lib.ptr(npts), _lib.ptr(centre), _lib.ptr(hw), _lib.ptr(out) if mean else None, None, None,
                                                  None, None, None, 0, 0, None)
    return rc, out


def test_refusals_need_no_device():
    err = _lib.last_error
    for bad in (np.nan, np.inf, -np.inf):
        rc, out = _abi_call(noise_sd=bad)
        assert rc == -1 and "noise_sd" in err() and (out == 9.0).all()
    rc, out = _abi_call(sigma=np.ones(16))
    assert rc == -2 and "sigma is not built" in err() and (out == 9.0).all()
    assert _abi_call(points=(2, 10, 2))[0] == -1 and "n_points[1]=10" in err()
    assert _abi_call(points=(2, 0, 2))[0] == -1 and "n_points[1]=0" in err()
    assert _abi_call(mean=False)[0] == -1 and "mean is NULL" in err()
    assert _abi_call(lo0=2.0)[0] == -1 and "free parameter 0" in err()
    assert _abi_call(n_vox=0)[0] == 0
    o = api.make_opts("tri_reduced", 16)
    five = np.zeros(5), np.ones(5), np.array([9, 9, 9, 9, 1], np.int32)
    z = np.zeros((5, 1))
    rc = _lib.load().pnx_curvefit_grid_refine_f64(C.byref(o), 1, _lib.ptr(np.zeros(16)), _lib.ptr(np.ones((1, 16))), None, _lib.ptr(five[0]),
                                                  _lib.ptr(five[1]), 0, 0.05, _lib.ptr(five[2]), _lib.ptr(z), _lib.ptr(z), _lib.ptr(z.copy()), None,
                                                  None, None, None, None, 0, 0, None)
    assert rc == -1 and "6561 atoms" in err() and "more than 4096" in err()
    if _lib.device_count() == 0:  # a valid call stops at the device
        assert _abi_call()[0] == -3


def test_a_voxel_without_a_fine_atom_is_not_a_success(monkeypatch):
    """The coarse builder admits atoms beyond f1 + f2 = 1, so a coarse mean can sit there; the fine box then holds no admitted atom and
    the voxel's NaN parameters are reported with success False, not True."""
    n = 3
    coarse = dict(mean=np.full((3, n), 0.25), sd=np.full((3, n), 0.01), map_p=np.zeros((3, n)), map_atom=np.array([0, -1, 5], np.int32),
                  log_evidence=np.zeros(n), ess=np.ones(n))
    fine_mean = np.full((3, n), 0.3)
    fine_mean[:, 1:] = np.nan  # voxel 1: a non-finite signal; voxel 2: no admitted atom
    fine = dict(mean=fine_mean, sd=fine_mean * 0.1, map_p=fine_mean, edge_mass=fine_mean * 0, ess=fine_mean[0], log_norm=fine_mean[0])
    monkeypatch.setattr(api, "grid_posterior", lambda *a, **k: coarse)
    monkeypatch.setattr(api, "grid_refine", lambda *a, **k: fine)
    s = _bi(noise_sd=0.05, refine=True).fit(np.linspace(0, 1000, 8), np.ones((n, 8)))
    results = list(s.pixel_results_)
    assert [r.success for r in results] == [True, False, False]
    assert "infs or NaNs" in results[1].message and "no atom of the fine grid" in results[2].message
    plain = _bi(noise_sd=0.05).fit(np.linspace(0, 1000, 8), np.ones((n, 8)))
    assert [r.success for r in plain.pixel_results_] == [True, False, True]  # without refine: the coarse mask, as before

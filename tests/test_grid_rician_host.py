"""The grid posterior under a Rician likelihood (pnx_curvefit_grid_posterior_rician_f64, pnx_log_i0e_f64; api.grid_posterior_rician /
log_i0e; HipBayesGridSolver(noise_model="rician")), the parts that need no GPU: log_i0e of csrc/pnx_bessel.hpp as a
host program against SciPy, the numpy reference against a brute-force Rice posterior and against the Gaussian reference at high
SNR, the reference's preconditions on every GPU case, the solver's options and refusals, the ABI's refusals in front of any device
work, and the worth of the likelihood on the reference alone."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT
from scipy.stats import rice
import grid_rician_cases as K
import grid_rician_reference as R
from grid_posterior_reference import reference as gauss_reference
from grid_start_reference import signals

from pyneapple_amd import _lib, api, synth
from pyneapple_amd.models import BiExpModel
from pyneapple_amd.solvers import HipBayesGridSolver

U = 2.0 ** -52
POSTERIOR, LOG_I0E = "pnx_curvefit_grid_posterior_rician_f64", "pnx_log_i0e_f64"
STUB_SRC = os.path.join(ROOT, "tests", "host_stub", "bessel_stub.cpp")


def _build_stub(exe, *flags):
    cmd = ["g++", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "pyneapple_amd", "csrc"), STUB_SRC, "-o", exe]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


# ---- log_i0e as a host program
@pytest.fixture(scope="module")
def plain_stub(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("bessel") / "bessel_stub")
    b = _build_stub(exe, "-O2", "-ffp-contract=off")
    assert b.returncode == 0, b.stderr[-4000:]
    return exe


def _evaluate(exe, z, tmp_path):
    z.tofile(str(tmp_path / "z.bin"))
    subprocess.run([exe, str(tmp_path / "z.bin"), str(tmp_path / "h.bin")], check=True, timeout=60)
    return np.fromfile(str(tmp_path / "h.bin"))


def test_log_i0e_against_scipy(plain_stub, tmp_path):
    """|error| / (2^-52 max(|h|, 1)) <= E_h = 4.5, the derived bound of csrc/pnx_bessel.hpp with its margin of 2 (the z^2 / 4 of the
    issue's measure never exceeds 1 where it applies).  Observed against SciPy: 1.75 on this list, 3.0 on a dense sweep of [0, 16]
    (SciPy's own log(ive) is off by up to 2 units below z = 2); against 40-digit arithmetic 1.0."""
    z = K.z_list()
    h = _evaluate(plain_stub, z, tmp_path)
    ref = R.reference_h(z)
    err = np.abs(h - ref) / (U * np.maximum(np.abs(ref), 1.0))
    print("log_i0e on the host: largest error", err.max(), "at z =", z[err.argmax()])
    assert h[0] == 0.0 and np.isfinite(h).all() and (h <= 0).all() and (np.diff(h[1:20002]) <= 0).all()
    assert err.max() <= R.E_H
    small = z[(z > 0) & (z < 1e-17)]
    assert (_evaluate(plain_stub, small, tmp_path) == -small).all()  # h = -z (1 - z / 4 + ...): -z to the last bit below 2^-54, down to the denormals
    bad = _evaluate(plain_stub, np.array([-1.0, np.nan, -5e-324, np.inf]), tmp_path)
    assert np.isnan(bad[:3]).all() and bad[3] == -np.inf
    text = open(os.path.join(ROOT, "pyneapple_amd", "csrc", "pnx_bessel.hpp")).read()
    assert f"kLogI0eBound = {R.E_H}" in text and "cyl_bessel" not in text


def test_stub_is_clean_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "bessel_stub_san")
    b = _build_stub(exe, "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer")
    if b.returncode and any(s in b.stderr for s in ("cannot find -lasan", "cannot find -lubsan")):
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-6000:]
    assert r.returncode == 0 and "grid rician stub ok" in r.stdout, out[-4000:]
    z = K.z_list()
    z.tofile(str(tmp_path / "z.bin"))
    r = subprocess.run([exe, str(tmp_path / "z.bin"), str(tmp_path / "h.bin")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "runtime error:" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


@pytest.mark.parametrize("n_b,n_free", [(1, 1), (4, 2), (5, 3), (32, 5), (33, 4), (64, 6), (128, 3), (128, 8)])
def test_python_slab_width_is_the_kernels(plain_stub, n_b, n_free):
    out = subprocess.run([plain_stub, "slab", str(n_b), str(n_free)], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == api.grid_rician_slab_atoms(n_b, n_free) and int(out[2]) <= 65536


# ---- the numpy reference
LAYOUTS = [("mono", {}), ("bi_reduced", {}), ("bi_s0", {}), ("bi_full", {}), ("tri_reduced", {}), ("tri_s0", {}), ("tri_full", {}),
           ("bi_reduced", dict(t1_mode=1, tr=3000.0))]


@pytest.mark.parametrize("model,kw", LAYOUTS)
def test_reference_against_a_brute_force_rice_posterior(model, kw):
    """50 voxels, 9 atoms, a non-uniform prior: log sum_g pi_g prod_i Rice(y_i | s_gi, sd) with scipy.stats.rice.logpdf."""
    rng = np.random.default_rng(7)
    names = K.names_of(model, kw)
    b = np.array([0.0, 50.0, 200.0, 800.0, 1500.0, 2500.0])
    atoms = np.stack([rng.uniform(*K.RANGES[n], 9) for n in names])
    truth = atoms[:, rng.integers(0, 9, 50)]
    sd = 0.08
    y = synth.rician_magnitude(signals(model, b, truth, **kw), sd, seed=3)
    lp = np.log(rng.uniform(0.1, 1.0, 9))
    lo, hi = np.zeros(len(names)), np.array([2 * K.RANGES[n][1] for n in names])
    ref = R.rician_posterior(model, b, y, atoms, lo, hi, sd, log_prior=lp, **kw)
    S = signals(model, b, atoms, **kw)
    ll = rice.logpdf(y[:, None, :], S[None] / sd, scale=sd).sum(axis=2) + lp[None]
    top = ll.max(axis=1, keepdims=True)
    ev = top[:, 0] + np.log(np.exp(ll - top).sum(axis=1))
    post = np.exp(ll - ev[:, None])
    np.testing.assert_allclose(ref["log_evidence"], ev - np.log(np.exp(lp).sum()), rtol=0, atol=1e-10)
    np.testing.assert_allclose(ref["mean"], post @ atoms.T, rtol=1e-10, atol=0)
    var = post @ (atoms.T ** 2) - (post @ atoms.T) ** 2  # the textbook form cancels: 1e-9 of the largest square
    assert (np.abs(ref["var"] - var) <= 1e-9 * (atoms.max(axis=1) ** 2)[None]).all()
    assert (ref["map_atom"] == ll.argmax(axis=1)).all() and ref["finite"].all()


def test_reference_is_the_gaussian_one_at_high_snr():
    """SNR >= 1000 on every b-value: z = y s / sd^2 >= 1e6 and h(z) = -log(2 pi z) / 2 + 1 / (8 z) + ...; the first term is a constant
    of the voxel plus -1/2 sum_i log s_gi, which goes into log_prior; what is left, at most n_b / (8 z_min) per atom, goes into eps."""
    rng = np.random.default_rng(11)
    b = np.linspace(0.0, 400.0, 8)
    atoms = np.stack([rng.uniform(0.1, 0.4, 40), rng.uniform(0.02, 0.05, 40), rng.uniform(5e-4, 2e-3, 40)])
    truth = atoms[:, rng.integers(0, 40, 30)]
    S = signals("bi_reduced", b, atoms)
    sd = S.min() / 2000.0
    y = synth.rician_magnitude(signals("bi_reduced", b, truth), sd, seed=1)
    assert (y / sd).min() >= 1000 and (S / sd).min() >= 1000
    lo, hi = np.zeros(3), np.ones(3)
    left = len(b) / (8 * (y.min() * S.min() / sd ** 2))
    ric = R.rician_posterior("bi_reduced", b, y, atoms, lo, hi, sd, extra_eps=left, max_eps=1e-4)
    gau = gauss_reference("bi_reduced", b, y, atoms, lo, hi, log_prior=-0.5 * np.log(S).sum(axis=1), noise_sd=sd, max_eps=1e-4)
    assert (np.abs(ric["mean"] - gau["mean"]) <= ric["bound_mean"] + gau["bound_mean"]).all()
    assert (np.abs(ric["var"] - gau["var"]) <= ric["bound_var"] + gau["bound_var"]).all()
    assert (ric["map_atom"] == gau["map_atom"]).mean() > 0.9


@pytest.mark.parametrize("name", list(K.CASES))
def test_reference_preconditions_hold_on_every_gpu_case(name):
    c = K.build(name)
    ref = R.rician_posterior(c["model"], c["b"], c["y"], c["atoms"], c["lo"], c["hi"], c["noise_sd"], log_prior=c["log_prior"], **c["kw"])
    assert ref["finite"].all() and (c["y"] >= 0).all() and ref["eps"].max() <= 1e-6
    assert ((c["atoms"] >= c["lo"][:, None]) & (c["atoms"] <= c["hi"][:, None])).all()


def test_cases_cover_the_kernel_paths():
    shapes = [(K.CASES[n][1], K.CASES[n][2], K.build(n)["atoms"].shape[1]) for n in K.CASES]
    assert {1, 15, 16, 17, 83, 200} <= {s[0] for s in shapes} and {4, 5, 33, 128} <= {s[1] for s in shapes}
    assert {1, 17} <= {s[2] for s in shapes} and any(K.CASES[n][3] == "slab+16" for n in K.CASES)
    assert {K.CASES[n][0] for n in K.CASES} == set(api.MODEL_PARAM_NAMES)
    # every compiled form: NF = 3 / 6 / 8 (n_free <= 3, <= 6, beyond) x NS = 8 / 32 (n_b <= 32, beyond)
    forms = {(3 if nf <= 3 else 6 if nf <= 6 else 8, 8 if K.CASES[n][2] <= 32 else 32)
             for n in K.CASES for nf in [len(K.names_of(K.CASES[n][0], K.CASES[n][5]))]}
    assert forms == {(nf, ns) for nf in (3, 6, 8) for ns in (8, 32)}


# ---- worth, on the reference alone
def _worth(sd, b_max):
    p = K.worth_population(sd, b_max)
    ric = R.rician_posterior("bi_reduced", p["b"], p["y"], p["atoms"], p["lo"], p["hi"], sd)
    gau = gauss_reference("bi_reduced", p["b"], p["y"], p["atoms"], p["lo"], p["hi"], noise_sd=sd)
    med = lambda r: np.median(np.abs(r["mean"].T - p["truth"]), axis=1)
    bias = lambda r: (r["mean"].T - p["truth"]).mean(axis=1)
    return med(ric) / med(gau), bias(ric), bias(gau)


def test_worth_of_the_rician_likelihood_on_the_reference():
    """The table of DESIGN.md 4.1t / README, printed whole; the asserted cell is the strongest: noise 0.10, b up to 2500, the slow rate
    D2 -- measured 0.288, asserted at measured + 0.1.  The fast rate D1 does NOT gain in any cell (1.05 to 1.14); the table says so."""
    table = {}
    for sd, b_max in K.WORTH_CELLS:
        ratio, bias_r, bias_g = table[(sd, b_max)] = _worth(sd, b_max)
        print(f"noise {sd} b <= {b_max}: median |error| Rician / Gaussian (f1, D1, D2) {np.round(ratio, 3)}; mean signed error Rician "
              f"{bias_r}, Gaussian {bias_g}")
    sd, b_max, k = K.WORTH_ASSERTED
    ratio, bias_r, bias_g = table[(sd, b_max)]
    assert ratio[k] == min(r[0].min() for r in table.values())  # the strongest cell is the asserted one
    assert ratio[k] <= K.WORTH_ASSERTED_RATIO < 0.9
    assert abs(bias_r[k]) < abs(bias_g[k])


# ---- the solver's options
def _bi(**kw):
    grid = {n: list(K.WORTH_GRID[n]) for n in ("f1", "D1", "D2")}
    return HipBayesGridSolver(BiExpModel(), grid, bounds=dict(K.WORTH_BOUNDS), **kw)


def test_solver_noise_model_options():
    assert _bi().noise_model == "gaussian" and _bi(noise_model="gaussian", noise_sd=0.05).noise_model == "gaussian"
    s = _bi(noise_model="rician", noise_sd=0.05)
    assert s.noise_model == "rician" and s.project is False and not s.needs_labels and not s.needs_neighbours
    for bad in ("rice", "Rician", None, 1):
        with pytest.raises(ValueError, match="noise_model must be 'gaussian' or 'rician'"):
            _bi(noise_model=bad, noise_sd=0.05)
    not_built = "noise_model 'rician' is not built with "
    for kw, what in ((dict(), "a marginalised noise scale"), (dict(noise_sd=0.0), "a marginalised noise scale"),
                     (dict(noise_sd=0.05, sigma=0.1), "sigma"), (dict(noise_sd=0.05, empirical_prior=True), "empirical_prior"),
                     (dict(noise_sd=0.05, spatial_prior={"strength": 4}), "spatial_prior"), (dict(noise_sd=0.05, marginals=True), "marginals"),
                     (dict(noise_sd=0.05, log_prior=np.zeros((2, 1215))), "per-label priors")):
        with pytest.raises(ValueError, match=re.escape(not_built + what)):
            _bi(noise_model="rician", **kw)
    s0 = dict(p0={"f1": 0.2, "D1": 0.01, "D2": 0.001, "S0": 1.0}, bounds={"f1": (0, 1), "D1": (1e-3, 0.1), "D2": (1e-5, 5e-3), "S0": (0.0, 10.0)})
    with pytest.raises(ValueError, match=re.escape(not_built + "a projected S0")):
        HipBayesGridSolver(BiExpModel(fit_s0=True), {"D1": [0.01, 0.05]}, **s0, noise_sd=0.05, noise_model="rician", project=True)
    on_grid = HipBayesGridSolver(BiExpModel(fit_s0=True), {"D1": [0.01, 0.05], "S0": [0.9, 1.1]}, **s0, noise_sd=0.05, noise_model="rician")
    assert on_grid.project is False and on_grid._atoms.shape == (4, 4)
    assert HipBayesGridSolver(BiExpModel(fit_s0=True), {"D1": [0.01, 0.05]}, **s0).project is True  # the Gaussian default, unchanged
    # the TOML loader's call: [Fitting.solver] noise_model = "rician" arrives as a keyword beside the arguments it always passes
    t = HipBayesGridSolver(BiExpModel(), {"f1": [0.1, 0.2]}, max_iter=100, tol=1e-6, p0={"D1": 0.02, "D2": 1e-3}, bounds=dict(K.WORTH_BOUNDS),
                           noise_sd=0.05, noise_model="rician", method="trf", multi_threading=True)
    assert t.noise_model == "rician" and t.solver_kwargs == {"method": "trf", "multi_threading": True}
    doc = HipBayesGridSolver.__doc__
    assert "noise_model" in doc and "rician" in doc and "pnx_curvefit_grid_posterior_rician_f64" in doc


def test_toml_round_trip():
    try:
        import tomllib
    except ImportError:  # Python 3.10
        import tomli as tomllib
    text = '[Fitting.solver]\nnoise_model = "rician"\nnoise_sd = 0.05\n[Fitting.solver.grid]\nf1 = [0.1, 0.2]\nD1 = [0.02]\nD2 = [0.001]\n'
    table = tomllib.loads(text)["Fitting"]["solver"]
    s = HipBayesGridSolver(BiExpModel(), max_iter=250, tol=1e-8, bounds=dict(K.WORTH_BOUNDS), **table)
    assert s.noise_model == "rician" and s.noise_sd == 0.05 and s._atoms.shape == (3, 2)


def test_default_path_is_unchanged(monkeypatch):
    """noise_model='gaussian' calls api.grid_posterior with the arguments it had; 'rician' calls the new entry."""
    calls = []
    fake = dict(mean=np.zeros((3, 2)), sd=np.zeros((3, 2)), map_p=np.zeros((3, 2)), map_atom=np.zeros(2, np.int32), log_evidence=np.zeros(2),
                ess=np.ones(2))
    monkeypatch.setattr(api, "grid_posterior", lambda *a, **k: calls.append(("gaussian", k)) or fake)
    monkeypatch.setattr(api, "grid_posterior_rician", lambda *a, **k: calls.append(("rician", k)) or fake)
    b, y = np.linspace(0, 1000, 8), np.ones((2, 8))
    g = _bi(noise_sd=0.05).fit(b, y)
    r = _bi(noise_sd=0.05, noise_model="rician").fit(b, y)
    assert [c[0] for c in calls] == ["gaussian", "rician"]
    assert set(calls[0][1]) == {"log_prior", "noise_sd", "fixed_idx", "fixed_vals", "sigma", "project_amplitude", "device"} | set(g._kernel_t1)
    assert calls[1][1]["noise_sd"] == 0.05 and "project_amplitude" not in calls[1][1] and "sigma" not in calls[1][1]
    assert "noise_model" not in g.diagnostics_ and r.diagnostics_["noise_model"] == "rician"


def test_no_cpu_fallback_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is visible here")
    p = K.worth_population(0.1, 1000.0, n_vox=4)
    with pytest.raises(_lib.PnxError):
        api.grid_posterior_rician("bi_reduced", p["b"], p["y"], p["atoms"], p["lo"], p["hi"], noise_sd=0.1)
    with pytest.raises(_lib.PnxError):
        api.log_i0e(np.ones(3))
    with pytest.raises(_lib.PnxError):
        _bi(noise_sd=0.1, noise_model="rician").fit(p["b"], p["y"])


# ---- the ABI without a device
def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnx.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    for name, n_args in ((POSTERIOR, 20), (LOG_I0E, 6)):
        assert re.search(r"PNX_API\s+int\s+" + name + r"\s*\(", text) and name in _lib.ABI_SYMBOLS and name in exported
        fn = getattr(_lib.load(), name)
        assert len(fn.argtypes) == n_args and fn.restype is C.c_int
    for name in ("grid_posterior_rician", "grid_posterior_rician_device", "log_i0e", "grid_rician_slab_atoms"):
        assert callable(getattr(api, name))
    assert callable(synth.rician_magnitude)


def _abi_call(noise_sd=0.05, sigma=None, atom=0.5, mean=True, n_vox=3, log_prior=None):
    o = api.make_opts("bi_reduced", 16, sigma=sigma)
    atoms, lo, hi, b, y = np.full((3, 4), 0.5), np.zeros(3), np.ones(3), np.zeros(16), np.ones((max(n_vox, 1), 16))
    atoms[1, 2] = atom
    out = np.full((3, max(n_vox, 1)), 9.0)
    lp = None if log_prior is None else np.asarray(log_prior, float)
    rc = _lib.load().pnx_curvefit_grid_posterior_rician_f64(C.byref(o), n_vox, _lib.ptr(b), _lib.ptr(y), 4, _lib.ptr(atoms), None, _lib.ptr(lo),
                                                            _lib.ptr(hi), _lib.ptr(lp), noise_sd, _lib.ptr(out) if mean else None, None, None,
                                                            None, None, None, 0, 0, None)
    return rc, out


def test_refusals_need_no_device():
    err = _lib.last_error
    for bad in (0.0, -0.05, np.nan, np.inf, -np.inf):
        rc, out = _abi_call(noise_sd=bad)
        assert rc == -1 and "noise_sd" in err() and "finite and > 0" in err() and (out == 9.0).all()
    rc, out = _abi_call(sigma=np.ones(16))
    assert rc == -2 and "sigma is not built" in err() and (out == 9.0).all()
    assert _abi_call(atom=1.5)[0] == -1 and "atom 2, free parameter 1" in err()
    assert _abi_call(mean=False)[0] == -1 and "mean is NULL" in err()
    assert _abi_call(log_prior=[-np.inf] * 4)[0] == -1 and "log_prior" in err()
    assert _abi_call(n_vox=0)[0] == 0
    lib = _lib.load()
    z = np.ones(4)
    assert lib.pnx_log_i0e_f64(-1, _lib.ptr(z), _lib.ptr(z), 0, 0, None) == -1 and "n < 0" in err()
    assert lib.pnx_log_i0e_f64(4, None, _lib.ptr(z), 0, 0, None) == -1 and "NULL" in err()
    assert lib.pnx_log_i0e_f64(4, _lib.ptr(z), _lib.ptr(z), 5, 0, None) == -1 and "mem=5" in err()
    assert lib.pnx_log_i0e_f64(0, None, None, 0, 0, None) == 0
    if _lib.device_count() == 0:  # a valid call stops at the device
        assert _abi_call()[0] == -3 and lib.pnx_log_i0e_f64(4, _lib.ptr(z), _lib.ptr(z), 0, 0, None) == -3


def test_synth_rician_magnitude():
    clean = np.linspace(0.0, 1.0, 5000).reshape(100, 50)
    a, b2 = synth.rician_magnitude(clean, 0.1, seed=3), synth.rician_magnitude(clean, 0.1, seed=3)
    assert a.tobytes() == b2.tobytes() and a.shape == clean.shape and (a >= 0).all() and a.flags.c_contiguous
    assert synth.rician_magnitude(clean, 0.1, seed=4).tobytes() != a.tobytes()
    assert synth.rician_magnitude(clean, 0.0).tobytes() == clean.tobytes()
    floor = synth.rician_magnitude(np.zeros(200000), 0.1, seed=0).mean()  # Rayleigh: sd sqrt(pi / 2)
    assert abs(floor - 0.1 * np.sqrt(np.pi / 2)) < 1e-3

"""The marginals of the variable-projection posterior (pnx_curvefit_varpro_marginals_f64, api.varpro_marginals,
HipBayesVarProSolver's marginals), the parts that need no GPU: the host-side argument checks, the table of bin indices and the
choice of the instantiation under AddressSanitizer / UBSan (a stand-alone program, tests/host_stub/varpro_marginal_args_stub.cpp),
the symbol, the ABI's refusals in front of any device work, the solver's option rules, the numpy reference against a brute-force
loop, its preconditions on the inputs of every GPU case, and the kernel's running-maximum arithmetic restated in numpy against the
two-pass reference."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT
from varpro_marginal_cases import cases, ref_kw
from varpro_marginal_reference import full_bins, geo_reference, reference, running_maximum
from varpro_reference import case_atoms, case_signals

from pyneapple_amd import _lib, api
from pyneapple_amd.models import TriExpModel
from pyneapple_amd.solvers import HipBayesGridSolver, HipBayesVarProSolver

NAME = "pnx_curvefit_varpro_marginals_f64"


# ---- the argument checks as a stand-alone program under the sanitizers
@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("stub") / "varpro_marginal_args_stub")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "pyneapple_amd", "csrc"), os.path.join(ROOT, "tests", "host_stub", "varpro_marginal_args_stub.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode and any(s in b.stderr for s in ("cannot find -lasan", "cannot find -lubsan")):
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-4000:]
    return exe


def test_argument_checks_are_clean_under_sanitizers(stub):
    """Every refusal by name -- bins on a fraction or S0, B = 0 and 129, a bin out of range, an atom off its bin's value, values that
    do not ascend, a level at 0 or 1, n_q = 9, NULL outputs, the posterior's and the variable projection's own -- the edges
    accepted, the table of global bin indices with its -1 padding, 4 / 8 chunks, the table inside the slab for every n_b and k."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=1")
    r = subprocess.run([stub], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-6000:]
    assert r.returncode == 0, out[-4000:]
    assert "varpro marginal args stub ok" in r.stdout


# ---- the ABI without a device
def _grid():
    """bi_reduced (f1, D1, D2) over 3 x 2 rates: (nl_atoms (2, 6), n_bins (3,), bin_of (3, 6), bin_value (5,))."""
    atoms = np.ascontiguousarray(np.array([(a, c) for a in (0.05, 0.1, 0.2) for c in (1e-3, 2e-3)]).T)
    return (atoms, *full_bins(3, [1, 2], atoms))


def _call(atoms, n_bins, bin_of, bin_value, probs=(0.5,), n_vox=1, noise_sd=0.0, marginal=True, quantile=True, n_q=None, model="bi_reduced",
          amplitudes=1):
    o = api.make_opts(model, 32)
    n = o.n_free
    atoms = np.ascontiguousarray(atoms, float)
    lo, hi = np.zeros(n), np.ones(n)
    b, y = np.zeros(128), np.ones(128)
    n_bins, bin_of = np.ascontiguousarray(n_bins, np.int32), np.ascontiguousarray(bin_of, np.int32)
    bin_value, probs = np.ascontiguousarray(bin_value, float), np.ascontiguousarray(probs, float)
    res = dict(marginal=np.full((max(int(n_bins.sum()), 1), max(n_vox, 1)), 9.0), quantile=np.full((8, n, max(n_vox, 1)), 9.0),
               geo_mean=np.full((n, max(n_vox, 1)), 9.0), log_evidence=np.full(max(n_vox, 1), 9.0))
    rc = _lib.load().pnx_curvefit_varpro_marginals_f64(C.byref(o), n_vox, _lib.ptr(b), _lib.ptr(y), atoms.shape[1], _lib.ptr(atoms), None,
                                                       _lib.ptr(lo), _lib.ptr(hi), None, noise_sd, amplitudes, _lib.ptr(n_bins), _lib.ptr(bin_of),
                                                       _lib.ptr(bin_value), len(probs) if n_q is None else n_q, _lib.ptr(probs),
                                                       _lib.ptr(res["marginal"]) if marginal else None,
                                                       _lib.ptr(res["quantile"]) if quantile else None, _lib.ptr(res["geo_mean"]),
                                                       _lib.ptr(res["log_evidence"]), 0, 0, None)
    return rc, res


def test_symbol_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnx.h")).read(), flags=re.S)
    assert re.search(r"PNX_API\s+int\s+" + NAME + r"\s*\(", text)
    assert NAME in _lib.ABI_SYMBOLS
    fn = getattr(_lib.load(), NAME)
    assert len(fn.argtypes) == 24 and fn.restype is C.c_int
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert NAME in [ln.split()[-1] for ln in out.splitlines() if ln.strip()]


def test_abi_refusals_need_no_device():
    atoms, n_bins, bin_of, bin_value = _grid()
    err = lambda **kw: (_call(**{**dict(atoms=atoms, n_bins=n_bins, bin_of=bin_of, bin_value=bin_value), **kw})[0], _lib.last_error())
    rc, msg = err(n_bins=[0, 0, 0], bin_value=[0.5])
    assert rc == -1 and "sum n_bins = 0" in msg
    rc, msg = err(n_bins=[2, 3, 2], bin_value=np.r_[0.1, 0.2, bin_value])
    assert rc == -1 and "n_bins[0]=2" in msg and "linear row" in msg
    rc, msg = err(n_bins=[0, 3, 126], bin_value=np.linspace(0.1, 0.9, 129))
    assert rc == -1 and "129" in msg
    bad = bin_of.copy()
    bad[2, 4] = 2
    rc, msg = err(bin_of=bad)
    assert rc == -1 and "bin_of[2, 4]=2" in msg
    off = bin_value.copy()
    off[4] = 2.5e-3
    rc, msg = err(bin_value=off)
    assert rc == -1 and "atom" in msg and "bin_value[4]" in msg
    desc = bin_value.copy()
    desc[[3, 4]] = desc[[4, 3]]
    rc, msg = err(bin_value=desc)
    assert rc == -1 and "ascending" in msg
    for p in (0.0, 1.0, float("nan")):
        rc, msg = err(probs=[0.5, p])
        assert rc == -1 and "probs[1]" in msg
    rc, msg = err(probs=[0.5] * 9)
    assert rc == -1 and "n_q=9" in msg
    rc, msg = err(marginal=False)
    assert rc == -1 and "marginal is NULL" in msg
    rc, msg = err(quantile=False)
    assert rc == -1 and "quantile is NULL" in msg
    rc, msg = err(noise_sd=-1.0)
    assert rc == -1 and "noise_sd" in msg
    rc, msg = err(amplitudes=2)
    assert rc == -1 and "marginal_amplitudes=2" in msg
    same = atoms.copy()
    same[1, 0] = same[0, 0]  # the variable projection's own refusal: two equal rates in an atom
    rc, msg = err(atoms=same)
    assert rc == -1 and "two equal rates" in msg
    rc, res = _call(atoms, n_bins, bin_of, bin_value, probs=[1.0])  # a refused call writes nothing
    assert rc == -1 and all((res[k] == 9.0).all() for k in res)
    assert _call(atoms, n_bins, bin_of, bin_value, n_vox=0)[0] == 0  # no voxels: nothing to do, no device needed
    if _lib.device_count() == 0:  # valid calls stop at the device
        assert _call(atoms, n_bins, bin_of, bin_value)[0] == -3
        assert _call(atoms, n_bins, bin_of, bin_value, probs=(), quantile=False)[0] == -3


def test_no_cpu_fallback_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is visible here")
    b, y = case_signals("tri_s0", 4)
    with pytest.raises(_lib.PnxError):
        api.varpro_marginals("tri_s0", b, y, case_atoms("tri_s0"), np.zeros(6), np.ones(6))
    with pytest.raises(_lib.PnxError):
        _solver(marginals=True).fit(b, y)


def test_api_derives_the_binning_and_refuses_a_malformed_one(monkeypatch):
    o = api.make_opts("tri_s0", 32)
    atoms = case_atoms("tri_s0")
    got = api._varpro_marginal_bins(o, "tri_s0", atoms, None)
    want = full_bins(6, [1, 3, 4], atoms)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    assert got[0].tolist() == [0, 4, 0, 4, 4, 0]
    monkeypatch.setattr(_lib, "require_device", lambda: None)
    b, y = case_signals("tri_s0", 4)
    lo, hi = np.zeros(6), np.ones(6)
    with pytest.raises(ValueError, match="bins must be"):
        api.varpro_marginals("tri_s0", b, y, atoms, lo, hi, bins=(np.ones(3, np.int32), np.zeros((3, 64), np.int32), np.zeros(3)))
    with pytest.raises(_lib.PnxError, match="n_q=9"):
        api.varpro_marginals("tri_s0", b, y, atoms, lo, hi, quantiles=[0.5] * 9)


# ---- the solver's option rules
BOUNDS = {"f1": (-40.0, 40.0), "D1": (1e-5, 0.5), "f2": (-40.0, 40.0), "D2": (1e-5, 0.5), "D3": (1e-5, 0.5), "S0": (0.0, 10.0)}
P0 = {"f1": 0.2, "D1": 0.1, "f2": 0.3, "D2": 0.01, "D3": 0.001, "S0": 1.0}
TRI = {"D1": [0.04, 0.3], "D2": [4e-3, 0.02], "D3": [3e-4, 1.5e-3]}


def _solver(**kw):
    return HipBayesVarProSolver(TriExpModel(fit_s0=True), TRI, p0=P0, bounds=BOUNDS, **kw)


def test_solver_marginals_rules():
    default = {"quantiles": (0.025, 0.5, 0.975)}
    for off in (None, False):
        assert _solver(marginals=off).marginals is None
    assert _solver().marginals is None
    assert _solver(marginals=True).marginals == default and _solver(marginals={}).marginals == default
    # the TOML loader's call: a table arrives as a plain dict, beside the arguments it always passes
    s = _solver(max_iter=100, tol=1e-6, method="trf", marginals={"quantiles": [0.1, 0.9]})
    assert s.marginals == {"quantiles": (0.1, 0.9)} and s.solver_kwargs == {"method": "trf"}
    assert _solver(marginals={"quantiles": []}).marginals == {"quantiles": ()}
    assert _solver(marginals={"quantiles": 0.5}).marginals == {"quantiles": (0.5,)}
    with pytest.raises(ValueError, match=r"unknown keys \['levels', 'probs'\]"):
        _solver(marginals={"probs": [0.5], "levels": 1, "quantiles": [0.5]})
    for bad in ([0.0], [1.0], [0.5, -0.1], [float("nan")], [0.5] * 9, ["median"], "lots"):
        with pytest.raises(ValueError, match="quantiles"):
            _solver(marginals={"quantiles": bad})
    for value in ("yes", 3, [("quantiles", [0.5])]):
        with pytest.raises(ValueError, match="marginals"):
            _solver(marginals=value)
    # one set of rules and messages for the two solvers: the same function
    assert HipBayesVarProSolver._marginals_options.__func__ is HipBayesGridSolver._marginals_options.__func__
    doc = HipBayesVarProSolver.__doc__
    assert "marginals" in doc and "[Fitting.solver.marginals]" in doc and "interpolated" in doc and "geo_mean" in doc


# ---- the numpy reference against a brute-force loop
def test_reference_on_a_tiny_case():
    """One voxel layout written out by hand: five atoms (one excluded) over 2 x 3 values, the geometric mean from the bins."""
    from grid_marginal_reference import marginals, weights

    ell = np.log(np.array([[1.0, 2.0, 3.0, 0.0, 4.0], [5.0, 1.0, 1.0, 0.0, 3.0]]), where=[True, True, True, False, True],
                 out=np.full((2, 5), -np.inf))
    n_bins, bin_of, bin_value = [0, 2, 3], np.array([[0] * 5, [0, 1, 0, 1, 1], [2, 0, 0, 1, 2]]), np.array([0.01, 0.1, 1e-3, 2e-3, 4e-3])
    marg = marginals(weights(ell), n_bins, bin_of)
    want = np.zeros((2, 5))
    W = np.array([[1, 2, 3, 0, 4], [5, 1, 1, 0, 3]]) / 10.0
    for v in range(2):
        off = 0
        for k in range(3):
            for g in range(5):
                if n_bins[k]:
                    want[v, off + bin_of[k, g]] += W[v, g]
            off += n_bins[k]
    np.testing.assert_allclose(marg, want, rtol=1e-15)
    assert (marg[:, 3] == 0).all()  # the bin only the excluded atom occupies: exactly 0
    S, bound = geo_reference(marg, np.full(2, 1e-9), n_bins, bin_value)
    assert np.isnan(S[:, 0]).all() and np.isnan(bound[:, 0]).all()
    brute = [[sum(W[v, g] * np.log(bin_value[o + bin_of[k, g]]) for g in range(5)) for k, o in ((1, 0), (2, 2))] for v in range(2)]
    np.testing.assert_allclose(S[:, 1:], brute, rtol=1e-14)
    np.testing.assert_allclose(np.exp(S[0, 1]), 0.01 ** 0.4 * 0.1 ** 0.6, rtol=1e-14)
    assert (bound[:, 1:] > 0).all() and (bound[:, 1:] < 1e-8).all()
    S0, _ = geo_reference(marg, np.full(2, 1e-9), n_bins, np.array([0.0, 0.1, 1e-3, 2e-3, 4e-3]))
    assert np.isnan(S0[:, 1]).all() and np.isfinite(S0[:, 2]).all()  # a grid value <= 0: no geometric mean for that parameter


def _reference_of(case, probs=(0.025, 0.5, 0.975)):
    o = api.make_opts(case["model"], len(case["b"]), case["kw"].get("fixed_idx", ()), t1_mode=case["kw"].get("t1_mode", 0))
    bins = api._varpro_marginal_bins(o, case["model"], case["atoms"], None)
    return bins, reference(case["model"], case["b"], case["y"], case["atoms"], case["lo"], case["hi"], *bins, probs=probs, **ref_kw(case))


@pytest.fixture(scope="module")
def references():
    return {name: _reference_of(case) for name, case in cases().items()}


def test_reference_preconditions_of_the_gpu_cases(references):
    """The reference alone on the inputs of every GPU case: eps_v <= 1e-6 on every finite voxel (the reference asserts it, and that
    no voxel sits on the cancellation floor); the narrow box alone is accepted at the explicit 1e-3."""
    all_cases = cases()
    assert set(references) == set(all_cases)
    for name, (bins, ref) in references.items():
        fin = ref["finite"]
        cap = 1e-3 if name == "narrow-box" else 1e-6
        assert all_cases[name]["max_eps"] == cap
        assert fin.all() and (ref["post"]["eps"][fin] <= cap).all(), name
        assert (ref["rel"] < 1e-2).all() and np.isfinite(ref["marginal"]).all()
    # what the special cases are there for
    # atoms 0..15 share D1's first grid value, atoms 16..31 its second: a bin that holds excluded atoms only, exactly 0
    assert references["first-tile-excluded"][1]["empty"].tolist() == [True] + [False] * 11
    assert references["middle-tile-excluded"][1]["empty"].tolist() == [False, True] + [False] * 10
    far = references["far-atoms-underflow"][1]
    assert ((far["marginal"] == 0) & ~far["empty"][None, :]).any(), "no occupied bin underflows to exactly 0"
    last = references["best-atom-last"][1]["post"]["l"]
    assert (np.diff(last.reshape(40, 4, 16).max(axis=2), axis=1) > 0).all() and (last.argmax(axis=1) == 63).all()
    assert references["narrow-box"][1]["post"]["clipped_mass"].mean() > 0.5


def test_running_maximum_arithmetic_against_the_two_pass_reference(references):
    """The kernel's one pass restated in numpy -- tile by tile, the rescale by alpha = exp(m - m') included -- on the l_g of every
    GPU case: every bin within rel_v ref + 1e-300 of the two-pass reference, L_v within the evidence's bound."""
    for name, ((n_bins, bin_of, _), ref) in references.items():
        post = ref["post"]
        marg, L = running_maximum(post["l"], n_bins, bin_of)
        assert (np.abs(marg - ref["marginal"]) <= ref["bound"]).all(), name
        assert (marg[:, ref["empty"]] == 0).all(), name
        # L itself: the prior's normaliser is the same constant on both sides
        two_pass = post["l"].max(axis=1) + np.log(np.exp(post["l"] - post["l"].max(axis=1)[:, None]).sum(axis=1))
        assert (np.abs(L - two_pass) <= ref["bound_log_evidence"]).all(), name
    # tiles of -inf in front, in the middle and alone: no NaN from (-inf) - (-inf)
    ell = np.full((3, 48), -np.inf)
    ell[0, 40], ell[1, 20], ell[1, 47], ell[2, 0] = -3.0, 700.0, -700.0, 5.0
    marg, L = running_maximum(ell, [48], np.arange(48)[None])
    assert np.isfinite(marg).all() and marg[0, 40] == 1.0 and marg[1, 20] == 1.0 and marg[1, 47] == 0.0 and marg[2, 0] == 1.0
    assert L.tolist() == [-3.0, 700.0, 5.0]

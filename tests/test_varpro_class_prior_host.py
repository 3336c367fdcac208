"""One prior row per segmentation label over the variable-projection dictionary (pnx_curvefit_varpro_posterior_classes_f64,
pnx_curvefit_varpro_prior_em_classes_f64, api.varpro_posterior_classes / varpro_prior_em_classes, HipBayesVarProSolver's per_label),
the parts that need no GPU: the host-side checks, starts, centres, report and slab sizing under AddressSanitizer / UBSan (a
stand-alone program, tests/host_stub/varpro_class_args_stub.cpp), the ABI's refusals in front of any device work, the solver's
option parsing, the label -> row mapping and its ValueErrors, the fitter's hand-over of segmentation[mask], the numpy reference on a
case worked by hand, and the CPU precondition of the GPU file's worth test."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT
from varpro_class_prior_reference import em_step_classes, normalise_rows, posterior, worth
from varpro_prior_reference import em_step
from varpro_reference import case_signals

from pyneapple_amd import _lib, api
from pyneapple_amd.fitters import HipPixelWiseFitter
from pyneapple_amd.models import BiExpModel
from pyneapple_amd.solvers import HipBayesGridSolver, HipBayesVarProSolver

POST, EM = "pnx_curvefit_varpro_posterior_classes_f64", "pnx_curvefit_varpro_prior_em_classes_f64"


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("stub") / "varpro_class_args_stub")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "pyneapple_amd", "csrc"), os.path.join(ROOT, "tests", "host_stub", "varpro_class_args_stub.cpp"), "-o", exe]
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
    """n_classes outside [1, 16], labels NULL, a row without a finite entry (named), a NaN / +inf entry (named), the unlabelled
    calls' refusals behind them, the centres, the starts and the report, and the slab inside 64 KB for every n_classes x k x n_b."""
    assert "varpro class args stub ok" in _run_stub(stub)


@pytest.mark.parametrize("n_b", [1, 32, 33, 128])
def test_slab_stays_inside_the_lds_budget_and_python_agrees(stub, n_b):
    kpad = (n_b + 3) & ~3
    for k in (1, 2, 3):
        for n_classes in range(1, 17):
            for extra in (k + 1, 4 * n_classes):  # the posterior; both EM passes
                w = api.varpro_class_slab_atoms(n_b, k, n_classes, extra)
                assert int(_run_stub(stub, n_b, k, n_classes, extra)) == w
                doubles = k * kpad * (w if w & 16 else w + 16) + (k * (k + 1) + n_classes + extra) * w
                assert w >= 16 and w % 16 == 0 and doubles * 8 <= 64 * 1024
        assert api.varpro_class_slab_atoms(n_b, k, 1, k + 1) == api.varpro_posterior_slab_atoms(n_b, k)
        assert api.varpro_class_slab_atoms(n_b, k, 1, 4) == api.varpro_prior_slab_atoms(n_b, k)
    if n_b == 32:
        assert api.varpro_class_slab_atoms(32, 3, 1, 4) == 48 and api.varpro_class_slab_atoms(32, 3, 16, 64) == 32


# ---- the ABI without a device
def _call(name, o, n_vox=1, n_atoms=4, n_classes=2, labels=True, log_prior=None, noise_sd=0.0, marg=1, n_iter=3, out=True):
    n = o.n_free
    nl = np.ascontiguousarray(np.stack([np.linspace(0.1, 0.2, max(n_atoms, 1)), np.full(max(n_atoms, 1), 0.01)]))  # bi_reduced: D1 > D2
    lo, hi = np.zeros(n), np.ones(n)
    b, y = np.zeros(128), np.ones(128)
    lab = np.zeros(max(n_vox, 1), np.int32)
    rows = max(min(n_classes, 16), 1)
    lp = None if log_prior is None else np.ascontiguousarray(log_prior, float)
    head = (C.byref(o), n_vox, _lib.ptr(b), _lib.ptr(y), n_atoms, _lib.ptr(nl), None, _lib.ptr(lo), _lib.ptr(hi), n_classes,
            _lib.ptr(lab) if labels else None, _lib.ptr(lp), noise_sd, marg)
    if name == POST:
        res = dict(mean=np.full((n, max(n_vox, 1)), 9.0))
        rc = _lib.load().pnx_curvefit_varpro_posterior_classes_f64(*head, _lib.ptr(res["mean"]) if out else None, None, None, None, None, None, None,
                                                                   0, 0, None)
    else:
        res = dict(log_prior=np.full((rows, max(n_atoms, 1)), 9.0), loglik=np.full(n_iter + 1, 9.0), loglik_class=np.full((n_iter + 1, rows), 9.0),
                   done=C.c_int(-7), n_eff=np.full(rows, -7, np.int64))
        rc = _lib.load().pnx_curvefit_varpro_prior_em_classes_f64(*head, n_iter, 0.0, 0.0, _lib.ptr(res["log_prior"]) if out else None,
                                                                  _lib.ptr(res["loglik"]), _lib.ptr(res["loglik_class"]), C.byref(res["done"]),
                                                                  _lib.ptr(res["n_eff"]), 0, 0, None)
    return rc, res


def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnx.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    unlabelled = {POST: "pnx_curvefit_varpro_posterior_f64", EM: "pnx_curvefit_varpro_prior_em_f64"}
    for name, n_args in ((POST, 24), (EM, 25)):
        assert re.search(r"PNX_API\s+int\s+" + name + r"\s*\(", text) and name in _lib.ABI_SYMBOLS and name in exported
        fn = getattr(_lib.load(), name)
        assert len(fn.argtypes) == n_args and fn.restype is C.c_int
        assert n_args == len(getattr(_lib.load(), unlabelled[name]).argtypes) + (2 if name == POST else 3)  # n_classes, labels (, loglik_class)
    for name in ("varpro_posterior_classes", "varpro_posterior_classes_device", "varpro_prior_em_classes", "varpro_prior_em_classes_device",
                 "varpro_class_slab_atoms"):
        assert callable(getattr(api, name))


@pytest.mark.parametrize("name", [POST, EM])
def test_abi_refusals_need_no_device(name):
    mk = lambda: api.make_opts("bi_reduced", 32)
    for bad in (0, -1, 17):
        assert _call(name, mk(), n_classes=bad)[0] == -1 and "n_classes" in _lib.last_error() and "[1,16]" in _lib.last_error()
    assert _call(name, mk(), labels=False)[0] == -1 and "labels" in _lib.last_error()
    table = np.zeros((2, 4))
    table[1] = -np.inf
    assert _call(name, mk(), log_prior=table)[0] == -1 and "row 1" in _lib.last_error() and "excludes every atom" in _lib.last_error()
    for bad in (np.nan, np.inf):
        table = np.zeros((2, 4))
        table[1, 2] = bad
        assert _call(name, mk(), log_prior=table)[0] == -1 and "log_prior[1, 2]" in _lib.last_error()
    # the unlabelled refusals behind them
    assert _call(name, mk(), noise_sd=-1.0)[0] == -1 and "noise_sd" in _lib.last_error()
    assert _call(name, mk(), marg=2)[0] == -1 and "marginal_amplitudes" in _lib.last_error()
    assert _call(name, mk(), n_atoms=0)[0] == -1 and "n_atoms" in _lib.last_error()
    assert _call(name, mk(), out=False)[0] == -1 and ("mean" if name == POST else "log_prior_out") in _lib.last_error()
    assert _call(name, api.make_opts("bi_reduced", 32, per_voxel=True))[0] < 0 and "per_voxel_p0_bounds" in _lib.last_error()
    rc, res = _call(name, mk(), n_classes=17)  # a refused call writes nothing
    assert rc == -1 and all((v == 9.0).all() for k, v in res.items() if k in ("mean", "log_prior", "loglik", "loglik_class"))
    if name == EM:
        assert _call(name, mk(), n_iter=0)[0] == -1 and "n_iter" in _lib.last_error()
    if _lib.device_count() == 0:  # valid calls stop at the device: rows that exclude different atoms are fine
        table = np.zeros((2, 4))
        table[0, :3] = -np.inf
        table[1, 1:] = -np.inf
        assert _call(name, mk(), log_prior=table)[0] == -3
        assert _call(name, mk(), n_classes=16)[0] == -3


def test_an_em_call_without_voxels_returns_the_normalised_start_rows():
    table = np.array([[np.log(3.0) + 5.0, -np.inf, 5.0, -np.inf], [0.0, 0.0, 0.0, 0.0]])
    rc, res = _call(EM, api.make_opts("bi_reduced", 32), n_vox=0, log_prior=table)
    assert rc == 0 and res["done"].value == 0 and res["n_eff"].tolist() == [0, 0]
    assert res["log_prior"].tobytes() == normalise_rows(table, 2, 4).tobytes()
    assert res["loglik"][0] == 0.0 and np.isnan(res["loglik"][1:]).all()
    assert (res["loglik_class"][0] == 0.0).all() and np.isnan(res["loglik_class"][1:]).all()


def _bi():
    lo, hi = np.array([0.0, 1e-5, 1e-5, 0.0]), np.array([1.0, 0.5, 0.5, 10.0])
    names = ["f1", "D1", "D2", "S0"]
    return names, lo, hi, {n: (float(a), float(b)) for n, a, b in zip(names, lo, hi)}


def test_api_checks_shapes_before_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "require_device", lambda: None)
    b, y = case_signals("bi_s0", 4, n_b=16)
    _, lo, hi, _ = _bi()
    nl = np.array([[0.05, 0.1], [0.001, 0.002]])
    lab = np.zeros(4, np.int32)
    for fn in (api.varpro_posterior_classes, api.varpro_prior_em_classes):
        with pytest.raises(ValueError, match="log_prior has shape"):
            fn("bi_s0", b, y, nl, lo, hi, lab, 2, log_prior=np.zeros(2))
        with pytest.raises(ValueError, match="n_classes=17"):
            fn("bi_s0", b, y, nl, lo, hi, lab, 17)
        with pytest.raises(ValueError, match="labels must be 4 integers"):
            fn("bi_s0", b, y, nl, lo, hi, lab[:3], 2)
        with pytest.raises(ValueError, match="labels must be 4 integers"):
            fn("bi_s0", b, y, nl, lo, hi, np.zeros(4), 2)
        with pytest.raises(ValueError, match="nl_atoms has 1 rows"):
            fn("bi_s0", b, y, nl[:1], lo, hi, lab, 2)


def test_no_cpu_fallback_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is visible here")
    b, y = case_signals("bi_s0", 4, n_b=16)
    _, lo, hi, _ = _bi()
    with pytest.raises(_lib.PnxError):
        api.varpro_posterior_classes("bi_s0", b, y, np.array([[0.05, 0.1], [0.001, 0.002]]), lo, hi, np.zeros(4, np.int32), 1)
    with pytest.raises(_lib.PnxError):
        _solver(empirical_prior={"per_label": True}).fit(b, y, labels=np.zeros(4, int))


# ---- the solver
RATES = {"D1": [0.05, 0.1], "D2": [0.001, 0.002]}  # ordered: 4 pairs


def _solver(**kw):
    return HipBayesVarProSolver(BiExpModel(fit_s0=True), rates=RATES, bounds=_bi()[3], **kw)


def test_solver_per_label_options():
    defaults = {"n_iter": 20, "pseudo_count": 0.0, "rel_tol": 1e-6, "max_voxels": None}
    G = _solver()._nl_atoms.shape[1]
    assert _solver(empirical_prior=True).empirical_prior == defaults and not _solver(empirical_prior=True).needs_labels
    assert _solver(empirical_prior={"per_label": False}).empirical_prior == defaults and not _solver().needs_labels
    given = {"per_label": True, "n_iter": 5}  # the TOML table [Fitting.solver.empirical_prior], the grid solver's
    s = _solver(empirical_prior=given)
    assert s.empirical_prior == {**defaults, "n_iter": 5, "per_label": True} and s.needs_labels and given == {"per_label": True, "n_iter": 5}
    grid = HipBayesGridSolver._empirical_prior_options(given)
    assert s.empirical_prior == grid  # the user-visible option is identical for both solvers
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="per_label must be a bool"):
            _solver(empirical_prior={"per_label": bad})
    with pytest.raises(ValueError, match=r"unknown keys \['per_labels'\]"):
        _solver(empirical_prior={"per_labels": True})
    with pytest.raises(ValueError, match="max_voxels is not built with per_label"):
        _solver(empirical_prior={"per_label": True, "max_voxels": 100})
    for kw in ({"empirical_prior": {"per_label": True}}, {"log_prior": np.zeros((2, G))}):
        with pytest.raises(ValueError, match="marginals are not built with per-label priors.*pnx_curvefit_varpro_marginals_f64"):
            _solver(marginals=True, **kw)
    with pytest.raises(ValueError, match="needs per_label"):
        _solver(log_prior=np.zeros((2, G)), empirical_prior=True)
    # a 2-D table: one row per class; (1, n_atoms) stays the single table
    assert _solver(log_prior=np.zeros((3, G))).needs_labels and _solver(log_prior=np.zeros((3, G))).log_prior.shape == (3, G)
    flat = _solver(log_prior=np.zeros((1, G)))
    assert flat.log_prior.shape == (G,) and not flat.needs_labels
    with pytest.raises(ValueError, match="17 rows: at most 16"):
        _solver(log_prior=np.zeros((17, G)))
    with pytest.raises(ValueError, match="in every row"):
        _solver(log_prior=np.concatenate([np.zeros((1, G)), np.full((1, G), -np.inf)]))
    with pytest.raises(ValueError, match=f"entries for {G} atoms"):
        _solver(log_prior=np.zeros(G + 1))
    doc = HipBayesVarProSolver.__doc__
    assert "per_label" in doc and "prior_labels" in doc


def test_label_to_row_mapping_is_the_grid_solvers():
    assert HipBayesVarProSolver.label_rows is HipBayesGridSolver.label_rows
    values, rows = HipBayesVarProSolver.label_rows(np.array([7, 3, -1, 7, 0, -5, 3]), 7)
    assert values.tolist() == [0, 3, 7] and rows.tolist() == [2, 1, -1, 2, 0, -1, 1] and rows.dtype == np.int32
    with pytest.raises(ValueError, match="17 distinct non-negative values: more than 16 classes"):
        HipBayesVarProSolver.label_rows(np.arange(17), 17)


def test_fit_asks_for_labels_and_the_fitter_hands_them_over(monkeypatch):
    b, y = case_signals("bi_s0", 8, n_b=16)
    G = _solver()._nl_atoms.shape[1]
    s = _solver(empirical_prior={"per_label": True})
    with pytest.raises(ValueError, match="labels .* is required"):
        s.fit(b, y)
    with pytest.raises(ValueError, match="distinct non-negative values"):
        s.fit(b, np.tile(y, (3, 1)), labels=np.arange(24))
    with pytest.raises(ValueError, match="2 rows for the 3 distinct labels"):
        _solver(log_prior=np.zeros((2, G)), empirical_prior={"per_label": True}).fit(b, y, labels=np.arange(8) % 3)
    seen = {}

    def fake_fit(xdata, ydata, pixel_fixed_params=None, labels=None, **kw):
        seen["labels"], seen["n"] = labels, ydata.shape[0]
        raise RuntimeError("stop here")

    monkeypatch.setattr(s, "fit", fake_fit)
    seg = np.array([0, 3, 7, 7, 3, 0, 3, 7]).reshape(2, 2, 2)
    with pytest.raises(RuntimeError, match="stop here"):
        HipPixelWiseFitter(s).fit(b, y.reshape(2, 2, 2, 16), segmentation=seg)
    assert seen["n"] == 6 and seen["labels"].tolist() == [3, 7, 7, 3, 3, 7]
    with pytest.raises(ValueError, match="pass a segmentation"):
        HipPixelWiseFitter(s).fit(b, y.reshape(2, 2, 2, 16))


# ---- the numpy reference, worked by hand
def test_reference_updates_each_row_from_its_own_voxels():
    """4.1n's example on a varpro l0: P[v, g] = [[4,1,1],[4,1,1],[1,4,1],[1,1,1]], labels (0, 0, 1, 1), uniform start.  Class 0:
    W = (4,1,1)/6 twice, pi = (4,1,1)/6.  Class 1: W = (1,4,1)/6 and (1,1,1)/3, S = (1/2, 1, 1/2), pi = (1/4, 1/2, 1/4).  Class 2
    has no voxel and keeps its row."""
    P = np.array([[4.0, 1, 1], [4, 1, 1], [1, 4, 1], [1, 1, 1]])
    l0, fin, lab = np.log(P), np.ones(4, bool), np.array([0, 0, 1, 1])
    lp0 = normalise_rows(None, 3, 3)
    S, lp1, ll, n = em_step_classes(l0, lp0, fin, lab)
    np.testing.assert_allclose(np.exp(lp1[0]), [4 / 6, 1 / 6, 1 / 6], rtol=1e-14)
    np.testing.assert_allclose(np.exp(lp1[1]), [0.25, 0.5, 0.25], rtol=1e-14)
    np.testing.assert_allclose(S[1], [0.5, 1.0, 0.5], rtol=1e-14)
    assert lp1[2].tobytes() == lp0[2].tobytes() and n.tolist() == [2, 2, 0] and ll[2] == 0.0
    assert ll[0] == pytest.approx(2 * np.log(2.0), rel=1e-14) and ll[1] == pytest.approx(np.log(2.0), rel=1e-14)
    assert ll.sum() == pytest.approx(em_step(l0, lp0[0], fin)[2], rel=1e-14)  # under equal rows the classes' sum is the volume's
    lab[3] = -1  # background takes no part
    S, lp1, ll, n = em_step_classes(l0, lp0, fin, lab)
    np.testing.assert_allclose(np.exp(lp1[1]), [1 / 6, 4 / 6, 1 / 6], rtol=1e-14)
    assert n.tolist() == [2, 1, 0]


def test_labelled_posterior_reference_is_the_unlabelled_reference_row_by_row():
    from varpro_marginal_cases import _case, ref_kw
    from varpro_posterior_reference import reference

    c = _case("bi_s0", 9, n_b=32)
    G = c["atoms"].shape[1]
    rows = np.log(np.random.default_rng(1).uniform(0.1, 1.0, (2, G)))
    lab = np.array([0, 1, 0, 1, -1, 2, 1, 0, 0])
    ref = posterior(c["model"], c["b"], c["y"], c["atoms"], c["lo"], c["hi"], lab, 2, log_prior=rows, **ref_kw(c))
    assert ref["finite"].tolist() == [True, True, True, True, False, False, True, True, True] and np.isnan(ref["mean"][4]).all()
    for k in range(2):
        one = reference(c["model"], c["b"], c["y"][lab == k], c["atoms"], c["lo"], c["hi"], log_prior=rows[k], **ref_kw(c))
        assert ref["mean"][lab == k].tobytes() == one["mean"].tobytes() and ref["bound_mean"][lab == k].tobytes() == one["bound_mean"].tobytes()


# ---- the CPU precondition of tests/test_gpu_varpro_class_axes.py: the references alone on every one of its cases
_AXES = {}


def _axes_cases():
    from varpro_class_axes_cases import cases

    if not _AXES:
        _AXES.update(cases())
    return _AXES


@pytest.mark.parametrize("family,count", [("layout-bi", 6), ("layout-mono", 2), ("layout-tri", 6), ("n_b-", 9), ("min-slab-", 2)])
def test_the_references_hold_their_precondition_on_every_case_of_the_axes_file(family, count):
    """eps_v <= the case's cap on EVERY voxel (asserted inside the references: 1e-6, or the 1e-3 of 16 b-values or fewer), for the
    labelled posterior under the GPU file's rows and for the EM's l0; no case clips but the two-compartment S0 / reduced layouts at
    16 b-values, whose neighbouring rates leave a share of 1e-5 at most on a clipped amplitude."""
    from varpro_marginal_cases import ref_kw
    from varpro_prior_reference import likelihoods

    assert len(_axes_cases()) == 7 * 2 + 9 + 2
    mine = {k: v for k, v in _axes_cases().items() if k.startswith(family)}
    assert len(mine) == count
    for name, per_mode in mine.items():
        for c in per_mode:
            n_classes, n_vox, G = c.get("n_classes", 3), c["y"].shape[0], c["atoms"].shape[1]
            assert n_vox == 65
            lab = np.arange(n_vox) % n_classes
            rows = np.log(np.random.default_rng(5).uniform(0.01, 1.0, (n_classes, G))) + 2.5  # the GPU file's _rows
            args = (c["model"], c["b"], c["y"], c["atoms"], c["lo"], c["hi"])
            ref = posterior(*args, lab, n_classes, log_prior=rows, **ref_kw(c))
            l0, eps0, fin = likelihoods(*args, **ref_kw(c))
            assert ref["finite"].all() and fin.all() and ref["eps"].max() <= c["max_eps"] and eps0.max() <= c["max_eps"], name
            assert c["max_eps"] == (1e-3 if len(c["b"]) <= 16 else 1e-6), name
            assert ref["clipped_mass"].max() <= (1e-5 if len(c["b"]) <= 16 else 0.0), name


# ---- the CPU precondition of the GPU file's worth test
@pytest.mark.parametrize("noise_sd,single,per_label", [(0.05, 0.10254, 0.08495), (0.0, 0.16883, 0.13024)])
def test_the_reference_shows_the_gain_the_gpu_test_asks_the_library_for(noise_sd, single, per_label):
    """Two narrow bi_s0 populations with the same fractions whose rates differ by factors 1.6 and 1.5, 1000 + 1000 voxels, 5 % noise,
    three updates: numpy's median |error| of f1 under the single learned table and under the per-label tables.  The GPU test asserts
    per_label < single on the library only because the reference shows at least a 10 % gain here."""
    w = worth(noise_sd, 3)
    print("median |error| of (f1, D1, D2): single", w["medians"][0], "per label", w["medians"][1])
    assert w["single"] == pytest.approx(single, rel=2e-4) and w["per_label"] == pytest.approx(per_label, rel=2e-4)
    assert w["per_label"] <= 0.9 * w["single"]

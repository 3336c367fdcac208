"""One prior row per segmentation label (pnx_curvefit_grid_posterior_classes_f64, pnx_curvefit_grid_prior_em_classes_f64,
api.grid_posterior_classes / grid_prior_em_classes, HipBayesGridSolver's per_label), the parts that need no GPU: the host-side
checks, starts, centres, report and slab sizing under AddressSanitizer / UBSan (a stand-alone program,
tests/host_stub/grid_class_args_stub.cpp), the ABI's refusals in front of any device work, the solver's option parsing, the label ->
row mapping and its ValueErrors, the fitter's hand-over of segmentation[mask], and the numpy reference on a case worked by hand."""
from __future__ import annotations

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from conftest import ROOT
from grid_class_prior_reference import em_step_classes, normalise_rows
from grid_prior_reference import em_step

from pyneapple_amd import _lib, api, synth
from pyneapple_amd.fitters import HipPixelWiseFitter
from pyneapple_amd.models import TriExpModel
from pyneapple_amd.solvers import HipBayesGridSolver

POST, EM = "pnx_curvefit_grid_posterior_classes_f64", "pnx_curvefit_grid_prior_em_classes_f64"


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("stub") / "grid_class_args_stub")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "pyneapple_amd", "csrc"), os.path.join(ROOT, "tests", "host_stub", "grid_class_args_stub.cpp"), "-o", exe]
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
    calls' refusals behind them, the starts and the report, and the slab inside 64 KB for every n_classes x n_b."""
    assert "grid class args stub ok" in _run_stub(stub)


@pytest.mark.parametrize("n_b", [1, 32, 33, 128])
def test_slab_stays_inside_the_lds_budget_and_python_agrees(stub, n_b):
    kpad = (n_b + 3) & ~3
    for n_classes in range(1, 17):
        for extra in (4 * n_classes, 3, 8):  # both EM passes; the posterior at 3 and 8 free parameters
            w = api.grid_class_slab_atoms(n_b, n_classes, extra)
            assert int(_run_stub(stub, n_b, n_classes, extra)) == w
            assert w >= 16 and w % 16 == 0 and (kpad * (w if w & 16 else w + 16) + (2 + n_classes + extra) * w) * 8 <= 64 * 1024
    assert api.grid_class_slab_atoms(n_b, 1, 4) == api.grid_prior_slab_atoms(n_b)
    assert api.grid_class_slab_atoms(n_b, 1, 3) == api.grid_posterior_slab_atoms(n_b, 3)


def _slab_image(kpad_rows, per_atom, w):
    """(stride, doubles) of the LDS image of a slab `w` atoms wide: kpad_rows dictionary rows of `stride` doubles and per_atom values
    per atom -- the layout grid_class_slab / varpro_class_slab of the csrc headers size."""
    stride = w if w & 16 else w + 16
    return stride, kpad_rows * stride + per_atom * w


def test_slab_rule_for_every_b_value_and_class_count():
    """Every (n_b in 1..128, n_classes in 1..16), grid_class_slab and varpro_class_slab (k = 1..3), for the posterior and for both EM
    passes: the width is a multiple of 16 and at least 16, the stride is 16 mod 32, the image fits 64 KB, and no wider slab would.
    Through api.grid_class_slab_atoms / api.varpro_class_slab_atoms: the stub prints one width per process (its own run sweeps the
    same product inside the C++), so the Python restatement is swept here and compared with the stub at the minimum-width corner
    below and at four b-values above."""
    for n_b in range(1, 129):
        kpad = (n_b + 3) & ~3
        for n_classes in range(1, 17):
            for extra in (4 * n_classes, 1, 8):  # both EM passes; the posterior at 1 and 8 free parameters
                w = api.grid_class_slab_atoms(n_b, n_classes, extra)
                stride, doubles = _slab_image(kpad, 2 + n_classes + extra, w)
                assert w >= 16 and w % 16 == 0 and w <= 256 and stride % 32 == 16 and stride >= w and doubles * 8 <= 64 * 1024
                assert w == 256 or _slab_image(kpad, 2 + n_classes + extra, w + 16)[1] * 8 > 64 * 1024  # the widest that fits
            for k in (1, 2, 3):
                for extra in (4 * n_classes, k + 1):  # both EM passes; the posterior
                    w = api.varpro_class_slab_atoms(n_b, k, n_classes, extra)
                    stride, doubles = _slab_image(k * kpad, k * (k + 1) + n_classes + extra, w)
                    assert w >= 16 and w % 16 == 0 and w <= 256 and stride % 32 == 16 and stride >= w and doubles * 8 <= 64 * 1024
                    assert w == 256 or _slab_image(k * kpad, k * (k + 1) + n_classes + extra, w + 16)[1] * 8 > 64 * 1024


def test_minimum_slab_width_corner(stub):
    """128 b-values and 16 classes leave the EM 16 atoms; 12 classes are the last to leave it 32.  Python and the C++ agree."""
    assert api.grid_class_slab_atoms(128, 16, 64) == 16 == int(_run_stub(stub, 128, 16, 64))
    assert api.grid_class_slab_atoms(128, 12, 48) == 32 == int(_run_stub(stub, 128, 12, 48))
    assert api.grid_class_slab_atoms(128, 13, 52) == 16 == int(_run_stub(stub, 128, 13, 52))
    assert _slab_image(128, 2 + 16 + 64, 16) == (16, 3360)


# ---- the ABI without a device
def _call(name, o, n_vox=1, n_atoms=4, n_classes=2, labels=True, log_prior=None, noise_sd=0.0, n_iter=3, out=True):
    n = o.n_free
    atoms = np.full((n, max(n_atoms, 1)), 0.5)
    lo, hi = np.zeros(n), np.ones(n)
    b, y = np.zeros(128), np.ones(128)
    lab = np.zeros(max(n_vox, 1), np.int32)
    rows = max(min(n_classes, 16), 1)
    lp = None if log_prior is None else np.ascontiguousarray(log_prior, float)
    head = (C.byref(o), n_vox, _lib.ptr(b), _lib.ptr(y), n_atoms, _lib.ptr(atoms), None, _lib.ptr(lo), _lib.ptr(hi), 0, n_classes,
            _lib.ptr(lab) if labels else None, _lib.ptr(lp), noise_sd)
    if name == POST:
        res = dict(mean=np.full((n, max(n_vox, 1)), 9.0))
        rc = _lib.load().pnx_curvefit_grid_posterior_classes_f64(*head, _lib.ptr(res["mean"]) if out else None, None, None, None, None, None, 0, 0, None)
    else:
        res = dict(log_prior=np.full((rows, max(n_atoms, 1)), 9.0), loglik=np.full(n_iter + 1, 9.0), loglik_class=np.full((n_iter + 1, rows), 9.0),
                   done=C.c_int(-7), n_eff=np.full(rows, -7, np.int64))
        rc = _lib.load().pnx_curvefit_grid_prior_em_classes_f64(*head, n_iter, 0.0, 0.0, _lib.ptr(res["log_prior"]) if out else None,
                                                                _lib.ptr(res["loglik"]), _lib.ptr(res["loglik_class"]), C.byref(res["done"]),
                                                                _lib.ptr(res["n_eff"]), 0, 0, None)
    return rc, res


def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnx.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    for name, n_args in ((POST, 23), (EM, 25)):
        assert re.search(r"PNX_API\s+int\s+" + name + r"\s*\(", text) and name in _lib.ABI_SYMBOLS and name in exported
        fn = getattr(_lib.load(), name)
        assert len(fn.argtypes) == n_args and fn.restype is C.c_int
    for name in ("grid_posterior_classes", "grid_posterior_classes_device", "grid_prior_em_classes", "grid_prior_em_classes_device"):
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
    assert _call(name, mk(), noise_sd=-1.0)[0] == -1 and "noise_sd" in _lib.last_error()
    assert _call(name, mk(), n_atoms=0)[0] == -1 and "n_atoms" in _lib.last_error()
    assert _call(name, mk(), out=False)[0] == -1 and ("mean" if name == POST else "log_prior_out") in _lib.last_error()
    assert _call(name, api.make_opts("bi_reduced", 32, per_voxel=True))[0] == -2 and "per_voxel_p0_bounds" in _lib.last_error()
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


def test_api_checks_shapes_before_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "require_device", lambda: None)
    b, y, _ = synth.make_numpy("tri_reduced", 4, 32)
    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    lab = np.zeros(4, np.int32)
    for fn in (api.grid_posterior_classes, api.grid_prior_em_classes):
        with pytest.raises(ValueError, match="log_prior has shape"):
            fn("tri_reduced", b, y, p0[:, None], lo, hi, lab, 2, log_prior=np.zeros(1))
        with pytest.raises(ValueError, match="n_classes=17"):
            fn("tri_reduced", b, y, p0[:, None], lo, hi, lab, 17)
        with pytest.raises(ValueError, match="labels must be 4 integers"):
            fn("tri_reduced", b, y, p0[:, None], lo, hi, lab[:3], 2)
        with pytest.raises(ValueError, match="labels must be 4 integers"):
            fn("tri_reduced", b, y, p0[:, None], lo, hi, np.zeros(4), 2)


def test_no_cpu_fallback_without_device():
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is visible here")
    b, y, _ = synth.make_numpy("tri_reduced", 4, 32)
    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    with pytest.raises(_lib.PnxError):
        api.grid_posterior_classes("tri_reduced", b, y, p0[:, None], lo, hi, np.zeros(4, np.int32), 1)
    with pytest.raises(_lib.PnxError):
        _solver(grid={"f1": [0.1, 0.2]}, empirical_prior={"per_label": True}).fit(b, y, labels=np.zeros(4, int))


# ---- the solver
def _tri():
    names, p0, lo, hi = synth.shared_arrays("tri_reduced")
    return dict(p0=dict(zip(names, map(float, p0))), bounds={n: (float(a), float(b)) for n, a, b in zip(names, lo, hi)})


def _solver(**kw):
    return HipBayesGridSolver(TriExpModel(), **{**_tri(), **kw})


def test_solver_per_label_options():
    defaults = {"n_iter": 20, "pseudo_count": 0.0, "rel_tol": 1e-6, "max_voxels": None}
    g = {"f1": [0.1, 0.2]}
    assert _solver(grid=g, empirical_prior=True).empirical_prior == defaults and not _solver(grid=g, empirical_prior=True).needs_labels
    assert _solver(grid=g, empirical_prior={"per_label": False}).empirical_prior == defaults
    s = _solver(grid=g, empirical_prior={"per_label": True, "n_iter": 5})  # the TOML table [Fitting.solver.empirical_prior]
    assert s.empirical_prior == {**defaults, "n_iter": 5, "per_label": True} and s.needs_labels
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="per_label must be a bool"):
            _solver(grid=g, empirical_prior={"per_label": bad})
    with pytest.raises(ValueError, match=r"unknown keys \['per_labels'\]"):
        _solver(grid=g, empirical_prior={"per_labels": True})
    with pytest.raises(ValueError, match="max_voxels is not built with per_label"):
        _solver(grid=g, empirical_prior={"per_label": True, "max_voxels": 100})
    for kw in ({"empirical_prior": {"per_label": True}}, {"log_prior": np.zeros((2, 2))}):
        with pytest.raises(ValueError, match="marginals are not built with per-label priors"):
            _solver(grid=g, marginals=True, **kw)
    # a 2-D table: one row per class; (1, n_atoms) stays the single table
    assert _solver(grid=g, log_prior=np.zeros((3, 2))).needs_labels and _solver(grid=g, log_prior=np.zeros((3, 2))).log_prior.shape == (3, 2)
    flat = _solver(grid=g, log_prior=np.zeros((1, 2)))
    assert flat.log_prior.shape == (2,) and not flat.needs_labels
    with pytest.raises(ValueError, match="17 rows: at most 16"):
        _solver(grid=g, log_prior=np.zeros((17, 2)))
    with pytest.raises(ValueError, match="in every row"):
        _solver(grid=g, log_prior=np.array([[0.0, 0.0], [-np.inf, -np.inf]]))
    with pytest.raises(ValueError, match="needs per_label"):
        _solver(grid=g, log_prior=np.zeros((2, 2)), empirical_prior=True)
    doc = HipBayesGridSolver.__doc__
    assert "per_label" in doc and "prior_labels" in doc and "neighbourhood (MRF)" in doc


def test_label_to_row_mapping():
    values, rows = HipBayesGridSolver.label_rows(np.array([7, 3, -1, 7, 0, -5, 3]), 7)
    assert values.tolist() == [0, 3, 7] and rows.tolist() == [2, 1, -1, 2, 0, -1, 1] and rows.dtype == np.int32
    values, rows = HipBayesGridSolver.label_rows(np.array([3.0, 7.0]), 2)  # a segmentation stored as floats
    assert values.tolist() == [3, 7] and rows.tolist() == [0, 1]
    assert HipBayesGridSolver.label_rows(np.arange(16), 16)[0].size == 16
    with pytest.raises(ValueError, match="17 distinct non-negative values: more than 16 classes"):
        HipBayesGridSolver.label_rows(np.arange(17), 17)
    for bad in (np.zeros(3, int), np.array([0.5, 1.0, 2.0, 3.0]), np.zeros((2, 2), int)):
        with pytest.raises(ValueError, match="labels must be 4 integers"):
            HipBayesGridSolver.label_rows(bad, 4)


def test_fit_asks_for_labels_and_the_fitter_hands_them_over(monkeypatch):
    b, y, _ = synth.make_numpy("tri_reduced", 8, 32)
    s = _solver(grid={"f1": [0.1, 0.2]}, empirical_prior={"per_label": True})
    with pytest.raises(ValueError, match="labels .* is required"):
        s.fit(b, y)
    with pytest.raises(ValueError, match="distinct non-negative values"):
        s.fit(b, np.tile(y, (3, 1)), labels=np.arange(24))
    with pytest.raises(ValueError, match="2 rows for the 3 distinct labels"):
        _solver(grid={"f1": [0.1, 0.2]}, log_prior=np.zeros((2, 2)), empirical_prior={"per_label": True}).fit(b, y, labels=np.arange(8) % 3)
    seen = {}

    def fake_fit(xdata, ydata, pixel_fixed_params=None, labels=None, **kw):
        seen["labels"], seen["n"] = labels, ydata.shape[0]
        raise RuntimeError("stop here")

    monkeypatch.setattr(s, "fit", fake_fit)
    seg = np.array([0, 3, 7, 7, 3, 0, 3, 7]).reshape(2, 2, 2)
    with pytest.raises(RuntimeError, match="stop here"):
        HipPixelWiseFitter(s).fit(b, y.reshape(2, 2, 2, 32), segmentation=seg)
    assert seen["n"] == 6 and seen["labels"].tolist() == [3, 7, 7, 3, 3, 7]
    with pytest.raises(ValueError, match="pass a segmentation"):
        HipPixelWiseFitter(s).fit(b, y.reshape(2, 2, 2, 32))
    plain = _solver(grid={"f1": [0.1, 0.2]})
    monkeypatch.setattr(plain, "fit", lambda xdata, ydata, pixel_fixed_params=None, **kw: seen.update(kw=kw) or (_ for _ in ()).throw(RuntimeError("plain")))
    with pytest.raises(RuntimeError, match="plain"):
        HipPixelWiseFitter(plain).fit(b, y.reshape(2, 2, 2, 32), segmentation=seg)
    assert seen["kw"] == {}  # every other solver's call is untouched


# ---- the numpy reference, worked by hand
def test_reference_updates_each_row_from_its_own_voxels():
    """P[v, g] = [[4,1,1],[4,1,1],[1,4,1],[1,1,1]], labels (0, 0, 1, 1), uniform start.  Class 0: W = (4,1,1)/6 twice, pi = (4,1,1)/6.
    Class 1: W = (1,4,1)/6 and (1,1,1)/3, S = (1/2, 1, 1/2), pi = (1/4, 1/2, 1/4).  Class 2 has no voxel and keeps its row."""
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


def test_per_label_is_the_grid_solvers_option_only():
    from pyneapple_amd.solvers import HipBayesVarProSolver

    assert HipBayesVarProSolver._empirical_prior_options(True) == {"n_iter": 20, "pseudo_count": 0.0, "rel_tol": 1e-6, "max_voxels": None}
    with pytest.raises(ValueError, match=r"unknown keys \['per_label'\]"):
        HipBayesVarProSolver._empirical_prior_options({"per_label": True})

"""IDEAL with the solver's constraint and sigma, the parts that need no GPU: the ABI symbol of the simplex projection, its
refusals in front of any device work, the numpy restatement of the projection against hand-worked cases, and the host-path
driver handing projected start values to a constrained solver only."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import ROOT

import ideal_reference as R
from pyneapple_amd import _lib
from pyneapple_amd.ideal import HipIDEALFitter, project_fractions

NAME = "pnx_ideal_bounds_simplex_f64"


def test_symbol_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pnx.h")).read(), flags=re.S)
    assert re.search(r"PNX_API\s+int\s+" + NAME + r"\s*\(", text)
    assert NAME in _lib.ABI_SYMBOLS
    fn = getattr(_lib.load(), NAME)
    plain = _lib.load().pnx_ideal_bounds_f64
    # the arguments of pnx_ideal_bounds_f64 with i_f1 and i_f2 behind tol
    assert list(fn.argtypes) == list(plain.argtypes[:6]) + [C.c_int, C.c_int] + list(plain.argtypes[6:])
    assert fn.restype is C.c_int


def _call(n_params, i_f1, i_f2, n_px=4):
    a = np.zeros(64)
    p = _lib.ptr(a)
    return _lib.load().pnx_ideal_bounds_simplex_f64(p, n_px, n_params, p, p, p, i_f1, i_f2, p, p, p, 0, None)


def test_abi_refusals_need_no_device():
    for n_params, i1, i2, word in ((5, 2, 2, "i_f1 == i_f2"), (5, -1, 2, "i_f1"), (5, 5, 2, "i_f1"), (5, 0, 5, "i_f2"), (5, 0, -3, "i_f2"),
                                   (9, 0, 2, "n_params"), (0, 0, 2, "n_params")):
        assert _call(n_params, i1, i2) == -1, (n_params, i1, i2)
        assert word in _lib.last_error(), (word, _lib.last_error())
    assert _call(5, 0, 2, n_px=-1) == -1 and "n_px" in _lib.last_error()
    a = np.zeros(8)
    assert _lib.load().pnx_ideal_bounds_simplex_f64(None, 4, 5, _lib.ptr(a), _lib.ptr(a), _lib.ptr(a), 0, 2, _lib.ptr(a), _lib.ptr(a),
                                                    _lib.ptr(a), 0, None) == -1 and "NULL" in _lib.last_error()
    assert _call(5, 0, 2, n_px=0) == 0  # nothing to do is not an error, and needs no device either


# [f1, D1, f2, D2, D3]: every number below is a dyadic fraction, so the expected values are exact
LO = np.array([0.0, 0.0, 0.0, 0.0, 0.0])
HI = np.array([1.0, 8.0, 1.0, 8.0, 8.0])
TOL = np.array([0.5, 0.25, 0.5, 0.25, 0.25])


def test_projection_against_hand_worked_cases():
    rows = np.array([
        [0.25, 1.0, 0.5, 2.0, 4.0],      # sum 0.75: untouched
        [0.25, 1.0, 0.75, 2.0, 4.0],     # sum exactly 1: e = 0 is not > 0, untouched
        [0.5, 1.0, 0.5625, 2.0, 4.0],    # sum 1.0625, both interior: 0.03125 off each
        [-0.5, 9.0, 0.5, 2.0, 4.0],      # step 1 alone: f1 -> 0, D1 -> 8
    ])
    p, over = R.project(rows, LO, HI, 0, 2)
    assert over.tolist() == [False, False, True, False]
    assert p.tolist() == [[0.25, 1.0, 0.5, 2.0, 4.0], [0.25, 1.0, 0.75, 2.0, 4.0], [0.46875, 1.0, 0.53125, 2.0, 4.0], [0.0, 8.0, 0.5, 2.0, 4.0]]
    p0, lower, upper = R.ideal_bounds_simplex(rows, LO, HI, TOL, 0, 2)
    assert p0.shape == (5, 4) and np.array_equal(p0, p.T)
    assert lower[:, 2].tolist() == [0.234375, 0.75, 0.265625, 1.5, 3.0]
    assert upper[:, 2].tolist() == [0.703125, 1.25, 0.796875, 2.5, 5.0]
    assert upper[:, 3].tolist() == [0.0, 8.0, 0.75, 2.5, 5.0]  # the window of a start on a bound is clipped to the bound
    # the sum 1.06 of decimal fractions: 0.03 off each, to the rounding of the three operations
    p, over = R.project(np.array([[0.5, 1.0, 0.56, 2.0, 4.0]]), LO, HI, 0, 2)
    assert over[0] and p[0, 0] == pytest.approx(0.47, abs=1e-15) and p[0, 2] == pytest.approx(0.53, abs=1e-15)
    assert p[0, 0] + p[0, 2] <= 1.0 + 2.0 ** -52
    # rows the projection does not touch are the plain kernel's statement bit for bit
    a, b = R.ideal_bounds_simplex(rows, LO, HI, TOL, 0, 2), R.ideal_bounds(rows, LO, HI, TOL)
    for x, y in zip(a, b):
        assert x[:, [0, 1, 3]].tobytes() == y[:, [0, 1, 3]].tobytes() and x[:, 2].tobytes() != y[:, 2].tobytes()


def test_projection_second_clip():
    """f1 is interpolated above its upper bound: step 1 puts it on the bound (0.75), e = 0.75 + 0.875 - 1 = 0.625, and
    0.75 - 0.3125 = 0.4375 lies below f1's lower bound 0.5, so step 3 clips it back to 0.5; f2 = 0.875 - 0.3125 = 0.5625.  The
    bounds leave the sum at 1.0625: the projection promises the nearest point of the box, not feasibility."""
    lo, hi = LO.copy(), HI.copy()
    lo[0], hi[0] = 0.5, 0.75
    p, over = R.project(np.array([[0.9375, 1.0, 0.875, 2.0, 4.0]]), lo, hi, 0, 2)
    assert over[0] and p[0].tolist() == [0.5, 1.0, 0.5625, 2.0, 4.0]
    p0, lower, upper = R.ideal_bounds_simplex(np.array([[0.9375, 1.0, 0.875, 2.0, 4.0]]), lo, hi, TOL, 0, 2)
    assert (p0[0, 0], lower[0, 0], upper[0, 0]) == (0.5, 0.5, 0.75) and (lower[2, 0], upper[2, 0]) == (0.28125, 0.84375)
    # the fraction rows may come in either order and sit anywhere
    q, _ = R.project(np.array([[1.0, 0.875, 2.0, 0.9375, 4.0]]), lo[[1, 2, 3, 0, 4]], hi[[1, 2, 3, 0, 4]], 3, 1)
    assert q[0].tolist() == [1.0, 0.5625, 2.0, 0.5, 4.0]


def test_drivers_numpy_projection_is_the_restatement():
    rng = np.random.default_rng(5)
    pmap = np.column_stack([rng.uniform(-0.1, 0.9, 300), rng.uniform(0, 9, 300), rng.uniform(0.2, 1.1, 300), rng.uniform(0, 9, 300),
                            rng.uniform(0, 9, 300)])
    lo, hi = LO + [0.05, 0, 0.1, 0, 0], HI - [0.2, 0, 0, 0, 0]
    want, over = R.project(pmap, lo, hi, 0, 2)
    assert 30 < over.sum() < 270
    got = project_fractions(np.clip(pmap, lo, hi).reshape(10, 15, 2, 5), lo, hi, 0, 2)
    assert got.shape == (10, 15, 2, 5) and got.reshape(-1, 5).tobytes() == want.tobytes()


class _Recorder:
    """A solver that records what each level hands it (tests/test_ideal.py's _FakeSolver, on the tri-exponential layout) and
    answers with fractions that sum to 1.05 everywhere -- the next level's interpolated start values are infeasible."""

    def __init__(self, constrained):
        from pyneapple_amd.models import TriExpModel

        self.model = TriExpModel()
        self.p0 = {"f1": 0.2, "D1": 0.05, "f2": 0.3, "D2": 0.005, "D3": 0.001}
        self.bounds = {"f1": (0.0, 1.0), "D1": (0.01, 0.5), "f2": (0.0, 1.0), "D2": (2e-3, 0.01), "D3": (1e-5, 2e-3)}
        if constrained:
            self.fraction_constraint, self._fraction_indices = True, [0, 2]
        self.calls, self.params_ = [], {}

    def fit(self, xdata, ydata, p0=None, bounds=None, **kw):
        self.calls.append((p0.copy(), bounds[0].copy(), bounds[1].copy()))
        n = ydata.shape[0]
        self.params_ = {"f1": np.full(n, 0.45), "D1": np.full(n, 0.05), "f2": np.full(n, 0.6), "D2": np.full(n, 0.005), "D3": np.full(n, 0.001)}
        return self


def test_host_path_projects_for_a_constrained_solver_only():
    b = np.linspace(0, 1000, 8)
    image = np.ones((8, 8, 1, 8))
    tol = {"f1": 0.01, "D1": 0.5, "f2": 0.01, "D2": 0.5, "D3": 0.5}
    starts = {}
    for constrained in (False, True):
        s = _Recorder(constrained)
        HipIDEALFitter(s, np.array([[4, 4], [8, 8]]), tol, device_resident=False).fit(b, image)
        assert len(s.calls) == 2 and s.calls[1][0].shape == (5, 64)
        starts[constrained] = s.calls[1]
    p0, lo, hi = starts[False]   # untouched: the interpolated 0.45 + 0.6, and a window that holds no feasible point
    assert np.allclose(p0[0], 0.45) and np.allclose(p0[2], 0.6) and (lo[0] + lo[2] > 1.0).all()
    p0, lo, hi = starts[True]    # 0.025 off each: on the face, the window around it reaches inside
    assert np.allclose(p0[0], 0.425) and np.allclose(p0[2], 0.575) and (lo[0] + lo[2] < 1.0).all() and (hi[0] + hi[2] > 1.0).all()
    np.testing.assert_array_equal(lo[0], np.clip(p0[0] * (1 - 0.01), 0.0, 1.0))
    for k in (1, 3, 4):  # the other rows do not know about the constraint
        for a, c in zip(starts[False], starts[True]):
            np.testing.assert_array_equal(a[k], c[k])

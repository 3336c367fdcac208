"""The method of the constrained curve fit -- two box-bounded TRF fits and a certificate -- restated with SciPy and run on the
g13 fixtures (tools/gen_constrained_golden.py): it solves the constrained problem at least as well as the reference's SLSQP
solver.  No GPU: this pins the method; tests/test_gpu_constrained.py pins the kernels against it."""
from __future__ import annotations

import numpy as np
import pytest
from conftest import load_golden

import constrained_reference as R

_CACHE = {}


def _solved(name):
    if name not in _CACHE:
        d = load_golden(name)
        model = str(d["model"])
        popt, lam, face = R.scipy_method(model, d["b"], d["y"], d["p0"], d["lo"], d["hi"], float(d["tol"]), int(d["max_iter"]))
        _CACHE[name] = (d, model, popt, lam, face)
    return _CACHE[name]


@pytest.mark.parametrize("name", ["g13_tri_constrained_reduced", "g13_tri_constrained_s0"])
def test_method_is_feasible_certified_and_no_worse_than_the_reference(name):
    d, model, popt, lam, face = _solved(name)
    b, y = d["b"], d["y"]
    cost = R.tri_cost(model, b, y, popt)
    ref = d["ref_popt"].T
    cost_ref = R.tri_cost(model, b, y, ref)
    ref_feasible = ref[:, 0] + ref[:, 2] <= 1.0 + 1e-12
    rel = cost / cost_ref - 1.0
    print(f"\n{name}: {int((face > 0).sum())} violators of {len(y)}, {int((lam < 0).sum())} negative multipliers, "
          f"largest relative cost difference {rel.max():+.3e}, reference more than 10 % worse on {int((rel < -1 / 11).sum())}, "
          f"reference successes {int(d['ref_success'].sum())}, reference feasible {int(ref_feasible.sum())}")
    assert (popt[:, 0] + popt[:, 2] <= 1.0).all()
    assert (popt >= d["lo"]).all() and (popt <= d["hi"]).all()
    assert (face > 0).sum() >= 10  # the fixture is about the face
    assert (lam[face > 0] >= 0).all() and (face != 2).all()
    on_face = face > 0
    assert (popt[on_face, 2] == 1.0 - popt[on_face, 0]).all()
    assert (cost <= cost_ref * (1 + 1e-6)).all(), np.flatnonzero(cost > cost_ref * (1 + 1e-6))

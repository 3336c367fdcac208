#!/usr/bin/env python3
"""What float32 arithmetic can deliver on the reference fixtures: the yardstick of the fp32 curve-fit path.

    python tools/f32_yardstick.py            # writes tests/golden/f32_yardstick.json

Needs numpy and SciPy only (no GPU, no library build).  For every unweighted fixture with all parameters free the reference
algorithm -- scipy.optimize.least_squares(method="trf", bounds, ftol=tol, xtol=gtol=1e-8, max_nfev) -- is run on a float32
MODEL: forward model and analytic Jacobian are evaluated in np.float32 and handed back to SciPy as float64, so SciPy's own
linear algebra stays fp64.  Its results are compared with the fixture's reference popt:

  cost_excess    the largest (c(p_y) - c(p_ref)) / (c(p_ref) + floor) over the voxels the yardstick fitted successfully,
                 c = float64 cost, floor = 0.5 n_b (FLT_EPSILON max|y|)^2 = the cost of float32 rounding of the model itself
                 (noise-free voxels end at 1e-26 in fp64 and cannot be compared otherwise);
  param_share    the share of voxels whose parameters are all within rtol 1e-3 of the reference;
  success_share  the share whose success flag equals the fixture's.

A fixture whose yardstick itself leaves more than 10 % of the voxels outside 1e-3 is dropped from the parameter criterion
("param_criterion": false): float32 cannot pin those parameters, whoever computes.

tests/test_gpu_curvefit_f32.py holds the kernel (pnx_curvefit_fast_f32) to these numbers; forward64 / cost64 / cost_floor
below are that test's evaluation code too.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FLT_EPSILON = float(np.finfo(np.float32).eps)

# fixture -> model key (parameter orders: include/pnx.h)
FIXTURES = {
    "g1_mono_b16": "mono", "g1_mono_b8": "mono",
    "g2_bi_reduced": "bi_reduced", "g2_bi_s0": "bi_s0", "g2_bi_full": "bi_full",
    "g3_tri_reduced": "tri_reduced", "g3_tri_s0": "tri_s0", "g3_tri_full": "tri_full",
    "g5_bi_pervoxel": "bi_reduced", "g5_tri_pervoxel": "tri_reduced",
}
N_PARAMS = {"mono": 2, "bi_reduced": 3, "bi_s0": 4, "bi_full": 4, "tri_reduced": 5, "tri_s0": 6, "tri_full": 6}


def _terms(model, P):
    """[(weight, D, scale)] of sum_c scale * weight_c * exp(-b D_c); P (..., n) -> arrays (...)."""
    one = np.ones_like(P[..., 0])
    if model == "mono":
        return [(P[..., 0], P[..., 1])], one
    if model == "bi_reduced":
        return [(P[..., 0], P[..., 1]), (1 - P[..., 0], P[..., 2])], one
    if model == "bi_s0":
        return [(P[..., 0], P[..., 1]), (1 - P[..., 0], P[..., 2])], P[..., 3]
    if model == "bi_full":
        return [(P[..., 0], P[..., 1]), (P[..., 2], P[..., 3])], one
    if model == "tri_reduced":
        return [(P[..., 0], P[..., 1]), (P[..., 2], P[..., 3]), (1 - P[..., 0] - P[..., 2], P[..., 4])], one
    if model == "tri_s0":
        return [(P[..., 0], P[..., 1]), (P[..., 2], P[..., 3]), (1 - P[..., 0] - P[..., 2], P[..., 4])], P[..., 5]
    if model == "tri_full":
        return [(P[..., 0], P[..., 1]), (P[..., 2], P[..., 3]), (P[..., 4], P[..., 5])], one
    raise ValueError(model)


def forward(model, b, P):
    """Signal (..., n_b) of parameters P (..., n) in the dtype of P."""
    terms, scale = _terms(model, P)
    b = b.astype(P.dtype)
    s = sum(w[..., None] * np.exp(-b * D[..., None]) for w, D in terms)
    return scale[..., None] * s


def jacobian(model, b, p):
    """Analytic Jacobian (n_b, n) at one parameter vector p (n,), in the dtype of p (models/*.py jacobian())."""
    b = b.astype(p.dtype)
    n = N_PARAMS[model]
    J = np.zeros((b.size, n), p.dtype)
    e = lambda D: np.exp(-b * D)
    if model == "mono":
        J[:, 0] = e(p[1]); J[:, 1] = -b * p[0] * e(p[1])
    elif model in ("bi_reduced", "bi_s0"):
        S0 = p[3] if model == "bi_s0" else p.dtype.type(1)
        J[:, 0] = S0 * (e(p[1]) - e(p[2])); J[:, 1] = -b * S0 * p[0] * e(p[1]); J[:, 2] = -b * S0 * (1 - p[0]) * e(p[2])
        if model == "bi_s0":
            J[:, 3] = p[0] * e(p[1]) + (1 - p[0]) * e(p[2])
    elif model == "bi_full":
        J[:, 0] = e(p[1]); J[:, 1] = -b * p[0] * e(p[1]); J[:, 2] = e(p[3]); J[:, 3] = -b * p[2] * e(p[3])
    elif model in ("tri_reduced", "tri_s0"):
        S0 = p[5] if model == "tri_s0" else p.dtype.type(1)
        f3 = 1 - p[0] - p[2]
        J[:, 0] = S0 * (e(p[1]) - e(p[4])); J[:, 1] = -b * S0 * p[0] * e(p[1]); J[:, 2] = S0 * (e(p[3]) - e(p[4]))
        J[:, 3] = -b * S0 * p[2] * e(p[3]); J[:, 4] = -b * S0 * f3 * e(p[4])
        if model == "tri_s0":
            J[:, 5] = p[0] * e(p[1]) + p[2] * e(p[3]) + f3 * e(p[4])
    elif model == "tri_full":
        for c in range(3):
            J[:, 2 * c] = e(p[2 * c + 1]); J[:, 2 * c + 1] = -b * p[2 * c] * e(p[2 * c + 1])
    else:
        raise ValueError(model)
    return J


def cost64(model, b, y, P):
    """float64 cost 0.5 sum (model - y)^2 per voxel; P (n_vox, n), y (n_vox, n_b)."""
    r = forward(model, np.asarray(b, np.float64), np.asarray(P, np.float64)) - np.asarray(y, np.float64)
    return 0.5 * (r * r).sum(axis=-1)


def cost_floor(y):
    """0.5 n_b (FLT_EPSILON max|y|)^2 per voxel: the cost of float32 rounding of the model itself."""
    y = np.asarray(y, np.float64)
    return 0.5 * y.shape[-1] * (FLT_EPSILON * np.abs(y).max(axis=-1)) ** 2


def cost_excess(model, b, y, P, P_ref):
    return (cost64(model, b, y, P) - cost64(model, b, y, P_ref)) / (cost64(model, b, y, P_ref) + cost_floor(y))


def param_within(P, P_ref, rtol=1e-3):
    return (np.abs(P - P_ref) <= rtol * np.abs(P_ref)).all(axis=-1)


def fit_f32_model(model, b, y, p0, lo, hi, ftol, max_nfev):
    """The reference algorithm on a float32 model; returns (popt float64 | p0 on failure, success)."""
    from scipy.optimize import least_squares

    b = np.asarray(b, np.float64)
    y32 = np.asarray(y, np.float32)
    fun = lambda p: (forward(model, b, p.astype(np.float32)) - y32).astype(np.float64)
    jac = lambda p: jacobian(model, b, p.astype(np.float32)).astype(np.float64)
    try:
        r = least_squares(fun, p0, jac=jac, bounds=(lo, hi), method="trf", ftol=ftol, xtol=1e-8, gtol=1e-8, max_nfev=max_nfev)
    except ValueError:
        return np.array(p0, float), False
    ok = r.status > 0  # curve_fit raises RuntimeError for status 0 (max_nfev): the reference's failure sentinel
    return (r.x if ok else np.array(p0, float)), bool(ok)


def run_fixture(name):
    model = FIXTURES[name]
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    b, y = d["bvalues"], d["y"]
    pv = "p0_arr" in d.files
    n_vox = y.shape[0]
    P = np.empty((n_vox, N_PARAMS[model]))
    ok = np.zeros(n_vox, bool)
    for i in range(n_vox):
        p0, lo, hi = (d["p0_arr"][:, i], d["lo_arr"][:, i], d["hi_arr"][:, i]) if pv else (d["p0_vals"], d["lo_vals"], d["hi_vals"])
        P[i], ok[i] = fit_f32_model(model, b, y[i], p0, lo, hi, float(d["tol"]), int(d["max_iter"]))
    ex = cost_excess(model, b, y, P, d["popt"])
    within = param_within(P, d["popt"])
    rec = {
        "model": model, "n_vox": int(n_vox), "n_b": int(b.size),
        "cost_excess": float(ex[ok].max()) if ok.any() else None,
        "param_share": float(within.mean()),
        "success_share": float((ok == d["success"]).mean()),
        "param_criterion": bool(within.mean() >= 0.9),
    }
    if not rec["param_criterion"]:
        rec["note"] = "the yardstick itself leaves more than 10 % of the voxels outside rtol 1e-3: dropped from the parameter criterion"
    return rec


def main():
    import scipy

    out = {"_about": "written by tools/f32_yardstick.py: scipy least_squares(trf) on a float32 model against the fixtures' reference popt",
           "_scipy": scipy.__version__, "_numpy": np.__version__, "fixtures": {}}
    for name in FIXTURES:
        out["fixtures"][name] = run_fixture(name)
        print(name, out["fixtures"][name], file=sys.stderr)
    with open(os.path.join(GOLDEN, "f32_yardstick.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()

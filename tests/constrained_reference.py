"""numpy / SciPy side of the constrained curve-fit tests (no test functions here): the two reduced tri-exponential models with
their gradients, and the method of pnx_curvefit_simplex_f64 restated with scipy.optimize.least_squares."""
from __future__ import annotations

import numpy as np

BI_OF_TRI = {"tri_reduced": "bi_reduced", "tri_s0": "bi_s0"}
FACE_ROWS = {"tri_reduced": [0, 1, 3], "tri_s0": [0, 1, 3, 5]}  # [f1, D1, D2 (, S0)] in the tri-exponential layout


def tri_signal(model, b, p):
    """p (n_vox, n_all) -> (n_vox, n_b)."""
    e = lambda D: np.exp(-b[None, :] * D[:, None])
    s = p[:, 0:1] * e(p[:, 1]) + p[:, 2:3] * e(p[:, 3]) + (1 - p[:, 0:1] - p[:, 2:3]) * e(p[:, 4])
    return s * p[:, 5:6] if model == "tri_s0" else s


def tri_cost(model, b, y, p):
    return 0.5 * ((tri_signal(model, b, p) - y) ** 2).sum(axis=1)


def tri_grad_f(model, b, y, p):
    """(g_f1, g_f2) of 0.5 ||model - y||^2 per voxel."""
    e = lambda D: np.exp(-b[None, :] * D[:, None])
    r = tri_signal(model, b, p) - y
    s0 = p[:, 5:6] if model == "tri_s0" else 1.0
    g1 = (s0 * (e(p[:, 1]) - e(p[:, 4])) * r).sum(axis=1)
    g2 = (s0 * (e(p[:, 3]) - e(p[:, 4])) * r).sum(axis=1)
    return g1, g2


def face_bounds(lo, hi):
    """Bounds of f1 on the face f2 = 1 - f1: its own, intersected with 1 - those of f2.  lo / hi (n_all,) or (n_all, n_vox)."""
    return np.maximum(lo[0], 1.0 - hi[2]), np.minimum(hi[0], 1.0 - lo[2])


def scipy_method(model, b, y, p0, lo, hi, tol, max_nfev):
    """Two box-bounded TRF fits and a certificate, per voxel, shared p0 / bounds.  Returns popt (n_vox, n_all), lambda, face."""
    from scipy.optimize import least_squares

    n_vox, n_all = len(y), len(p0)
    rows = FACE_ROWS[model]
    popt, lam, face = np.empty((n_vox, n_all)), np.zeros(n_vox), np.zeros(n_vox, np.int8)
    l0, h0 = face_bounds(lo, hi)
    lo2, hi2 = lo[rows].copy(), hi[rows].copy()
    lo2[0], hi2[0] = l0, h0
    for v in range(n_vox):
        full = lambda p: tri_signal(model, b, p[None, :])[0] - y[v]
        r1 = least_squares(full, p0, bounds=(lo, hi), method="trf", ftol=tol, xtol=1e-8, gtol=1e-8, max_nfev=max_nfev)
        assert r1.status > 0
        popt[v] = r1.x
        if r1.x[0] + r1.x[2] <= 1.0:
            continue

        def on_face(q):
            p = r1.x.copy()
            p[rows] = q
            p[2] = 1.0 - q[0]
            return tri_signal(model, b, p[None, :])[0] - y[v]

        q0 = r1.x[rows].copy()
        q0[0] = min(max(r1.x[0] / (r1.x[0] + r1.x[2]), l0), h0)
        r2 = least_squares(on_face, q0, bounds=(lo2, hi2), method="trf", ftol=tol, xtol=1e-8, gtol=1e-8,
                           max_nfev=max(1, max_nfev - r1.nfev))
        assert r2.status > 0
        popt[v, rows] = r2.x
        popt[v, 2] = 1.0 - r2.x[0]
        g1, g2 = tri_grad_f(model, b, y[v:v + 1], popt[v:v + 1])
        lam[v] = -0.5 * (g1[0] + g2[0])
        face[v] = 1 if lam[v] >= 0 else 2
    return popt, lam, face

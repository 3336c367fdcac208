"""numpy restatement of pnx_curvefit_grid_start_f64 (include/pnx.h) for the tests: the dictionary from the stand-in models of
pyneapple_amd/models.py, DIRECT costs 0.5 ||w (y - a s_g)||^2 (the library evaluates the expanded form), the acceptance bound
derived from the rounding of that expanded form, and the acceptance itself."""
from __future__ import annotations

import numpy as np

from pyneapple_amd import api, models

_MODELS = {
    "mono": (models.MonoExpModel, {}),
    "bi_reduced": (models.BiExpModel, {}),
    "bi_s0": (models.BiExpModel, dict(fit_s0=True)),
    "bi_full": (models.BiExpModel, dict(fit_reduced=False)),
    "tri_reduced": (models.TriExpModel, {}),
    "tri_s0": (models.TriExpModel, dict(fit_s0=True)),
    "tri_full": (models.TriExpModel, dict(fit_reduced=False)),
}


def forward_model(model, t1_mode=0, tr=0.0, tm=0.0):
    cls, kw = _MODELS[model]
    kw = dict(kw)
    if t1_mode:
        kw.update(fit_t1=True, repetition_time=tr)
    if t1_mode == 2:
        kw.update(fit_t1_steam=True, mixing_time=tm)
    return cls(**kw)


def signals(model, b, free, fixed_idx=(), fixed_vals=None, t1_mode=0, tr=0.0, tm=0.0):
    """model(b; params) for parameter-major free values (n_free, n) and shared fixed values -> (n, n_b)."""
    m = forward_model(model, t1_mode, tr, tm)
    n_all = len(m._all_param_names)
    fixed_idx = list(fixed_idx)
    free_idx = [i for i in range(n_all) if i not in fixed_idx]
    free = np.asarray(free, float)
    P = np.empty((n_all, free.shape[1]))
    P[free_idx] = free
    for k, i in enumerate(fixed_idx):
        P[i] = fixed_vals[k]
    b = np.asarray(b, float)
    return np.stack([m.forward(b, *P[:, g]) for g in range(P.shape[1])])


def s0_row(model, fixed_idx=()):
    pos = api.MODEL_PARAM_NAMES[model].index("S0")
    return [i for i in range(len(api.MODEL_PARAM_NAMES[model]) + 1) if i not in fixed_idx].index(pos)


def reference(model, b, y, atoms, lo, hi, fixed_idx=(), fixed_vals=None, sigma=None, project=False, t1_mode=0, tr=0.0, tm=0.0):
    """dict(c (n_vox, n_atoms) direct costs, a (n_vox, n_atoms) clipped amplitudes or None, tol (n_vox,), finite (n_vox,) bool)."""
    b, y, atoms = np.asarray(b, float), np.atleast_2d(np.asarray(y, float)), np.array(atoms, float)
    w = np.ones(len(b)) if sigma is None else 1.0 / np.broadcast_to(np.asarray(sigma, float).reshape(-1), (len(b),))
    row = s0_row(model, fixed_idx) if project else None
    if project:
        atoms[row] = 1.0  # the dictionary is built with S0 = 1, whatever the atoms hold
    S = signals(model, b, atoms, fixed_idx, fixed_vals, t1_mode, tr, tm) * w  # (n_atoms, n_b)
    finite = np.isfinite(y * w).all(axis=1)
    yw = np.where(finite[:, None], y * w, 0.0)
    nrm = (S * S).sum(axis=1)
    c = np.empty((len(y), len(S)))
    a = np.empty_like(c) if project else None
    for v0 in range(0, len(y), 512):  # bounded memory: (512, n_atoms, n_b) at a time
        yv = yw[v0:v0 + 512]
        if project:
            with np.errstate(divide="ignore", invalid="ignore"):
                q = np.where(nrm > 0, (yv @ S.T) / nrm, 0.0)
            av = np.clip(q, lo[row], hi[row])
            a[v0:v0 + 512] = av
            c[v0:v0 + 512] = 0.5 * ((yv[:, None, :] - av[:, :, None] * S[None]) ** 2).sum(axis=2)
        else:
            c[v0:v0 + 512] = 0.5 * ((yv[:, None, :] - S[None]) ** 2).sum(axis=2)
    # Each dot product of n_b terms of the expanded form carries a rounding error of at most n_b 2^-53 ||y|| ||s_g||
    tol = 4 * len(b) * 2.0 ** -52 * ((yw * yw).sum(axis=1) + nrm.max())
    return dict(c=c, a=a, tol=tol, finite=finite, s0_row=row)


def accept(ref, got, atoms):
    """The acceptance of the issue, per finite voxel, against a result dict(p0, best, cost) of numpy arrays."""
    c, tol, fin = ref["c"], ref["tol"], ref["finite"]
    best, cost, p0 = got["best"], got["cost"], got["p0"]
    n_atoms = c.shape[1]
    assert best.dtype == np.int32 and best.shape == (len(c),)
    assert ((best[fin] >= 0) & (best[fin] < n_atoms)).all(), "a padded atom or no atom won"
    idx = np.flatnonzero(fin)
    cb = c[idx, best[idx]]
    excess = cb - c[idx].min(axis=1)
    assert (excess <= tol[idx]).all(), f"chosen atom worse than the best by {(excess / tol[idx]).max():.3g} tol"
    dev = np.abs(cost[idx] - cb)
    assert (dev <= tol[idx]).all(), f"reported cost off by {(dev / tol[idx]).max():.3g} tol"
    rows = [k for k in range(p0.shape[0]) if k != ref["s0_row"]]
    bits = lambda x: np.ascontiguousarray(x, np.float64).view(np.uint64)
    assert (bits(p0[rows][:, idx]) == bits(np.asarray(atoms, float)[rows][:, best[idx]])).all(), "p0_out is not a copy of the atom"
    if ref["a"] is not None:
        np.testing.assert_allclose(p0[ref["s0_row"], idx], ref["a"][idx, best[idx]], rtol=1e-12)

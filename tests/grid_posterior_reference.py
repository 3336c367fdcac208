"""numpy restatement of pnx_curvefit_grid_posterior_f64 (include/pnx.h) for the tests: DIRECT costs and the
cancellation bound tol_v from tests/grid_start_reference.py, the same floor, a two-pass log-sum-exp, weighted mean and centred
variance in float64 -- and the acceptance bound per voxel, derived in DESIGN.md 4.1g:

    eps_v   = tol_v / noise_sd^2                       (known noise)
            = (nu / 2) tol_v / (min_g c_g - tol_v)     (marginalised)         + 8 2^-52 max_g |l_g|    the error of one l_g
    gamma   = 4 (G + 16) 2^-52                                                 a weighted sum of G terms
    E_v     = expm1(2 eps_v)                                                   what the normalised weights move by
    R_k     = max_g theta_kg - min_g theta_kg over the admissible atoms (per voxel in a projected S0 row), A_k = max_g |theta_kg|,
    S_k     = R_k for a row centred on the host, A_k for the projected S0 row (accumulated about 0)
    |mean - ref|         <= E_v R_k + gamma S_k + 2^-52 A_k
    |sd^2 - ref|         <= 3 (E_v R_k^2 + gamma S_k^2)
    |log_evidence - ref| <= eps_v + gamma + 2^-52 (|L| + |log sum exp log_prior|)
    |ess - ref|          <= 4 (E_v + gamma) ess_ref
    l_ref[map_atom]      >= max_g l_ref - 2 eps_v

`reference` asserts the precondition of an oracle comparison, eps_v <= 1e-6 on every finite voxel, unless told the case is an
extreme one (max_eps)."""
from __future__ import annotations

import numpy as np
from grid_start_reference import reference as grid_reference

U = 2.0 ** -52


def reference(model, b, y, atoms, lo, hi, log_prior=None, noise_sd=0.0, project=False, max_eps=1e-6, **kw):
    """dict of the reference outputs (n_vox leading), l (n_vox, n_atoms), eps (n_vox,), the bounds per output, finite (n_vox,)."""
    atoms = np.array(atoms, float)
    gs = grid_reference(model, b, y, atoms, lo, hi, project=project, **kw)
    c, amp, tol, fin, row = gs["c"], gs["a"], gs["tol"], gs["finite"], gs["s0_row"]
    n_vox, G = c.shape
    n_b = len(np.asarray(b))
    lp = np.zeros(G) if log_prior is None else np.asarray(log_prior, float)
    adm = lp > -np.inf
    assert adm.any() and not np.isnan(lp).any()
    if noise_sd > 0:
        ell = lp[None, :] - c / noise_sd ** 2
        eps = tol / noise_sd ** 2
    else:
        nu = n_b - (1 if project else 0)
        cmin = c[:, adm].min(axis=1)
        assert (cmin[fin] > tol[fin]).all(), "a compared voxel sits on the cancellation floor"
        ell = lp[None, :] - 0.5 * nu * np.log(np.maximum(c, tol[:, None]))
        eps = 0.5 * nu * tol / np.where(fin, cmin - tol, 1.0)
    ell[:, ~adm] = -np.inf
    eps = eps + 8 * U * np.abs(ell[:, adm]).max(axis=1)
    assert (eps[fin] <= max_eps).all(), f"precondition: eps_v = {eps[fin].max():.3g} > {max_eps:g}"
    m = ell.max(axis=1)
    w = np.exp(ell - m[:, None])  # two passes: the maximum, then the sums
    s = w.sum(axis=1)
    L = m + np.log(s)
    W = w / s[:, None]
    theta = np.repeat(atoms[None], n_vox, axis=0)  # (n_vox, n_free, n_atoms)
    if project:
        theta[:, row, :] = amp
    mean = (W[:, None, :] * theta).sum(axis=2)
    var = (W[:, None, :] * (theta - mean[:, :, None]) ** 2).sum(axis=2)
    ess = 1.0 / (W * W).sum(axis=1)
    lpn = np.log(np.exp(lp[adm] - lp[adm].max()).sum()) + lp[adm].max()
    map_atom = ell.argmax(axis=1)  # the first among equal l
    ta = theta[:, :, adm]
    R = ta.max(axis=2) - ta.min(axis=2)
    A = np.abs(ta).max(axis=2)
    S = R.copy()
    if project:
        S[:, row] = A[:, row]
    gamma = 4 * (G + 16) * U
    E = np.expm1(2 * eps)
    return dict(mean=mean, var=var, log_evidence=L - lpn, ess=ess, map_atom=map_atom, l=ell, eps=eps, finite=fin, s0_row=row, amp=amp,
                bound_mean=E[:, None] * R + gamma * S + U * A, bound_var=3 * (E[:, None] * R * R + gamma * S * S),
                bound_log_evidence=eps + gamma + U * (np.abs(L) + abs(lpn)), bound_ess=4 * (E + gamma) * ess)


def ratios(ref, got):
    """Largest error-to-bound ratio per output over the finite voxels (0 / 0 counts as 0: a row whose bound is 0 must match exactly)."""
    fin = ref["finite"]

    def ratio(err, bound):
        err, bound = np.asarray(err)[fin], np.asarray(bound)[fin]
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / bound)
        return float(q.max()) if q.size else 0.0

    return {"mean": ratio(np.abs(got["mean"].T - ref["mean"]), ref["bound_mean"]),
            "var": ratio(np.abs(got["sd"].T ** 2 - ref["var"]), ref["bound_var"]),
            "log_evidence": ratio(np.abs(got["log_evidence"] - ref["log_evidence"]), ref["bound_log_evidence"]),
            "ess": ratio(np.abs(got["ess"] - ref["ess"]), ref["bound_ess"])}


def accept(ref, got, atoms, scale=1.0):
    """The acceptance of every output of a result dict (api.grid_posterior) on EVERY voxel; returns the error-to-bound ratios."""
    fin, ell = ref["finite"], ref["l"]
    n_vox, G = ell.shape
    atoms = np.asarray(atoms, float)
    for key in ("mean", "sd", "map_p"):
        assert got[key].shape == (atoms.shape[0], n_vox) and got[key].dtype == np.float64
    ma = got["map_atom"]
    assert ma.dtype == np.int32 and ma.shape == (n_vox,)
    # non-finite voxels: NaN everywhere, atom -1
    assert (ma[~fin] == -1).all()
    for key in ("mean", "sd", "map_p"):
        assert np.isnan(got[key][:, ~fin]).all()
    assert np.isnan(got["log_evidence"][~fin]).all() and np.isnan(got["ess"][~fin]).all()
    idx = np.flatnonzero(fin)
    for key in ("mean", "sd", "map_p", "log_evidence", "ess"):
        assert np.isfinite(got[key][..., idx]).all(), key
    assert ((ma[idx] >= 0) & (ma[idx] < G)).all(), "a padded atom or no atom is the MAP"
    short = ell[idx].max(axis=1) - ell[idx, ma[idx]]
    assert (short <= 2 * ref["eps"][idx]).all(), f"MAP atom short of the best l by {(short / ref['eps'][idx]).max():.3g} eps"
    rows = [k for k in range(atoms.shape[0]) if k != ref["s0_row"]]
    bits = lambda x: np.ascontiguousarray(x, np.float64).view(np.uint64)
    assert (bits(got["map_p"][rows][:, idx]) == bits(atoms[rows][:, ma[idx]])).all(), "map_p is not a copy of the atom"
    if ref["amp"] is not None:
        np.testing.assert_allclose(got["map_p"][ref["s0_row"], idx], ref["amp"][idx, ma[idx]], rtol=1e-12)
    assert (got["sd"][:, idx] >= 0).all() and (got["ess"][idx] >= 1 - 1e-12).all() and (got["ess"][idx] <= G * (1 + 1e-12)).all()
    q = ratios(ref, got)
    print("error / bound:", {k: f"{v:.3g}" for k, v in q.items()})
    for key, v in q.items():
        assert v <= scale, f"{key}: error is {v:.3g} x its bound"
    return q

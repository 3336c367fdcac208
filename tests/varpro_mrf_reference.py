"""numpy restatement of the neighbourhood (MRF) prior of the posterior over the variable projection's dictionary (include/pnx.h,
DESIGN.md 4.1q) for the tests, on top of tests/varpro_posterior_reference.py: the field added to its l_g, one colour update, the
driver and the variational free energy.  The gather is tests/grid_mrf_reference.gather (the device's is the grid prior's too).

    l_g(v) = l0_g(v) + sum_{k non-linear} thetac_kg q_vk - 1/2 n_v r_g        l0: varpro_posterior_reference's l, term for term
    thetac_kg = nl_atoms[row_k, g] - centre_k;  q_vk = lambda_k sum_{u present} (mean[k, u] - centre_k);  r_g = sum_k lambda_k thetac_kg^2

A fraction or S0 row has lambda = 0 and centre = 0: it takes no part.  The acceptance bound is the posterior's
(varpro_posterior_reference: eps_v, E_v, gamma, the moment bounds) with eps_v enlarged by the rounding of the field, the term
tests/grid_mrf_reference.py derives, over the n_nl non-linear rows:

    eps_v  +=  4 (n_nl + 2) 2^-52 max_g (sum_k |thetac_kg| |q_vk| + 1/2 n_v r_g)

    F = sum_v sum_g q_vg (l0_vg - log q_vg) - 1/2 sum_edges sum_k lambda_k (var_vk + var_uk + (mu_vk - mu_uk)^2)

is the variational free energy; a colour update is coordinate ascent on it, so it never decreases."""
from __future__ import annotations

import numpy as np
from grid_mrf_reference import colour_sort, gather  # noqa: F401  (colour_sort: for the tests)
from varpro_posterior_reference import U, param_bound
from varpro_posterior_reference import reference as posterior_reference
from varpro_reference import reference as varpro_reference


def base_posterior(model, b, y, nl_atoms, lo, hi, log_prior=None, noise_sd=0.0, marginal=True, max_eps=1e-6, **kw):
    """(varpro_posterior_reference's dict with the clip flags of every pair beside it, nl_atoms, log_prior as an array)."""
    nl_atoms = np.array(nl_atoms, float)
    base = posterior_reference(model, b, y, nl_atoms, lo, hi, log_prior=log_prior, noise_sd=noise_sd, marginal=marginal, max_eps=max_eps, **kw)
    vr = varpro_reference(model, np.asarray(b, float), np.atleast_2d(np.asarray(y, float)), nl_atoms, np.asarray(lo, float), np.asarray(hi, float), **kw)
    base["clipped"] = vr["clipped"]
    base["unsure"] = vr["dist"] <= (vr["K"] + 1) * vr["ptol"]
    base["vr"] = vr
    lp = np.zeros(nl_atoms.shape[1]) if log_prior is None else np.asarray(log_prior, float)
    return base, nl_atoms, lp


def n_free_of(base):
    return len(base["lin_rows"]) + len(base["nl_rows"])


def centres(base, nl_atoms, lp):
    """(n_free,): min + (max - min) / 2 of a non-linear row over the admissible atoms, 0 for a linear row."""
    adm = lp > -np.inf
    mn, mx = nl_atoms[:, adm].min(axis=1), nl_atoms[:, adm].max(axis=1)
    c = np.zeros(n_free_of(base))
    c[base["nl_rows"]] = mn + 0.5 * (mx - mn)
    return c


def ranges(base, nl_atoms, lp):
    adm = lp > -np.inf
    r = np.zeros(n_free_of(base))
    r[base["nl_rows"]] = nl_atoms[:, adm].max(axis=1) - nl_atoms[:, adm].min(axis=1)
    return r


def precision_of(base, nl_atoms, lp, strength):
    """strength / range^2 on the non-linear rows (0 for a one-value row), 0 on the linear rows."""
    r = ranges(base, nl_atoms, lp)
    return np.where(r > 0, strength / np.where(r > 0, r, 1.0) ** 2, 0.0)


def r_row(base, nl_atoms, centre, precision):
    """r_g = sum_k lambda_k thetac_kg^2, k ascending over the free rows that are non-linear."""
    r = np.zeros(nl_atoms.shape[1])
    for j, k in enumerate(base["nl_rows"]):
        t = nl_atoms[j] - centre[k]
        r = r + precision[k] * (t * t)
    return r


def field_terms(base, nl_atoms, centre, precision, q, n):
    """(fld (n_vox, G), magnitude (n_vox,)): the field added to l and the largest sum of the magnitudes of its terms per voxel."""
    rows = list(base["nl_rows"])
    tc = nl_atoms - np.asarray(centre, float)[rows, None]
    r = r_row(base, nl_atoms, centre, precision)
    qn = np.asarray(q, float)[rows]
    fld = qn.T @ tc - 0.5 * n[:, None] * r[None, :]
    mag = (np.abs(qn.T) @ np.abs(tc) + 0.5 * n[:, None] * r[None, :]).max(axis=1)
    return fld, mag


def _posterior_from_l(ell, eps, base, nl_atoms, lp):
    """varpro_posterior_reference's outputs and bounds from a matrix l (n_vox, G) and a per-voxel eps."""
    n_vox, G = ell.shape
    fin, lin, lin_rows, nl_rows = base["finite"], base["lin"], base["lin_rows"], base["nl_rows"]
    n_free = n_free_of(base)
    adm = lp > -np.inf
    m = ell.max(axis=1)
    wgt = np.exp(ell - m[:, None])
    s = wgt.sum(axis=1)
    L = m + np.log(s)
    W = wgt / s[:, None]
    theta = np.empty((n_vox, n_free, G))
    theta[:, nl_rows, :] = nl_atoms[None]
    theta[:, lin_rows, :] = lin.transpose(0, 2, 1)
    mid = np.where(adm[None, None, :], theta, np.nan)
    mid = np.nanmin(mid, axis=2) + 0.5 * (np.nanmax(mid, axis=2) - np.nanmin(mid, axis=2))
    mean = mid + (W[:, None, :] * (theta - mid[:, :, None])).sum(axis=2)
    var = (W[:, None, :] * (theta - mean[:, :, None]) ** 2).sum(axis=2)
    ess = 1.0 / (W * W).sum(axis=1)
    cmass = np.minimum((W * base["clipped"]).sum(axis=1), 1.0)
    lpn = np.log(np.exp(lp[adm] - lp[adm].max()).sum()) + lp[adm].max()
    ta = theta[:, :, adm]
    R = ta.max(axis=2) - ta.min(axis=2)
    A = np.abs(ta).max(axis=2)
    S = R.copy()
    S[:, lin_rows] = A[:, lin_rows]
    pb = param_bound(base["vr"], lin)
    P = np.zeros((n_vox, n_free))
    P[:, lin_rows] = pb[:, adm, :].max(axis=1)
    gamma = 4 * (G + 16) * U
    E = np.expm1(2 * eps)
    return dict(mean=mean, var=var, log_evidence=L - lpn, ess=ess, clipped_mass=cmass, map_atom=ell.argmax(axis=1), l=ell, eps=eps, finite=fin,
                lin=lin, param_bound=pb, lin_rows=lin_rows, nl_rows=nl_rows, W=W, K=base["K"], cls=base["cls"],
                bound_mean=E[:, None] * R + gamma * S + U * A + P, bound_var=3 * (E[:, None] * R * R + gamma * S * S) + 4 * R * P + 4 * P * P,
                bound_log_evidence=eps + gamma + U * (np.abs(L) + abs(lpn)), bound_ess=4 * (E + gamma) * ess,
                bound_clipped_mass=E + gamma + (W * base["unsure"]).sum(axis=1))


def field_posterior(base, nl_atoms, lp, q, n, precision):
    """One update of ALL voxels of `base` under the field (q (n_free, n_vox), n (n_vox,)); the caller keeps the rows of its range.
    The dict of varpro_posterior_reference.reference with the enlarged eps."""
    centre = centres(base, nl_atoms, lp)
    fld, mag = field_terms(base, nl_atoms, centre, np.asarray(precision, float), np.asarray(q, float), np.asarray(n))
    with np.errstate(invalid="ignore"):
        ell = base["l"] + fld
    ell[:, ~(lp > -np.inf)] = -np.inf
    eps = base["eps"] + 4 * (len(base["nl_rows"]) + 2) * U * mag
    return _posterior_from_l(ell, eps, base, nl_atoms, lp)


def free_energy(base, W, mean, var, nb, precision):
    fin = base["finite"]
    l0 = base["l"]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(W > 0, W * (l0 - np.log(np.where(W > 0, W, 1.0))), 0.0)
    F = t[fin].sum()
    lam = np.asarray(precision, float)
    for slot in range(nb.shape[1]):
        u = nb[:, slot]
        ok = (u >= 0) & fin
        ok[ok] &= fin[u[ok]]
        v = np.flatnonzero(ok)
        uu = u[ok]
        F -= 0.25 * (lam[None, :] * (var[v] + var[uu] + (mean[v] - mean[uu]) ** 2)).sum()  # every edge is met from both ends
    return float(F)


def mrf(model, b, y, nl_atoms, lo, hi, nb, colour_start, precision, n_sweeps, tol=0.0, trace_free_energy=False, **kw):
    """The driver: sweep 0 the plain posterior, then colour after colour the gather and the update of that colour's range.
    Returns the last state (n_vox leading), delta (list), and F after every colour update."""
    base, nl_atoms, lp = base_posterior(model, b, y, nl_atoms, lo, hi, **kw)
    nb = np.asarray(nb)
    n_vox = nb.shape[0]
    n_free = n_free_of(base)
    precision = np.asarray(precision, float)
    centre = centres(base, nl_atoms, lp)
    zero = field_posterior(base, nl_atoms, lp, np.zeros((n_free, n_vox)), np.zeros(n_vox, np.int32), precision)
    keys = ("mean", "var", "log_evidence", "ess", "clipped_mass", "map_atom", "W", "l", "eps", "bound_mean", "bound_var", "bound_log_evidence",
            "bound_ess", "bound_clipped_mass")
    state = {k: np.array(zero[k]) for k in keys}
    fin = base["finite"]
    rng = np.where(precision > 0, ranges(base, nl_atoms, lp), 0.0)
    Fs = [free_energy(base, state["W"], state["mean"], state["var"], nb, precision)] if trace_free_energy else []
    delta = []
    for s in range(n_sweeps):
        d = 0.0
        for c in range(len(colour_start) - 1):
            lo_c, hi_c = int(colour_start[c]), int(colour_start[c + 1])
            if hi_c == lo_c:
                continue
            mean_pm = np.where(fin[None, :], state["mean"].T, np.nan)
            q, n = gather(nb, mean_pm, centre, precision)
            new = field_posterior(base, nl_atoms, lp, q, n, precision)
            sel = np.arange(lo_c, hi_c)
            take = sel[fin[sel]]
            for k in np.flatnonzero(rng > 0):
                if take.size:
                    d = max(d, float((np.abs(new["mean"][take, k] - state["mean"][take, k]) / rng[k]).max()))
            for key in keys:
                state[key][sel] = new[key][sel]
            if trace_free_energy:
                Fs.append(free_energy(base, state["W"], state["mean"], state["var"], nb, precision))
        delta.append(d)
        if tol > 0 and d <= tol:
            break
    state.update(finite=fin, lin_rows=base["lin_rows"], nl_rows=base["nl_rows"])
    return state, delta, Fs


def phantom(seed=0, noise=0.05, H=24, W=24):
    """The 24 x 24 two-region bi-exponential phantom with S0 (bi_s0: f1, D1, D2, S0): 16 b-values, the ordered pairs of 19 rates
    over three decades (171 atoms), a 4-neighbourhood, 2 colours.  The regions' rates lie an octave (D1) and 0.85 octave (D2)
    apart.  Returns dict(b, y, truth (n, 4), nl_atoms (2, 171), lo, hi, nb (n, 4), colours (n,))."""
    rng = np.random.default_rng(seed)
    b = np.array([0, 5, 10, 20, 30, 50, 75, 100, 150, 200, 300, 400, 500, 600, 700, 800.0])
    rates = np.geomspace(3e-4, 0.3, 19)
    nl_atoms = np.ascontiguousarray(np.array([(a, c) for a in rates for c in rates if a > c]).T)
    truth = np.zeros((H, W, 4))
    truth[...] = [0.15, 0.02, 0.0010, 1.0]
    truth[H // 4:3 * H // 4, W // 3:5 * W // 6] = [0.30, 0.04, 0.0018, 1.0]
    truth = truth.reshape(-1, 4)
    sig = truth[:, 3:] * (truth[:, :1] * np.exp(-b * truth[:, 1:2]) + (1 - truth[:, :1]) * np.exp(-b * truth[:, 2:3]))
    y = sig + noise * rng.standard_normal(sig.shape)
    idx = np.arange(H * W).reshape(H, W)
    nb = -np.ones((H * W, 4), np.int32)
    nb[idx[1:].ravel(), 0] = idx[:-1].ravel()
    nb[idx[:-1].ravel(), 1] = idx[1:].ravel()
    nb[idx[:, 1:].ravel(), 2] = idx[:, :-1].ravel()
    nb[idx[:, :-1].ravel(), 3] = idx[:, 1:].ravel()
    colours = (np.add.outer(np.arange(H), np.arange(W)) & 1).ravel().astype(np.int32)
    lo, hi = np.array([0.0, 1e-5, 1e-5, 0.0]), np.array([1.0, 0.5, 0.5, 10.0])
    return dict(b=b, y=y, truth=truth, nl_atoms=nl_atoms, lo=lo, hi=hi, nb=nb, colours=colours)

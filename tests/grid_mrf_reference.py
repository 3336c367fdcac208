"""numpy restatement of the neighbourhood (MRF) prior of the grid posterior (include/pnx.h) for the tests, on top
of tests/grid_posterior_reference.py: the gather in slot order, one colour update, the driver and the variational free energy.

    l_g(v) = l0_g(v) + sum_k thetac_kg q_vk - 1/2 n_v r_g          l0: grid_posterior_reference's l, term for term
    thetac_kg = atoms[k, g] - centre_k;  q_vk = lambda_k sum_{u present} (mean[k, u] - centre_k);  r_g = sum_k lambda_k thetac_kg^2

The acceptance bound is the posterior's (grid_posterior_reference: eps_v, E_v, gamma, the moment bounds) with eps_v enlarged by the
rounding of the field.  The field of one pair is a sum of n_free products and one more product, n_free + 1 terms, added to l0 by one
more rounding: evaluated in any order (the matrix cores sum a k-step of four in an order of their own) its error is at most
(n_free + 2) 2^-52 times the sum of the magnitudes of its terms, sum_k |thetac_kg| |q_vk| + 1/2 n_v r_g, to first order.  r_g and
q_vk reach the kernel already rounded (n_free and n_nb additions each, relative error <= 8 2^-52 each), and the reference rounds
the same sums in its own order; a factor 4 over the first-order term covers both sides and the second order:

    eps_v  +=  4 (n_free + 2) 2^-52 max_g (sum_k |thetac_kg| |q_vk| + 1/2 n_v r_g)

    F = sum_v sum_g q_vg (l0_vg - log q_vg) - 1/2 sum_edges sum_k lambda_k (var_vk + var_uk + (mu_vk - mu_uk)^2)

is the variational free energy (l0 holds the log-likelihood and the log prior of the atom); a colour update is coordinate ascent
on it, so it never decreases."""
from __future__ import annotations

import numpy as np
from grid_posterior_reference import U
from grid_posterior_reference import reference as posterior_reference


def centres(atoms, log_prior=None, s0_row=-1):
    atoms = np.asarray(atoms, float)
    adm = np.ones(atoms.shape[1], bool) if log_prior is None else np.asarray(log_prior, float) > -np.inf
    mn, mx = atoms[:, adm].min(axis=1), atoms[:, adm].max(axis=1)
    c = mn + 0.5 * (mx - mn)
    if s0_row is not None and s0_row >= 0:
        c[s0_row] = 0.0
    return c


def gather(nb, mean, centre, precision, first=0, count=None):
    """(q (n_free, count), n (count,)) of the voxels [first, first + count): the slots summed in slot order, then one multiply."""
    nb, mean = np.asarray(nb), np.asarray(mean, float)
    n_free, n_vox = mean.shape
    count = n_vox - first if count is None else count
    rows = nb[first:first + count]
    s = np.zeros((n_free, count))
    n = np.zeros(count, np.int32)
    for slot in range(rows.shape[1]):
        u = rows[:, slot].astype(np.int64)
        ok = (u >= 0) & (u < n_vox)
        uu = np.where(ok, u, 0)
        ok &= np.isfinite(mean[0, uu])
        for k in range(n_free):
            s[k] = np.where(ok, s[k] + (mean[k, uu] - centre[k]), s[k])
        n += ok
    return np.asarray(precision, float)[:, None] * s, n


def _posterior_from_l(ell, eps, base, atoms, lp):
    """grid_posterior_reference's outputs and bounds from a matrix l (n_vox, G) and a per-voxel eps."""
    n_vox, G = ell.shape
    fin, amp = base["finite"], base["amp"]
    row = -1 if base["s0_row"] is None else base["s0_row"]
    adm = lp > -np.inf
    m = ell.max(axis=1)
    w = np.exp(ell - m[:, None])
    s = w.sum(axis=1)
    L = m + np.log(s)
    W = w / s[:, None]
    theta = np.repeat(atoms[None], n_vox, axis=0)
    if row >= 0:
        theta[:, row, :] = amp
    mean = (W[:, None, :] * theta).sum(axis=2)
    var = (W[:, None, :] * (theta - mean[:, :, None]) ** 2).sum(axis=2)
    ess = 1.0 / (W * W).sum(axis=1)
    lpn = np.log(np.exp(lp[adm] - lp[adm].max()).sum()) + lp[adm].max()
    ta = theta[:, :, adm]
    R = ta.max(axis=2) - ta.min(axis=2)
    A = np.abs(ta).max(axis=2)
    S = R.copy()
    if row >= 0:
        S[:, row] = A[:, row]
    gamma = 4 * (G + 16) * U
    E = np.expm1(2 * eps)
    return dict(mean=mean, var=var, log_evidence=L - lpn, ess=ess, map_atom=ell.argmax(axis=1), l=ell, eps=eps, finite=fin, s0_row=base["s0_row"], amp=amp,
                W=W, bound_mean=E[:, None] * R + gamma * S + U * A, bound_var=3 * (E[:, None] * R * R + gamma * S * S),
                bound_log_evidence=eps + gamma + U * (np.abs(L) + abs(lpn)), bound_ess=4 * (E + gamma) * ess)


def field_terms(atoms, centre, precision, q, n, s0_row=-1):
    """(fld (n_vox, G), magnitude (n_vox,)): the field added to l and the largest sum of the magnitudes of its terms per voxel."""
    tc = np.asarray(atoms, float) - np.asarray(centre, float)[:, None]
    if s0_row >= 0:
        tc[s0_row] = 0.0
    lam = np.asarray(precision, float)
    r = np.zeros(tc.shape[1])
    for k in range(tc.shape[0]):
        r = r + lam[k] * (tc[k] * tc[k])
    fld = q.T @ tc - 0.5 * n[:, None] * r[None, :]
    mag = (np.abs(q.T) @ np.abs(tc) + 0.5 * n[:, None] * r[None, :]).max(axis=1)
    return fld, mag


def base_posterior(model, b, y, atoms, lo, hi, log_prior=None, noise_sd=0.0, project=False, max_eps=1e-6, **kw):
    atoms = np.array(atoms, float)
    base = posterior_reference(model, b, y, atoms, lo, hi, log_prior=log_prior, noise_sd=noise_sd, project=project, max_eps=max_eps, **kw)
    lp = np.zeros(atoms.shape[1]) if log_prior is None else np.asarray(log_prior, float)
    return base, atoms, lp


def field_posterior(base, atoms, lp, q, n, precision):
    """One update of ALL voxels of `base` (base_posterior's first result) under the field (q (n_free, n_vox), n (n_vox,)); the
    caller keeps the rows of its range.  The dict of grid_posterior_reference.reference with the enlarged eps."""
    row = -1 if base["s0_row"] is None else base["s0_row"]
    centre = centres(atoms, lp, row)
    fld, mag = field_terms(atoms, centre, precision, np.asarray(q, float), np.asarray(n), row)
    with np.errstate(invalid="ignore"):
        ell = base["l"] + fld
    ell[:, ~(lp > -np.inf)] = -np.inf
    eps = base["eps"] + 4 * (atoms.shape[0] + 2) * U * mag
    return _posterior_from_l(ell, eps, base, atoms, lp)


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


def mrf(model, b, y, atoms, lo, hi, nb, colour_start, precision, n_sweeps, tol=0.0, trace_free_energy=False, **kw):
    """The driver: sweep 0 the plain posterior, then colour after colour the gather and the update of that colour's range.
    Returns the last state (n_vox leading, as grid_posterior_reference), delta (list), and F after every colour update."""
    base, atoms, lp = base_posterior(model, b, y, atoms, lo, hi, **kw)
    nb = np.asarray(nb)
    n_vox = nb.shape[0]
    precision = np.asarray(precision, float)
    centre = centres(atoms, lp, base["s0_row"])  # None: no projected row
    zero = field_posterior(base, atoms, lp, np.zeros((atoms.shape[0], n_vox)), np.zeros(n_vox, np.int32), precision)
    keys = ("mean", "var", "log_evidence", "ess", "map_atom", "W", "l", "eps", "bound_mean", "bound_var", "bound_log_evidence", "bound_ess")
    state = {k: np.array(zero[k]) for k in keys}
    fin = base["finite"]
    adm = lp > -np.inf
    rng = np.where(precision > 0, atoms[:, adm].max(axis=1) - atoms[:, adm].min(axis=1), 0.0)
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
            new = field_posterior(base, atoms, lp, q, n, precision)
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
    state.update(finite=fin, s0_row=base["s0_row"], amp=base["amp"])
    return state, delta, Fs


def phantom(seed=0, noise=0.05, H=24, W=24):
    """The 24 x 24 two-region reduced bi-exponential phantom: 16 b-values, an 8^3 grid, a 4-neighbourhood, 2 colours.  Returns
    dict(b, y, truth (n, 3), atoms (3, 512), lo, hi, nb (n, 4), colours (n,))."""
    rng = np.random.default_rng(seed)
    b = np.array([0, 5, 10, 20, 30, 50, 75, 100, 150, 200, 300, 400, 500, 600, 700, 800.0])
    f, D1, D2 = np.linspace(0.05, 0.5, 8), np.geomspace(0.005, 0.1, 8), np.geomspace(0.0005, 0.003, 8)
    atoms = np.stack(np.meshgrid(f, D1, D2, indexing="ij"), -1).reshape(-1, 3).T.copy()
    truth = np.zeros((H, W, 3))
    truth[...] = [0.15, 0.02, 0.0010]
    truth[H // 4:3 * H // 4, W // 3:5 * W // 6] = [0.30, 0.04, 0.0018]
    truth = truth.reshape(-1, 3)
    sig = truth[:, :1] * np.exp(-b * truth[:, 1:2]) + (1 - truth[:, :1]) * np.exp(-b * truth[:, 2:3])
    y = sig + noise * rng.standard_normal(sig.shape)
    idx = np.arange(H * W).reshape(H, W)
    nb = -np.ones((H * W, 4), np.int32)
    nb[idx[1:].ravel(), 0] = idx[:-1].ravel()
    nb[idx[:-1].ravel(), 1] = idx[1:].ravel()
    nb[idx[:, 1:].ravel(), 2] = idx[:, :-1].ravel()
    nb[idx[:, :-1].ravel(), 3] = idx[:, 1:].ravel()
    colours = (np.add.outer(np.arange(H), np.arange(W)) & 1).ravel().astype(np.int32)
    lo, hi = np.array([0.0, 0.001, 0.0001]), np.array([1.0, 0.5, 0.01])
    return dict(b=b, y=y, truth=truth, atoms=atoms, lo=lo, hi=hi, nb=nb, colours=colours)


def colour_sort(nb, colours):
    """(order, sorted table, colour_start): what HipBayesGridSolver.colour_sort does, restated."""
    order = np.argsort(colours, kind="stable")
    place = np.empty(order.size, np.int64)
    place[order] = np.arange(order.size)
    rows = nb[order]
    return order, np.where(rows >= 0, place[np.maximum(rows, 0)], -1).astype(np.int32), np.concatenate([[0], np.cumsum(np.bincount(colours))]).astype(np.int64)

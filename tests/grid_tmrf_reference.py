"""numpy restatement of the edge-preserving (Student-t) neighbourhood prior of the grid posterior (include/pnx.h)
for the tests, on top of tests/grid_mrf_reference.py (imported, not copied): the weighted gather in the stated order of operations,
one colour update under a real weight sum, the driver, and the free energy with an explicit weight per edge.

    s_uv = sum_k lambda_k (var_vk + var_uk + (mu_vk - mu_uk)^2)     k ascending, rows with lambda_k = 0 skipped, var = sd * sd
    w_uv = (nu + K) / (nu + s_uv)                                    K = #{k: lambda_k > 0}
    q_vk = lambda_k sum_{u present} w_uv (mean[k, u] - centre_k);  W_v = sum_{u present} w_uv;  l_g(v) = l0_g(v) + thetac_g . q_v - 1/2 W_v r_g

The bound of the gather, from the operation count (u = 2^-53; the kernel fuses some multiply-adds, numpy none, so each side has
its own roundings and the bound covers both).  A term sd_v^2 + sd_u^2 + d^2 is a sum of positive parts: three products and two
additions on a once-rounded d, relative error <= 4 u; times lambda_k, + u; K positive terms summed, + (K - 1) u: s is within
(K + 5) u.  nu + s, the quotient and the host's nu + K add one rounding each: w is within (K + 8) u per side,

    |w_dev - w_ref| <= (K + 8) 2^-52 w                                                      EW = (K + 8) 2^-52

Carried through: a term w (m - c) has one rounding in the difference and one in the product, the sum over the n_nb slots n_nb more,
the final multiply by lambda_k one:

    |q_dev - q_ref| <= (EW + (n_nb + 3) 2^-52) lambda_k sum_u w_uv |mean[k, u] - centre_k|
    |W_dev - W_ref| <= (EW + n_nb 2^-52) W_v

The bound of one colour update is grid_mrf_reference.field_posterior's with n_v replaced by W_v in the field's magnitude
(field_terms takes a real weight as it stands).

    F = sum_v sum_g q_vg (l0_vg - log q_vg) + sum_edges [a log w_uv - 1/2 w_uv (nu + s_uv)],      a = (nu + K) / 2

is the free energy with the edge weights explicit: every update -- of a colour's q_v, or of the weights of the edges that touch
it -- maximises F over that block, so F never decreases, whatever the number of colours."""
from __future__ import annotations

import numpy as np
import grid_mrf_reference as R
from grid_mrf_reference import U  # noqa: F401  (2^-52, the unit the bounds are written in)


def n_rows(precision):
    return int((np.asarray(precision, float) > 0).sum())


def weight_rel_bound(precision):
    return (n_rows(precision) + 8) * 2.0 ** -52


def gather(nb, mean, sd, centre, precision, dof, first=0, count=None):
    """dict(q (n_free, count), w (count,), n (count,) int32, edge (count, n_nb), bound_q, bound_w) of the voxels
    [first, first + count), in the order of operations include/pnx.h states."""
    nb, mean, sd = np.asarray(nb), np.asarray(mean, float), np.asarray(sd, float)
    lam, centre = np.asarray(precision, float), np.asarray(centre, float)
    n_free, n_vox = mean.shape
    count = n_vox - first if count is None else count
    rows = nb[first:first + count]
    v = np.arange(first, first + count)
    own = np.isfinite(mean[0, v])
    K = n_rows(lam)
    dof_k = dof + K
    acc, mag = np.zeros((n_free, count)), np.zeros((n_free, count))
    wsum = np.zeros(count)
    n = np.zeros(count, np.int32)
    edge = np.zeros(rows.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        for slot in range(rows.shape[1]):
            u = rows[:, slot].astype(np.int64)
            ok = (u >= 0) & (u < n_vox)
            uu = np.where(ok, u, 0)
            ok &= np.isfinite(mean[0, uu]) & own
            s = np.zeros(count)
            for k in np.flatnonzero(lam > 0):
                d = mean[k, v] - mean[k, uu]
                s = s + lam[k] * (sd[k, v] * sd[k, v] + sd[k, uu] * sd[k, uu] + d * d)
            w = np.where(ok, dof_k / (dof + s), 0.0)
            edge[:, slot] = w
            wsum = np.where(ok, wsum + w, wsum)
            n += ok
            for k in range(n_free):
                t = w * (mean[k, uu] - centre[k])
                acc[k] = np.where(ok, acc[k] + t, acc[k])
                mag[k] = np.where(ok, mag[k] + np.abs(t), mag[k])
    ew = weight_rel_bound(lam)
    return dict(q=lam[:, None] * acc, w=wsum, n=n, edge=edge, bound_q=(ew + (rows.shape[1] + 3) * R.U) * lam[:, None] * mag,
                bound_w=(ew + rows.shape[1] * R.U) * wsum, bound_edge=ew * edge)


def field_posterior(base, atoms, lp, q, w, precision):
    """grid_mrf_reference.field_posterior under a real weight sum w (n_vox,): the same l, the same bounds with n_v -> W_v."""
    return R.field_posterior(base, atoms, lp, q, np.asarray(w, float), precision)


def edge_s(nb, mean, var, precision, fin):
    """(s (n_vox, n_nb), present (n_vox, n_nb)) from mean, var (n_vox, n_free): every directed slot."""
    lam = np.asarray(precision, float)
    u = np.maximum(nb, 0)
    ok = (nb >= 0) & fin[:, None] & fin[u]
    with np.errstate(invalid="ignore"):
        s = (lam[None, None, :] * (var[:, None, :] + var[u] + (mean[:, None, :] - mean[u]) ** 2)).sum(axis=2)
    return np.where(ok, s, 0.0), ok


def free_energy(base, W, mean, var, nb, precision, dof, w_edge):
    """F with the explicit weights w_edge (n_vox, n_nb), one per directed slot; an undirected edge is met from both ends."""
    fin = base["finite"]
    l0 = base["l"]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(W > 0, W * (l0 - np.log(np.where(W > 0, W, 1.0))), 0.0)
    F = t[fin].sum()
    a = 0.5 * (dof + n_rows(precision))
    s, ok = edge_s(nb, mean, var, precision, fin)
    w = np.where(ok, w_edge, 1.0)
    F += 0.5 * np.where(ok, a * np.log(w) - 0.5 * w * (dof + s), 0.0).sum()
    return float(F)


def tmrf(model, b, y, atoms, lo, hi, nb, colour_start, precision, dof, n_sweeps, tol=0.0, trace_free_energy=False, **kw):
    """The driver: sweep 0 the plain posterior, then colour after colour the weighted gather and the update of that colour's range.
    Returns the last state (n_vox leading, with field_w and field_n of every voxel's last update), delta (list), and -- with
    trace_free_energy -- F after the start, after every refresh of a colour's edge weights and after every colour update."""
    base, atoms, lp = R.base_posterior(model, b, y, atoms, lo, hi, **kw)
    nb = np.asarray(nb)
    n_vox = nb.shape[0]
    precision = np.asarray(precision, float)
    centre = R.centres(atoms, lp, base["s0_row"])
    zero = field_posterior(base, atoms, lp, np.zeros((atoms.shape[0], n_vox)), np.zeros(n_vox), precision)
    keys = ("mean", "var", "log_evidence", "ess", "map_atom", "W", "l", "eps", "bound_mean", "bound_var", "bound_log_evidence", "bound_ess")
    state = {k: np.array(zero[k]) for k in keys}
    state["field_w"], state["field_n"] = np.zeros(n_vox), np.zeros(n_vox, np.int32)
    fin = base["finite"]
    adm = lp > -np.inf
    rng = np.where(precision > 0, atoms[:, adm].max(axis=1) - atoms[:, adm].min(axis=1), 0.0)
    K = n_rows(precision)
    Fs, w_edge = [], None
    if trace_free_energy:  # the start: every weight at its optimum for the plain posterior's moments
        s, ok = edge_s(nb, state["mean"], state["var"], precision, fin)
        w_edge = np.where(ok, (dof + K) / (dof + s), 0.0)
        Fs.append(free_energy(base, state["W"], state["mean"], state["var"], nb, precision, dof, w_edge))
    delta = []
    for _ in range(n_sweeps):
        d = 0.0
        for c in range(len(colour_start) - 1):
            lo_c, hi_c = int(colour_start[c]), int(colour_start[c + 1])
            if hi_c == lo_c:
                continue
            mean_pm = np.where(fin[None, :], state["mean"].T, np.nan)
            with np.errstate(invalid="ignore"):
                sd_pm = np.sqrt(np.maximum(state["var"].T, 0.0))
            g = gather(nb, mean_pm, sd_pm, centre, precision, dof)
            sel = np.arange(lo_c, hi_c)
            if trace_free_energy:  # the edges that touch the colour take their new weights, from both ends; the others keep theirs
                touch = np.zeros(nb.shape, bool)
                touch[sel] = True
                touch |= (nb >= lo_c) & (nb < hi_c)
                w_edge = np.where(touch, g["edge"], w_edge)
                Fs.append(free_energy(base, state["W"], state["mean"], state["var"], nb, precision, dof, w_edge))
            new = field_posterior(base, atoms, lp, g["q"], g["w"], precision)
            take = sel[fin[sel]]
            for k in np.flatnonzero(rng > 0):
                if take.size:
                    d = max(d, float((np.abs(new["mean"][take, k] - state["mean"][take, k]) / rng[k]).max()))
            for key in keys:
                state[key][sel] = new[key][sel]
            state["field_w"][sel], state["field_n"][sel] = g["w"][sel], g["n"][sel]
            if trace_free_energy:
                Fs.append(free_energy(base, state["W"], state["mean"], state["var"], nb, precision, dof, w_edge))
        delta.append(d)
        if tol > 0 and d <= tol:
            break
    state.update(finite=fin, s0_row=base["s0_row"], amp=base["amp"])
    return state, delta, Fs


def delta_tolerance(before, after, atoms, lp, precision, dof, n_nb):
    """How far the first sweep's delta of a device run may lie from the reference's.  The device's means and variances differ from
    the reference's by at most their bounds, dm = max bound_mean / R and dv = max bound_var / R^2 in units of the rows' ranges R_k
    (S_k = lambda_k R_k^2 the strengths, S their sum).  The second colour's gather reads such moments: |d| <= R and var <= R^2 / 4
    give |ds| <= S (2 dv + 4 dm), |dw| <= w_max |ds| / nu with w_max = (nu + K) / nu; with |thetac| <= R / 2 and r_g <= S / 4 the
    field moves by at most dl = n_nb S (w_max dm / 2 + 3 dw / 8), and a field off by dl moves a mean by at most expm1(2 dl) R
    (the posterior's own argument for eps).  On top come the bounds of the old and of the new mean themselves."""
    lam = np.asarray(precision, float)
    adm = lp > -np.inf
    Rk = atoms[:, adm].max(axis=1) - atoms[:, adm].min(axis=1)
    rows = np.flatnonzero((lam > 0) & (Rk > 0))
    fin = before["finite"]
    dm = max(float((st["bound_mean"][fin][:, rows] / Rk[rows]).max()) for st in (before, after))
    dv = max(float((st["bound_var"][fin][:, rows] / Rk[rows] ** 2).max()) for st in (before, after))
    S = float((lam[rows] * Rk[rows] ** 2).sum())
    w_max = (dof + n_rows(lam)) / dof
    dw = w_max * S * (2 * dv + 4 * dm) / dof
    dl = n_nb * S * (0.5 * w_max * dm + 0.375 * dw)
    return 2 * dm + float(np.expm1(2 * dl))

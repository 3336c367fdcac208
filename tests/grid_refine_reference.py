"""numpy restatement of pnx_curvefit_grid_refine_f64 (include/pnx.h) for the tests: per voxel the axes of the fine
grid, their Cartesian product (first row slowest), the fraction-sum rule, the DIRECT cost 1/2 sum_i (y_i - s_i)^2 (after the clipped
amplitude under projection), l, a two-pass log-sum-exp, weighted mean and centred variance, ess, log_norm and edge_mass -- and the
acceptance bound per voxel, derived as tests/grid_posterior_reference.py derives its own, with the cancellation bound tol_v replaced
by the rounding of the direct cost.  With U = 2^-52, per voxel v and atom g:

    T       = max |b_i x| over the rate axes; an axis value differs between the two sides by at most 3 U max(|a|, |b|) (the step
              and the fma against two roundings), the argument b_i x by 4 U |b_i x|, exp by 2 U on either side:
    dE      = (4 |b_i x| + 4) U E <= (4 T + 4) U E
    ds_i    = (4 T + 10) U A_i,  A_i = sum_c |w_c| E_ci >= |s_i|      (the weights, their products and the sum: 6 U A_i more)
    no projection:  dd_i = ds_i + U |d_i|
    projection:     da = [sum |y_i| ds_i + (n_b + 1) U sum |y_i s_i| + |a| (2 sum |s_i| ds_i + (n_b + 1) U nrm)] / nrm + U |a|
                    dd_i = |a| ds_i + |s_i| da + 2 U (|y_i| + |a s_i|)
    dc_g    = sum_i |d_i| dd_i + (n_b + 4) U c_g
    eps_v   = max_g dc_g / noise_sd^2                  (known noise)
            = (nu / 2) max_g dc_g / c_g                (marginalised; asserted: c_g > tol_v)         + 8 U max_g |l_g|
    gamma   = 4 (G + 64) U          a weighted sum of G terms, folded in 64 lanes and merged in 6 steps
    E_v     = expm1(2 eps_v)
    R_k     = b - a of the voxel's axis (max - min of a_g in a projected S0 row), A_k = max |theta_kg|, dth_k = 4 U A_k (max_g da_g in a
              projected S0 row), S_k = R_k (A_k in the projected S0 row, accumulated about 0)
    |mean - ref|      <= E_v R_k + gamma S_k + U A_k + dth_k
    |sd^2 - ref|      <= 3 (E_v R_k^2 + gamma S_k^2) + 4 R_k dth_k
    |ess - ref|       <= 4 (E_v + gamma) ess_ref
    |log_norm - ref|  <= eps_v + gamma + 2 U (|L| + log n_admitted)
    |edge_mass - ref| <= 2 (E_v + gamma)
    l_ref[MAP atom]   >= max_g l_ref - 2 eps_v;  map_p within dth_k of that atom's values

Nothing here is tuned on the device.  `margin` is the smallest |f1 + f2 - 1| (|f1 - 1|) over the atoms that do not sit on the face
exactly by construction: a case is only compared when no atom is within 1e-9 of the face, where one rounding would flip it."""
from __future__ import annotations

import itertools

import numpy as np

U = 2.0 ** -52
DBL_MIN = 2.2250738585072014e-308
LAYOUT = {"mono": ["S0", "D1"], "bi_reduced": ["f1", "D1", "D2"], "bi_s0": ["f1", "D1", "D2", "S0"], "bi_full": ["f1", "D1", "f2", "D2"],
          "tri_reduced": ["f1", "D1", "f2", "D2", "D3"], "tri_s0": ["f1", "D1", "f2", "D2", "D3", "S0"],
          "tri_full": ["f1", "D1", "f2", "D2", "f3", "D3"]}
RATES = {"mono": [1], "bi_reduced": [1, 2], "bi_s0": [1, 2], "bi_full": [1, 3], "tri_reduced": [1, 3, 4], "tri_s0": [1, 3, 4], "tri_full": [1, 3, 5]}
S0_POS = {"mono": 0, "bi_s0": 3, "tri_s0": 5}


def weights(model, P):
    """The weight of every exponential, (n_comp, n): s = S0 * sum_c w_c exp(-b D_c) (S0 = 1 where the layout has none)."""
    if model == "mono":
        return np.ones((1, P.shape[1]))
    if model in ("bi_reduced", "bi_s0"):
        return np.stack([P[0], 1 - P[0]])
    if model == "bi_full":
        return np.stack([P[0], P[2]])
    if model in ("tri_reduced", "tri_s0"):
        return np.stack([P[0], P[2], 1 - P[0] - P[2]])
    return np.stack([P[0], P[2], P[4]])


def admissible(model, P):
    if model in ("bi_reduced", "bi_s0"):
        return P[0] <= 1.0
    if model in ("tri_reduced", "tri_s0"):
        return P[0] + P[2] <= 1.0
    return np.ones(P.shape[1], bool)


def face_distance(model, P):
    if model in ("bi_reduced", "bi_s0"):
        return np.abs(P[0] - 1.0)
    if model in ("tri_reduced", "tri_s0"):
        return np.abs(P[0] + P[2] - 1.0)
    return np.full(P.shape[1], np.inf)


def axis(lo, hi, c, h, m):
    """(values, a, b) of one axis of one voxel, the header's construction."""
    a, b = max(lo, c - h), min(hi, c + h)
    if m == 1 or not b > a:
        v = min(max(c, lo), hi)
        return np.array([v]), v, v
    step = (b - a) / (m - 1)
    x = a + np.arange(m) * step
    x[-1] = b
    return x, a, b


def reference(model, b, y, lo, hi, n_points, centre, half_width, noise_sd=0.0, project=False, fixed_idx=(), fixed_vals=None, max_eps=1e-6):
    """dict of the reference outputs (n_vox leading), the bounds per output, finite (n_vox,), per voxel the atoms (n_free, G_v),
    their admitted mask and l."""
    b, y = np.asarray(b, float), np.atleast_2d(np.asarray(y, float))
    centre, half_width = np.asarray(centre, float), np.asarray(half_width, float)
    n_vox, n_b = y.shape
    n_all = len(LAYOUT[model])
    fixed_idx = list(fixed_idx)
    free_idx = [i for i in range(n_all) if i not in fixed_idx]
    n_free = len(free_idx)
    s0_row = free_idx.index(S0_POS[model]) if project else None
    nu = n_b - (1 if project else 0)
    marginal = not noise_sd > 0
    keys2 = ("mean", "var", "map_p", "edge_mass", "bound_mean", "bound_var", "bound_map_p")
    out = {k: np.full((n_vox, n_free), np.nan) for k in keys2}
    for k in ("ess", "log_norm", "eps", "bound_ess", "bound_log_norm", "bound_edge_mass", "margin"):
        out[k] = np.full(n_vox, np.nan)
    out["finite"] = np.zeros(n_vox, bool)
    out["n_atoms"] = np.zeros(n_vox, int)
    out["n_admitted"] = np.zeros(n_vox, int)
    out["atoms"], out["l"], out["adm"] = [None] * n_vox, [None] * n_vox, [None] * n_vox
    out["s0_row"] = s0_row
    for v in range(n_vox):
        rows = [k for k in range(n_free) if k != s0_row]
        ok = np.isfinite(y[v]).all() and np.isfinite(centre[rows, v]).all() and np.isfinite(half_width[rows, v]).all() and (half_width[rows, v] >= 0).all()
        if not ok:
            continue
        axes, span, cc = [], np.zeros(n_free), np.zeros(n_free)
        for k in range(n_free):
            if k == s0_row:
                axes.append(np.array([1.0]))
                continue
            x, a_, b_ = axis(lo[k], hi[k], centre[k, v], half_width[k, v], int(n_points[k]))
            axes.append(x)
            span[k] = b_ - a_
            cc[k] = min(max(centre[k, v], lo[k]), hi[k])
        idx = np.array(list(itertools.product(*[range(len(x)) for x in axes]))).T  # (n_free, G), the first row slowest
        theta = np.stack([axes[k][idx[k]] for k in range(n_free)])
        G = theta.shape[1]
        P = np.empty((n_all, G))
        P[free_idx] = theta
        for k, i in enumerate(fixed_idx):
            P[i] = fixed_vals[k]
        adm = admissible(model, P)
        fd = face_distance(model, P)
        out["margin"][v] = fd[fd > 0].min() if (fd > 0).any() else np.inf
        out["n_atoms"][v], out["n_admitted"][v] = G, int(adm.sum())
        out["atoms"][v], out["adm"][v] = theta, adm
        if not adm.any():
            continue
        out["finite"][v] = True
        w = weights(model, P)  # (n_comp, G)
        D = P[RATES[model]]  # (n_comp, G)
        arg = b[None, None, :] * D[:, :, None]
        Ex = np.exp(-arg)
        base = (w[:, :, None] * Ex).sum(axis=0)  # (G, n_b)
        A = (np.abs(w)[:, :, None] * Ex).sum(axis=0)
        T = np.abs(arg).max()
        s0 = 1.0 if (project or model not in S0_POS) else P[S0_POS[model]][:, None]
        s = base * s0
        ds = (4 * T + 10) * U * A * np.abs(s0)
        yv = y[v][None, :]
        if project:
            dot, nrm = (yv * s).sum(axis=1), (s * s).sum(axis=1)
            with np.errstate(divide="ignore", invalid="ignore"):
                amp = np.where(nrm > 0, dot / nrm, lo[s0_row])
            amp = np.clip(amp, lo[s0_row], hi[s0_row])
            with np.errstate(divide="ignore", invalid="ignore"):
                da = ((np.abs(yv) * ds).sum(axis=1) + (n_b + 1) * U * np.abs(yv * s).sum(axis=1)
                      + np.abs(amp) * (2 * (np.abs(s) * ds).sum(axis=1) + (n_b + 1) * U * nrm)) / nrm + U * np.abs(amp)
            da = np.where(nrm > 0, da, 0.0)
            d = yv - amp[:, None] * s
            dd = np.abs(amp)[:, None] * ds + np.abs(s) * da[:, None] + 2 * U * (np.abs(yv) + np.abs(amp[:, None] * s))
            theta = theta.copy()
            theta[s0_row] = amp
        else:
            d = yv - s
            dd = ds + U * np.abs(d)
        c = 0.5 * (d * d).sum(axis=1)
        dc = (np.abs(d) * dd).sum(axis=1) + (n_b + 4) * U * c
        if marginal:
            tol = max(4 * n_b * U * float((y[v] ** 2).sum()), DBL_MIN)
            assert (c[adm] > tol).all(), "a compared voxel sits on the floor of the cost"
            ell = -0.5 * nu * np.log(np.maximum(c, tol))
            eps = 0.5 * nu * (dc[adm] / c[adm]).max()
        else:
            ell = -c / noise_sd ** 2
            eps = dc[adm].max() / noise_sd ** 2
        ell = np.where(adm, ell, -np.inf)
        eps = eps + 8 * U * np.abs(ell[adm]).max()
        assert eps <= max_eps, f"precondition: eps_v = {eps:.3g} > {max_eps:g}"
        m = ell.max()
        wt = np.exp(ell - m)
        sw = wt.sum()
        L = m + np.log(sw)
        W = wt / sw
        mean = cc + (W[None] * (theta - cc[:, None])).sum(axis=1)  # about the clipped centre, as the header: exact for a one-value row
        var = (W[None] * (theta - mean[:, None]) ** 2).sum(axis=1)
        n_adm = int(adm.sum())
        edge = np.zeros(n_free)
        for k in range(n_free):
            mk = len(axes[k])
            if mk > 1:
                edge[k] = W[(idx[k] == 0) | (idx[k] == mk - 1)].sum()
        ta = theta[:, adm]
        Ak = np.abs(ta).max(axis=1)
        R, S, dth = span.copy(), span.copy(), 4 * U * Ak
        if project:
            R[s0_row] = ta[s0_row].max() - ta[s0_row].min()
            S[s0_row] = Ak[s0_row]
            dth[s0_row] = da[adm].max()
        gamma = 4 * (G + 64) * U
        E = np.expm1(2 * eps)
        g = int(ell.argmax())
        out["mean"][v], out["var"][v], out["map_p"][v], out["edge_mass"][v] = mean, var, theta[:, g], edge
        out["ess"][v], out["log_norm"][v], out["eps"][v] = 1.0 / (W * W).sum(), L - np.log(n_adm), eps
        out["l"][v] = ell
        out["bound_mean"][v] = E * R + gamma * S + U * Ak + dth
        out["bound_var"][v] = 3 * (E * R * R + gamma * S * S) + 4 * R * dth
        out["bound_map_p"][v] = dth
        out["bound_ess"][v] = 4 * (E + gamma) * out["ess"][v]
        out["bound_log_norm"][v] = eps + gamma + 2 * U * (abs(L) + np.log(n_adm))
        out["bound_edge_mass"][v] = 2 * (E + gamma)
        out.setdefault("theta", [None] * n_vox)[v] = theta
    return out


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
            "ess": ratio(np.abs(got["ess"] - ref["ess"]), ref["bound_ess"]),
            "log_norm": ratio(np.abs(got["log_norm"] - ref["log_norm"]), ref["bound_log_norm"]),
            "edge_mass": ratio(np.abs(got["edge_mass"].T - ref["edge_mass"]), ref["bound_edge_mass"][:, None] * np.ones_like(ref["edge_mass"]))}


def accept(ref, got, scale=1.0):
    """The acceptance of every output of a result dict (api.grid_refine) on EVERY voxel; returns the error-to-bound ratios."""
    fin = ref["finite"]
    n_vox, n_free = ref["mean"].shape
    for key in ("mean", "sd", "map_p", "edge_mass"):
        assert got[key].shape == (n_free, n_vox) and got[key].dtype == np.float64
        assert np.isnan(got[key][:, ~fin]).all(), key
        assert np.isfinite(got[key][:, fin]).all(), key
    for key in ("ess", "log_norm"):
        assert got[key].shape == (n_vox,) and np.isnan(got[key][~fin]).all() and np.isfinite(got[key][fin]).all(), key
    assert (ref["margin"][fin] > 1e-9).all(), "precondition: an atom sits within a rounding of the face f1 + f2 = 1"
    for v in np.flatnonzero(fin):
        # the MAP atom: the values reported belong to an atom whose l is within 2 eps of the best
        th, ell = ref["theta"][v], ref["l"][v]
        near = (np.abs(th - got["map_p"][:, v][:, None]) <= ref["bound_map_p"][v][:, None]).all(axis=0) & ref["adm"][v]
        assert near.any(), f"voxel {v}: map_p is no atom of the fine grid"
        assert ell[near].max() >= ell.max() - 2 * ref["eps"][v], f"voxel {v}: the MAP atom is short of the best l"
    assert (got["sd"][:, fin] >= 0).all() and (got["edge_mass"][:, fin] >= 0).all() and (got["edge_mass"][:, fin] <= 1 + 1e-12).all()
    assert (got["ess"][fin] >= 1 - 1e-12).all() and (got["ess"][fin] <= ref["n_admitted"][fin] * (1 + 1e-12)).all()
    q = ratios(ref, got)
    print("error / bound:", {k: f"{v:.3g}" for k, v in q.items()})
    for key, v in q.items():
        assert v <= scale, f"{key}: error is {v:.3g} x its bound"
    return q


# ---- the levels of HipBayesGridSolver(refine=...), restated: the coarse posterior, the half-widths and the chain of calls
def coarse_posterior(model, b, y, grid_axes, noise_sd):
    """Uniform prior over the Cartesian product of `grid_axes` (one array per free parameter), direct cost, known noise: mean and sd."""
    b, y = np.asarray(b, float), np.atleast_2d(np.asarray(y, float))
    theta = np.array(list(itertools.product(*grid_axes))).T
    w = weights(model, theta)
    Ex = np.exp(-b[None, None, :] * theta[RATES[model]][:, :, None])
    s = (w[:, :, None] * Ex).sum(axis=0)
    c = 0.5 * ((y[:, None, :] - s[None]) ** 2).sum(axis=2)
    ell = -c / noise_sd ** 2
    W = np.exp(ell - ell.max(axis=1, keepdims=True))
    W /= W.sum(axis=1, keepdims=True)
    mean = W @ theta.T
    var = (W[:, :, None] * (theta.T[None] - mean[:, None, :]) ** 2).sum(axis=1)
    return mean.T, np.sqrt(var).T  # (n_free, n_vox)


def coarse_cell(values, mean):
    """Width of the coarse grid cell that holds `mean`: the gap between the two neighbouring grid values, the end gap at the ends, 0
    for a one-value axis."""
    values = np.sort(np.asarray(values, float))
    if values.size < 2:
        return np.zeros_like(mean)
    gaps = np.diff(values)
    j = np.clip(np.searchsorted(values, mean, side="right") - 1, 0, gaps.size - 1)
    return gaps[j]


def refine_levels(model, b, y, lo, hi, grid_axes, noise_sd, points=5, levels=1, span=1.0, n_sd=2.0, run=None):
    """The chain of HipBayesGridSolver(refine=...): level 0 on the coarse grid, then `levels` fine grids.  run: the callable that
    evaluates one level (default: `reference`; the GPU test passes api.grid_refine).  Returns the list of per-level dicts."""
    mean, sd = coarse_posterior(model, b, y, grid_axes, noise_sd)
    n_free = len(grid_axes)
    npts = np.array([points if len(grid_axes[k]) > 1 else 1 for k in range(n_free)], np.int32)
    cell = np.stack([coarse_cell(grid_axes[k], mean[k]) for k in range(n_free)])
    out = [dict(mean=mean, sd=sd)]
    for _ in range(levels):
        hw = np.where(npts[:, None] > 1, np.maximum(span * cell, n_sd * sd), 0.0)
        if run is None:
            r = reference(model, b, y, lo, hi, npts, mean, hw, noise_sd=noise_sd, max_eps=1.0)
            res = dict(mean=r["mean"].T, sd=np.sqrt(r["var"]).T, ess=r["ess"], edge_mass=r["edge_mass"].T)
        else:
            res = run(model, b, y, lo, hi, npts, mean, hw, noise_sd=noise_sd)
        lo_b = np.maximum(np.asarray(lo)[:, None], mean - hw)
        hi_b = np.minimum(np.asarray(hi)[:, None], mean + hw)
        cell = np.where(npts[:, None] > 1, np.maximum(hi_b - lo_b, 0.0) / np.maximum(npts[:, None] - 1, 1), 0.0)
        mean, sd = res["mean"], res["sd"]
        out.append(res)
    return out

"""numpy restatement of pnx_curvefit_varpro_f64 (include/pnx.h) for the tests: the unit columns from the stand-in
models of pyneapple_amd/models.py, amplitudes by numpy.linalg.lstsq on the weighted columns, the clip rule, DIRECT costs
0.5 ||w (y - Phi a')||^2 (the library evaluates the expanded form with a stored inverse), the acceptance bound derived from the
rounding of that form, and the acceptance itself."""
from __future__ import annotations

import numpy as np
from grid_start_reference import signals

from pyneapple_amd import api

FREE, REDUCED, S0 = 0, 1, 2
CLASS = {"mono": FREE, "bi_reduced": REDUCED, "bi_s0": S0, "bi_full": FREE, "tri_reduced": REDUCED, "tri_s0": S0, "tri_full": FREE}
U = 2.0 ** -52


RATES = list(np.geomspace(3e-4, 0.3, 8))  # kappa(M) <= 1.3e4 over its ordered pairs and triples at 32 b-values from 0 to 1000
# per-compartment lists for the tri-exponential layouts: kappa(M) <= 520, which keeps the bound (its first-order term grows with
# lambda_1^2 / (lambda_2 lambda_3)) below 1e-3 of the smallest cost at noise sd 0.02; the ordered triples of RATES do not
TRI_RATES = [list(np.geomspace(0.04, 0.3, 4)), list(np.geomspace(4e-3, 0.02, 4)), list(np.geomspace(3e-4, 1.5e-3, 4))]


def case_signals(model, n_vox, n_b=32, seed=3, b_max=1000.0):
    """(b, y): signals of order 1 with additive noise sd 0.02 from rates drawn apart from the dictionaries'."""
    rng = np.random.default_rng(seed)
    b = np.linspace(0.0, b_max, n_b)
    names = api.MODEL_PARAM_NAMES[model]
    truth = np.empty((len(names), n_vox))
    for i, n in enumerate(names):
        if n.startswith("D"):
            truth[i] = {"D": 2e-3, "D1": 0.08, "D2": 7e-3, "D3": 6e-4}[n] * rng.uniform(0.7, 1.4, n_vox)
        else:
            truth[i] = rng.uniform(0.15, 0.4, n_vox) if n.startswith("f") else rng.uniform(0.8, 1.2, n_vox)
    return b, signals(model, b, truth) + 0.02 * rng.standard_normal((n_vox, n_b))


def case_atoms(model):
    """nl_atoms (K, n_atoms): the ordered tuples of RATES (mono: 8, bi: 28), the product of TRI_RATES (64) for three compartments."""
    import itertools

    k = api.VARPRO_COMPARTMENTS[model]
    if k == 3:
        return np.ascontiguousarray(np.array(list(itertools.product(*TRI_RATES))).T)
    return np.ascontiguousarray(np.array([t for t in itertools.product(RATES, repeat=k) if all(a > b for a, b in zip(t, t[1:]))]).T)


def case_box(model, narrow=False):
    """(lo, hi) of every parameter; narrow: the fractions in [0.3, 0.35] and S0 in [0.9, 0.95], so that the truth lies outside."""
    names = api.MODEL_PARAM_NAMES[model]
    lo = np.array([0.0 if not n.startswith("D") else 1e-5 for n in names])
    hi = np.array([1.0 if n.startswith("f") else 10.0 if n == "S0" else 0.5 for n in names])
    if narrow:
        for i, n in enumerate(names):
            if n.startswith("f"):
                lo[i], hi[i] = 0.3, 0.35
            if n == "S0":
                lo[i], hi[i] = 0.9, 0.95
    return lo, hi


def layout(model, fixed_idx=(), t1_mode=0):
    """(K, class, rows of the linear slots among the free parameters, rows of the free non-linear parameters)."""
    names = api.MODEL_PARAM_NAMES[model] + (["T1"] if t1_mode else [])
    free = [i for i in range(len(names)) if i not in fixed_idx]
    lin = [names.index(n) for n in api.varpro_linear_names(model)]
    assert all(i in free for i in lin), "a fixed fraction or S0"
    return api.VARPRO_COMPARTMENTS[model], CLASS[model], [free.index(i) for i in lin], [k for k, i in enumerate(free) if i not in lin]


def columns(model, b, nl_atoms, fixed_idx=(), fixed_vals=None, sigma=None, t1_mode=0, tr=0.0, tm=0.0):
    """Phi (n_atoms, n_b, K): the weighted unit columns of every atom."""
    K, cls, lin_rows, nl_rows = layout(model, fixed_idx, t1_mode)
    nl_atoms = np.asarray(nl_atoms, float)
    n_atoms = nl_atoms.shape[1]
    w = np.ones(len(b)) if sigma is None else 1.0 / np.broadcast_to(np.asarray(sigma, float).reshape(-1), (len(b),))
    Phi = np.empty((n_atoms, len(b), K))
    for j in range(K):
        P = np.zeros((len(lin_rows) + len(nl_rows), n_atoms))
        P[nl_rows] = nl_atoms
        for slot, r in enumerate(lin_rows):
            P[r] = 1.0 if (cls == S0 and slot == K - 1) or slot == j else 0.0
        Phi[:, :, j] = signals(model, b, P, fixed_idx, fixed_vals, t1_mode, tr, tm) * w
    return Phi, w


def _clip_map(cls, K, ah, lo, hi):
    """a_hat (K or K - 1, n_vox) -> (a' (K, n_vox) full amplitude vector, reported linear parameters, clipped (n_vox,), distance of
    a_hat to the nearest clip edge (n_vox,))."""
    if cls == FREE:
        ap = np.clip(ah, lo[:, None], hi[:, None])
        dist = np.minimum(np.abs(ah - lo[:, None]), np.abs(ah - hi[:, None])).min(axis=0)
        return ap, ap, (ap != ah).any(axis=0), dist
    if cls == REDUCED:
        q = np.clip(ah, lo[:, None], hi[:, None])
        dist = np.minimum(np.abs(ah - lo[:, None]), np.abs(ah - hi[:, None])).min(axis=0)
        return np.vstack([q, 1.0 - q.sum(axis=0, keepdims=True)]), q, (q != ah).any(axis=0), dist
    s = ah.sum(axis=0)
    S = np.clip(s, lo[K - 1], hi[K - 1])
    lo_s, hi_s = lo[:K - 1, None] * S, hi[:K - 1, None] * S
    q = np.clip(ah[:K - 1], lo_s, hi_s)
    dist = np.minimum(np.abs(s - lo[K - 1]), np.abs(s - hi[K - 1]))
    if K > 1:
        dist = np.minimum(dist, np.minimum(np.abs(ah[:K - 1] - lo_s), np.abs(ah[:K - 1] - hi_s)).min(axis=0))
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(S > 0, np.clip(q / S, lo[:K - 1, None], hi[:K - 1, None]), lo[:K - 1, None] * np.ones_like(S))
    clipped = (S != s) | (q != ah[:K - 1]).any(axis=0)
    return np.vstack([q, S - q.sum(axis=0, keepdims=True)]), np.vstack([f, S[None]]), clipped, dist


def reference(model, b, y, nl_atoms, lo, hi, fixed_idx=(), fixed_vals=None, sigma=None, t1_mode=0, tr=0.0, tm=0.0, noisy=False):
    """dict(c (n_vox, n_atoms) direct costs, lin (n_vox, n_atoms, n_lin) reported linear parameters, clipped, dist (n_vox, n_atoms),
    tol (n_vox,), ptol (n_vox, n_atoms) the bound's parameter form, finite, kappa (n_atoms,), rows).
    noisy: assert the condition that keeps the bound honest, tol_v <= 1e-3 min_g c[v, g]."""
    b, y = np.asarray(b, float), np.atleast_2d(np.asarray(y, float))
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    K, cls, lin_rows, nl_rows = layout(model, fixed_idx, t1_mode)
    Phi, w = columns(model, b, nl_atoms, fixed_idx, fixed_vals, sigma, t1_mode, tr, tm)
    n_atoms, n_b = Phi.shape[0], len(b)
    finite = np.isfinite(y * w).all(axis=1)
    yw = np.where(finite[:, None], y * w, 0.0)  # (n_vox, n_b)
    n_vox, n_lin = len(yw), len(lin_rows)
    llo, lhi = lo[lin_rows], hi[lin_rows]
    c = np.empty((n_vox, n_atoms))
    lin = np.empty((n_vox, n_atoms, n_lin))
    clipped = np.empty((n_vox, n_atoms), bool)
    dist, tol, ptol = (np.empty((n_vox, n_atoms)) for _ in range(3))
    kappa = np.empty(n_atoms)
    ynorm = np.sqrt((yw * yw).sum(axis=1))
    L = K + 1.0  # Lipschitz constant of the clip map (S0 class: S moves the fraction bounds)
    for g in range(n_atoms):
        P = Phi[g]
        if cls == REDUCED:  # the difference system: columns phi_j - phi_K, data y - phi_K
            A, rhs, extra = P[:, :K - 1] - P[:, K - 1:], yw.T - P[:, K - 1:], np.linalg.norm(P[:, K - 1])
        else:
            A, rhs, extra = P, yw.T, 0.0
        ah = np.linalg.lstsq(A, rhs, rcond=None)[0]  # (cols, n_vox)
        ap, rep, clipped[:, g], dist[:, g] = _clip_map(cls, K, ah, llo, lhi)
        r = yw.T - P @ ap
        c[:, g] = 0.5 * (r * r).sum(axis=0)
        lin[:, g] = rep.T
        # the bound: rounding of the expanded form at a'; the error of a_hat (dot products through M^-1, the stored
        # inverse) enters the cost to first order only where a clip is active (the gradient M (a' - a_hat) is zero otherwise)
        N = A.T @ A
        sv = np.linalg.svd(A, compute_uv=False)
        kappa[g] = np.linalg.cond(P) ** 2  # kappa(M)
        phimax = np.sqrt((P * P).sum(axis=0).max())
        cn = np.linalg.norm(A.T @ rhs, axis=0)
        # error of a_hat: the K dot products through M^-1; the cofactors of the stored inverse (products of two entries, K = 3
        # only) applied to c; the relative error of its determinant (K terms of K factors) applied to a_hat
        lam = sv ** 2
        adj = 8 * lam[0] / (lam[1] * lam[2]) * cn if len(lam) == 3 else 0.0
        d_a = U * (n_b * np.sqrt(K) * (ynorm + extra) * 2 * phimax / lam[-1] + adj + 8 * lam[0] ** len(lam) / lam.prod() * np.linalg.norm(ah, axis=0))
        grad = np.linalg.norm(N @ (ap[:A.shape[1]] - ah), axis=0)
        a1 = np.abs(ap).sum(axis=0)
        tol[:, g] = 4 * n_b * U * (ynorm ** 2 + a1 ** 2 * phimax ** 2) + 4 * grad * L * d_a + sv[0] ** 2 * (L * d_a) ** 2
        ptol[:, g] = L * d_a
    tol_v = tol.max(axis=1)
    if noisy:
        assert (tol_v[finite] <= 1e-3 * c[finite].min(axis=1)).all(), "the bound is not small against the costs: no honest comparison"
    return dict(c=c, lin=lin, clipped=clipped, dist=dist, tol=tol_v, ptol=ptol, finite=finite, kappa=kappa, lin_rows=lin_rows, nl_rows=nl_rows,
                K=K, cls=cls)


def accept(ref, got, nl_atoms, fallback=None):
    """The acceptance of the issue, per voxel, against a result dict(params, atom, cost, clipped) of numpy arrays."""
    c, tol, fin = ref["c"], ref["tol"], ref["finite"]
    best, cost, params, clp = got["atom"], got["cost"], got["params"], got["clipped"]
    n_atoms = c.shape[1]
    assert best.dtype == np.int32 and best.shape == (len(c),) and clp.dtype == np.int8
    assert ((best[fin] >= 0) & (best[fin] < n_atoms)).all(), "a padded atom or no atom won"
    idx = np.flatnonzero(fin)
    bi = best[idx]
    cb = c[idx, bi]
    excess = cb - c[idx].min(axis=1)
    assert (excess <= tol[idx]).all(), f"chosen atom worse than the best by {(excess / tol[idx]).max():.3g} tol"
    dev = np.abs(cost[idx] - cb)
    assert (dev <= tol[idx]).all(), f"reported cost off by {(dev / tol[idx]).max():.3g} tol"
    bits = lambda x: np.ascontiguousarray(x, np.float64).view(np.uint64)
    nl_atoms = np.asarray(nl_atoms, float)
    assert (bits(params[ref["nl_rows"]][:, idx]) == bits(nl_atoms[:, bi])).all(), "the non-linear parameters are not a copy of the atom"
    # the bound's parameter form: |a'_kernel - a'_ref| <= L d_a; a fraction of the S0 class is a quotient by S
    want, pt = ref["lin"][idx, bi], ref["ptol"][idx, bi]
    have = params[ref["lin_rows"]][:, idx].T
    bound = np.repeat(pt[:, None], want.shape[1], axis=1) + 4 * U * np.abs(want)
    if ref["cls"] == S0 and ref["K"] > 1:
        S = np.maximum(want[:, -1:], 1e-300)
        bound[:, :-1] = 2 * pt[:, None] / S * (1 + np.abs(want[:, :-1])) + 4 * U * np.abs(want[:, :-1])
        bound[:, -1] = ref["K"] * pt + 4 * U * np.abs(want[:, -1])
    assert (np.abs(have - want) <= bound).all(), f"parameters off by {(np.abs(have - want) / bound).max():.3g} of their bound"
    sure = ref["dist"][idx, bi] > (ref["K"] + 1) * pt
    assert (clp[idx][sure].astype(bool) == ref["clipped"][idx, bi][sure]).all(), "clipped disagrees away from the clip edge"
    if (~fin).any():
        assert (best[~fin] == -1).all() and np.isnan(cost[~fin]).all() and (clp[~fin] == 0).all()
        if fallback is not None:
            assert (bits(params[:, ~fin]) == bits(np.repeat(np.asarray(fallback, float)[:, None], (~fin).sum(), axis=1))).all()

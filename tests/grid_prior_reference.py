"""numpy restatement of pnx_curvefit_grid_prior_em_f64 (include/pnx.h) for the tests: the EM update of the prior
over a dictionary, built on the l_g, eps_v and finite flags of tests/grid_posterior_reference.py (imported, not restated), and
the acceptance bound of ONE update, derived in DESIGN.md 4.1j:

    eps_v    the posterior reference's bound on the error of one l_g (taken under the uniform prior) + 8 2^-52 max_g |log_prior_g|
    E        = expm1(2 max_v eps_v)            what a normalised weight W_vg moves by
    gamma_G  = 4 (G + 16) 2^-52                the sum over G atoms inside L_v
    gamma_N  = 4 (N + 16) 2^-52                the sum over N voxels
    rel      = E + gamma_G + gamma_N
    |S_g - S_ref|       <= rel S_ref + N 1e-300
    |lp_next - ref|     <= log1p(rel)                              for atoms with S_ref > 1e-290; below that -inf or any value under
                                                                   log(1e-290 / N) is accepted
    |sum_v L_v - ref|   <= sum_v (eps_v + gamma_G + 2^-52 (|L_v| + |log sum exp log_prior|)) + gamma_N sum_v |L_v|

A perturbation eta of log_prior moves the next log_prior by at most 2 eta (the weights move by e^{+-2 eta}), so after t library
updates the distance to an all-numpy run is at most (2^t - 1) single-step bounds: used for t <= 3 only.  Longer runs are checked
step by step against the library's own previous prior."""
from __future__ import annotations

import numpy as np
from grid_posterior_reference import U, reference


def normalise(log_prior, n_atoms):
    """The start of the EM: log_prior - log sum exp(log_prior); None is the uniform prior."""
    lp = np.zeros(n_atoms) if log_prior is None else np.asarray(log_prior, float)
    top = lp.max()
    return lp - (top + np.log(np.exp(lp - top).sum()))


def likelihoods(model, b, y, atoms, lo, hi, noise_sd=0.0, project=False, **kw):
    """(l0 (n_vox, G) = l_g under log_prior = 0, eps0 (n_vox,), finite (n_vox,)) from the posterior reference."""
    ref = reference(model, b, y, atoms, lo, hi, log_prior=None, noise_sd=noise_sd, project=project, **kw)
    return ref["l"], ref["eps"], ref["finite"]


def _voxel_sums(l0, lp, finite):
    adm = lp > -np.inf
    ell = l0[finite][:, adm] + lp[adm][None, :]
    m = ell.max(axis=1)
    w = np.exp(ell - m[:, None])
    s = w.sum(axis=1)
    return adm, w / s[:, None], m + np.log(s)


def em_step(l0, lp, finite, alpha=0.0):
    """One update from the normalised log prior lp: (S_g (G,), lp_next (G,), sum over the finite voxels of L_v under lp)."""
    lp = np.asarray(lp, float)
    adm, W, L = _voxel_sums(l0, lp, finite)
    S = np.zeros(lp.shape)
    S[adm] = W.sum(axis=0)
    n = int(finite.sum())
    lp_next = np.full(lp.shape, -np.inf)
    if n == 0:
        return S, lp.copy(), 0.0
    pi = (S[adm] + alpha) / (n + alpha * adm.sum())
    with np.errstate(divide="ignore"):
        lp_next[adm] = np.log(pi)
    return S, lp_next, float(L.sum())


def em(l0, lp, finite, alpha=0.0, n_iter=1):
    """n_iter updates from the normalised start lp: (log prior, loglik (n_iter + 1,) as the library reports it with rel_tol = 0)."""
    trace = []
    for _ in range(n_iter):
        _, lp, ll = em_step(l0, lp, finite, alpha)
        trace.append(ll)
    trace.append(em_step(l0, lp, finite, alpha)[2])
    return lp, np.array(trace)


def step_bounds(l0, lp, eps0, finite, S_ref):
    """dict(rel, S (G,), lp, loglik) of one update from lp, per the module docstring."""
    lp = np.asarray(lp, float)
    n_vox, G = l0.shape
    n = int(finite.sum())
    adm, _, L = _voxel_sums(l0, lp, finite)
    eps = eps0[finite] + 8 * U * np.abs(lp[adm]).max()
    gamma_g, gamma_n = 4 * (G + 16) * U, 4 * (n + 16) * U
    rel = float(np.expm1(2 * eps.max())) + gamma_g + gamma_n if n else 0.0
    top = lp[adm].max()
    lpn = top + np.log(np.exp(lp[adm] - top).sum())
    return dict(rel=rel, S=rel * S_ref + n * 1e-300, lp=float(np.log1p(rel)),
                loglik=float((eps + gamma_g + U * (np.abs(L) + abs(lpn))).sum() + gamma_n * np.abs(L).sum()))


def accept_step(lp_got, lp_before, lp_ref, S_ref, n, bound_lp, alpha=0.0, scale=1.0):
    """log_prior after an update from lp_before against the reference's lp_ref: an excluded atom stays at -inf, an atom whose
    weight sum is above 1e-290 is held to `scale` bounds, one below it is -inf or under log(1e-290 / n).  Returns the largest
    error-to-bound ratio."""
    lp_got, lp_ref = np.asarray(lp_got), np.asarray(lp_ref)
    assert lp_got.shape == lp_ref.shape and not np.isnan(lp_got).any() and (lp_got < np.inf).all()
    adm = np.asarray(lp_before) > -np.inf
    assert (lp_got[~adm] == -np.inf).all(), "an excluded atom came back"
    heavy = adm & (S_ref + alpha > 1e-290)
    light = adm & ~heavy
    assert ((lp_got[light] == -np.inf) | (lp_got[light] <= np.log(1e-290 / max(n, 1)) + 1e-9)).all()
    assert np.isfinite(lp_got[heavy]).all()
    q = float((np.abs(lp_got[heavy] - lp_ref[heavy]) / bound_lp).max()) if heavy.any() else 0.0
    assert q <= scale, f"log_prior after the update: error is {q:.3g} x its bound ({scale:g} allowed)"
    return q


def population(n_vox, seed=0, noise=0.05, n_b=16):
    """The narrow IVIM population of DESIGN.md 4.1j: bi_s0 with S0 = 1, f1 ~ N(0.15, 0.03), D1 and D2 log-normal about 0.05 and
    0.0012 (sd 0.2 of the logarithm), additive Gaussian noise; and a grid of 8 x 6 x 8 = 384 atoms over far wider ranges, S0 projected.
    Returns (b, y, truth (4, n_vox), grid dict, atoms (4, 384), lo, hi)."""
    import itertools

    from grid_start_reference import signals

    rng = np.random.default_rng(seed)
    b = np.array([0, 5, 10, 20, 30, 50, 75, 100, 150, 200, 300, 400, 500, 600, 700, 800], float)[:n_b]
    truth = np.stack([np.clip(rng.normal(0.15, 0.03, n_vox), 0.02, 0.5), 0.05 * np.exp(0.2 * rng.standard_normal(n_vox)),
                      0.0012 * np.exp(0.2 * rng.standard_normal(n_vox)), np.ones(n_vox)])
    y = np.ascontiguousarray(signals("bi_s0", b, truth) + noise * rng.standard_normal((n_vox, len(b))))
    grid = {"f1": np.linspace(0.04, 0.46, 8), "D1": np.geomspace(0.01, 0.3, 6), "D2": np.geomspace(4e-4, 3e-3, 8)}
    cols = list(itertools.product(grid["f1"], grid["D1"], grid["D2"]))
    atoms = np.ascontiguousarray(np.array([[f, d1, d2, 1.0] for f, d1, d2 in cols]).T)
    lo, hi = np.array([0.0, 5e-3, 1e-4, 0.2]), np.array([1.0, 0.5, 5e-3, 5.0])
    return b, y, truth, grid, atoms, lo, hi

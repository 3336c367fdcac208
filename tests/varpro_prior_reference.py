"""numpy restatement of pnx_curvefit_varpro_prior_em_f64 (include/pnx.h) for the tests: the EM update of the prior
over a variable-projection dictionary.  l_g (the Occam term plus the likelihood term: `reference(..., log_prior=None)`), eps_v and
the finite flags come from tests/varpro_posterior_reference.py; the update, the start, the bounds of ONE update and their
acceptance are tests/grid_prior_reference.py's, imported, not restated:

    eps_v    varpro_posterior_reference's bound on the error of one l_g (it holds eps_ld, the rounding of the determinant) under the
             uniform prior, + 8 2^-52 max_g |log_prior_g| (step_bounds adds it)
    E        = expm1(2 max_v eps_v);  gamma_G = 4 (G + 16) 2^-52;  gamma_N = 4 (N + 16) 2^-52
    |S_g - S_ref|       <= (E + gamma_G + gamma_N) S_ref + N 1e-300
    |lp_next - ref|     <= log1p(E + gamma_G + gamma_N)                    for atoms with S_ref > 1e-290
    |sum_v L_v - ref|   <= sum_v bound_log_evidence_v + gamma_N sum_v |L_v|
    t library updates lie within (2^t - 1) single-step bounds of an all-numpy run: used for t <= 3.

The library forms lw_g = log pi_g + occ_g in one addition where the reference adds log pi_g to l_g; that rounding, 2^-52 |lw_g|,
is inside the 8 2^-52 max_g |l_g| of eps_v.

The narrow population of `population` and the reference's own gain on it (`reference_gain`) are chosen and recorded here, on the
CPU; tests/test_gpu_varpro_prior.py holds the library to them."""
from __future__ import annotations

import numpy as np
from grid_prior_reference import accept_step, em, em_step, normalise, step_bounds  # noqa: F401  (re-exported for the tests)
from varpro_posterior_reference import reference


def likelihoods(model, b, y, nl_atoms, lo, hi, noise_sd=0.0, marginal=True, max_eps=1e-6, **kw):
    """(l0 (n_vox, G) = occ_g + the likelihood term, eps0 (n_vox,), finite (n_vox,)) from the posterior reference under log_prior =
    None (a `log_prior` among the keywords is the EM's start, not part of l0: dropped); the reference asserts eps_v <= max_eps on
    every finite voxel."""
    kw = {k: v for k, v in kw.items() if k != "log_prior"}
    ref =reference(model, b, y, nl_atoms, lo, hi, log_prior=None, noise_sd=noise_sd, marginal=marginal, max_eps=max_eps, **kw)
    return ref["l"], ref["eps"], ref["finite"]


def population(n_vox, seed=0, noise=0.05):
    """A population narrower than the dictionary, 4.1j's idea on a bi_s0 variable-projection dictionary: S0 = 1, f1 ~ N(0.15, 0.03),
    D1 and D2 log-normal about 0.05 and 0.0012 (sd 0.2 of the logarithm), additive Gaussian noise, 16 b-values; the dictionary is
    the ordered pairs of 14 rates over three decades (91 atoms).  Returns (b, y, truth (4, n_vox), nl_atoms (2, 91), lo, hi)."""
    import itertools

    from grid_start_reference import signals

    rng = np.random.default_rng(seed)
    b = np.array([0, 5, 10, 20, 30, 50, 75, 100, 150, 200, 300, 400, 500, 600, 700, 800], float)
    truth = np.stack([np.clip(rng.normal(0.15, 0.03, n_vox), 0.02, 0.5), 0.05 * np.exp(0.2 * rng.standard_normal(n_vox)),
                      0.0012 * np.exp(0.2 * rng.standard_normal(n_vox)), np.ones(n_vox)])
    y = np.ascontiguousarray(signals("bi_s0", b, truth) + noise * rng.standard_normal((n_vox, len(b))))
    rates = np.geomspace(3e-4, 0.3, 14)
    atoms = np.ascontiguousarray(np.array([t for t in itertools.product(rates, repeat=2) if t[0] > t[1]]).T)
    lo, hi = np.array([0.0, 1e-5, 1e-5, 0.0]), np.array([1.0, 0.5, 0.5, 10.0])
    return b, y, truth, atoms, lo, hi


def posterior_mean(l0, lp, lin, nl_atoms, lin_rows, nl_rows):
    """Posterior mean (n_vox, n_free) under the log prior lp from the reference's l0 and per-pair linear parameters."""
    ell = l0 + lp[None, :]
    W = np.exp(ell - ell.max(axis=1, keepdims=True))
    W /= W.sum(axis=1, keepdims=True)
    mean = np.empty((l0.shape[0], len(lin_rows) + len(nl_rows)))
    mean[:, nl_rows] = W @ nl_atoms.T
    mean[:, lin_rows] = (W[:, :, None] * lin).sum(axis=1)
    return mean


def reference_gain(n_vox=1000, seed=0, noise_sd=0.05, n_iter=30, max_eps=1e-3):
    """The ratio learned / uniform of the median |error| of the posterior mean of (f1, D1, D2) that numpy alone reaches on
    `population`: the numpy EM (n_iter updates) on varpro_posterior_reference's l_g.  noise_sd = 0 marginalises the noise."""
    b, y, truth, atoms, lo, hi = population(n_vox, seed)
    ref = reference("bi_s0", b, y, atoms, lo, hi, log_prior=None, noise_sd=noise_sd, marginal=True, max_eps=max_eps)
    l0, fin = ref["l"], ref["finite"]
    lp0 = normalise(None, atoms.shape[1])
    lp, _ = em(l0, lp0, fin, 0.0, n_iter)
    err = lambda m: np.median(np.abs(m[:, :3] - truth[:3].T), axis=0)
    flat = err(posterior_mean(l0, lp0, ref["lin"], atoms, ref["lin_rows"], ref["nl_rows"]))
    learned = err(posterior_mean(l0, np.where(np.isfinite(lp), lp, -1e300), ref["lin"], atoms, ref["lin_rows"], ref["nl_rows"]))
    return learned / flat, flat, learned

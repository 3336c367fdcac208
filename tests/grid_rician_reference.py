"""numpy restatement of pnx_curvefit_grid_posterior_rician_f64 (include/pnx.h) for the tests.  `rician_posterior`
is tests/grid_posterior_reference.py's `reference` (known noise, no projection) with the Rician correction added to l in the
header's order of operations, h = log(scipy.special.ive(0, z)):

    z_vgi = |(y_vi s_gi) inv|, inv = 1 / noise_sd^2;   C_g(v) = sum_i h(z_vgi), i ascending in one chain;   l = (lp - c / sd^2) + C
    log_evidence = L - log sum exp(lp) + sum_i log(y_vi inv)

Its dict has the keys of that reference, so its `accept` and `ratios` judge a result; the bounds are that module's with one more
term in eps_v, the rounding of one l_g.  With U = 2^-52, E_h = 4.5 (csrc/pnx_bessel.hpp; test_grid_rician_host.py asserts SciPy
inside it too) and H = max(max_gi |h(z_vgi)|, 1), per term of the sum: the device's h is off by at most E_h U H, SciPy's by as
much; the two roundings of z move h by |z h'(z)| U <= U (z (1 - I1 / I0) stays below 0.61); and a chain of n_b additions rounds
by at most U / 2 times the sum of the magnitudes of its partial sums, (U / 2) H n_b (n_b - 1) / 2, on either side.  The last addition
l = lg + C is one more rounding of l:

    eps_v += (n_b (2 E_h + 1) + n_b (n_b - 1) / 2) U H + 2 U max_g |l_g|

and the evidence's constant K_v = sum_i log(y_i inv) adds (n_b + 2) U sum_i |log(y_i inv)| to bound_log_evidence (a log to 1 ulp on
either side, the product inside it, the additions).  Nothing here is tuned on the device.

A voxel with a negative entry counts as non-finite.  A zero entry makes log_evidence -inf on both sides: `accept` compares those
voxels' evidence by sign and the rest of their outputs as usual."""
from __future__ import annotations

import numpy as np
from scipy.special import ive

import grid_posterior_reference as P
from grid_start_reference import reference as grid_reference, signals

U = 2.0 ** -52
E_H = 4.5  # kLogI0eBound of csrc/pnx_bessel.hpp


def log_i0e(z):
    return np.log(ive(0, z))


def reference_h(z):
    """h(z) for the comparison of log_i0e: log(ive(0, z)) up to 1e3, beyond it -log(2 pi z) / 2 + log of the asymptotic series in
    1 / (8 z) to five terms in numpy.longdouble (the sixth is below 1e-20 there)."""
    z = np.asarray(z, float)
    with np.errstate(divide="ignore", invalid="ignore"):
        zl = z.astype(np.longdouble)
        x = 1 / (8 * zl)
        series = 1 + x * (1 + x * (np.longdouble(9) / 2) * (1 + x * (np.longdouble(25) / 3) * (1 + x * (np.longdouble(49) / 4) * (1 + x * np.longdouble(81) / 5))))
        asym = (-np.log(2 * np.longdouble(np.pi) * zl) / 2 + np.log(series)).astype(float)
        small = log_i0e(z)
    return np.where(z > 1e3, asym, small)


def correction(y, S, noise_sd, chunk=256):
    """C (n_vox, n_atoms) = sum_i h(|(y_vi s_gi) inv|) with i ascending, and H (n_vox,) = max(max_gi |h|, 1)."""
    inv = 1.0 / (noise_sd * noise_sd)
    C = np.zeros((len(y), len(S)))
    H = np.ones(len(y))
    for v0 in range(0, len(y), chunk):
        yv = y[v0:v0 + chunk]
        acc = np.zeros((len(yv), len(S)))
        for i in range(y.shape[1]):
            h = log_i0e(np.abs((yv[:, i, None] * S[None, :, i]) * inv))
            acc = acc + h
            H[v0:v0 + chunk] = np.maximum(H[v0:v0 + chunk], np.abs(h).max(axis=1))
        C[v0:v0 + chunk] = acc
    return C, H


def rician_posterior(model, b, y, atoms, lo, hi, noise_sd, log_prior=None, max_eps=1e-6, extra_eps=0.0, **kw):
    atoms = np.array(atoms, float)
    y = np.atleast_2d(np.asarray(y, float))
    assert noise_sd > 0 and np.isfinite(noise_sd)
    gs = grid_reference(model, b, y, atoms, lo, hi, **kw)
    with np.errstate(invalid="ignore"):
        fin = gs["finite"] & ~(y < 0).any(axis=1)
    c, tol = gs["c"], gs["tol"]
    n_vox, G = c.shape
    n_b = y.shape[1]
    yz = np.where(fin[:, None], y, 0.0)
    S = signals(model, b, atoms, kw.get("fixed_idx", ()), kw.get("fixed_vals"), kw.get("t1_mode", 0), kw.get("tr", 0.0), kw.get("tm", 0.0))
    C, H = correction(yz, S, noise_sd)
    lp = np.zeros(G) if log_prior is None else np.asarray(log_prior, float)
    adm = lp > -np.inf
    assert adm.any() and not np.isnan(lp).any()
    inv = 1.0 / (noise_sd * noise_sd)
    ell = (lp[None, :] - c / noise_sd ** 2) + C
    ell[:, ~adm] = -np.inf
    ell[~fin] = np.where(adm, 0.0, -np.inf)[None]
    lmax = np.abs(ell[:, adm]).max(axis=1)
    eps = tol / noise_sd ** 2 + 8 * U * lmax + (n_b * (2 * E_H + 1) + n_b * (n_b - 1) / 2) * U * H + 2 * U * lmax + extra_eps
    assert (eps[fin] <= max_eps).all(), f"precondition: eps_v = {eps[fin].max():.3g} > {max_eps:g}"
    m = ell.max(axis=1)
    w = np.exp(ell - m[:, None])
    s = w.sum(axis=1)
    L = m + np.log(s)
    W = w / s[:, None]
    theta = np.repeat(atoms[None], n_vox, axis=0)
    mean = (W[:, None, :] * theta).sum(axis=2)
    var = (W[:, None, :] * (theta - mean[:, :, None]) ** 2).sum(axis=2)
    ess = 1.0 / (W * W).sum(axis=1)
    lpn = np.log(np.exp(lp[adm] - lp[adm].max()).sum()) + lp[adm].max()
    with np.errstate(divide="ignore"):
        logs = np.log(yz * inv)
    K = logs.sum(axis=1)
    with np.errstate(invalid="ignore"):
        Kabs = np.where(np.isfinite(K), np.abs(logs).sum(axis=1), 0.0)
    ta = theta[:, :, adm]
    R = ta.max(axis=2) - ta.min(axis=2)
    A = np.abs(ta).max(axis=2)
    gamma = 4 * (G + 16) * U
    E = np.expm1(2 * eps)
    return dict(mean=mean, var=var, log_evidence=(L - lpn) + K, ess=ess, map_atom=ell.argmax(axis=1), l=ell, eps=eps, finite=fin, s0_row=None,
                amp=None, bound_mean=E[:, None] * R + gamma * R + U * A, bound_var=3 * (E[:, None] * R * R + gamma * R * R),
                bound_log_evidence=eps + gamma + U * (np.abs(L) + abs(lpn)) + (n_b + 2) * U * Kabs + 2 * U * np.where(np.isfinite(K), np.abs(K), 0.0),
                bound_ess=4 * (E + gamma) * ess, C=C, K=K)


def accept(ref, got, atoms, scale=1.0):
    """grid_posterior_reference.accept on every voxel; where a zero entry makes the reference's evidence -inf the result's must be
    -inf too, and the voxel's other outputs are judged as usual."""
    zero = ref["finite"] & (ref["log_evidence"] == -np.inf)
    assert (got["log_evidence"][zero] == -np.inf).all(), "a zero entry: log_evidence must be -inf"
    got2, ref2 = dict(got), dict(ref)
    got2["log_evidence"] = np.where(zero, 0.0, got["log_evidence"])
    ref2["log_evidence"] = np.where(zero, 0.0, ref["log_evidence"])
    ref2["bound_log_evidence"] = np.where(zero, 1.0, ref["bound_log_evidence"])
    return P.accept(ref2, got2, atoms, scale)

"""numpy restatement of pnx_curvefit_varpro_marginals_f64 (include/pnx.h) for the tests: the marginal posterior of
every free rate (and a free T1) over its grid values, the quantiles and the geometric mean from it, built on the W, l_g, eps_v and
finite flags of tests/varpro_posterior_reference.py (imported, not restated; TWO passes: the maximum, then the sums), the sums per
bin and the quantile acceptance of tests/grid_marginal_reference.py (imported), and the bounds, derived here and in DESIGN.md 4.1l:

    eps_v    the posterior reference's bound on the error of one l_g: a normalised weight moves by e^{+-2 eps_v}
    E_v      = expm1(2 eps_v)
    gamma_G  = 4 (G + 16) 2^-52     a sum over at most G atoms, in any order.  The kernel's numerator (a bin's sum) and its
             denominator (the sum of all weights) are one such sum each; each has gone through at most G / 16 rescales by
             alpha = exp(m - m') of one rounding each (G / 16 2^-53 < gamma_G / 128), the weights are exp's of a difference whose
             rounding eps_v already counts (8 2^-52 max |l_g|), and the quotient is one rounding: a third gamma_G holds all of that.
    rel_v    = E_v + 3 gamma_G
    |marginal - ref| <= rel_v ref + 1e-300          per bin, and |sum_j marginal - 1| <= rel_v + 1e-300 per parameter
    quantile: grid_marginal_reference.accept's rule -- the reported bin is accepted when the reference's running sum can cross the
             level there within the running sum of the bins' bounds
    log_evidence: the posterior reference's bound + gamma_G (the rescales of the sum of weights)
    geo_mean: with x_j = log v_j, S = sum_j P_j x_j / sum_j P_j.  P_j = ref_j (1 + d_j), |d_j| <= rel_v, so S - x_mid is a
             weighted mean of (x_j - x_mid) whose weights move by at most (1 + rel) / (1 - rel):  |S - S_ref| <= 2 rel / (1 - rel) R,
             R = max_j |x_j - x_mid|, x_mid = (min x + max x) / 2.  The kernel sums P_j x_j uncentred over n_bins terms (gamma_B
             max |x_j|), takes one quotient, one exp, and the test one log (8 2^-52 max |x_j| holds them):
    |log geo_mean - S_ref| <= 2 rel_v / (1 - rel_v) R + (gamma_B + 8 2^-52) max_j |x_j|,   gamma_B = 4 (B + 16) 2^-52
"""
from __future__ import annotations

import numpy as np
from grid_marginal_reference import accept as accept_marginals
from grid_marginal_reference import marginals, quantile_bins
from varpro_posterior_reference import U
from varpro_posterior_reference import reference as posterior_reference


def full_bins(n_free, nl_rows, nl_atoms):
    """(n_bins (n_free,), bin_of (n_free, G), bin_value) over ALL free parameters from np.unique per row of nl_atoms: what
    api.varpro_marginals derives when no binning is passed (restated: the test of the derivation compares the two)."""
    nl_atoms = np.asarray(nl_atoms, float)
    n_bins, bin_of, values = np.zeros(n_free, np.int32), np.zeros((n_free, nl_atoms.shape[1]), np.int32), []
    for row, k in enumerate(nl_rows):
        val, inv = np.unique(nl_atoms[row], return_inverse=True)
        n_bins[k], bin_of[k] = val.size, inv.reshape(-1)
        values.append(val)
    return n_bins, bin_of, np.concatenate(values)


def geo_reference(marg, rel, n_bins, bin_value):
    """(S_ref (n_vox, n_free), bound (n_vox, n_free)): NaN for a parameter without bins or with a bin value <= 0."""
    n_vox, n_free = marg.shape[0], len(n_bins)
    S, bound = np.full((n_vox, n_free), np.nan), np.full((n_vox, n_free), np.nan)
    B, off = int(np.sum(n_bins)), 0
    for k, nb in enumerate(n_bins):
        val = np.asarray(bin_value[off:off + nb], float)
        if nb and (val > 0).all():
            x = np.log(val)
            p = marg[:, off:off + nb]
            S[:, k] = (p * x).sum(axis=1) / p.sum(axis=1)
            R = 0.5 * (x.max() - x.min())
            bound[:, k] = 2 * rel / (1 - rel) * R + (4 * (B + 16) + 8) * U * np.abs(x).max()
        off += nb
    return S, bound


def reference(model, b, y, nl_atoms, lo, hi, n_bins, bin_of, bin_value, probs=(), log_prior=None, noise_sd=0.0, marginal=True, max_eps=1e-6,
              **kw):
    """grid_marginal_reference.reference's dict (marginal, bound, rel, quantile_bin, log_evidence, bound_log_evidence, finite, empty,
    post) plus geo (n_vox, n_free) = S_ref and bound_geo."""
    post = posterior_reference(model, b, y, nl_atoms, lo, hi, log_prior=log_prior, noise_sd=noise_sd, marginal=marginal, max_eps=max_eps, **kw)
    G = post["l"].shape[1]
    marg = marginals(post["W"], n_bins, bin_of)
    gamma = 4 * (G + 16) * U
    rel = np.expm1(2 * post["eps"]) + 3 * gamma
    adm = np.ones(G, bool) if log_prior is None else np.asarray(log_prior, float) > -np.inf
    empty = np.concatenate([[not (adm & (np.asarray(bin_of[k]) == j)).any() for j in range(nb)] for k, nb in enumerate(n_bins) if nb])
    qbin, off = {}, 0
    for k, nb in enumerate(n_bins):
        if nb:
            qbin[k] = quantile_bins(np.cumsum(marg[:, off:off + nb], axis=1), probs)
        off += nb
    geo, bound_geo = geo_reference(marg, rel, n_bins, bin_value)
    return dict(marginal=marg, bound=rel[:, None] * marg + 1e-300, rel=rel, quantile_bin=qbin, log_evidence=post["log_evidence"],
                bound_log_evidence=post["bound_log_evidence"] + gamma, finite=post["finite"], empty=np.asarray(empty, bool), post=post,
                geo=geo, bound_geo=bound_geo)


def accept(ref, got, n_bins, bin_value, probs):
    """The acceptance of a result dict of api.varpro_marginals on EVERY voxel; returns the largest error-to-bound ratio per output."""
    fin = ref["finite"]
    worst = accept_marginals(ref, got, n_bins, bin_value, probs)  # every bin, the sums to 1, the exact zeros, the quantiles, the evidence
    assert sorted(got["geo_mean"]) == [k for k, nb in enumerate(n_bins) if nb]
    worst_geo = 0.0
    for k, g in got["geo_mean"].items():
        assert g.shape == (len(fin),) and np.isnan(g[~fin]).all()
        if np.isnan(ref["geo"][fin, k]).any():
            assert np.isnan(g[fin]).all(), f"parameter {k}: a geometric mean over a grid value <= 0"
            continue
        assert (g[fin] > 0).all()
        err = np.abs(np.log(g[fin]) - ref["geo"][fin, k])
        assert (err <= ref["bound_geo"][fin, k]).all(), f"parameter {k}: log geo_mean is {(err / ref['bound_geo'][fin, k]).max():.3g} x its bound off"
        worst_geo = max(worst_geo, float((err / ref["bound_geo"][fin, k]).max()) if err.size else 0.0)
    err = np.abs(got["log_evidence"][fin] - ref["log_evidence"][fin])
    q = {"marginal": worst, "geo_mean": worst_geo, "log_evidence": float((err / ref["bound_log_evidence"][fin]).max()) if err.size else 0.0}
    print("error / bound:", {k: f"{v:.3g}" for k, v in q.items()})
    return q


def running_maximum(ell, n_bins, bin_of, tile=16):
    """The kernel's arithmetic restated in numpy for ONE call: l (n_vox, G) taken tile by tile (16 atoms), the running maximum m, the
    rescale alpha = exp(m - m') of the sums when it moves (guarded: (-inf) - (-inf) never reaches exp), the weights exp(l - m'),
    the bins' sums and the sum of all weights; marginal = sums / total, L = m + log total.  Returns (marginal (n_vox, B), L)."""
    n_vox, G = ell.shape
    B = int(np.sum(n_bins))
    ind = np.zeros((G, B))
    off = 0
    for k, nb in enumerate(n_bins):
        if nb:
            ind[np.arange(G), off + np.asarray(bin_of[k])] = 1.0
        off += nb
    m, sw, acc = np.full(n_vox, -np.inf), np.zeros(n_vox), np.zeros((n_vox, B))
    for g0 in range(0, G, tile):
        lt = ell[:, g0:g0 + tile]
        mn = np.maximum(m, lt.max(axis=1))
        with np.errstate(invalid="ignore"):
            alpha = np.where(mn == m, 1.0, np.exp(m - mn))
            w = np.where(lt > -np.inf, np.exp(lt - mn[:, None]), 0.0)
        sw, acc, m = sw * alpha + w.sum(axis=1), acc * alpha[:, None] + w @ ind[g0:g0 + tile], mn
    return acc / sw[:, None], m + np.log(sw)

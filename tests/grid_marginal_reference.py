"""numpy restatement of pnx_curvefit_grid_marginals_f64 (include/pnx.h) for the tests: the marginal posterior of
every free parameter over its grid values and the quantiles from it, built on the l_g, eps_v and finite flags of
tests/grid_posterior_reference.py (imported, not restated), and the acceptance, derived as in DESIGN.md 4.1j:

    eps_v    the posterior reference's bound on the error of one l_g
    E_v      = expm1(2 eps_v)                   what a normalised weight W_vg moves by
    gamma_G  = 4 (G + 16) 2^-52                 a sum over at most G atoms, in any order
    |marginal - ref| <= (E_v + gamma_G) ref + 1e-300          per bin, and |sum_j marginal - 1| <= E_v + gamma_G + 1e-300
    quantile: its bin j* is accepted when  cdf_ref[j*] + D[j*] >= p  and  cdf_ref[j* - 1] - D[j* - 1] < p  (j* > 0), with D the
              running sum of the bins' bounds: the library's running sum can cross p at any bin the reference's does within them.
"""
from __future__ import annotations

import numpy as np
from grid_posterior_reference import U, reference as posterior_reference


def weights(ell):
    """Normalised weights (n_vox, G) of l (n_vox, G) by a two-pass log-sum-exp; an atom at -inf weighs exactly 0."""
    m = ell.max(axis=1)
    w = np.exp(ell - m[:, None])
    return w / w.sum(axis=1)[:, None]


def marginals(W, n_bins, bin_of):
    """(n_vox, B): per parameter k with n_bins[k] > 0 and bin j the sum of W over the atoms with bin_of[k, g] == j."""
    out = np.zeros((W.shape[0], int(np.sum(n_bins))))
    off = 0
    for k, nb in enumerate(n_bins):
        for j in range(nb):
            out[:, off + j] = W[:, np.asarray(bin_of[k]) == j].sum(axis=1)
        off += nb
    return out


def quantile_bins(cdf, probs):
    """(n_q, n_vox) index of the first bin with cdf >= p, the last bin if none reaches it; cdf (n_vox, nb)."""
    nb = cdf.shape[1]
    out = np.empty((len(probs), cdf.shape[0]), int)
    for i, p in enumerate(probs):
        hit = cdf >= p
        out[i] = np.where(hit.any(axis=1), hit.argmax(axis=1), nb - 1)
    return out


def reference(model, b, y, atoms, lo, hi, n_bins, bin_of, bin_value, probs=(), log_prior=None, noise_sd=0.0, project=False, **kw):
    """dict(marginal (n_vox, B), bound (n_vox, B), rel (n_vox,), quantile_bin {k: (n_q, n_vox)}, log_evidence, bound_log_evidence,
    finite, empty (B,): the bin holds no admissible atom, post: the posterior reference's dict)."""
    post = posterior_reference(model, b, y, atoms, lo, hi, log_prior=log_prior, noise_sd=noise_sd, project=project, **kw)
    G = post["l"].shape[1]
    W = weights(post["l"])
    marg = marginals(W, n_bins, bin_of)
    rel = np.expm1(2 * post["eps"]) + 4 * (G + 16) * U
    adm = np.ones(G, bool) if log_prior is None else np.asarray(log_prior, float) > -np.inf
    empty = np.concatenate([[not (adm & (np.asarray(bin_of[k]) == j)).any() for j in range(nb)] for k, nb in enumerate(n_bins) if nb])
    qbin, off = {}, 0
    for k, nb in enumerate(n_bins):
        if nb:
            qbin[k] = quantile_bins(np.cumsum(marg[:, off:off + nb], axis=1), probs)
        off += nb
    return dict(marginal=marg, bound=rel[:, None] * marg + 1e-300, rel=rel, quantile_bin=qbin, log_evidence=post["log_evidence"],
                bound_log_evidence=post["bound_log_evidence"], finite=post["finite"], empty=np.asarray(empty, bool), post=post)


def accept(ref, got, n_bins, bin_value, probs):
    """The acceptance of a result dict of api.grid_marginals on EVERY voxel; returns the largest error-to-bound ratio of a bin."""
    fin = ref["finite"]
    n_vox = len(fin)
    bin_value = np.asarray(bin_value, float)
    worst, off = 0.0, 0
    assert got["log_evidence"].shape == (n_vox,) and np.isnan(got["log_evidence"][~fin]).all()
    err = np.abs(got["log_evidence"][fin] - ref["log_evidence"][fin])
    assert (err <= ref["bound_log_evidence"][fin]).all(), "log_evidence outside its bound"
    assert sorted(got["marginal"]) == [k for k, nb in enumerate(n_bins) if nb] == sorted(got["values"]) == sorted(got["quantiles"])
    for k, nb in enumerate(n_bins):
        if not nb:
            continue
        m, val, q = got["marginal"][k], got["values"][k], got["quantiles"][k]
        assert m.shape == (nb, n_vox) and m.dtype == np.float64 and q.shape == (len(probs), n_vox)
        assert val.tobytes() == bin_value[off:off + nb].tobytes()
        assert np.isnan(m[:, ~fin]).all() and np.isnan(q[:, ~fin]).all()
        mf, rf, bf = m[:, fin].T, ref["marginal"][fin, off:off + nb], ref["bound"][fin, off:off + nb]
        assert np.isfinite(mf).all() and (mf >= 0).all()
        assert (mf[:, ref["empty"][off:off + nb]] == 0).all(), "a bin without an admissible atom is not exactly 0"
        err = np.abs(mf - rf)
        assert (err <= bf).all(), f"parameter {k}: a bin is {(err / bf).max():.3g} x its bound off"
        worst = max(worst, float((err / bf).max()))
        total = np.abs(mf.sum(axis=1) - 1.0)
        assert (total <= ref["rel"][fin] + 1e-300).all(), f"parameter {k}: the bins sum to 1 +- {total.max():.3g}"
        cdf, D = np.cumsum(rf, axis=1), np.cumsum(bf, axis=1)
        rows = np.arange(cdf.shape[0])
        for i, p in enumerate(probs):
            js = np.searchsorted(val, q[i, fin])
            assert (js < nb).all() and (val[js] == q[i, fin]).all(), "a quantile is not a grid value"
            assert (cdf[rows, js] + D[rows, js] >= p).all(), f"parameter {k}, level {p}: the reported bin is too low"
            low = js > 0
            assert (cdf[rows[low], js[low] - 1] - D[rows[low], js[low] - 1] < p).all(), f"parameter {k}, level {p}: the reported bin is too high"
        off += nb
    return worst

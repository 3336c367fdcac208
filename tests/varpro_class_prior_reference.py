"""numpy restatement of pnx_curvefit_varpro_posterior_classes_f64 and pnx_curvefit_varpro_prior_em_classes_f64 (include/pnx.h,
DESIGN.md 4.1o) for the tests, built on tests/varpro_posterior_reference.py, tests/varpro_prior_reference.py and
tests/grid_class_prior_reference.py (imported, not restated): a voxel is judged under the row of its label, and a class's row is
updated by `em_step` on that class's voxels alone.  `em_step_classes` and `normalise_rows` apply as they stand to the varpro l0
(the Occam term plus the likelihood term).

Acceptance is those modules' bound machinery and nothing else:
    posterior   the per-voxel bounds of varpro_posterior_reference.reference computed under the voxel's own row;
    one update  grid_prior_reference.step_bounds per class, on the class's voxels (N in gamma_N is the class's count);
    t updates   (2^t - 1) single-step bounds per class, t <= 3 (a class's row depends on its own voxels and its own row only);
    loglik      the sum over the classes of the per-class bounds.
A label outside [0, n_classes) marks a voxel that takes no part: `finite` is False for it."""
from __future__ import annotations

import numpy as np
from grid_class_prior_reference import accept_em as _accept_em_rows
from grid_class_prior_reference import em_step_classes, in_range, normalise_rows, same_start, table  # noqa: F401  (re-exported)
from varpro_posterior_reference import ratios, reference  # noqa: F401
from varpro_prior_reference import em_step, likelihoods, normalise, population  # noqa: F401

PER_VOXEL = ("mean", "var", "log_evidence", "ess", "clipped_mass", "map_atom", "l", "eps", "lin", "param_bound", "bound_mean", "bound_var",
             "bound_log_evidence", "bound_ess", "bound_clipped_mass")


def posterior(model, b, y, nl_atoms, lo, hi, labels, n_classes, log_prior=None, noise_sd=0.0, marginal=True, max_eps=1e-6, **kw):
    """The posterior reference per voxel under its own row: the dict of varpro_posterior_reference.reference, assembled class by
    class (l is the (n_vox, n_atoms) matrix under each voxel's row); a voxel with a label out of range is not finite."""
    labels = np.asarray(labels)
    y = np.atleast_2d(np.asarray(y, float))
    n_vox, G = y.shape[0], np.asarray(nl_atoms).shape[1]
    tab = table(log_prior, n_classes, G)
    out = None
    for c in range(n_classes):
        idx = np.flatnonzero(labels == c)
        if not idx.size:
            continue
        ref = reference(model, b, y[idx], nl_atoms, lo, hi, log_prior=tab[c], noise_sd=noise_sd, marginal=marginal, max_eps=max_eps, **kw)
        if out is None:
            out = {k: np.full((n_vox,) + np.shape(ref[k])[1:], np.nan) for k in PER_VOXEL}
            out["map_atom"] = np.full(n_vox, -1)
            out["finite"] = np.zeros(n_vox, bool)
            out.update({k: ref[k] for k in ("lin_rows", "nl_rows", "K", "cls")})
        for k in PER_VOXEL:
            out[k][idx] = ref[k]
        out["finite"][idx] = ref["finite"]
    assert out is not None, "no voxel carries a label in range"
    return out


def accept_em(got, l0, eps0, finite, labels, lp0, alpha, steps):
    """The result of `steps` updates (rel_tol = 0) of api.varpro_prior_em_classes against the all-numpy run from the normalised
    start lp0 (C, G), class by class: grid_class_prior_reference.accept_em on the varpro l0.  An atom whose Occam term is not finite
    (l0 = -inf in every voxel) is inadmissible in every row: the start the update sees holds -inf there, as the library's does.
    Returns the largest error-to-bound ratios (log_prior, loglik)."""
    lp0 = np.array(lp0, float)
    dead = np.isneginf(np.asarray(l0)[np.asarray(finite)]).all(axis=0) if np.asarray(finite).any() else np.zeros(lp0.shape[1], bool)
    lp0[:, dead] = -np.inf
    return _accept_em_rows(got, l0, eps0, finite, labels, lp0, alpha, steps)


def wide(lo, hi):
    """The box of `population` with the fraction in [-40, 40]: no pair clips, so eps_v stays under 1e-6 and the derived bounds apply
    (tests/test_gpu_varpro_prior.py's choice for the same population)."""
    wlo, whi = np.array(lo, float), np.array(hi, float)
    wlo[0], whi[0] = -40.0, 40.0
    return wlo, whi


# the second tissue of `two_populations`: the same fractions, both rates a modest factor (1.6, 1.5) away from the first tissue's
TISSUE_1 = dict(f1=0.15, d1=0.08, d2=0.0008)
WORTH_ROW = 0  # the parameter whose median |error| is compared: f1, 4.1m's figure (a table over the rates moves it through them)


def two_populations(n_each=1000, seed=0, noise=0.05):
    """Two narrow bi_s0 populations of n_each voxels, labelled 0 and 1, on the 91-atom dictionary of varpro_prior_reference.population:
    label 0 is that population (f1 ~ N(0.15, 0.03), D1 ~ 0.05, D2 ~ 0.0012, sd 0.2 of the logarithm), label 1 has the SAME fractions
    and rates a modest factor away (D1 ~ 0.08, D2 ~ 0.0008).  The table is over the rates only, so populations that differ in a
    fraction alone cannot gain from a row of their own.  (Ratio per-label / single of the numpy reference's median |error| of
    (f1, D1, D2) after three updates, noise known | marginalised, for the candidates tried: (0.03, 0.0018) 1.01 0.95 0.94 | 1.01
    0.93 0.97; (0.035, 0.0016) 0.91 0.97 0.99 | 0.91 0.96 1.01; (0.05, 0.002) 0.96 1.01 0.93 | 0.93 1.00 0.92; this one 0.83 0.93
    0.94 | 0.77 0.92 0.89 -- the only one past 10 % in both modes, and only for f1.)  The fraction's box is `wide`.
    Returns (b, y, truth (4, 2 n_each), labels, nl_atoms, lo, hi)."""
    from grid_start_reference import signals

    b, y0, t0, atoms, lo, hi = population(n_each, seed=seed, noise=noise)
    rng = np.random.default_rng(seed + 101)
    t1 = np.stack([np.clip(rng.normal(TISSUE_1["f1"], 0.03, n_each), 0.02, 0.5), TISSUE_1["d1"] * np.exp(0.2 * rng.standard_normal(n_each)),
                   TISSUE_1["d2"] * np.exp(0.2 * rng.standard_normal(n_each)), np.ones(n_each)])
    y1 = signals("bi_s0", b, t1) + noise * rng.standard_normal((n_each, len(b)))
    labels = np.repeat(np.array([0, 1], np.int32), n_each)
    lo, hi = wide(lo, hi)
    return b, np.ascontiguousarray(np.concatenate([y0, y1])), np.concatenate([t0, t1], axis=1), labels, atoms, lo, hi


def worth(noise_sd=0.05, n_iter=3, n_each=1000):
    """The numpy run of the 'what it is worth' case: median |error| of f1 (and of f1, D1, D2 in `medians`) under the single
    learned table and under the per-label tables, with the posterior references under both."""
    b, y, truth, labels, atoms, lo, hi = two_populations(n_each)
    l0, eps0, fin = likelihoods("bi_s0", b, y, atoms, lo, hi, noise_sd=noise_sd)
    G = atoms.shape[1]
    single = normalise(None, G)
    rows = normalise_rows(None, 2, G)
    for _ in range(n_iter):
        single = em_step(l0, single, fin)[1]
        rows = em_step_classes(l0, rows, fin, labels)[1]
    one = reference("bi_s0", b, y, atoms, lo, hi, log_prior=single, noise_sd=noise_sd)
    per = posterior("bi_s0", b, y, atoms, lo, hi, labels, 2, log_prior=rows, noise_sd=noise_sd)
    med = lambda ref: np.median(np.abs(ref["mean"][:, :3] - truth[:3].T), axis=0)
    return dict(single=float(med(one)[WORTH_ROW]), per_label=float(med(per)[WORTH_ROW]), medians=(med(one), med(per)), ref_single=one,
                ref_per_label=per, table_single=single, table_per_label=rows, truth=truth, data=(b, y, labels, atoms, lo, hi))


__all__ = ["accept_em", "same_start", "em_step_classes", "in_range", "normalise_rows", "posterior", "ratios", "table", "two_populations",
           "worth", "wide"]

"""numpy restatement of pnx_curvefit_grid_posterior_classes_f64 and pnx_curvefit_grid_prior_em_classes_f64 (include/pnx.h, DESIGN.md
4.1n) for the tests, built on tests/grid_posterior_reference.py and tests/grid_prior_reference.py (imported, not restated): a voxel
is judged under the row of its label, and a class's row is updated by `em_step` on that class's voxels alone.

Acceptance is those modules' bound machinery and nothing else:
    posterior   the per-voxel bounds of grid_posterior_reference.reference computed under the voxel's own row;
    one update  grid_prior_reference.step_bounds per class, on the class's voxels (N in gamma_N is the class's count);
    t updates   (2^t - 1) single-step bounds per class, t <= 3 (a class's row depends on its own voxels and its own row only, so the
                drift argument of grid_prior_reference holds class by class);
    loglik      the sum over the classes of the per-class bounds.
A label outside [0, n_classes) marks a voxel that takes no part: `finite` is False for it."""
from __future__ import annotations

import numpy as np
from grid_posterior_reference import ratios, reference
from grid_prior_reference import accept_step, em_step, likelihoods, normalise, step_bounds

KEYS = ("mean", "var", "log_evidence", "ess", "map_atom", "eps", "bound_mean", "bound_var", "bound_log_evidence", "bound_ess")


def table(log_prior, n_classes, n_atoms):
    """(n_classes, n_atoms) float table; None is uniform in every row."""
    return np.zeros((n_classes, n_atoms)) if log_prior is None else np.asarray(log_prior, float).reshape(n_classes, n_atoms)


def normalise_rows(log_prior, n_classes, n_atoms):
    return np.stack([normalise(row, n_atoms) for row in table(log_prior, n_classes, n_atoms)])


def in_range(labels, n_classes):
    labels = np.asarray(labels)
    return (labels >= 0) & (labels < n_classes)


def posterior(model, b, y, atoms, lo, hi, labels, n_classes, log_prior=None, noise_sd=0.0, project=False, **kw):
    """The posterior reference per voxel under its own row: the dict of grid_posterior_reference.reference, assembled class by class
    (l is the (n_vox, n_atoms) matrix under each voxel's row); a voxel with a label out of range is not finite."""
    labels = np.asarray(labels)
    y = np.asarray(y, float)
    n_vox, G = y.shape[0], np.asarray(atoms).shape[1]
    tab = table(log_prior, n_classes, G)
    out = None
    for c in range(n_classes):
        idx = np.flatnonzero(labels == c)
        if not idx.size:
            continue
        ref = reference(model, b, y[idx], atoms, lo, hi, log_prior=tab[c], noise_sd=noise_sd, project=project, **kw)
        if out is None:
            out = {k: np.full((n_vox,) + np.shape(ref[k])[1:], np.nan) for k in KEYS + ("l",)}
            out["map_atom"] = np.full(n_vox, -1)
            out["finite"] = np.zeros(n_vox, bool)
            out["amp"] = None if ref["amp"] is None else np.full((n_vox, G), np.nan)
            out["s0_row"] = ref["s0_row"]
        for k in KEYS + ("l",):
            out[k][idx] = ref[k]
        out["finite"][idx] = ref["finite"]
        if out["amp"] is not None:
            out["amp"][idx] = ref["amp"]
    assert out is not None, "no voxel carries a label in range"
    return out


def same_start(row, ref):
    """A normalised start row of the library against numpy's: -inf where numpy has -inf, elsewhere within the rounding of the
    normaliser (a sum of G terms in another order: gamma_G = 4 (G + 16) 2^-52) and of the subtraction (2^-52 |entry|)."""
    row, ref = np.asarray(row), np.asarray(ref)
    adm = ref > -np.inf
    if not ((row[~adm] == -np.inf).all() and np.isfinite(row[adm]).all()):
        return False
    return bool((np.abs(row[adm] - ref[adm]) <= 4 * (ref.size + 16) * 2.0 ** -52 + 2.0 ** -52 * np.abs(ref[adm])).all())


def em_step_classes(l0, lp, finite, labels, alpha=0.0):
    """One update of every row from the normalised table lp (C, G): (S (C, G), lp_next (C, G), loglik per class (C,), n per class).
    A class without a voxel that takes part keeps its row."""
    lp = np.asarray(lp, float)
    C = lp.shape[0]
    S, nxt, ll, n = np.zeros(lp.shape), lp.copy(), np.zeros(C), np.zeros(C, int)
    for c in range(C):
        part = finite & (np.asarray(labels) == c)
        S[c], nxt[c], ll[c] = em_step(l0, lp[c], part, alpha)
        n[c] = int(part.sum())
    return S, nxt, ll, n


def accept_em(got, l0, eps0, finite, labels, lp0, alpha, steps):
    """The result of `steps` updates (rel_tol = 0) of api.grid_prior_em_classes against the all-numpy run from the normalised start
    lp0 (C, G), class by class as grid_prior tests accept the single table.  Returns the largest error-to-bound ratios
    (log_prior, loglik)."""
    labels = np.asarray(labels)
    C, G = lp0.shape
    part = [finite & (labels == c) for c in range(C)]
    n = np.array([int(p.sum()) for p in part])
    assert got["n_eff"].tolist() == n.tolist() and got["n_iter"] == steps
    assert got["loglik"].shape == (steps + 1,) and got["loglik_class"].shape == (steps + 1, C) and got["log_prior"].shape == (C, G)
    lp, drift, worst_ll, worst_lp = lp0.copy(), np.zeros(C), 0.0, 0.0
    last = [None] * C
    for t in range(steps + 1):
        total_bound, total_ref = 0.0, 0.0
        for c in range(C):
            if not n[c]:
                assert got["loglik_class"][t, c] == 0.0
                continue
            S, lp_next, ll = em_step(l0, lp[c], part[c], alpha)
            bd = step_bounds(l0, lp[c], eps0, part[c], S)
            bound = bd["loglik"] + n[c] * drift[c]  # a row moved by eta moves every L_v of its class by at most eta
            err = abs(got["loglik_class"][t, c] - ll)
            assert err <= bound, f"loglik_class[{t}, {c}]: error is {err / bound:.3g} x its bound"
            worst_ll = max(worst_ll, err / bound)
            total_bound += bound
            total_ref += ll
            if t < steps:
                drift[c] = 2 * drift[c] + bd["lp"]
                last[c] = (lp_next, S)
                lp[c] = lp_next
        assert abs(got["loglik"][t] - total_ref) <= total_bound, f"loglik[{t}]"
        # the sum over the classes, in class order: a few ulp of the summed magnitudes
        assert abs(got["loglik"][t] - got["loglik_class"][t].sum()) <= 4 * C * 2.0 ** -52 * np.abs(got["loglik_class"][t]).sum()
    for c in range(C):
        if not n[c]:  # the normalised start, untouched
            assert same_start(got["log_prior"][c], lp0[c]), f"class {c} has no voxel: its row must be the normalised start"
            continue
        worst_lp = max(worst_lp, accept_step(got["log_prior"][c], lp0[c], last[c][0], last[c][1], n[c], drift[c], alpha))
    print(f"log_prior: error / bound = {worst_lp:.3g} after {steps} update(s); loglik worst {worst_ll:.3g}")
    return worst_lp, worst_ll


def two_populations(n_each=1000, seed=0, noise=0.05):
    """Two narrow bi_s0 populations of n_each voxels, labelled 0 and 1, on the grid of grid_prior_reference.population: label 0 is
    that population (f1 ~ N(0.15, 0.03), D1 ~ 0.05, D2 ~ 0.0012), label 1 has the same rates and f1 ~ N(0.25, 0.03): two tissues the
    signal of one voxel barely tells apart, which is where the label helps.  (Tried first: label 1 at f1 ~ 0.35, D1 ~ 0.02,
    D2 ~ 0.0022 -- so far from label 0 that the single table unmixes them by itself and the per-label gain in the median |error| of
    f1 is 1.5 %; also tried f1 0.30 / 0.35 at the same rates, D1 0.1, and (0.30, 0.03, 0.0015): gains of 8 to 25 %.)
    Returns (b, y, truth (4, 2 n_each), labels, atoms, lo, hi)."""
    from grid_prior_reference import population
    from grid_start_reference import signals

    b, y0, t0, _, atoms, lo, hi = population(n_each, seed=seed, noise=noise)
    rng = np.random.default_rng(seed + 101)
    t1 = np.stack([np.clip(rng.normal(0.25, 0.03, n_each), 0.02, 0.5), 0.05 * np.exp(0.2 * rng.standard_normal(n_each)),
                   0.0012 * np.exp(0.2 * rng.standard_normal(n_each)), np.ones(n_each)])
    y1 = signals("bi_s0", b, t1) + noise * rng.standard_normal((n_each, len(b)))
    labels = np.repeat(np.array([0, 1], np.int32), n_each)
    return b, np.ascontiguousarray(np.concatenate([y0, y1])), np.concatenate([t0, t1], axis=1), labels, atoms, lo, hi


def worth(noise_sd=0.05, n_iter=3):
    """The numpy run of the 'what it is worth' case: median |error| of f1 under the single learned table and under the per-label
    tables, with the posterior means and their bounds under both (for the comparison of the library against them)."""
    b, y, truth, labels, atoms, lo, hi = two_populations()
    l0, eps0, fin = likelihoods("bi_s0", b, y, atoms, lo, hi, noise_sd=noise_sd, project=True)
    G = atoms.shape[1]
    single = normalise(None, G)
    rows = normalise_rows(None, 2, G)
    for _ in range(n_iter):
        single = em_step(l0, single, fin)[1]
        rows = em_step_classes(l0, rows, fin, labels)[1]
    one = reference("bi_s0", b, y, atoms, lo, hi, log_prior=single, noise_sd=noise_sd, project=True)
    per = posterior("bi_s0", b, y, atoms, lo, hi, labels, 2, log_prior=rows, noise_sd=noise_sd, project=True)
    med = lambda ref: float(np.median(np.abs(ref["mean"][:, 0] - truth[0])))
    return dict(single=med(one), per_label=med(per), ref_single=one, ref_per_label=per, table_single=single, table_per_label=rows,
                truth=truth, data=(b, y, labels, atoms, lo, hi))


__all__ = ["accept_em", "same_start", "em_step_classes", "in_range", "normalise_rows", "posterior", "ratios", "table", "two_populations", "worth"]

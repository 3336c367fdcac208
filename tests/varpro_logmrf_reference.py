"""numpy restatement of the neighbourhood (MRF) prior of the variable-projection posterior with a per-row linear or log coupling
(include/pnx.h) for the tests, on top of tests/varpro_mrf_reference.py: the field rows f, field_mean, one colour
update, the driver and the variational free energy.

    f_kg = nl_atoms[row_k, g] (coupling 0) or log nl_atoms[row_k, g] (coupling 1);  fc = f - fcentre
    l_g(v) = l0_g(v) + sum_k fc_kg q_vk - 1/2 n_v r_g;  q_vk = lambda_k sum_{u present} (field_mean[k, u] - fcentre_k)
    field_mean[k, v] = E_W[f_k] on a non-linear row, mean[k, v] on a fraction / S0 row

mean, var and the other outputs stay varpro_mrf_reference's, over the linear theta.  The acceptance bounds are 4.1q's with two
changes: the field's rounding term is taken over |fc| (field_terms is fed f and fcentre), and bound_field_mean is bound_mean's
formula E R + gamma S + U A with R, S, A over f.

    F = sum_v sum_g W (l0 - log W) - 1/2 sum_edges sum_k lambda_k (var_f + var_f' + (m_f - m_f')^2)      over the coupled f

is the variational free energy; a colour update is coordinate ascent on it, so it never decreases."""
from __future__ import annotations

import numpy as np
import varpro_mrf_reference as R
from varpro_mrf_reference import base_posterior, colour_sort, gather, n_free_of, phantom  # noqa: F401  (for the tests)
from varpro_posterior_reference import U


def coupling_of(base, value):
    """(n_free,) int: `value` an array of flags, or "log" / "linear" for every non-linear row."""
    c = np.zeros(n_free_of(base), int)
    if isinstance(value, str):
        c[base["nl_rows"]] = int(value == "log")
        return c
    c[:] = np.asarray(value, int)
    assert not c[base["lin_rows"]].any()
    return c


def f_rows(base, nl_atoms, lp, coupling):
    """(n_nl, G): the coupled quantity per row of nl_atoms; 0 at an excluded atom (its weight is 0)."""
    adm = lp > -np.inf
    f = np.array(nl_atoms, float)
    for j, k in enumerate(base["nl_rows"]):
        if coupling[k]:
            assert (f[j, adm] > 0).all()
            f[j] = np.where(adm, np.log(np.where(adm, f[j], 1.0)), 0.0)
    return f


def centres(base, nl_atoms, lp, coupling):
    return R.centres(base, f_rows(base, nl_atoms, lp, coupling), lp)


def ranges(base, nl_atoms, lp, coupling):
    return R.ranges(base, f_rows(base, nl_atoms, lp, coupling), lp)


def precision_of(base, nl_atoms, lp, strength, coupling):
    """strength / range(f)^2 on the non-linear rows (0 for a one-value row), 0 on the linear rows."""
    return R.precision_of(base, f_rows(base, nl_atoms, lp, coupling), lp, strength)


def effective(coupling, precision):
    """The flags the ABI takes: 0 where the precision is 0."""
    return np.where(np.asarray(precision) > 0, coupling, 0).astype(np.int32)


def field_posterior(base, nl_atoms, lp, q, n, precision, coupling):
    """One update of ALL voxels under the field; varpro_mrf_reference.field_posterior's dict (moments over the linear theta) with
    field_mean, var_f (n_vox, n_free) and bound_field_mean beside it."""
    f = f_rows(base, nl_atoms, lp, coupling)
    fcentre = R.centres(base, f, lp)
    fld, mag = R.field_terms(base, f, fcentre, np.asarray(precision, float), np.asarray(q, float), np.asarray(n))
    with np.errstate(invalid="ignore"):
        ell = base["l"] + fld
    adm = lp > -np.inf
    ell[:, ~adm] = -np.inf
    eps = base["eps"] + 4 * (len(base["nl_rows"]) + 2) * U * mag
    out = R._posterior_from_l(ell, eps, base, nl_atoms, lp)
    W, rows = out["W"], list(base["nl_rows"])
    fm, vf = np.array(out["mean"]), np.array(out["var"])  # a coupling-0 row: mean itself, as the device writes its bytes
    for j, k in enumerate(rows):
        if coupling[k]:
            fm[:, k] = fcentre[k] + W @ (f[j] - fcentre[k])
            vf[:, k] = (W * (f[j][None, :] - fm[:, k, None]) ** 2).sum(axis=1)
    G = ell.shape[1]
    Rf = f[:, adm].max(axis=1) - f[:, adm].min(axis=1)
    Af = np.abs(f[:, adm]).max(axis=1)
    gamma = 4 * (G + 16) * U
    E = np.expm1(2 * eps)
    bound = np.array(out["bound_mean"])
    for j, k in enumerate(rows):
        if coupling[k]:
            bound[:, k] = E * Rf[j] + gamma * Rf[j] + U * Af[j]
    out.update(field_mean=fm, var_f=vf, bound_field_mean=bound)
    return out


KEYS = ("mean", "var", "log_evidence", "ess", "clipped_mass", "map_atom", "W", "l", "eps", "bound_mean", "bound_var", "bound_log_evidence",
        "bound_ess", "bound_clipped_mass", "field_mean", "var_f", "bound_field_mean")


def mrf(model, b, y, nl_atoms, lo, hi, nb, colour_start, precision, coupling, n_sweeps, tol=0.0, trace_free_energy=False, **kw):
    """The driver: sweep 0 the plain posterior (with its field_mean), then colour after colour the gather over field_mean and the
    update of that colour's range.  Returns the last state (n_vox leading), delta (list), and F after every colour update."""
    base, nl_atoms, lp = base_posterior(model, b, y, nl_atoms, lo, hi, **kw)
    nb = np.asarray(nb)
    n_vox, n_free = nb.shape[0], n_free_of(base)
    precision = np.asarray(precision, float)
    coupling = effective(coupling_of(base, coupling), precision)
    fcentre = centres(base, nl_atoms, lp, coupling)
    zero = field_posterior(base, nl_atoms, lp, np.zeros((n_free, n_vox)), np.zeros(n_vox, np.int32), precision, coupling)
    state = {k: np.array(zero[k]) for k in KEYS}
    fin = base["finite"]
    rng = np.where(precision > 0, ranges(base, nl_atoms, lp, coupling), 0.0)
    energy = lambda: R.free_energy(base, state["W"], state["field_mean"], state["var_f"], nb, precision)
    Fs = [energy()] if trace_free_energy else []
    delta = []
    for s in range(n_sweeps):
        d = 0.0
        for c in range(len(colour_start) - 1):
            lo_c, hi_c = int(colour_start[c]), int(colour_start[c + 1])
            if hi_c == lo_c:
                continue
            q, n = gather(nb, np.where(fin[None, :], state["field_mean"].T, np.nan), fcentre, precision)
            new = field_posterior(base, nl_atoms, lp, q, n, precision, coupling)
            sel = np.arange(lo_c, hi_c)
            take = sel[fin[sel]]
            for k in np.flatnonzero(rng > 0):
                if take.size:
                    d = max(d, float((np.abs(new["field_mean"][take, k] - state["field_mean"][take, k]) / rng[k]).max()))
            for key in KEYS:
                state[key][sel] = new[key][sel]
            if trace_free_energy:
                Fs.append(energy())
        delta.append(d)
        if tol > 0 and d <= tol:
            break
    state.update(finite=fin, lin_rows=base["lin_rows"], nl_rows=base["nl_rows"], lin=base["lin"], param_bound=zero["param_bound"],
                 K=base["K"], cls=base["cls"], coupling=coupling)
    return state, delta, Fs


def accept_field_mean(ref, got_field_mean, got_mean, coupling, sel=None):
    """field_mean (n_free, n_vox) inside bound_field_mean on every finite voxel of `sel`, NaN on the others, and the bytes of mean
    on every coupling-0 row; returns the largest error / bound."""
    n_vox = ref["finite"].shape[0]
    sel = np.arange(n_vox) if sel is None else np.asarray(sel)
    fin = ref["finite"][sel]
    fm, mean = np.asarray(got_field_mean)[:, sel], np.asarray(got_mean)[:, sel]
    assert np.isnan(fm[:, ~fin]).all() and np.isfinite(fm[:, fin]).all()
    for k in np.flatnonzero(np.asarray(coupling) == 0):
        assert np.ascontiguousarray(fm[k]).tobytes() == np.ascontiguousarray(mean[k]).tobytes(), f"field_mean row {k} is not mean's bytes"
    err = np.abs(fm[:, fin].T - ref["field_mean"][sel][fin])
    bound = ref["bound_field_mean"][sel][fin]
    worst = float((err / np.where(bound > 0, bound, 1.0))[(bound > 0) | (err > 0)].max(initial=0.0))
    print("field_mean error / bound:", f"{worst:.3g}")
    assert (err <= bound).all(), f"field_mean: error is {worst:.3g} x its bound"
    return worst

"""numpy restatement of pnx_peel_f64 (include/pnx.h) for the tests, in two forms that share nothing but the definition of the
problem: `centred` fits every stage's line by the closed form as the header writes it, `lstsq` solves the same weighted line with
np.linalg.lstsq on sqrt(w)-scaled rows.  Each form runs its OWN chain of stages: the residual a stage sees is what the same form
left of the signal.  No tests here.

Both return dict(params (n_params, n_vox), status int8, n_used (K, n_vox) int32, ss_res (n_vox,)), voxel by voxel."""
from __future__ import annotations

import numpy as np

NAN = float("nan")
STAGES = {"mono": 1, "bi_reduced": 2, "bi_s0": 2, "bi_full": 2, "tri_reduced": 3, "tri_s0": 3, "tri_full": 3}
N_PARAMS = {"mono": 2, "bi_reduced": 3, "bi_s0": 4, "bi_full": 4, "tri_reduced": 5, "tri_s0": 6, "tri_full": 6}
THRESHOLDS = {1: [], 2: [150.0], 3: [30.0, 250.0]}


def bvalues(n_b):
    """unique(round([0] + geomspace(5, 1200, n_b - 1), 3)): the issue's b-values."""
    b = np.unique(np.round(np.concatenate([[0.0], np.geomspace(5.0, 1200.0, n_b - 1)]), 3))
    assert b.size == n_b
    return b


def threshold_masks(b, K, thresholds):
    """(K, n_b) bool: stage 0 takes b >= t_{K-1}, a middle stage k t_{K-1-k} <= b < t_{K-k}, the last stage b < t_1."""
    edges = np.concatenate([[-np.inf], np.asarray(thresholds, float), [np.inf]])
    return np.stack([(b >= edges[K - 1 - k]) & (b < edges[K - k]) for k in range(K)])


def stage_masks(b, K):
    """The masks of the parity signals: the issue's thresholds ([150] for two, [30, 250] for three exponentials) where they leave
    every stage at least two b-values; for the few b-values where they do not (2K, 2K + 1), K contiguous groups of nearly equal
    size, the highest b-values first."""
    m = threshold_masks(b, K, THRESHOLDS[K])
    if (m.sum(axis=1) >= 2).all():
        return m
    m = np.zeros((K, b.size), bool)
    for k, idx in enumerate(np.array_split(np.argsort(b)[::-1], K)):
        m[k, idx] = True
    return m


def signals(model, n_vox, n_b, seed=0, noise=5e-4):
    """(b, y, masks): the issue's parity signals.  S0 in [200, 2000], the slow D in [8e-4, 2e-3]; two exponentials: fast D in
    [0.02, 0.08] with f in [0.15, 0.35]; three: D in [0.008, 0.02] and [0.1, 0.3] with fractions in [0.2, 0.35] and [0.15, 0.3];
    multiplicative noise, all positive."""
    K = STAGES[model]
    rng = np.random.default_rng(100003 * seed + 131 * n_vox + 7 * n_b + K)
    b = bvalues(n_b)
    u = lambda lo, hi: rng.uniform(lo, hi, n_vox)[:, None]
    S0, Ds = u(200.0, 2000.0), u(8e-4, 2e-3)
    if K == 1:
        s = np.exp(-b * Ds)
    elif K == 2:
        f, Df = u(0.15, 0.35), u(0.02, 0.08)
        s = f * np.exp(-b * Df) + (1 - f) * np.exp(-b * Ds)
    else:
        f2, D2, f1, D1 = u(0.2, 0.35), u(0.008, 0.02), u(0.15, 0.3), u(0.1, 0.3)
        s = f1 * np.exp(-b * D1) + f2 * np.exp(-b * D2) + (1 - f1 - f2) * np.exp(-b * Ds)
    y = S0 * s * (1.0 + noise * rng.standard_normal((n_vox, n_b)))
    assert (y > 0).all()
    return b, np.ascontiguousarray(y), stage_masks(b, K)


def _line_centred(b, l, w):
    sw = w.sum()
    bm = (w * b).sum() / sw
    lm = (w * l).sum() / sw
    sbb = (w * (b - bm) ** 2).sum()
    D = -(w * (b - bm) * (l - lm)).sum() / sbb
    return lm + D * bm, D, sbb


def _line_lstsq(b, l, w):
    sq = np.sqrt(w)
    X = np.stack([np.ones_like(b), -b], axis=1)
    sol = np.linalg.lstsq(X * sq[:, None], l * sq, rcond=None)[0]
    sbb = (w * (b - (w * b).sum() / w.sum()) ** 2).sum()  # only for the status rule Sbb == 0
    return sol[0], sol[1], sbb


def model_signal(model, p, b):
    """The layout's signal at the parameter vector p (include/pnx.h, PNX_MODEL_*)."""
    e = lambda D: np.exp(-b * D)
    if model == "mono":
        return p[0] * e(p[1])
    if model in ("bi_reduced", "bi_s0"):
        s = p[0] * e(p[1]) + (1.0 - p[0]) * e(p[2])
        return p[3] * s if model == "bi_s0" else s
    if model == "bi_full":
        return p[0] * e(p[1]) + p[2] * e(p[3])
    if model in ("tri_reduced", "tri_s0"):
        s = p[0] * e(p[1]) + p[2] * e(p[3]) + (1.0 - p[0] - p[2]) * e(p[4])
        return p[5] * s if model == "tri_s0" else s
    return p[0] * e(p[1]) + p[2] * e(p[3]) + p[4] * e(p[5])


def _layout(model, A, D):
    S = sum(A)
    if model == "mono":
        return [A[0], D[0]]
    if model in ("bi_reduced", "bi_s0"):
        return [A[1] / S, D[1], D[0]] + ([S] if model == "bi_s0" else [])
    if model == "bi_full":
        return [A[1], D[1], A[0], D[0]]
    if model in ("tri_reduced", "tri_s0"):
        return [A[2] / S, D[2], A[1] / S, D[1], D[0]] + ([S] if model == "tri_s0" else [])
    return [A[2], D[2], A[1], D[1], A[0], D[0]]


def _one(model, b, y, masks, weighting, clip, lo, hi, fallback, form):
    K, n = STAGES[model], N_PARAMS[model]
    line = _line_centred if form == "centred" else _line_lstsq
    fail = list(fallback) if fallback is not None else [NAN] * n
    out = dict(params=fail, status=0, n_used=[0] * K, ss_res=NAN)
    M = masks.any(axis=0)
    if not np.isfinite(y[M]).all():
        out["status"] = -2
        return out
    r = y.copy()
    A, D = [], []
    with np.errstate(all="ignore"):
        for k in range(K):
            U = masks[k] & (r > 0)
            out["n_used"][k] = int(U.sum())
            if U.sum() < 2:
                return out
            ru, bu = r[U], b[U]
            w = ru * ru if weighting == 1 else np.ones_like(ru)
            a_k, D_k, sbb = line(bu, np.log(ru), w)
            A_k = np.exp(a_k)
            if sbb == 0 or not (np.isfinite(a_k) and np.isfinite(D_k) and np.isfinite(A_k)):
                return out
            A.append(A_k)
            D.append(D_k)
            r = r - A_k * np.exp(-b * D_k)
        p = np.array(_layout(model, A, D), float)
        st = 1
        if clip:
            c = np.where(p < lo, lo, np.where(p > hi, hi, p))
            st = 2 if ((p < lo) | (p > hi)).any() else 1
            p = c
        out.update(params=list(p), status=st, ss_res=((model_signal(model, p, b[M]) - y[M]) ** 2).sum())
    return out


def reference(model, b, y, masks, weighting=1, clip=None, fallback=None, form="centred"):
    """The peel of every row of y (n_vox, n_b) in float64.  masks (K, n_b) bool; weighting 0 (w = 1) / 1 (w = r^2); clip: None or
    (lo, hi) with one entry per parameter; fallback: None or the vector of a failed voxel.  form: "centred" or "lstsq"."""
    b = np.asarray(b, float)
    y = np.atleast_2d(np.asarray(y, float))
    masks = np.asarray(masks, bool)
    lo, hi = (np.asarray(a, float) for a in clip) if clip is not None else (None, None)
    rows = [_one(model, b, row, masks, weighting, clip is not None, lo, hi, fallback, form) for row in y]
    return dict(params=np.array([r["params"] for r in rows]).T.copy(), status=np.array([r["status"] for r in rows], np.int8),
                n_used=np.array([r["n_used"] for r in rows], np.int32).T.copy(), ss_res=np.array([r["ss_res"] for r in rows]))


EPS = 2.0 ** -52


def differences(got, ref, y, masks):
    """Largest relative difference per compared quantity between two results on the same rows, every voxel included:
      "params": |got - ref| / |ref| over every parameter;
      "ss_res": |got - ref| / (ref + EPS * sum of y_i^2 over the samples of any stage) -- each prediction carries a rounding error
                of EPS |y_i|, so a row's ss_res is not defined below EPS * sum y^2 (exact two-point lines leave rounding noise).
    Entries that are NaN in the reference must be NaN in `got` (asserted here, they do not enter the maximum)."""
    y = np.atleast_2d(np.asarray(y, float))
    M = np.asarray(masks, bool).any(axis=0)
    out = {}
    for key in ("params", "ss_res"):
        g, r = np.asarray(got[key], float), np.asarray(ref[key], float)
        assert g.shape == r.shape, (key, g.shape, r.shape)
        nan = np.isnan(r)
        assert (np.isnan(g) == nan).all(), f"{key}: NaN entries differ"
        with np.errstate(invalid="ignore", divide="ignore"):
            if key == "ss_res":
                floor = EPS * (np.where(np.isfinite(y[:, M]), y[:, M], 0.0) ** 2).sum(axis=1)
                d = np.abs(g - r) / (r + floor)
            else:
                d = np.abs(g - r) / np.abs(r)
        d = d[~nan]
        out[key] = float(d.max()) if d.size else 0.0
    return out


def parity_case(model, n_vox, n_b, weighting, seed=0):
    """(b, y, masks, lstsq form, measured difference of the two forms) on the parity signals.  Asserts what the parity tests rely
    on: every voxel complete in both forms, with equal statuses and n_used.  Under weighting 0 the logarithm of a small residual
    amplifies rounding and a noisy tri-exponential voxel can lose a stage; the noise is lowered (a factor 4 at a time, from the
    issue's 0.05 %) until every voxel is complete, so that the tests compare every voxel and skip none."""
    noise = 5e-4
    for _ in range(6):
        b, y, masks = signals(model, n_vox, n_b, seed=seed, noise=noise)
        cen = reference(model, b, y, masks, weighting=weighting, form="centred")
        lsq = reference(model, b, y, masks, weighting=weighting, form="lstsq")
        if (cen["status"] == 1).all() and (lsq["status"] == 1).all():
            break
        noise /= 4.0
    assert (cen["status"] == 1).all() and (lsq["status"] == 1).all(), (model, n_vox, n_b, weighting)
    assert np.array_equal(cen["n_used"], lsq["n_used"])
    return b, y, masks, lsq, differences(cen, lsq, y, masks)

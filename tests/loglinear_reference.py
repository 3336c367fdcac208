"""numpy restatement of pnx_loglinear_f64 (include/pnx.h) for the tests, in two forms that share nothing but the definition of
the problem: `centred` is the closed form as the header writes it, `lstsq` solves the same weighted line with np.linalg.lstsq on
sqrt(w)-scaled rows and takes the covariance from the explicit inverse of X^T W X.  No tests here.

Both return dict(params (2, n_vox), pcov (n_vox, 2, 2), status int8, n_used int32, ss_res (n_vox,)), voxel by voxel."""
from __future__ import annotations

import numpy as np

NAN = float("nan")


def signals(n_vox, n_b, seed=0, noise=0.01):
    """(b, y, S0, D): the issue's parity signals.  S0 in [200, 2000], D in [3e-4, 3e-3], multiplicative noise, all positive;
    b = linspace(0, 1200, n_b), and [0, 800] for two b-values."""
    rng = np.random.default_rng(100003 * seed + 131 * n_vox + n_b)
    b = np.array([0.0, 800.0]) if n_b == 2 else np.linspace(0.0, 1200.0, n_b)
    S0 = rng.uniform(200.0, 2000.0, n_vox)
    D = rng.uniform(3e-4, 3e-3, n_vox)
    y = S0[:, None] * np.exp(-b[None, :] * D[:, None]) * (1.0 + noise * rng.standard_normal((n_vox, n_b)))
    assert (y > 0).all()
    return b, np.ascontiguousarray(y), S0, D


def _weights(mode, y, b, a, D):
    if mode == 0:
        return np.ones_like(y)
    if mode == 1:
        return y * y
    return np.exp(a - b * D) ** 2


def _fit_centred(b, l, w):
    sw = w.sum()
    bm = (w * b).sum() / sw
    lm = (w * l).sum() / sw
    sbb = (w * (b - bm) ** 2).sum()
    D = -(w * (b - bm) * (l - lm)).sum() / sbb
    return lm + D * bm, D, (sw, bm, sbb)


def _cov_centred(b, l, w, a, D, aux, n):
    sw, bm, sbb = aux
    r = l - (a - b * D)
    s2 = (w * r * r).sum() / (n - 2)
    return s2 * (1.0 / sw + bm * bm / sbb), s2 * bm / sbb, s2 / sbb


def _fit_lstsq(b, l, w):
    sq = np.sqrt(w)
    X = np.stack([np.ones_like(b), -b], axis=1)
    sol = np.linalg.lstsq(X * sq[:, None], l * sq, rcond=None)[0]
    sbb = (w * (b - (w * b).sum() / w.sum()) ** 2).sum()  # only for the status rule Sbb == 0
    return sol[0], sol[1], (X, sbb)


def _cov_lstsq(b, l, w, a, D, aux, n):
    X = aux[0]
    r = l - X @ np.array([a, D])
    s2 = (w * r * r).sum() / (n - 2)
    C = s2 * np.linalg.inv(X.T @ (w[:, None] * X))
    return C[0, 0], C[0, 1], C[1, 1]


def _one(b, y, use, weighting, n_reweight, clip, lo, hi, form):
    fit, cov = (_fit_centred, _cov_centred) if form == "centred" else (_fit_lstsq, _cov_lstsq)
    out = dict(params=[NAN, NAN], pcov=np.full((2, 2), NAN), status=0, n_used=0, ss_res=NAN)
    yu, bu = y[use], b[use]
    if not np.isfinite(yu).all():
        out["status"] = -2
        return out
    pos = yu > 0
    n = int(pos.sum())
    out["n_used"] = n
    if n < 2:
        return out
    bp, yp = bu[pos], yu[pos]
    l = np.log(yp)
    a = D = 0.0
    with np.errstate(all="ignore"):
        for p in range(n_reweight + 1):
            w = _weights(2 if p else weighting, yp, bp, a, D)
            a, D, aux = fit(bp, l, w)
            if aux[-1] == 0:
                return out
        if not (np.isfinite(a) and np.isfinite(D)):
            return out
        S0 = np.exp(a)
        if n >= 3:
            va, cad, vd = cov(bp, l, w, a, D, aux, n)
            out["pcov"] = np.array([[S0 * S0 * va, S0 * cad], [S0 * cad, vd]])
        S0c, Dc, st = S0, D, 1
        if clip:
            S0c, Dc = min(max(S0, lo[0]), hi[0]), min(max(D, lo[1]), hi[1])
            st = 2 if (S0c != S0 or Dc != D) else 1
        out.update(params=[S0c, Dc], status=st, ss_res=((S0c * np.exp(-bu * Dc) - yu) ** 2).sum())
    return out


def reference(b, y, use=None, weighting=1, n_reweight=0, clip=None, form="centred"):
    """The fit of every row of y (n_vox, n_b) in float64.  use: (n_b,) bool or None; weighting 0 (w = 1) / 1 (w = y^2);
    clip: None or (lo, hi) with two entries each.  form: "centred" or "lstsq"."""
    b = np.asarray(b, float)
    y = np.atleast_2d(np.asarray(y, float))
    use = np.ones(b.size, bool) if use is None else np.asarray(use, bool)
    lo, hi = clip if clip is not None else (None, None)
    rows = [_one(b, row, use, weighting, n_reweight, clip is not None, lo, hi, form) for row in y]
    return dict(params=np.array([r["params"] for r in rows]).T.copy(), pcov=np.stack([r["pcov"] for r in rows]),
                status=np.array([r["status"] for r in rows], np.int8), n_used=np.array([r["n_used"] for r in rows], np.int32),
                ss_res=np.array([r["ss_res"] for r in rows]))


EPS = 2.0 ** -52


def differences(got, ref, y, use=None):
    """Largest relative difference per compared quantity between two results on the same rows, every voxel included:
      "params": |got - ref| / |ref| over S0 and D;
      "pcov":   |got - ref| / |ref| over the four entries (every entry of the covariance of a decaying signal is far from zero);
      "ss_res": |got - ref| / (ref + EPS * sum of y_i^2 over the masked-in samples) -- each prediction carries a rounding error of
                EPS |y_i|, so a row's ss_res is not defined below EPS * sum y^2 (an exact two-point line has ss_res = rounding noise).
    Entries that are NaN in the reference must be NaN in `got` (asserted here, they do not enter the maximum)."""
    y = np.atleast_2d(np.asarray(y, float))
    use = np.ones(y.shape[1], bool) if use is None else np.asarray(use, bool)
    out = {}
    for key in ("params", "pcov", "ss_res"):
        g, r = np.asarray(got[key], float), np.asarray(ref[key], float)
        assert g.shape == r.shape, (key, g.shape, r.shape)
        nan = np.isnan(r)
        assert (np.isnan(g) == nan).all(), f"{key}: NaN entries differ"
        with np.errstate(invalid="ignore", divide="ignore"):
            if key == "ss_res":
                floor = EPS * np.where(np.isfinite(y[:, use]), y[:, use], 0.0).__pow__(2).sum(axis=1)
                d = np.abs(g - r) / (r + floor)
            else:
                d = np.abs(g - r) / np.abs(r)
        d = d[~nan]
        out[key] = float(d.max()) if d.size else 0.0
    return out

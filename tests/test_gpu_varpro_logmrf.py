"""The log coupling of the neighbourhood (MRF) prior over the variable-projection dictionary on the device
(pnx_curvefit_varpro_posterior_logfield_f64, pnx_curvefit_varpro_posterior_logmrf_f64) against
tests/varpro_logmrf_reference.py: every output, field_mean included, inside the reference's own bounds (no tolerance of this file's
own); all-linear coupling as the bytes of the linear calls; a zero field as the bytes of api.varpro_posterior; the driver as the
bytes of its composition by hand; refusals that leave the device usable; and HipBayesVarProSolver's coupling="log" end to end on the
phantom, with its worth.  The inputs are tests/varpro_logmrf_cases.py's; tests/test_varpro_logmrf_host.py checks the reference's
preconditions on every one of them without a GPU."""
from __future__ import annotations

import numpy as np
import pytest
import varpro_logmrf_cases as cases
import varpro_logmrf_reference as LR
import varpro_mrf_reference as R
from varpro_posterior_reference import accept

from pyneapple_amd import _lib, api
from pyneapple_amd.models import BiExpModel
from pyneapple_amd.solvers import HipBayesVarProSolver

pytestmark = pytest.mark.gpu

POST_KEYS = ("mean", "sd", "map_p", "map_atom", "log_evidence", "ess", "clipped_mass")
ALL_KEYS = POST_KEYS + ("field_mean",)
N_VOX = 200
FIRSTS, COUNTS = (0, 1, 15, 16, 17), (1, 15, 16, 17, 83)


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _kw(c):
    kw = dict(c["kw"])
    kw["marginal_amplitudes"] = kw.pop("marginal")
    return kw


def logfield_on_device(gpu, c, q, n, pr, cp, first, count, start, want_delta=False, linear=False):
    """One (log)field posterior over [first, first + count) on device tensors that start as the arrays of `start`; numpy out."""
    import torch

    out = {k: _dev(start[k]) for k in (POST_KEYS if linear else ALL_KEYS)}
    delta = torch.full((1,), -1.0, dtype=torch.float64, device="cuda") if want_delta else None
    args = (c["model"], c["b"], _dev(c["y"]), c["nl_atoms"], c["lo"], c["hi"], _dev(q), _dev(n), pr)
    if linear:
        gpu.varpro_posterior_field(*args, out, first=first, count=count, delta_max=delta, **_kw(c))
    else:
        gpu.varpro_posterior_logfield(*args, cp, out, first=first, count=count, delta_max=delta, **_kw(c))
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    if want_delta:
        res["delta"] = float(delta.cpu()[0])
    return res


def sentinel(n_free, n_vox):
    s = {k: np.full((n_free, n_vox), -777.0) for k in ("mean", "sd", "map_p", "field_mean")}
    s.update(map_atom=np.full(n_vox, -777, np.int32), log_evidence=np.full(n_vox, -777.0), ess=np.full(n_vox, -777.0),
             clipped_mass=np.full(n_vox, -777.0))
    return s


def same_bytes(a, b, keys=POST_KEYS, sel=None):
    for k in keys:
        x, y = (a[k], b[k]) if sel is None else (a[k][..., sel], b[k][..., sel])
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), k


def accept_range(ref, got, nl_atoms, cp, sel):
    """varpro_posterior_reference.accept and the field_mean bound on the voxels `sel` only."""
    n = ref["finite"].shape[0]
    cut = {k: (v[sel] if isinstance(v, np.ndarray) and v.shape[:1] == (n,) else v) for k, v in ref.items()}
    q = accept(cut, {k: np.ascontiguousarray(got[k][..., sel]) for k in POST_KEYS}, nl_atoms)
    q["field_mean"] = LR.accept_field_mean(ref, got["field_mean"], got["mean"], cp, sel)
    return q


def field_case(gpu, c):
    """Sweep 0 on the device (the driver with no sweeps: the plain posterior and its field_mean), the field gathered from its
    field_mean over a random table, and the reference under it."""
    base, nl, lp = R.base_posterior(c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], **c["kw"])
    cp0 = LR.coupling_of(base, c["coupling"])
    pr = LR.precision_of(base, nl, lp, c["strength"], cp0)
    cp = LR.effective(cp0, pr)
    n_vox = c["y"].shape[0]
    nb = cases.table(n_vox, 8)
    zero = gpu.varpro_posterior_logmrf(c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], np.full((n_vox, 1), -1, np.int32),
                                       np.array([0, n_vox]), pr, cp, n_sweeps=0, **_kw(c))
    q, n = LR.gather(nb, zero["field_mean"], LR.centres(base, nl, lp, cp), pr)
    return dict(c, zero=zero, pr=pr, cp=cp, q=q, n=n, ref=LR.field_posterior(base, nl, lp, q, n, pr, cp), rng=LR.ranges(base, nl, lp, cp),
                base=base, lp=lp)


# ---- 1. the log-field posterior against the reference
@pytest.mark.parametrize("n_b", [4, 5, 33])
def test_logfield_posterior_on_every_range(gpu, n_b):
    """first x count out of 200 bi_s0 voxels; with an odd n_b the range's first signal row is only 8-byte aligned."""
    c = field_case(gpu, cases.range_case(n_b))
    n_free = len(c["lo"])
    worst = {}
    for first in FIRSTS:
        for count in COUNTS:
            got = logfield_on_device(gpu, c, c["q"], c["n"], c["pr"], c["cp"], first, count, sentinel(n_free, N_VOX))
            sel = np.arange(first, first + count)
            same_bytes(got, sentinel(n_free, N_VOX), keys=ALL_KEYS, sel=np.setdiff1d(np.arange(N_VOX), sel))  # nothing outside the range
            for k, v in accept_range(c["ref"], got, c["nl_atoms"], c["cp"], sel).items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("logfield posterior, n_b", n_b, "largest error / bound:", worst)


def _check_whole(gpu, name):
    c = field_case(gpu, cases.GPU_CASES[name]())
    n_vox = c["y"].shape[0]
    plain = gpu.varpro_posterior(c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], **_kw(c))
    same_bytes(c["zero"], plain)  # sweep 0: the plain posterior's bytes for every existing output
    got = logfield_on_device(gpu, c, c["q"], c["n"], c["pr"], c["cp"], 0, n_vox, c["zero"], want_delta=True)
    assert (c["n"] == 0).any() and (c["n"] == 8).any()  # field_n = 0 beside field_n = 8 within a strip
    print("logfield posterior", name, "largest error / bound:", accept_range(c["ref"], got, c["nl_atoms"], c["cp"], np.arange(n_vox)))
    # delta: the largest move of field_mean against sweep 0's, in units of the range of f
    rows = np.flatnonzero((c["pr"] > 0) & (c["rng"] > 0))
    fin = c["ref"]["finite"]
    if rows.size:
        move = np.abs(got["field_mean"][rows][:, fin] - c["zero"]["field_mean"][rows][:, fin]) / c["rng"][rows, None]
        assert got["delta"] == move.max() and got["delta"] > 0
    else:
        assert got["delta"] == 0.0
        same_bytes(got, c["zero"], keys=ALL_KEYS)
    return c, got


@pytest.mark.parametrize("n_atoms", [1, 17, "slab+16"])
@pytest.mark.parametrize("model", cases.MODELS)
def test_logfield_posterior_layouts_and_atoms(gpu, model, n_atoms):
    """All seven (K, class) pairs at 1 atom, 17 atoms and one LDS slab + 16 (the slab that carries the field rows)."""
    _check_whole(gpu, f"atoms-{model}-{n_atoms}")


@pytest.mark.parametrize("n_b", [16, 33, 128])
def test_logfield_posterior_free_t1_mixed_coupling(gpu, n_b):
    """K = 3 with a free T1, the rates log and T1 linear: both NS forms, the row-split form (16) and the two-pass form (33, 128)."""
    c, got = _check_whole(gpu, f"axes-{n_b}")
    assert c["cp"].tolist() == [0, 1, 0, 1, 1, 0]


@pytest.mark.parametrize("name", ["t1-tri_full-16", "t1-tri_s0-16", "t1-tri_full-33", "s0-33", "s0-128"])
def test_logfield_posterior_on_the_other_remedied_forms(gpu, name):
    """The forms whose fold differs from the linear kernel's beyond the added means: NS = 8, K = 3 with a free T1 in the free and the S0
    class (two rows per sweep), NS = 32, K = 3, free class with T1 and S0 class without (two passes: the second one writes field_mean
    and delta, both judged here)."""
    c, got = _check_whole(gpu, name)
    assert c["cp"].sum() == 3 and got["delta"] > 0


@pytest.mark.parametrize("noise_sd,marginal", [(0.0, False), (0.0, True), (cases.NOISE_SD, True), (cases.NOISE_SD, False)])
def test_logfield_posterior_noise_modes_and_weights(gpu, noise_sd, marginal):
    _check_whole(gpu, f"modes-{noise_sd}-{marginal}")


@pytest.mark.parametrize("name", ["sigma", "lead-inf", "nan"])
def test_logfield_posterior_sigma_excluded_atoms_and_a_non_finite_voxel(gpu, name):
    c, got = _check_whole(gpu, name)
    if name == "lead-inf":
        assert (got["map_atom"] >= 3).all()
    if name == "nan":
        assert np.isnan(got["field_mean"][:, [5, 40]]).all() and np.isfinite(got["field_mean"][:, [4, 6, 39, 41]]).all()


# ---- 2. byte equality
@pytest.mark.parametrize("name", ["driver", "axes-16", "axes-33"])
def test_all_linear_coupling_returns_the_linear_calls_bytes(gpu, name):
    c = cases.GPU_CASES[name]()
    base, nl, lp = R.base_posterior(c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], **c["kw"])
    pr = R.precision_of(base, nl, lp, c["strength"])
    n_free, n_vox = len(c["lo"]), c["y"].shape[0]
    cp = np.zeros(n_free, np.int32)
    plain = gpu.varpro_posterior(c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], **_kw(c))
    q, n = R.gather(cases.table(n_vox, 8), plain["mean"], R.centres(base, nl, lp), pr)
    start = dict(plain, field_mean=plain["mean"])
    want = logfield_on_device(gpu, c, q, n, pr, cp, 17, 60, start, want_delta=True, linear=True)
    got = logfield_on_device(gpu, c, q, n, pr, cp, 17, 60, start, want_delta=True)
    same_bytes(got, want)
    assert got["delta"] == want["delta"] > 0 and got["field_mean"].tobytes() == got["mean"].tobytes()
    # the driver
    nb, cs = _coloured(n_vox, (40, n_vox - 40))
    a = (c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], nb, cs, pr)
    want = gpu.varpro_posterior_mrf(*a, n_sweeps=2, **_kw(c))
    got = gpu.varpro_posterior_logmrf(*a, cp, n_sweeps=2, **_kw(c))
    same_bytes(got, want)
    assert got["delta"].tobytes() == want["delta"].tobytes() and got["field_mean"].tobytes() == got["mean"].tobytes()


@pytest.mark.parametrize("model,n_b", [("tri_s0", 16), ("tri_s0", 33), ("bi_reduced", 16), ("bi_reduced", 33), ("mono", 33)])
def test_zero_field_with_log_coupling_returns_the_posteriors_bytes(gpu, model, n_b):
    from varpro_posterior_reference import wide_box
    from varpro_reference import case_atoms, case_signals

    b, y = case_signals(model, N_VOX, n_b=n_b)
    y[7] = y[20] = np.nan  # outside and inside the range below
    lo, hi = wide_box(model)
    c = dict(model=model, b=b, y=y, nl_atoms=case_atoms(model)[:, :33], lo=lo, hi=hi, kw=dict(noise_sd=0.0, marginal=True))
    plain = gpu.varpro_posterior(model, b, y, c["nl_atoms"], lo, hi, **_kw(c))
    n_free = len(lo)
    nonlin = np.array([nme.startswith("D") for nme in api.MODEL_PARAM_NAMES[model]])
    pr, cp = np.where(nonlin, 1e3, 0.0), nonlin.astype(np.int32)
    rng = np.random.default_rng(1)
    rq, rn = rng.normal(size=(n_free, N_VOX)), rng.integers(0, 9, N_VOX).astype(np.int32)
    zq, zn = np.zeros((n_free, N_VOX)), np.zeros(N_VOX, np.int32)
    sel = np.arange(17, 100)
    for q, n, p, k in ((zq, zn, pr, cp), (rq, rn, np.zeros(n_free), np.zeros(n_free, np.int32)), (-zq, zn, pr, cp)):
        got = logfield_on_device(gpu, c, q, n, p, k, 17, 83, sentinel(n_free, N_VOX), want_delta=True)
        same_bytes(got, plain, sel=sel)  # clipped_mass included
        assert np.isfinite(got["delta"])
    assert np.isnan(plain["mean"][:, [7, 20]]).all() and np.isnan(got["field_mean"][:, 20]).all() and (got["field_mean"][:, 7] == -777.0).all()


def _compose(gpu, c, nb, start, pr, cp, n_sweeps):
    import torch

    kw = _kw(c)
    n_vox = c["y"].shape[0]
    zero = gpu.varpro_posterior_logmrf(c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], nb, start, pr, cp, n_sweeps=0, **kw)
    out = {k: _dev(zero[k]) for k in ALL_KEYS}
    n_free = zero["mean"].shape[0]
    yd, nbd = _dev(c["y"]), _dev(nb)
    fld = dict(field_q=_dev(np.zeros((n_free, n_vox))), field_n=_dev(np.zeros(n_vox, np.int32)))
    nonlinear = [nme.startswith("D") for nme in api.MODEL_PARAM_NAMES[c["model"]]]
    fcentre = api.varpro_logmrf_centre(c["nl_atoms"], nonlinear, cp, kw.get("log_prior"))[0]
    delta = []
    d = torch.zeros(1, dtype=torch.float64, device="cuda")
    for s in range(n_sweeps):
        worst = 0.0
        for col in range(len(start) - 1):
            first, count = int(start[col]), int(start[col + 1] - start[col])
            if count == 0:
                continue
            gpu.grid_neighbour_field(nbd, out["field_mean"], fcentre, pr, first=first, count=count, out=fld)
            gpu.varpro_posterior_logfield(c["model"], c["b"], yd, c["nl_atoms"], c["lo"], c["hi"], fld["field_q"], fld["field_n"], pr, cp, out,
                                          first=first, count=count, delta_max=d, **kw)
            torch.cuda.synchronize()
            worst = max(worst, float(d.cpu()[0]))
        delta.append(worst)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update(delta=delta, zero=zero)
    return res


def _coloured(n_vox, sizes, n_nb=6, seed=1):
    """A symmetric random graph whose edges run between different colour ranges only."""
    rng = np.random.default_rng(seed)
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    colour = np.repeat(np.arange(len(sizes)), sizes)
    nb = np.full((n_vox, n_nb), -1, np.int32)
    fill = np.zeros(n_vox, int)
    for _ in range(6 * n_vox):
        u, v = rng.integers(0, n_vox, 2)
        if colour[u] != colour[v] and fill[u] < n_nb and fill[v] < n_nb and v not in nb[u]:
            nb[u, fill[u]], nb[v, fill[v]] = v, u
            fill[u] += 1
            fill[v] += 1
    return nb, start


def _driver_inputs(n_vox):
    c = dict(cases.cases.driver_case(n_vox), coupling="log")
    nonlin = np.array([nme.startswith("D") for nme in api.MODEL_PARAM_NAMES[c["model"]]])
    cp = nonlin.astype(np.int32)
    rng = api.varpro_logmrf_centre(c["nl_atoms"], nonlin, cp)[1]
    pr = np.where(rng > 0, 16.0 / np.where(rng > 0, rng, 1.0) ** 2, 0.0)
    return c, pr, cp


@pytest.mark.parametrize("sizes", [(37, 46), (21, 0, 33, 29)])
def test_driver_equals_its_composition(gpu, sizes):
    import torch

    n_vox = sum(sizes)
    c, pr, cp = _driver_inputs(n_vox)
    c["y"][5] = np.nan  # a non-finite voxel: NaN everywhere, counts for nobody
    nb, start = _coloured(n_vox, sizes)
    args = (c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], nb, start, pr, cp)
    kw = _kw(c)
    want = _compose(gpu, c, nb, start, pr, cp, 3)
    got = gpu.varpro_posterior_logmrf(*args, n_sweeps=3, tol=0.0, **kw)
    same_bytes(got, want, keys=ALL_KEYS)
    assert got["n_sweeps"] == 3 and got["delta"].tolist() == want["delta"] and got["delta"][0] > 0  # delta exact against the composition
    assert np.isnan(got["mean"][:, 5]).all() and np.isnan(got["field_mean"][:, 5]).all() and got["map_atom"][5] == -1
    same_bytes(got, gpu.varpro_posterior_logmrf(*args, n_sweeps=3, **kw), keys=ALL_KEYS)  # two calls
    dev = gpu.varpro_posterior_logmrf(c["model"], c["b"], _dev(c["y"]), c["nl_atoms"], c["lo"], c["hi"], _dev(nb), start, pr, cp, n_sweeps=3, **kw)
    torch.cuda.synchronize()
    same_bytes(got, {k: dev[k].cpu().numpy() for k in ALL_KEYS}, keys=ALL_KEYS)  # PNX_MEM_HOST and PNX_MEM_DEVICE
    assert dev["delta"].tobytes() == got["delta"].tobytes()
    plain = gpu.varpro_posterior(c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], **kw)
    same_bytes(want["zero"], plain)  # sweep 0 alone: the plain posterior
    assert want["zero"]["n_sweeps"] == 0 and want["zero"]["delta"].size == 0
    # the driver against the reference's driver, inside its bounds
    state, rdelta, _ = LR.mrf(c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], nb, start, pr, cp, 3, **c["kw"])
    print("driver, largest error / bound:", accept_range(state, got, c["nl_atoms"], cp, np.arange(n_vox)))


def test_refusals_leave_the_device_usable(gpu):
    c, pr, cp = _driver_inputs(60)
    nb, start = _coloured(60, (30, 30))
    args = (c["model"], c["b"], c["y"], c["nl_atoms"], c["lo"], c["hi"], nb, start)
    kw = _kw(c)
    bad = cp.copy()
    bad[0] = 1  # tri_s0: f1
    with pytest.raises(_lib.PnxError, match=r"coupling\[0\]=1 on a fraction / S0 row must be 0") as e:
        gpu.varpro_posterior_logmrf(*args, pr, bad, **kw)
    assert e.value.code == -1
    atoms = c["nl_atoms"].copy()
    atoms[1, 4] = 0.0
    lo0 = c["lo"].copy()
    lo0[3] = -1.0  # a box that admits the zero rate: the variable projection's own atom check passes, the log row refuses
    with pytest.raises(_lib.PnxError, match=r"coupling\[3\]=1 \(log\) needs positive values: nl_atoms\[1, 4\]=0") as e:
        gpu.varpro_posterior_logmrf(c["model"], c["b"], c["y"], atoms, lo0, c["hi"], nb, start, pr, cp, **kw)
    assert e.value.code == -1
    ok = gpu.varpro_posterior_logmrf(*args, pr, cp, n_sweeps=1, **kw)  # and the device is fine afterwards: a valid call is correct
    same_bytes(ok, _compose(gpu, c, nb, start, pr, cp, 1), keys=ALL_KEYS)
    assert np.isfinite(ok["mean"]).all() and np.isfinite(ok["field_mean"]).all()


# ---- 3. the solver end to end
def test_solver_on_the_phantom(gpu):
    """phantom(seed=0, noise=0.05) through HipBayesVarProSolver(spatial_prior={strength 64, 6 sweeps, coupling "log"}): the caller's
    order, inside the reference's bounds, the three worth ratios <= 0.8, and the diagnostics."""
    ph = LR.phantom(seed=0, noise=0.05)
    names = ["f1", "D1", "D2", "S0"]
    rates = np.geomspace(3e-4, 0.3, 19)
    bounds = {n: (float(ph["lo"][i]), float(ph["hi"][i])) for i, n in enumerate(names)}
    common = dict(bounds=bounds, noise_sd=0.05)
    solver = HipBayesVarProSolver(BiExpModel(fit_s0=True), {"D1": list(rates), "D2": list(rates)}, spatial_prior={
        "strength": 64, "n_sweeps": 6, "coupling": "log", "connectivity": 4}, **common)
    plain = HipBayesVarProSolver(BiExpModel(fit_s0=True), {"D1": list(rates), "D2": list(rates)}, **common)
    assert np.array_equal(solver._nl_atoms, ph["nl_atoms"])
    solver.fit(ph["b"], ph["y"], neighbours=ph["nb"], colours=ph["colours"])
    plain.fit(ph["b"], ph["y"])
    d = solver.diagnostics_
    assert d["spatial_coupling"] == {"f1": "linear", "D1": "log", "D2": "log", "S0": "linear"} and d["spatial_sweeps"] == 6
    assert set(d["geo_mean"]) == {"D1", "D2"}
    mean = np.stack([np.asarray(solver.params_[n]) for n in names], axis=1)
    base = np.stack([np.asarray(plain.params_[n]) for n in names], axis=1)
    for n in ("D1", "D2"):  # exp E[log D] <= E[D] (Jensen), and both inside the rate axis
        g = d["geo_mean"][n]
        assert g.shape == (576,) and (g <= np.asarray(solver.params_[n]) * (1 + 1e-12)).all() and (g >= rates[0] * (1 - 1e-12)).all()
    # the reference in colour order, the device in the caller's: put the reference back
    order, snb, start = LR.colour_sort(ph["nb"], ph["colours"])
    args = ("bi_s0", ph["b"], ph["y"][order], ph["nl_atoms"], ph["lo"], ph["hi"])
    rb, nl, lp = R.base_posterior(*args, noise_sd=0.05, max_eps=1e-3)
    lam = LR.precision_of(rb, nl, lp, 64.0, LR.coupling_of(rb, "log"))
    assert [d["spatial_precision"][n] for n in names] == lam.tolist()
    state, rdelta, _ = LR.mrf(*args, snb, start, lam, "log", 6, noise_sd=0.05, max_eps=1e-3)
    got = dict(mean=mean.T[:, order], sd=np.stack([d["posterior_sd"][n] for n in names])[:, order],
               map_p=np.stack([d["map"][n] for n in names])[:, order], map_atom=d["map_atom"][order], log_evidence=d["log_evidence"][order],
               ess=d["ess"][order], clipped_mass=d["clipped_mass"][order])
    got["field_mean"] = np.array(got["mean"])
    for i, n in enumerate(names):
        if n in d["geo_mean"]:
            got["field_mean"][i] = np.log(d["geo_mean"][n][order])
    print("solver on the phantom, largest error / bound:", accept(state, got, ph["nl_atoms"]))
    err = np.abs(got["field_mean"].T - state["field_mean"])  # through exp and log: two more roundings of a value of magnitude <= |log 3e-4|
    assert (err <= state["bound_field_mean"] + 4 * 2.0 ** -52 * np.abs(state["field_mean"])).all()
    ratio = np.median(np.abs(mean - ph["truth"]), axis=0) / np.median(np.abs(base - ph["truth"]), axis=0)
    print("solver on the phantom: ratio to plain of the median |error| (f1, D1, D2, S0):", ratio)
    assert (ratio[:3] <= 0.8).all(), ratio

"""The edge-preserving (Student-t) neighbourhood prior of the grid posterior on the device (pnx_curvefit_grid_neighbour_wfield_f64,
pnx_curvefit_grid_posterior_wfield_f64, pnx_curvefit_grid_posterior_tmrf_f64) against tests/grid_tmrf_reference.py:
the weighted gather inside the bound derived there from the operation count, the weighted field posterior as the bytes of the
Gaussian one at integer weights and inside the reference's bounds at real ones, the driver as the bytes of its composition by hand,
HipBayesGridSolver's potential = "student_t" end to end, and what the potential is worth at the edge of the two-region phantom.
No tolerance of this file's own."""
from __future__ import annotations

import numpy as np
import pytest
import grid_mrf_reference as R
import grid_tmrf_reference as T
from grid_posterior_reference import accept
from test_gpu_grid_mrf import COUNTS, FIRSTS, N_VOX, POST_KEYS, _accept_range, _coloured, _dev, _same_bytes, _sentinel, _table
from test_gpu_grid_posterior import _case as _case_t1
from test_gpu_grid_prior import NOISE_SD

from pyneapple_amd import _lib, api
from pyneapple_amd.models import BiExpModel
from pyneapple_amd.solvers import HipBayesGridSolver

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1


# ---- 1. the weighted gather
def _gather_inputs(n_nb, n_vox=N_VOX, n_free=5):
    rng = np.random.default_rng(20 + n_nb)
    mean = rng.normal(0.3, 1.0, (n_free, n_vox))
    sd = rng.uniform(0.0, 0.8, (n_free, n_vox))
    sd[:, 7] = 0.0
    mean[:, 11] = np.nan  # a NaN neighbour: counts for nobody ...
    sd[:, 11] = np.nan
    mean[:, 40] = np.nan  # ... and a NaN own voxel inside every tested range below 41
    nb = _table(n_vox, n_nb)
    nb[5, 0] = 11
    nb[16, 0] = 11
    nb[40, 0] = 3
    centre, pr = rng.normal(0.3, 0.1, n_free), np.array([2.0, 0.0, 1e3, 0.5, 7.0])
    return nb, mean, sd, centre, pr


def _check_gather(ref, got, first, count, n_nb):
    sel = slice(first, first + count)
    assert got["field_n"][sel].tobytes() == ref["n"][sel].tobytes() and got["field_n"].dtype == np.int32
    assert (np.abs(got["field_q"][:, sel] - ref["q"][:, sel]) <= ref["bound_q"][:, sel]).all()
    assert (np.abs(got["field_w"][sel] - ref["w"][sel]) <= ref["bound_w"][sel]).all()
    if "edge_weight" in got:
        assert (np.abs(got["edge_weight"][sel] - ref["edge"][sel]) <= ref["bound_edge"][sel]).all()
        assert (got["edge_weight"][sel][ref["edge"][sel] == 0] == 0).all()  # exactly 0 in an absent slot
    with np.errstate(divide="ignore", invalid="ignore"):
        return max(float(np.nanmax(np.abs(got["field_q"][:, sel] - ref["q"][:, sel]) / ref["bound_q"][:, sel], initial=0.0)),
                   float(np.nanmax(np.abs(got["field_w"][sel] - ref["w"][sel]) / ref["bound_w"][sel], initial=0.0)))


@pytest.mark.parametrize("dof", [4.0, 0.5])
@pytest.mark.parametrize("n_nb", [1, 4, 6, 8])
def test_weighted_gather_on_every_range(gpu, n_nb, dof):
    import torch

    nb, mean, sd, centre, pr = _gather_inputs(n_nb)
    n_free = mean.shape[0]
    ref = T.gather(nb, mean, sd, centre, pr, dof)
    assert ref["n"][40] == 0 and ref["w"][40] == 0 and (ref["q"][:, 40] == 0).all() and (ref["n"] == 0).sum() > 1 and ref["n"].max() == n_nb
    whole = gpu.grid_neighbour_wfield(nb, mean, sd, centre, pr, dof, edge_weight=True)
    worst = _check_gather(ref, whole, 0, N_VOX, n_nb)
    nbd, md, sdd = _dev(nb), _dev(mean), _dev(sd)
    for first in FIRSTS:
        for count in COUNTS:
            sent = lambda: dict(field_q=_dev(np.full((n_free, N_VOX), -777.0)), field_w=_dev(np.full(N_VOX, -777.0)),
                                field_n=_dev(np.full(N_VOX, -777, np.int32)))
            with_e, without = sent(), sent()
            with_e["edge_weight"] = _dev(np.full((N_VOX, n_nb), -777.0))
            flag = _dev(np.array([INT_MAX], np.int32))
            gpu.grid_neighbour_wfield(nbd, md, sdd, centre, pr, dof, first=first, count=count, out=with_e, flag=flag)
            gpu.grid_neighbour_wfield(nbd, md, sdd, centre, pr, dof, first=first, count=count, out=without, flag=flag)
            torch.cuda.synchronize()
            a, b = ({k: v.cpu().numpy() for k, v in d.items()} for d in (with_e, without))
            for k in ("field_q", "field_w", "field_n"):  # edge_weight NULL and non-NULL: the same q, W and n
                assert a[k].tobytes() == b[k].tobytes(), k
            worst = max(worst, _check_gather(ref, a, first, count, n_nb))
            out = np.setdiff1d(np.arange(N_VOX), np.arange(first, first + count))
            assert (a["field_q"][:, out] == -777.0).all() and (a["field_w"][out] == -777.0).all() and (a["field_n"][out] == -777).all()
            assert (a["edge_weight"][out] == -777.0).all() and int(flag.cpu()[0]) == INT_MAX
            for k in ("field_q", "field_w", "field_n", "edge_weight"):  # and a range is the whole call's numbers
                assert np.ascontiguousarray(a[k][..., first:first + count] if k == "field_q" else a[k][first:first + count]).tobytes() == \
                    np.ascontiguousarray(whole[k][..., first:first + count] if k == "field_q" else whole[k][first:first + count]).tobytes(), k
    print(f"weighted gather n_nb={n_nb} dof={dof}: largest error / bound = {worst:.3f}")


def test_weighted_gather_reports_an_index_out_of_range_without_reading_it(gpu):
    import torch

    mean, sd = np.ones((3, 40)), np.full((3, 40), 0.1)
    for bad in (40, INT_MAX, -2, -(2 ** 31)):
        nb = np.full((40, 4), -1, np.int32)
        nb[9, 1], nb[23, 3], nb[9, 0] = bad, bad, 5
        with pytest.raises(_lib.PnxError, match="voxel 9 hold an index outside") as e:
            gpu.grid_neighbour_wfield(nb, mean, sd, np.zeros(3), np.ones(3), 4.0)
        assert e.value.code == -1
        flag = _dev(np.array([INT_MAX], np.int32))
        out = dict(field_q=_dev(np.zeros((3, 40))), field_w=_dev(np.zeros(40)), field_n=_dev(np.zeros(40, np.int32)),
                   edge_weight=_dev(np.full((40, 4), 5.0)))
        gpu.grid_neighbour_wfield(_dev(nb), _dev(mean), _dev(sd), np.zeros(3), np.ones(3), 4.0, first=10, count=30, out=out, flag=flag)
        torch.cuda.synchronize()
        assert int(flag.cpu()[0]) == 23 and int(out["field_n"].cpu()[23]) == 0 and float(out["field_w"].cpu()[23]) == 0.0
        assert (out["edge_weight"].cpu().numpy()[23] == 0.0).all() and int(out["field_n"].cpu()[9]) == 0


# ---- 2. the weighted field posterior
T1 = dict(t1_mode=1, tr=3000.0)
FORMS = [("bi_reduced", False, 16, {}), ("bi_reduced", False, 33, {}), ("mono", True, 16, {}), ("mono", True, 33, {}),  # NF = 3
         ("tri_reduced", False, 16, {}), ("tri_reduced", False, 33, {}), ("bi_s0", True, 16, {}), ("bi_s0", True, 33, {}),  # NF = 6
         ("tri_reduced", False, 128, {}),  # the wide register file at its limit
         ("tri_s0", True, 16, T1), ("tri_s0", True, 33, T1), ("tri_s0", False, 16, T1), ("tri_s0", False, 33, T1)]  # NF = 8 (7 rows)
_CASES = {}


def _wcase(gpu, model, project, n_b, noise_sd, extra):
    """83 voxels, 33 atoms with three -inf atoms in front; the reference is computed once per form and shared."""
    key = (model, project, n_b, noise_sd, tuple(extra))
    if key in _CASES:
        return _CASES[key]
    n_vox, n_atoms = 83, 33
    b, y, atoms, lo, hi = _case_t1(model, n_vox, n_atoms, n_b, **extra)
    lp = np.log(np.random.default_rng(9).uniform(0.1, 1.0, n_atoms))
    lp[:3] = -np.inf
    kw = dict(noise_sd=noise_sd, project_amplitude=project, log_prior=lp, **extra)
    plain = gpu.grid_posterior(model, b, y, atoms, lo, hi, **kw)
    base, atoms_f, lpf = R.base_posterior(model, b, y, atoms, lo, hi, log_prior=lp, noise_sd=noise_sd, project=project, **extra)
    row = -1 if base["s0_row"] is None else base["s0_row"]
    adm = lpf > -np.inf
    rng_k = atoms[:, adm].max(axis=1) - atoms[:, adm].min(axis=1)
    pr = 16.0 / rng_k ** 2
    if row >= 0:
        pr[row] = 0.0
    nb = _table(n_vox, 8)
    centre = R.centres(atoms, lp, row)
    q, n = R.gather(nb, plain["mean"], centre, pr)
    g = T.gather(nb, plain["mean"], plain["sd"], centre, pr, 4.0)
    w = g["w"].copy()  # real weights: the gather's own, then some below 1 and some above 8 where a neighbour is present
    some = np.flatnonzero(g["n"] > 0)
    w[some[0::3]] = 0.05 + 0.9 * np.random.default_rng(3).random(some[0::3].size)
    w[some[1::3]] = 8.5 + 3.0 * np.random.default_rng(4).random(some[1::3].size)
    assert (w[some] < 1).any() and (w > 8).any() and (w == 0).any() and (n == 0).any() and (n == 8).any()
    c = dict(b=b, y=y, atoms=atoms, lo=lo, hi=hi, kw=kw, plain=plain, pr=pr, q=q, n=n, gq=g["q"], w=w, rng=rng_k,
             ref=T.field_posterior(base, atoms_f, lpf, g["q"], w, pr))
    _CASES[key] = c
    return c


def _wfield(gpu, model, c, q, w, first, count, start, gaussian=False, want_delta=False):
    import torch

    out = {k: _dev(start[k]) for k in POST_KEYS}
    delta = torch.full((1,), -1.0, dtype=torch.float64, device="cuda") if want_delta else None
    call = gpu.grid_posterior_field if gaussian else gpu.grid_posterior_wfield
    call(model, c["b"], _dev(c["y"]), c["atoms"], c["lo"], c["hi"], _dev(q), _dev(w), c["pr"], out, first=first, count=count, delta_max=delta,
         **c["kw"])
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    if want_delta:
        res["delta"] = float(delta.cpu()[0])
    return res


@pytest.mark.parametrize("model,project,n_b,extra", FORMS)
@pytest.mark.parametrize("noise_sd", [0.0, NOISE_SD])
def test_weighted_field_posterior_is_the_gaussian_one_at_integer_weights(gpu, model, project, n_b, extra, noise_sd):
    c = _wcase(gpu, model, project, n_b, noise_sd, extra)
    want = _wfield(gpu, model, c, c["q"], c["n"], 0, 83, c["plain"], gaussian=True, want_delta=True)
    got = _wfield(gpu, model, c, c["q"], c["n"].astype(np.float64), 0, 83, c["plain"], want_delta=True)
    _same_bytes(got, want)
    assert got["delta"] == want["delta"] and got["delta"] > 0
    zero = _wfield(gpu, model, c, np.zeros_like(c["q"]), np.zeros(83), 0, 83, _sentinel(c["atoms"].shape[0], 83))
    _same_bytes(zero, c["plain"])  # a zero field with a zero weight: the plain posterior


@pytest.mark.parametrize("model,project,n_b,extra", FORMS)
@pytest.mark.parametrize("noise_sd", [0.0, NOISE_SD])
def test_weighted_field_posterior_at_real_weights(gpu, model, project, n_b, extra, noise_sd):
    c = _wcase(gpu, model, project, n_b, noise_sd, extra)
    got = _wfield(gpu, model, c, c["gq"], c["w"], 0, 83, c["plain"], want_delta=True)
    ratios = accept(c["ref"], got, c["atoms"])
    print(f"weighted field posterior: {model} n_b={n_b} project={project} noise_sd={noise_sd} rows={c['atoms'].shape[0]}: error / bound = {ratios}")
    rows = np.flatnonzero((c["pr"] > 0) & (c["rng"] > 0))
    fin = c["ref"]["finite"]
    move = np.abs(got["mean"][rows][:, fin] - c["plain"]["mean"][rows][:, fin]) / c["rng"][rows, None]
    assert got["delta"] == move.max() and got["delta"] > 0


def test_weighted_field_posterior_leaves_the_other_voxels_alone(gpu):
    model, project, n_b = "tri_reduced", False, 16
    c = _wcase(gpu, model, project, n_b, NOISE_SD, {})
    n_free = c["atoms"].shape[0]
    for first, count in ((0, 1), (15, 17), (17, 16), (16, 67), (1, 15)):
        got = _wfield(gpu, model, c, c["gq"], c["w"], first, count, _sentinel(n_free, 83))
        sel = np.arange(first, first + count)
        _same_bytes(got, _sentinel(n_free, 83), sel=np.setdiff1d(np.arange(83), sel))
        _accept_range(c["ref"], got, c["atoms"], sel)


# ---- 3. the driver is its composition
def _compose(gpu, model, b, y, atoms, lo, hi, nb, start, pr, dof, n_sweeps, **kw):
    import torch

    plain = gpu.grid_posterior(model, b, y, atoms, lo, hi, **kw)
    out = {k: _dev(plain[k]) for k in POST_KEYS}
    n_free, n_vox = plain["mean"].shape
    yd, nbd = _dev(y), _dev(nb)
    fld = dict(field_q=_dev(np.zeros((n_free, n_vox))), field_w=_dev(np.zeros(n_vox)), field_n=_dev(np.zeros(n_vox, np.int32)))
    row = api.MODEL_PARAM_NAMES[model].index("S0") if kw.get("project_amplitude") else -1
    centre = api.grid_mrf_centre(atoms, kw.get("log_prior"), row)
    delta = []
    d = torch.zeros(1, dtype=torch.float64, device="cuda")
    for _ in range(n_sweeps):
        worst = 0.0
        for c in range(len(start) - 1):
            first, count = int(start[c]), int(start[c + 1] - start[c])
            if count == 0:
                continue
            gpu.grid_neighbour_wfield(nbd, out["mean"], out["sd"], centre, pr, dof, first=first, count=count, out=fld)
            gpu.grid_posterior_wfield(model, b, yd, atoms, lo, hi, fld["field_q"], fld["field_w"], pr, out, first=first, count=count, delta_max=d,
                                      **kw)
            torch.cuda.synchronize()
            worst = max(worst, float(d.cpu()[0]))
        delta.append(worst)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update(delta=delta, plain=plain, field_w=fld["field_w"].cpu().numpy(), field_n=fld["field_n"].cpu().numpy())
    return res


@pytest.mark.parametrize("model,project,sizes", [("tri_reduced", False, (37, 46)), ("bi_s0", True, (19, 30, 17, 17)), ("bi_s0", True, (21, 0, 33, 29))])
def test_driver_equals_its_composition(gpu, model, project, sizes):
    import torch

    from test_gpu_grid_prior import _case

    n_vox, dof = sum(sizes), 4.0
    b, y, atoms, lo, hi = _case(model, n_vox, 33, 16)
    y[5] = np.nan  # a non-finite voxel: NaN everywhere, counts for nobody
    nb, start = _coloured(n_vox, sizes)
    rng_k = atoms.max(axis=1) - atoms.min(axis=1)
    pr = 16.0 / rng_k ** 2
    if project:
        pr[api.MODEL_PARAM_NAMES[model].index("S0")] = 0.0
    kw = dict(noise_sd=NOISE_SD, project_amplitude=project)
    keys = POST_KEYS + ("field_w", "field_n")
    want = _compose(gpu, model, b, y, atoms, lo, hi, nb, start, pr, dof, 3, **kw)
    got = gpu.grid_posterior_tmrf(model, b, y, atoms, lo, hi, nb, start, pr, dof, n_sweeps=3, **kw)
    _same_bytes(got, want, keys=keys)
    assert got["n_sweeps"] == 3 and got["delta"].tolist() == want["delta"] and got["delta"][0] > 0
    assert np.isnan(got["mean"][:, 5]).all() and got["map_atom"][5] == -1 and got["field_w"][5] == 0 and got["field_n"][5] == 0
    assert (got["field_w"][got["field_n"] > 0] > 0).all() and not (got["field_w"] == got["field_n"]).all()
    _same_bytes(got, gpu.grid_posterior_tmrf(model, b, y, atoms, lo, hi, nb, start, pr, dof, n_sweeps=3, **kw), keys=keys)  # two calls
    dev = gpu.grid_posterior_tmrf(model, b, _dev(y), atoms, lo, hi, _dev(nb), start, pr, dof, n_sweeps=3, **kw)  # device tensors
    torch.cuda.synchronize()
    _same_bytes(got, {k: dev[k].cpu().numpy() for k in keys}, keys=keys)
    assert dev["delta"].tobytes() == got["delta"].tobytes()
    zero = gpu.grid_posterior_tmrf(model, b, y, atoms, lo, hi, nb, start, pr, dof, n_sweeps=0, **kw)  # sweep 0 alone: the plain posterior
    _same_bytes(zero, want["plain"])
    assert zero["n_sweeps"] == 0 and zero["delta"].size == 0 and (zero["field_w"] == 0).all() and (zero["field_n"] == 0).all()
    none = gpu.grid_posterior_tmrf(model, b, y, atoms, lo, hi, nb, start, np.zeros_like(pr), dof, n_sweeps=2, **kw)  # K = 0
    _same_bytes(none, want["plain"])
    # the first sweep's delta against the reference's, within the mean bounds carried through one gather (the derivation is
    # grid_tmrf_reference.delta_tolerance's)
    one = gpu.grid_posterior_tmrf(model, b, y, atoms, lo, hi, nb, start, pr, dof, n_sweeps=1, **kw)
    rkw = dict(noise_sd=NOISE_SD, project=project)
    before, _, _ = T.tmrf(model, b, y, atoms, lo, hi, nb, start, pr, dof, 0, **rkw)
    after, delta_ref, _ = T.tmrf(model, b, y, atoms, lo, hi, nb, start, pr, dof, 1, **rkw)
    tol = T.delta_tolerance(before, after, atoms, np.zeros(atoms.shape[1]), pr, dof, nb.shape[1])
    print(f"driver {model} {sizes}: delta device {one['delta'][0]!r} reference {delta_ref[0]!r} tolerance {tol:.3e}")
    assert tol < 1e-3 * delta_ref[0] and abs(one["delta"][0] - delta_ref[0]) <= tol


def test_driver_argument_errors_are_no_faults(gpu):
    from test_gpu_grid_prior import _case

    b, y, atoms, lo, hi = _case("tri_reduced", 60, 17, 16)
    nb, start = _coloured(60, (30, 30))
    pr = np.ones(5)
    bad = nb.copy()
    bad[3, 0], bad[31, 0] = 7, 40  # edges inside a colour
    with pytest.raises(_lib.PnxError, match="voxel 3 has a neighbour inside its own colour") as e:
        gpu.grid_posterior_tmrf("tri_reduced", b, y, atoms, lo, hi, bad, start, pr, 4.0)
    assert e.value.code == -1
    for index in (60, INT_MAX, -2):
        bad = nb.copy()
        bad[44, 2] = index
        with pytest.raises(_lib.PnxError, match="voxel 44 hold an index outside") as e:
            gpu.grid_posterior_tmrf("tri_reduced", b, y, atoms, lo, hi, bad, start, pr, 4.0)
        assert e.value.code == -1
    with pytest.raises(_lib.PnxError, match="dof") as e:
        gpu.grid_posterior_tmrf("tri_reduced", b, y, atoms, lo, hi, nb, start, pr, 0.0)
    ok = gpu.grid_posterior_tmrf("tri_reduced", b, y, atoms, lo, hi, nb, start, pr, 4.0, n_sweeps=1)  # and the device is fine afterwards
    assert np.isfinite(ok["mean"]).all()


# ---- 4. through the solver
def test_solver_end_to_end_on_the_small_phantom(gpu):
    """The 12 x 12 phantom through HipBayesGridSolver.fit: the results in the caller's order inside the reference's bounds, the new
    diagnostics, and a voxel at the region's edge with a lower edge weight than the median."""
    ph = R.phantom(seed=0, noise=0.05, H=12, W=12)
    f, D1, D2 = np.linspace(0.05, 0.5, 8), np.geomspace(0.005, 0.1, 8), np.geomspace(0.0005, 0.003, 8)
    names = ["f1", "D1", "D2"]
    bounds = {n: (float(a), float(b)) for n, a, b in zip(names, ph["lo"], ph["hi"])}
    sp = {"strength": 64, "n_sweeps": 2, "connectivity": 4, "potential": "student_t", "dof": 4.0}
    solver = HipBayesGridSolver(BiExpModel(fit_reduced=True), {"f1": f, "D1": D1, "D2": D2}, bounds=bounds, noise_sd=0.05, spatial_prior=sp)
    assert solver._atoms.tobytes() == ph["atoms"].tobytes()
    solver.fit(ph["b"], ph["y"], neighbours=ph["nb"], colours=ph["colours"])
    d = solver.diagnostics_
    order, nb, start = R.colour_sort(ph["nb"], ph["colours"])
    lam = 64.0 / (ph["atoms"].max(axis=1) - ph["atoms"].min(axis=1)) ** 2
    ref, delta_ref, _ = T.tmrf("bi_reduced", ph["b"], ph["y"][order], ph["atoms"], ph["lo"], ph["hi"], nb, start, lam, 4.0, 2, noise_sd=0.05)
    got = dict(mean=np.stack([np.asarray(solver.params_[n])[order] for n in names]), sd=np.stack([d["posterior_sd"][n][order] for n in names]),
               map_p=np.stack([d["map"][n][order] for n in names]), map_atom=d["map_atom"][order], log_evidence=d["log_evidence"][order],
               ess=d["ess"][order])
    print("solver, student_t, 2 sweeps: error / bound =", accept(ref, got, ph["atoms"]))
    assert d["spatial_potential"] == "student_t" and d["spatial_dof"] == 4.0 and d["spatial_sweeps"] == 2
    assert [d["spatial_precision"][n] for n in names] == lam.tolist()
    ew = d["spatial_edge_weight"]
    drv = gpu.grid_posterior_tmrf("bi_reduced", ph["b"], ph["y"][order], ph["atoms"], ph["lo"], ph["hi"], nb, start, lam, 4.0, n_sweeps=2,
                                  noise_sd=0.05)
    assert ew.shape == (144,) and np.isfinite(ew).all() and (ew > 0).all() and (ew <= 1).all() and (drv["field_n"] >= 2).all()
    assert ew[order].tobytes() == (drv["field_w"] / drv["field_n"] * (4.0 / (4.0 + 3))).tobytes()  # W_v / n_v scaled by nu / (nu + K)
    assert d["spatial_delta"].tobytes() == drv["delta"].tobytes()
    region = (ph["truth"][:, 0] == 0.30)
    edge = np.array([(ph["nb"][v][ph["nb"][v] >= 0].size and (region[ph["nb"][v][ph["nb"][v] >= 0]] != region[v]).any()) for v in range(144)], bool)
    print("edge weight: median", np.median(ew), "edge voxels", np.sort(ew[edge])[:5], "inner median", np.median(ew[~edge]))
    assert edge.sum() > 0 and ew[edge].min() < np.median(ew)
    gauss = HipBayesGridSolver(BiExpModel(fit_reduced=True), {"f1": f, "D1": D1, "D2": D2}, bounds=bounds, noise_sd=0.05,
                               spatial_prior={"strength": 64, "n_sweeps": 2, "connectivity": 4})
    gauss.fit(ph["b"], ph["y"], neighbours=ph["nb"], colours=ph["colours"])
    assert gauss.diagnostics_["spatial_potential"] == "gaussian" and gauss.diagnostics_["spatial_dof"] is None
    assert "spatial_edge_weight" not in gauss.diagnostics_
    assert all(np.abs(np.asarray(solver.params_[n]) - np.asarray(gauss.params_[n])).max() > 0 for n in names)


# ---- 5. what it is worth at the edge
def test_worth_at_the_edge_of_the_two_region_phantom(gpu):
    """24 x 24, 5 % noise, strength 64, dof 4, 6 sweeps, seed 0, the 92 voxels with a neighbour in the other region: the medians of
    |error| of D1 and D2 under the Student-t prior are at most 0.9 of the Gaussian prior's -- first on the reference alone, then
    on the device.  f1 and the other voxels are printed, not asserted."""
    ph = R.phantom(seed=0, noise=0.05)
    order, nb, start = R.colour_sort(ph["nb"], ph["colours"])
    y, truth = ph["y"][order], ph["truth"][order]
    region = truth[:, 0] == 0.30
    edge = ((nb >= 0) & (region[np.maximum(nb, 0)] != region[:, None])).any(axis=1)
    assert edge.sum() == 92
    lam = 64.0 / (ph["atoms"].max(axis=1) - ph["atoms"].min(axis=1)) ** 2
    args = ("bi_reduced", ph["b"], y, ph["atoms"], ph["lo"], ph["hi"], nb, start, lam)
    err = lambda mean, sel: np.median(np.abs(mean[sel] - truth[sel]), axis=0)
    ref_g, _, _ = R.mrf(*args, 6, noise_sd=0.05)
    ref_t, _, _ = T.tmrf(*args, 4.0, 6, noise_sd=0.05)
    ratio_ref = err(ref_t["mean"], edge) / err(ref_g["mean"], edge)
    print("reference, edge voxels: gaussian", err(ref_g["mean"], edge), "student_t", err(ref_t["mean"], edge), "ratios f1 / D1 / D2", ratio_ref)
    print("reference, other voxels: ratios", err(ref_t["mean"], ~edge) / err(ref_g["mean"], ~edge))
    assert (ratio_ref[1:] <= 0.9).all()
    got_g = gpu.grid_posterior_mrf(*args, n_sweeps=6, noise_sd=0.05)
    got_t = gpu.grid_posterior_tmrf(*args, 4.0, n_sweeps=6, noise_sd=0.05)
    ratio = err(got_t["mean"].T, edge) / err(got_g["mean"].T, edge)
    print("device, edge voxels: gaussian", err(got_g["mean"].T, edge), "student_t", err(got_t["mean"].T, edge), "ratios f1 / D1 / D2", ratio)
    print("device, other voxels: ratios", err(got_t["mean"].T, ~edge) / err(got_g["mean"].T, ~edge), "delta", got_t["delta"])
    assert (ratio[1:] <= 0.9).all() and got_t["n_sweeps"] == 6

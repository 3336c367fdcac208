"""The neighbourhood (MRF) prior of the grid posterior on the device (pnx_curvefit_grid_neighbour_field_f64,
pnx_curvefit_grid_posterior_field_f64, pnx_curvefit_grid_posterior_mrf_f64) against tests/grid_mrf_reference.py:
the gather byte for byte, the field posterior inside the posterior's own bounds with eps_v enlarged by the field's rounding (the
derivation is in the reference file; no tolerance of this file's own), a zero field and the driver's sweep 0 as the bytes of
api.grid_posterior, the driver as the bytes of its composition by hand, argument errors that are no faults, what the prior is
worth on the two-region phantom, and HipBayesGridSolver's spatial_prior end to end.

The largest error-to-bound ratios observed are recorded in DESIGN.md 4.1p."""
from __future__ import annotations

import numpy as np
import pytest
import grid_mrf_reference as R
from grid_posterior_reference import accept
from test_gpu_grid_prior import NOISE_SD, PROJ, _case

from pyneapple_amd import _lib, api
from pyneapple_amd.fitters import HipPixelWiseFitter
from pyneapple_amd.models import BiExpModel
from pyneapple_amd.solvers import HipBayesGridSolver

pytestmark = pytest.mark.gpu

POST_KEYS = ("mean", "sd", "map_p", "map_atom", "log_evidence", "ess")
N_VOX = 200
FIRSTS, COUNTS = (0, 1, 15, 16, 17), (1, 15, 16, 17, 83)


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _table(n_vox, n_nb, seed=3):
    """A random table: -1 slots in front, in the middle and at the end, voxels with no neighbour at all beside full ones."""
    rng = np.random.default_rng(seed + n_nb)
    nb = rng.integers(0, n_vox, (n_vox, n_nb)).astype(np.int32)
    nb[rng.random((n_vox, n_nb)) < 0.3] = -1
    nb[0::7, 0] = -1
    nb[1::7, n_nb // 2] = -1
    nb[2::7, -1] = -1
    nb[3::7] = -1  # field_n = 0 ...
    nb[4::7] = rng.integers(0, n_vox, nb[4::7].shape)  # ... beside full rows in one strip
    return nb


def _field_on_device(gpu, model, b, y, atoms, lo, hi, q, n, pr, first, count, start, want_delta=False, **kw):
    """One field posterior over [first, first + count) on device tensors that start as the arrays of `start`; numpy out."""
    import torch

    out = {k: _dev(start[k]) for k in POST_KEYS}
    delta = torch.full((1,), -1.0, dtype=torch.float64, device="cuda") if want_delta else None
    gpu.grid_posterior_field(model, b, _dev(y), atoms, lo, hi, _dev(q), _dev(n), pr, out, first=first, count=count, delta_max=delta, **kw)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    if want_delta:
        res["delta"] = float(delta.cpu()[0])
    return res


def _sentinel(n_free, n_vox):
    s = {k: np.full((n_free, n_vox), -777.0) for k in ("mean", "sd", "map_p")}
    s.update(map_atom=np.full(n_vox, -777, np.int32), log_evidence=np.full(n_vox, -777.0), ess=np.full(n_vox, -777.0))
    return s


def _same_bytes(a, b, keys=POST_KEYS, sel=None):
    for k in keys:
        x, y = (a[k], b[k]) if sel is None else (a[k][..., sel], b[k][..., sel])
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), k


def _accept_range(ref, got, atoms, sel):
    """grid_posterior_reference.accept on the voxels `sel` only: every voxel of the range counts."""
    cut = {k: (v[sel] if isinstance(v, np.ndarray) and v.shape[:1] == ref["finite"].shape else v) for k, v in ref.items()}
    return accept(cut, {k: np.ascontiguousarray(got[k][..., sel]) for k in POST_KEYS}, atoms)


# ---- 1. the gather
@pytest.mark.parametrize("n_nb", [1, 4, 6, 8])
def test_gather_is_numpy_in_slot_order(gpu, n_nb):
    import torch

    rng = np.random.default_rng(n_nb)
    n_free, n_vox = 5, 150
    mean = rng.normal(0.3, 1.0, (n_free, n_vox))
    mean[:, 11] = np.nan  # a non-finite voxel counts for nobody
    mean[:, 40] = np.nan
    nb = _table(n_vox, n_nb)
    nb[5, 0] = 11
    centre, pr = rng.normal(0.3, 0.1, n_free), np.array([2.0, 0.0, 1e3, 0.5, 7.0])
    q, n = R.gather(nb, mean, centre, pr)
    got = gpu.grid_neighbour_field(nb, mean, centre, pr)
    assert got["field_q"].tobytes() == q.tobytes() and got["field_n"].tobytes() == n.tobytes() and got["field_n"].dtype == np.int32
    for first, count in ((0, n_vox), (17, 70), (149, 1), (64, 0)):  # the voxels outside the range stay untouched, host and device
        out = dict(field_q=np.full((n_free, n_vox), -777.0), field_n=np.full(n_vox, -777, np.int32))
        gpu.grid_neighbour_field(nb, mean, centre, pr, first=first, count=count, out=out)
        dq, dn = _dev(np.full((n_free, n_vox), -777.0)), _dev(np.full(n_vox, -777, np.int32))
        flag = _dev(np.array([2 ** 31 - 1], np.int32))
        gpu.grid_neighbour_field(_dev(nb), _dev(mean), centre, pr, first=first, count=count, out=dict(field_q=dq, field_n=dn), flag=flag)
        torch.cuda.synchronize()
        want_q, want_n = np.full((n_free, n_vox), -777.0), np.full(n_vox, -777, np.int32)
        want_q[:, first:first + count], want_n[first:first + count] = q[:, first:first + count], n[first:first + count]
        for gq, gn in ((out["field_q"], out["field_n"]), (dq.cpu().numpy(), dn.cpu().numpy())):
            assert gq.tobytes() == want_q.tobytes() and gn.tobytes() == want_n.tobytes()
        assert int(flag.cpu()[0]) == 2 ** 31 - 1


def test_gather_reports_an_index_out_of_range_without_reading_it(gpu):
    import torch

    mean = np.ones((3, 40))
    for bad in (40, 2 ** 31 - 1, -2, -(2 ** 31)):
        nb = np.full((40, 4), -1, np.int32)
        nb[9, 1], nb[23, 3], nb[9, 0] = bad, bad, 5
        with pytest.raises(_lib.PnxError, match="voxel 9 hold an index outside") as e:
            gpu.grid_neighbour_field(nb, mean, np.zeros(3), np.ones(3))
        assert e.value.code == -1
        flag, out = _dev(np.array([2 ** 31 - 1], np.int32)), dict(field_q=_dev(np.zeros((3, 40))), field_n=_dev(np.zeros(40, np.int32)))
        gpu.grid_neighbour_field(_dev(nb), _dev(mean), np.zeros(3), np.ones(3), first=10, count=30, out=out, flag=flag)
        torch.cuda.synchronize()
        assert int(flag.cpu()[0]) == 23 and int(out["field_n"].cpu()[23]) == 0 and int(out["field_n"].cpu()[9]) == 0


# ---- 2. the field posterior against the reference
def _field_case(gpu, model, project, n_atoms, n_b, noise_sd, lead_inf=0, n_vox=N_VOX):
    b, y, atoms, lo, hi = _case(model, n_vox, n_atoms, n_b)
    lp = None
    if lead_inf:
        lp = np.log(np.random.default_rng(9).uniform(0.1, 1.0, n_atoms))
        lp[:lead_inf] = -np.inf
    kw = dict(noise_sd=noise_sd, project_amplitude=project, log_prior=lp)
    plain = gpu.grid_posterior(model, b, y, atoms, lo, hi, **kw)
    base, atoms_f, lpf = R.base_posterior(model, b, y, atoms, lo, hi, log_prior=lp, noise_sd=noise_sd, project=project)
    row = -1 if base["s0_row"] is None else base["s0_row"]
    adm = lpf > -np.inf
    rng_k = atoms[:, adm].max(axis=1) - atoms[:, adm].min(axis=1)
    pr = np.where(rng_k > 0, 16.0 / np.where(rng_k > 0, rng_k, 1.0) ** 2, 0.0)
    if row >= 0:
        pr[row] = 0.0
    nb = _table(n_vox, 8)
    q, n = R.gather(nb, plain["mean"], R.centres(atoms, lp, row), pr)
    ref = R.field_posterior(base, atoms_f, lpf, q, n, pr)
    return dict(b=b, y=y, atoms=atoms, lo=lo, hi=hi, kw=kw, plain=plain, pr=pr, q=q, n=n, ref=ref, rng=rng_k)


@pytest.mark.parametrize("n_b", [1, 3, 33])
def test_field_posterior_on_every_range(gpu, n_b):
    """first x count out of 200 voxels; with an odd n_b the range's first signal row is only 8-byte aligned."""
    model, project = "tri_reduced", False
    c = _field_case(gpu, model, project, 33, n_b, NOISE_SD)
    n_free = c["atoms"].shape[0]
    worst = {}
    for first in FIRSTS:
        for count in COUNTS:
            got = _field_on_device(gpu, model, c["b"], c["y"], c["atoms"], c["lo"], c["hi"], c["q"], c["n"], c["pr"], first, count,
                                   _sentinel(n_free, N_VOX), **c["kw"])
            sel = np.arange(first, first + count)
            out = np.setdiff1d(np.arange(N_VOX), sel)
            _same_bytes(got, _sentinel(n_free, N_VOX), sel=out)  # nothing outside the range is touched
            for k, v in _accept_range(c["ref"], got, c["atoms"], sel).items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("field posterior, n_b", n_b, "largest error / bound:", worst)


@pytest.mark.parametrize("model,project", PROJ)
@pytest.mark.parametrize("noise_sd", [0.0, NOISE_SD])
@pytest.mark.parametrize("n_atoms", [1, 17, "slab+16"])
def test_field_posterior_atoms_modes_and_projection(gpu, model, project, noise_sd, n_atoms):
    n_b = 16
    n_free = len(api.MODEL_PARAM_NAMES[model])
    if n_atoms == "slab+16":
        n_atoms = api.grid_mrf_slab_atoms(n_b, n_free) + 16  # a second slab with one tile
    lead = 0 if n_atoms == 1 else 3  # -inf atoms in front
    c = _field_case(gpu, model, project, n_atoms, n_b, noise_sd, lead_inf=lead, n_vox=83)
    got = _field_on_device(gpu, model, c["b"], c["y"], c["atoms"], c["lo"], c["hi"], c["q"], c["n"], c["pr"], 0, 83, c["plain"],
                           want_delta=True, **c["kw"])
    assert (c["n"] == 0).any() and (c["n"] == 8).any()  # field_n = 0 beside field_n = 8
    q = accept(c["ref"], got, c["atoms"])
    print("field posterior", model, noise_sd, n_atoms, "largest error / bound:", q)
    # delta: the largest move of a mean against the plain posterior's, in units of the row's range, inside the two mean bounds
    rows = np.flatnonzero((c["pr"] > 0) & (c["rng"] > 0))
    fin = c["ref"]["finite"]
    if rows.size:
        move = np.abs(got["mean"][rows][:, fin] - c["plain"]["mean"][rows][:, fin]) / c["rng"][rows, None]
        assert got["delta"] == move.max()
    else:
        assert got["delta"] == 0.0


def test_field_posterior_on_a_narrow_axis_far_from_zero(gpu):
    """S0 on 1000 .. 1000.01, unprojected: uncentred, thetac q would cancel twelve digits; the centred form keeps the bound."""
    rng = np.random.default_rng(4)
    b = np.array([0, 10, 20, 40, 80, 150, 300, 500, 800.0, 1000, 1200, 1500])
    s0, d = np.linspace(1000.0, 1000.01, 9), np.geomspace(5e-4, 3e-3, 7)
    atoms = np.stack(np.meshgrid(s0, d, indexing="ij"), -1).reshape(-1, 2).T.copy()
    lo, hi = np.array([999.0, 1e-4]), np.array([1001.0, 1e-2])
    truth_s0, truth_d = rng.uniform(1000.002, 1000.008, 83), rng.uniform(8e-4, 2e-3, 83)
    y = truth_s0[:, None] * np.exp(-b * truth_d[:, None]) + 20.0 * rng.standard_normal((83, b.size))
    kw = dict(noise_sd=20.0, project_amplitude=False, log_prior=None)
    plain = gpu.grid_posterior("mono", b, y, atoms, lo, hi, **kw)
    base, atoms_f, lpf = R.base_posterior("mono", b, y, atoms, lo, hi, noise_sd=20.0)
    pr = 64.0 / (atoms.max(axis=1) - atoms.min(axis=1)) ** 2
    around = plain["mean"].copy()  # neighbours spread over the narrow range: the data say little about S0 at this noise, the field much
    around[0] = rng.uniform(1000.0, 1000.01, 83)
    q, n = R.gather(_table(83, 8), around, R.centres(atoms), pr)
    got = _field_on_device(gpu, "mono", b, y, atoms, lo, hi, q, n, pr, 0, 83, plain, **kw)
    print("narrow axis, largest error / bound:", accept(R.field_posterior(base, atoms_f, lpf, q, n, pr), got, atoms))
    # eight neighbours at strength 64 pull towards their average, which lies about 0.1 of the range off the centre
    assert np.abs(got["mean"][0] - plain["mean"][0]).max() > 1e-3 * 0.01


# ---- 3. a zero field is the plain posterior
@pytest.mark.parametrize("model,project", PROJ)
@pytest.mark.parametrize("noise_sd", [0.0, NOISE_SD])
def test_zero_field_returns_the_posteriors_bytes(gpu, model, project, noise_sd):
    c = _field_case(gpu, model, project, 33, 16, noise_sd)
    n_free = c["atoms"].shape[0]
    sel = np.arange(17, 100)
    zq, zn = np.zeros((n_free, N_VOX)), np.zeros(N_VOX, np.int32)
    for q, n, pr in ((zq, zn, c["pr"]), (c["q"], c["n"], np.zeros(n_free)), (-zq, zn, c["pr"])):
        got = _field_on_device(gpu, model, c["b"], c["y"], c["atoms"], c["lo"], c["hi"], q, n, pr, 17, 83, _sentinel(n_free, N_VOX),
                               want_delta=True, **c["kw"])
        _same_bytes(got, c["plain"], sel=sel)
        assert np.isfinite(got["delta"])


# ---- 4. the driver is its composition
def _compose(gpu, model, b, y, atoms, lo, hi, nb, start, pr, n_sweeps, tol, **kw):
    import torch

    plain = gpu.grid_posterior(model, b, y, atoms, lo, hi, **kw)
    out = {k: _dev(plain[k]) for k in POST_KEYS}
    n_free, n_vox = plain["mean"].shape
    yd, nbd = _dev(y), _dev(nb)
    fld = dict(field_q=_dev(np.zeros((n_free, n_vox))), field_n=_dev(np.zeros(n_vox, np.int32)))
    row = api.MODEL_PARAM_NAMES[model].index("S0") if kw.get("project_amplitude") else -1
    centre = api.grid_mrf_centre(atoms, kw.get("log_prior"), row)
    delta, done = [], 0
    d = torch.zeros(1, dtype=torch.float64, device="cuda")
    for s in range(n_sweeps):
        worst = 0.0
        for c in range(len(start) - 1):
            first, count = int(start[c]), int(start[c + 1] - start[c])
            if count == 0:
                continue
            gpu.grid_neighbour_field(nbd, out["mean"], centre, pr, first=first, count=count, out=fld)
            gpu.grid_posterior_field(model, b, yd, atoms, lo, hi, fld["field_q"], fld["field_n"], pr, out, first=first, count=count, delta_max=d, **kw)
            torch.cuda.synchronize()
            worst = max(worst, float(d.cpu()[0]))
        delta.append(worst)
        done = s + 1
        if tol > 0 and worst <= tol:
            break
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update(delta=delta, n_sweeps=done, plain=plain)
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


@pytest.mark.parametrize("model,project", PROJ)
@pytest.mark.parametrize("sizes", [(37, 46), (21, 0, 33, 29), (19, 30, 17, 17)])
def test_driver_equals_its_composition(gpu, model, project, sizes):
    import torch

    n_vox = sum(sizes)
    b, y, atoms, lo, hi = _case(model, n_vox, 33, 16)
    y[5] = np.nan  # a non-finite voxel: NaN everywhere, counts for nobody
    nb, start = _coloured(n_vox, sizes)
    rng_k = atoms.max(axis=1) - atoms.min(axis=1)
    pr = 16.0 / rng_k ** 2
    if project:
        pr[api.MODEL_PARAM_NAMES[model].index("S0")] = 0.0
    kw = dict(noise_sd=NOISE_SD, project_amplitude=project)
    want = _compose(gpu, model, b, y, atoms, lo, hi, nb, start, pr, 3, 0.0, **kw)
    got = gpu.grid_posterior_mrf(model, b, y, atoms, lo, hi, nb, start, pr, n_sweeps=3, tol=0.0, **kw)
    _same_bytes(got, want)
    assert got["n_sweeps"] == 3 and got["delta"].tolist() == want["delta"] and got["delta"][0] > 0
    assert np.isnan(got["mean"][:, 5]).all() and got["map_atom"][5] == -1
    _same_bytes(got, gpu.grid_posterior_mrf(model, b, y, atoms, lo, hi, nb, start, pr, n_sweeps=3, **kw))  # two calls
    dev = gpu.grid_posterior_mrf(model, b, _dev(y), atoms, lo, hi, _dev(nb), start, pr, n_sweeps=3, **kw)  # device tensors
    torch.cuda.synchronize()
    _same_bytes(got, {k: dev[k].cpu().numpy() for k in POST_KEYS})
    assert dev["delta"].tobytes() == got["delta"].tobytes()
    zero = gpu.grid_posterior_mrf(model, b, y, atoms, lo, hi, nb, start, pr, n_sweeps=0, **kw)  # sweep 0 alone: the plain posterior
    _same_bytes(zero, want["plain"])
    assert zero["n_sweeps"] == 0 and zero["delta"].size == 0
    # the tol stop: after the first sweep whose delta is at most tol; the rest of delta is NaN
    tol = float(want["delta"][1])
    stop = gpu.grid_posterior_mrf(model, b, y, atoms, lo, hi, nb, start, pr, n_sweeps=3, tol=tol, **kw)
    early = _compose(gpu, model, b, y, atoms, lo, hi, nb, start, pr, 3, tol, **kw)
    assert stop["n_sweeps"] == early["n_sweeps"] == 2 and stop["delta"][:2].tolist() == early["delta"] and np.isnan(stop["delta"][2])
    _same_bytes(stop, early)
    # delta recomputed from the composed means of one more sweep
    one = _compose(gpu, model, b, y, atoms, lo, hi, nb, start, pr, 1, 0.0, **kw)
    fin = np.isfinite(one["plain"]["mean"][0])
    rows = np.flatnonzero(pr > 0)
    moves = []
    state = one["plain"]["mean"].copy()
    for c in range(len(sizes)):  # colour after colour: a voxel's old mean is the one before its own colour's update
        sel = np.arange(start[c], start[c + 1])[fin[start[c]:start[c + 1]]]
        if sel.size:
            moves.append((np.abs(one["mean"][rows][:, sel] - state[rows][:, sel]) / rng_k[rows, None]).max())
    assert one["delta"] == [max(moves)]


def test_driver_argument_errors_are_no_faults(gpu):
    b, y, atoms, lo, hi = _case("tri_reduced", 60, 17, 16)
    nb, start = _coloured(60, (30, 30))
    pr = np.ones(5)
    bad = nb.copy()
    bad[3, 0], bad[31, 0] = 7, 40  # 3 -> 7 and 31 -> 40: edges inside a colour
    with pytest.raises(_lib.PnxError, match="voxel 3 has a neighbour inside its own colour") as e:
        gpu.grid_posterior_mrf("tri_reduced", b, y, atoms, lo, hi, bad, start, pr)
    assert e.value.code == -1
    for index in (60, 2 ** 31 - 1, -2):
        bad = nb.copy()
        bad[44, 2] = index
        with pytest.raises(_lib.PnxError, match="voxel 44 hold an index outside") as e:
            gpu.grid_posterior_mrf("tri_reduced", b, y, atoms, lo, hi, bad, start, pr)
        assert e.value.code == -1
    ok = gpu.grid_posterior_mrf("tri_reduced", b, y, atoms, lo, hi, nb, start, pr, n_sweeps=1)  # and the device is fine afterwards
    assert np.isfinite(ok["mean"]).all()


# ---- 5. what it is worth
def test_worth_on_the_two_region_phantom(gpu):
    """24 x 24, 5 % noise, strength 64, 6 sweeps, seed 0: the medians of |error| of f1, D1, D2 under the MRF are at most 0.9 of the
    plain posterior's -- first on the reference alone (0.74 / 0.66 / 0.65 there), then on the device."""
    ph = R.phantom(seed=0, noise=0.05)
    order, nb, start = R.colour_sort(ph["nb"], ph["colours"])
    y, truth = ph["y"][order], ph["truth"][order]
    lam = 64.0 / (ph["atoms"].max(axis=1) - ph["atoms"].min(axis=1)) ** 2
    args = ("bi_reduced", ph["b"], y, ph["atoms"], ph["lo"], ph["hi"], nb, start, lam)
    ref0, _, _ = R.mrf(*args, 0, noise_sd=0.05)
    ref6, _, _ = R.mrf(*args, 6, noise_sd=0.05)
    err = lambda mean: np.median(np.abs(mean - truth), axis=0)
    ratio_ref = err(ref6["mean"]) / err(ref0["mean"])
    print("reference: plain", err(ref0["mean"]), "mrf", err(ref6["mean"]), "ratios", ratio_ref)
    assert (ratio_ref <= 0.9).all()
    got0 = gpu.grid_posterior_mrf(*args, n_sweeps=0, noise_sd=0.05)
    got6 = gpu.grid_posterior_mrf(*args, n_sweeps=6, noise_sd=0.05)
    ratio = err(got6["mean"].T) / err(got0["mean"].T)
    print("device: plain", err(got0["mean"].T), "mrf", err(got6["mean"].T), "ratios", ratio, "delta", got6["delta"])
    assert (ratio <= 0.9).all() and got6["n_sweeps"] == 6


# ---- 6. through the plugin
def test_through_the_fitter(gpu):
    rng = np.random.default_rng(2)
    b = np.array([0, 10, 30, 60, 120, 250, 500, 800.0])
    names = ["f1", "D1", "D2"]
    grid = {"f1": np.linspace(0.05, 0.5, 6), "D1": np.geomspace(0.01, 0.1, 5), "D2": np.geomspace(0.0005, 0.003, 5)}
    bounds = {"f1": (0.0, 1.0), "D1": (0.005, 0.5), "D2": (0.0001, 0.01)}
    sig = 0.2 * np.exp(-b * 0.03) + 0.8 * np.exp(-b * 0.001)
    image = sig + 0.05 * rng.standard_normal((6, 5, 4, 8))
    seg = np.ones((6, 5, 4), int)
    seg[0, :3, 0] = 0
    seg[4, 2, 1:3] = 0
    sp = {"strength": {"f1": 16.0, "D1": 16.0, "D2": 4.0}, "n_sweeps": 3, "connectivity": 6}
    solver = HipBayesGridSolver(BiExpModel(fit_reduced=True), grid, bounds=bounds, noise_sd=0.05, spatial_prior=sp)
    plain = HipBayesGridSolver(BiExpModel(fit_reduced=True), grid, bounds=bounds, noise_sd=0.05)
    assert solver.needs_neighbours and not plain.needs_neighbours
    HipPixelWiseFitter(solver).fit(b, image, segmentation=seg)
    HipPixelWiseFitter(plain).fit(b, image, segmentation=seg)
    mask = seg != 0
    pix = np.ascontiguousarray(image[mask])
    nb, col = api.grid_neighbours(mask, 6)
    order, snb, start = R.colour_sort(nb, col)
    atoms = solver._atoms
    lo, hi = np.array([bounds[n][0] for n in names]), np.array([bounds[n][1] for n in names])
    pr = np.array([sp["strength"][n] for n in names]) / (atoms.max(axis=1) - atoms.min(axis=1)) ** 2
    want = gpu.grid_posterior_mrf("bi_reduced", b, pix[order], atoms, lo, hi, snb, start, pr, n_sweeps=3, noise_sd=0.05)
    d = solver.diagnostics_
    assert d["spatial_sweeps"] == 3 and d["spatial_delta"].tobytes() == want["delta"].tobytes()
    assert [d["spatial_precision"][n] for n in names] == pr.tolist()
    for i, n in enumerate(names):
        assert np.asarray(solver.params_[n])[order].tobytes() == want["mean"][i].tobytes()
        assert d["posterior_sd"][n][order].tobytes() == want["sd"][i].tobytes()
    assert d["map_atom"][order].tobytes() == want["map_atom"].tobytes() and d["n_pixels"] == mask.sum() == 115
    # under spatial_prior the results differ from a solver without it (an option that is swallowed would leave them equal)
    assert all(np.abs(np.asarray(solver.params_[n]) - np.asarray(plain.params_[n])).max() > 0 for n in names)
    assert "spatial_sweeps" not in plain.diagnostics_

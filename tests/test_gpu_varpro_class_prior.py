"""pnx_curvefit_varpro_posterior_classes_f64 and pnx_curvefit_varpro_prior_em_classes_f64 on the device (one prior row per
segmentation label over the variable-projection dictionary) against tests/varpro_class_prior_reference.py: byte
equality with the unlabelled calls where the sums are the same sums, the references' bounds where they are not (the varpro
posterior's per-voxel bound, grid_prior_reference.step_bounds per class, (2^t - 1) single-step bounds after t <= 3 updates -- no
tolerance of this file's own), exclusions per row, labels out of range, reproducibility, what the per-label table is worth, and
HipBayesVarProSolver's per_label end to end.

Shapes: 65 voxels (strips of 16: four full and one voxel), the case dictionaries of tests/varpro_reference.py (28 pairs for bi_s0),
16 b-values unless stated.  The largest error-to-bound ratios observed are recorded in DESIGN.md 4.1o."""
from __future__ import annotations

import functools

import numpy as np
import pytest
from grid_prior_reference import em_step, step_bounds
from test_gpu_varpro_prior import _accept, _singular_case
from varpro_class_prior_reference import accept_em, normalise_rows, posterior, same_start, two_populations, worth
from varpro_marginal_cases import NOISE_SD
from varpro_marginal_cases import _case as _case32
from varpro_posterior_reference import accept, ratios, reference
from varpro_prior_cases import call_kw, cases, ref_kw, wide_pairs
from varpro_prior_reference import likelihoods, normalise

from pyneapple_amd import api
from pyneapple_amd.fitters import HipPixelWiseFitter
from pyneapple_amd.models import BiExpModel
from pyneapple_amd.solvers import HipBayesVarProSolver

pytestmark = pytest.mark.gpu

MODELS = ["bi_s0", "tri_reduced"]
# (noise_sd, marginal_amplitudes): both noise modes and both amplitude weights
MODES = [(0.0, True), (NOISE_SD, True), (0.0, False), (NOISE_SD, False)]
POST_KEYS = ("mean", "sd", "map_p", "map_atom", "log_evidence", "ess", "clipped_mass")
EM_KEYS = ("log_prior", "loglik", "loglik_class", "n_eff")


def _case(model, n_vox, n_b=16, **kw):
    """varpro_marginal_cases._case at 16 b-values by default.  With 16 b-values or fewer the case dictionaries hold neighbouring rates
    whose columns are close to dependent: the reference's eps_v reaches 6.6e-4 there (2.7e-7 at 32), so those cases state the
    reference's wider precondition eps_v <= 1e-3 -- its bounds are computed from the eps_v it finds, not from the cap."""
    c = _case32(model, n_vox, n_b=n_b, **kw)
    if n_b <= 16:
        c["max_eps"] = 1e-3
    return c


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _rows(n_classes, n_atoms, seed=5):
    """Random finite rows, not normalised: the library normalises."""
    return np.log(np.random.default_rng(seed).uniform(0.01, 1.0, (n_classes, n_atoms))) + 2.5


def _same_bytes(a, b, keys, idx=None):
    for k in keys:
        x, y = (a[k], b[k]) if idx is None else (a[k][..., idx[0]], b[k][..., idx[1]])
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), k


def _args(c):
    return c["model"], c["b"], c["y"], c["atoms"], c["lo"], c["hi"]


def _special():
    """One case each with a sigma vector and a free T1, taken from varpro_prior_cases."""
    c = cases()
    return [c["sigma"], c["free-t1"]]


# ---- 1. one class is the unlabelled call, byte for byte
@pytest.mark.parametrize("model", MODELS)
def test_one_class_returns_the_unlabelled_bytes(gpu, model):
    for n_b in (16, 33):  # both register-file instantiations: n_b <= 32 and <= 128
        for noise_sd, marginal in MODES:
            c = _case(model, 65, n_b=n_b, noise_sd=noise_sd, marginal=marginal)
            G = c["atoms"].shape[1]
            lab = np.zeros(65, np.int32)
            for prior in (None, _rows(1, G)):
                flat = None if prior is None else prior[0]
                _same_bytes(gpu.varpro_posterior_classes(*_args(c), lab, 1, log_prior=prior, **call_kw(c)),
                            gpu.varpro_posterior(*_args(c), log_prior=flat, **call_kw(c)), POST_KEYS)
                for alpha in (0.0, 0.5):
                    em = dict(n_iter=3, pseudo_count=alpha, rel_tol=0.0, **call_kw(c))
                    one = gpu.varpro_prior_em_classes(*_args(c), lab, 1, log_prior=prior, **em)
                    ref = gpu.varpro_prior_em(*_args(c), log_prior=flat, **em)
                    assert one["log_prior"].shape == (1, G) and one["log_prior"][0].tobytes() == ref["log_prior"].tobytes()
                    assert one["loglik"].tobytes() == ref["loglik"].tobytes() and one["loglik_class"][:, 0].tobytes() == ref["loglik"].tobytes()
                    assert one["n_iter"] == ref["n_iter"] == 3 and one["n_eff"].tolist() == [ref["n_eff"]]


def test_one_class_sigma_and_free_t1(gpu):
    for c in _special():
        lab = np.zeros(c["y"].shape[0], np.int32)
        _same_bytes(gpu.varpro_posterior_classes(*_args(c), lab, 1, **call_kw(c)), gpu.varpro_posterior(*_args(c), **call_kw(c)), POST_KEYS)
        em = dict(n_iter=3, rel_tol=0.0, **call_kw(c))
        one, ref = gpu.varpro_prior_em_classes(*_args(c), lab, 1, **em), gpu.varpro_prior_em(*_args(c), **em)
        assert one["log_prior"][0].tobytes() == ref["log_prior"].tobytes() and one["loglik"].tobytes() == ref["loglik"].tobytes()


# ---- 2. the posterior with classes mixed inside every strip
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n_classes", [3, 16])
def test_posterior_under_each_voxels_own_row(gpu, model, n_classes):
    lab = (np.arange(65) % n_classes).astype(np.int32)
    for noise_sd, marginal in MODES:
        c = _case(model, 65, n_b=16, noise_sd=noise_sd, marginal=marginal)
        rows = _rows(n_classes, c["atoms"].shape[1])
        got = gpu.varpro_posterior_classes(*_args(c), lab, n_classes, log_prior=rows, **call_kw(c))
        accept(posterior(*_args(c), lab, n_classes, log_prior=rows, **ref_kw(c)), got, c["atoms"])
        for k in range(n_classes):  # a voxel's sums depend on the order of the atoms only
            idx = np.flatnonzero(lab == k)
            _same_bytes(got, gpu.varpro_posterior(*_args(c), log_prior=rows[k], **call_kw(c)), POST_KEYS, (idx, idx))


def test_posterior_sigma_and_free_t1(gpu):
    for c in _special():
        n, G = c["y"].shape[0], c["atoms"].shape[1]
        lab = (np.arange(n) % 3).astype(np.int32)
        rows = _rows(3, G)
        got = gpu.varpro_posterior_classes(*_args(c), lab, 3, log_prior=rows, **call_kw(c))
        accept(posterior(*_args(c), lab, 3, log_prior=rows, **ref_kw(c)), got, c["atoms"])


# ---- 3. rows that exclude different atoms
@pytest.mark.parametrize("model", MODELS)
def test_exclusions_per_row(gpu, model):
    """Row 0 excludes the whole first tile and one atom more (its first admissible atom comes late), row 1 every atom but the last,
    row 2 none; the labels are interleaved.  An excluded pair weighs exactly 0: seen through map_atom, ess and the EM's -inf.  The
    moments are centred over the union of the rows' atoms, so mean and sd are not held to the per-row reference here; the outputs
    that do not depend on the centre are byte-equal to the unlabelled call under the row."""
    lab = (np.arange(65) % 3).astype(np.int32)
    for noise_sd, marginal in MODES:
        c = _case(model, 65, n_b=16, noise_sd=noise_sd, marginal=marginal)
        G = c["atoms"].shape[1]
        rows = _rows(3, G)
        rows[0, :17] = -np.inf
        rows[1, :G - 1] = -np.inf
        got = gpu.varpro_posterior_classes(*_args(c), lab, 3, log_prior=rows, **call_kw(c))
        for k in POST_KEYS:
            assert not np.isnan(got[k]).any(), k
        assert (got["map_atom"][lab == 0] >= 17).all() and (got["map_atom"][lab == 1] == G - 1).all() and (got["map_atom"] >= 0).all()
        assert (got["ess"][lab == 1] == 1.0).all()
        ref = posterior(*_args(c), lab, 3, log_prior=rows, **ref_kw(c))
        assert (got["sd"][np.ix_(ref["nl_rows"], np.flatnonzero(lab == 1))] == 0.0).all()  # one atom carries the posterior
        q = ratios(ref, got)
        print("error / bound:", q)
        assert q["log_evidence"] <= 1.0 and q["ess"] <= 1.0 and q["clipped_mass"] <= 1.0
        assert (ref["l"][np.arange(65), got["map_atom"]] >= ref["l"].max(axis=1) - 2 * ref["eps"]).all()
        for k in range(3):
            idx = np.flatnonzero(lab == k)
            _same_bytes(got, gpu.varpro_posterior(*_args(c), log_prior=rows[k], **call_kw(c)), ("map_atom", "ess", "log_evidence", "clipped_mass"),
                        (idx, idx))
        for alpha in (0.0, 0.5):
            em = gpu.varpro_prior_em_classes(*_args(c), lab, 3, log_prior=rows, n_iter=3, pseudo_count=alpha, rel_tol=0.0, **call_kw(c))
            assert not np.isnan(em["log_prior"]).any() and np.isfinite(em["loglik"]).all() and np.isfinite(em["loglik_class"]).all()
            assert (em["log_prior"][np.isinf(rows)] == -np.inf).all()
            assert em["log_prior"][1, G - 1] == 0.0  # the one admissible atom of row 1 holds all of its mass
            if alpha:
                assert np.isfinite(em["log_prior"][np.isfinite(rows)]).all()
            l0, eps0, fin = likelihoods(*_args(c), **ref_kw(c))
            accept_em(em, l0, eps0, fin, lab, normalise_rows(rows, 3, G), alpha, 3)


def test_singular_atoms_are_inadmissible_in_every_row(gpu):
    """4.1m's dictionary with two atoms whose N is exactly singular, two classes, the amplitudes marginalised: those atoms are -inf in
    every row whatever the start says, n_adm_c leaves them out (seen through the pseudo count's floor), and a voxel's MAP is never
    one of them."""
    c, sing, good = _singular_case(True)
    lab = (np.arange(70) % 2).astype(np.int32)
    rows = _rows(2, 30)
    rows[1, :3] = -np.inf
    rest = np.setdiff1d(np.arange(30), sing)
    em = gpu.varpro_prior_em_classes(*_args(c), lab, 2, log_prior=rows, n_iter=1, rel_tol=0.0, pseudo_count=0.5, **call_kw(c))
    lp = em["log_prior"]
    assert (lp[:, sing] == -np.inf).all() and np.isfinite(lp[0, rest]).all() and (lp[1, :3] == -np.inf).all() and em["n_eff"].tolist() == [35, 35]
    for k, n_adm in ((0, 28), (1, 25)):
        adm = np.isfinite(lp[k])
        assert adm.sum() == n_adm and abs(np.exp(lp[k, adm]).sum() - 1.0) <= 1e-12
        assert (lp[k, adm] >= np.log(0.5 / (35 + 0.5 * n_adm)) - 1e-12).all()  # n_adm_c counts neither the singular nor the excluded atoms
    # numpy on the dictionary without them, from the rows the library normalised over all 30 atoms
    l0, eps0, fin = likelihoods(c["model"], c["b"], c["y"], good, c["lo"], c["hi"], **ref_kw(c))
    accept_em(dict(em, log_prior=np.ascontiguousarray(lp[:, rest])), l0, eps0, fin, lab, normalise_rows(rows, 2, 30)[:, rest], 0.5, 1)
    post = gpu.varpro_posterior_classes(*_args(c), lab, 2, log_prior=rows, **call_kw(c))
    assert not np.isin(post["map_atom"], sing).any() and (post["map_atom"] >= 0).all() and (post["map_atom"][lab == 1] >= 3).all()
    # a class whose finite entries all sit on such atoms has no voxel that takes part
    only = np.full((2, 30), -np.inf)
    only[0, sing] = 0.0
    only[1] = 0.0
    lone = gpu.varpro_prior_em_classes(*_args(c), lab, 2, log_prior=only, n_iter=1, rel_tol=0.0, **call_kw(c))
    assert lone["n_eff"].tolist() == [0, 35] and lone["loglik_class"][0, 0] == 0.0 and (lone["log_prior"][0] == -np.inf).all()
    lost = gpu.varpro_posterior_classes(*_args(c), lab, 2, log_prior=only, **call_kw(c))
    assert (lost["map_atom"][lab == 0] == -1).all() and np.isnan(lost["mean"][:, lab == 0]).all() and (lost["map_atom"][lab == 1] >= 0).all()


# ---- 4. labels out of range mark voxels that take no part
@pytest.mark.parametrize("model", MODELS)
def test_labels_out_of_range(gpu, model):
    lab = (np.arange(65) % 3).astype(np.int32)
    out = np.array([0, 15, 16, 64])
    lab[out] = [-1, 3, -1, 3]
    keep = np.setdiff1d(np.arange(65), out)
    for noise_sd, marginal in MODES[:2]:
        c = _case(model, 65, n_b=16, noise_sd=noise_sd, marginal=marginal)
        model_, b, y, atoms, lo, hi = _args(c)
        G = atoms.shape[1]
        rows = _rows(3, G)
        got = gpu.varpro_posterior_classes(*_args(c), lab, 3, log_prior=rows, **call_kw(c))
        assert (got["map_atom"][out] == -1).all()
        for k in ("mean", "sd", "map_p", "log_evidence", "ess", "clipped_mass"):
            assert np.isnan(got[k][..., out]).all(), k
        less = gpu.varpro_posterior_classes(model_, b, np.ascontiguousarray(y[keep]), atoms, lo, hi, lab[keep], 3, log_prior=rows, **call_kw(c))
        _same_bytes(got, less, POST_KEYS, (keep, np.arange(61)))
        em = gpu.varpro_prior_em_classes(*_args(c), lab, 3, log_prior=rows, n_iter=1, rel_tol=0.0, **call_kw(c))
        assert em["n_eff"].tolist() == [int((lab == k).sum()) for k in range(3)] and em["n_eff"].sum() == 61
        l0, eps0, fin = likelihoods(*_args(c), **ref_kw(c))
        accept_em(em, l0, eps0, fin & (lab >= 0) & (lab < 3), lab, normalise_rows(rows, 3, G), 0.0, 1)
    none = gpu.varpro_prior_em_classes(*_args(c), np.full(65, -1, np.int32), 3, log_prior=rows, n_iter=3, **call_kw(c))
    assert none["n_iter"] == 0 and none["n_eff"].tolist() == [0, 0, 0] and none["loglik"][0] == 0.0 and np.isnan(none["loglik"][1:]).all()
    assert all(same_start(none["log_prior"][k], normalise_rows(rows, 3, G)[k]) for k in range(3))


# ---- 5. the EM against numpy: four rows, the last without a voxel; every strip mixed, and one class per strip
def _labels(kind, n_vox):
    lab = np.arange(n_vox) % 3
    return (np.sort(lab) if kind == "sorted" else lab).astype(np.int32)


def _em(gpu, c, kind, steps, alpha, prior=None):
    lab = _labels(kind, c["y"].shape[0])
    got = gpu.varpro_prior_em_classes(*_args(c), lab, 4, log_prior=prior, n_iter=steps, pseudo_count=alpha, rel_tol=0.0, **call_kw(c))
    start = gpu.varpro_prior_em_classes(*_args(c), np.full(len(lab), -1, np.int32), 4, log_prior=prior, n_iter=1, **call_kw(c))["log_prior"]
    assert got["log_prior"][3].tobytes() == start[3].tobytes()  # the class without a voxel: the library's normalised start, untouched
    l0, eps0, fin = likelihoods(*_args(c), **ref_kw(c))
    return accept_em(got, l0, eps0, fin, lab, normalise_rows(prior, 4, c["atoms"].shape[1]), alpha, steps)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("kind", ["mixed", "sorted"])
@pytest.mark.parametrize("n_vox", [1, 15, 16, 17, 65])
def test_one_step_voxel_axis(gpu, n_vox, kind, model):
    for noise_sd, marginal in MODES[:2]:
        _em(gpu, _case(model, n_vox, n_b=16, noise_sd=noise_sd, marginal=marginal), kind, 1, 0.0)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("kind", ["mixed", "sorted"])
@pytest.mark.parametrize("n_atoms", [17, "slab + 16"])
def test_one_step_atom_axis(gpu, n_atoms, kind, model):
    """The second: two slabs of this call's own width (four rows at 32 b-values), the second partly filled."""
    k = 2 if model.startswith("bi") else 3
    if n_atoms == "slab + 16":
        n_atoms = api.varpro_class_slab_atoms(32, k, 4, 16) + 16
    atoms = wide_pairs(n_atoms) if k == 2 else _case(model, 1)["atoms"][:, :n_atoms]
    assert atoms.shape[1] == n_atoms
    for (noise_sd, marginal), alpha in zip(MODES[1:3], (0.0, 0.5)):
        _em(gpu, _case(model, 65, n_b=32, atoms=atoms, noise_sd=noise_sd, marginal=marginal), kind, 1, alpha, prior=_rows(4, n_atoms))


@pytest.mark.parametrize("kind", ["mixed", "sorted"])
def test_one_step_more_voxel_groups_than_blocks(gpu, kind):
    n_vox = 2 * _cus() * 64 + 69
    _em(gpu, _case("bi_s0", n_vox, n_b=8, atoms=wide_pairs(48), noise_sd=NOISE_SD), kind, 1, 0.0)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("kind", ["mixed", "sorted"])
def test_three_steps_against_numpy(gpu, kind, model):
    atoms = wide_pairs(100) if model == "bi_s0" else None  # tri_reduced: the case dictionary (64 triples)
    for (noise_sd, marginal), alpha in zip(MODES[:2], (0.5, 0.0)):
        _em(gpu, _case(model, 300, n_b=16, atoms=atoms, noise_sd=noise_sd, marginal=marginal), kind, 3, alpha)


def test_one_step_sigma_and_free_t1(gpu):
    for c in _special():
        _em(gpu, c, "mixed", 1, 0.0)


# ---- 6. reproducible, and the same from device memory
@pytest.mark.parametrize("model", MODELS)
def test_two_calls_and_device_arrays_return_equal_bytes(gpu, model):
    import torch

    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    lab = _labels("mixed", 300)
    for noise_sd, marginal in MODES[:2]:
        c = _case(model, 300, n_b=16, noise_sd=noise_sd, marginal=marginal)
        model_, b, y, atoms, lo, hi = _args(c)
        rows = _rows(4, atoms.shape[1])
        yd, ld = torch.from_numpy(y).to(dev), torch.from_numpy(lab).to(dev)
        o = api.make_opts(model, len(b), jac="analytic")
        n_free = len(lo)
        one = gpu.varpro_prior_em_classes(*_args(c), lab, 4, log_prior=rows, n_iter=3, rel_tol=0.0, **call_kw(c))
        two = gpu.varpro_prior_em_classes(*_args(c), lab, 4, log_prior=rows, n_iter=3, rel_tol=0.0, **call_kw(c))
        three = api.varpro_prior_em_classes_device(o, 300, b, yd, atoms, None, lo, hi, ld, 4, rows, noise_sd, marginal, 3, 0.0, 0.0, 0, st)
        for other in (two, three):
            _same_bytes(one, other, EM_KEYS)
        p1 = gpu.varpro_posterior_classes(*_args(c), lab, 4, log_prior=rows, **call_kw(c))
        p2 = gpu.varpro_posterior_classes(*_args(c), lab, 4, log_prior=rows, **call_kw(c))
        t = {k: torch.empty((n_free, 300), dtype=torch.float64, device=dev) for k in ("mean", "sd", "map_p")}
        t["map_atom"] = torch.empty(300, dtype=torch.int32, device=dev)
        t["log_evidence"], t["ess"], t["clipped_mass"] = (torch.empty(300, dtype=torch.float64, device=dev) for _ in range(3))
        api.varpro_posterior_classes_device(o, 300, b, yd, atoms, None, lo, hi, ld, 4, rows, noise_sd, marginal, t["mean"], t["sd"],
                                            t["map_atom"], t["map_p"], t["log_evidence"], t["ess"], t["clipped_mass"], 0, st)
        torch.cuda.synchronize(dev)
        _same_bytes(p1, p2, POST_KEYS)
        _same_bytes(p1, {k: v.cpu().numpy() for k, v in t.items()}, POST_KEYS)


# ---- 7. what it is worth
@functools.lru_cache(maxsize=None)
def _worth(noise_sd):
    return worth(noise_sd, 3)


def _drift(l0, eps0, part, lp, steps):
    """The derived distance of a row after `steps` library updates to the all-numpy row: (2^t - 1) single-step bounds."""
    d = 0.0
    for _ in range(steps):
        S, nxt, _ = em_step(l0, lp, part)
        d = 2 * d + step_bounds(l0, lp, eps0, part, S)["lp"]
        lp = nxt
    return d


@pytest.mark.parametrize("noise_sd", [0.0, 0.05])
def test_it_earns_its_keep(gpu, noise_sd):
    """1000 + 1000 voxels of two narrow bi_s0 populations with the same fractions whose rates differ modestly
    (varpro_class_prior_reference.two_populations), 5 % noise, the 91-atom dictionary of 4.1m's claim, three updates each; the
    compared figure is the median |error| of the posterior mean of f1.  The library's tables are held to numpy's by (2^3 - 1)
    single-step bounds, its posterior means to the reference's under its own tables by the posterior's bound, and its two medians to
    the reference's two by the largest of those bounds plus what the tables' distance moves a mean by.  The inequality per_label <
    single is asserted on the library only where the reference shows at least a 10 % gain: a condition on the input, checked on the
    CPU in tests/test_varpro_class_prior_host.py, which records the reference's medians."""
    w = _worth(noise_sd)
    b, y, lab, atoms, lo, hi = w["data"]
    G = atoms.shape[1]
    kw = dict(noise_sd=noise_sd)
    per = gpu.varpro_prior_em_classes("bi_s0", b, y, atoms, lo, hi, lab, 2, n_iter=3, rel_tol=0.0, **kw)
    one = gpu.varpro_prior_em("bi_s0", b, y, atoms, lo, hi, n_iter=3, rel_tol=0.0, **kw)
    l0, eps0, fin = likelihoods("bi_s0", b, y, atoms, lo, hi, noise_sd=noise_sd)
    accept_em(per, l0, eps0, fin, lab, normalise_rows(None, 2, G), 0.0, 3)
    _accept(one, l0, eps0, fin, normalise(None, G), 0.0, 3)
    eta_per = max(_drift(l0, eps0, fin & (lab == k), normalise(None, G), 3) for k in range(2))
    eta_one = _drift(l0, eps0, fin, normalise(None, G), 3)
    m_per = gpu.varpro_posterior_classes("bi_s0", b, y, atoms, lo, hi, lab, 2, log_prior=per["log_prior"], **kw)
    m_one = gpu.varpro_posterior("bi_s0", b, y, atoms, lo, hi, log_prior=one["log_prior"], **kw)
    r_per = posterior("bi_s0", b, y, atoms, lo, hi, lab, 2, log_prior=per["log_prior"], noise_sd=noise_sd)
    r_one = reference("bi_s0", b, y, atoms, lo, hi, log_prior=one["log_prior"], noise_sd=noise_sd)
    accept(r_per, m_per, atoms)
    accept(r_one, m_one, atoms)
    truth = w["truth"][0]
    med = lambda mean: float(np.median(np.abs(mean - truth)))
    got_per, got_one = med(m_per["mean"][0]), med(m_one["mean"][0])
    # a median moves by at most the largest move of an element: the posterior's bound under the library's own tables, and the
    # tables' derived distance eta to numpy's, just asserted (a table moved by eta moves the weights by e^{+-2 eta}, a mean by
    # expm1(2 eta) x the range of the voxel's f1 over the atoms)
    for got, ref, lib_ref, eta in ((got_per, w["per_label"], r_per, eta_per), (got_one, w["single"], r_one, eta_one)):
        f1 = lib_ref["lin"][:, :, 0]
        span = float((f1.max(axis=1) - f1.min(axis=1)).max())
        bound = float(lib_ref["bound_mean"][:, 0].max()) + float(np.expm1(2 * eta)) * span
        print(f"median |error| of f1: library {got!r}, reference {ref!r}, bound {bound:.3g}")
        assert abs(got - ref) <= bound
    if w["per_label"] <= 0.9 * w["single"]:  # the condition on the input
        assert got_per < got_one


# ---- 8. through the plugin
def test_through_the_fitter(gpu):
    b, y, _, lab, atoms, lo, hi = two_populations(64)
    names = ["f1", "D1", "D2", "S0"]
    bounds = {n: (float(lo[i]), float(hi[i])) for i, n in enumerate(names)}
    rates = np.geomspace(3e-4, 0.3, 14)
    solver = HipBayesVarProSolver(BiExpModel(fit_s0=True), rates={"D1": rates, "D2": rates}, bounds=bounds, noise_sd=0.05,
                                  empirical_prior={"per_label": True, "n_iter": 5})
    nl = solver._nl_atoms
    assert solver.needs_labels and nl.shape == (2, 91)
    image = y.reshape(8, 8, 2, 16)
    seg = np.where(lab == 0, 3, 7).reshape(8, 8, 2)
    seg[0, :4, 0] = 0  # masked out
    fitter = HipPixelWiseFitter(solver)
    fitter.fit(b, image, segmentation=seg)
    mask = seg != 0
    rows = np.where(seg[mask] == 3, 0, 1).astype(np.int32)
    pix = np.ascontiguousarray(image[mask])
    em = gpu.varpro_prior_em_classes("bi_s0", b, pix, nl, lo, hi, rows, 2, n_iter=5, pseudo_count=0.0, rel_tol=1e-6, noise_sd=0.05)
    want = gpu.varpro_posterior_classes("bi_s0", b, pix, nl, lo, hi, rows, 2, log_prior=em["log_prior"], noise_sd=0.05)
    d = solver.diagnostics_
    assert d["prior_labels"] == [3, 7] and d["log_prior"].shape == (2, 91) and d["log_prior"].tobytes() == em["log_prior"].tobytes()
    assert d["prior_loglik"].shape == (6, 2) and d["prior_loglik"].tobytes() == em["loglik_class"].tobytes()
    assert d["prior_loglik_total"].tobytes() == em["loglik"].tobytes() and d["prior_n_eff"].tolist() == em["n_eff"].tolist()
    assert d["prior_n_eff"].sum() == mask.sum() == 124 and d["prior_n_iter"] == em["n_iter"]
    for i, n in enumerate(names):
        assert np.asarray(solver.params_[n]).tobytes() == want["mean"][i].tobytes() and d["posterior_sd"][n].tobytes() == want["sd"][i].tobytes()
    assert d["log_evidence"].tobytes() == want["log_evidence"].tobytes() and d["clipped_mass"].tobytes() == want["clipped_mass"].tobytes()
    assert solver.log_prior is None

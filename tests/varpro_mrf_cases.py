"""The inputs of the GPU cases of tests/test_gpu_varpro_mrf.py and tests/test_gpu_varpro_mrf_axes.py, shared with
tests/test_varpro_mrf_host.py, which runs the numpy reference alone on every one of them and so checks its eps_v preconditions
(wide box, eps_v <= 1e-6) without a GPU.  Nothing here touches the device."""
from __future__ import annotations

import itertools

import numpy as np
from grid_start_reference import signals
from varpro_posterior_reference import apart_atoms, wide_box
from varpro_reference import TRI_RATES, case_atoms, case_signals

from pyneapple_amd import api

NOISE_SD = 0.02  # the additive noise of case_signals: the known-noise mode
MODELS = sorted(api.MODEL_IDS)


def table(n_vox, n_nb, seed=3):
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


def many_atoms(model, n_b):
    """(n_b, nl_atoms) with one LDS slab + 16 atoms: mono 272 rates at 16 b-values; two compartments the pairs at least two apart
    of a 16-rate list (the ratio of neighbouring rates of the 8-rate list), the first 96 at 32 b-values; three the 64 of case_atoms
    at 32 b-values."""
    k = api.VARPRO_COMPARTMENTS[model]
    if k == 1:
        atoms = np.geomspace(3e-4, 0.3, 272)[None]
    elif k == 2:
        r = np.geomspace(3e-4, 0.3, 16)
        atoms = np.ascontiguousarray(np.array([(r[i], r[j]) for i in range(15, -1, -1) for j in range(i - 2, -1, -1)]).T)[:, :96]
    else:
        atoms = case_atoms(model)
    assert atoms.shape[1] == api.varpro_mrf_slab_atoms(n_b, k) + 16
    return np.ascontiguousarray(atoms)


def _layout_case(model, n_atoms, noise_sd, marginal, n_vox=83):
    k = api.VARPRO_COMPARTMENTS[model]
    n_b = 16 if k == 1 else 32
    if n_atoms == "slab+16":
        atoms = many_atoms(model, n_b)
    else:
        atoms = np.ascontiguousarray(case_atoms(model)[:, :: max(1, case_atoms(model).shape[1] // 17)][:, :n_atoms] if n_atoms > 1
                                     else case_atoms(model)[:, 3:4])
        if k == 1 and n_atoms > 1:
            atoms = np.geomspace(3e-4, 0.3, n_atoms)[None]
        assert atoms.shape[1] == n_atoms
    b, y = case_signals(model, n_vox, n_b=n_b)
    lo, hi = wide_box(model)
    return dict(model=model, b=b, y=y, nl_atoms=atoms, lo=lo, hi=hi, kw=dict(noise_sd=noise_sd, marginal=marginal), strength=16.0)


def range_case(n_b):
    """200 voxels for the first x count ranges: mono at 4 and 5 b-values (an odd n_b leaves a range's first row 8-byte aligned only),
    tri_s0 at 33."""
    model = "mono" if n_b < 8 else "tri_s0"
    b, y = case_signals(model, 200, n_b=n_b)
    lo, hi = wide_box(model)
    atoms = np.geomspace(3e-4, 0.3, 33)[None] if model == "mono" else case_atoms(model)[:, :33]
    return dict(model=model, b=b, y=y, nl_atoms=np.ascontiguousarray(atoms), lo=lo, hi=hi, kw=dict(noise_sd=NOISE_SD, marginal=True), strength=16.0)


def sigma_case():
    b, y = case_signals("bi_s0", 83)
    lo, hi = wide_box("bi_s0")
    return dict(model="bi_s0", b=b, y=y, nl_atoms=apart_atoms("bi_s0"), lo=lo, hi=hi,
                kw=dict(noise_sd=NOISE_SD, marginal=True, sigma=np.linspace(0.5, 2.0, 32)), strength=16.0)


def lead_inf_case():
    b, y = case_signals("tri_s0", 83)
    lo, hi = wide_box("tri_s0")
    lp = np.log(np.random.default_rng(9).uniform(0.1, 1.0, 64))
    lp[:3] = -np.inf
    return dict(model="tri_s0", b=b, y=y, nl_atoms=case_atoms("tri_s0"), lo=lo, hi=hi, kw=dict(noise_sd=0.0, marginal=True, log_prior=lp),
                strength=16.0)


def _t1_signals(model, b, n_vox, t1_values, seed=11):
    rng = np.random.default_rng(seed)
    names = api.MODEL_PARAM_NAMES[model]
    truth = np.empty((len(names) + 1, n_vox))
    for i, n in enumerate(names):
        if n.startswith("D"):
            truth[i] = {"D": 2e-3, "D1": 0.08, "D2": 7e-3, "D3": 6e-4}[n] * rng.uniform(0.7, 1.4, n_vox)
        else:
            truth[i] = rng.uniform(0.15, 0.4, n_vox) if n.startswith("f") else rng.uniform(0.8, 1.2, n_vox)
    truth[-1] = rng.uniform(min(t1_values), max(t1_values), n_vox)
    kw = dict(t1_mode=1, tr=3000.0, tm=0.0)
    return signals(model, b, truth, **kw) + 0.02 * rng.standard_normal((n_vox, b.size)), kw


def t1_case(narrow=False):
    """mono with a free T1 as a grid axis; narrow: T1 on 1000 .. 1000.01, a narrow axis far from zero -- uncentred, thetac q would
    cancel twelve digits."""
    b = np.linspace(0.0, 1000.0, 32)
    t1 = np.linspace(1000.0, 1000.01, 5) if narrow else np.array([600.0, 1000.0, 1600.0])
    y, kw = _t1_signals("mono", b, 83, t1)
    d = np.geomspace(3e-4, 0.03, 8)
    atoms = np.ascontiguousarray(np.array([(a, t) for a in d for t in t1]).T)
    return dict(model="mono", b=b, y=y, nl_atoms=atoms, lo=np.array([0.0, 1e-5, 100.0]), hi=np.array([10.0, 0.5, 5000.0]),
                kw=dict(noise_sd=NOISE_SD, marginal=True, **kw), strength=64.0 if narrow else 16.0)


def axes_case(n_b):
    """K = 3 with a free T1 at 16, 33 and 128 b-values: 83 voxels, 33 atoms (11 rate triples x 3 values of T1)."""
    b = np.linspace(0.0, 1000.0, n_b)
    t1 = np.array([600.0, 1000.0, 1600.0])
    y, kw = _t1_signals("tri_reduced", b, 83, t1)
    triples = list(itertools.product(*TRI_RATES))[::6][:11]
    atoms = np.ascontiguousarray(np.array([(*t, v) for t in triples for v in t1]).T)
    lo, hi = wide_box("tri_reduced")
    return dict(model="tri_reduced", b=b, y=y, nl_atoms=atoms, lo=np.append(lo, 100.0), hi=np.append(hi, 5000.0),
                kw=dict(noise_sd=NOISE_SD, marginal=True, **kw), strength=16.0)


def driver_case(n_vox, model="tri_s0", n_b=16):
    b, y = case_signals(model, n_vox, n_b=n_b)
    lo, hi = wide_box(model)
    return dict(model=model, b=b, y=y, nl_atoms=np.ascontiguousarray(case_atoms(model)[:, :33]), lo=lo, hi=hi,
                kw=dict(noise_sd=NOISE_SD, marginal=True), strength=16.0)


def small_phantom(seed=0):
    """6 x 5 voxels in two regions, bi_s0 over the 21 apart pairs of the 8-rate list at 32 b-values, 4-neighbourhood, by colour."""
    from grid_mrf_reference import colour_sort

    rng = np.random.default_rng(seed)
    H, W = 6, 5
    b = np.linspace(0.0, 1000.0, 32)
    truth = np.zeros((H, W, 4))
    truth[...] = [0.2, 0.06, 0.0015, 1.0]
    truth[2:5, 1:4] = [0.35, 0.1, 0.003, 1.0]
    truth = truth.reshape(-1, 4)
    y = signals("bi_s0", b, truth.T) + 0.02 * rng.standard_normal((H * W, 32))
    idx = np.arange(H * W).reshape(H, W)
    nb = -np.ones((H * W, 4), np.int32)
    nb[idx[1:].ravel(), 0] = idx[:-1].ravel()
    nb[idx[:-1].ravel(), 1] = idx[1:].ravel()
    nb[idx[:, 1:].ravel(), 2] = idx[:, :-1].ravel()
    nb[idx[:, :-1].ravel(), 3] = idx[:, 1:].ravel()
    colours = (np.add.outer(np.arange(H), np.arange(W)) & 1).ravel().astype(np.int32)
    order, snb, start = colour_sort(nb, colours)
    lo, hi = wide_box("bi_s0")
    return dict(model="bi_s0", b=b, y=y[order], nl_atoms=apart_atoms("bi_s0"), lo=lo, hi=hi, nb=snb, start=start, noise_sd=NOISE_SD)


# every GPU case that is compared with the reference, by name
GPU_CASES = {}
for _m in MODELS:
    for _a in (1, 17, "slab+16"):
        GPU_CASES[f"atoms-{_m}-{_a}"] = (lambda m=_m, a=_a: _layout_case(m, a, 0.0, True))
    for _ns, _mg in ((0.0, False), (NOISE_SD, True), (NOISE_SD, False)):
        GPU_CASES[f"modes-{_m}-{_ns}-{_mg}"] = (lambda m=_m, ns=_ns, mg=_mg: _layout_case(m, 17, ns, mg))
for _nb in (4, 5, 33):
    GPU_CASES[f"range-{_nb}"] = (lambda n=_nb: range_case(n))
for _nb in (16, 33, 128):
    GPU_CASES[f"axes-{_nb}"] = (lambda n=_nb: axes_case(n))
GPU_CASES.update({"sigma": sigma_case, "lead-inf": lead_inf_case, "t1": t1_case, "narrow-t1": lambda: t1_case(True),
                  "driver": lambda: driver_case(83)})

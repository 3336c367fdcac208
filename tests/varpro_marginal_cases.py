"""The inputs of the GPU cases of tests/test_gpu_varpro_marginals.py, by name: that file runs them on the device,
tests/test_varpro_marginals_host.py runs the reference alone on every one of them (its precondition eps_v <= the case's cap).
A case is dict(model, b, y, atoms, lo, hi, kw) with kw the keywords api.varpro_marginals and the reference share (noise_sd,
log_prior, sigma, fixed_idx, ...), `marginal` (marginal_amplitudes) and max_eps (1e-6 but for the narrow box)."""
from __future__ import annotations

import numpy as np
from grid_start_reference import signals
from varpro_posterior_reference import apart_atoms, wide_box
from varpro_reference import case_atoms, case_box, case_signals

from pyneapple_amd import api

NOISE_SD = 0.02  # the additive noise of case_signals: the known-noise mode
CUS = 256        # an MI355X: two blocks per CU is the cap of the grid


def _case(model, n_vox, n_b=32, atoms=None, narrow=False, noise_sd=0.0, marginal=True, **kw):
    b, y = case_signals(model, n_vox, n_b=n_b)
    lo, hi = case_box(model, True) if narrow else wide_box(model)
    return dict(model=model, b=b, y=y, atoms=case_atoms(model) if atoms is None else np.ascontiguousarray(atoms), lo=lo, hi=hi,
                noise_sd=noise_sd, marginal=marginal, max_eps=1e-3 if narrow else 1e-6, kw=kw)


def _ramp(n, step):
    return np.arange(n) * float(step) - (n - 1) * float(step)


def _t1_case():
    """mono with a free T1 as a second grid axis: a non-linear row with bins that is not a rate."""
    rng = np.random.default_rng(11)
    b = np.linspace(0.0, 1000.0, 32)
    kw = dict(t1_mode=1, tr=3000.0, tm=0.0)
    truth = np.stack([rng.uniform(0.8, 1.2, 40), rng.uniform(1e-3, 3e-3, 40), rng.uniform(700.0, 1500.0, 40)])
    y = signals("mono", b, truth, **kw) + 0.02 * rng.standard_normal((40, 32))
    atoms = np.ascontiguousarray(np.array([(a, t) for a in np.geomspace(3e-4, 0.03, 8) for t in (600.0, 1000.0, 1600.0)]).T)
    return dict(model="mono", b=b, y=y, atoms=atoms, lo=np.array([0.0, 1e-5, 100.0]), hi=np.array([10.0, 0.5, 5000.0]), noise_sd=0.0,
                marginal=True, max_eps=1e-6, kw=kw)


def _excluded(first, last):
    lp = np.log(np.random.default_rng(3).uniform(0.05, 1.0, 64)) + 2.5  # not normalised: the library normalises
    lp[first:last] = -np.inf
    return lp


def cases():
    """{name: case}.  The sizes are the smallest at which the kernel takes another path: a strip is 16 voxels and a block 64, a tile
    16 atoms, the slab of the tri-exponential layouts at 32 b-values 48 atoms, the register file is sized for n_b <= 32 or <= 128,
    the accumulators for B <= 64 or <= 128."""
    c = {}
    for n_vox in (1, 15, 16, 17, 65):
        c[f"voxels-{n_vox}"] = _case("tri_s0", n_vox, noise_sd=NOISE_SD if n_vox % 2 else 0.0)
    c["voxels-more-groups-than-blocks"] = _case("mono", 2 * CUS * 64 + 69, n_b=5)
    assert api.varpro_posterior_slab_atoms(32, 3) == 48
    for n_atoms in (1, 15, 16, 17, 48 + 16):
        c[f"atoms-{n_atoms}"] = _case("tri_reduced", 50, atoms=case_atoms("tri_reduced")[:, :n_atoms], noise_sd=0.0 if n_atoms % 2 else NOISE_SD)
    # K + 1 (mono: 2), 4, 5, 32, 33.  K + 1 of two or three compartments is left to mono: three or four points spread over 0..1000
    # leave the columns of the fast rates numerically dependent, and the reference's own precondition (eps_v <= 1e-6) refuses it
    for model, n_b in (("mono", 2), ("mono", 4), ("mono", 5), ("tri_s0", 32), ("tri_s0", 33)):
        c[f"n_b-{model}-{n_b}"] = _case(model, 40, n_b=n_b)
    for B in (1, 16, 17, 64, 65, 128):
        c[f"bins-{B}"] = _case("mono", 40, n_b=8, atoms=np.geomspace(3e-4, 0.3, B)[None] if B > 1 else np.array([[2e-3]]),
                               noise_sd=NOISE_SD if B % 2 else 0.0)
    for i, model in enumerate(sorted(api.MODEL_IDS)):  # every layout in both noise modes and with both amplitude weights
        c[f"layout-{model}-a"] = _case(model, 70, noise_sd=0.0, marginal=bool(i % 2))
        c[f"layout-{model}-b"] = _case(model, 70, noise_sd=NOISE_SD, marginal=not i % 2)
    c["free-t1"] = _t1_case()
    c["sigma"] = _case("bi_s0", 60, atoms=apart_atoms("bi_s0"), sigma=np.linspace(0.5, 2.0, 32))
    # the running maximum
    c["first-tile-excluded"] = _case("tri_s0", 40, log_prior=_excluded(0, 16))      # also: D1's first bin holds excluded atoms only
    c["middle-tile-excluded"] = _case("tri_s0", 40, log_prior=_excluded(16, 32))
    c["best-atom-last"] = _case("tri_reduced", 40, log_prior=_ramp(64, 60.0))        # two slabs; every tile moves the maximum
    c["far-atoms-underflow"] = _case("mono", 40, noise_sd=0.002)                     # l spans thousands: far atoms weigh exactly 0
    c["narrow-box"] = _case("tri_s0", 70, narrow=True)
    return c


def call_kw(case):
    """The keywords of api.varpro_marginals / api.varpro_posterior for a case."""
    return dict(noise_sd=case["noise_sd"], marginal_amplitudes=case["marginal"], **case["kw"])


def ref_kw(case):
    """The keywords of the references for a case."""
    return dict(noise_sd=case["noise_sd"], marginal=case["marginal"], max_eps=case["max_eps"], **case["kw"])

"""Inputs shared by tests/test_grid_rician_host.py (the reference's preconditions, no GPU) and tests/test_gpu_grid_rician.py: the
z list of log_i0e, the posterior's cases (every model layout the Gaussian call serves without projection, both kernel forms,
the voxel / b-value / atom counts at which the kernel takes another path) and the worth population."""
from __future__ import annotations

import numpy as np

from pyneapple_amd import api, synth
from grid_start_reference import signals

BREAKS = (2.0, 4.0, 8.0)  # the break points of csrc/pnx_bessel.hpp


def z_list():
    """0, 20 001 points of geomspace(1e-300, 1e300), the denormal edge, both sides of every break point."""
    edge = [5e-324, 2.2250738585072009e-308, 2.2250738585072014e-308]
    sides = [f(x) for x in BREAKS for f in (lambda v: np.nextafter(v, 0.0), lambda v: v, lambda v: np.nextafter(v, np.inf))]
    return np.concatenate([[0.0], np.geomspace(1e-300, 1e300, 20001), edge, sides])


def rician_slab_atoms(n_b, n_free):
    """grid_rician_slab of csrc/pnx_grid_rician_args.hpp (the stub prints the kernel's for the host test to compare)."""
    return api.grid_rician_slab_atoms(n_b, n_free)


RANGES = {"f1": (0.05, 0.3), "f2": (0.1, 0.35), "f3": (0.2, 0.5), "D1": (0.02, 0.1), "D2": (2e-3, 8e-3), "D3": (3e-4, 1.5e-3),
          "D": (5e-4, 3e-3), "S0": (0.7, 1.3), "T1": (600.0, 2500.0)}

# name: (model, n_vox, n_b, n_atoms or "slab+16", log_prior with -inf entries, extra keywords)
CASES = {
    "mono_1vox_1atom": ("mono", 1, 4, 1, False, {}),
    "bi_reduced_15": ("bi_reduced", 15, 5, 17, False, {}),
    "bi_s0_on_grid_wide_slab": ("bi_s0", 16, 33, "slab+16", False, {}),
    "bi_full_128b": ("bi_full", 17, 128, 17, False, {}),
    "tri_reduced_prior_slab": ("tri_reduced", 83, 5, "slab+16", True, {}),
    "tri_s0_on_grid_200": ("tri_s0", 200, 4, 17, False, {}),
    "tri_full_odd_stride": ("tri_full", 17, 33, 17, True, {}),
    "bi_reduced_free_t1": ("bi_reduced", 83, 5, 17, False, dict(t1_mode=1, tr=3000.0)),
    "tri_reduced_fixed_128b_slab": ("tri_reduced", 16, 128, "slab+16", False, dict(fixed_idx=[2, 4], fixed_vals=np.array([0.25, 8e-4]))),
    "bi_reduced_1atom_200": ("bi_reduced", 200, 33, 1, False, {}),
    # seven free parameters: the NF = 8 forms of the kernel, narrow and wide
    "tri_s0_free_t1_nf8": ("tri_s0", 17, 5, 17, False, dict(t1_mode=1, tr=3000.0)),
    "tri_full_free_t1_nf8_wide": ("tri_full", 16, 33, 17, True, dict(t1_mode=1, tr=3000.0)),
}
NOISE_SD = 0.05


def names_of(model, kw):
    names = list(api.MODEL_PARAM_NAMES[model]) + (["T1"] if kw.get("t1_mode") else [])
    return [n for i, n in enumerate(names) if i not in kw.get("fixed_idx", ())]


def build(name):
    """dict(model, b, y (magnitudes), atoms, lo, hi, noise_sd, log_prior, kw) of a case, seeded by its position."""
    model, n_vox, n_b, n_atoms, with_prior, kw = CASES[name]
    rng = np.random.default_rng(1000 + list(CASES).index(name))
    names = names_of(model, kw)
    if n_atoms == "slab+16":
        n_atoms = rician_slab_atoms(n_b, len(names)) + 16
    atoms = np.stack([rng.uniform(*RANGES[n], n_atoms) for n in names])
    lo = np.array([0.0 for _ in names])
    hi = np.array([2 * RANGES[n][1] for n in names])
    b = np.linspace(0.0, 1500.0, n_b)
    truth = atoms[:, rng.integers(0, n_atoms, n_vox)]
    clean = signals(model, b, truth, kw.get("fixed_idx", ()), kw.get("fixed_vals"), kw.get("t1_mode", 0), kw.get("tr", 0.0), kw.get("tm", 0.0))
    y = synth.rician_magnitude(clean, NOISE_SD, seed=int(rng.integers(1 << 30)))
    lp = None
    if with_prior:
        lp = np.log(rng.uniform(0.1, 1.0, n_atoms))
        lp[rng.random(n_atoms) < 0.3] = -np.inf
        lp[0] = -np.inf
        lp[-1] = -0.5
    return dict(model=model, b=b, y=y, atoms=atoms, lo=lo, hi=hi, noise_sd=NOISE_SD, log_prior=lp, kw=kw)


# ---- the worth population: reduced bi-exponential truths on a grid that contains them, Rician noise, seed 0
WORTH_GRID = {"f1": np.linspace(0.05, 0.45, 9), "D1": np.geomspace(0.01, 0.1, 9), "D2": np.linspace(2e-4, 3e-3, 15)}
WORTH_BOUNDS = {"f1": (0.0, 1.0), "D1": (1e-3, 0.5), "D2": (1e-5, 5e-3)}
WORTH_VOXELS = 400


def worth_population(noise_sd, b_max, n_vox=WORTH_VOXELS, seed=0):
    """b (32,), clean and magnitude signals, truths (3, n_vox) drawn from the grid values, atoms (3, 1215) in itertools.product order."""
    import itertools

    rng = np.random.default_rng(seed)
    b = np.linspace(0.0, b_max, 32)
    axes = [WORTH_GRID[n] for n in ("f1", "D1", "D2")]
    atoms = np.ascontiguousarray(np.array(list(itertools.product(*axes)), float).T)
    truth = np.stack([rng.choice(a, n_vox) for a in axes])
    clean = signals("bi_reduced", b, truth)
    y = synth.rician_magnitude(clean, noise_sd, seed=seed)
    lo = np.array([WORTH_BOUNDS[n][0] for n in ("f1", "D1", "D2")])
    hi = np.array([WORTH_BOUNDS[n][1] for n in ("f1", "D1", "D2")])
    return dict(b=b, y=y, clean=clean, truth=truth, atoms=atoms, lo=lo, hi=hi)


WORTH_CELLS = [(0.05, 1000.0), (0.05, 2500.0), (0.10, 1000.0), (0.10, 2500.0)]
# the strongest cell of the table measured on the reference: the slow rate D2 at noise 0.10 with b up to 2500,
# ratio of the median |error| Rician / Gaussian 0.288; the assertion is the measured figure + 0.1
WORTH_ASSERTED = (0.10, 2500.0, 2)
WORTH_ASSERTED_RATIO = 0.288 + 0.1

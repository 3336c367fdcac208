"""The cases of the fine-grid tests (pnx_curvefit_grid_refine_f64), shared by tests/test_grid_refine_host.py (the
reference's preconditions) and tests/test_gpu_grid_refine.py (the device inside the reference's bounds), and the population of the
worth table.  Shapes are the smallest at which the kernel takes another path: n_vox 1 / 17 / 130 (one wave, a partial block, more
than one block), n_b 1 / 4 / 5 / 32 / 33 / 128, atom counts below, at and off a multiple of 64, every layout."""
from __future__ import annotations

import numpy as np

import grid_refine_reference as R

RANGES = {"f1": (0.1, 0.35), "f2": (0.1, 0.3), "f3": (0.1, 0.3), "D1": (0.02, 0.08), "D2": (0.004, 0.012), "D3": (0.0005, 0.002), "S0": (0.8, 1.2)}
BOUNDS = {"f1": (0.0, 1.0), "f2": (0.0, 1.0), "f3": (0.0, 1.0), "D1": (0.005, 0.2), "D2": (0.001, 0.02), "D3": (0.0001, 0.004), "S0": (0.1, 5.0)}
MONO = {"S0": (0.8, 1.2), "D1": (0.0008, 0.003)}
MONO_BOUNDS = {"S0": (0.1, 5.0), "D1": (0.0001, 0.01)}

# name: (model, n_vox, n_b, points per free row, noise_sd (0: marginalised), project, fixed {position: value})
CASES = {
    "mono_grid": ("mono", 17, 4, (3, 5), 0.02, False, {}),
    "mono_projected": ("mono", 1, 5, (1, 9), 0.0, True, {}),
    "bi_reduced_125": ("bi_reduced", 130, 32, (5, 5, 5), 0.02, False, {}),
    "bi_reduced_one_point": ("bi_reduced", 17, 33, (1, 1, 1), 0.02, False, {}),
    "bi_reduced_one_b": ("bi_reduced", 17, 1, (2, 3, 1), 0.02, False, {}),
    "bi_s0_projected": ("bi_s0", 17, 32, (2, 3, 4, 1), 0.0, True, {}),
    "bi_s0_grid": ("bi_s0", 17, 5, (3, 3, 3, 3), 0.02, False, {}),
    "bi_full_wide": ("bi_full", 17, 128, (2, 3, 2, 3), 0.0, False, {}),
    "tri_reduced_3125": ("tri_reduced", 17, 32, (5, 5, 5, 5, 5), 0.02, False, {}),
    "tri_reduced_nine": ("tri_reduced", 130, 4, (1, 9, 1, 3, 2), 0.02, False, {}),
    "tri_s0_projected_fixed": ("tri_s0", 17, 33, (2, 3, 2, 3, 1), 0.02, True, {4: 0.001}),
    "tri_full_64": ("tri_full", 1, 128, (2, 2, 2, 2, 2, 2), 0.0, False, {}),
    "tri_reduced_wide_nine": ("tri_reduced", 1, 128, (2, 9, 2, 9, 9), 0.02, False, {}),
}


def names_of(model, fixed=()):
    return [n for i, n in enumerate(R.LAYOUT[model]) if i not in fixed]


def build(name, seed=5):
    model, n_vox, n_b, pts, noise_sd, project, fixed = CASES[name]
    rng = np.random.default_rng(seed + sum(map(ord, name)))
    rg, bd = (MONO, MONO_BOUNDS) if model == "mono" else (RANGES, BOUNDS)
    all_names = R.LAYOUT[model]
    fixed_idx = sorted(fixed)
    names = names_of(model, fixed_idx)
    truth = np.stack([rng.uniform(*rg[n], n_vox) for n in all_names])
    for i, val in fixed.items():
        truth[i] = val
    b = np.array([100.0]) if n_b == 1 else np.linspace(0.0, 800.0, n_b)
    w = R.weights(model, truth)
    s = (w[:, :, None] * np.exp(-b[None, None, :] * truth[R.RATES[model]][:, :, None])).sum(axis=0)
    if model in R.S0_POS:
        s = s * truth[R.S0_POS[model]][:, None]
    y = s + rng.normal(0.0, 0.02, s.shape)
    free = [i for i in range(len(all_names)) if i not in fixed_idx]
    lo, hi = np.array([bd[n][0] for n in names]), np.array([bd[n][1] for n in names])
    width = np.array([rg[n][1] - rg[n][0] for n in names])
    centre = truth[free] + rng.uniform(-0.1, 0.1, (len(names), n_vox)) * width[:, None]
    half = rng.uniform(0.05, 0.3, (len(names), n_vox)) * width[:, None]
    return dict(model=model, b=b, y=np.ascontiguousarray(y), lo=lo, hi=hi, n_points=np.array(pts, np.int32), centre=np.ascontiguousarray(centre),
                half_width=np.ascontiguousarray(half), noise_sd=noise_sd, project=project, fixed_idx=fixed_idx,
                fixed_vals=np.array([fixed[i] for i in fixed_idx]) if fixed_idx else None, names=names)


def reference_of(c, **kw):
    return R.reference(c["model"], c["b"], c["y"], c["lo"], c["hi"], c["n_points"], c["centre"], c["half_width"], noise_sd=c["noise_sd"],
                       project=c["project"], fixed_idx=c["fixed_idx"], fixed_vals=c["fixed_vals"], **kw)


def call_kwargs(c):
    return dict(noise_sd=c["noise_sd"], fixed_idx=c["fixed_idx"], fixed_vals=c["fixed_vals"], project_amplitude=c["project"])


def edge_case():
    """bi_reduced, 17 voxels x 32 b-values, 5 x 5 x 5 points with f1 allowed up to 1.5, and per voxel one oddity:
    3: the D1 box is cut by the upper bound; 5: the D2 box lies beyond the lower bound and collapses to the bound; 6: half-width 0
    on f1; 7: a NaN signal; 9: a NaN centre; 11: a negative half-width; 13: every atom has f1 > 1; 14: the f1 box straddles 1."""
    c = build("bi_reduced_125")
    c["y"] = np.ascontiguousarray(c["y"][:17])
    for key in ("centre", "half_width"):
        c[key] = np.ascontiguousarray(c[key][:, :17])
    c["hi"] = c["hi"].copy()
    c["hi"][0] = 1.5
    c["centre"][1, 3], c["half_width"][1, 3] = 0.19, 0.03
    c["centre"][2, 5], c["half_width"][2, 5] = 0.0004, 0.0005
    c["half_width"][0, 6] = 0.0
    c["y"][7, 4] = np.nan
    c["centre"][1, 9] = np.nan
    c["half_width"][2, 11] = -1e-3
    c["centre"][0, 13], c["half_width"][0, 13] = 1.3, 0.1
    c["centre"][0, 14], c["half_width"][0, 14] = 0.9713, 0.1
    return c, dict(nan=[7, 9, 11, 13], cut=3, single=5, zero_width=6, straddle=14)


# ---- a fine grid that coincides with a coarse one: every value below is exact in binary, and so are centre -+ half_width
COINCIDE_AXES = [np.array([0.125, 0.25, 0.375]), np.array([1.0, 2.0, 3.0]) * 2.0 ** -6, np.array([1.0, 2.0, 3.0]) * 2.0 ** -10]

# ---- worth: 400 reduced bi-exponential voxels, truths uniform inside a 4 x 4 x 4 grid's ranges, 32 b-values, seed 0
WORTH_AXES = [np.linspace(0.1, 0.4, 4), np.linspace(0.02, 0.08, 4), np.linspace(0.0005, 0.002, 4)]
WORTH_LO, WORTH_HI = np.array([0.0, 0.005, 0.0001]), np.array([1.0, 0.2, 0.004])
WORTH_NOISE = (0.01, 0.05)
WORTH_LEVELS = (1, 2)
# median |error| refined / coarse per (noise, levels) for (f1, D1, D2), measured on the reference (test_grid_refine_host.py prints the
# table); a cell below 1 is asserted at measured + 0.1, the house margin
WORTH_MEASURED = {(0.01, 1): (0.4199, 0.6881, 0.4158), (0.01, 2): (0.2086, 0.4489, 0.2030),
                  (0.05, 1): (0.6068, 0.9945, 0.6204), (0.05, 2): (0.5371, 1.2369, 0.5643)}


def worth_population(noise, n_vox=400, seed=0):
    rng = np.random.default_rng(seed)
    truth = np.stack([rng.uniform(ax[0], ax[-1], n_vox) for ax in WORTH_AXES])
    b = np.linspace(0.0, 1000.0, 32)
    s = truth[0][:, None] * np.exp(-b[None] * truth[1][:, None]) + (1 - truth[0])[:, None] * np.exp(-b[None] * truth[2][:, None])
    return dict(b=b, y=s + rng.normal(0.0, noise, s.shape), truth=truth)

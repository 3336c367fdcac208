"""The inputs of the GPU cases of tests/test_gpu_varpro_class_axes.py, by name: that file runs them on the device,
tests/test_varpro_class_prior_host.py runs the references alone on every one of them (their precondition eps_v <= the case's cap:
1e-6, or the 1e-3 that tests/test_gpu_varpro_class_prior.py's `_case` states for 16 b-values or fewer).  The choice of inputs is made
here, on the CPU.  A case is tests/varpro_marginal_cases.py's dict; `n_classes` is added where it is not three.

65 voxels (four full strips and one voxel).  The layouts and the b-axis take the case dictionaries of tests/varpro_reference.py (8
rates, 28 pairs, 64 triples: one partly filled tile, two tiles, four), the minimum-width slabs 33 atoms (three slabs of 16, the last
holding one atom)."""
from __future__ import annotations

import numpy as np
from test_gpu_varpro_class_prior import MODES, _case
from varpro_prior_cases import wide_pairs

from pyneapple_amd import api

N_VOX = 65
B_AXIS = [("mono", 2), ("mono", 5), ("tri_s0", 31), ("tri_s0", 32), ("tri_s0", 33), ("tri_s0", 64), ("tri_s0", 65), ("tri_s0", 128),
          ("bi_full", 128)]  # the points of tests/test_gpu_varpro_posterior.py::test_b_axis
LAYOUT_NB = (16, 33)  # both register-file instantiations: n_b <= 32 and <= 128
# the minimum slab width at 128 b-values: at one compartment 16 classes force it (12 classes still fit 32 atoms), at three the
# dictionary rows alone do and 16 classes make the EM's LDS image the largest of all (7616 doubles)
MIN_SLAB = [("mono", 16), ("tri_s0", 16)]


def atoms_33(model):
    """33 atoms: 33 rates over three decades, the first 33 of wide_pairs, the first 33 triples of the case dictionary."""
    k = api.VARPRO_COMPARTMENTS[model]
    if k == 1:
        return np.ascontiguousarray(np.geomspace(3e-4, 0.3, 33)[None])
    return wide_pairs(33) if k == 2 else np.ascontiguousarray(_case(model, 1)["atoms"][:, :33])


def mode_cases(model, n_b, atoms=None, modes=MODES):
    """The case under each (noise_sd, marginal_amplitudes) of `modes`."""
    return [_case(model, N_VOX, n_b=n_b, atoms=atoms, noise_sd=noise_sd, marginal=marginal) for noise_sd, marginal in modes]


def cases():
    """{name: [case per mode]} of every case the GPU file runs."""
    c = {}
    for model in sorted(api.MODEL_IDS):
        for n_b in LAYOUT_NB:
            # bi_full at 16 b-values: the neighbouring rates of the 28-pair dictionary carry the reference's eps_v to 0.83 (the two
            # free amplitudes of nearly equal columns), past any cap; the first 33 of wide_pairs keep it at 3e-9
            atoms = wide_pairs(33) if (model, n_b) == ("bi_full", 16) else None
            c[f"layout-{model}-{n_b}"] = mode_cases(model, n_b, atoms=atoms)
    for model, n_b in B_AXIS:
        c[f"n_b-{model}-{n_b}"] = mode_cases(model, n_b, modes=MODES[:2])
    for model, n_classes in MIN_SLAB:
        c[f"min-slab-{model}"] = [dict(case, n_classes=n_classes) for case in mode_cases(model, 128, atoms=atoms_33(model), modes=MODES[:2])]
    return c

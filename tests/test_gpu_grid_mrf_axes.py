"""pnx_curvefit_grid_posterior_field_f64 on the device over the axes grid_mrf_posterior_kernel is instantiated on:
both register-file sizes (NS = 8 for n_b <= 32, NS = 32 up to 128) projected and not, and the parameter rows NF = 3 (mono, bi_reduced)
beside NF = 6 -- 83 voxels, 33 atoms with three -inf atoms in front, both noise modes, field_n = 0 beside 8 in a strip -- and the driver
at 33 b-values, projected, against its composition by hand.

Acceptance is tests/grid_mrf_reference.py's field posterior inside the posterior's own bounds (error / bound <= 1; no tolerance of this
file's own); delta is the largest move of a mean, exactly.  The largest error-to-bound ratios observed are recorded in DESIGN.md 4.1p."""
from __future__ import annotations

import numpy as np
import pytest
from grid_posterior_reference import accept
from test_gpu_grid_mrf import POST_KEYS, _coloured, _compose, _dev, _field_case, _field_on_device, _same_bytes
from test_gpu_grid_prior import NOISE_SD, _case

from pyneapple_amd import api

pytestmark = pytest.mark.gpu

CASES = [("bi_s0", True, 33), ("bi_s0", True, 128), ("tri_reduced", False, 33), ("tri_reduced", False, 128),  # NF = 6 in the wide file
         ("mono", True, 16), ("mono", True, 33), ("bi_reduced", False, 16), ("bi_reduced", False, 33),       # NF = 3 in both
         ("tri_s0", True, 33)]


@pytest.mark.parametrize("model,project,n_b", CASES)
@pytest.mark.parametrize("noise_sd", [0.0, NOISE_SD])
def test_field_posterior_register_files_and_parameter_rows(gpu, model, project, n_b, noise_sd):
    c = _field_case(gpu, model, project, 33, n_b, noise_sd, lead_inf=3, n_vox=83)
    got = _field_on_device(gpu, model, c["b"], c["y"], c["atoms"], c["lo"], c["hi"], c["q"], c["n"], c["pr"], 0, 83, c["plain"],
                           want_delta=True, **c["kw"])
    assert (c["n"] == 0).any() and (c["n"] == 8).any()  # field_n = 0 beside field_n = 8
    q = accept(c["ref"], got, c["atoms"])
    print(f"field posterior: {model} n_b={n_b} NS={8 if n_b <= 32 else 32} project={project} noise_sd={noise_sd}: error / bound = {q}")
    # delta: the largest move of a mean against the plain posterior's, in units of the row's range
    rows = np.flatnonzero((c["pr"] > 0) & (c["rng"] > 0))
    fin = c["ref"]["finite"]
    assert rows.size
    move = np.abs(got["mean"][rows][:, fin] - c["plain"]["mean"][rows][:, fin]) / c["rng"][rows, None]
    assert got["delta"] == move.max() and got["delta"] > 0


def test_driver_equals_its_composition_in_the_wide_register_file(gpu):
    import torch

    model, sizes = "bi_s0", (19, 30, 17, 17)
    n_vox = sum(sizes)
    b, y, atoms, lo, hi = _case(model, n_vox, 33, 33)
    y[5] = np.nan  # a non-finite voxel: NaN everywhere, counts for nobody
    nb, start = _coloured(n_vox, sizes)
    pr = 16.0 / (atoms.max(axis=1) - atoms.min(axis=1)) ** 2
    pr[api.MODEL_PARAM_NAMES[model].index("S0")] = 0.0
    kw = dict(noise_sd=NOISE_SD, project_amplitude=True)
    want = _compose(gpu, model, b, y, atoms, lo, hi, nb, start, pr, 3, 0.0, **kw)
    got = gpu.grid_posterior_mrf(model, b, y, atoms, lo, hi, nb, start, pr, n_sweeps=3, tol=0.0, **kw)
    _same_bytes(got, want)
    assert got["n_sweeps"] == 3 and got["delta"].tolist() == want["delta"] and got["delta"][0] > 0
    assert np.isnan(got["mean"][:, 5]).all() and got["map_atom"][5] == -1
    dev = gpu.grid_posterior_mrf(model, b, _dev(y), atoms, lo, hi, _dev(nb), start, pr, n_sweeps=3, **kw)  # device tensors
    torch.cuda.synchronize()
    _same_bytes(got, {k: dev[k].cpu().numpy() for k in POST_KEYS})
    assert dev["delta"].tobytes() == got["delta"].tobytes()

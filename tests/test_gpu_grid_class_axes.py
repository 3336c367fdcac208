"""pnx_curvefit_grid_posterior_classes_f64 and pnx_curvefit_grid_prior_em_classes_f64 on the device over the axes
their kernels are instantiated on, with several classes mixed inside every strip: the b-axis through both register-file sizes
(NS = 8 for n_b <= 32, NS = 32 up to 128), projected and not; every layout (NF = 3, 6 and -- tri_s0 with a free T1, seven free
parameters -- 8 parameter rows); a sigma vector, a shared fixed parameter and the T1 factor through the labelled entry points; and
the minimum slab width of 16 atoms at 128 b-values and 16 classes, where every tile is a slab reload.

65 voxels (four full strips and one voxel), 33 atoms (two tiles and one atom), three classes interleaved unless a case says
otherwise.  Acceptance is tests/grid_class_prior_reference.py's derived bounds (error / bound <= 1) and nothing else; where two calls
perform the same sums (a class's voxels under the unlabelled call with that class's row) the bytes are equal.  The largest
error-to-bound ratios observed are recorded in DESIGN.md 4.1n."""
from __future__ import annotations

import numpy as np
import pytest
from grid_class_prior_reference import accept_em, normalise_rows, posterior
from grid_posterior_reference import accept
from grid_prior_reference import likelihoods
from test_gpu_grid_class_prior import MODES, POST_KEYS, _em, _rows, _same_bytes
from test_gpu_grid_posterior import _case as _case_kw  # test_gpu_grid_prior._case with fixed parameters and a T1 factor
from test_gpu_grid_prior import _case

from pyneapple_amd import api

pytestmark = pytest.mark.gpu

N_VOX, N_ATOMS = 65, 33


def _note(what, model, case, project, noise_sd, q):
    n_b = len(case[0])
    print(f"grid class {what}: {model} n_b={n_b} NS={8 if n_b <= 32 else 32} project={project} noise_sd={noise_sd}: error / bound = {q}")


def _posterior(gpu, model, case, project, n_classes=3, **kw):
    """The labelled posterior under random rows, classes interleaved, in both noise modes: the reference's bounds on every voxel, and
    per class the bytes of the unlabelled call under that class's row (a voxel's sums depend on the order of the atoms only)."""
    b, y, atoms, lo, hi = case
    lab = (np.arange(len(y)) % n_classes).astype(np.int32)
    rows = _rows(n_classes, atoms.shape[1])
    for noise_sd in MODES:
        call = dict(noise_sd=noise_sd, project_amplitude=project, **kw)
        got = gpu.grid_posterior_classes(model, b, y, atoms, lo, hi, lab, n_classes, log_prior=rows, **call)
        ref = posterior(model, b, y, atoms, lo, hi, lab, n_classes, log_prior=rows, noise_sd=noise_sd, project=project, **kw)
        _note("posterior", model, case, project, noise_sd, accept(ref, got, atoms))
        for c in range(n_classes):
            idx = np.flatnonzero(lab == c)
            _same_bytes(got, gpu.grid_posterior(model, b, y, atoms, lo, hi, log_prior=rows[c], **call), POST_KEYS, (idx, idx))


def _updates(gpu, model, case, project):
    """One EM update with every strip mixed and with one class per strip (test_gpu_grid_class_prior._em: four rows, the last without
    a voxel), in both noise modes."""
    for kind in ("mixed", "sorted"):
        for noise_sd in MODES:
            q = _em(gpu, model, case, kind, 1, project, noise_sd, 0.0, prior=_rows(4, case[2].shape[1]))
            _note(f"EM {kind}", model, case, project, noise_sd, q)


def _update_kw(gpu, model, case, project, n_classes=3, **kw):
    """One EM update under the interleaved labels with the keywords of the call handed to the library and to the reference alike."""
    b, y, atoms, lo, hi = case
    lab = (np.arange(len(y)) % n_classes).astype(np.int32)
    rows = _rows(n_classes, atoms.shape[1])
    for noise_sd in MODES:
        got = gpu.grid_prior_em_classes(model, b, y, atoms, lo, hi, lab, n_classes, log_prior=rows, noise_sd=noise_sd, n_iter=1, rel_tol=0.0,
                                        project_amplitude=project, **kw)
        l0, eps0, fin = likelihoods(model, b, y, atoms, lo, hi, noise_sd=noise_sd, project=project, **kw)
        q = accept_em(got, l0, eps0, fin, lab, normalise_rows(rows, n_classes, atoms.shape[1]), 0.0, 1)
        _note(f"EM {n_classes} classes", model, case, project, noise_sd, q)


# ---- 1. the b-axis with several classes: 33 and up take the larger register file; 1, 5, 33 and 65 pad the k-steps
@pytest.mark.parametrize("n_b", [1, 5, 33, 64, 65, 128])
def test_b_axis(gpu, n_b):
    case = _case("tri_reduced", N_VOX, N_ATOMS, n_b)
    _posterior(gpu, "tri_reduced", case, False)
    _updates(gpu, "tri_reduced", case, False)


@pytest.mark.parametrize("n_b", [5, 33, 65, 128])
def test_b_axis_projected(gpu, n_b):
    case = _case("bi_s0", N_VOX, N_ATOMS, n_b)
    _posterior(gpu, "bi_s0", case, True)
    _updates(gpu, "bi_s0", case, True)


# ---- 2. every layout in both register files: NF = 3 (mono, bi_reduced), NF = 6, and NF = 8 below
@pytest.mark.parametrize("n_b", [16, 33])
@pytest.mark.parametrize("model", sorted(api.MODEL_IDS))
def test_every_layout_in_both_register_files(gpu, model, n_b):
    project = model in api.PROJECT_MODELS
    case = _case(model, N_VOX, N_ATOMS, n_b)
    _posterior(gpu, model, case, project)
    _updates(gpu, model, case, project)


@pytest.mark.parametrize("project", [False, True])
@pytest.mark.parametrize("n_b", [16, 33])
def test_seven_free_parameters(gpu, n_b, project):
    """tri_s0 with a free T1 is the widest layout the argument check admits: seven free parameters, the NF = 8 instantiation."""
    kw = dict(t1_mode=1, tr=3000.0)
    case = _case_kw("tri_s0", N_VOX, N_ATOMS, n_b, **kw)
    assert case[2].shape[0] == 7
    _posterior(gpu, "tri_s0", case, project, **kw)
    _update_kw(gpu, "tri_s0", case, project, **kw)


# ---- 3. keywords through the labelled path, at 33 b-values
def test_sigma_vector(gpu):
    sigma = np.linspace(0.5, 3.0, 33)
    for model, project in (("tri_reduced", False), ("bi_s0", True)):
        case = _case(model, N_VOX, N_ATOMS, 33)
        _posterior(gpu, model, case, project, sigma=sigma)
        _update_kw(gpu, model, case, project, sigma=sigma)


@pytest.mark.parametrize("project", [False, True])
def test_shared_fixed_parameter(gpu, project):
    kw = dict(fixed_idx=[1], fixed_vals=np.array([0.07]))  # D1 of [f1, D1, D2, S0]
    case = _case_kw("bi_s0", N_VOX, N_ATOMS, 33, **kw)
    assert case[2].shape[0] == 3
    _posterior(gpu, "bi_s0", case, project, **kw)
    _update_kw(gpu, "bi_s0", case, project, **kw)


@pytest.mark.parametrize("t1_mode", [1, 2])
def test_t1_factor_on_mono(gpu, t1_mode):
    kw = dict(t1_mode=t1_mode, tr=3000.0, tm=30.0 if t1_mode == 2 else 0.0)
    case = _case_kw("mono", N_VOX, N_ATOMS, 33, **kw)
    _posterior(gpu, "mono", case, True, **kw)
    _update_kw(gpu, "mono", case, True, **kw)


# ---- 4. the minimum slab width
@pytest.mark.parametrize("model,project", [("tri_reduced", False), ("bi_s0", True)])
@pytest.mark.parametrize("n_atoms", [33, "posterior slab + 1"])
def test_minimum_slab_width(gpu, model, project, n_atoms):
    """128 b-values and 16 classes: the EM's 2 + 16 + 64 values per atom leave room for 16 atoms, so its 33 atoms are three slabs, the
    last holding one atom; the posterior's slab is wider, and one atom past it gives that kernel a second slab too."""
    n_free = len(api.MODEL_PARAM_NAMES[model])
    assert api.grid_class_slab_atoms(128, 16, 64) == 16 and api.grid_class_slab_atoms(128, 16, n_free) >= 16
    if n_atoms == "posterior slab + 1":
        n_atoms = api.grid_class_slab_atoms(128, 16, n_free) + 1
    case = _case(model, N_VOX, n_atoms, 128)
    _posterior(gpu, model, case, project, n_classes=16)
    _update_kw(gpu, model, case, project, n_classes=16)

"""pnx_curvefit_varpro_posterior_classes_f64 and pnx_curvefit_varpro_prior_em_classes_f64 on the device over the
axes their kernels are instantiated on, with several classes mixed inside every strip: every (K, CLS) arm of the three kernels in
both register-file sizes (n_b <= 32 and <= 128), the b-axis points of the unlabelled posterior's test, and the minimum slab width
of 16 atoms at 128 b-values (every tile a slab reload).  The cases are tests/varpro_class_axes_cases.py's;
tests/test_varpro_class_prior_host.py runs the references alone on every one of them.

Acceptance is tests/varpro_class_prior_reference.py's derived bounds (error / bound <= 1) and nothing else; where two calls perform
the same sums (a class's voxels under the unlabelled call with that class's row) the bytes are equal.  The largest error-to-bound
ratios observed are recorded in DESIGN.md 4.1o."""
from __future__ import annotations

import functools

import numpy as np
import pytest
from test_gpu_varpro_class_prior import POST_KEYS, _args, _em, _rows, _same_bytes
from varpro_class_axes_cases import B_AXIS, LAYOUT_NB, MIN_SLAB, cases
from varpro_class_prior_reference import accept_em, normalise_rows, posterior
from varpro_marginal_cases import call_kw, ref_kw
from varpro_posterior_reference import accept
from varpro_prior_reference import likelihoods

from pyneapple_amd import api

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _cases():
    return cases()


def _note(what, c, q):
    print(f"varpro class {what}: {c['model']} n_b={len(c['b'])} NS={8 if len(c['b']) <= 32 else 32} noise_sd={c['noise_sd']} "
          f"marginal={c['marginal']}: error / bound = {q}")


def _posterior(gpu, c):
    """The labelled posterior under random rows, classes interleaved: the reference's bounds on every voxel, and per class the bytes
    of the unlabelled call under that class's row (a voxel's sums depend on the order of the atoms only)."""
    n_classes = c.get("n_classes", 3)
    lab = (np.arange(c["y"].shape[0]) % n_classes).astype(np.int32)
    rows = _rows(n_classes, c["atoms"].shape[1])
    got = gpu.varpro_posterior_classes(*_args(c), lab, n_classes, log_prior=rows, **call_kw(c))
    q = accept(posterior(*_args(c), lab, n_classes, log_prior=rows, **ref_kw(c)), got, c["atoms"])
    _note("posterior", c, q)
    for k in range(n_classes):
        idx = np.flatnonzero(lab == k)
        _same_bytes(got, gpu.varpro_posterior(*_args(c), log_prior=rows[k], **call_kw(c)), POST_KEYS, (idx, idx))


def _updates(gpu, c):
    """One EM update with every strip mixed and with one class per strip (test_gpu_varpro_class_prior._em: four rows, the last
    without a voxel)."""
    for kind in ("mixed", "sorted"):
        _note(f"EM {kind}", c, _em(gpu, c, kind, 1, 0.0, prior=_rows(4, c["atoms"].shape[1])))


# ---- 1. every (K, CLS) arm in both register-file sizes
@pytest.mark.parametrize("n_b", LAYOUT_NB)
@pytest.mark.parametrize("model", sorted(api.MODEL_IDS))
def test_every_layout_in_both_register_files(gpu, model, n_b):
    for c in _cases()[f"layout-{model}-{n_b}"]:  # both noise modes x both amplitude weights
        _posterior(gpu, c)
        _updates(gpu, c)


# ---- 2. the b-axis with several classes
@pytest.mark.parametrize("model,n_b", B_AXIS)
def test_b_axis(gpu, model, n_b):
    for c in _cases()[f"n_b-{model}-{n_b}"]:
        _posterior(gpu, c)
        _updates(gpu, c)


# ---- 3. the minimum slab width: 33 atoms are three slabs, the last holding one atom
@pytest.mark.parametrize("model,n_classes", MIN_SLAB)
def test_minimum_slab_width(gpu, model, n_classes):
    k = api.VARPRO_COMPARTMENTS[model]
    assert api.varpro_class_slab_atoms(128, k, n_classes, 4 * n_classes) == 16  # both EM passes
    assert api.varpro_class_slab_atoms(128, k, n_classes, k + 1) == (48 if k == 1 else 16)  # the posterior: one slab, or three
    if k == 1:  # here the classes force it: twelve would still fit 32 atoms
        assert api.varpro_class_slab_atoms(128, 1, 12, 48) == 32 and api.varpro_class_slab_atoms(128, 1, 13, 52) == 16
    for c in _cases()[f"min-slab-{model}"]:
        G = c["atoms"].shape[1]
        assert G == 33
        _posterior(gpu, c)
        lab = (np.arange(c["y"].shape[0]) % n_classes).astype(np.int32)
        rows = _rows(n_classes, G)
        got = gpu.varpro_prior_em_classes(*_args(c), lab, n_classes, log_prior=rows, n_iter=1, rel_tol=0.0, **call_kw(c))
        l0, eps0, fin = likelihoods(*_args(c), **ref_kw(c))
        _note(f"EM {n_classes} classes", c, accept_em(got, l0, eps0, fin, lab, normalise_rows(rows, n_classes, G), 0.0, 1))

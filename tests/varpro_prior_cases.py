"""The inputs of the one-update GPU cases of tests/test_gpu_varpro_prior.py, by name: that file runs them on the device,
tests/test_varpro_prior_host.py runs the reference alone on every one of them (its precondition eps_v <= the case's cap: 1e-6 in
wide_box, the explicit 1e-3 for the narrow box only).  The choice of inputs is made here, on the CPU.  A case is
tests/varpro_marginal_cases.py's dict(model, b, y, atoms, lo, hi, noise_sd, marginal, max_eps, kw): most are that file's own --
the same kernel axes (a strip is 16 voxels and a block 64, a tile 16 atoms, the register file is sized for n_b <= 32 or <= 128) --
and this file adds what the EM's kernels take differently: their own slab width at two compartments and 128 b-values.

n_b = K + 1 at K = 2, 3 is left out for 4.1l's reason: three or four points spread over 0..1000 leave the columns of the fast
rates numerically dependent, and the reference's own precondition (eps_v <= 1e-6) refuses the case; K + 1 is covered at K = 1."""
from __future__ import annotations

import itertools

import numpy as np
from varpro_marginal_cases import CUS, NOISE_SD, _case, call_kw, ref_kw  # noqa: F401  (call_kw / ref_kw re-exported)
from varpro_marginal_cases import cases as marginal_cases

from pyneapple_amd import api

KEEP = ("voxels-", "atoms-", "n_b-", "layout-", "free-t1", "sigma", "first-tile-excluded", "middle-tile-excluded", "narrow-box")


def wide_pairs(n_atoms):
    """The first n_atoms ordered pairs (D1 > D2) of 18 rates over three decades that are at least two list places apart (136)."""
    rates = list(np.geomspace(3e-4, 0.3, 18))
    pairs = [(a, c) for (i, a), (j, c) in itertools.product(enumerate(rates), repeat=2) if i - j >= 2]
    assert len(pairs) >= n_atoms
    return np.ascontiguousarray(np.array(pairs[:n_atoms]).T)


def cases():
    c = {k: v for k, v in marginal_cases().items() if k.startswith(KEEP)}
    # two slabs with the second partly filled: at three compartments the EM's slab is the posterior's (48 atoms at 32 b-values: the
    # "atoms-64" case above); at two it is narrower, so both edges are crossed
    post, prior = api.varpro_posterior_slab_atoms(32, 2), api.varpro_prior_slab_atoms(32, 2)
    assert (post, prior) == (96, 80) and api.varpro_prior_slab_atoms(32, 3) == api.varpro_posterior_slab_atoms(32, 3) == 48
    c["atoms-bi-posterior-slab+16"] = _case("bi_s0", 50, atoms=wide_pairs(post + 16), noise_sd=NOISE_SD)
    c["atoms-bi-prior-slab+16"] = _case("bi_reduced", 50, atoms=wide_pairs(prior + 16))
    c["n_b-mono-128"] = _case("mono", 40, n_b=128)
    c["n_b-bi_s0-128"] = _case("bi_s0", 40, n_b=128, noise_sd=NOISE_SD)
    return c

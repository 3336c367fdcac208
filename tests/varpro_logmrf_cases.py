"""The inputs of the GPU cases of tests/test_gpu_varpro_logmrf.py, shared with tests/test_varpro_logmrf_host.py, which runs the numpy
reference alone on every one of them and so checks its eps_v preconditions (eps_v <= 1e-6) without a GPU.  Built on
tests/varpro_mrf_cases.py; every case carries "coupling": "log", "linear" or a per-row list.  Nothing here touches the device."""
from __future__ import annotations

import numpy as np
import varpro_mrf_cases as cases
from varpro_posterior_reference import apart_atoms, wide_box
from varpro_reference import case_signals

from pyneapple_amd import api

MODELS, NOISE_SD, table = cases.MODELS, cases.NOISE_SD, cases.table


def range_case(n_b):
    """200 bi_s0 voxels for the first x count ranges at 4, 5 and 33 b-values (an odd n_b leaves a range's first row 8-byte aligned
    only).  At 4 and 5 b-values two exponentials and S0 are nearly degenerate: the 21 apart pairs miss the reference's eps_v
    precondition there (eps_v = 538 at 5), the 12 pairs of three fast and four slow rates keep it (7e-11)."""
    b, y = case_signals("bi_s0", 200, n_b=n_b)
    lo, hi = wide_box("bi_s0")
    far = np.ascontiguousarray(np.array([(a, c) for a in (0.2, 0.1, 0.05) for c in (0.0005, 0.001, 0.002, 0.003)]).T)
    return dict(model="bi_s0", b=b, y=y, nl_atoms=apart_atoms("bi_s0") if n_b > 8 else far, lo=lo, hi=hi,
                kw=dict(noise_sd=NOISE_SD, marginal=True), strength=16.0, coupling="log")


def layout_case(model, n_atoms, noise_sd=0.0, marginal=True):
    c = cases._layout_case(model, n_atoms, noise_sd, marginal)
    if n_atoms == "slab+16":  # the new slab width, which carries the field rows
        k = api.VARPRO_COMPARTMENTS[model]
        assert c["nl_atoms"].shape[1] == api.varpro_logmrf_slab_atoms(c["b"].size, k) + 16
    return dict(c, coupling="log")


def axes_case(n_b):
    """K = 3 with a free T1 at 16, 33 and 128 b-values, mixed coupling: the rates log, T1 linear (tri_reduced: f1 D1 f2 D2 D3 T1)."""
    return dict(cases.axes_case(n_b), coupling=[0, 1, 0, 1, 1, 0])


def t1_axes_case(model, n_b):
    """cases.axes_case for any K = 3 layout: a free T1 beside the rates (log) and the fractions / S0, T1 linear.  With axes_case
    (tri_reduced) these reach every form the register remedies touch: the row-split forms of all three classes (n_b <= 32) and
    the two-pass forms of the free and the reduced class (n_b > 32)."""
    import itertools

    from varpro_reference import TRI_RATES

    b = np.linspace(0.0, 1000.0, n_b)
    t1 = np.array([600.0, 1000.0, 1600.0])
    y, kw = cases._t1_signals(model, b, 83, t1)
    triples = list(itertools.product(*TRI_RATES))[::6][:11]
    atoms = np.ascontiguousarray(np.array([(*t, v) for t in triples for v in t1]).T)
    lo, hi = wide_box(model)
    names = api.MODEL_PARAM_NAMES[model]
    return dict(model=model, b=b, y=y, nl_atoms=atoms, lo=np.append(lo, 100.0), hi=np.append(hi, 5000.0),
                kw=dict(noise_sd=NOISE_SD, marginal=True, **kw), strength=16.0, coupling=[int(n.startswith("D")) for n in names] + [0])


def s0_wide_case(n_b):
    """tri_s0 without T1 above 32 b-values: the two-pass form of the S0 class, whose second pass exists for field_mean and delta."""
    return dict(cases.driver_case(83, "tri_s0", n_b), coupling="log")


def nan_case():
    """A voxel with a non-finite signal beside finite neighbours."""
    c = dict(cases.sigma_case(), coupling="log")
    c["kw"] = dict(noise_sd=NOISE_SD, marginal=True)
    c["y"] = c["y"].copy()
    c["y"][5, 3] = np.nan
    c["y"][40] = np.inf
    return c


GPU_CASES = {}
for _m in MODELS:
    for _a in (1, 17, "slab+16"):
        GPU_CASES[f"atoms-{_m}-{_a}"] = (lambda m=_m, a=_a: layout_case(m, a))
for _ns, _mg in ((0.0, False), (0.0, True), (NOISE_SD, True), (NOISE_SD, False)):  # both noise modes x both amplitude weights
    GPU_CASES[f"modes-{_ns}-{_mg}"] = (lambda ns=_ns, mg=_mg: layout_case("tri_s0", 17, ns, mg))
for _nb in (4, 5, 33):
    GPU_CASES[f"range-{_nb}"] = (lambda n=_nb: range_case(n))
for _nb in (16, 33, 128):
    GPU_CASES[f"axes-{_nb}"] = (lambda n=_nb: axes_case(n))
for _m, _nb in (("tri_full", 16), ("tri_s0", 16), ("tri_full", 33)):
    GPU_CASES[f"t1-{_m}-{_nb}"] = (lambda m=_m, n=_nb: t1_axes_case(m, n))
for _nb in (33, 128):
    GPU_CASES[f"s0-{_nb}"] = (lambda n=_nb: s0_wide_case(n))
GPU_CASES.update({"sigma": lambda: dict(cases.sigma_case(), coupling="log"), "lead-inf": lambda: dict(cases.lead_inf_case(), coupling="log"),
                  "nan": nan_case, "driver": lambda: dict(cases.driver_case(83), coupling="log")})

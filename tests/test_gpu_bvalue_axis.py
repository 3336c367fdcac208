"""The number of b-values is the one input axis that reshapes the curve-fit kernel at launch time: the LDS image of a block
grows with it and the launcher drops from 4 waves per block to 3, 2 and 1; its parity decides how the last value of a row is
loaded.  The rest of the suite stays at 64 b-values and below (one mono case at 128).  Here: the HIP path against the oracle
(pinned to SciPy up to 128 b-values by tests/test_oracle_trf.py::test_oracle_matches_scipy_at_65_to_128_bvalues) on both sides of
every block-shape boundary, for every number of free parameters, every option once above 64 b-values, and the odd-row tail.
Which block shape ran is read from the library's launch trace (PNX_LAUNCH_TRACE, include/pnx.h "Environment"), never computed.
Criteria: those of tests/test_gpu_curvefit.py (test_matches_oracle_seeded, test_sigma_matches_oracle_seeded), unchanged."""
from __future__ import annotations

import re

import numpy as np
import pytest
from conftest import pcov_norm_err, rel_err

pytestmark = pytest.mark.gpu
RTOL = 1e-4
TR, TM = 3000.0, 25.0

_CF_LINE = re.compile(r"\[pnx launch\] curvefit (.*)")


def curvefit_launches(err):
    """The curve-fit launches of a captured stderr: one dict of integers per `[pnx launch] curvefit key=value ...` line."""
    return [{k: int(v) for k, v in (kv.split("=") for kv in m.group(1).split())} for m in _CF_LINE.finditer(err)]


def traced(capfd, monkeypatch, fn):
    """(fn(), its curve-fit launch lines)."""
    monkeypatch.setenv("PNX_LAUNCH_TRACE", "1")
    capfd.readouterr()
    try:
        res = fn()
    finally:
        err = capfd.readouterr().err
        monkeypatch.delenv("PNX_LAUNCH_TRACE")
    launches = curvefit_launches(err)
    assert launches, "no launch line on stderr"
    return res, launches


def one_shape(launches, **want):
    """Every launch of the call used one instantiation and one block shape; returns its trace line."""
    first = launches[0]
    for l in launches:
        assert {k: l[k] for k in l if k != "grid"} == {k: first[k] for k in first if k != "grid"}, launches
    for k, v in want.items():
        assert first[k] == v, f"{k}: traced {first[k]}, expected {v}: {first}"
    return first


# kind -> (kernel model, synth model, signal scale, fixed positions, t1_mode, free parameters)
KINDS = {
    "mono_fixed_D": ("mono", "mono", 1.0, (1,), 0, 1),
    "mono": ("mono", "mono", 1.0, (), 0, 2),
    "bi_reduced": ("bi_reduced", "bi_reduced", 1.0, (), 0, 3),
    "bi_s0": ("bi_s0", "bi_reduced", 1000.0, (), 0, 4),
    "tri_reduced": ("tri_reduced", "tri_reduced", 1.0, (), 0, 5),
    "tri_s0": ("tri_s0", "tri_reduced", 1000.0, (), 0, 6),
    "tri_s0_t1": ("tri_s0", "tri_reduced", 1000.0, (), 1, 7),  # free T1 beside a free S0: only their product is determined
    "tri_fixed_D1": ("tri_reduced", "tri_reduced", 1.0, (1,), 0, 4),
    "tri_fixed_D2_D3": ("tri_reduced", "tri_reduced", 1.0, (3, 4), 0, 3),
    "tri_fixed_4": ("tri_reduced", "tri_reduced", 1.0, (1, 2, 3, 4), 0, 1),
    "mono_t1_fixed": ("mono", "mono", 1.0, (2,), 1, 2),
    "mono_steam_fixed": ("mono", "mono", 1.0, (2,), 2, 2),
}


def t1_factor(T1, t1_mode):
    return (1 - np.exp(-TR / T1)) * (np.exp(-TM / T1) if t1_mode == 2 else 1.0)


def make_case(kind, n_b, n_vox, seed, jac="fd", b=None):
    """(model, b, y, p0, lo, hi, keyword arguments shared by api.curvefit and oracle.curvefit) of a seeded case: the suite's
    synthetic signal (pyneapple_amd.synth, 1 % noise) with the start values and bounds of the seeded oracle tests.  Fixed
    parameters are per-voxel maps of the true values (what SegmentedFitter's second step carries over)."""
    from pyneapple_amd import api, synth

    model, base, scale, fixed_idx, t1_mode, n_free = KINDS[kind]
    bb, y, P = synth.make_numpy(base, n_vox, n_b, sigma=0.01, seed=seed)
    if b is not None:  # another b-value set: the same truth and noise on it
        rng = np.random.default_rng(seed)
        P = {k: rng.uniform(lo_, hi_, n_vox) for k, (lo_, hi_) in synth.TRUTH[base].items()}
        bb = np.asarray(b, float)
        y = synth._signal(np, base, bb, P) * (1.0 + 0.01 * rng.standard_normal((n_vox, len(bb))))
    y = y * scale
    names, p0, lo, hi = synth.shared_arrays(base)
    truth = [P[n] for n in names]
    if model.endswith("_s0"):
        p0, lo, hi = np.append(p0, 1000.0), np.append(lo, 1.0), np.append(hi, 5000.0)
        truth.append(np.full(n_vox, scale))
    kw = dict(jac=jac)
    if t1_mode:
        T1 = np.random.default_rng(seed + 1).uniform(800, 1600, n_vox)
        y = y * t1_factor(T1, t1_mode)[:, None]
        p0, lo, hi = np.append(p0, 1000.0), np.append(lo, 100.0), np.append(hi, 5000.0)
        truth.append(T1)
        kw.update(t1_mode=t1_mode, tr=TR, tm=TM if t1_mode == 2 else 0.0)
    assert len(p0) == len(api.MODEL_PARAM_NAMES[model]) + (1 if t1_mode else 0)
    if fixed_idx:
        free = [k for k in range(len(p0)) if k not in fixed_idx]
        assert len(free) == n_free
        kw.update(fixed_idx=list(fixed_idx), fixed_vals=np.stack([truth[k] for k in fixed_idx]), jac="analytic")
        p0, lo, hi = p0[free], lo[free], hi[free]
    return model, bb, np.ascontiguousarray(y), p0, lo, hi, kw


def check_seeded(r, o, label="", median=True):
    """The criteria of tests/test_gpu_curvefit.py::test_matches_oracle_seeded.  median=False leaves out the bound on the median
    error -- a statistic of a population, which a batch of one voxel is not (test_voxel_counts_against_one_wave_blocks)."""
    n_vox = len(r["status"])
    e = rel_err(r["popt"], o["popt"]).max(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        dc = np.abs(r["cost"] - o["cost"]) / np.abs(o["cost"])
    print(f"{label}: {n_vox} voxels, status sign differs {int(((r['status'] > 0) != (o['status'] > 0)).sum())}, beyond 1e-4 "
          f"{int((e > RTOL).sum())}, median {np.median(e):.2e}, nfev differs {int((r['nfev'] != o['nfev']).sum())}, "
          f"worst cost difference {np.nanmax(dc):.2e}")
    assert ((r["status"] > 0) == (o["status"] > 0)).all()
    assert (e <= RTOL).mean() >= 0.995, f"{(e > RTOL).sum()} of {n_vox} voxels differ by more than 1e-4"
    assert not median or np.median(e) < 1e-7
    assert (r["nfev"] == o["nfev"]).mean() > 0.99
    np.testing.assert_allclose(r["cost"], o["cost"], rtol=1e-5, atol=1e-300)


def check_sigma_seeded(r, o, label=""):
    """The criteria of tests/test_gpu_curvefit.py::test_sigma_matches_oracle_seeded (estimates, cost, status, covariance)."""
    e = rel_err(r["popt"], o["popt"]).max(axis=0)
    near = e <= RTOL
    with np.errstate(divide="ignore", invalid="ignore"):
        pe = pcov_norm_err(r["pcov"][near], o["pcov"][near])
    print(f"{label}: {len(e)} voxels, beyond 1e-4 {int((~near).sum())}, median {np.median(e):.2e}, pcov median {np.nanmedian(pe):.2e}")
    assert ((r["status"] > 0) == (o["status"] > 0)).all() and (r["status"] > 0).mean() > 0.99
    assert near.mean() >= 0.99 and np.median(e) < 1e-7
    assert np.allclose(r["cost"][near], o["cost"][near], rtol=1e-6)
    assert np.nanmedian(pe) < 1e-5


def check_product_and_cost(r, o, y, amp, t1_mode, label=""):
    """A free T1 beside a free amplitude: only amplitude x relaxation factor is identifiable (conftest.check_g7).  Its bounds:
    the product to 1e-5, the cost to 1e-6 relative + 1e-12 of the signal energy; the status sign on every voxel.  The
    identifiable parameters (everything but the amplitude and T1) under the seeded criteria: 99.5 % within rtol 1e-4."""
    prod = lambda q: q[amp] * t1_factor(q[-1], t1_mode)
    dp = np.abs(prod(r["popt"]) / prod(o["popt"]) - 1)
    scale = 0.5 * np.sum(y ** 2, axis=1)
    dcost = np.abs(r["cost"] - o["cost"])
    others = [k for k in range(r["popt"].shape[0]) if k not in (amp, r["popt"].shape[0] - 1)]
    e = rel_err(r["popt"][others], o["popt"][others]).max(axis=0)
    print(f"{label}: product worst {dp.max():.2e}, cost worst {np.max(dcost / o['cost']):.2e} relative, others beyond 1e-4 "
          f"{int((e > RTOL).sum())} of {len(e)}")
    assert ((r["status"] > 0) == (o["status"] > 0)).all()
    assert dp.max() < 1e-5
    assert (dcost <= 1e-6 * o["cost"] + 1e-12 * scale).all()
    assert (e <= RTOL).mean() >= 0.995


def device_fit(gpu, model, b, y, p0, lo, hi, *, fixed_idx=(), fixed_vals=None, jac="fd", order=None, want_pcov=True, **kw):
    """api.curvefit_device on HBM-resident copies of host arrays (shared p0 / bounds); results as numpy arrays."""
    import torch

    dev = torch.device("cuda", 0)
    n_vox, n_b = y.shape
    fpv = fixed_vals is not None and np.ndim(fixed_vals) == 2
    o = gpu.make_opts(model, n_b, fixed_idx, False, fpv, jac=jac, **kw)
    n = o.n_free
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    fx = None if fixed_vals is None else (up(fixed_vals, np.float64) if fpv else np.ascontiguousarray(fixed_vals, np.float64))
    out = dict(popt=torch.empty((n, n_vox), dtype=torch.float64, device=dev),
               pcov=torch.empty((n_vox, n, n), dtype=torch.float64, device=dev) if want_pcov else None,
               status=torch.empty(n_vox, dtype=torch.int8, device=dev), nfev=torch.empty(n_vox, dtype=torch.int32, device=dev),
               cost=torch.empty(n_vox, dtype=torch.float64, device=dev))
    gpu.curvefit_device(o, n_vox, b, up(y, np.float64), p0, lo, hi, fx, out["popt"], out["pcov"], out["status"], out["nfev"],
                        out["cost"], 0, torch.cuda.current_stream().cuda_stream, order=None if order is None else up(order, np.int32))
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def assert_same_bits(a, b, keep=None, label=""):
    for k in ("popt", "pcov", "status", "nfev", "cost"):
        if a[k] is None and b[k] is None:
            continue
        x, y = (np.moveaxis(v, -1, 0) if k == "popt" else v for v in (a[k], b[k]))  # voxel axis first
        if keep is not None:
            x, y = x[keep], y[keep]
        assert np.array_equal(x, y, equal_nan=True), f"{label}: {k} differs"


# ---------------------------------------------------------------------------------------------------------- block shapes
def test_wave_count_boundaries_read_from_the_trace(gpu, capfd, monkeypatch):
    """Five free parameters, every b-value count from 1 to 128, one voxel and one evaluation each, without and with a vector
    sigma: the traced block shape falls 4 -> 3 -> 2 -> 1 waves, each exactly once, between the counts the parity cases below
    straddle; the 1 / sigma table moves the 3 -> 2 step from 66 | 67 to 64 | 65 and leaves the others."""
    from pyneapple_amd import synth

    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    waves = {False: {}, True: {}}
    for n_b in range(1, 129):
        b, y, _ = synth.make_numpy("tri_reduced", 1, n_b, sigma=0.01, seed=n_b)
        for with_sigma in (False, True):
            sigma = np.full(n_b, 0.01) if with_sigma else None
            _, launches = traced(capfd, monkeypatch, lambda: gpu.curvefit("tri_reduced", b, y, p0, lo, hi, max_nfev=1, want_pcov=False, sigma=sigma))
            waves[with_sigma][n_b] = one_shape(launches, N=5, n_b=n_b, sigma=int(with_sigma))["waves"]
    steps = lambda w: [(n, w[n], w[n + 1]) for n in range(1, 128) if w[n] != w[n + 1]]
    assert steps(waves[False]) == [(38, 4, 3), (66, 3, 2), (118, 2, 1)], steps(waves[False])
    assert steps(waves[True]) == [(38, 4, 3), (64, 3, 2), (118, 2, 1)], steps(waves[True])
    assert waves[False][1] == 4 and waves[False][128] == 1


@pytest.mark.parametrize("n_b,waves", [(38, 4), (39, 3), (66, 3), (67, 2), (118, 2), (119, 1), (127, 1), (128, 1)])
@pytest.mark.parametrize("jac", ["fd", "analytic"])
def test_five_free_parameters_on_both_sides_of_every_block_shape(gpu, oracle, capfd, monkeypatch, jac, n_b, waves):
    """tri_reduced, all free: the last count of each block shape and the first of the next, 127 and 128 (one wave per block --
    a shape no other test launches); the shape is asserted from the launch line."""
    model, b, y, p0, lo, hi, kw = make_case("tri_reduced", n_b, 1500 + 1, seed=1000 + n_b, jac=jac)
    r, launches = traced(capfd, monkeypatch, lambda: gpu.curvefit(model, b, y, p0, lo, hi, **kw))
    one_shape(launches, N=5, FD=int(jac == "fd"), PV=0, T1=0, n_b=n_b, sigma=0, waves=waves)
    check_seeded(r, oracle.curvefit(model, b, y, p0, lo, hi, n_threads=8, **kw), f"tri_reduced {jac} n_b={n_b} waves={waves}")


@pytest.mark.parametrize("n_b", [97, 128])
@pytest.mark.parametrize("kind", ["mono_fixed_D", "mono", "bi_reduced", "bi_s0", "tri_s0", "tri_s0_t1"])
def test_every_other_number_of_free_parameters_above_64(gpu, oracle, capfd, monkeypatch, kind, n_b):
    """N = 1 (mono with D fixed), 2, 3, 4, 6 and 7 (tri_s0 with a free T1) at an odd count above 64 and at 128: the traced
    instantiation has that N; these never go below two waves per block."""
    n_free = KINDS[kind][5]
    model, b, y, p0, lo, hi, kw = make_case(kind, n_b, 1200 + 3, seed=2000 + n_b)
    r, launches = traced(capfd, monkeypatch, lambda: gpu.curvefit(model, b, y, p0, lo, hi, **kw))
    shape = one_shape(launches, N=n_free, n_b=n_b, T1=int(kind == "tri_s0_t1"))
    assert shape["waves"] >= 2
    o = oracle.curvefit(model, b, y, p0, lo, hi, n_threads=8, **kw)
    if kind == "tri_s0_t1":
        check_product_and_cost(r, o, y, amp=5, t1_mode=1, label=f"{kind} n_b={n_b}")
    else:
        check_seeded(r, o, f"{kind} n_b={n_b} waves={shape['waves']}")


@pytest.mark.parametrize("n_b", [65, 66])
def test_sigma_table_moves_a_block_shape_boundary(gpu, oracle, capfd, monkeypatch, n_b):
    """The same voxels without and with a vector sigma where the 1 KiB table of 1 / sigma costs a wave: the two launch lines
    differ (3 waves against 2), and each result matches its own oracle run."""
    model, b, y, p0, lo, hi, kw = make_case("tri_reduced", n_b, 1500 + 1, seed=3000 + n_b)
    sigma = 0.01 * (1.0 + b / 400.0)
    plain, l0 = traced(capfd, monkeypatch, lambda: gpu.curvefit(model, b, y, p0, lo, hi, **kw))
    weighted, l1 = traced(capfd, monkeypatch, lambda: gpu.curvefit(model, b, y, p0, lo, hi, sigma=sigma, absolute_sigma=True, **kw))
    s0, s1 = one_shape(l0, N=5, n_b=n_b, sigma=0), one_shape(l1, N=5, n_b=n_b, sigma=1)
    assert (s0["waves"], s1["waves"]) == (3, 2) and s1["lds"] != s0["lds"]
    check_seeded(plain, oracle.curvefit(model, b, y, p0, lo, hi, n_threads=8, **kw), f"plain n_b={n_b}")
    check_sigma_seeded(weighted, oracle.curvefit(model, b, y, p0, lo, hi, sigma=sigma, absolute_sigma=True, n_threads=8, **kw), f"sigma n_b={n_b}")
    assert np.median(rel_err(plain["popt"], weighted["popt"]).max(axis=0)) > 1e-6  # the weights do change the answer


@pytest.mark.parametrize("n_vox", [1, 63, 64, 65, 64 * 9 + 1])
def test_voxel_counts_against_one_wave_blocks(gpu, oracle, capfd, monkeypatch, n_vox):
    """128 b-values, five free parameters: blocks of ONE wave, 64 lanes.  Less than a block, exactly one, one voxel more, and
    many blocks plus one voxel.  Every count against the oracle on its own voxels (status sign, 99.5 % within rtol 1e-4,
    evaluation counts, cost), and bit for bit the first rows of the 577-voxel batch (a voxel's arithmetic is its own), which
    meets all the seeded criteria including the median error below 1e-7: the median of ONE voxel is that voxel's error (2.4e-7
    for the first one, far inside rtol 1e-4), so that bound is asserted on the batch the small counts are rows of."""
    big = 64 * 9 + 1
    model, b, y, p0, lo, hi, kw = make_case("tri_reduced", 128, big, seed=4000)
    r, launches = traced(capfd, monkeypatch, lambda: gpu.curvefit(model, b, y[:n_vox], p0, lo, hi, **kw))
    one_shape(launches, N=5, n_b=128, waves=1)
    check_seeded(r, oracle.curvefit(model, b, y[:n_vox], p0, lo, hi, n_threads=8, **kw), f"n_vox={n_vox}", median=n_vox >= 63)
    if n_vox < big:
        whole = gpu.curvefit(model, b, y, p0, lo, hi, **kw)
        check_seeded(whole, oracle.curvefit(model, b, y, p0, lo, hi, n_threads=8, **kw), f"the {big} voxels around n_vox={n_vox}")
        head = {k: (v[:, :n_vox] if k == "popt" else v[:n_vox]) for k, v in whole.items()}
        assert_same_bits(r, head, label=f"n_vox={n_vox} against the first rows of {big}")


# ---------------------------------------------------------------------------------------------------------- odd-row tail
# (kind, n_b, b-values or None for the suite's linspace(0, 1200, n_b)); one b-value = one free parameter
ODD_CASES = {1: ("mono_fixed_D", [400.0]), 3: ("mono", None), 65: ("tri_reduced", None), 127: ("tri_reduced", None)}


def _orders(n_vox):
    return {"none": None, "reversed": np.arange(n_vox - 1, -1, -1), "shuffled": np.random.default_rng(n_vox).permutation(n_vox)}


@pytest.mark.parametrize("n_b", sorted(ODD_CASES))
def test_odd_row_tail_matches_the_oracle_in_any_queue_order(gpu, oracle, n_b):
    """An odd number of b-values: the last value of a row is loaded together with the first value of the NEXT row, the last row
    of the array on a path of its own.  Device-pointer fits in index order, in reversed order (the last row of the array is the
    first voxel pulled) and in a shuffled one return the same bits, and those match the oracle."""
    kind, bset = ODD_CASES[n_b]
    n_vox = 700 + 5
    model, b, y, p0, lo, hi, kw = make_case(kind, n_b, n_vox, seed=5000 + n_b, b=bset)
    want_pcov = n_b > KINDS[kind][5]  # the covariance divides by n_b - n_free
    runs = {name: device_fit(gpu, model, b, y, p0, lo, hi, order=order, want_pcov=want_pcov, **kw) for name, order in _orders(n_vox).items()}
    for name in ("reversed", "shuffled"):
        assert_same_bits(runs[name], runs["none"], label=f"n_b={n_b} order={name}")
    r = runs["none"]
    o = oracle.curvefit(model, b, y, p0, lo, hi, n_threads=8, **kw)
    if n_b == 1:
        # one measurement, one free parameter: the residual at the solution is ZERO, so the cost (1e-30 of the signal energy on
        # both sides) and the evaluation at which the iteration notices have no relative meaning.  Estimates on every voxel at
        # rtol 1e-4, status sign, and the cost against the signal energy (the fuzzer's floor: 1e-9 of 0.5 y^2).
        e = rel_err(r["popt"], o["popt"]).max(axis=0)
        print(f"n_b=1: worst {e.max():.2e}, cost worst {np.max(r['cost'] / (0.5 * y[:, 0] ** 2)):.2e} of the energy")
        assert ((r["status"] > 0) == (o["status"] > 0)).all() and (r["status"] > 0).all()
        assert e.max() <= RTOL and np.median(e) < 1e-7
        assert (np.abs(r["cost"] - o["cost"]) <= 1e-9 * 0.5 * y[:, 0] ** 2).all()
    else:
        check_seeded(r, o, f"odd tail {kind} n_b={n_b}")
    host = gpu.curvefit(model, b, y, p0, lo, hi, want_pcov=want_pcov, **kw)
    assert_same_bits(host, r, label=f"n_b={n_b} host arrays")


@pytest.mark.parametrize("order", ["none", "reversed", "shuffled"])
@pytest.mark.parametrize("n_b", sorted(ODD_CASES))
def test_odd_row_partner_value_never_reaches_a_result(gpu, n_b, order):
    """Leak test of the paired load: with the FIRST value of row i + 1 set to NaN, voxel i + 1 fails with status -2 (non-finite
    signal) and voxel i -- whose last value travelled with that NaN as its unused partner -- returns the bits of the clean run,
    as does every other voxel.  Rows: the second, one in the middle of a 64-lane tile, one across a tile boundary, and the last
    row of the array (whose predecessor is the last voxel with a paired load)."""
    kind, bset = ODD_CASES[n_b]
    n_vox = 300 + 3
    model, b, y, p0, lo, hi, kw = make_case(kind, n_b, n_vox, seed=6000 + n_b, b=bset)
    perm = _orders(n_vox)[order]
    clean = device_fit(gpu, model, b, y, p0, lo, hi, order=perm, want_pcov=False, **kw)
    assert (clean["status"] > 0).all()
    for i in (0, 37, 63, 127, n_vox - 2):
        dirty_y = y.copy()
        dirty_y[i + 1, 0] = np.nan
        dirty = device_fit(gpu, model, b, dirty_y, p0, lo, hi, order=perm, want_pcov=False, **kw)
        assert dirty["status"][i + 1] == -2, (i, dirty["status"][i + 1])
        keep = np.arange(n_vox) != i + 1
        assert_same_bits(dirty, clean, keep=keep, label=f"n_b={n_b} NaN at row {i + 1}")


# ---------------------------------------------------------------------------------------------------------- every option once
def test_per_voxel_start_values_and_bounds_above_64(gpu, oracle, capfd, monkeypatch):
    model, b, y, p0, lo, hi, kw = make_case("bi_reduced", 97, 1500 + 1, seed=7001)
    n_vox = len(y)
    rng = np.random.default_rng(7)
    p0v = np.tile(p0[:, None], (1, n_vox)) * rng.uniform(0.9, 1.1, (3, n_vox))
    lov = np.tile(lo[:, None], (1, n_vox)) * rng.uniform(0.8, 1.0, (3, n_vox))
    hiv = np.tile(hi[:, None], (1, n_vox)) * rng.uniform(1.0, 1.2, (3, n_vox))
    r, launches = traced(capfd, monkeypatch, lambda: gpu.curvefit(model, b, y, p0v, lov, hiv, **kw))
    one_shape(launches, N=3, PV=1, n_b=97)
    check_seeded(r, oracle.curvefit(model, b, y, p0v, lov, hiv, n_threads=8, **kw), "per-voxel p0 / bounds n_b=97")


@pytest.mark.parametrize("kind,n_b", [("tri_fixed_D1", 97), ("tri_fixed_D2_D3", 127), ("tri_fixed_4", 128)])
def test_per_voxel_fixed_maps_above_64(gpu, oracle, capfd, monkeypatch, kind, n_b):
    """One, two and four per-voxel fixed maps (analytic Jacobian): N = 4, 3 and 1 of tri_reduced's five parameters."""
    model, b, y, p0, lo, hi, kw = make_case(kind, n_b, 1500 + 1, seed=7100 + n_b)
    assert kw["fixed_vals"].shape == (5 - KINDS[kind][5], len(y))
    r, launches = traced(capfd, monkeypatch, lambda: gpu.curvefit(model, b, y, p0, lo, hi, **kw))
    one_shape(launches, N=KINDS[kind][5], FD=0, n_b=n_b)
    check_seeded(r, oracle.curvefit(model, b, y, p0, lo, hi, n_threads=8, **kw), f"{kind} n_b={n_b}")


@pytest.mark.parametrize("kind,n_b", [("mono_t1_fixed", 97), ("mono_steam_fixed", 128)])
def test_t1_factor_with_a_fixed_t1_map_above_64(gpu, oracle, capfd, monkeypatch, kind, n_b):
    model, b, y, p0, lo, hi, kw = make_case(kind, n_b, 1500 + 1, seed=7200 + n_b)
    r, launches = traced(capfd, monkeypatch, lambda: gpu.curvefit(model, b, y, p0, lo, hi, **kw))
    one_shape(launches, N=2, T1=1, n_b=n_b)
    check_seeded(r, oracle.curvefit(model, b, y, p0, lo, hi, n_threads=8, **kw), f"{kind} n_b={n_b}")


def test_covariance_at_128_b_values(gpu, oracle):
    """want_pcov on one-wave blocks: the covariance epilogue against the oracle's, where the oracle's own covariance is numerically
    meaningful (cond < 1e10) and the estimates agree -- the pcov_norm_err bar of test_fd_matches_reference_golden."""
    model, b, y, p0, lo, hi, kw = make_case("tri_reduced", 128, 1500 + 1, seed=7300)
    r = gpu.curvefit(model, b, y, p0, lo, hi, want_pcov=True, **kw)
    o = oracle.curvefit(model, b, y, p0, lo, hi, n_threads=8, **kw)
    check_seeded(r, o, "pcov n_b=128")
    sel = (o["status"] > 0) & (rel_err(r["popt"], o["popt"]).max(axis=0) <= RTOL)
    cond = np.array([np.linalg.cond(c) if np.isfinite(c).all() else np.inf for c in o["pcov"][sel]])
    good = cond < 1e10
    assert good.mean() > 0.5
    e = pcov_norm_err(r["pcov"][sel][good], o["pcov"][sel][good])
    print(f"pcov: {int(good.sum())} voxels, median {np.median(e):.2e}, beyond 1e-2: {int((e >= 1e-2).sum())}")
    assert np.median(e) < 1e-5 and (e < 1e-2).mean() > 0.97
    no = gpu.curvefit(model, b, y, p0, lo, hi, want_pcov=False, **kw)
    assert no["pcov"] is None and np.array_equal(no["popt"], r["popt"])


def test_float32_arrays_at_127_b_values(gpu, monkeypatch):
    """fp32 storage equals the fp64 entry point on the widened inputs, rounded (tests/test_gpu_f32_io.py), on an odd count and
    one-wave blocks, through several ragged chunks of the ring."""
    model, b, y, p0, lo, hi, kw = make_case("tri_reduced", 127, 3000 + 5, seed=7400)
    monkeypatch.setenv("PNX_HOST_CHUNK", "1024")
    r32 = gpu.curvefit(model, b, y.astype(np.float32), p0, lo, hi, **kw)
    w = lambda a: np.asarray(a, np.float32).astype(np.float64)
    r64 = gpu.curvefit(model, w(b), w(y), w(p0), w(lo), w(hi), **kw)
    assert r32["popt"].dtype == np.float32 and r32["pcov"].dtype == np.float32 and r32["cost"].dtype == np.float32
    np.testing.assert_array_equal(r32["status"], r64["status"])
    np.testing.assert_array_equal(r32["nfev"], r64["nfev"])
    np.testing.assert_array_equal(r32["popt"], r64["popt"].astype(np.float32))
    np.testing.assert_array_equal(r32["pcov"], r64["pcov"].astype(np.float32))
    np.testing.assert_array_equal(r32["cost"], r64["cost"].astype(np.float32))
    assert (r64["status"] > 0).mean() > 0.99


def test_device_pointer_call_at_128_b_values(gpu, oracle, capfd, monkeypatch):
    model, b, y, p0, lo, hi, kw = make_case("tri_reduced", 128, 2000 + 7, seed=7500)
    r, launches = traced(capfd, monkeypatch, lambda: device_fit(gpu, model, b, y, p0, lo, hi, **kw))
    one_shape(launches, N=5, n_b=128, waves=1, STREAM=0)
    check_seeded(r, oracle.curvefit(model, b, y, p0, lo, hi, n_threads=8, **kw), "device pointers n_b=128")
    assert_same_bits(gpu.curvefit(model, b, y, p0, lo, hi, **kw), r, label="host arrays against device pointers")


def test_more_than_128_b_values_is_refused_on_the_host(gpu):
    from pyneapple_amd import _lib, synth

    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    with pytest.raises(_lib.PnxError):
        gpu.curvefit("tri_reduced", np.linspace(0, 1200, 129), np.ones((3, 129)), p0, lo, hi)

"""Streaming rate of the two kernels of csrc/pnx_predict.hip and the end-to-end cost of R^2 for an NNLS volume.

    python profiles/fit_stats_probe.py [--vox 1048576] [--reps 7] [--skip-e2e]

Prints one JSON line per measurement.  Kernel times are HIP events around one launch on device-resident tensors, after two
warm-up launches, `reps` repetitions; median and min .. max are reported.  GB/s counts the algorithmic bytes only
(stats: 8 (n_bins + n_meas + 1) per voxel; predict: 8 (n_free + n_x) per voxel) and is given as a fraction of the 5.6 TB/s the
sweep kernel reaches, this repository's demonstrated streaming rate.
The end-to-end part times HipPixelWiseFitter._assemble on host arrays, default path against device_stats=True, alternating,
three runs each (the default path is the parent's numpy arithmetic, unchanged).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SWEEP_TBS = 5.6


def timed(fn, reps):
    import torch

    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def report(name, n_vox, bytes_per_vox, t):
    gbs = n_vox * bytes_per_vox / (t[0] * 1e-3) / 1e9
    print(json.dumps({"what": name, "n_vox": n_vox, "bytes_per_voxel": bytes_per_vox, "ms_median": round(t[0], 4), "ms_min": round(t[1], 4),
                      "ms_max": round(t[2], 4), "GBps": round(gbs, 1), "fraction_of_sweep_rate": round(gbs / (SWEEP_TBS * 1e3), 3)}), flush=True)


def main():
    import torch

    from pyneapple_amd import api, synth

    ap = argparse.ArgumentParser()
    ap.add_argument("--vox", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    n = a.vox
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)

    # ---- nnls_fit_stats_kernel: 250 bins x 32 b-values, ss_res only
    bins, basis, _ = synth.nnls_matrices(32)
    plan = api.NnlsPlan(basis, None, 0)
    coeff = torch.rand((n, basis.shape[1]), dtype=torch.float64, device=dev, generator=g)
    y = torch.rand((n, 32), dtype=torch.float64, device=dev, generator=g)
    report("nnls_fit_stats ss_res only 250x32", n, 8 * (basis.shape[1] + 32 + 1), timed(lambda: plan.fit_stats(y, coeff), a.reps))
    report("nnls_fit_stats ss_res + pred 250x32", n, 8 * (basis.shape[1] + 2 * 32 + 1), timed(lambda: plan.fit_stats(y, coeff, want_pred=True), a.reps))
    del coeff, y

    # ---- model_predict_kernel: triexp (tri_reduced), 32 x-values, pred only: 40 B in + 256 B out
    x = np.linspace(0.0, 1000.0, 32)
    p = torch.rand((5, n), dtype=torch.float64, device=dev, generator=g) * 0.01
    report("model_predict tri_reduced 32 x-values", n, 8 * (5 + 32), timed(lambda: api.predict("tri_reduced", x, p), a.reps))
    del p
    torch.cuda.empty_cache()
    if a.skip_e2e:
        plan.close()
        return

    # ---- end to end: _assemble of an NNLS volume from host arrays
    from pyneapple_amd.fitters import HipPixelWiseFitter
    from pyneapple_amd.models import NNLSModel

    rng = np.random.default_rng(0)
    model = NNLSModel(d_range=(float(bins[0]), float(bins[-1])), n_bins=int(bins.size))
    b = np.linspace(0.0, 1000.0, 32)
    coeffs = np.zeros((n, bins.size))
    cols = rng.integers(0, bins.size, (n, 4))
    coeffs[np.arange(n)[:, None], cols] = rng.uniform(0, 1000, (n, 4))
    pixels = np.empty((n, 32))
    B = np.asarray(model.get_basis(b))
    for s in range(0, n, 1 << 18):
        pixels[s:s + (1 << 18)] = coeffs[s:s + (1 << 18)] @ B.T
    pixels += rng.normal(0, 5.0, pixels.shape)

    class Solver:
        reg_order, device, pixel_results_ = 2, 0, None

        def __init__(self):
            self.model = model
            self.params_ = {"coefficients": coeffs}
            self.diagnostics_ = {"status": np.ones(n, np.int8), "residual": np.zeros(n)}

    fitters = {"default": HipPixelWiseFitter(Solver()), "device_stats": HipPixelWiseFitter(Solver(), device_stats=True)}
    for f in fitters.values():
        f.image_shape, f.pixel_indices, f.fitted_params_ = (n, 1, 1, 32), None, {"coefficients": coeffs}
    times = {k: [] for k in fitters}
    r2 = {}
    for rep in range(4):  # the first round warms both paths up and is dropped
        for k, f in fitters.items():
            t0 = time.perf_counter()
            r2[k] = f._assemble(b, pixels, 0.0).r_squared
            if rep:
                times[k].append(time.perf_counter() - t0)
    print(json.dumps({"what": "_assemble NNLS 250x32 from host arrays", "n_vox": n,
                      "seconds": {k: [round(t, 3) for t in v] for k, v in times.items()},
                      "max_abs_r2_difference": float(np.nanmax(np.abs(r2["default"] - r2["device_stats"])))}), flush=True)
    plan.close()


if __name__ == "__main__":
    main()

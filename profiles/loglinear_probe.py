#!/usr/bin/env python
"""The log-linear mono-exponential fit (pnx_loglinear_f64 / _f32), measured: kernel time on a device-resident volume, bytes per
voxel, achieved TB/s and its share of the 8 TB/s HBM peak (the fp32 sweep probe reaches 5.7 TB/s), the same step-1 problem
through what the segmented fitter ran before -- api.curvefit_device, mono-exponential, finite-difference Jacobian, on the sliced
b-subset -- and the host-array call.

    python profiles/loglinear_probe.py [--out profiles/loglinear_probe.json] [--log2-voxels 22] [--resources-only]

Times are device events around the enqueued call (median, min and max of 7 runs behind 2 warm-up runs); the host-array call
is a host clock around the blocking call.  Bytes per voxel are counted from the shapes: the signal row in, parameters,
covariance, status, n_used and ss_res out."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from pyneapple_amd import _build, api  # noqa: E402

HBM_PEAK_TBS = 8.0
SWEEP_F32_TBS = 5.7  # what pnx_sweep_f32 reaches on the same card


def kernel_resources():
    src = os.path.join(_build.CSRC, "pnx_loglin.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.HIPCC, *_build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "l.o")]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            t = re.search(r"loglinear_kernelI([df])E", m.group(2))
            name = f"loglinear_kernel<{'double' if t.group(1) == 'd' else 'float'}>" if t else None
            if name:
                out[name] = {}
        elif name:
            out[name][m.group(1)] = int(m.group(2))
    lds = {f"n_b={n_b}": 2 * 64 * 8 * (n_b | 1) for n_b in (16, 32, 64, 128)}
    return {"kernels": out, "dynamic_lds_bytes (pnx_loglin_args.hpp loglin_lds_bytes)": lds,
            "blocks_per_CU_by_LDS (160 KB, one wave each)": {k: min(32, (160 * 1024) // v) for k, v in lds.items()}}


def timed(torch, dev, fn, runs=7, warm=2):
    ms = []
    for it in range(warm + runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize(dev)
        if it >= warm:
            ms.append(t0.elapsed_time(t1))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "loglinear_probe.json"))
    ap.add_argument("--log2-voxels", type=int, default=22)
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    if a.resources_only:
        out = {}
        if os.path.exists(a.out):
            with open(a.out) as fh:
                out = json.load(fh)
        out["resources"] = kernel_resources()
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
        return
    import torch

    n, n_b = 1 << a.log2_voxels, 32
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    b = np.linspace(0.0, 1200.0, n_b)
    keep = b >= 200  # the segmented fit's step-1 subset
    g = torch.Generator(device=dev).manual_seed(1)
    S0 = 200.0 + 1800.0 * torch.rand(n, 1, dtype=torch.float64, device=dev, generator=g)
    D = 3e-4 + 2.7e-3 * torch.rand(n, 1, dtype=torch.float64, device=dev, generator=g)
    y = S0 * torch.exp(-torch.from_numpy(b).to(dev)[None, :] * D)
    y *= 1.0 + 0.01 * torch.randn(n, n_b, dtype=torch.float64, device=dev, generator=g)
    del S0, D
    out = {"_source_ids": _build.source_ids(), "device": torch.cuda.get_device_name(0), "n_vox": n, "n_b": n_b, "runs": 7, "warmup": 2,
           "hbm_peak_TBs": HBM_PEAK_TBS, "sweep_f32_TBs": SWEEP_F32_TBS}

    def fit_rows(yd, dt, esize, tag):
        params, pcov, status, n_used, ss = e((2, n), dt), e((n, 2, 2), dt), e(n, torch.int8), e(n, torch.int32), e(n, dt)
        for key, kw, outs in ((f"{tag}_all_outputs", {}, (params, pcov, status, n_used, ss)),
                              (f"{tag}_all_outputs_mask_b>=200", {"bvalue_mask": keep}, (params, pcov, status, n_used, ss)),
                              (f"{tag}_all_outputs_n_reweight_2", {"n_reweight": 2}, (params, pcov, status, n_used, ss)),
                              (f"{tag}_params_only", {}, (params, None, None, None, None))):
            t = timed(torch, dev, lambda: api.loglinear_device(b, yd, *outs, 0, stream=s, **kw))
            per_vox = n_b * esize + 2 * esize + (0 if outs[1] is None else 4 * esize + 1 + 4 + esize)
            tbs = per_vox * n / t["median_ms"] / 1e9
            out[key] = dict(t, bytes_per_voxel=per_vox, TBs=tbs, share_of_hbm_peak=tbs / HBM_PEAK_TBS, share_of_sweep_f32=tbs / SWEEP_F32_TBS,
                            Mvox_per_s=n / t["median_ms"] / 1e3)
            print(key, json.dumps(out[key]), flush=True)
        assert int((status.cpu().numpy() == 1).sum()) == n

    fit_rows(y, torch.float64, 8, "f64")
    y32 = y.to(torch.float32)
    fit_rows(y32, torch.float32, 4, "f32")
    del y32

    # ---- the step 1 the segmented fitter ran before: the bounded TRF fit of the mono-exponential model on the sliced subset
    ys = y[:, torch.from_numpy(keep).to(dev)].contiguous()
    nb1 = int(keep.sum())
    o = api.make_opts("mono", nb1, jac="fd")
    p0, lo, hi = np.array([1000.0, 1e-3]), np.array([1.0, 1e-5]), np.array([5000.0, 0.1])
    popt, pcov, status, nfev, cost = e((2, n), torch.float64), e((n, 2, 2), torch.float64), e(n, torch.int8), e(n, torch.int32), e(n, torch.float64)
    t_trf = timed(torch, dev, lambda: api.curvefit_device(o, n, b[keep], ys, p0, lo, hi, None, popt, pcov, status, nfev, cost, 0, s))
    t_slice = timed(torch, dev, lambda: y[:, torch.from_numpy(keep).to(dev)].contiguous())
    out["step1_before (curvefit mono, FD Jacobian, sliced b >= 200)"] = dict(t_trf, n_b=nb1, mean_nfev=float(nfev.float().mean().item()),
                                                                             device_slice_ms=t_slice["median_ms"])
    out["step1_ratio_before_over_loglinear_masked"] = t_trf["median_ms"] / out["f64_all_outputs_mask_b>=200"]["median_ms"]
    print("step1_before", json.dumps(out["step1_before (curvefit mono, FD Jacobian, sliced b >= 200)"]),
          "ratio", out["step1_ratio_before_over_loglinear_masked"], flush=True)
    del ys, popt, pcov, status, nfev, cost

    # ---- the host-array call (pageable numpy memory through the chunk ring), and the host slice the masked call replaces
    yh = y.cpu().numpy()
    del y
    api.loglinear(b, yh[: 1 << 16], bvalue_mask=keep)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        api.loglinear(b, yh, bvalue_mask=keep)
        host.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    np.ascontiguousarray(yh[:, keep])
    out["host_array_call_mask_b>=200"] = {"median_ms": float(np.median(host)), "min_ms": float(min(host)), "max_ms": float(max(host)),
                                          "runs": 3, "input_GB": yh.nbytes / 1e9}
    out["host_slice_of_the_subset_numpy_ms"] = (time.perf_counter() - t0) * 1e3
    print("host", json.dumps(out["host_array_call_mask_b>=200"]), "slice", out["host_slice_of_the_subset_numpy_ms"], flush=True)
    out["resources"] = kernel_resources()
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""The exponential-peeling fit (pnx_peel_f64 / _f32), measured on a device-resident volume of 2^22 voxels x 32 b-values:

  * kernel time, bytes per voxel and achieved TB/s for the bi-S0 and tri-S0 layouts in fp64 and fp32 storage, beside
    pnx_loglinear_f64 on the same volume (the closest kernel of the commit before);
  * the curve fit of the same volume at 1 % and 5 % noise started from the shared p0, from p0_grid (a 1024-atom dictionary) and
    from the peel: mean nfev, step time including the start-value kernel, and the share of voxels within rtol 1e-4 of the
    shared-p0 result.

    python profiles/peel_probe.py [--out profiles/peel_probe.json] [--log2-voxels 22] [--resources-only]

Times are device events around the enqueued calls (median, min and max of 7 runs behind 2 warm-up runs).  Bytes per voxel are
counted from the shapes: the signal row in, parameters, status, n_used and ss_res out."""
import argparse
import itertools
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from pyneapple_amd import _build, api  # noqa: E402

HBM_PEAK_TBS = 8.0
N_B = 32
SETUP = {
    "bi_s0": dict(thresholds=[150.0], p0=[0.2, 0.05, 1e-3, 1000.0], lo=[0.0, 5e-3, 1e-5, 1.0], hi=[1.0, 0.5, 5e-3, 5000.0],
                  grid=[np.linspace(0.05, 0.6, 8), np.geomspace(0.01, 0.3, 16), np.geomspace(3e-4, 3e-3, 8), [1000.0]]),
    "tri_s0": dict(thresholds=[30.0, 250.0], p0=[0.2, 0.2, 0.3, 0.012, 1.2e-3, 1000.0], lo=[0.0, 0.05, 0.0, 5e-3, 1e-5, 1.0],
                   hi=[1.0, 1.0, 1.0, 0.05, 5e-3, 5000.0],
                   grid=[np.linspace(0.1, 0.4, 4), np.geomspace(0.08, 0.5, 4), np.linspace(0.1, 0.4, 4), np.geomspace(6e-3, 0.03, 4),
                         np.geomspace(5e-4, 3e-3, 4), [1000.0]]),
}


def kernel_resources():
    src = os.path.join(_build.CSRC, "pnx_peel.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.HIPCC, *_build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "p.o")]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            t = re.search(r"peel_kernelI([df])E", m.group(2))
            name = f"peel_kernel<{'double' if t.group(1) == 'd' else 'float'}>" if t else None
            if name:
                out[name] = {}
        elif name:
            out[name][m.group(1)] = int(m.group(2))
    lds = {f"n_b={n_b}": 2 * 64 * 8 * (n_b | 1) for n_b in (16, 32, 64, 128)}
    return {"kernels": out, "dynamic_lds_bytes (pnx_peel_args.hpp peel_lds_bytes)": lds,
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


def bvalues():
    return np.unique(np.round(np.concatenate([[0.0], np.geomspace(5.0, 1200.0, N_B - 1)]), 3))


def volume(torch, dev, model, n, b, noise, seed):
    """(n, 32) float64 on the device: the layout's signal with S0 in [200, 2000] and additive Gaussian noise of noise * S0."""
    g = torch.Generator(device=dev).manual_seed(seed)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(n, 1, dtype=torch.float64, device=dev, generator=g)
    bd = torch.from_numpy(b).to(dev)[None, :]
    S0, Ds = u(200.0, 2000.0), u(8e-4, 2e-3)
    if model == "bi_s0":
        f, Df = u(0.15, 0.35), u(0.02, 0.08)
        s = f * torch.exp(-bd * Df) + (1 - f) * torch.exp(-bd * Ds)
    else:
        f2, D2, f1, D1 = u(0.2, 0.35), u(0.008, 0.02), u(0.15, 0.3), u(0.1, 0.3)
        s = f1 * torch.exp(-bd * D1) + f2 * torch.exp(-bd * D2) + (1 - f1 - f2) * torch.exp(-bd * Ds)
    y = S0 * s
    y += noise * S0 * torch.randn(n, b.size, dtype=torch.float64, device=dev, generator=g)
    return y.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "peel_probe.json"))
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

    n = 1 << a.log2_voxels
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    b = bvalues()
    out = {"_source_ids": _build.source_ids(), "device": torch.cuda.get_device_name(0), "n_vox": n, "n_b": N_B, "runs": 7, "warmup": 2,
           "hbm_peak_TBs": HBM_PEAK_TBS, "kernel": {}, "curvefit_start": {}}

    def save():
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    # ---- the kernel beside pnx_loglinear_f64 on the same volume
    for model, cfg in SETUP.items():
        K, npar = api.PEEL_STAGES[model], len(api.MODEL_PARAM_NAMES[model])
        y = volume(torch, dev, model, n, b, 0.01, 1)
        for tag, dt, esize, yd in (("f64", torch.float64, 8, y), ("f32", torch.float32, 4, None)):
            yd = y.to(torch.float32) if yd is None else yd
            params, status, n_used, ss = e((npar, n), dt), e(n, torch.int8), e((K, n), torch.int32), e(n, dt)
            for key, outs in ((f"{model}_{tag}_all_outputs", (params, status, n_used, ss)), (f"{model}_{tag}_params_only", (params, None, None, None))):
                t = timed(torch, dev, lambda: api.peel_device(b, yd, model, *outs, 0, b_thresholds=cfg["thresholds"], clip=(cfg["lo"], cfg["hi"]),
                                                              fallback=cfg["p0"], stream=s))
                per_vox = N_B * esize + npar * esize + (0 if outs[1] is None else 1 + 4 * K + esize)
                tbs = per_vox * n / t["median_ms"] / 1e9
                out["kernel"][key] = dict(t, bytes_per_voxel=per_vox, TBs=tbs, share_of_hbm_peak=tbs / HBM_PEAK_TBS, Mvox_per_s=n / t["median_ms"] / 1e3)
                print(key, json.dumps(out["kernel"][key]), flush=True)
            st = status.cpu().numpy()
            out["kernel"][f"{model}_{tag}_status_counts"] = {str(k): int((st == k).sum()) for k in (-2, 0, 1, 2)}
            del params, status, n_used, ss
        if model == "bi_s0":
            params, pcov, status, n_used, ss = e((2, n), torch.float64), e((n, 2, 2), torch.float64), e(n, torch.int8), e(n, torch.int32), e(n, torch.float64)
            t = timed(torch, dev, lambda: api.loglinear_device(b, y, params, pcov, status, n_used, ss, 0, stream=s))
            per_vox = N_B * 8 + 2 * 8 + 4 * 8 + 1 + 4 + 8
            tbs = per_vox * n / t["median_ms"] / 1e9
            out["kernel"]["loglinear_f64_all_outputs_same_volume"] = dict(t, bytes_per_voxel=per_vox, TBs=tbs, share_of_hbm_peak=tbs / HBM_PEAK_TBS)
            print("loglinear", json.dumps(out["kernel"]["loglinear_f64_all_outputs_same_volume"]), flush=True)
            del params, pcov, status, n_used, ss
        del y
        save()

    # ---- the curve fit from three kinds of start values
    for model, cfg in SETUP.items():
        npar = len(api.MODEL_PARAM_NAMES[model])
        p0, lo, hi = (np.array(cfg[k], float) for k in ("p0", "lo", "hi"))
        atoms = np.ascontiguousarray(np.array(list(itertools.product(*cfg["grid"])), float).T)
        assert atoms.shape == (npar, 1024)
        o_shared = api.make_opts(model, N_B, jac="fd")
        o_pv = api.make_opts(model, N_B, per_voxel=True, jac="fd")
        o_grid = api.make_opts(model, N_B, jac="analytic")
        lo_t = torch.from_numpy(np.repeat(lo[:, None], n, axis=1).copy()).to(dev)
        hi_t = torch.from_numpy(np.repeat(hi[:, None], n, axis=1).copy()).to(dev)
        for noise in (0.01, 0.05):
            y = volume(torch, dev, model, n, b, noise, 2)
            popt, pcov, status, nfev, cost = e((npar, n), torch.float64), e((n, npar, npar), torch.float64), e(n, torch.int8), e(n, torch.int32), e(n, torch.float64)
            p0v, pst = e((npar, n), torch.float64), e(n, torch.int8)
            fit_pv = lambda: api.curvefit_device(o_pv, n, b, y, p0v, lo_t, hi_t, None, popt, pcov, status, nfev, cost, 0, s)

            def from_shared():
                api.curvefit_device(o_shared, n, b, y, p0, lo, hi, None, popt, pcov, status, nfev, cost, 0, s)

            def from_grid():
                api.grid_start_device(o_grid, n, b, y, atoms, None, lo, hi, True, p0v, None, None, 0, s)
                fit_pv()

            def from_peel():
                api.peel_device(b, y, model, p0v, pst, None, None, 0, b_thresholds=cfg["thresholds"], clip=(lo, hi), fallback=p0, stream=s)
                fit_pv()

            base = None
            for name, fn, start_only in (("shared_p0", from_shared, None),
                                         ("p0_grid_1024", from_grid, lambda: api.grid_start_device(o_grid, n, b, y, atoms, None, lo, hi, True, p0v, None, None, 0, s)),
                                         ("p0_peel", from_peel, lambda: api.peel_device(b, y, model, p0v, pst, None, None, 0, b_thresholds=cfg["thresholds"],
                                                                                        clip=(lo, hi), fallback=p0, stream=s))):
                t = timed(torch, dev, fn)
                r = dict(t, mean_nfev=float(nfev.float().mean().item()), max_nfev=int(nfev.max().item()),
                         p99_nfev=float(torch.quantile(nfev[: 1 << 20].float(), 0.99).item()), success_share=float((status > 0).float().mean().item()),
                         Mvox_per_s=n / t["median_ms"] / 1e3)
                if start_only is not None:
                    r["start_kernel_ms"] = timed(torch, dev, start_only)["median_ms"]
                if base is None:
                    base = popt.clone()
                    r["within_rtol_1e-4_of_shared_p0"] = 1.0
                else:
                    rel = ((popt - base).abs() / base.abs().clamp_min(1e-300)).amax(dim=0)
                    r["within_rtol_1e-4_of_shared_p0"] = float((rel <= 1e-4).float().mean().item())
                if name == "p0_peel":
                    st = pst.cpu().numpy()
                    r["p0_status_counts"] = {str(k): int((st == k).sum()) for k in (-2, 0, 1, 2)}
                out["curvefit_start"][f"{model}_noise_{noise:g}_{name}"] = r
                print(model, noise, name, json.dumps(r), flush=True)
            del y, popt, pcov, status, nfev, cost, p0v, pst, base
            save()
    out["resources"] = kernel_resources()
    save()


if __name__ == "__main__":
    main()

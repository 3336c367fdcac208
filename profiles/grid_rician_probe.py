#!/usr/bin/env python3
"""The grid posterior under a Rician likelihood (pnx_curvefit_grid_posterior_rician_f64) measured beside the
Gaussian call (pnx_curvefit_grid_posterior_f64, known noise) in the same process.  Device resident, HIP events, two warm-up runs
and the median of seven timed runs each; the Gaussian call is timed before and after the Rician one: the difference is the drift.

  time       2^20 tri-exponential reduced voxels, 32 b-values, 1024 atoms, Rician magnitudes at noise sd 0.02, known noise.  The
             ratio of the two calls and the cost per evaluation of h it implies: (t_rician - t_gaussian) / (n_vox n_atoms n_b).
  resources  --resources-only (no GPU): VGPR / AGPR / scratch / waves per SIMD of every kernel of pnx_grid_rician.hip from the
             compiler's summary for gfx950, merged into the JSON.
python profiles/grid_rician_probe.py [--out profiles/grid_rician_probe.json] [--log2-vox 20] [--resources-only | --time-only]"""
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
sys.path.insert(0, os.path.join(HERE, "profiles"))
from grid_start_probe import AXES, timed  # noqa: E402  the same 4^5 atoms and the same timing loop

from pyneapple_amd import _build, api, synth  # noqa: E402

NOTES = ("cost_per_h_ps is the difference of the two calls over n_vox * n_atoms * n_b: it holds the evaluation of h, the LDS reads "
         "of the signal rows and the narrower slab's extra loads together. That the correction loop is bound by the fp64 vector "
         "units (four divergent polynomial pieces per element, so a wave that meets several pieces pays for each) is read from the "
         "code, not from counters. The separable large-z form was not built: nothing was measured for it.")


def kernel_resources():
    src = os.path.join(_build.CSRC, "pnx_grid_rician.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.HIPCC, *_build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "g.o")]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    keys = {"VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch_bytes", "Occupancy [waves/SIMD]": "waves_per_simd", "TotalSGPRs": "sgpr"}
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            p = re.search(r"grid_rician_posterior_kernelILi(\d+)ELi(\d+)ELi(\d+)E", m.group(2))
            name = f"grid_rician_posterior_kernel<NS={p.group(1)}, NF={p.group(2)}, NW={p.group(3)}>" if p else "log_i0e_kernel" if "log_i0e_kernel" in m.group(2) else None
            if name:
                out[name] = {}
        elif name:
            out[name][keys[m.group(1)]] = int(m.group(2))
    return out


def measure(log2_vox):
    import torch

    dev = torch.device("cuda:0")
    n_vox, n_b, sd = 1 << log2_vox, 32, 0.02
    names, _, lo, hi = synth.shared_arrays("tri_reduced")
    atoms = np.ascontiguousarray(np.array(list(itertools.product(*[AXES[n] for n in names])), float).T)
    b, clean = synth.make_torch("tri_reduced", n_vox, n_b, dev, sigma=0.0)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    n1 = torch.randn(clean.shape, generator=g, dtype=torch.float64, device=dev)
    n2 = torch.randn(clean.shape, generator=g, dtype=torch.float64, device=dev)
    y = torch.hypot(clean + sd * n1, sd * n2).contiguous()
    del clean, n1, n2
    o = api.make_opts("tri_reduced", n_b, jac="analytic")
    n = atoms.shape[0]
    out = dict(mean=torch.empty((n, n_vox), dtype=torch.float64, device=dev), sd=torch.empty((n, n_vox), dtype=torch.float64, device=dev),
               map_p=torch.empty((n, n_vox), dtype=torch.float64, device=dev), map_atom=torch.empty(n_vox, dtype=torch.int32, device=dev),
               ev=torch.empty(n_vox, dtype=torch.float64, device=dev), ess=torch.empty(n_vox, dtype=torch.float64, device=dev))
    gauss = lambda: api.grid_posterior_device(o, n_vox, b, y, atoms, None, lo, hi, False, None, sd, out["mean"], out["sd"], out["map_atom"],
                                              out["map_p"], out["ev"], out["ess"], 0)
    rician = lambda: api.grid_posterior_rician_device(o, n_vox, b, y, atoms, None, lo, hi, None, sd, out["mean"], out["sd"], out["map_atom"],
                                                      out["map_p"], out["ev"], out["ess"], 0)
    t_g0 = timed(torch, dev, gauss)
    t_r = timed(torch, dev, rician)
    t_g1 = timed(torch, dev, gauss)
    pairs = n_vox * atoms.shape[1]
    res = dict(n_vox=n_vox, n_b=n_b, n_atoms=int(atoms.shape[1]), noise_sd=sd, gaussian_ms_before=t_g0["median_ms"], rician_ms=t_r["median_ms"],
               gaussian_ms_after=t_g1["median_ms"], gaussian_spread=[t_g0, t_g1], rician_spread=t_r)
    res["drift"] = res["gaussian_ms_after"] / res["gaussian_ms_before"] - 1.0
    res["ratio_rician_over_gaussian"] = res["rician_ms"] / res["gaussian_ms_before"]
    res["gaussian_ps_per_pair"] = res["gaussian_ms_before"] * 1e9 / pairs
    res["cost_per_h_ps"] = (res["rician_ms"] - res["gaussian_ms_before"]) * 1e9 / (pairs * n_b)
    res["separable_large_z_form"] = "not built"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "grid_rician_probe.json"))
    ap.add_argument("--log2-vox", type=int, default=20)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--time-only", action="store_true", help="skip the compiler's summary (it recompiles the unit)")
    a = ap.parse_args()
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            res = json.load(fh)
    if not a.time_only:
        res["resources"] = kernel_resources()
    res["source_id"] = _build.source_id("grid_rician")
    if not a.resources_only:
        res["time"] = measure(a.log2_vox)
        res["time"]["source_id"] = res["source_id"]
        res["notes"] = NOTES
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "notes"}, indent=1))


if __name__ == "__main__":
    main()

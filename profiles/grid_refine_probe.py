#!/usr/bin/env python3
"""The per-voxel fine grid (pnx_curvefit_grid_refine_f64) measured beside the coarse posterior call
(pnx_curvefit_grid_posterior_f64, known noise, 1024 atoms) in the same process.  Device resident, HIP events, two warm-up runs and
the median of seven timed runs each; the coarse call is timed before and after the fine one: the difference is the drift.

  time       2^20 tri-exponential reduced voxels, 32 b-values, 5^5 = 3125 fine atoms per voxel around the truth (half-width: a
             tenth of each parameter's range), known noise.  ps per (voxel, atom) pair of both calls.
  resources  --resources-only (no GPU): VGPR / AGPR / scratch / waves per SIMD of every instantiation of grid_refine_kernel from the
             compiler's summary for gfx950, merged into the JSON.
             The p0_grid-started TRF fit (pnx_curvefit_grid_start_f64 on the same 1024 atoms, then the per-voxel bounded fit, FD
             Jacobian, max_nfev 250) runs on the same voxels in the same process.
  accuracy   the 400-voxel worth population of tests/grid_refine_cases.py (reduced bi-exponential, 4 x 4 x 4 coarse grid, 1 % and 5 %
             noise): median |error| per parameter of the coarse posterior mean, of one and two fine levels and of the TRF fit started
             from the best coarse atom -- reported, not asserted.
  resources  as above.
Every hipcc run has its own timeout; the measuring steps have none of their own: run the probe as
  timeout -k 10 300 python profiles/grid_refine_probe.py --time-only
python profiles/grid_refine_probe.py [--out profiles/grid_refine_probe.json] [--log2-vox 20] [--resources-only | --time-only]"""
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
sys.path.insert(0, os.path.join(HERE, "tests"))
from grid_start_probe import AXES, timed  # noqa: E402  the same 4^5 coarse atoms and the same timing loop

from pyneapple_amd import _build, api, synth  # noqa: E402

NOTES = ("ps_per_pair is the call's time over n_vox * atoms per voxel. What bounds the fine kernel is supposed from the code, not read "
         "from counters: per atom and b-value three ds_read_b64 of the table (lanes of one read hold up to 5 different rows), the broadcast "
         "read of the signal and five fp64 fma / mul; the fp64 vector units should bound it at 32 b-values.")
MODELS = ["mono", "bi_reduced", "bi_s0", "bi_full", "tri_reduced", "tri_s0", "tri_full"]


def kernel_resources():
    src = os.path.join(_build.CSRC, "pnx_grid_refine.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.HIPCC, *_build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "g.o")]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True, timeout=600).stderr
    out, name = {}, None
    keys = {"VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch_bytes", "Occupancy [waves/SIMD]": "waves_per_simd", "TotalSGPRs": "sgpr"}
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            p = re.search(r"grid_refine_kernelILi(\d+)E", m.group(2))
            name = f"grid_refine_kernel<{MODELS[int(p.group(1))]}>" if p else None
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
    b, y = synth.make_torch("tri_reduced", n_vox, n_b, dev, sigma=sd)
    o = api.make_opts("tri_reduced", n_b, jac="analytic")
    n = atoms.shape[0]
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    out = dict(mean=new(n, n_vox), sd=new(n, n_vox), map_p=new(n, n_vox), map_atom=torch.empty(n_vox, dtype=torch.int32, device=dev),
               ev=new(n_vox), ess=new(n_vox), edge=new(n, n_vox), fmean=new(n, n_vox))
    coarse = lambda: api.grid_posterior_device(o, n_vox, b, y, atoms, None, lo, hi, False, None, sd, out["mean"], out["sd"], out["map_atom"],
                                               out["map_p"], out["ev"], out["ess"], 0)
    coarse()
    torch.cuda.synchronize()
    centre = out["mean"].clone()  # the coarse mean, formed and kept on the device
    width = torch.as_tensor(np.array([AXES[k][-1] - AXES[k][0] for k in names]) / 10.0, dtype=torch.float64, device=dev)
    half = (width[:, None] * torch.ones((1, n_vox), dtype=torch.float64, device=dev)).contiguous()
    npts = np.full(n, 5, np.int32)
    fine = lambda: api.grid_refine_device(o, n_vox, b, y, None, lo, hi, False, sd, npts, centre, half, out["fmean"], out["sd"], out["map_p"],
                                          out["ess"], out["ev"], out["edge"], 0)
    t_c0 = timed(torch, dev, coarse)
    t_f = timed(torch, dev, fine)
    t_c1 = timed(torch, dev, coarse)
    res = dict(n_vox=n_vox, n_b=n_b, coarse_atoms=int(atoms.shape[1]), fine_atoms=int(np.prod(npts)), noise_sd=sd, coarse_ms_before=t_c0["median_ms"],
               fine_ms=t_f["median_ms"], coarse_ms_after=t_c1["median_ms"], coarse_spread=[t_c0, t_c1], fine_spread=t_f)
    res["drift"] = res["coarse_ms_after"] / res["coarse_ms_before"] - 1.0
    res["coarse_ps_per_pair"] = res["coarse_ms_before"] * 1e9 / (n_vox * atoms.shape[1])
    res["fine_ps_per_pair"] = res["fine_ms"] * 1e9 / (n_vox * int(np.prod(npts)))
    # the p0_grid-started TRF fit on the same voxels: the dictionary search on the coarse atoms, then the per-voxel bounded fit
    st = torch.cuda.current_stream(dev).cuda_stream
    p0v, best, gcost = new(n, n_vox), torch.empty(n_vox, dtype=torch.int32, device=dev), new(n_vox)
    lo_t = torch.from_numpy(np.ascontiguousarray(np.repeat(lo[:, None], n_vox, 1))).to(dev)
    hi_t = torch.from_numpy(np.ascontiguousarray(np.repeat(hi[:, None], n_vox, 1))).to(dev)
    popt, pcov = new(n, n_vox), new(n_vox, n, n)
    status, nfev, cost = torch.empty(n_vox, dtype=torch.int8, device=dev), torch.empty(n_vox, dtype=torch.int32, device=dev), new(n_vox)
    o_pv = api.make_opts("tri_reduced", n_b, per_voxel=True, max_nfev=250, ftol=1e-8, jac="fd")
    search = lambda: api.grid_start_device(o, n_vox, b, y, atoms, None, lo, hi, False, p0v, best, gcost, 0, st)
    fit = lambda: api.curvefit_device(o_pv, n_vox, b, y, p0v, lo_t, hi_t, None, popt, pcov, status, nfev, cost, 0, st)
    t_trf = timed(torch, dev, lambda: (search(), fit()))
    res["trf_search_and_fit_ms"] = t_trf["median_ms"]
    res["trf_spread"] = t_trf
    res["trf_nfev_mean"] = float(nfev.float().mean().item())
    res["trf_failed_share"] = float((status <= 0).float().mean().item())
    res["coarse_plus_one_level_ms"] = res["coarse_ms_before"] + res["fine_ms"]
    res["ratio_trf_over_coarse_plus_one_level"] = res["trf_search_and_fit_ms"] / res["coarse_plus_one_level_ms"]
    return res


def accuracy():
    """Median |error| on the worth population: coarse posterior mean, one and two fine levels (device), the grid-started TRF fit."""
    import grid_refine_cases as K
    import grid_refine_reference as R

    atoms = np.ascontiguousarray(np.array(list(itertools.product(*K.WORTH_AXES))).T)
    run = lambda model, b, y, lo, hi, npts, centre, hw, noise_sd: api.grid_refine(model, b, y, lo, hi, npts, np.ascontiguousarray(centre),
                                                                                  np.ascontiguousarray(hw), noise_sd=noise_sd)
    out = {}
    for noise in K.WORTH_NOISE:
        p = K.worth_population(noise)
        n_vox = p["y"].shape[0]
        med = lambda m: [float(x) for x in np.median(np.abs(m - p["truth"]), axis=1)]
        lv = R.refine_levels("bi_reduced", p["b"], p["y"], K.WORTH_LO, K.WORTH_HI, K.WORTH_AXES, noise, points=5, levels=2, run=run)
        start = api.grid_start("bi_reduced", p["b"], p["y"], atoms, K.WORTH_LO, K.WORTH_HI)
        tile = lambda a: np.ascontiguousarray(np.repeat(a[:, None], n_vox, 1))
        fit = api.curvefit("bi_reduced", p["b"], p["y"], start["p0"], tile(K.WORTH_LO), tile(K.WORTH_HI), want_pcov=False)
        ok = fit["status"] > 0
        out[f"noise_{noise}"] = {"parameters": ["f1", "D1", "D2"], "coarse": med(lv[0]["mean"]), "refine_1_level": med(lv[1]["mean"]),
                                 "refine_2_levels": med(lv[2]["mean"]), "trf_grid_started": med(fit["popt"]),
                                 "trf_converged_share": float(ok.mean()), "trf_nfev_mean": float(fit["nfev"].mean())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "grid_refine_probe.json"))
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
    res["source_id"] = _build.source_id("grid_refine")
    if not a.resources_only:
        res["time"] = measure(a.log2_vox)
        res["time"]["source_id"] = res["source_id"]
        res["accuracy"] = accuracy()
        res["notes"] = NOTES
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "notes"}, indent=1))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The Bayesian grid posterior (pnx_curvefit_grid_posterior_f64), measured against the dictionary search it shares its MFMA product
with.  Device resident, HIP events, two warm-up runs and seven timed runs each.

  time       2^20 tri-exponential reduced voxels, 32 b-values, 1 % noise, 1024 atoms (the shape of DESIGN.md 4.1d): the new call
             with a known and with a marginalised noise scale, and pnx_curvefit_grid_start_f64 on the same inputs in the same
             process -- the yardstick.  per_pair_ns = (posterior - grid start) / (n_vox n_atoms): what the fold costs per pair.
  accuracy   2^16 voxels of synth.make_numpy (which returns the truth) at 1 % and 5 % noise: median absolute error against the
             truth of the posterior mean, the MAP atom and the p0_grid-started TRF fit, per parameter.  For the reader, not a gate.
  resources  --resources-only (no GPU): VGPR / AGPR / scratch of the posterior kernels from the compiler's summary for gfx950,
             merged into the JSON.
python profiles/grid_posterior_probe.py [--out profiles/grid_posterior_probe.json] [--log2-voxels 20] [--resources-only]"""
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


def kernel_resources():
    src = os.path.join(_build.CSRC, "pnx_grid_posterior.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.HIPCC, *_build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "g.o")]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            t = re.search(r"grid_posterior_kernelILi(\d+)ELi(\d+)ELb([01])E", m.group(2))
            name = f"grid_posterior_kernel<NS={t.group(1)}, NF={t.group(2)}, PROJ={t.group(3)}>" if t else None
            if name:
                out[name] = {}
        elif name:
            out[name][m.group(1)] = int(m.group(2))
    lds = {f"n_b={n_b}, n_free={nf}": api.grid_posterior_slab_atoms(n_b, nf) for n_b, nf in ((16, 5), (32, 5), (32, 8), (64, 5), (128, 8))}
    return {"kernels": out, "atoms_per_lds_slab (pnx_grid_posterior_args.hpp grid_posterior_slab)": lds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "grid_posterior_probe.json"))
    ap.add_argument("--log2-voxels", type=int, default=20)
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    if a.resources_only:
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
    names, p0, lo, hi = synth.shared_arrays("tri_reduced")
    atoms = np.ascontiguousarray(np.array(list(itertools.product(*[AXES[k] for k in names]))).T)
    n_atoms = atoms.shape[1]
    b = synth.bvalues(n_b)
    s = torch.cuda.current_stream(dev).cuda_stream
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    out = {"_source_ids": _build.source_ids(), "device": torch.cuda.get_device_name(0), "n_vox": n, "n_b": n_b, "n_atoms": n_atoms,
           "runs": 7, "warmup": 2, "atoms": {k: [float(x) for x in v] for k, v in AXES.items()}}
    o = api.make_opts("tri_reduced", n_b, jac="analytic")

    # ---- time
    y = synth.make_torch_rows("tri_reduced", 0, n, n_b, dev, sigma=0.01)[1]
    p0v, best, gcost = e((5, n), torch.float64), e(n, torch.int32), e(n, torch.float64)
    mean, sd, mp = e((5, n), torch.float64), e((5, n), torch.float64), e((5, n), torch.float64)
    atom, lev, ess = e(n, torch.int32), e(n, torch.float64), e(n, torch.float64)
    post = lambda nsd: api.grid_posterior_device(o, n, b, y, atoms, None, lo, hi, False, None, nsd, mean, sd, atom, mp, lev, ess, 0, s)
    t = {"grid_start": timed(torch, dev, lambda: api.grid_start_device(o, n, b, y, atoms, None, lo, hi, False, p0v, best, gcost, 0, s)),
         "posterior_known_noise (noise_sd 0.01)": timed(torch, dev, lambda: post(0.01)),
         "posterior_marginalised": timed(torch, dev, lambda: post(0.0))}
    g = t["grid_start"]["median_ms"]
    for key in ("posterior_known_noise (noise_sd 0.01)", "posterior_marginalised"):
        t[key]["ratio_to_grid_start"] = t[key]["median_ms"] / g
        t[key]["per_pair_ns"] = (t[key]["median_ms"] - g) * 1e6 / (float(n) * n_atoms)
    out["time"] = t
    print("time", json.dumps(t), flush=True)
    del y, p0v, best, gcost, mean, sd, mp, atom, lev, ess

    # ---- accuracy against the synthetic truth
    m = 1 << min(16, a.log2_voxels)
    tile = lambda v: np.ascontiguousarray(np.repeat(v[:, None], m, axis=1))
    for noise in (0.01, 0.05):
        _, yh, truth = synth.make_numpy("tri_reduced", m, n_b, sigma=noise)
        tr = np.stack([np.asarray(truth[k]) for k in names])
        res = api.grid_posterior("tri_reduced", b, yh, atoms, lo, hi, noise_sd=noise)
        gs = api.grid_start("tri_reduced", b, yh, atoms, lo, hi)
        fit = api.curvefit("tri_reduced", b, yh, gs["p0"], tile(lo), tile(hi), max_nfev=250, ftol=1e-8, jac="fd", want_pcov=False)
        med = lambda est: {k: float(np.median(np.abs(est[i] - tr[i]))) for i, k in enumerate(names)}
        r = {"n_vox": m, "posterior_mean": med(res["mean"]), "map_atom": med(res["map_p"]), "p0_grid_trf_fit": med(fit["popt"]),
             "ess_median": float(np.median(res["ess"])), "trf_nfev_mean": float(fit["nfev"].mean()),
             "posterior_sd_median": {k: float(np.median(res["sd"][i])) for i, k in enumerate(names)}}
        out[f"median_abs_error_noise_{noise}"] = r
        print(f"noise_{noise}", json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

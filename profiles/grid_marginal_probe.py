#!/usr/bin/env python3
"""The per-parameter marginals of the grid posterior (pnx_curvefit_grid_marginals_f64), measured beside the posterior and one EM
update, which run the same MFMA product.  Device resident, HIP events, two warm-up runs and seven timed runs each.

  time       2^20 tri-exponential reduced voxels, 32 b-values, 1 % noise, 4^5 = 1024 atoms (the shape of DESIGN.md 4.1d / 4.1g /
             4.1j), B = 20 bins (the 2-chunk instantiation): the whole marginals call with three quantiles and log_evidence, the
             same without quantiles and log_evidence (no quantile kernel), pnx_curvefit_grid_posterior_f64 and one n_iter = 1 EM call
             (two normaliser passes, one accumulate pass) on the same inputs in the same process, known and marginalised noise.
             And a 16^3 bi-exponential grid (4096 atoms, B = 48: the 4-chunk instantiation) on the same number of voxels.
  passes     --kernel-stats FILE: the per-kernel times of a separate run of `--time-only` under a kernel trace (a *kernel_stats.csv),
             merged into the JSON: the marginal pass beside the EM's normaliser and accumulate passes.
  resources  --resources-only (no GPU): VGPR / AGPR / scratch / waves per SIMD of every instantiation from the compiler's summary
             for gfx950, merged into the JSON.
python profiles/grid_marginal_probe.py [--out profiles/grid_marginal_probe.json] [--log2-voxels 20] [--time-only] [--resources-only]
                                       [--kernel-stats FILE]"""
import argparse
import csv
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
    src = os.path.join(_build.CSRC, "pnx_grid_marginal.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.HIPCC, *_build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "g.o")]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            t = re.search(r"grid_marginal_kernelILi(\d+)ELb([01])ELi(\d+)E", m.group(2))
            name = f"grid_marginal_kernel<NS={t.group(1)}, PROJ={t.group(2)}, NC={t.group(3)}>" if t else \
                "grid_marginal_quantile_kernel" if "quantile_kernel" in m.group(2) else None
            if name:
                out[name] = {}
        elif name:
            out[name][m.group(1)] = int(m.group(2))
    return {"kernels": out,
            "note": "Occupancy is the register file's; a block holds up to 64 KB of the CU's 160 KB of LDS, so two blocks (two waves per SIMD) is the most that run."}


def kernel_stats(path):
    rows = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Name", "")
            if re.search(r"grid_(?:marginal|prior|posterior|dict)\w*", name):
                rows[name] = {"calls": int(r["Calls"]), "average_ms": float(r["AverageNs"]) * 1e-6, "total_ms": float(r["TotalDurationNs"]) * 1e-6}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "grid_marginal_probe.json"))
    ap.add_argument("--log2-voxels", type=int, default=20)
    ap.add_argument("--time-only", action="store_true")
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    if a.resources_only or a.kernel_stats:
        with open(a.out) as fh:
            out = json.load(fh)
        if a.resources_only:
            out["resources"] = kernel_resources()
        if a.kernel_stats:
            out["kernel_trace (separate run of --time-only under a kernel trace; every average spans both noise modes)"] = kernel_stats(a.kernel_stats)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
        return
    import torch

    n, n_b = 1 << a.log2_voxels, 32
    dev = torch.device("cuda", 0)
    b = synth.bvalues(n_b)
    s = torch.cuda.current_stream(dev).cuda_stream
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    out = {"_source_ids": _build.source_ids(), "device": torch.cuda.get_device_name(0), "n_vox": n, "n_b": n_b, "runs": 7, "warmup": 2}
    probs = [0.025, 0.5, 0.975]

    def measure(model, atoms, lo, hi, y):
        o = api.make_opts(model, n_b, jac="analytic")
        nf = atoms.shape[0]
        bins = api.grid_marginal_bins(atoms)
        B = int(bins[0].sum())
        mean, sd, mp = e((nf, n), torch.float64), e((nf, n), torch.float64), e((nf, n), torch.float64)
        atom, lev, ess = e(n, torch.int32), e(n, torch.float64), e(n, torch.float64)
        marg, quant = e((B, n), torch.float64), e((3, nf, n), torch.float64)
        post = lambda nsd: api.grid_posterior_device(o, n, b, y, atoms, None, lo, hi, False, None, nsd, mean, sd, atom, mp, lev, ess, 0, s)
        em = lambda nsd: api.grid_prior_em_device(o, n, b, y, atoms, None, lo, hi, False, None, nsd, 1, 0.0, 0.0, 0, s)
        full = lambda nsd: api.grid_marginals_device(o, n, b, y, atoms, None, lo, hi, False, None, nsd, *bins, probs, marg, quant, lev, 0, s)
        bare = lambda nsd: api.grid_marginals_device(o, n, b, y, atoms, None, lo, hi, False, None, nsd, *bins, [], marg, None, None, 0, s)
        t = {"n_atoms": int(atoms.shape[1]), "n_bins": B, "chunks": 2 if B <= 32 else 4 if B <= 64 else 8}
        for label, nsd in (("known_noise (noise_sd 0.01)", 0.01), ("marginalised", 0.0)):
            r = {"posterior": timed(torch, dev, lambda: post(nsd)), "prior_em_n_iter_1": timed(torch, dev, lambda: em(nsd)),
                 "marginals_3_quantiles_log_evidence": timed(torch, dev, lambda: full(nsd)),
                 "marginals_alone": timed(torch, dev, lambda: bare(nsd))}
            r["marginals_over_posterior"] = r["marginals_3_quantiles_log_evidence"]["median_ms"] / r["posterior"]["median_ms"]
            r["marginals_over_em_1"] = r["marginals_3_quantiles_log_evidence"]["median_ms"] / r["prior_em_n_iter_1"]["median_ms"]
            t[label] = r
        return t

    names, _, lo, hi = synth.shared_arrays("tri_reduced")
    atoms = np.ascontiguousarray(np.array(list(itertools.product(*[AXES[k] for k in names]))).T)
    y = synth.make_torch_rows("tri_reduced", 0, n, n_b, dev, sigma=0.01)[1]
    out["tri_reduced_4^5_atoms_20_bins"] = measure("tri_reduced", atoms, lo, hi, y)
    print("tri_reduced", json.dumps(out["tri_reduced_4^5_atoms_20_bins"]), flush=True)
    del y
    if not a.time_only:
        names, _, lo, hi = synth.shared_arrays("bi_reduced")
        axes = {"f1": np.linspace(0.05, 0.5, 16), "D1": np.geomspace(0.005, 0.09, 16), "D2": np.geomspace(2e-4, 3e-3, 16)}
        atoms = np.ascontiguousarray(np.array(list(itertools.product(*[axes[k] for k in names]))).T)
        y = synth.make_torch_rows("bi_reduced", 0, n, n_b, dev, sigma=0.01)[1]
        out["bi_reduced_16^3_atoms_48_bins"] = measure("bi_reduced", atoms, lo, hi, y)
        print("bi_reduced", json.dumps(out["bi_reduced_16^3_atoms_48_bins"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

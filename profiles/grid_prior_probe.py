#!/usr/bin/env python3
"""The empirical-Bayes prior over the grid (pnx_curvefit_grid_prior_em_f64), measured beside the posterior it shares its MFMA
product with.  Device resident, HIP events, two warm-up runs and seven timed runs each.

  time       2^20 tri-exponential reduced voxels, 32 b-values, 1 % noise, 1024 atoms (the shape of DESIGN.md 4.1d / 4.1g): the
             whole call at n_iter = 1, 2, 3 with rel_tol = 0 (n_iter updates and n_iter + 1 normaliser passes, each with its 16-byte
             read-back), known and marginalised noise, and pnx_curvefit_grid_posterior_f64 on the same inputs in the same process.
             one_iteration_ms = call(3) - call(2): a normaliser pass, an accumulate pass, the two small kernels and the read-back.
  passes     --kernel-stats FILE: the per-kernel times of a separate run of `--time-only` under a kernel trace (a *kernel_stats.csv),
             merged into the JSON: the normaliser and the accumulate pass on their own.
  accuracy   the 2^16 voxels of profiles/grid_posterior_probe.py (synth.make_numpy, which returns the truth) at 1 % and 5 % noise:
             median absolute error of the posterior mean under the uniform prior and under the prior learned in 30 updates.  The
             truths are uniform over the grid's own ranges: the case in which a learned prior has the least to add.
             And the narrow population of DESIGN.md 4.1j (bi_s0, 16 b-values, 384 atoms) at 1000 and at 37 voxels.
  resources  --resources-only (no GPU): VGPR / AGPR / scratch / waves per SIMD of every instantiation from the compiler's summary
             for gfx950, merged into the JSON.
python profiles/grid_prior_probe.py [--out profiles/grid_prior_probe.json] [--log2-voxels 20] [--time-only] [--resources-only]
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
    src = os.path.join(_build.CSRC, "pnx_grid_prior.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.HIPCC, *_build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "g.o")]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            t = re.search(r"(grid_prior_(?:norm|acc)_kernel)ILi(\d+)ELb([01])E", m.group(2))
            s = re.search(r"(grid_prior_(?:stats|finish)_kernel)", m.group(2))
            name = f"{t.group(1)}<NS={t.group(2)}, PROJ={t.group(3)}>" if t else s.group(1) if s else None
            if name:
                out[name] = {}
        elif name:
            out[name][m.group(1)] = int(m.group(2))
    lds = {f"n_b={n_b}": api.grid_prior_slab_atoms(n_b) for n_b in (16, 32, 64, 128)}
    return {"kernels": out, "atoms_per_lds_slab (pnx_grid_prior_args.hpp grid_prior_slab)": lds,
            "note": "Occupancy is the register file's; a block holds up to 64 KB of the CU's 160 KB of LDS, so two blocks (two waves per SIMD) is the most that run."}


def kernel_stats(path):
    rows = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Name", "")
            m = re.search(r"grid_(?:prior|posterior|dict)\w*", name)
            if m:
                rows[name] = {"calls": int(r["Calls"]), "average_ms": float(r["AverageNs"]) * 1e-6, "total_ms": float(r["TotalDurationNs"]) * 1e-6}
    return rows


def med_err(est, truth, names):
    return {k: float(np.median(np.abs(est[i] - truth[i]))) for i, k in enumerate(names)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "grid_prior_probe.json"))
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
    mean, sd, mp = e((5, n), torch.float64), e((5, n), torch.float64), e((5, n), torch.float64)
    atom, lev, ess = e(n, torch.int32), e(n, torch.float64), e(n, torch.float64)
    post = lambda nsd: api.grid_posterior_device(o, n, b, y, atoms, None, lo, hi, False, None, nsd, mean, sd, atom, mp, lev, ess, 0, s)
    em = lambda nsd, k: api.grid_prior_em_device(o, n, b, y, atoms, None, lo, hi, False, None, nsd, k, 0.0, 0.0, 0, s)
    t = {}
    for label, nsd in (("known_noise (noise_sd 0.01)", 0.01), ("marginalised", 0.0)):
        r = {"posterior": timed(torch, dev, lambda: post(nsd))}
        for k in (1, 2, 3):
            r[f"prior_em_n_iter_{k}"] = timed(torch, dev, lambda: em(nsd, k))
        r["one_iteration_ms"] = r["prior_em_n_iter_3"]["median_ms"] - r["prior_em_n_iter_2"]["median_ms"]
        r["iteration_over_posterior"] = r["one_iteration_ms"] / r["posterior"]["median_ms"]
        t[label] = r
    out["time"] = t
    print("time", json.dumps(t), flush=True)
    del y, mean, sd, mp, atom, lev, ess

    if not a.time_only:
        # ---- accuracy against the synthetic truth: the posterior probe's volume, truths uniform over the grid's ranges
        m = 1 << min(16, a.log2_voxels)
        for noise in (0.01, 0.05):
            _, yh, truth = synth.make_numpy("tri_reduced", m, n_b, sigma=noise)
            tr = np.stack([np.asarray(truth[k]) for k in names])
            flat = api.grid_posterior("tri_reduced", b, yh, atoms, lo, hi, noise_sd=noise)
            learned = api.grid_prior_em("tri_reduced", b, yh, atoms, lo, hi, noise_sd=noise, n_iter=30, rel_tol=0.0)
            emp = api.grid_posterior("tri_reduced", b, yh, atoms, lo, hi, noise_sd=noise, log_prior=learned["log_prior"])
            r = {"n_vox": m, "uniform_prior": med_err(flat["mean"], tr, names), "em_prior": med_err(emp["mean"], tr, names),
                 "loglik_first_last": [float(learned["loglik"][0]), float(learned["loglik"][-1])],
                 "atoms_left": int(np.isfinite(learned["log_prior"]).sum()),
                 "prior_entropy_atoms": float(np.exp(-(np.exp(learned["log_prior"]) * np.where(np.isfinite(learned["log_prior"]), learned["log_prior"], 0.0)).sum()))}
            out[f"median_abs_error_noise_{noise}"] = r
            print(f"noise_{noise}", json.dumps(r), flush=True)
        # ---- the narrow population of DESIGN.md 4.1j, where the prior has something to learn -- and too few voxels to learn it from
        sys.path.insert(0, os.path.join(HERE, "tests"))
        from grid_prior_reference import population  # noqa: E402

        pn = ["f1", "D1", "D2"]
        for n_pop in (1000, 37):
            bb, yy, truth, _, at, plo, phi = population(n_pop, seed=0)
            for label, nsd in (("known_noise", 0.05), ("marginalised", 0.0)):
                kw = dict(noise_sd=nsd, project_amplitude=True)
                flat = api.grid_posterior("bi_s0", bb, yy, at, plo, phi, **kw)
                learned = api.grid_prior_em("bi_s0", bb, yy, at, plo, phi, n_iter=30, rel_tol=0.0, **kw)
                emp = api.grid_posterior("bi_s0", bb, yy, at, plo, phi, log_prior=learned["log_prior"], **kw)
                r = {"uniform_prior": med_err(flat["mean"], truth, pn), "em_prior": med_err(emp["mean"], truth, pn)}
                out[f"population_{n_pop}_voxels_noise_0.05_{label}"] = r
                print(f"population_{n_pop}_{label}", json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

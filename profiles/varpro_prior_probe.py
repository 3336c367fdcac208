#!/usr/bin/env python3
"""The empirical-Bayes prior over the variable-projection dictionary (pnx_curvefit_varpro_prior_em_f64), measured
beside the calls it shares its products with.  Device resident, HIP events, two warm-up runs and seven timed runs each, one process.

  time       2^20 tri-S0 voxels x 32 b-values (0 .. 1000) x 969 atoms (ordered triples of 19 rates), the shape of 4.1h / 4.1i /
             4.1l: `varpro`, `varpro_posterior` and `varpro_marginals` as they stand, then the whole EM call at n_iter = 1, 2, 3 with
             rel_tol = 0 (n_iter updates and n_iter + 1 normaliser passes, each with its 16-byte read-back), known and marginalised
             noise.  one_update_ms = call(3) - call(2): a normaliser pass, an accumulate pass, the small kernels and the read-back.
  passes     --kernel-stats FILE: the per-kernel times of a separate run of `--time-only` under a kernel trace (a *kernel_stats.csv),
             merged into the JSON: the normaliser, the accumulate pass and the finish on their own.
  quality    the narrow population of tests/varpro_prior_reference.py (bi_s0, 16 b-values, 91 atoms, 5 % noise) at 1000 and at 37
             voxels, known and marginalised noise; and the 2^16 tri-S0 voxels of profiles/varpro_probe.py at 1 % and 5 % noise --
             truths uniform over ranges inside the dictionary's three decades -- under the uniform prior, under the prior learned in
             30 updates, and the 4^5 grid posterior (S0 projected) beside them.  Median absolute error of the posterior mean.
  resources  --resources-only (no GPU): VGPR / AGPR / scratch / waves per SIMD of every instantiation from the compiler's summary.
python profiles/varpro_prior_probe.py [--out profiles/varpro_prior_probe.json] [--log2-voxels 20] [--time-only] [--resources-only]
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
from varpro_probe import AXES, HI, LO, NAMES, P0, RATES, data, timed  # noqa: E402

from pyneapple_amd import _build, api  # noqa: E402


def kernel_resources():
    src = os.path.join(_build.CSRC, "pnx_varpro_prior.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.HIPCC, *_build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "v.o")]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            t = re.search(r"(varpro_prior_(?:norm|acc)_kernel)ILi(\d+)ELi(\d+)ELi(\d+)E", m.group(2))
            s = re.search(r"(varpro_prior_(?:init|stats|finish)_kernel)", m.group(2))
            name = f"{t.group(1)}<NS={t.group(2)}, K={t.group(3)}, CLS={t.group(4)}>" if t else s.group(1) if s else None
            if name:
                out[name] = {}
        elif name:
            out[name][m.group(1)] = int(m.group(2))
    lds = {f"n_b={n_b}, k={k}": api.varpro_prior_slab_atoms(n_b, k) for n_b in (16, 32, 64, 128) for k in (1, 2, 3)}
    return {"kernels": out, "atoms_per_lds_slab (pnx_varpro_prior_args.hpp varpro_prior_slab)": lds,
            "note": "Occupancy is the register file's; a block holds up to 64 KB of the CU's 160 KB of LDS, so two blocks (two waves per SIMD) is the most that run."}


def kernel_stats(path):
    rows = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Name", "")
            if re.search(r"varpro_\w*", name):
                rows[name] = {"calls": int(r["Calls"]), "average_ms": float(r["AverageNs"]) * 1e-6, "total_ms": float(r["TotalDurationNs"]) * 1e-6}
    return rows


def med_err(est, truth, names):
    return {k: float(np.median(np.abs(est[i] - truth[i]))) for i, k in enumerate(names)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "varpro_prior_probe.json"))
    ap.add_argument("--log2-voxels", type=int, default=20)
    ap.add_argument("--time-only", action="store_true")
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    if a.resources_only or a.kernel_stats:
        out = {}
        if os.path.exists(a.out):
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

    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    e = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)
    nl = np.ascontiguousarray(np.array([t for t in itertools.product(RATES, repeat=3) if t[0] > t[1] > t[2]]).T)
    n_small, n = 1 << min(16, a.log2_voxels), 1 << a.log2_voxels
    o = api.make_opts("tri_s0", 32, jac="analytic")
    n_bins, bin_of, bin_value = api._varpro_marginal_bins(o, "tri_s0", nl, None)
    B = int(n_bins.sum())
    out = {}
    if os.path.exists(a.out) and not a.time_only:
        with open(a.out) as fh:
            out = {k: v for k, v in json.load(fh).items() if k == "resources" or k.startswith("kernel_trace")}
    out.update({"_source_ids": _build.source_ids(), "device": torch.cuda.get_device_name(0), "n_vox": n, "n_b": 32, "n_atoms": int(nl.shape[1]),
                "runs": 7, "warmup": 2})

    # ---- time
    b, y_h, _ = data(n_small, 0.01, 1)
    y = torch.from_numpy(y_h).to(dev).repeat(n // n_small, 1).contiguous()
    p, atom, cost, clp = e((6, n)), e(n, torch.int32), e(n), e(n, torch.int8)
    mean, sd, mp, lev, ess, cm = e((6, n)), e((6, n)), e((6, n)), e(n), e(n), e(n)
    marg, quant, geo = e((B, n)), e((3, 6, n)), e((6, n))
    t = {"varpro": timed(torch, dev, lambda: api.varpro_device(o, n, b, y, nl, None, LO, HI, P0, p, atom, cost, clp, 0, s))}
    for label, nsd in (("known_noise (noise_sd 0.01)", 0.01), ("marginalised", 0.0)):
        r = {"varpro_posterior": timed(torch, dev, lambda: api.varpro_posterior_device(o, n, b, y, nl, None, LO, HI, None, nsd, True, mean, sd, atom,
                                                                                      mp, lev, ess, cm, 0, s)),
             "varpro_marginals": timed(torch, dev, lambda: api.varpro_marginals_device(o, n, b, y, nl, None, LO, HI, None, nsd, True, n_bins, bin_of,
                                                                                      bin_value, (0.025, 0.5, 0.975), marg, quant, geo, lev, 0, s))}
        for k in (1, 2, 3):
            r[f"prior_em_n_iter_{k}"] = timed(torch, dev, lambda: api.varpro_prior_em_device(o, n, b, y, nl, None, LO, HI, None, nsd, True, k, 0.0, 0.0,
                                                                                            0, s))
        r["one_update_ms"] = r["prior_em_n_iter_3"]["median_ms"] - r["prior_em_n_iter_2"]["median_ms"]
        r["update_over_posterior"] = r["one_update_ms"] / r["varpro_posterior"]["median_ms"]
        r["update_over_varpro"] = r["one_update_ms"] / t["varpro"]["median_ms"]
        r["update_over_marginals"] = r["one_update_ms"] / r["varpro_marginals"]["median_ms"]
        t[label] = r
    out["time"] = t
    print("time", json.dumps(t), flush=True)
    del y, p, atom, cost, clp, mean, sd, mp, lev, ess, cm, marg, quant, geo

    if not a.time_only:
        # ---- the narrow population, where the prior has something to learn -- and too few voxels to learn it from
        sys.path.insert(0, os.path.join(HERE, "tests"))
        from varpro_prior_reference import population  # noqa: E402

        pn = ["f1", "D1", "D2"]
        for n_pop in (1000, 37):
            bb, yy, truth, at, plo, phi = population(n_pop, seed=0)
            for label, nsd in (("known_noise", 0.05), ("marginalised", 0.0)):
                flat = api.varpro_posterior("bi_s0", bb, yy, at, plo, phi, noise_sd=nsd)
                learned = api.varpro_prior_em("bi_s0", bb, yy, at, plo, phi, noise_sd=nsd, n_iter=30, rel_tol=0.0)
                emp = api.varpro_posterior("bi_s0", bb, yy, at, plo, phi, noise_sd=nsd, log_prior=learned["log_prior"])
                r = {"uniform_prior": med_err(flat["mean"], truth, pn), "em_prior": med_err(emp["mean"], truth, pn),
                     "atoms_left": int(np.isfinite(learned["log_prior"]).sum())}
                out[f"population_{n_pop}_voxels_noise_0.05_{label}"] = r
                print(f"population_{n_pop}_{label}", json.dumps(r), flush=True)
        # ---- the synthetic volume of 4.1h / 4.1i: truths uniform over ranges the 4^5 grid is a prior on
        atoms = np.ascontiguousarray(np.array(list(itertools.product(*[AXES[k] for k in NAMES]))).T)
        for noise in (0.01, 0.05):
            bq, yq, P = data(n_small, noise, 2)
            flat = api.varpro_posterior("tri_s0", bq, yq, nl, LO, HI)
            learned = api.varpro_prior_em("tri_s0", bq, yq, nl, LO, HI, n_iter=30, rel_tol=0.0)
            emp = api.varpro_posterior("tri_s0", bq, yq, nl, LO, HI, log_prior=learned["log_prior"])
            grid = api.grid_posterior("tri_s0", bq, yq, atoms, LO, HI, project_amplitude=True)
            lp = learned["log_prior"]
            r = {"n_vox": n_small, "varpro_uniform_prior": med_err(flat["mean"], P, NAMES), "varpro_em_prior": med_err(emp["mean"], P, NAMES),
                 "grid_4^5_posterior": med_err(grid["mean"], P, NAMES), "loglik_first_last": [float(learned["loglik"][0]), float(learned["loglik"][-1])],
                 "atoms_left": int(np.isfinite(lp).sum()),
                 "prior_entropy_atoms": float(np.exp(-(np.exp(lp) * np.where(np.isfinite(lp), lp, 0.0)).sum()))}
            out[f"median_abs_error_noise_{noise}"] = r
            print(f"noise_{noise}", json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

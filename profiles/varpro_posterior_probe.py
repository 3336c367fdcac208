#!/usr/bin/env python3
"""The posterior over the variable-projection dictionary (pnx_curvefit_varpro_posterior_f64), measured.  Device resident, HIP
events, two warm-up runs and seven timed runs each, everything in one process; the workloads are profiles/varpro_probe.py's.

  rate       2^20 tri-S0 voxels x 32 b-values (0 .. 1000) x 969 atoms (ordered triples of 19 rates): known and marginalised noise,
             marginal_amplitudes on and off, against pnx_curvefit_varpro_f64 on the same dictionary and
             pnx_curvefit_grid_posterior_f64 at 1024 atoms (4^5 grid) in the same process.
  accuracy   2^16 voxels at 1 % and 5 % additive noise: median absolute error per parameter of the VARPRO posterior mean
             (marginalised noise, marginal amplitudes), of the VARPRO argmin, of the 4^5 grid posterior mean and of p0_grid + TRF;
             median ess and clipped_mass.
  resources  --resources-only (no GPU): VGPR / AGPR / scratch of every kernel of pnx_varpro_posterior.hip from the compiler's summary.
python profiles/varpro_posterior_probe.py [--out profiles/varpro_posterior_probe.json] [--resources-only]"""
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
from varpro_probe import AXES, HI, LO, NAMES, P0, RATES, data, timed  # noqa: E402

from pyneapple_amd import _build, api  # noqa: E402


def kernel_resources():
    src = os.path.join(_build.CSRC, "pnx_varpro_posterior.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.HIPCC, *_build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "v.o")]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            t = re.search(r"varpro_posterior_kernelILi(\d+)ELi(\d+)ELi(\d+)E", m.group(2))
            p = re.search(r"varpro_posterior_prep_kernelILi(\d+)E", m.group(2))
            name = (f"varpro_posterior_kernel<NS={t.group(1)}, K={t.group(2)}, CLS={t.group(3)}>" if t else
                    f"varpro_posterior_prep_kernel<K={p.group(1)}>" if p else m.group(2))
            out[name] = {}
        elif name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "varpro_posterior_probe.json"))
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

    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    e = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)
    nl = np.ascontiguousarray(np.array([t for t in itertools.product(RATES, repeat=3) if t[0] > t[1] > t[2]]).T)
    atoms = np.ascontiguousarray(np.array(list(itertools.product(*[AXES[k] for k in NAMES]))).T)
    n_small, n = 1 << 16, 1 << 20
    out = {"_source_ids": _build.source_ids(), "device": torch.cuda.get_device_name(0), "n_vox_rate": n, "n_vox_accuracy": n_small, "n_b": 32,
           "varpro_atoms": int(nl.shape[1]), "grid_atoms": int(atoms.shape[1]), "runs": 7, "warmup": 2}
    o = api.make_opts("tri_s0", 32, jac="analytic")
    o_pv = api.make_opts("tri_s0", 32, per_voxel=True, max_nfev=250, ftol=1e-8, jac="fd")

    # ---- rate
    b, y_h, _ = data(n_small, 0.01, 1)
    y = torch.from_numpy(y_h).to(dev).repeat(n // n_small, 1).contiguous()
    p, atom, cost, clp = e((6, n)), e(n, torch.int32), e(n), e(n, torch.int8)
    mean, sd, mp, lev, ess, cm = e((6, n)), e((6, n)), e((6, n)), e(n), e(n), e(n)
    vpp = lambda noise_sd, marg: api.varpro_posterior_device(o, n, b, y, nl, None, LO, HI, None, noise_sd, marg, mean, sd, atom, mp, lev, ess, cm, 0, s)
    rate = {"varpro_call": timed(torch, dev, lambda: api.varpro_device(o, n, b, y, nl, None, LO, HI, P0, p, atom, cost, clp, 0, s)),
            "grid_posterior_call": timed(torch, dev, lambda: api.grid_posterior_device(o, n, b, y, atoms, None, LO, HI, True, None, 0.0, mean, sd, atom,
                                                                                       mp, lev, ess, 0, s))}
    for label, noise_sd, marg in (("marginalised_noise, marginal_amplitudes", 0.0, True), ("marginalised_noise, profile", 0.0, False),
                                  ("known_noise, marginal_amplitudes", 0.01, True), ("known_noise, profile", 0.01, False)):
        rate["varpro_posterior_call (" + label + ")"] = timed(torch, dev, lambda: vpp(noise_sd, marg))
    worst = max(v["median_ms"] for k, v in rate.items() if k.startswith("varpro_posterior_call"))
    rate["ratio_posterior_over_varpro (slowest variant)"] = worst / rate["varpro_call"]["median_ms"]
    rate["ratio_posterior_over_grid_posterior (slowest variant)"] = worst / rate["grid_posterior_call"]["median_ms"]
    rate["ratio_posterior_over_grid_posterior_per_atom"] = rate["ratio_posterior_over_grid_posterior (slowest variant)"] * atoms.shape[1] / nl.shape[1]
    out["rate"] = rate
    print("rate", json.dumps(rate), flush=True)
    del y, p, atom, cost, clp, mean, sd, mp, lev, ess, cm

    # ---- accuracy, 2^16 voxels
    m = n_small
    tile = lambda v: torch.from_numpy(np.ascontiguousarray(np.repeat(v[:, None], m, 1))).to(dev)
    lo_t, hi_t = tile(LO), tile(HI)
    mae = lambda est, P: {k: float(np.median(np.abs(est[i] - P[i]))) for i, k in enumerate(NAMES)}
    for noise in (0.01, 0.05):
        b, y_h, P = data(m, noise, 2)
        y = torch.from_numpy(y_h).to(dev)
        r = {}
        mean, sd, ess, cm, atom = e((6, m)), e((6, m)), e(m), e(m), e(m, torch.int32)
        for label, noise_sd, marg in (("varpro_posterior_mean", 0.0, True), ("varpro_posterior_mean (profile weight)", 0.0, False),
                                      ("varpro_posterior_mean (known noise)", noise, True)):
            api.varpro_posterior_device(o, m, b, y, nl, None, LO, HI, None, noise_sd, marg, mean, sd, atom, None, None, ess, cm, 0, s)
            torch.cuda.synchronize(dev)
            r[label] = {"median_abs_error": mae(mean.cpu().numpy(), P), "median_ess": float(np.median(ess.cpu().numpy())),
                        "median_clipped_mass": float(np.median(cm.cpu().numpy())),
                        "median_posterior_sd": {k: float(np.median(sd.cpu().numpy()[i])) for i, k in enumerate(NAMES)}}
        p, cost, clp = e((6, m)), e(m), e(m, torch.int8)
        api.varpro_device(o, m, b, y, nl, None, LO, HI, P0, p, atom, cost, clp, 0, s)
        torch.cuda.synchronize(dev)
        r["varpro"] = {"median_abs_error": mae(p.cpu().numpy(), P)}
        api.grid_posterior_device(o, m, b, y, atoms, None, LO, HI, True, None, 0.0, mean, None, None, None, None, ess, 0, s)
        torch.cuda.synchronize(dev)
        r["grid_posterior_mean"] = {"median_abs_error": mae(mean.cpu().numpy(), P), "median_ess": float(np.median(ess.cpu().numpy()))}
        g0, popt, pcov, st, nf, fc = e((6, m)), e((6, m)), e((m, 6, 6)), e(m, torch.int8), e(m, torch.int32), e(m)
        api.grid_start_device(o, m, b, y, atoms, None, LO, HI, True, g0, atom, cost, 0, s)
        api.curvefit_device(o_pv, m, b, y, g0, lo_t, hi_t, None, popt, pcov, st, nf, fc, 0, s)
        torch.cuda.synchronize(dev)
        r["p0_grid_then_trf"] = {"median_abs_error": mae(popt.cpu().numpy(), P)}
        out[f"noise_{noise}"] = r
        print(f"noise_{noise}", json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The marginals of the variable-projection posterior (pnx_curvefit_varpro_marginals_f64), measured.  Device resident, HIP events,
two warm-up runs and seven timed runs each, everything in one process; the workloads are profiles/varpro_probe.py's.

  rate       2^20 tri-S0 voxels x 32 b-values (0 .. 1000) x 969 atoms (ordered triples of 19 rates, B = 57 bins): known and
             marginalised noise, against pnx_curvefit_varpro_posterior_f64 and pnx_curvefit_varpro_f64 on the same dictionary in the
             same process.  The one-pass design is held against the SUM of those two calls: what a normaliser pass plus a weight
             pass would cost at the least.
  quality    2^16 voxels at 1 % and 5 % additive noise: median absolute error of geo_mean for D1, D2, D3 beside the posterior
             mean's, the median's and p0_grid + TRF's, and the share of voxels whose [0.025, 0.975] interval holds the truth.
  resources  --resources-only (no GPU): VGPR / AGPR / scratch of every kernel of pnx_varpro_marginal.hip from the compiler's summary.
python profiles/varpro_marginal_probe.py [--out profiles/varpro_marginal_probe.json] [--resources-only]"""
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

PROBS = (0.025, 0.5, 0.975)


def kernel_resources():
    src = os.path.join(_build.CSRC, "pnx_varpro_marginal.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.HIPCC, *_build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "v.o")]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            t = re.search(r"varpro_marginal_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", m.group(2))
            name = f"varpro_marginal_kernel<NS={t.group(1)}, K={t.group(2)}, CLS={t.group(3)}, NC={t.group(4)}>" if t else (
                "varpro_marginal_quantile_kernel" if "quantile_kernel" in m.group(2) else m.group(2))
            out[name] = {}
        elif name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "varpro_marginal_probe.json"))
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            out = json.load(fh)
    if a.resources_only:
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
    o = api.make_opts("tri_s0", 32, jac="analytic")
    o_pv = api.make_opts("tri_s0", 32, per_voxel=True, max_nfev=250, ftol=1e-8, jac="fd")
    n_bins, bin_of, bin_value = api._varpro_marginal_bins(o, "tri_s0", nl, None)
    B = int(n_bins.sum())
    out.update({"_source_ids": _build.source_ids(), "device": torch.cuda.get_device_name(0), "n_vox_rate": n, "n_vox_quality": n_small, "n_b": 32,
                "varpro_atoms": int(nl.shape[1]), "bins": B, "runs": 7, "warmup": 2})

    # ---- rate
    b, y_h, _ = data(n_small, 0.01, 1)
    y = torch.from_numpy(y_h).to(dev).repeat(n // n_small, 1).contiguous()
    p, atom, cost, clp = e((6, n)), e(n, torch.int32), e(n), e(n, torch.int8)
    mean, sd, mp, lev, ess, cm = e((6, n)), e((6, n)), e((6, n)), e(n), e(n), e(n)
    marg, quant, geo = e((B, n)), e((3, 6, n)), e((6, n))
    rate = {"varpro_call": timed(torch, dev, lambda: api.varpro_device(o, n, b, y, nl, None, LO, HI, P0, p, atom, cost, clp, 0, s))}
    for label, noise_sd in (("marginalised_noise", 0.0), ("known_noise", 0.01)):
        post = timed(torch, dev, lambda: api.varpro_posterior_device(o, n, b, y, nl, None, LO, HI, None, noise_sd, True, mean, sd, atom, mp, lev, ess,
                                                                    cm, 0, s))
        mg = timed(torch, dev, lambda: api.varpro_marginals_device(o, n, b, y, nl, None, LO, HI, None, noise_sd, True, n_bins, bin_of, bin_value,
                                                                   PROBS, marg, quant, geo, lev, 0, s))
        only = timed(torch, dev, lambda: api.varpro_marginals_device(o, n, b, y, nl, None, LO, HI, None, noise_sd, True, n_bins, bin_of, bin_value,
                                                                     (), marg, None, None, None, 0, s))
        two_pass_floor = post["median_ms"] + rate["varpro_call"]["median_ms"]
        rate[label] = {"varpro_posterior_call": post, "varpro_marginals_call": mg, "varpro_marginals_call (marginal only, no second kernel)": only,
                       "posterior_plus_varpro_ms (the least a two-pass design costs)": two_pass_floor,
                       "ratio_marginals_over_two_pass_floor": mg["median_ms"] / two_pass_floor,
                       "ratio_marginals_over_posterior": mg["median_ms"] / post["median_ms"]}
    out["rate"] = rate
    print("rate", json.dumps(rate), flush=True)
    del y, p, atom, cost, clp, mean, sd, mp, lev, ess, cm, marg, quant, geo

    # ---- estimator quality, 2^16 voxels
    m = n_small
    rows = [(k, NAMES[k]) for k in range(6) if n_bins[k]]
    tile = lambda v: torch.from_numpy(np.ascontiguousarray(np.repeat(v[:, None], m, 1))).to(dev)
    lo_t, hi_t = tile(LO), tile(HI)
    med = lambda est, truth: float(np.median(np.abs(est - truth)))
    for noise in (0.01, 0.05):
        b, y_h, P = data(m, noise, 2)
        y = torch.from_numpy(y_h).to(dev)
        mean, sd, ess, cm, atom = e((6, m)), e((6, m)), e(m), e(m), e(m, torch.int32)
        marg, quant, geo, lev = e((B, m)), e((3, 6, m)), e((6, m)), e(m)
        api.varpro_posterior_device(o, m, b, y, nl, None, LO, HI, None, 0.0, True, mean, sd, atom, None, None, ess, cm, 0, s)
        api.varpro_marginals_device(o, m, b, y, nl, None, LO, HI, None, 0.0, True, n_bins, bin_of, bin_value, PROBS, marg, quant, geo, lev, 0, s)
        g0, popt, pcov, st, nf, fc, cost = e((6, m)), e((6, m)), e((m, 6, 6)), e(m, torch.int8), e(m, torch.int32), e(m), e(m)
        api.grid_start_device(o, m, b, y, atoms, None, LO, HI, True, g0, atom, cost, 0, s)
        api.curvefit_device(o_pv, m, b, y, g0, lo_t, hi_t, None, popt, pcov, st, nf, fc, 0, s)
        torch.cuda.synchronize(dev)
        mean_h, geo_h, q_h, trf_h = mean.cpu().numpy(), geo.cpu().numpy(), quant.cpu().numpy(), popt.cpu().numpy()
        r = {"median_ess": float(np.median(ess.cpu().numpy()))}
        for k, name in rows:
            inside = (q_h[0, k] <= P[k]) & (P[k] <= q_h[2, k])
            r[name] = {"median_abs_error": {"geo_mean": med(geo_h[k], P[k]), "posterior_mean": med(mean_h[k], P[k]),
                                            "posterior_median": med(q_h[1, k], P[k]), "p0_grid_then_trf": med(trf_h[k], P[k])},
                       "interval_0.025_0.975_holds_truth": float(inside.mean()),
                       "median_interval_width_over_truth": float(np.median((q_h[2, k] - q_h[0, k]) / P[k]))}
        out[f"noise_{noise}"] = r
        print(f"noise_{noise}", json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

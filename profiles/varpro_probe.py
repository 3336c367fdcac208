#!/usr/bin/env python3
"""The variable-projection dictionary fit (pnx_curvefit_varpro_f64), measured.  Device resident, HIP events, two warm-up runs and
seven timed runs each, everything in one process.

  rate       2^20 tri-S0 voxels x 32 b-values (0 .. 1000) x 969 atoms (ordered triples of 19 rates) against
             pnx_curvefit_grid_start_f64 (projected amplitude) and pnx_curvefit_grid_posterior_f64 at 1024 atoms (4^5 grid).
  accuracy   2^16 voxels at 1 % and 5 % additive noise: median absolute error per parameter of the VARPRO estimate, the posterior
             mean, the peel, and p0_grid + TRF.
  the fit    nfev and time of the TRF fit from the shared p0 and from the VARPRO start on the same 2^16 voxels.
  resources  --resources-only (no GPU): VGPR / AGPR / scratch of every kernel of pnx_varpro.hip from the compiler's summary.
python profiles/varpro_probe.py [--out profiles/varpro_probe.json] [--resources-only]"""
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

NAMES = api.MODEL_PARAM_NAMES["tri_s0"]
TRUTH = {"f1": (0.1, 0.3), "D1": (0.03, 0.1), "f2": (0.2, 0.4), "D2": (3e-3, 8e-3), "D3": (5e-4, 1.5e-3), "S0": (0.8, 1.2)}
P0 = np.array([0.2, 0.05, 0.3, 0.005, 0.001, 1.0])
LO = np.array([0.0, 1e-5, 0.0, 1e-5, 1e-5, 0.0])
HI = np.array([1.0, 0.5, 1.0, 0.5, 0.5, 10.0])
RATES = np.geomspace(3e-4, 0.3, 19)
AXES = {"f1": np.linspace(0.1, 0.3, 4), "D1": np.geomspace(0.03, 0.1, 4), "f2": np.linspace(0.2, 0.4, 4),
        "D2": np.geomspace(3e-3, 8e-3, 4), "D3": np.geomspace(5e-4, 1.5e-3, 4), "S0": np.array([1.0])}


def kernel_resources():
    src = os.path.join(_build.CSRC, "pnx_varpro.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.HIPCC, *_build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "v.o")]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            t = re.search(r"varpro_match_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", m.group(2))
            name = f"varpro_match_kernel<NS={t.group(1)}, MS={t.group(2)}, K={t.group(3)}, CLS={t.group(4)}>" if t else m.group(2)
            out[name] = {}
        elif name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def data(n, noise, seed):
    rng = np.random.default_rng(seed)
    b = np.linspace(0.0, 1000.0, 32)
    P = np.stack([rng.uniform(*TRUTH[k], n) for k in NAMES])
    e = lambda D: np.exp(-b[None, :] * D[:, None])
    y = P[5][:, None] * (P[0][:, None] * e(P[1]) + P[2][:, None] * e(P[3]) + (1 - P[0] - P[2])[:, None] * e(P[4]))
    return b, y + noise * rng.standard_normal(y.shape), P


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
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "varpro_probe.json"))
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

    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    e = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)
    nl = np.ascontiguousarray(np.array([t for t in itertools.product(RATES, repeat=3) if t[0] > t[1] > t[2]]).T)
    atoms = np.ascontiguousarray(np.array(list(itertools.product(*[AXES[k] for k in NAMES]))).T)
    n_small, n = 1 << 16, 1 << 20
    out = {"_source_ids": _build.source_ids(), "device": torch.cuda.get_device_name(0), "n_vox_rate": n, "n_vox_accuracy": n_small, "n_b": 32,
           "varpro_atoms": int(nl.shape[1]), "grid_atoms": int(atoms.shape[1]), "runs": 7, "warmup": 2}
    o = api.make_opts("tri_s0", 32, jac="analytic")
    o_sh = api.make_opts("tri_s0", 32, max_nfev=250, ftol=1e-8, jac="fd")
    o_pv = api.make_opts("tri_s0", 32, per_voxel=True, max_nfev=250, ftol=1e-8, jac="fd")

    # ---- rate
    b, y_h, _ = data(n_small, 0.01, 1)
    y = torch.from_numpy(y_h).to(dev).repeat(n // n_small, 1).contiguous()
    p, atom, cost, clp = e((6, n)), e(n, torch.int32), e(n), e(n, torch.int8)
    mean, sd, mp, lev, ess = e((6, n)), e((6, n)), e((6, n)), e(n), e(n)
    vp = lambda nv=n: api.varpro_device(o, nv, b, y, nl, None, LO, HI, P0, p, atom, cost, clp, 0, s)
    gs = lambda: api.grid_start_device(o, n, b, y, atoms, None, LO, HI, True, p, atom, cost, 0, s)
    post = lambda: api.grid_posterior_device(o, n, b, y, atoms, None, LO, HI, True, None, 0.0, mean, sd, atom, mp, lev, ess, 0, s)
    rate = {"varpro_call": timed(torch, dev, vp), "varpro_dictionary_only (16 voxels)": timed(torch, dev, lambda: vp(16)),
            "grid_start_call": timed(torch, dev, gs), "grid_posterior_call": timed(torch, dev, post)}
    rate["ratio_varpro_over_grid_start"] = rate["varpro_call"]["median_ms"] / rate["grid_start_call"]["median_ms"]
    rate["ratio_varpro_over_grid_start_per_atom"] = rate["ratio_varpro_over_grid_start"] * atoms.shape[1] / nl.shape[1]
    rate["ratio_varpro_over_grid_posterior"] = rate["varpro_call"]["median_ms"] / rate["grid_posterior_call"]["median_ms"]
    out["rate"] = rate
    print("rate", json.dumps(rate), flush=True)
    del y, p, atom, cost, clp, mean, sd, mp, lev, ess

    # ---- accuracy and the fit, 2^16 voxels
    m = n_small
    tile = lambda v: torch.from_numpy(np.ascontiguousarray(np.repeat(v[:, None], m, 1))).to(dev)
    lo_t, hi_t = tile(LO), tile(HI)
    mae = lambda est, P: {k: float(np.median(np.abs(est[i] - P[i]))) for i, k in enumerate(NAMES)}
    for noise in (0.01, 0.05):
        b, y_h, P = data(m, noise, 2)
        y = torch.from_numpy(y_h).to(dev)
        p, atom, cost, clp = e((6, m)), e(m, torch.int32), e(m), e(m, torch.int8)
        popt, pcov, st, nf, fc = e((6, m)), e((m, 6, 6)), e(m, torch.int8), e(m, torch.int32), e(m)
        r = {}
        api.varpro_device(o, m, b, y, nl, None, LO, HI, P0, p, atom, cost, clp, 0, s)
        torch.cuda.synchronize(dev)
        r["varpro"] = {"median_abs_error": mae(p.cpu().numpy(), P), "clipped_share": float(clp.cpu().numpy().mean())}
        fit_vp = lambda: api.curvefit_device(o_pv, m, b, y, p, lo_t, hi_t, None, popt, pcov, st, nf, fc, 0, s)
        r["varpro_then_trf"] = {"fit": timed(torch, dev, fit_vp)}
        r["varpro_then_trf"].update(median_abs_error=mae(popt.cpu().numpy(), P), nfev_mean=float(nf.cpu().numpy().mean()),
                                    nfev_p999=float(np.percentile(nf.cpu().numpy(), 99.9)), failed_share=float((st.cpu().numpy() <= 0).mean()))
        c_vp = fc.cpu().numpy().copy()
        fit_sh = lambda: api.curvefit_device(o_sh, m, b, y, P0, LO, HI, None, popt, pcov, st, nf, fc, 0, s)
        r["shared_p0_trf"] = {"fit": timed(torch, dev, fit_sh)}
        r["shared_p0_trf"].update(median_abs_error=mae(popt.cpu().numpy(), P), nfev_mean=float(nf.cpu().numpy().mean()),
                                  nfev_p999=float(np.percentile(nf.cpu().numpy(), 99.9)), failed_share=float((st.cpu().numpy() <= 0).mean()))
        rel = (c_vp - fc.cpu().numpy()) / np.maximum(fc.cpu().numpy(), 1e-300)
        r["final_cost_varpro_start_vs_shared"] = {"lower": float((rel < -1e-9).mean()), "equal_1e-9": float((np.abs(rel) <= 1e-9).mean()),
                                                  "higher": float((rel > 1e-9).mean())}
        g0 = e((6, m))
        api.grid_start_device(o, m, b, y, atoms, None, LO, HI, True, g0, atom, cost, 0, s)
        api.curvefit_device(o_pv, m, b, y, g0, lo_t, hi_t, None, popt, pcov, st, nf, fc, 0, s)
        torch.cuda.synchronize(dev)
        r["p0_grid_then_trf"] = {"median_abs_error": mae(popt.cpu().numpy(), P), "nfev_mean": float(nf.cpu().numpy().mean())}
        mean = e((6, m))
        api.grid_posterior_device(o, m, b, y, atoms, None, LO, HI, True, None, 0.0, mean, None, None, None, None, None, 0, s)
        torch.cuda.synchronize(dev)
        r["posterior_mean"] = {"median_abs_error": mae(mean.cpu().numpy(), P)}
        pe = api.peel(b, y_h, "tri_s0", b_thresholds=[60.0, 350.0], clip=(LO, HI), fallback=P0)
        r["peel"] = {"median_abs_error": mae(pe["params"], P), "failed_share": float((pe["status"] <= 0).mean())}
        out[f"noise_{noise}"] = r
        print(f"noise_{noise}", json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The dictionary search for per-voxel start values (pnx_curvefit_grid_start_f64), measured: its rate against the repository's
other fp64 MFMA product, and what it buys the fit.  Device resident, HIP events, two warm-up runs and seven timed runs each.

  kernel rate   2^20 C3 voxels (tri-exponential reduced, 32 b-values, 1 % noise), 1024 atoms: the whole call (dictionary + match)
                and the dictionary alone (the same call on 16 voxels); flops = 2 n_vox n_b_padded n_atoms.  Yardstick:
                pnx_nnls_aty_f64 in the same process on the same y (2 n_vox 32 x 250 flops, 2 KB written per voxel).
  the fit       the same volume at 1 % and 5 % noise: shared p0 against search + fit from per-voxel p0 with the bounds tiled --
                nfev (mean, 99.9th percentile, at the limit), the fit's time alone, the total with the search, and the share of
                voxels whose final cost is lower / equal within 1e-9 relative / higher.
  resources     --resources-only (no GPU): VGPR / AGPR / LDS / scratch of the match kernels from the compiler's summary for gfx950,
                merged into the JSON.
python profiles/grid_start_probe.py [--out profiles/grid_start_probe.json] [--log2-voxels 20] [--resources-only]"""
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
from pyneapple_amd import _build, api, synth  # noqa: E402

# 4^5 = 1024 atoms over the ranges the benchmark's truth is drawn from (synth.TRUTH), geometric in the diffusivities
AXES = {"f1": np.linspace(0.1, 0.3, 4), "D1": np.geomspace(0.03, 0.1, 4), "f2": np.linspace(0.2, 0.4, 4),
        "D2": np.geomspace(3e-3, 8e-3, 4), "D3": np.geomspace(5e-4, 1.5e-3, 4)}


NOTES = ("grid_TFLOPs_match subtracts the dictionary-only call (atoms upload, forward model, transposition: launch-bound"
         ") from the whole call. Per flop the whole call is slower than pnx_nnls_aty_f64 when ratio_grid_call_over_aty <"
         " 1 (0.94 on the recorded run; the match alone is level): the dictionary costs 0.18 ms of the 2.2, and the matc"
         "h kernel takes 173-238 VGPRs, one block of eight waves per CU, with the argmin fold issuing between the MFMAs "
         "-- reasons read from the code and the compiler's summary, not confirmed with counters. The fit from per-voxel "
         "start values runs the per-voxel instantiation of the fit kernel (p0 and both bounds read per voxel), so its ti"
         "me differs from the shared-p0 kernel's by more than the evaluation count.")


def slab_lds_bytes(n_b):
    """grid_slab of csrc/pnx_grid_args.hpp: [kpad][stride] doubles plus two per atom of the slab."""
    kpad = (n_b + 3) & ~3
    stride = lambda w: w if w & 16 else w + 16
    w = max(w for w in range(16, 257, 16) if kpad * stride(w) + 2 * w <= 8192)
    return 8 * (kpad * stride(w) + 2 * w)


def kernel_resources():
    src = os.path.join(_build.CSRC, "pnx_grid.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.HIPCC, *_build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "g.o")]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            t = re.search(r"grid_match_kernelILi(\d+)ELi(\d+)ELb([01])E", m.group(2))
            name = f"grid_match_kernel<NS={t.group(1)}, MS={t.group(2)}, PROJ={t.group(3)}>" if t else None
            if name:
                out[name] = {}
        elif name:
            out[name][m.group(1)] = int(m.group(2))
    from_host = {f"n_b={n_b}": slab_lds_bytes(n_b) for n_b in (16, 32, 64, 128)}
    return {"kernels": out, "dynamic_lds_bytes (pnx_grid_args.hpp grid_slab)": from_host}


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
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "grid_start_probe.json"))
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
    o_grid = api.make_opts("tri_reduced", n_b, jac="analytic")
    p0v, best, gcost = e((5, n), torch.float64), e(n, torch.int32), e(n, torch.float64)
    lo_t = torch.from_numpy(np.ascontiguousarray(np.repeat(lo[:, None], n, 1))).to(dev)
    hi_t = torch.from_numpy(np.ascontiguousarray(np.repeat(hi[:, None], n, 1))).to(dev)

    # ---- kernel rate
    y = synth.make_torch_rows("tri_reduced", 0, n, n_b, dev, sigma=0.01)[1]
    search = lambda nv=n: api.grid_start_device(o_grid, nv, b, y, atoms, None, lo, hi, False, p0v, best, gcost, 0, s)
    t_call, t_dict = timed(torch, dev, search), timed(torch, dev, lambda: search(16))
    _, basis, reg = synth.nnls_matrices(n_b)
    plan = api.NnlsPlan(basis, reg, 0)
    aty = e((n, 256), torch.float64)
    t_aty = timed(torch, dev, lambda: plan.aty_device(n, y, aty, s))
    plan.close()
    del aty
    fl_grid, fl_aty = 2.0 * n * ((n_b + 3) & ~3) * n_atoms, 2.0 * n * n_b * basis.shape[1]
    match_ms = t_call["median_ms"] - t_dict["median_ms"]
    rate = {"grid_call": t_call, "grid_dictionary_only (16 voxels)": t_dict, "aty": t_aty, "grid_flops": fl_grid, "aty_flops": fl_aty,
            "grid_TFLOPs_call": fl_grid / t_call["median_ms"] / 1e9, "grid_TFLOPs_match": fl_grid / match_ms / 1e9,
            "aty_TFLOPs": fl_aty / t_aty["median_ms"] / 1e9}
    rate["ratio_grid_call_over_aty"] = rate["grid_TFLOPs_call"] / rate["aty_TFLOPs"]
    out["kernel_rate"] = rate
    print("kernel_rate", json.dumps(rate), flush=True)

    # ---- what it buys the fit
    popt, pcov, st, nf, cost = e((5, n), torch.float64), e((n, 5, 5), torch.float64), e(n, torch.int8), e(n, torch.int32), e(n, torch.float64)
    o_sh = api.make_opts("tri_reduced", n_b, max_nfev=250, ftol=1e-8, jac="fd")
    o_pv = api.make_opts("tri_reduced", n_b, per_voxel=True, max_nfev=250, ftol=1e-8, jac="fd")
    for noise in (0.01, 0.05):
        y = synth.make_torch_rows("tri_reduced", 0, n, n_b, dev, sigma=noise)[1]
        search = lambda: api.grid_start_device(o_grid, n, b, y, atoms, None, lo, hi, False, p0v, best, gcost, 0, s)
        fit_sh = lambda: api.curvefit_device(o_sh, n, b, y, p0, lo, hi, None, popt, pcov, st, nf, cost, 0, s)
        fit_pv = lambda: api.curvefit_device(o_pv, n, b, y, p0v, lo_t, hi_t, None, popt, pcov, st, nf, cost, 0, s)
        r = {}
        r["shared_p0"] = {"fit": timed(torch, dev, fit_sh)}
        nf_sh, c_sh, st_sh = nf.cpu().numpy().copy(), cost.cpu().numpy().copy(), st.cpu().numpy().copy()
        r["grid_start"] = {"search": timed(torch, dev, search), "fit": timed(torch, dev, fit_pv),
                           "search_and_fit": timed(torch, dev, lambda: (search(), fit_pv()))}
        nf_g, c_g, st_g = nf.cpu().numpy(), cost.cpu().numpy(), st.cpu().numpy()
        for key, nfv, stv in (("shared_p0", nf_sh, st_sh), ("grid_start", nf_g, st_g)):
            r[key].update(nfev_mean=float(nfv.mean()), nfev_p999=float(np.percentile(nfv, 99.9)), nfev_max=int(nfv.max()),
                          at_limit_share=float((stv == 0).mean()), failed_share=float((stv <= 0).mean()))
        both = (st_sh > 0) & (st_g > 0)
        rel = (c_g[both] - c_sh[both]) / np.maximum(c_sh[both], 1e-300)
        r["final_cost_grid_vs_shared"] = {"lower": float((rel < -1e-9).mean()), "equal_1e-9": float((np.abs(rel) <= 1e-9).mean()),
                                          "higher": float((rel > 1e-9).mean()), "compared_share": float(both.mean())}
        out[f"noise_{noise}"] = r
        print(f"noise_{noise}", json.dumps(r), flush=True)
    out["notes"] = NOTES
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The edge-preserving (Student-t) neighbourhood prior of the grid posterior (pnx_curvefit_grid_posterior_tmrf_f64 and its two
parts), measured beside the Gaussian prior's calls in the same process.  Device resident, HIP events, two warm-up
runs and seven timed runs each.

  time       2^20 tri-exponential reduced voxels, 32 b-values, 1 % noise, 1024 atoms, known and marginalised noise; a 1024 x 1024
             slice sorted by colour, 4-neighbourhood, 2 colours (the workload of profiles/grid_mrf_probe.py).  The Gaussian gather
             and the weighted one; the Gaussian field posterior and the weighted one; both drivers at 0 and at 4 sweeps, one sweep
             as the difference.  The Gaussian calls are timed before and after the weighted ones: their difference is the drift.
  phantom    tests/grid_mrf_reference.phantom on the device at 5 % and 2 % noise, strength 16 and 64, dof infinity (the Gaussian
             driver), 4 and 1, 6 sweeps, seed 0: the ratio of the median |error| of f1 / D1 / D2 to the plain posterior's over all
             voxels, the 92 voxels with a neighbour in the other region, and the others -- with tests/grid_tmrf_reference.py's
             figures beside them.
  resources  --resources-only (no GPU): VGPR / AGPR / scratch / waves per SIMD of every kernel of pnx_grid_tmrf.hip from the
             compiler's summary for gfx950, merged into the JSON.
python profiles/grid_tmrf_probe.py [--out profiles/grid_tmrf_probe.json] [--log2-side 10] [--resources-only] [--no-time]"""
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
from grid_start_probe import AXES, timed  # noqa: E402  the same 4^5 atoms and the same timing loop

from pyneapple_amd import _build, api, synth  # noqa: E402


def kernel_resources():
    src = os.path.join(_build.CSRC, "pnx_grid_tmrf.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.HIPCC, *_build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "g.o")]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            p = re.search(r"(grid_mrf_posterior_kernel)ILi(\d+)ELi(\d+)ELb([01])ELb([01])E", m.group(2))
            s = re.search(r"(grid_tmrf_gather_kernel)", m.group(2))
            name = f"{p.group(1)}<NS={p.group(2)}, NF={p.group(3)}, PROJ={p.group(4)}, WREAL={p.group(5)}>" if p else s.group(1) if s else None
            if name:
                out[name] = {}
        elif name:
            out[name][m.group(1)] = int(m.group(2))
    return {"kernels": out, "any_scratch": any(k.get("ScratchSize [bytes/lane]", 0) for k in out.values())}


def phantom_ratios():
    import grid_mrf_reference as R
    import grid_tmrf_reference as T

    res = {}
    for noise in (0.05, 0.02):
        ph = R.phantom(seed=0, noise=noise)
        order, nb, start = R.colour_sort(ph["nb"], ph["colours"])
        y, truth = ph["y"][order], ph["truth"][order]
        region = truth[:, 0] == 0.30
        edge = ((nb >= 0) & (region[np.maximum(nb, 0)] != region[:, None])).any(axis=1)
        rng = ph["atoms"].max(axis=1) - ph["atoms"].min(axis=1)
        sets = {"all": np.ones(edge.size, bool), "edge": edge, "other": ~edge}
        err = lambda mean: {k: np.median(np.abs(mean[s] - truth[s]), axis=0) for k, s in sets.items()}
        args = ("bi_reduced", ph["b"], y, ph["atoms"], ph["lo"], ph["hi"], nb, start)
        plain = err(api.grid_posterior_mrf(*args, np.zeros(3), n_sweeps=0, noise_sd=noise)["mean"].T)
        r = {"n_edge_voxels": int(edge.sum()), "plain_median_abs_error (f1, D1, D2)": {k: v.tolist() for k, v in plain.items()}}
        for strength in (16.0, 64.0):
            lam = strength / rng ** 2
            for dof in (None, 4.0, 1.0):
                if dof is None:
                    got = api.grid_posterior_mrf(*args, lam, n_sweeps=6, noise_sd=noise)
                    ref = R.mrf(*args, lam, 6, noise_sd=noise)[0]
                else:
                    got = api.grid_posterior_tmrf(*args, lam, dof, n_sweeps=6, noise_sd=noise)
                    ref = T.tmrf(*args, lam, dof, 6, noise_sd=noise)[0]
                e_dev, e_ref = err(got["mean"].T), err(ref["mean"])
                r[f"strength_{strength:g}_dof_{'inf' if dof is None else format(dof, 'g')}"] = {
                    "device_ratio_to_plain": {k: (e_dev[k] / plain[k]).tolist() for k in sets},
                    "reference_ratio_to_plain": {k: (e_ref[k] / plain[k]).tolist() for k in sets}, "delta": got["delta"].tolist()}
        res[f"noise_{noise:g}"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "grid_tmrf_probe.json"))
    ap.add_argument("--log2-side", type=int, default=10)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--no-time", action="store_true")
    a = ap.parse_args()
    old = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            old = json.load(fh)
    if a.resources_only:
        old["resources"] = kernel_resources()
        with open(a.out, "w") as fh:
            json.dump(old, fh, indent=1)
            fh.write("\n")
        return
    import torch

    side, n_b, dof = 1 << a.log2_side, 32, 4.0
    n = side * side
    dev = torch.device("cuda", 0)
    names, p0, lo, hi = synth.shared_arrays("tri_reduced")
    atoms = np.ascontiguousarray(np.array(list(itertools.product(*[AXES[k] for k in names]))).T)
    b = synth.bvalues(n_b)
    s = torch.cuda.current_stream(dev).cuda_stream
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    out = {"_source_ids": _build.source_ids(), "device": torch.cuda.get_device_name(0), "n_vox": n, "n_b": n_b, "n_atoms": atoms.shape[1],
           "n_nb": 4, "n_colours": 2, "dof": dof, "runs": 7, "warmup": 2}
    if not a.no_time:
        y = synth.make_torch_rows("tri_reduced", 0, n, n_b, dev, sigma=0.01)[1]
        res = {k: e((5, n), torch.float64) for k in ("mean", "sd", "map_p")}
        res.update(map_atom=e(n, torch.int32), log_evidence=e(n, torch.float64), ess=e(n, torch.float64), field_w=e(n, torch.float64),
                   field_n=e(n, torch.int32))
        nb, col = api.grid_neighbours(np.ones((side, side), bool), 4)
        order = np.argsort(col, kind="stable")
        place = np.empty(n, np.int64)
        place[order] = np.arange(n)
        nb = torch.from_numpy(np.where(nb[order] >= 0, place[np.maximum(nb[order], 0)], -1).astype(np.int32)).to(dev)
        start = np.concatenate([[0], np.cumsum(np.bincount(col))]).astype(np.int64)
        pr = 16.0 / (atoms.max(axis=1) - atoms.min(axis=1)) ** 2
        centre = api.grid_mrf_centre(atoms)
        fld = dict(field_q=e((5, n), torch.float64), field_n=e(n, torch.int32), field_w=e(n, torch.float64))
        t = {}
        for label, nsd in (("known_noise (noise_sd 0.01)", 0.01), ("marginalised", 0.0)):
            mrf = lambda k: api.grid_posterior_mrf("tri_reduced", b, y, atoms, lo, hi, nb, start, pr, n_sweeps=k, noise_sd=nsd, out=res, stream=s)
            tmrf = lambda k: api.grid_posterior_tmrf("tri_reduced", b, y, atoms, lo, hi, nb, start, pr, dof, n_sweeps=k, noise_sd=nsd, out=res,
                                                     stream=s)
            gather = lambda: api.grid_neighbour_field(nb, res["mean"], centre, pr, out=fld, stream=s)
            wgather = lambda: api.grid_neighbour_wfield(nb, res["mean"], res["sd"], centre, pr, dof, out=fld, stream=s)
            field = lambda: api.grid_posterior_field("tri_reduced", b, y, atoms, lo, hi, fld["field_q"], fld["field_n"], pr, res, noise_sd=nsd,
                                                     stream=s)
            wfield = lambda: api.grid_posterior_wfield("tri_reduced", b, y, atoms, lo, hi, fld["field_q"], fld["field_w"], pr, res, noise_sd=nsd,
                                                       stream=s)
            mrf(0)
            wgather()
            r = {"gaussian_gather": timed(torch, dev, gather), "weighted_gather": timed(torch, dev, wgather),
                 "gaussian_gather_again": timed(torch, dev, gather)}
            r["gaussian_field_posterior"] = timed(torch, dev, field)
            r["weighted_field_posterior"] = timed(torch, dev, wfield)
            r["gaussian_field_posterior_again"] = timed(torch, dev, field)
            r["gaussian_driver_0_sweeps"], r["gaussian_driver_4_sweeps"] = timed(torch, dev, lambda: mrf(0)), timed(torch, dev, lambda: mrf(4))
            r["weighted_driver_0_sweeps"], r["weighted_driver_4_sweeps"] = timed(torch, dev, lambda: tmrf(0)), timed(torch, dev, lambda: tmrf(4))
            r["gaussian_one_sweep_ms"] = (r["gaussian_driver_4_sweeps"]["median_ms"] - r["gaussian_driver_0_sweeps"]["median_ms"]) / 4
            r["weighted_one_sweep_ms"] = (r["weighted_driver_4_sweeps"]["median_ms"] - r["weighted_driver_0_sweeps"]["median_ms"]) / 4
            r["weighted_gather_over_gaussian"] = r["weighted_gather"]["median_ms"] / r["gaussian_gather"]["median_ms"]
            r["weighted_field_over_gaussian"] = r["weighted_field_posterior"]["median_ms"] / r["gaussian_field_posterior"]["median_ms"]
            r["weighted_sweep_over_gaussian"] = r["weighted_one_sweep_ms"] / r["gaussian_one_sweep_ms"]
            print(label, json.dumps(r), flush=True)
            t[label] = r
        out["time"] = t
    elif "time" in old:
        out["time"] = old["time"]
    out["phantom"] = phantom_ratios()
    print(json.dumps(out["phantom"]), flush=True)
    out["resources"] = old.get("resources")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

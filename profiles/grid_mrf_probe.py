#!/usr/bin/env python3
"""The neighbourhood (MRF) prior of the grid posterior (pnx_curvefit_grid_posterior_mrf_f64 and its two parts), measured beside the
plain posterior in the same process.  Device resident, HIP events, two warm-up runs and seven timed runs each.

  time       2^20 tri-exponential reduced voxels, 32 b-values, 1 % noise, 1024 atoms (the shape of DESIGN.md 4.1g), known and
             marginalised noise; the voxels are a 1024 x 1024 slice sorted by colour, 4-neighbourhood, 2 colours.  The plain
             posterior; the driver at 0 and at 4 sweeps (tol = 0: no host round trip per sweep; the call synchronises at its end,
             the events are recorded around it); one field posterior over all voxels; one gather over all voxels.  The
             expectation, not a gate: one sweep = one posterior call + a bandwidth-bound gather.
  phantom    tests/grid_mrf_reference.phantom (24 x 24, two regions, 16 b-values, 8^3 atoms) on the device: medians of |error| of
             the plain posterior and of the MRF at strength 4 and 64, 6 sweeps, at 5 % and 2 % noise, seed 0.
  resources  --resources-only (no GPU): VGPR / AGPR / scratch / waves per SIMD of every kernel of pnx_grid_mrf.hip from the
             compiler's summary for gfx950, and the atoms per LDS slab, merged into the JSON.
python profiles/grid_mrf_probe.py [--out profiles/grid_mrf_probe.json] [--log2-side 10] [--resources-only]"""
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
    src = os.path.join(_build.CSRC, "pnx_grid_mrf.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.HIPCC, *_build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "g.o")]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            p = re.search(r"(grid_mrf_posterior_kernel)ILi(\d+)ELi(\d+)ELb([01])E", m.group(2))
            s = re.search(r"(grid_mrf_(?:gather|colour_check|delta|flags)_kernel)", m.group(2))
            name = f"{p.group(1)}<NS={p.group(2)}, NF={p.group(3)}, PROJ={p.group(4)}>" if p else s.group(1) if s else None
            if name:
                out[name] = {}
        elif name:
            out[name][m.group(1)] = int(m.group(2))
    lds = {f"n_b={n_b}, n_free={k}": api.grid_mrf_slab_atoms(n_b, k) for n_b in (16, 32, 128) for k in (3, 5, 8)}
    return {"kernels": out, "atoms_per_lds_slab (pnx_grid_mrf_args.hpp grid_mrf_slab)": lds}


def phantom_ratios():
    import grid_mrf_reference as R

    res = {}
    for noise in (0.05, 0.02):
        ph = R.phantom(seed=0, noise=noise)
        order, nb, start = R.colour_sort(ph["nb"], ph["colours"])
        y, truth = ph["y"][order], ph["truth"][order]
        rng = ph["atoms"].max(axis=1) - ph["atoms"].min(axis=1)
        err = lambda r: np.median(np.abs(r["mean"].T - truth), axis=0)
        args = ("bi_reduced", ph["b"], y, ph["atoms"], ph["lo"], ph["hi"], nb, start)
        plain = err(api.grid_posterior_mrf(*args, np.zeros(3), n_sweeps=0, noise_sd=noise))
        r = {"plain_median_abs_error (f1, D1, D2)": plain.tolist()}
        for strength in (4.0, 64.0):
            got = api.grid_posterior_mrf(*args, strength / rng ** 2, n_sweeps=6, noise_sd=noise)
            r[f"strength_{strength:g}"] = {"median_abs_error": err(got).tolist(), "ratio_to_plain": (err(got) / plain).tolist(),
                                           "delta": got["delta"].tolist()}
        res[f"noise_{noise:g}"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "grid_mrf_probe.json"))
    ap.add_argument("--log2-side", type=int, default=10)
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

    side, n_b = 1 << a.log2_side, 32
    n = side * side
    dev = torch.device("cuda", 0)
    names, p0, lo, hi = synth.shared_arrays("tri_reduced")
    atoms = np.ascontiguousarray(np.array(list(itertools.product(*[AXES[k] for k in names]))).T)
    b = synth.bvalues(n_b)
    s = torch.cuda.current_stream(dev).cuda_stream
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    out = {"_source_ids": _build.source_ids(), "device": torch.cuda.get_device_name(0), "n_vox": n, "n_b": n_b, "n_atoms": atoms.shape[1],
           "n_nb": 4, "n_colours": 2, "runs": 7, "warmup": 2}
    o = api.make_opts("tri_reduced", n_b, jac="analytic")
    y = synth.make_torch_rows("tri_reduced", 0, n, n_b, dev, sigma=0.01)[1]
    res = {k: e((5, n), torch.float64) for k in ("mean", "sd", "map_p")}
    res.update(map_atom=e(n, torch.int32), log_evidence=e(n, torch.float64), ess=e(n, torch.float64))
    nb, col = api.grid_neighbours(np.ones((side, side), bool), 4)
    order = np.argsort(col, kind="stable")
    place = np.empty(n, np.int64)
    place[order] = np.arange(n)
    nb = torch.from_numpy(np.where(nb[order] >= 0, place[np.maximum(nb[order], 0)], -1).astype(np.int32)).to(dev)
    start = np.concatenate([[0], np.cumsum(np.bincount(col))]).astype(np.int64)
    pr = 16.0 / (atoms.max(axis=1) - atoms.min(axis=1)) ** 2
    centre = api.grid_mrf_centre(atoms)
    fld = dict(field_q=e((5, n), torch.float64), field_n=e(n, torch.int32))
    t = {}
    for label, nsd in (("known_noise (noise_sd 0.01)", 0.01), ("marginalised", 0.0)):
        post = lambda: api.grid_posterior_device(o, n, b, y, atoms, None, lo, hi, False, None, nsd, res["mean"], res["sd"], res["map_atom"],
                                                 res["map_p"], res["log_evidence"], res["ess"], 0, s)
        mrf = lambda k: api.grid_posterior_mrf("tri_reduced", b, y, atoms, lo, hi, nb, start, pr, n_sweeps=k, noise_sd=nsd, out=res, stream=s)
        gather = lambda: api.grid_neighbour_field(nb, res["mean"], centre, pr, out=fld, stream=s)
        field = lambda: api.grid_posterior_field("tri_reduced", b, y, atoms, lo, hi, fld["field_q"], fld["field_n"], pr, res, noise_sd=nsd, stream=s)
        r = {"posterior": timed(torch, dev, post)}
        gather()
        r["gather_all_voxels"] = timed(torch, dev, gather)
        r["field_posterior_all_voxels"] = timed(torch, dev, field)
        r["driver_0_sweeps"], r["driver_4_sweeps"] = timed(torch, dev, lambda: mrf(0)), timed(torch, dev, lambda: mrf(4))
        r["posterior_again"] = timed(torch, dev, post)  # the yardstick once more, behind the others: the drift of the run
        pm = r["posterior"]["median_ms"]
        r["one_sweep_ms"] = (r["driver_4_sweeps"]["median_ms"] - r["driver_0_sweeps"]["median_ms"]) / 4
        r["one_sweep_over_posterior"] = r["one_sweep_ms"] / pm
        r["field_posterior_over_posterior"] = r["field_posterior_all_voxels"]["median_ms"] / pm
        r["gather_over_posterior"] = r["gather_all_voxels"]["median_ms"] / pm
        print(label, json.dumps(r), flush=True)
        t[label] = r
    out["time"] = t
    out["phantom"] = phantom_ratios()
    print(json.dumps(out["phantom"]), flush=True)
    if os.path.exists(a.out):
        with open(a.out) as fh:
            out["resources"] = json.load(fh).get("resources")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the neighbourhood (MRF) prior of the variable-projection posterior costs and what it is worth; writes
profiles/varpro_mrf_probe.json.

  time       device resident, 2^20 tri-S0 voxels x 32 b-values x 969 atoms (ordered triples of 19 rates), a 1024 x 1024 slice sorted
             by colour (4-neighbourhood, 2 colours), HIP events, median of 7 after 2 warm-ups, one process: the plain posterior,
             the gather and the field posterior over all voxels, the driver at 0 and at 4 sweeps (one sweep = their difference / 4),
             known and marginalised noise.  The grid solver's sweep costs 1.10 - 1.11 x its posterior: the expectation, not a gate.
  phantom    --phantom-reference (no GPU): tests/varpro_mrf_reference.phantom (24 x 24, two regions, bi-exponential with S0, 16
             b-values, 171 rate pairs) through the numpy reference: medians of |error| of the plain posterior and of the MRF at
             strength 4, 16 and 64, 6 sweeps, 5 % noise, seed 0.
  resources  --resources-only (no GPU): VGPR / AGPR / scratch / waves per SIMD of every kernel of pnx_varpro_mrf.hip from the
             compiler's summary for gfx950, and the atoms per LDS slab, merged into the JSON.
python profiles/varpro_mrf_probe.py [--out profiles/varpro_mrf_probe.json] [--log2-side 10] [--resources-only | --phantom-reference]"""
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
from varpro_probe import HI, LO, NAMES, RATES, data, timed  # noqa: E402  the posterior probe's dictionary, signals and timing loop

from pyneapple_amd import _build, api  # noqa: E402


def kernel_resources():
    src = os.path.join(_build.CSRC, "pnx_varpro_mrf.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.HIPCC, *_build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "v.o")]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            p = re.search(r"varpro_mrf_posterior_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])E", m.group(2))
            s = re.search(r"(varpro_mrf_flags_kernel)", m.group(2))
            name = f"varpro_mrf_posterior_kernel<NS={p.group(1)}, K={p.group(2)}, CLS={p.group(3)}, T1={p.group(4)}>" if p else s.group(1) if s else None
            if name:
                out[name] = {}
        elif name:
            out[name][m.group(1)] = int(m.group(2))
    lds = {f"n_b={n_b}, K={k}": api.varpro_mrf_slab_atoms(n_b, k) for n_b in (16, 32, 128) for k in (1, 2, 3)}
    return {"kernels": out, "atoms_per_lds_slab (pnx_varpro_mrf_args.hpp varpro_mrf_slab)": lds}


def phantom_reference():
    import varpro_mrf_reference as R

    ph = R.phantom(seed=0, noise=0.05)
    order, nb, start = R.colour_sort(ph["nb"], ph["colours"])
    y, truth = ph["y"][order], ph["truth"][order]
    err = lambda mean: np.median(np.abs(mean - truth), axis=0)
    # 1e-3: the box [0, 1] of the fraction clips at wrong-basin atoms, which loosens the reference's own eps_v past 1e-6 (1.5e-6 here);
    # medians over 576 voxels are compared, not voxels against a rounding bound
    kw = dict(noise_sd=0.05, max_eps=1e-3)
    args = ("bi_s0", ph["b"], y, ph["nl_atoms"], ph["lo"], ph["hi"], nb, start)
    base, nl, lp = R.base_posterior(*args[:6], **kw)
    plain = err(R.mrf(*args, np.zeros(4), 0, **kw)[0]["mean"])
    res = {"n_vox": int(y.shape[0]), "n_atoms": int(nl.shape[1]), "noise": 0.05, "n_sweeps": 6, "seed": 0,
           "plain_median_abs_error (f1, D1, D2, S0)": plain.tolist()}
    for strength in (4.0, 16.0, 64.0):
        state, delta, _ = R.mrf(*args, R.precision_of(base, nl, lp, strength), 6, **kw)
        res[f"strength_{strength:g}"] = {"median_abs_error": err(state["mean"]).tolist(), "ratio_to_plain": (err(state["mean"]) / plain).tolist(),
                                         "delta": delta}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "varpro_mrf_probe.json"))
    ap.add_argument("--log2-side", type=int, default=10)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--phantom-reference", action="store_true")
    a = ap.parse_args()
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            out = json.load(fh)
    if a.resources_only or a.phantom_reference:
        if a.resources_only:
            out["resources"] = kernel_resources()
        else:
            out["phantom_reference"] = phantom_reference()
            print(json.dumps(out["phantom_reference"]), flush=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
        return
    import torch

    side, n_b = 1 << a.log2_side, 32
    n = side * side
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    e = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)
    nl = np.ascontiguousarray(np.array([t for t in itertools.product(RATES, repeat=3) if t[0] > t[1] > t[2]]).T)
    out.update({"_source_ids": _build.source_ids(), "device": torch.cuda.get_device_name(0), "n_vox": n, "n_b": n_b, "n_atoms": int(nl.shape[1]),
                "n_nb": 4, "n_colours": 2, "runs": 7, "warmup": 2})
    o = api.make_opts("tri_s0", n_b, jac="analytic")
    n_small = min(n, 1 << 16)
    b, y_h, _ = data(n_small, 0.01, 1)
    y = torch.from_numpy(y_h).to(dev).repeat(n // n_small, 1).contiguous()
    res = {k: e((6, n)) for k in ("mean", "sd", "map_p")}
    res.update(map_atom=e(n, torch.int32), log_evidence=e(n), ess=e(n), clipped_mass=e(n))
    nb, col = api.grid_neighbours(np.ones((side, side), bool), 4)
    order = np.argsort(col, kind="stable")
    place = np.empty(n, np.int64)
    place[order] = np.arange(n)
    nb = torch.from_numpy(np.where(nb[order] >= 0, place[np.maximum(nb[order], 0)], -1).astype(np.int32)).to(dev)
    start = np.concatenate([[0], np.cumsum(np.bincount(col))]).astype(np.int64)
    nonlinear = np.array([k.startswith("D") for k in NAMES])
    pr = np.zeros(6)
    pr[nonlinear] = 16.0 / (nl.max(axis=1) - nl.min(axis=1)) ** 2
    centre = api.varpro_mrf_centre(nl, nonlinear)
    fld = dict(field_q=e((6, n)), field_n=e(n, torch.int32))
    t = {}
    for label, nsd in (("known_noise (noise_sd 0.01)", 0.01), ("marginalised", 0.0)):
        post = lambda: api.varpro_posterior_device(o, n, b, y, nl, None, LO, HI, None, nsd, True, res["mean"], res["sd"], res["map_atom"],
                                                   res["map_p"], res["log_evidence"], res["ess"], res["clipped_mass"], 0, s)
        mrf = lambda k: api.varpro_posterior_mrf("tri_s0", b, y, nl, LO, HI, nb, start, pr, n_sweeps=k, noise_sd=nsd, out=res, stream=s)
        gather = lambda: api.grid_neighbour_field(nb, res["mean"], centre, pr, out=fld, stream=s)
        field = lambda: api.varpro_posterior_field("tri_s0", b, y, nl, LO, HI, fld["field_q"], fld["field_n"], pr, res, noise_sd=nsd, stream=s)
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
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

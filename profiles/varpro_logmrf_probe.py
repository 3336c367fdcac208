#!/usr/bin/env python3
"""What the log coupling of the neighbourhood (MRF) prior of the variable-projection posterior costs and what it is worth
(DESIGN.md 4.1r); writes profiles/varpro_logmrf_probe.json.

  time       device resident, 2^20 tri-S0 voxels x 32 b-values x 969 atoms (ordered triples of 19 rates), a 1024 x 1024 slice sorted
             by colour (4-neighbourhood, 2 colours), HIP events, median of 7 after 2 warm-ups, one process: the plain posterior, the
             linear field posterior and the log-field posterior over all voxels, the log driver at 0 and at 4 sweeps (one sweep =
             their difference / 4), as ratios to the linear field call of the same run; known and marginalised noise.
  phantom    --phantom-reference (no GPU): tests/varpro_logmrf_reference.phantom through the numpy reference, coupling "log",
             strengths 4 / 16 / 64 / 256, 6 sweeps, 2 % and 5 % noise, seed 0: the ratios to the plain posterior of the median
             |error| of the linear posterior mean.  --phantom-device: the same through api.varpro_posterior_logmrf.
  remedies   --remedied-forms: the forms that pay for the register remedies, tri-reduced with a free T1 (2^18 voxels x 969 rate
             triples x 3 values of T1 = 2907 atoms, rates log, T1 linear): 32 b-values (two voxel rows per sweep instead of four) and
             64 b-values (two passes), the log-field call beside the linear field call of the same run.
  resources  --resources-only (no GPU): VGPR / AGPR / scratch / waves per SIMD of every kernel of pnx_varpro_logmrf.hip from the
             compiler's summary for gfx950 (the condition: scratch 0 everywhere), and the atoms per LDS slab, merged into the JSON.
python profiles/varpro_logmrf_probe.py [--out ...] [--log2-side 10] [--resources-only | --phantom-reference | --phantom-device |
--remedied-forms]"""
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
    src = os.path.join(_build.CSRC, "pnx_varpro_logmrf.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.HIPCC, *_build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "v.o")]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            p = re.search(r"varpro_logmrf_posterior_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])E", m.group(2))
            s = re.search(r"(varpro_logmrf_flags_kernel)", m.group(2))
            name = f"varpro_logmrf_posterior_kernel<NS={p.group(1)}, K={p.group(2)}, CLS={p.group(3)}, T1={p.group(4)}>" if p else s.group(1) if s else None
            if name:
                out[name] = {}
        elif name:
            out[name][m.group(1)] = int(m.group(2))
    lds = {f"n_b={n_b}, K={k}": api.varpro_logmrf_slab_atoms(n_b, k) for n_b in (16, 32, 128) for k in (1, 2, 3)}
    return {"kernels": out, "scratch_free": all(v.get("ScratchSize [bytes/lane]", 1) == 0 for v in out.values()),
            "atoms_per_lds_slab (pnx_varpro_logmrf_args.hpp varpro_logmrf_slab)": lds}


def phantom(device):
    import varpro_logmrf_reference as LR
    import varpro_mrf_reference as R

    res = {"n_sweeps": 6, "seed": 0, "coupling": "log", "columns": "f1, D1, D2, S0"}
    for noise in (0.02, 0.05):
        ph = LR.phantom(seed=0, noise=noise)
        order, nb, start = LR.colour_sort(ph["nb"], ph["colours"])
        y, truth = ph["y"][order], ph["truth"][order]
        err = lambda mean: np.median(np.abs(mean - truth), axis=0)
        # 1e-3: as profiles/varpro_mrf_probe.py -- medians over 576 voxels are compared, not voxels against a rounding bound
        kw = dict(noise_sd=noise, max_eps=1e-3)
        args = ("bi_s0", ph["b"], y, ph["nl_atoms"], ph["lo"], ph["hi"])
        base, nl, lp = R.base_posterior(*args, **kw)
        cp = LR.coupling_of(base, "log")
        plain = err(base["mean"])
        r = {"plain_median_abs_error": plain.tolist()}
        for strength in (4.0, 16.0, 64.0, 256.0):
            lam = LR.precision_of(base, nl, lp, strength, cp)
            if device:
                mean = api.varpro_posterior_logmrf(*args, nb, start, lam, cp, n_sweeps=6, noise_sd=noise)["mean"].T
            else:
                mean = LR.mrf(*args, nb, start, lam, cp, 6, **kw)[0]["mean"]
            r[f"strength_{strength:g}_ratio_to_plain"] = (err(mean) / plain).tolist()
        res[f"noise_{noise:g}"] = r
    return res


def remedied_forms():
    import torch

    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    n = 1 << 18
    triples = np.array([t for t in itertools.product(RATES, repeat=3) if t[0] > t[1] > t[2]])
    nl = np.ascontiguousarray(np.array([(*t, v) for t in triples for v in (600.0, 1000.0, 1600.0)]).T)
    lo, hi = np.array([0.0, 1e-5, 0.0, 1e-5, 1e-5, 100.0]), np.array([1.0, 0.5, 1.0, 0.5, 0.5, 5000.0])  # f1 D1 f2 D2 D3 T1
    nonlinear = np.array([False, True, False, True, True, True])
    cp = np.array([0, 1, 0, 1, 1, 0], np.int32)
    fcentre, frange = api.varpro_logmrf_centre(nl, nonlinear, cp)
    pr = np.where(frange > 0, 16.0 / np.where(frange > 0, frange, 1.0) ** 2, 0.0)
    pr_lin = np.zeros(6)
    pr_lin[nonlinear] = 16.0 / (nl.max(axis=1) - nl.min(axis=1)) ** 2
    nb, col = api.grid_neighbours(np.ones((512, 512), bool), 4)
    nbd = torch.from_numpy(nb).to(dev)  # timing only: the table feeds one gather, the colouring is not used
    e = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)
    out = {"n_vox": n, "n_atoms": int(nl.shape[1]), "model": "tri_reduced + free T1", "runs": 7, "warmup": 2}
    rng = np.random.default_rng(0)
    for n_b, form in ((32, "NS=8, two rows per sweep"), (64, "NS=32, two passes")):
        b = np.linspace(0.0, 1000.0, n_b)
        y_h = (1 - np.exp(-3000.0 / 1000.0)) * (0.2 * np.exp(-b * 0.08) + 0.3 * np.exp(-b * 0.007) + 0.5 * np.exp(-b * 6e-4))
        y = torch.from_numpy(y_h[None, :] + 0.01 * rng.standard_normal((1 << 14, n_b))).to(dev).repeat(n >> 14, 1).contiguous()
        res = {k: e((6, n)) for k in ("mean", "sd", "map_p", "field_mean")}
        res.update(map_atom=e(n, torch.int32), log_evidence=e(n), ess=e(n), clipped_mass=e(n))
        fld = dict(field_q=e((6, n)), field_n=e(n, torch.int32))
        kw = dict(noise_sd=0.01, t1_mode=1, tr=3000.0, stream=s)
        api.varpro_posterior_logmrf("tri_reduced", b, y, nl, lo, hi, torch.full((n, 1), -1, dtype=torch.int32, device=dev), np.array([0, n]), pr, cp,
                                    n_sweeps=0, out=res, **kw)
        api.grid_neighbour_field(nbd, res["field_mean"], fcentre, pr, out=fld, stream=s)
        lin = lambda: api.varpro_posterior_field("tri_reduced", b, y, nl, lo, hi, fld["field_q"], fld["field_n"], pr_lin, res, **kw)
        log = lambda: api.varpro_posterior_logfield("tri_reduced", b, y, nl, lo, hi, fld["field_q"], fld["field_n"], pr, cp, res, **kw)
        r = {"form": form, "linear_field": timed(torch, dev, lin), "log_field": timed(torch, dev, log), "linear_field_again": timed(torch, dev, lin)}
        r["log_over_linear"] = r["log_field"]["median_ms"] / r["linear_field"]["median_ms"]
        print(n_b, json.dumps(r), flush=True)
        out[f"n_b={n_b}"] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "varpro_logmrf_probe.json"))
    ap.add_argument("--log2-side", type=int, default=10)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--phantom-reference", action="store_true")
    ap.add_argument("--phantom-device", action="store_true")
    ap.add_argument("--remedied-forms", action="store_true")
    a = ap.parse_args()
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            out = json.load(fh)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    if a.resources_only or a.phantom_reference or a.phantom_device or a.remedied_forms:
        if a.resources_only:
            out["resources"] = kernel_resources()
        elif a.remedied_forms:
            out["remedied_forms"] = remedied_forms()
        else:
            key = "phantom_device" if a.phantom_device else "phantom_reference"
            out[key] = phantom(a.phantom_device)
            print(json.dumps(out[key]), flush=True)
        return save()
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
    res = {k: e((6, n)) for k in ("mean", "sd", "map_p", "field_mean")}
    res.update(map_atom=e(n, torch.int32), log_evidence=e(n), ess=e(n), clipped_mass=e(n))
    nb, col = api.grid_neighbours(np.ones((side, side), bool), 4)
    order = np.argsort(col, kind="stable")
    place = np.empty(n, np.int64)
    place[order] = np.arange(n)
    nb = torch.from_numpy(np.where(nb[order] >= 0, place[np.maximum(nb[order], 0)], -1).astype(np.int32)).to(dev)
    start = np.concatenate([[0], np.cumsum(np.bincount(col))]).astype(np.int64)
    nonlinear = np.array([k.startswith("D") for k in NAMES])
    cp = nonlinear.astype(np.int32)
    pr_lin = np.zeros(6)
    pr_lin[nonlinear] = 16.0 / (nl.max(axis=1) - nl.min(axis=1)) ** 2
    fcentre, frange = api.varpro_logmrf_centre(nl, nonlinear, cp)
    pr = np.where(frange > 0, 16.0 / np.where(frange > 0, frange, 1.0) ** 2, 0.0)
    fld = dict(field_q=e((6, n)), field_n=e(n, torch.int32))
    t = {}
    for label, nsd in (("known_noise (noise_sd 0.01)", 0.01), ("marginalised", 0.0)):
        post = lambda: api.varpro_posterior_device(o, n, b, y, nl, None, LO, HI, None, nsd, True, res["mean"], res["sd"], res["map_atom"],
                                                   res["map_p"], res["log_evidence"], res["ess"], res["clipped_mass"], 0, s)
        mrf = lambda k: api.varpro_posterior_logmrf("tri_s0", b, y, nl, LO, HI, nb, start, pr, cp, n_sweeps=k, noise_sd=nsd, out=res, stream=s)
        lin = lambda: api.varpro_posterior_field("tri_s0", b, y, nl, LO, HI, fld["field_q"], fld["field_n"], pr_lin, res, noise_sd=nsd, stream=s)
        log = lambda: api.varpro_posterior_logfield("tri_s0", b, y, nl, LO, HI, fld["field_q"], fld["field_n"], pr, cp, res, noise_sd=nsd,
                                                    stream=s)
        r = {"posterior": timed(torch, dev, post)}
        mrf(0)  # field_mean of the plain posterior, then a field from it
        api.grid_neighbour_field(nb, res["field_mean"], fcentre, pr, out=fld, stream=s)
        r["linear_field_posterior_all_voxels"] = timed(torch, dev, lin)
        mrf(0)
        api.grid_neighbour_field(nb, res["field_mean"], fcentre, pr, out=fld, stream=s)
        r["log_field_posterior_all_voxels"] = timed(torch, dev, log)
        r["log_driver_0_sweeps"], r["log_driver_4_sweeps"] = timed(torch, dev, lambda: mrf(0)), timed(torch, dev, lambda: mrf(4))
        r["linear_field_again"] = timed(torch, dev, lin)  # the yardstick once more, behind the others: the drift of the run
        lm = r["linear_field_posterior_all_voxels"]["median_ms"]
        r["one_log_sweep_ms"] = (r["log_driver_4_sweeps"]["median_ms"] - r["log_driver_0_sweeps"]["median_ms"]) / 4
        r["ratios_to_linear_field"] = {"log_field": r["log_field_posterior_all_voxels"]["median_ms"] / lm, "one_log_sweep": r["one_log_sweep_ms"] / lm,
                                       "log_driver_0_sweeps": r["log_driver_0_sweeps"]["median_ms"] / lm,
                                       "log_driver_4_sweeps": r["log_driver_4_sweeps"]["median_ms"] / lm,
                                       "posterior": r["posterior"]["median_ms"] / lm}
        print(label, json.dumps(r), flush=True)
        t[label] = r
    out["time"] = t
    save()


if __name__ == "__main__":
    main()

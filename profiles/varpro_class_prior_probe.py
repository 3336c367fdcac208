#!/usr/bin/env python3
"""One prior row per segmentation label over the variable-projection dictionary (pnx_curvefit_varpro_posterior_classes_f64,
pnx_curvefit_varpro_prior_em_classes_f64), measured beside the unlabelled posterior and one unlabelled EM update in the same
process.  Device resident, HIP events, two warm-up runs and seven timed runs each.

  time       2^20 tri-S0 voxels x 32 b-values (0 .. 1000) x 969 atoms (ordered triples of 19 rates), the shape of DESIGN.md 4.1i /
             4.1m, known and marginalised noise.  n_classes in {1, 4, 16}, labels sorted by class (one class per strip of 16
             voxels) and labels v % n_classes (every strip mixed).  posterior: the whole call.  one EM update:
             call(n_iter = 3) - call(n_iter = 2) at rel_tol = 0 -- a normaliser pass, an accumulate pass, the small kernels and
             the read-back.  Ratios are to the unlabelled calls of the same run.
  resources  --resources-only (no GPU): VGPR / AGPR / scratch / waves per SIMD of every instantiation of pnx_varpro_class.hip
             from the compiler's summary for gfx950, and the atoms per LDS slab, merged into the JSON.
python profiles/varpro_class_prior_probe.py [--out profiles/varpro_class_prior_probe.json] [--log2-voxels 20] [--resources-only]"""
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
from varpro_probe import HI, LO, RATES, data, timed  # noqa: E402  the same rates, box, signals and timing loop

from pyneapple_amd import _build, api  # noqa: E402

CLASSES = (1, 4, 16)


def kernel_resources():
    src = os.path.join(_build.CSRC, "pnx_varpro_class.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_build.HIPCC, *_build.CXXFLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "g.o")]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|TotalSGPRs): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            t = re.search(r"(varpro_class_(?:posterior|norm|acc)_kernel)ILi(\d+)ELi(\d+)ELi(\d+)E", m.group(2))
            s = re.search(r"(varpro_class_(?:table|sums|stats|finish)_kernel)", m.group(2))
            name = f"{t.group(1)}<NS={t.group(2)}, K={t.group(3)}, CLS={t.group(4)}>" if t else s.group(1) if s else None
            if name:
                out[name] = {}
        elif name:
            out[name][m.group(1)] = int(m.group(2))
    lds = {f"n_b={n_b}, k={k}, n_classes={c}": {"posterior": api.varpro_class_slab_atoms(n_b, k, c, k + 1), "em": api.varpro_class_slab_atoms(n_b, k, c, 4 * c)}
           for n_b in (16, 32, 128) for k in (2, 3) for c in CLASSES}
    return {"kernels": out, "atoms_per_lds_slab (pnx_varpro_class_args.hpp varpro_class_slab)": lds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "varpro_class_prior_probe.json"))
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

    n_small, n = 1 << min(16, a.log2_voxels), 1 << a.log2_voxels
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    e = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)
    nl = np.ascontiguousarray(np.array([t for t in itertools.product(RATES, repeat=3) if t[0] > t[1] > t[2]]).T)
    o = api.make_opts("tri_s0", 32, jac="analytic")
    out = {"_source_ids": _build.source_ids(), "device": torch.cuda.get_device_name(0), "n_vox": n, "n_b": 32, "n_atoms": int(nl.shape[1]),
           "runs": 7, "warmup": 2}
    b, y_h, _ = data(n_small, 0.01, 1)
    y = torch.from_numpy(y_h).to(dev).repeat(n // n_small, 1).contiguous()
    mean, sd, mp, lev, ess, cm, atom = e((6, n)), e((6, n)), e((6, n)), e(n), e(n), e(n), e(n, torch.int32)
    idx = torch.arange(n, device=dev, dtype=torch.int64)
    labels = {(c, "sorted"): (idx * c // n).to(torch.int32) for c in CLASSES}
    labels.update({(c, "interleaved"): (idx % c).to(torch.int32) for c in CLASSES})
    post = lambda nsd: api.varpro_posterior_device(o, n, b, y, nl, None, LO, HI, None, nsd, True, mean, sd, atom, mp, lev, ess, cm, 0, s)
    em = lambda nsd, k: api.varpro_prior_em_device(o, n, b, y, nl, None, LO, HI, None, nsd, True, k, 0.0, 0.0, 0, s)
    postc = lambda nsd, c, lab: api.varpro_posterior_classes_device(o, n, b, y, nl, None, LO, HI, lab, c, None, nsd, True, mean, sd, atom, mp, lev,
                                                                    ess, cm, 0, s)
    emc = lambda nsd, c, lab, k: api.varpro_prior_em_classes_device(o, n, b, y, nl, None, LO, HI, lab, c, None, nsd, True, k, 0.0, 0.0, 0, s)
    t = {}
    for label, nsd in (("known_noise (noise_sd 0.01)", 0.01), ("marginalised", 0.0)):
        r = {"posterior": timed(torch, dev, lambda: post(nsd))}
        e2, e3 = timed(torch, dev, lambda: em(nsd, 2)), timed(torch, dev, lambda: em(nsd, 3))
        r["em_n_iter_2"], r["em_n_iter_3"] = e2, e3
        r["one_update_ms"] = e3["median_ms"] - e2["median_ms"]
        for (c, kind), lab in labels.items():
            if c == 1 and kind == "interleaved":
                continue  # the same labels as sorted
            q = {"posterior": timed(torch, dev, lambda: postc(nsd, c, lab))}
            c2, c3 = timed(torch, dev, lambda: emc(nsd, c, lab, 2)), timed(torch, dev, lambda: emc(nsd, c, lab, 3))
            q["em_n_iter_2"], q["em_n_iter_3"] = c2, c3
            q["one_update_ms"] = c3["median_ms"] - c2["median_ms"]
            q["posterior_over_unlabelled"] = q["posterior"]["median_ms"] / r["posterior"]["median_ms"]
            q["update_over_unlabelled"] = q["one_update_ms"] / r["one_update_ms"]
            r[f"n_classes_{c}_{kind}"] = q
            print(label, c, kind, json.dumps(q), flush=True)
        r["posterior_again"] = timed(torch, dev, lambda: post(nsd))  # the yardstick once more, behind the sweep: the drift of the run
        print(label, "unlabelled", json.dumps({k: v for k, v in r.items() if not k.startswith("n_classes")}), flush=True)
        t[label] = r
    out["time"] = t
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

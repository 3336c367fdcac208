#!/usr/bin/env python3
"""What the constraint f1 + f2 <= 1 costs: pnx_curvefit_simplex_f64 against the box-only pnx_curvefit_batch_f64, device resident,
HIP events, two warm-up runs and seven interleaved timed runs each, on two volumes of 2^22 tri-exponential voxels x 32 b-values:
  c3          the benchmark's C3 volume (f3 >= 0.3 everywhere: hardly a violator)
  half_face   the recipe of the g13 fixtures: f3 = 0 on even voxels, U(0, 0.05) on odd ones, 2 % noise
python profiles/constrained_probe.py [--out profiles/constrained_probe.json] [--log2-voxels 22]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from pyneapple_amd import _build, api, synth  # noqa: E402


def half_face_volume(n, n_b, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64, device=dev)
    T = synth.TRUTH["tri_reduced"]
    b = torch.linspace(0.0, 1200.0, n_b, dtype=torch.float64, device=dev)
    f1 = u(0.2, 0.6)
    f3 = torch.where(torch.arange(n, device=dev) % 2 == 0, torch.zeros((), dtype=torch.float64, device=dev), u(0.0, 0.05))
    e = lambda D: torch.exp(-b[None, :] * D[:, None])
    y = f1[:, None] * e(u(*T["D1"])) + (1 - f1 - f3)[:, None] * e(u(*T["D2"])) + f3[:, None] * e(u(*T["D3"]))
    return y * (1.0 + 0.02 * torch.randn(y.shape, generator=g, dtype=torch.float64, device=dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "constrained_probe.json"))
    ap.add_argument("--log2-voxels", type=int, default=22)
    a = ap.parse_args()
    n, n_b = 1 << a.log2_voxels, 32
    dev = torch.device("cuda", 0)
    _, p0, lo, hi = synth.shared_arrays("tri_reduced")
    b = synth.bvalues(n_b)
    opts = api.make_opts("tri_reduced", n_b, max_nfev=250, ftol=1e-8, jac="fd")
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    popt, pcov, st, nf, cost = e((5, n), torch.float64), e((n, 5, 5), torch.float64), e(n, torch.int8), e(n, torch.int32), e(n, torch.float64)
    lam, face = e(n, torch.float64), e(n, torch.int8)
    s = torch.cuda.current_stream(dev).cuda_stream
    out = {"_source_ids": _build.source_ids(), "device": torch.cuda.get_device_name(0), "n_vox": n, "n_b": n_b, "runs": 7, "warmup": 2}
    for name in ("c3", "half_face"):
        y = synth.make_torch_rows("tri_reduced", 0, n, n_b, dev, sigma=0.01)[1] if name == "c3" else half_face_volume(n, n_b, dev)
        calls = {"box": lambda: api.curvefit_device(opts, n, b, y, p0, lo, hi, None, popt, pcov, st, nf, cost, 0, s),
                 "simplex": lambda: api.curvefit_constrained_device(opts, n, b, y, p0, lo, hi, popt, pcov, st, nf, cost, lam, face, 0, s)}
        ms = {k: [] for k in calls}
        for it in range(9):  # interleaved: box, simplex, box, simplex, ...
            for k, fn in calls.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                torch.cuda.synchronize(dev)
                if it >= 2:
                    ms[k].append(t0.elapsed_time(t1))
        f = face.cpu().numpy()  # of the last simplex run
        r = {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))} for k, v in ms.items()}
        r["violator_share"] = float((f > 0).mean())
        r["not_certified_share"] = float((f == 2).mean())
        r["failed_share"] = float((st.cpu().numpy() <= 0).mean())
        r["overhead_ms"] = r["simplex"]["median_ms"] - r["box"]["median_ms"]
        out[name] = r
        print(name, json.dumps(r), flush=True)
        del y
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""fp32-arithmetic curve fit against the fp64 one on C3: triexp reduced, 2^22 voxels, 32 b-values, 1 % noise, device resident,
the same float32 signal for both paths in one process:

    pnx_curvefit_fast_f32                      (fp32 arithmetic, analytic Jacobian)
    pnx_curvefit_batch_f32, jac="analytic"     (fp32 storage, fp64 arithmetic: the parent's kernel)

    python profiles/curvefit_f32_probe.py [--out profiles/curvefit_f32_probe.json] [--reps 7] [--log2n 22]

Two warm-up runs per path, then `reps` timed runs each, interleaved (A B A B ...) so that clock drift hits both; reported per
path: median, min, max of the wall time around enqueue + synchronize, voxels/s at the median, the spread (max - min) / median;
the ratio of the medians; mean evaluations per voxel and success share of each path; the cost of the fp32 result relative to
the fp64 result on the first 65 536 voxels; and the registers / LDS / scratch of the triexp instantiations
(tools/kernel_resources.py on the unit's object file, or profiles/curvefit_f32_resources.txt)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--log2n", type=int, default=22)
    a = ap.parse_args()
    import numpy as np
    import torch

    from pyneapple_amd import api, synth

    n, n_b = 1 << a.log2n, 32
    dev = torch.device("cuda", 0)
    names, p0, lo, hi = synth.shared_arrays("tri_reduced")
    b, y = synth.make_torch_rows("tri_reduced", 0, n, n_b, dev, sigma=0.01, dtype=torch.float32)
    opts = api.make_opts("tri_reduced", n_b, max_nfev=250, ftol=1e-8, jac="analytic")
    s = torch.cuda.current_stream(dev).cuda_stream

    def buffers():
        return dict(popt=torch.empty((5, n), dtype=torch.float32, device=dev), pcov=torch.empty((n, 5, 5), dtype=torch.float32, device=dev),
                    status=torch.empty(n, dtype=torch.int8, device=dev), nfev=torch.empty(n, dtype=torch.int32, device=dev),
                    cost=torch.empty(n, dtype=torch.float32, device=dev))

    out = {"fast_f32": buffers(), "batch_f32_analytic": buffers()}

    def run(path):
        o = out[path]
        api.curvefit_device(opts, n, b, y, p0, lo, hi, None, o["popt"], o["pcov"], o["status"], o["nfev"], o["cost"], 0, s,
                            precision="float32" if path == "fast_f32" else "float64")
        torch.cuda.synchronize(dev)

    for _ in range(2):
        for path in out:
            run(path)
    ts = {path: [] for path in out}
    for _ in range(a.reps):
        for path in out:
            t = time.perf_counter()
            run(path)
            ts[path].append(time.perf_counter() - t)
    res = {"workload": f"tri_reduced n_vox=2^{a.log2n} n_b={n_b} sigma=0.01 float32 signal, device resident", "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}
    for path, t in ts.items():
        med = statistics.median(t)
        o = out[path]
        res[path] = {"ms_median": med * 1e3, "ms_min": min(t) * 1e3, "ms_max": max(t) * 1e3, "spread": (max(t) - min(t)) / med,
                     "voxels_per_s": n / med, "mean_nfev": float(o["nfev"].double().mean()),
                     "success_share": float((o["status"] > 0).double().mean())}
    res["ratio_fast_over_batch"] = res["fast_f32"]["voxels_per_s"] / res["batch_f32_analytic"]["voxels_per_s"]
    m = min(n, 1 << 16)
    sys.path.insert(0, os.path.join(HERE, "tools"))
    import f32_yardstick as Y

    yh, bh = y[:m].cpu().numpy().astype(float), np.asarray(b, float)
    P32 = out["fast_f32"]["popt"][:, :m].cpu().numpy().T.astype(float)
    P64 = out["batch_f32_analytic"]["popt"][:, :m].cpu().numpy().T.astype(float)
    both = ((out["fast_f32"]["status"][:m] > 0) & (out["batch_f32_analytic"]["status"][:m] > 0)).cpu().numpy()
    ex = Y.cost_excess("tri_reduced", bh, yh, P32, P64)[both]
    res["cost_excess_vs_fp64_first_65536"] = {"max": float(ex.max()), "p99": float(np.quantile(ex, 0.99)), "median": float(np.median(ex))}
    # registers / LDS / scratch are a property of the build: from the unit's object file when it is at hand, else from the
    # listing kept beside this script (python tools/kernel_resources.py pyneapple_amd/csrc/_obj/pnx_curvefit_f32.o)
    obj = os.path.join(HERE, "pyneapple_amd", "csrc", "_obj", "pnx_curvefit_f32.o")
    if os.path.exists(obj):
        kr = subprocess.run([sys.executable, os.path.join(HERE, "tools", "kernel_resources.py"), obj], capture_output=True, text=True).stdout
    else:
        kr = open(os.path.join(HERE, "profiles", "curvefit_f32_resources.txt")).read()
    res["kernel_resources"] = [" ".join(ln.split()) for ln in kr.splitlines() if "curvefit_f32_kernel<4," in ln]
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

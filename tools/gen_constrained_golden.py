"""Fixtures of the constrained curve fit: tests/golden/g13_tri_constrained_{reduced,s0}.npz.

    PYNEAPPLE_SRC=<checkout of darksim33/Pyneapple>/src python tools/gen_constrained_golden.py

The reference is imported at run time (its ConstrainedCurveFitSolver, SLSQP through SciPy) with the two stand-ins of SURVEY.md
Appendix B in sys.modules; nothing of it is copied.  A fixture holds the inputs, the reference's popt and success flags and
the SciPy / numpy versions that produced them.

Recipe: 128 voxels, b = linspace(0, 1200, 32), default_rng(11); f1 ~ U(0.2, 0.6), f3 = 0 on even voxels and U(0, 0.05) on odd
ones, f2 = 1 - f1 - f3; D1, D2, D3 from the benchmark's ranges (pyneapple_amd/synth.py TRUTH); 2 % multiplicative noise; the
benchmark's tri-exponential p0 and bounds.  The S0 fixture multiplies the signal by 1000 and adds S0: p0 900, bounds (1, 5000).
The slow compartment is small or absent, so a fit with box bounds alone returns f1 + f2 > 1 on many voxels.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

N_VOX, N_B, SEED, NOISE = 128, 32, 11, 0.02
MAX_ITER, TOL = 250, 1e-8


def _import_reference():
    src = os.environ.get("PYNEAPPLE_SRC")
    if not src or not os.path.isdir(os.path.join(src, "pyneapple")):
        sys.exit("set PYNEAPPLE_SRC to the src/ directory of a Pyneapple checkout")
    sys.dont_write_bytecode = True
    sys.path.insert(0, src)

    class _Quiet:
        def __getattr__(self, name):
            return lambda *a, **k: None

    loguru = types.ModuleType("loguru")
    loguru.logger = _Quiet()
    sys.modules.setdefault("loguru", loguru)
    cv2 = types.ModuleType("cv2")
    cv2.INTER_LINEAR, cv2.INTER_CUBIC = 1, 2
    sys.modules.setdefault("cv2", cv2)
    import pyneapple

    return pyneapple


def signal():
    from pyneapple_amd import synth

    rng = np.random.default_rng(SEED)
    T = synth.TRUTH["tri_reduced"]
    b = np.linspace(0.0, 1200.0, N_B)
    f1 = rng.uniform(0.2, 0.6, N_VOX)
    f3 = np.where(np.arange(N_VOX) % 2 == 0, 0.0, rng.uniform(0.0, 0.05, N_VOX))
    f2 = 1.0 - f1 - f3
    D1, D2, D3 = (rng.uniform(*T[k], N_VOX) for k in ("D1", "D2", "D3"))
    e = lambda D: np.exp(-b[None, :] * D[:, None])
    y = f1[:, None] * e(D1) + f2[:, None] * e(D2) + f3[:, None] * e(D3)
    y = y * (1.0 + NOISE * rng.standard_normal(y.shape))
    truth = np.stack([f1, D1, f2, D2, D3])
    return b, np.ascontiguousarray(y), truth


def main():
    import scipy

    from pyneapple_amd import synth

    P = _import_reference()
    b, y, truth = signal()
    names, p0, lo, hi = synth.shared_arrays("tri_reduced")
    for tag, s0 in (("reduced", False), ("s0", True)):
        nm, p, l, h, yy = list(names), p0, lo, hi, y
        if s0:
            nm, yy = nm + ["S0"], y * 1000.0
            p, l, h = np.append(p0, 900.0), np.append(lo, 1.0), np.append(hi, 5000.0)
        model = P.TriExpModel(fit_reduced=True, fit_s0=s0)
        assert list(model.param_names) == nm, model.param_names
        solver = P.ConstrainedCurveFitSolver(model=model, p0=dict(zip(nm, map(float, p))),
                                             bounds={n: (float(a), float(c)) for n, a, c in zip(nm, l, h)},
                                             max_iter=MAX_ITER, tol=TOL, fraction_constraint=True)
        solver.fit(b, yy)
        popt = np.stack([np.atleast_1d(np.asarray(solver.params_[n], float)) for n in nm])
        success = np.array([bool(r.success) for r in solver.pixel_results_])
        out = os.path.join(ROOT, "tests", "golden", f"g13_tri_constrained_{tag}.npz")
        np.savez_compressed(out, model="tri_s0" if s0 else "tri_reduced", names=np.array(nm), b=b, y=yy, p0=p, lo=l, hi=h,
                            truth=truth, max_iter=MAX_ITER, tol=TOL, ref_popt=popt, ref_success=success,
                            scipy_version=scipy.__version__, numpy_version=np.__version__)
        f12 = popt[0] + popt[2]
        print(f"{out}: {int(success.sum())}/{N_VOX} reference successes, reference f1 + f2 max {f12.max():.17g}")


if __name__ == "__main__":
    main()

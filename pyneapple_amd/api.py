"""Array-level front-end of the C ABI: numpy (host staging) or torch-cuda tensors (HBM resident)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import CurvefitOpts, JAC_ANALYTIC, JAC_FD, MEM_DEVICE, MEM_HOST, check, load, ptr

MODEL_IDS = {"mono": 0, "bi_reduced": 1, "bi_s0": 2, "bi_full": 3, "tri_reduced": 4, "tri_s0": 5, "tri_full": 6}
MODEL_PARAM_NAMES = {
    "mono": ["S0", "D"],
    "bi_reduced": ["f1", "D1", "D2"],
    "bi_s0": ["f1", "D1", "D2", "S0"],
    "bi_full": ["f1", "D1", "f2", "D2"],
    "tri_reduced": ["f1", "D1", "f2", "D2", "D3"],
    "tri_s0": ["f1", "D1", "f2", "D2", "D3", "S0"],
    "tri_full": ["f1", "D1", "f2", "D2", "f3", "D3"],
}


def _is_torch(a):
    return a is not None and not isinstance(a, np.ndarray) and hasattr(a, "data_ptr")


def make_opts(model, n_b, fixed_idx=(), per_voxel=False, fixed_per_voxel=False, max_nfev=250, ftol=1e-8, xtol=1e-8,
              gtol=1e-8, jac="fd", t1_mode=0, tr=0.0, tm=0.0, sigma=None, absolute_sigma=False):
    """pnx_curvefit_opts.  sigma: None, a scalar or (n_b,) -- curve_fit's 1-D sigma shared by all voxels (a 2-D sigma is
    refused as SciPy refuses a wrong shape); absolute_sigma as in curve_fit.  The struct keeps the sigma array alive."""
    n_all = len(MODEL_PARAM_NAMES[model]) + (1 if t1_mode else 0)
    fixed_idx = [int(i) for i in fixed_idx]
    free_idx = [i for i in range(n_all) if i not in fixed_idx]
    o = CurvefitOpts()
    o.model = MODEL_IDS[model]
    o.n_b = int(n_b)
    o.n_free = len(free_idx)
    o.n_fixed = len(fixed_idx)
    for k, i in enumerate(free_idx):
        o.free_idx[k] = i
    for k, i in enumerate(fixed_idx):
        o.fixed_idx[k] = i
    o.per_voxel_p0_bounds = int(per_voxel)
    o.fixed_per_voxel = int(fixed_per_voxel)
    o.max_nfev = int(max_nfev)
    o.jac_mode = JAC_FD if jac == "fd" else JAC_ANALYTIC
    o.t1_mode, o.tr, o.tm = int(t1_mode), float(tr), float(tm)
    o.ftol, o.xtol, o.gtol = float(ftol), float(xtol), float(gtol)
    o.absolute_sigma = int(bool(absolute_sigma))
    if sigma is not None:
        sg = np.asarray(sigma, np.float64)
        if sg.size == 1:
            sg = np.full(int(n_b), float(sg.reshape(-1)[0]))
        elif sg.shape != (int(n_b),):
            raise ValueError("`sigma` has incorrect shape." if sg.ndim != 2 else
                             "a 2-D sigma (covariance matrix of the measurements) is not implemented by the HIP solver")
        o._sigma_keepalive = np.ascontiguousarray(sg)  # the struct holds a raw pointer
        o.sigma = o._sigma_keepalive.ctypes.data
    return o


def _precision(precision):
    if precision not in ("float64", "float32"):
        raise ValueError(f"precision must be 'float64' or 'float32', got {precision!r}")
    return precision == "float32"


def _out(out, key, shape, dtype):
    """A caller-provided result array (`out[key]`: C-contiguous, right shape and dtype -- e.g. a row range of a larger array
    that several device shards fill) or a fresh one."""
    a = None if out is None else out.get(key)
    if a is None:
        return np.empty(shape, dtype)
    if a.shape != tuple(np.atleast_1d(shape)) or a.dtype != np.dtype(dtype) or not a.flags.c_contiguous:
        raise ValueError(f"out[{key!r}] must be a C-contiguous {np.dtype(dtype).name} array of shape {shape}")
    return a


def curvefit(model, b, y, p0, lo, hi, *, fixed_idx=(), fixed_vals=None, max_nfev=250, ftol=1e-8, xtol=1e-8,
             gtol=1e-8, jac=None, want_pcov=True, device=0, t1_mode=0, tr=0.0, tm=0.0, out=None, sigma=None,
             absolute_sigma=False, precision="float64"):
    """Batched bounded NLLS on host (numpy) arrays.  Shapes as in include/pnx.h.

    A float32 signal array selects the fp32-storage entry point (pnx_curvefit_batch_f32: every data array float32 in
    and out, fp64 arithmetic on the device); anything else goes through pnx_curvefit_batch_f64.
    Returns dict(popt (n_free, n_vox), pcov (n_vox, n_free, n_free) | None, status int8, nfev int32, cost).
    `out`: optional dict of preallocated result arrays ("pcov", "status", "nfev", "cost") to write into.
    jac: "fd" or "analytic"; None = "fd" (SciPy's 2-point differences), and "analytic" with precision="float32".
    precision="float32": fp32 ARITHMETIC (pnx_curvefit_fast_f32, a separate kernel): every array crosses the ABI as float32
    whatever dtype the signal has, analytic Jacobian only, all parameters free, no T1 factor, no sigma.  The results are
    float32-quality minima, not SciPy-parity results (include/pnx.h).
    """
    fast = _precision(precision)
    if fast:
        if jac == "fd":
            raise ValueError("precision='float32' fits with the analytic Jacobian: SciPy's 2-point step is below fp32 resolution")
        if len(fixed_idx) or t1_mode or sigma is not None:
            raise ValueError("precision='float32' is built for all parameters free, without the T1 / STEAM factor and without sigma")
        jac = "analytic"
    elif jac is None:
        jac = "fd"
    _lib.require_device()
    dt = np.float32 if fast or getattr(y, "dtype", None) == np.float32 else np.float64
    b = np.ascontiguousarray(b, dt)
    y = np.ascontiguousarray(np.atleast_2d(y), dt)
    n_vox, n_b = y.shape
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    p0 = np.ascontiguousarray(p0, dt)
    lo = np.ascontiguousarray(lo, dt)
    hi = np.ascontiguousarray(hi, dt)
    per_voxel = p0.ndim == 2
    fv = None
    fpv = False
    if len(fixed_idx):
        fv = np.ascontiguousarray(fixed_vals, dt)
        fpv = fv.ndim == 2
    o = make_opts(model, n_b, fixed_idx, per_voxel, fpv, max_nfev, ftol, xtol, gtol, jac, t1_mode, tr, tm, sigma, absolute_sigma)
    n = o.n_free
    want = (n, n_vox) if per_voxel else (n,)
    if p0.shape != want or lo.shape != want or hi.shape != want:
        raise ValueError(f"p0/lo/hi must have shape {want}")
    if fv is not None and fv.shape != ((o.n_fixed, n_vox) if fpv else (o.n_fixed,)):
        raise ValueError("fixed_vals has the wrong shape")
    popt = np.empty((n, n_vox), dt)
    pcov = _out(out, "pcov", (n_vox, n, n), dt) if want_pcov else None
    status = _out(out, "status", (n_vox,), np.int8)
    nfev = _out(out, "nfev", (n_vox,), np.int32)
    cost = _out(out, "cost", (n_vox,), dt)
    fn = load().pnx_curvefit_fast_f32 if fast else load().pnx_curvefit_batch_f32 if dt is np.float32 else load().pnx_curvefit_batch_f64
    check(fn(C.byref(o), n_vox, ptr(b), ptr(y), ptr(p0), ptr(lo), ptr(hi), ptr(fv),
                                        ptr(popt), ptr(pcov), ptr(status), ptr(nfev), ptr(cost), MEM_HOST, device, None))
    return dict(popt=popt, pcov=pcov, status=status, nfev=nfev, cost=cost)


CONSTRAINED_MODELS = ("tri_reduced", "tri_s0")  # the layouts with exactly two fractions and f3 = 1 - f1 - f2


def _constrained_refusals(model, fixed_idx=(), fixed_vals=None, t1_mode=0, sigma=None, precision="float64"):
    if model not in CONSTRAINED_MODELS:
        raise ValueError(f"the constraint f1 + f2 <= 1 is defined for the models {CONSTRAINED_MODELS}, not for {model!r}")
    if len(fixed_idx) or fixed_vals is not None or t1_mode or sigma is not None:
        raise ValueError("the constrained fit is built for all parameters free, without the T1 / STEAM factor and without sigma")
    if precision != "float64":
        raise ValueError("the constrained fit is built for precision='float64' only")


def curvefit_constrained(model, b, y, p0, lo, hi, *, fixed_idx=(), fixed_vals=None, max_nfev=250, ftol=1e-8, xtol=1e-8,
                         gtol=1e-8, jac=None, want_pcov=True, device=0, t1_mode=0, tr=0.0, tm=0.0, out=None, sigma=None,
                         absolute_sigma=False, precision="float64"):
    """`curvefit` with the constraint f1 + f2 <= 1 (pnx_curvefit_simplex_f64; method and outputs: include/pnx.h), float64 host
    arrays, model "tri_reduced" or "tri_s0".  The signature is `curvefit`'s; what the constrained fit is not built for (fixed
    parameters, T1, sigma, precision="float32") raises ValueError.  Returns `curvefit`'s dict plus "lambda" (n_vox,) float64,
    the multiplier of the constraint (0 for an interior voxel), and "face" (n_vox,) int8: 0 interior -- the voxel's entries are
    those of `curvefit` --, 1 on the face f1 + f2 = 1 with lambda >= 0, 2 on the face and not certified.
    `out` may also hold "lambda" and "face"."""
    _constrained_refusals(model, fixed_idx, fixed_vals, t1_mode, sigma, precision)
    _lib.require_device()
    dt = np.float64
    b = np.ascontiguousarray(b, dt)
    y = np.ascontiguousarray(np.atleast_2d(y), dt)
    n_vox, n_b = y.shape
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    p0, lo, hi = (np.ascontiguousarray(a, dt) for a in (p0, lo, hi))
    per_voxel = p0.ndim == 2
    o = make_opts(model, n_b, (), per_voxel, False, max_nfev, ftol, xtol, gtol, jac or "fd", absolute_sigma=absolute_sigma)
    n = o.n_free
    want = (n, n_vox) if per_voxel else (n,)
    if p0.shape != want or lo.shape != want or hi.shape != want:
        raise ValueError(f"p0/lo/hi must have shape {want}")
    popt = np.empty((n, n_vox), dt)
    pcov = _out(out, "pcov", (n_vox, n, n), dt) if want_pcov else None
    status = _out(out, "status", (n_vox,), np.int8)
    nfev = _out(out, "nfev", (n_vox,), np.int32)
    cost = _out(out, "cost", (n_vox,), dt)
    lam = _out(out, "lambda", (n_vox,), dt)
    face = _out(out, "face", (n_vox,), np.int8)
    check(load().pnx_curvefit_simplex_f64(C.byref(o), n_vox, ptr(b), ptr(y), ptr(p0), ptr(lo), ptr(hi), None, ptr(popt), ptr(pcov),
                                          ptr(status), ptr(nfev), ptr(cost), ptr(lam), ptr(face), MEM_HOST, device, None))
    return {"popt": popt, "pcov": pcov, "status": status, "nfev": nfev, "cost": cost, "lambda": lam, "face": face}


def curvefit_constrained_device(opts, n_vox, b, y, p0, lo, hi, popt, pcov, status, nfev, cost, lam, face, device, stream=None):
    """The constrained fit on HBM-resident float64 torch tensors (pnx_curvefit_simplex_f64, PNX_MEM_DEVICE).  Unlike
    `curvefit_device` the call synchronises the stream once, behind the first fit, to read the number of violators; the second
    fit and the merge are enqueued.  `lam` (float64) / `face` (int8): device tensors of n_vox entries, or None."""
    b = np.ascontiguousarray(b, np.float64)
    if not getattr(opts, "per_voxel_p0_bounds", 0):
        p0, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (p0, lo, hi))
    check(load().pnx_curvefit_simplex_f64(C.byref(opts), int(n_vox), ptr(b), ptr(y), ptr(p0), ptr(lo), ptr(hi), None, ptr(popt),
                                          ptr(pcov), ptr(status), ptr(nfev), ptr(cost), ptr(lam), ptr(face), MEM_DEVICE, int(device),
                                          stream))


def release_staging(device=0):
    """Free the device staging slab / pinned block / streams a streamed host-array curve fit keeps for the next call."""
    check(load().pnx_release_staging(int(device)))


def curvefit_device(opts, n_vox, b, y, p0, lo, hi, fixed, popt, pcov, status, nfev, cost, device, stream=None, order=None,
                    precision="float64"):
    """Enqueue a batched fit on HBM-resident torch tensors (asynchronous; caller synchronises).  float32 tensors
    select the fp32-storage entry point.  `order`: optional int32 device tensor, a permutation of the voxel indices in which
    the kernel's queue hands the voxels out (longest fits first hides the straggler tail; results do not depend on it).
    precision="float32": fp32 arithmetic (pnx_curvefit_fast_f32); the tensors must be float32 and `opts` made with
    jac="analytic" -- everything the fp32 kernel is not built for is refused by the library."""
    fast = _precision(precision)
    f32 = "float32" in str(getattr(y, "dtype", ""))
    if fast and not f32:
        raise ValueError("precision='float32' takes float32 tensors")
    b = np.ascontiguousarray(b, np.float32 if f32 else np.float64)
    if not getattr(opts, "per_voxel_p0_bounds", 0):
        p0, lo, hi = (np.ascontiguousarray(a, b.dtype) for a in (p0, lo, hi))
    if isinstance(fixed, np.ndarray):
        fixed = np.ascontiguousarray(fixed, b.dtype)
    fn = load().pnx_curvefit_fast_f32 if fast else load().pnx_curvefit_batch_f32 if f32 else load().pnx_curvefit_batch_f64
    if order is not None and (tuple(order.shape) != (int(n_vox),) or "int32" not in str(order.dtype)):
        raise ValueError("order must be an int32 device tensor of n_vox entries")
    opts.queue_order = ptr(order)  # explicit per call (None clears what an earlier call with these opts set)
    try:
        check(fn(C.byref(opts), int(n_vox), ptr(b), ptr(y), ptr(p0), ptr(lo), ptr(hi),
                 ptr(fixed), ptr(popt), ptr(pcov), ptr(status), ptr(nfev), ptr(cost), MEM_DEVICE, int(device), stream))
    finally:
        opts.queue_order = None


GRID_MAX_ATOMS = 4096  # kGridMaxAtoms of csrc/pnx_grid_args.hpp
PROJECT_MODELS = ("mono", "bi_s0", "tri_s0")  # the layouts with a linear amplitude S0


def grid_start(model, b, y, atoms, lo, hi, *, fixed_idx=(), fixed_vals=None, sigma=None, project_amplitude=False, t1_mode=0,
               tr=0., tm=0., device=0, out=None):
    """Per-voxel start values from a dictionary search on host (numpy) arrays (pnx_curvefit_grid_start_f64; method: include/pnx.h).

    atoms (n_free, n_atoms <= 4096) parameter-major like p0, every column a candidate start inside the shared bounds lo / hi
    (n_free,); fixed_idx / fixed_vals (n_fixed,) and sigma as `curvefit` takes them (shared values only).  project_amplitude: fit
    the linear amplitude S0 per voxel and atom (clipped to its bounds) instead of taking it from the atoms; models "mono",
    "bi_s0", "tri_s0".  Returns dict(p0 (n_free, n_vox) -- ready for `curvefit(..., p0=p0, lo tiled, hi tiled)` --, best (n_vox,)
    int32 index of the chosen atom, -1 for a non-finite signal, cost (n_vox,) 0.5 ||(y - s_best) / sigma||^2).
    `out`: optional dict of preallocated result arrays ("p0", "best", "cost")."""
    _lib.require_device()
    b = np.ascontiguousarray(b, np.float64)
    y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
    n_vox, n_b = y.shape
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    atoms, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (atoms, lo, hi))
    fv = None
    if len(fixed_idx):
        fv = np.ascontiguousarray(fixed_vals, np.float64)
        if fv.ndim != 1:
            raise ValueError("grid_start takes shared fixed values (n_fixed,): per-voxel fixed maps are not built")
    o = make_opts(model, n_b, fixed_idx, jac="analytic", t1_mode=t1_mode, tr=tr, tm=tm, sigma=sigma)
    n = o.n_free
    if atoms.ndim != 2 or atoms.shape[0] != n or lo.shape != (n,) or hi.shape != (n,):
        raise ValueError(f"atoms must have shape ({n}, n_atoms), lo / hi ({n},)")
    if fv is not None and fv.shape != (o.n_fixed,):
        raise ValueError("fixed_vals has the wrong shape")
    p0 = _out(out, "p0", (n, n_vox), np.float64)
    best = _out(out, "best", (n_vox,), np.int32)
    cost = _out(out, "cost", (n_vox,), np.float64)
    check(load().pnx_curvefit_grid_start_f64(C.byref(o), n_vox, ptr(b), ptr(y), int(atoms.shape[1]), ptr(atoms), ptr(fv), ptr(lo), ptr(hi),
                                             int(bool(project_amplitude)), ptr(p0), ptr(best), ptr(cost), MEM_HOST, int(device), None))
    return dict(p0=p0, best=best, cost=cost)


def grid_start_device(opts, n_vox, b, y, atoms, fixed, lo, hi, project_amplitude, p0, best, cost, device, stream=None):
    """Enqueue the dictionary search on HBM-resident float64 torch tensors (asynchronous; caller synchronises): y (n_vox, n_b),
    p0 (n_free, n_vox), best (n_vox,) int32 or None, cost (n_vox,) or None on the device; b, atoms (n_free, n_atoms), shared fixed
    values, lo, hi are host arrays.  `opts` from make_opts (model, fixed positions, T1, sigma)."""
    b, atoms, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (b, atoms, lo, hi))
    if fixed is not None:
        fixed = np.ascontiguousarray(fixed, np.float64)
    if atoms.ndim != 2:
        raise ValueError("atoms must have shape (n_free, n_atoms)")
    check(load().pnx_curvefit_grid_start_f64(C.byref(opts), int(n_vox), ptr(b), ptr(y), int(atoms.shape[1]), ptr(atoms), ptr(fixed), ptr(lo),
                                             ptr(hi), int(bool(project_amplitude)), ptr(p0), ptr(best), ptr(cost), MEM_DEVICE, int(device),
                                             stream))


def grid_posterior_slab_atoms(n_b, n_free):
    """Atoms per LDS slab of the posterior kernel (grid_posterior_slab of csrc/pnx_grid_posterior_args.hpp): the widest multiple of
    16, at most 256, whose dictionary rows ([n_b padded to 4][stride], stride = 16 mod 32) and 3 + n_free values per atom fit 64 KB."""
    kpad, width = (int(n_b) + 3) & ~3, 16
    for w in range(16, 257, 16):
        if kpad * (w if w & 16 else w + 16) + (3 + int(n_free)) * w <= 8192:
            width = w
    return width


def _posterior_log_prior(log_prior, n_atoms):
    if log_prior is None:
        return None
    lp = np.ascontiguousarray(log_prior, np.float64)
    if lp.shape != (n_atoms,):
        raise ValueError(f"log_prior has shape {lp.shape}, expected ({n_atoms},): one entry per atom")
    return lp


def grid_posterior(model, b, y, atoms, lo, hi, *, log_prior=None, noise_sd=0.0, fixed_idx=(), fixed_vals=None, sigma=None,
                   project_amplitude=False, t1_mode=0, tr=0., tm=0., device=0, out=None):
    """Posterior of every voxel over a dictionary of parameter vectors on host (numpy) arrays (pnx_curvefit_grid_posterior_f64;
    method: include/pnx.h).  The arguments of `grid_start`, and
    log_prior: None (uniform) or (n_atoms,) log prior weights, finite or -inf (an atom at -inf is excluded);
    noise_sd: > 0 a known Gaussian noise sd in the units of the (sigma-weighted) signal, 0 (default) marginalises the noise scale.
    Returns dict(mean, sd, map_p (n_free, n_vox), map_atom (n_vox,) int32 (-1 for a non-finite signal, whose floating outputs are
    NaN), log_evidence (n_vox,), ess (n_vox,) the effective number of atoms that carry the posterior: near 1 the grid is too
    coarse for sd to mean anything).  `out`: optional dict of preallocated result arrays under the same keys."""
    _lib.require_device()
    b = np.ascontiguousarray(b, np.float64)
    y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
    n_vox, n_b = y.shape
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    atoms, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (atoms, lo, hi))
    fv = None
    if len(fixed_idx):
        fv = np.ascontiguousarray(fixed_vals, np.float64)
        if fv.ndim != 1:
            raise ValueError("grid_posterior takes shared fixed values (n_fixed,): per-voxel fixed maps are not built")
    o = make_opts(model, n_b, fixed_idx, jac="analytic", t1_mode=t1_mode, tr=tr, tm=tm, sigma=sigma)
    n = o.n_free
    if atoms.ndim != 2 or atoms.shape[0] != n or lo.shape != (n,) or hi.shape != (n,):
        raise ValueError(f"atoms must have shape ({n}, n_atoms), lo / hi ({n},)")
    if fv is not None and fv.shape != (o.n_fixed,):
        raise ValueError("fixed_vals has the wrong shape")
    lp = _posterior_log_prior(log_prior, atoms.shape[1])
    res = {key: _out(out, key, (n, n_vox), np.float64) for key in ("mean", "sd", "map_p")}
    res["map_atom"] = _out(out, "map_atom", (n_vox,), np.int32)
    res["log_evidence"] = _out(out, "log_evidence", (n_vox,), np.float64)
    res["ess"] = _out(out, "ess", (n_vox,), np.float64)
    check(load().pnx_curvefit_grid_posterior_f64(C.byref(o), n_vox, ptr(b), ptr(y), int(atoms.shape[1]), ptr(atoms), ptr(fv), ptr(lo), ptr(hi),
                                                 int(bool(project_amplitude)), ptr(lp), float(noise_sd), ptr(res["mean"]), ptr(res["sd"]),
                                                 ptr(res["map_atom"]), ptr(res["map_p"]), ptr(res["log_evidence"]), ptr(res["ess"]), MEM_HOST,
                                                 int(device), None))
    return res


def grid_posterior_device(opts, n_vox, b, y, atoms, fixed, lo, hi, project_amplitude, log_prior, noise_sd, mean, sd, map_atom, map_p,
                          log_evidence, ess, device, stream=None):
    """Enqueue the grid posterior on HBM-resident float64 torch tensors (asynchronous; caller synchronises): y (n_vox, n_b), mean /
    sd / map_p (n_free, n_vox), map_atom (n_vox,) int32, log_evidence / ess (n_vox,) on the device, all but mean may be None; b,
    atoms (n_free, n_atoms), shared fixed values, lo, hi and log_prior (n_atoms,) or None are host arrays.  `opts` from make_opts."""
    b, atoms, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (b, atoms, lo, hi))
    if fixed is not None:
        fixed = np.ascontiguousarray(fixed, np.float64)
    if atoms.ndim != 2:
        raise ValueError("atoms must have shape (n_free, n_atoms)")
    lp = _posterior_log_prior(log_prior, atoms.shape[1])
    check(load().pnx_curvefit_grid_posterior_f64(C.byref(opts), int(n_vox), ptr(b), ptr(y), int(atoms.shape[1]), ptr(atoms), ptr(fixed), ptr(lo),
                                                 ptr(hi), int(bool(project_amplitude)), ptr(lp), float(noise_sd), ptr(mean), ptr(sd),
                                                 ptr(map_atom), ptr(map_p), ptr(log_evidence), ptr(ess), MEM_DEVICE, int(device), stream))


def grid_rician_slab_atoms(n_b, n_free):
    """Atoms per LDS slab of the Rician posterior kernel (grid_rician_slab of csrc/pnx_grid_rician_args.hpp): the posterior's rule
    with the signal rows of the block's waves (4 up to 32 b-values, 2 beyond; 16 rows of n_b padded to 4, plus 2, each) taken out of
    the 64 KB first."""
    kpad, width = (int(n_b) + 3) & ~3, 16
    room = 8192 - (4 if kpad <= 32 else 2) * 16 * (kpad + 2)
    for w in range(16, 257, 16):
        if kpad * (w if w & 16 else w + 16) + (3 + int(n_free)) * w <= room:
            width = w
    return width


def log_i0e(z, *, device=0, out=None, stream=None):
    """h(z) = log(exp(-z) I0(z)), the log of the exponentially scaled modified Bessel function of order zero, on the device
    (pnx_log_i0e_f64; csrc/pnx_bessel.hpp).  z: a float64 numpy array of any shape -- returns an array of that shape (`out`: optional
    preallocated result) --, or an HBM-resident float64 torch tensor with `out` a tensor of the same size (asynchronous on `stream`;
    returns `out`).  z >= 0 up to 1e300; a negative or NaN entry gives NaN."""
    _lib.require_device()
    if isinstance(z, np.ndarray) or not hasattr(z, "data_ptr"):
        z = np.ascontiguousarray(z, np.float64)
        res = _out({"h": out} if out is not None else None, "h", z.shape, np.float64)
        check(load().pnx_log_i0e_f64(int(z.size), ptr(z), ptr(res), MEM_HOST, int(device), None))
        return res
    if out is None or out.numel() != z.numel():
        raise ValueError("log_i0e on a device tensor takes `out`, a float64 device tensor of the same size")
    check(load().pnx_log_i0e_f64(int(z.numel()), ptr(z), ptr(out), MEM_DEVICE, int(device), stream))
    return out


def grid_posterior_rician(model, b, y, atoms, lo, hi, *, noise_sd, log_prior=None, fixed_idx=(), fixed_vals=None, sigma=None, t1_mode=0,
                          tr=0., tm=0., device=0, out=None):
    """`grid_posterior` under a Rician likelihood with a known noise sd, for magnitude signals y >= 0 on host (numpy) arrays
    (pnx_curvefit_grid_posterior_rician_f64; method: include/pnx.h).  The arguments of `grid_posterior` without project_amplitude
    (a free S0 sits on the grid as a row of `atoms`); noise_sd: the noise sd of the real and imaginary channels, finite and > 0
    (required: a marginalised noise scale is not built); sigma is refused by the library, by name.  Returns `grid_posterior`'s dict;
    log_evidence is log sum_g pi_g prod_i Rice(y_i | s_gi, noise_sd).  A voxel with a negative or non-finite entry gets NaN and
    map_atom = -1; a zero entry gives log_evidence = -inf and finite moments."""
    _lib.require_device()
    b = np.ascontiguousarray(b, np.float64)
    y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
    n_vox, n_b = y.shape
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    atoms, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (atoms, lo, hi))
    fv = None
    if len(fixed_idx):
        fv = np.ascontiguousarray(fixed_vals, np.float64)
        if fv.ndim != 1:
            raise ValueError("grid_posterior_rician takes shared fixed values (n_fixed,): per-voxel fixed maps are not built")
    o = make_opts(model, n_b, fixed_idx, jac="analytic", t1_mode=t1_mode, tr=tr, tm=tm, sigma=sigma)
    n = o.n_free
    if atoms.ndim != 2 or atoms.shape[0] != n or lo.shape != (n,) or hi.shape != (n,):
        raise ValueError(f"atoms must have shape ({n}, n_atoms), lo / hi ({n},)")
    if fv is not None and fv.shape != (o.n_fixed,):
        raise ValueError("fixed_vals has the wrong shape")
    lp = _posterior_log_prior(log_prior, atoms.shape[1])
    res = {key: _out(out, key, (n, n_vox), np.float64) for key in ("mean", "sd", "map_p")}
    res["map_atom"] = _out(out, "map_atom", (n_vox,), np.int32)
    res["log_evidence"] = _out(out, "log_evidence", (n_vox,), np.float64)
    res["ess"] = _out(out, "ess", (n_vox,), np.float64)
    check(load().pnx_curvefit_grid_posterior_rician_f64(C.byref(o), n_vox, ptr(b), ptr(y), int(atoms.shape[1]), ptr(atoms), ptr(fv), ptr(lo),
                                                        ptr(hi), ptr(lp), float(noise_sd), ptr(res["mean"]), ptr(res["sd"]),
                                                        ptr(res["map_atom"]), ptr(res["map_p"]), ptr(res["log_evidence"]), ptr(res["ess"]),
                                                        MEM_HOST, int(device), None))
    return res


def grid_posterior_rician_device(opts, n_vox, b, y, atoms, fixed, lo, hi, log_prior, noise_sd, mean, sd, map_atom, map_p, log_evidence, ess,
                                 device, stream=None):
    """Enqueue the Rician grid posterior on HBM-resident float64 torch tensors (asynchronous; caller synchronises): the tensors and
    host arrays of `grid_posterior_device`, without project_amplitude.  `opts` from make_opts."""
    b, atoms, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (b, atoms, lo, hi))
    if fixed is not None:
        fixed = np.ascontiguousarray(fixed, np.float64)
    if atoms.ndim != 2:
        raise ValueError("atoms must have shape (n_free, n_atoms)")
    lp = _posterior_log_prior(log_prior, atoms.shape[1])
    check(load().pnx_curvefit_grid_posterior_rician_f64(C.byref(opts), int(n_vox), ptr(b), ptr(y), int(atoms.shape[1]), ptr(atoms), ptr(fixed),
                                                        ptr(lo), ptr(hi), ptr(lp), float(noise_sd), ptr(mean), ptr(sd), ptr(map_atom),
                                                        ptr(map_p), ptr(log_evidence), ptr(ess), MEM_DEVICE, int(device), stream))


GRID_REFINE_MAX_POINTS = 9  # kRefineMaxPoints of csrc/pnx_grid_refine_args.hpp


def grid_refine(model, b, y, lo, hi, n_points, centre, half_width, *, noise_sd=0.0, fixed_idx=(), fixed_vals=None, sigma=None,
                project_amplitude=False, t1_mode=0, tr=0., tm=0., device=0, out=None):
    """Posterior of every voxel over a fine grid of its own on host (numpy) arrays (pnx_curvefit_grid_refine_f64; method:
    include/pnx.h): along free parameter k the n_points[k] (1..9) values from max(lo, centre - half_width) to
    min(hi, centre + half_width), a uniform prior over their Cartesian product (at most 4096 atoms), the direct cost.
    centre, half_width: (n_free, n_vox).  noise_sd > 0 known, <= 0 marginalised.  sigma and the T1 / STEAM factor are refused by the
    library, by name.  Returns dict(mean, sd, map_p, edge_mass (n_free, n_vox), ess, log_norm (n_vox,)); log_norm is a local
    normaliser, not an evidence; a voxel with a non-finite signal, centre or half-width, a negative half-width or no admitted atom is
    NaN everywhere.  `out`: optional dict of preallocated result arrays under the same keys."""
    _lib.require_device()
    b = np.ascontiguousarray(b, np.float64)
    y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
    n_vox, n_b = y.shape
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    lo, hi, centre, half_width = (np.ascontiguousarray(a, np.float64) for a in (lo, hi, centre, half_width))
    fv = None
    if len(fixed_idx):
        fv = np.ascontiguousarray(fixed_vals, np.float64)
        if fv.ndim != 1:
            raise ValueError("grid_refine takes shared fixed values (n_fixed,): per-voxel fixed maps are not built")
    o = make_opts(model, n_b, fixed_idx, jac="analytic", t1_mode=t1_mode, tr=tr, tm=tm, sigma=sigma)
    n = o.n_free
    npts = np.ascontiguousarray(n_points, np.int32)
    if lo.shape != (n,) or hi.shape != (n,) or npts.shape != (n,):
        raise ValueError(f"lo / hi / n_points must have shape ({n},)")
    if centre.shape != (n, n_vox) or half_width.shape != (n, n_vox):
        raise ValueError(f"centre and half_width must have shape ({n}, {n_vox}), got {centre.shape} and {half_width.shape}")
    if fv is not None and fv.shape != (o.n_fixed,):
        raise ValueError("fixed_vals has the wrong shape")
    res = {key: _out(out, key, (n, n_vox), np.float64) for key in ("mean", "sd", "map_p", "edge_mass")}
    res["ess"] = _out(out, "ess", (n_vox,), np.float64)
    res["log_norm"] = _out(out, "log_norm", (n_vox,), np.float64)
    check(load().pnx_curvefit_grid_refine_f64(C.byref(o), n_vox, ptr(b), ptr(y), ptr(fv), ptr(lo), ptr(hi), int(bool(project_amplitude)),
                                              float(noise_sd), ptr(npts), ptr(centre), ptr(half_width), ptr(res["mean"]), ptr(res["sd"]),
                                              ptr(res["map_p"]), ptr(res["ess"]), ptr(res["log_norm"]), ptr(res["edge_mass"]), MEM_HOST,
                                              int(device), None))
    return res


def grid_refine_device(opts, n_vox, b, y, fixed, lo, hi, project_amplitude, noise_sd, n_points, centre, half_width, mean, sd, map_p, ess,
                       log_norm, edge_mass, device, stream=None):
    """Enqueue the fine-grid posterior on HBM-resident float64 torch tensors (asynchronous; caller synchronises): y (n_vox, n_b),
    centre / half_width / mean / sd / map_p / edge_mass (n_free, n_vox), ess / log_norm (n_vox,) on the device, all outputs but mean
    may be None; b, shared fixed values, lo, hi and n_points are host arrays.  `opts` from make_opts."""
    b, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (b, lo, hi))
    if fixed is not None:
        fixed = np.ascontiguousarray(fixed, np.float64)
    npts = np.ascontiguousarray(n_points, np.int32)
    check(load().pnx_curvefit_grid_refine_f64(C.byref(opts), int(n_vox), ptr(b), ptr(y), ptr(fixed), ptr(lo), ptr(hi),
                                              int(bool(project_amplitude)), float(noise_sd), ptr(npts), ptr(centre), ptr(half_width), ptr(mean),
                                              ptr(sd), ptr(map_p), ptr(ess), ptr(log_norm), ptr(edge_mass), MEM_DEVICE, int(device), stream))


def grid_prior_slab_atoms(n_b):
    """Atoms per LDS slab of the two EM passes (grid_prior_slab of csrc/pnx_grid_prior_args.hpp): the posterior's slab at four
    parameter rows -- the four wave-private rows of the accumulate pass take the place of the parameter values."""
    return grid_posterior_slab_atoms(n_b, 4)


def _prior_em_call(o, n_vox, b, y, atoms, fv, lo, hi, project_amplitude, lp, noise_sd, n_iter, pseudo_count, rel_tol, mem, device, stream):
    n_iter = int(n_iter)
    out = np.empty(atoms.shape[1], np.float64)
    loglik = np.full(min(max(n_iter, 0), 1000) + 1, np.nan)  # outside 1..1000 the library refuses before it writes
    done, n_eff = C.c_int(0), C.c_int64(0)
    check(load().pnx_curvefit_grid_prior_em_f64(C.byref(o), int(n_vox), ptr(b), ptr(y), int(atoms.shape[1]), ptr(atoms), ptr(fv), ptr(lo),
                                                ptr(hi), int(bool(project_amplitude)), ptr(lp), float(noise_sd), n_iter, float(pseudo_count),
                                                float(rel_tol), ptr(out), ptr(loglik), C.byref(done), C.byref(n_eff), mem, int(device),
                                                stream))
    return dict(log_prior=out, loglik=loglik, n_iter=int(done.value), n_eff=int(n_eff.value))


def grid_prior_em(model, b, y, atoms, lo, hi, *, log_prior=None, noise_sd=0.0, n_iter=20, pseudo_count=0.0, rel_tol=1e-6, fixed_idx=(),
                  fixed_vals=None, sigma=None, project_amplitude=False, t1_mode=0, tr=0., tm=0., device=0):
    """The prior of `grid_posterior` learned from the voxels themselves on host (numpy) arrays (pnx_curvefit_grid_prior_em_f64;
    method: include/pnx.h): the maximum-likelihood mixture over the atoms by EM, pi_g <- mean over the finite voxels of their
    posterior weight on atom g.  The arguments of `grid_posterior` (log_prior is the start: None is uniform, an atom at -inf stays
    excluded), and
    n_iter: the most updates, 1..1000;  pseudo_count >= 0: added to every admissible atom's weight sum (0: plain maximum likelihood);
    rel_tol >= 0: stop once an update gains at most rel_tol |loglik| (0 runs all n_iter).
    Returns dict(log_prior (n_atoms,) normalised -- ready for `grid_posterior(..., log_prior=...)` --, loglik (n_iter + 1,) the
    log-likelihood of the volume under the prior before each update and under the returned one, NaN past n_iter, n_iter the updates
    done, n_eff the voxels with a finite signal).  The prior needs many voxels: a few dozen over-fit."""
    _lib.require_device()
    b = np.ascontiguousarray(b, np.float64)
    y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
    n_vox, n_b = y.shape
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    atoms, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (atoms, lo, hi))
    fv = None
    if len(fixed_idx):
        fv = np.ascontiguousarray(fixed_vals, np.float64)
        if fv.ndim != 1:
            raise ValueError("grid_prior_em takes shared fixed values (n_fixed,): per-voxel fixed maps are not built")
    o = make_opts(model, n_b, fixed_idx, jac="analytic", t1_mode=t1_mode, tr=tr, tm=tm, sigma=sigma)
    n = o.n_free
    if atoms.ndim != 2 or atoms.shape[0] != n or lo.shape != (n,) or hi.shape != (n,):
        raise ValueError(f"atoms must have shape ({n}, n_atoms), lo / hi ({n},)")
    if fv is not None and fv.shape != (o.n_fixed,):
        raise ValueError("fixed_vals has the wrong shape")
    lp = _posterior_log_prior(log_prior, atoms.shape[1])
    return _prior_em_call(o, n_vox, b, y, atoms, fv, lo, hi, project_amplitude, lp, noise_sd, n_iter, pseudo_count, rel_tol, MEM_HOST, device,
                          None)


def grid_prior_em_device(opts, n_vox, b, y, atoms, fixed, lo, hi, project_amplitude, log_prior, noise_sd, n_iter, pseudo_count, rel_tol,
                         device, stream=None):
    """`grid_prior_em` on an HBM-resident float64 torch tensor y (n_vox, n_b), read in place; b, atoms (n_free, n_atoms), shared fixed
    values, lo, hi and log_prior (n_atoms,) or None are host arrays, `opts` from make_opts.  The results are small host arrays, so
    unlike `grid_posterior_device` the call synchronises `stream` before it returns the same dict."""
    b, atoms, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (b, atoms, lo, hi))
    if fixed is not None:
        fixed = np.ascontiguousarray(fixed, np.float64)
    if atoms.ndim != 2:
        raise ValueError("atoms must have shape (n_free, n_atoms)")
    lp = _posterior_log_prior(log_prior, atoms.shape[1])
    return _prior_em_call(opts, n_vox, b, y, atoms, fixed, lo, hi, project_amplitude, lp, noise_sd, n_iter, pseudo_count, rel_tol, MEM_DEVICE,
                          device, stream)


GRID_MAX_CLASSES = 16  # kGridMaxClasses of csrc/pnx_grid_class_args.hpp


def grid_class_slab_atoms(n_b, n_classes, extra):
    """Atoms per LDS slab of the per-label kernels (grid_class_slab of csrc/pnx_grid_class_args.hpp): the widest multiple of 16, at
    most 256, whose dictionary rows and 2 + n_classes + extra values per atom fit 64 KB.  extra: n_free for the posterior,
    4 n_classes (the wave-private rows per class) for both EM passes."""
    kpad, width = (int(n_b) + 3) & ~3, 16
    for w in range(16, 257, 16):
        if kpad * (w if w & 16 else w + 16) + (2 + int(n_classes) + int(extra)) * w <= 8192:
            width = w
    return width


def _class_table(log_prior, n_classes, n_atoms):
    n_classes = int(n_classes)
    if not 1 <= n_classes <= GRID_MAX_CLASSES:
        raise ValueError(f"n_classes={n_classes} out of range [1, {GRID_MAX_CLASSES}]")
    if log_prior is None:
        return None
    lp = np.ascontiguousarray(log_prior, np.float64)
    if lp.shape != (n_classes, n_atoms):
        raise ValueError(f"log_prior has shape {lp.shape}, expected ({n_classes}, {n_atoms}): one row per class, one entry per atom")
    return lp


def _class_labels(labels, n_vox):
    """One int32 label per voxel for the per-label calls of either solver; a label that int32 cannot hold is background (-1)."""
    lab = np.asarray(labels)
    if lab.shape != (n_vox,) or lab.dtype.kind not in "iu":
        raise ValueError(f"labels must be {n_vox} integers (one per voxel), got shape {lab.shape} and dtype {lab.dtype}")
    return np.ascontiguousarray(np.where((lab < 0) | (lab > np.iinfo(np.int32).max), -1, lab), np.int32)


def _class_host_inputs(who, model, b, y, atoms, lo, hi, labels, fixed_idx, fixed_vals, sigma, t1_mode, tr, tm):
    b = np.ascontiguousarray(b, np.float64)
    y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
    n_vox, n_b = y.shape
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    atoms, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (atoms, lo, hi))
    fv = None
    if len(fixed_idx):
        fv = np.ascontiguousarray(fixed_vals, np.float64)
        if fv.ndim != 1:
            raise ValueError(f"{who} takes shared fixed values (n_fixed,): per-voxel fixed maps are not built")
    o = make_opts(model, n_b, fixed_idx, jac="analytic", t1_mode=t1_mode, tr=tr, tm=tm, sigma=sigma)
    n = o.n_free
    if atoms.ndim != 2 or atoms.shape[0] != n or lo.shape != (n,) or hi.shape != (n,):
        raise ValueError(f"atoms must have shape ({n}, n_atoms), lo / hi ({n},)")
    if fv is not None and fv.shape != (o.n_fixed,):
        raise ValueError("fixed_vals has the wrong shape")
    return o, n_vox, b, y, atoms, fv, lo, hi, _class_labels(labels, n_vox)


def grid_posterior_classes(model, b, y, atoms, lo, hi, labels, n_classes, *, log_prior=None, noise_sd=0.0, fixed_idx=(), fixed_vals=None,
                           sigma=None, project_amplitude=False, t1_mode=0, tr=0., tm=0., device=0, out=None):
    """`grid_posterior` with one prior row per segmentation label on host (numpy) arrays (pnx_curvefit_grid_posterior_classes_f64;
    method: include/pnx.h).  The arguments of `grid_posterior`, and
    labels (n_vox,) integers: the row of the table each voxel is judged under; a label outside [0, n_classes) -- background, -1 by
        convention -- gives the voxel NaN outputs and map_atom -1, as a non-finite signal does;
    n_classes: 1..16;  log_prior: None (every row uniform) or (n_classes, n_atoms), finite or -inf, every row with a finite entry.
    Returns the dict of `grid_posterior`."""
    _lib.require_device()
    o, n_vox, b, y, atoms, fv, lo, hi, lab = _class_host_inputs("grid_posterior_classes", model, b, y, atoms, lo, hi, labels, fixed_idx,
                                                                fixed_vals, sigma, t1_mode, tr, tm)
    n = o.n_free
    lp = _class_table(log_prior, n_classes, atoms.shape[1])
    res = {key: _out(out, key, (n, n_vox), np.float64) for key in ("mean", "sd", "map_p")}
    res["map_atom"] = _out(out, "map_atom", (n_vox,), np.int32)
    res["log_evidence"] = _out(out, "log_evidence", (n_vox,), np.float64)
    res["ess"] = _out(out, "ess", (n_vox,), np.float64)
    check(load().pnx_curvefit_grid_posterior_classes_f64(C.byref(o), n_vox, ptr(b), ptr(y), int(atoms.shape[1]), ptr(atoms), ptr(fv), ptr(lo),
                                                         ptr(hi), int(bool(project_amplitude)), int(n_classes), ptr(lab), ptr(lp),
                                                         float(noise_sd), ptr(res["mean"]), ptr(res["sd"]), ptr(res["map_atom"]),
                                                         ptr(res["map_p"]), ptr(res["log_evidence"]), ptr(res["ess"]), MEM_HOST, int(device),
                                                         None))
    return res


def grid_posterior_classes_device(opts, n_vox, b, y, atoms, fixed, lo, hi, project_amplitude, labels, n_classes, log_prior, noise_sd, mean,
                                  sd, map_atom, map_p, log_evidence, ess, device, stream=None):
    """Enqueue `grid_posterior_classes` on HBM-resident torch tensors (asynchronous; caller synchronises): the tensors of
    `grid_posterior_device` and labels (n_vox,) int32 on the device; log_prior (n_classes, n_atoms) or None is a host array."""
    b, atoms, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (b, atoms, lo, hi))
    if fixed is not None:
        fixed = np.ascontiguousarray(fixed, np.float64)
    if atoms.ndim != 2:
        raise ValueError("atoms must have shape (n_free, n_atoms)")
    lp = _class_table(log_prior, n_classes, atoms.shape[1])
    check(load().pnx_curvefit_grid_posterior_classes_f64(C.byref(opts), int(n_vox), ptr(b), ptr(y), int(atoms.shape[1]), ptr(atoms), ptr(fixed),
                                                         ptr(lo), ptr(hi), int(bool(project_amplitude)), int(n_classes), ptr(labels), ptr(lp),
                                                         float(noise_sd), ptr(mean), ptr(sd), ptr(map_atom), ptr(map_p), ptr(log_evidence),
                                                         ptr(ess), MEM_DEVICE, int(device), stream))


def _prior_em_classes_call(o, n_vox, b, y, atoms, fv, lo, hi, project_amplitude, labels, n_classes, lp, noise_sd, n_iter, pseudo_count,
                           rel_tol, mem, device, stream):
    n_iter, n_classes = int(n_iter), int(n_classes)
    out = np.empty((n_classes, atoms.shape[1]), np.float64)
    n_t = min(max(n_iter, 0), 1000) + 1  # outside 1..1000 the library refuses before it writes
    loglik, loglik_class = np.full(n_t, np.nan), np.full((n_t, n_classes), np.nan)
    done, n_eff = C.c_int(0), np.zeros(n_classes, np.int64)
    check(load().pnx_curvefit_grid_prior_em_classes_f64(C.byref(o), int(n_vox), ptr(b), ptr(y), int(atoms.shape[1]), ptr(atoms), ptr(fv),
                                                        ptr(lo), ptr(hi), int(bool(project_amplitude)), n_classes, ptr(labels), ptr(lp),
                                                        float(noise_sd), n_iter, float(pseudo_count), float(rel_tol), ptr(out), ptr(loglik),
                                                        ptr(loglik_class), C.byref(done), ptr(n_eff), mem, int(device), stream))
    return dict(log_prior=out, loglik=loglik, loglik_class=loglik_class, n_iter=int(done.value), n_eff=n_eff)


def grid_prior_em_classes(model, b, y, atoms, lo, hi, labels, n_classes, *, log_prior=None, noise_sd=0.0, n_iter=20, pseudo_count=0.0,
                          rel_tol=1e-6, fixed_idx=(), fixed_vals=None, sigma=None, project_amplitude=False, t1_mode=0, tr=0., tm=0., device=0):
    """`grid_prior_em` with one prior row per segmentation label, every row learned from its own voxels in one pass pair over the
    volume (pnx_curvefit_grid_prior_em_classes_f64; method: include/pnx.h).  The arguments of `grid_prior_em`, labels and n_classes as
    `grid_posterior_classes` takes them (a label outside [0, n_classes) takes no part), log_prior None or (n_classes, n_atoms): the
    start.  Returns dict(log_prior (n_classes, n_atoms) every row normalised -- ready for `grid_posterior_classes` --, loglik
    (n_iter + 1,) the sum over the classes, loglik_class (n_iter + 1, n_classes), n_iter the updates done, n_eff (n_classes,) the
    voxels of each class that took part; a class without one keeps its normalised start row)."""
    _lib.require_device()
    o, n_vox, b, y, atoms, fv, lo, hi, lab = _class_host_inputs("grid_prior_em_classes", model, b, y, atoms, lo, hi, labels, fixed_idx,
                                                                fixed_vals, sigma, t1_mode, tr, tm)
    lp = _class_table(log_prior, n_classes, atoms.shape[1])
    return _prior_em_classes_call(o, n_vox, b, y, atoms, fv, lo, hi, project_amplitude, lab, n_classes, lp, noise_sd, n_iter, pseudo_count,
                                  rel_tol, MEM_HOST, device, None)


def grid_prior_em_classes_device(opts, n_vox, b, y, atoms, fixed, lo, hi, project_amplitude, labels, n_classes, log_prior, noise_sd, n_iter,
                                 pseudo_count, rel_tol, device, stream=None):
    """`grid_prior_em_classes` on HBM-resident torch tensors y (n_vox, n_b) float64 and labels (n_vox,) int32, read in place; the
    other arguments are host arrays, `opts` from make_opts.  Synchronises `stream` before it returns the same dict."""
    b, atoms, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (b, atoms, lo, hi))
    if fixed is not None:
        fixed = np.ascontiguousarray(fixed, np.float64)
    if atoms.ndim != 2:
        raise ValueError("atoms must have shape (n_free, n_atoms)")
    lp = _class_table(log_prior, n_classes, atoms.shape[1])
    return _prior_em_classes_call(opts, n_vox, b, y, atoms, fixed, lo, hi, project_amplitude, labels, n_classes, lp, noise_sd, n_iter,
                                  pseudo_count, rel_tol, MEM_DEVICE, device, stream)


GRID_MRF_MAX_NEIGHBOURS = 8  # kGridMrfMaxNeighbours, kGridMrfMaxColours, kGridMrfMaxSweeps of csrc/pnx_grid_mrf_args.hpp
GRID_MRF_MAX_COLOURS = 8
GRID_MRF_MAX_SWEEPS = 100
_GRID_OFFSETS = {4: ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0)),
                 8: ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (-1, -1, 0), (-1, 1, 0), (1, -1, 0), (1, 1, 0)),
                 6: ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))}


def grid_mrf_slab_atoms(n_b, n_free):
    """Atoms per LDS slab of the field posterior (grid_mrf_slab of csrc/pnx_grid_mrf_args.hpp): the widest multiple of 16, at most
    256, whose dictionary rows, 4 + n_free values per atom (||s||^2, its inverse, log_prior, r_g, the centred parameter values) and
    the 8 doubles of the delta reduction fit 64 KB."""
    kpad, width = (int(n_b) + 3) & ~3, 16
    for w in range(16, 257, 16):
        if kpad * (w if w & 16 else w + 16) + (4 + int(n_free)) * w + 8 <= 8192:
            width = w
    return width


def grid_neighbours(mask, connectivity=6):
    """The neighbour table and the colours of the voxels of a boolean mask (2-D or 3-D), in mask-flattened (C) order -- the order
    of image[mask].  connectivity 4 or 8: in-plane, per slice of the last spatial axis of a 3-D mask; 6: the 3-D axis neighbours.
    Returns (neighbours (n, connectivity) int32 with -1 where a slot has no voxel inside the mask, colours (n,) int32): the
    coordinate parities, (i + j [+ k]) & 1 for connectivity 4 and 6 (2 colours), (i & 1) + 2 (j & 1) for 8 (4 colours), so that no
    voxel has a neighbour of its own colour.  Slot order: -x, +x, -y, +y, then the diagonals (8) or -z, +z (6)."""
    if connectivity not in _GRID_OFFSETS:
        raise ValueError(f"connectivity must be 4, 8 (in-plane) or 6 (3-D), got {connectivity!r}")
    mask = np.asarray(mask).astype(bool)
    if mask.ndim == 2:
        mask = mask[:, :, None]
    if mask.ndim != 3:
        raise ValueError(f"mask must be a 2-D or 3-D array, got shape {mask.shape}")
    n = int(mask.sum())
    if n > np.iinfo(np.int32).max:
        raise ValueError("the mask holds more voxels than an int32 index can address")
    idx = np.full(tuple(s + 2 for s in mask.shape), -1, np.int32)  # one voxel of padding on every side: absent
    inner = idx[1:-1, 1:-1, 1:-1]
    inner[mask] = np.arange(n, dtype=np.int32)
    offsets = _GRID_OFFSETS[connectivity]
    nb = np.empty((n, len(offsets)), np.int32)
    X, Y, Z = mask.shape
    for s, (dx, dy, dz) in enumerate(offsets):
        nb[:, s] = idx[1 + dx:1 + dx + X, 1 + dy:1 + dy + Y, 1 + dz:1 + dz + Z][mask]
    i, j, k = np.nonzero(mask)
    colours = ((i & 1) + 2 * (j & 1)) if connectivity == 8 else ((i + j + (k if connectivity == 6 else 0)) & 1)
    return nb, colours.astype(np.int32)


def grid_mrf_centre(atoms, log_prior=None, s0_row=-1):
    """The centres the posterior accumulates its moments about (grid_posterior_check_args): min + (max - min) / 2 of every row of
    atoms over the admissible atoms (log_prior > -inf), 0 for a projected S0 row.  What `grid_neighbour_field` takes as `centre`."""
    atoms = np.asarray(atoms, np.float64)
    adm = np.ones(atoms.shape[1], bool) if log_prior is None else np.asarray(log_prior, np.float64) > -np.inf
    mn, mx = atoms[:, adm].min(axis=1), atoms[:, adm].max(axis=1)
    centre = mn + 0.5 * (mx - mn)
    if s0_row >= 0:
        centre[s0_row] = 0.0
    return centre


def _mrf_precision(precision, n_free):
    pr = np.ascontiguousarray(precision, np.float64)
    if pr.shape != (n_free,):
        raise ValueError(f"precision has shape {pr.shape}, expected ({n_free},): one value per free parameter")
    return pr


def grid_neighbour_field(neighbours, mean, centre, precision, *, first=0, count=None, out=None, flag=None, device=0, stream=None):
    """The field of the neighbourhood prior for the voxels [first, first + count) (pnx_curvefit_grid_neighbour_field_f64; method:
    include/pnx.h): field_q[k, v] = precision[k] * sum over the present neighbours u of (mean[k, u] - centre[k]), slots in order,
    and field_n[v] their number.  neighbours (n_vox, n_nb) int32 and mean (n_free, n_vox) float64 are numpy arrays (staged; the
    call synchronises and raises on an index outside [-1, n_vox)) or torch tensors on the device (enqueued; `flag`, a device int32
    tensor preset to 2**31 - 1, receives the lowest offending voxel).  `out`: dict with "field_q" (n_free, n_vox) and "field_n"
    (n_vox,) int32 -- required for tensors, optional for arrays; only the range is written.  Returns that dict."""
    dev = _is_torch(mean)
    if dev != _is_torch(neighbours):
        raise ValueError("neighbours and mean must both be numpy arrays or both torch tensors")
    n_free, n_vox = mean.shape
    if tuple(neighbours.shape[:1]) != (n_vox,) or neighbours.ndim != 2:
        raise ValueError(f"neighbours must have shape ({n_vox}, n_nb), got {tuple(neighbours.shape)}")
    n_nb = int(neighbours.shape[1])
    centre, pr = _mrf_precision(centre, n_free), _mrf_precision(precision, n_free)
    count = n_vox - int(first) if count is None else int(count)
    if dev:
        if out is None or "field_q" not in out or "field_n" not in out:
            raise ValueError("device tensors need out={'field_q': ..., 'field_n': ...}")
        res = dict(field_q=out["field_q"], field_n=out["field_n"])
    else:
        _lib.require_device()
        neighbours = np.ascontiguousarray(neighbours, np.int32)
        mean = np.ascontiguousarray(mean, np.float64)
        res = dict(field_q=_out(out, "field_q", (n_free, n_vox), np.float64), field_n=_out(out, "field_n", (n_vox,), np.int32))
    check(load().pnx_curvefit_grid_neighbour_field_f64(n_vox, int(first), count, n_free, n_nb, ptr(neighbours), ptr(mean), ptr(centre), ptr(pr),
                                                       ptr(res["field_q"]), ptr(res["field_n"]), ptr(flag), MEM_DEVICE if dev else MEM_HOST,
                                                       int(device), stream))
    return res


def _mrf_host_inputs(who, model, b, n_b, atoms, lo, hi, fixed_idx, fixed_vals, sigma, t1_mode, tr, tm, log_prior):
    b = np.ascontiguousarray(b, np.float64)
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    atoms, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (atoms, lo, hi))
    fv = None
    if len(fixed_idx):
        fv = np.ascontiguousarray(fixed_vals, np.float64)
        if fv.ndim != 1:
            raise ValueError(f"{who} takes shared fixed values (n_fixed,): per-voxel fixed maps are not built")
    o = make_opts(model, n_b, fixed_idx, jac="analytic", t1_mode=t1_mode, tr=tr, tm=tm, sigma=sigma)
    n = o.n_free
    if atoms.ndim != 2 or atoms.shape[0] != n or lo.shape != (n,) or hi.shape != (n,):
        raise ValueError(f"atoms must have shape ({n}, n_atoms), lo / hi ({n},)")
    if fv is not None and fv.shape != (o.n_fixed,):
        raise ValueError("fixed_vals has the wrong shape")
    return o, b, atoms, fv, lo, hi, _posterior_log_prior(log_prior, atoms.shape[1])


_POSTERIOR_KEYS = ("mean", "sd", "map_atom", "map_p", "log_evidence", "ess")


def grid_posterior_field(model, b, y, atoms, lo, hi, field_q, field_n, precision, out, *, first=0, count=None, log_prior=None,
                         noise_sd=0.0, fixed_idx=(), fixed_vals=None, sigma=None, project_amplitude=False, t1_mode=0, tr=0., tm=0.,
                         delta_max=None, device=0, stream=None):
    """One colour update of the neighbourhood prior (pnx_curvefit_grid_posterior_field_f64; method: include/pnx.h): the posterior
    of the voxels [first, first + count) with the field inside l_g, written in place into the full-length tensors of `out`.
    Device only, asynchronous (the caller synchronises): y (n_vox, n_b), field_q (n_free, n_vox), field_n (n_vox,) int32 and
    out["mean"] (required, and read: delta compares against it), out["sd"], out["map_p"] (n_free, n_vox), out["map_atom"] (n_vox,)
    int32, out["log_evidence"], out["ess"] (n_vox,) are torch tensors on the device; delta_max: a one-element float64 device tensor
    or None.  The other arguments are `grid_posterior`'s host arrays and precision (n_free,).  Returns `out`."""
    for name, t in (("y", y), ("field_q", field_q), ("field_n", field_n), ("out['mean']", (out or {}).get("mean"))):
        if not _is_torch(t):
            raise ValueError(f"grid_posterior_field works in place on device tensors: {name} is not a torch tensor")
    n_vox, n_b = y.shape
    o, b, atoms, fv, lo, hi, lp = _mrf_host_inputs("grid_posterior_field", model, b, n_b, atoms, lo, hi, fixed_idx, fixed_vals, sigma, t1_mode,
                                                   tr, tm, log_prior)
    pr = _mrf_precision(precision, o.n_free)
    count = n_vox - int(first) if count is None else int(count)
    check(load().pnx_curvefit_grid_posterior_field_f64(C.byref(o), int(n_vox), ptr(b), ptr(y), int(atoms.shape[1]), ptr(atoms), ptr(fv), ptr(lo),
                                                       ptr(hi), int(bool(project_amplitude)), ptr(lp), float(noise_sd), int(first), count,
                                                       ptr(field_q), ptr(field_n), ptr(pr), ptr(out["mean"]), ptr(out.get("sd")),
                                                       ptr(out.get("map_atom")), ptr(out.get("map_p")), ptr(out.get("log_evidence")),
                                                       ptr(out.get("ess")), ptr(delta_max), MEM_DEVICE, int(device), stream))
    return out


def grid_posterior_mrf(model, b, y, atoms, lo, hi, neighbours, colour_start, precision, *, n_sweeps=4, tol=0.0, log_prior=None, noise_sd=0.0,
                       fixed_idx=(), fixed_vals=None, sigma=None, project_amplitude=False, t1_mode=0, tr=0., tm=0., device=0, out=None,
                       stream=None):
    """The grid posterior under a neighbourhood (MRF) prior by coloured mean-field sweeps (pnx_curvefit_grid_posterior_mrf_f64;
    method: include/pnx.h).  The arguments of `grid_posterior`, and
    neighbours (n_vox, n_nb <= 8) int32, -1 where a slot is empty, a symmetric graph; the voxels sorted by colour, with
    colour_start (n_colours + 1,) the offsets of the colour ranges (0 .. n_vox; no voxel has a neighbour inside its own range);
    precision (n_free,) >= 0, 0 on a projected S0; n_sweeps 0..100 (0: the plain posterior); tol >= 0: stop once a sweep moves no
    mean by more than tol of its grid range (0 runs all sweeps).
    y and neighbours are numpy arrays (staged once) or torch tensors on the device (read in place; `out` may hold preallocated
    result tensors); the call synchronises either way.  Returns the dict of `grid_posterior` -- log_evidence is the local normaliser
    of the last update, not a model evidence -- with "delta" (n_sweeps,) the largest relative move of a mean per sweep, NaN past
    "n_sweeps", the sweeps done."""
    dev = _is_torch(y)
    if dev != _is_torch(neighbours):
        raise ValueError("y and neighbours must both be numpy arrays or both torch tensors")
    if not dev:
        _lib.require_device()
        y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
        neighbours = np.ascontiguousarray(neighbours, np.int32)
    n_vox, n_b = y.shape
    o, b, atoms, fv, lo, hi, lp = _mrf_host_inputs("grid_posterior_mrf", model, b, n_b, atoms, lo, hi, fixed_idx, fixed_vals, sigma, t1_mode, tr,
                                                   tm, log_prior)
    n = o.n_free
    if neighbours.ndim != 2 or neighbours.shape[0] != n_vox:
        raise ValueError(f"neighbours must have shape ({n_vox}, n_nb), got {tuple(neighbours.shape)}")
    pr = _mrf_precision(precision, n)
    cs = np.ascontiguousarray(colour_start, np.int64)
    if cs.ndim != 1 or cs.size < 2:
        raise ValueError("colour_start must hold n_colours + 1 offsets")
    n_sweeps = int(n_sweeps)
    if dev:
        import torch

        mk = lambda key, shape, dt: (out or {}).get(key) if (out or {}).get(key) is not None else torch.empty(shape, dtype=dt, device=y.device)
        res = {key: mk(key, (n, n_vox), torch.float64) for key in ("mean", "sd", "map_p")}
        res["map_atom"] = mk("map_atom", (n_vox,), torch.int32)
        res["log_evidence"], res["ess"] = mk("log_evidence", (n_vox,), torch.float64), mk("ess", (n_vox,), torch.float64)
    else:
        res = {key: _out(out, key, (n, n_vox), np.float64) for key in ("mean", "sd", "map_p")}
        res["map_atom"] = _out(out, "map_atom", (n_vox,), np.int32)
        res["log_evidence"] = _out(out, "log_evidence", (n_vox,), np.float64)
        res["ess"] = _out(out, "ess", (n_vox,), np.float64)
    delta = np.full(min(max(n_sweeps, 0), GRID_MRF_MAX_SWEEPS), np.nan)  # outside 0..100 the library refuses before it writes
    done = C.c_int(0)
    check(load().pnx_curvefit_grid_posterior_mrf_f64(C.byref(o), int(n_vox), ptr(b), ptr(y), int(atoms.shape[1]), ptr(atoms), ptr(fv), ptr(lo),
                                                     ptr(hi), int(bool(project_amplitude)), ptr(lp), float(noise_sd), int(neighbours.shape[1]),
                                                     ptr(neighbours), int(cs.size - 1), ptr(cs), ptr(pr), n_sweeps, float(tol), ptr(res["mean"]),
                                                     ptr(res["sd"]), ptr(res["map_atom"]), ptr(res["map_p"]), ptr(res["log_evidence"]),
                                                     ptr(res["ess"]), ptr(delta), C.byref(done), MEM_DEVICE if dev else MEM_HOST, int(device),
                                                     stream))
    res["delta"], res["n_sweeps"] = delta, int(done.value)
    return res


def grid_neighbour_wfield(neighbours, mean, sd, centre, precision, dof, *, first=0, count=None, out=None, flag=None, edge_weight=False,
                          device=0, stream=None):
    """The weighted field of the edge-preserving (Student-t) neighbourhood prior for the voxels [first, first + count)
    (pnx_curvefit_grid_neighbour_wfield_f64; method and order of operations: include/pnx.h): per present neighbour u the weight
    w = (dof + K) / (dof + s_uv), s_uv = sum over the rows with a precision of precision[k] (sd[k, v]^2 + sd[k, u]^2 + (mean[k, v] -
    mean[k, u])^2); field_q[k, v] = precision[k] * sum w (mean[k, u] - centre[k]), field_w[v] = sum w, field_n[v] the present count.
    The arguments of `grid_neighbour_field` with sd (n_free, n_vox) like mean and dof > 0.  `out`: dict with "field_q", "field_w"
    (n_vox,) float64, "field_n" (n_vox,) int32 and optionally "edge_weight" (n_vox, n_nb) float64 -- required for tensors;
    edge_weight=True allocates the last for arrays.  Returns that dict."""
    dev = _is_torch(mean)
    if dev != _is_torch(neighbours) or dev != _is_torch(sd):
        raise ValueError("neighbours, mean and sd must all be numpy arrays or all torch tensors")
    n_free, n_vox = mean.shape
    if tuple(sd.shape) != (n_free, n_vox):
        raise ValueError(f"sd must have the shape of mean ({n_free}, {n_vox}), got {tuple(sd.shape)}")
    if tuple(neighbours.shape[:1]) != (n_vox,) or neighbours.ndim != 2:
        raise ValueError(f"neighbours must have shape ({n_vox}, n_nb), got {tuple(neighbours.shape)}")
    n_nb = int(neighbours.shape[1])
    centre, pr = _mrf_precision(centre, n_free), _mrf_precision(precision, n_free)
    count = n_vox - int(first) if count is None else int(count)
    if dev:
        if out is None or any(k not in out for k in ("field_q", "field_w", "field_n")):
            raise ValueError("device tensors need out={'field_q': ..., 'field_w': ..., 'field_n': ...}")
        res = {k: out[k] for k in ("field_q", "field_w", "field_n")}
        if out.get("edge_weight") is not None:
            res["edge_weight"] = out["edge_weight"]
    else:
        _lib.require_device()
        neighbours = np.ascontiguousarray(neighbours, np.int32)
        mean, sd = np.ascontiguousarray(mean, np.float64), np.ascontiguousarray(sd, np.float64)
        res = dict(field_q=_out(out, "field_q", (n_free, n_vox), np.float64), field_w=_out(out, "field_w", (n_vox,), np.float64),
                   field_n=_out(out, "field_n", (n_vox,), np.int32))
        if edge_weight or (out is not None and out.get("edge_weight") is not None):
            res["edge_weight"] = _out(out, "edge_weight", (n_vox, n_nb), np.float64)
    check(load().pnx_curvefit_grid_neighbour_wfield_f64(n_vox, int(first), count, n_free, n_nb, ptr(neighbours), ptr(mean), ptr(sd), ptr(centre),
                                                        ptr(pr), float(dof), ptr(res["field_q"]), ptr(res["field_w"]), ptr(res["field_n"]),
                                                        ptr(res.get("edge_weight")), ptr(flag), MEM_DEVICE if dev else MEM_HOST, int(device),
                                                        stream))
    return res


def grid_posterior_wfield(model, b, y, atoms, lo, hi, field_q, field_w, precision, out, *, first=0, count=None, log_prior=None,
                          noise_sd=0.0, fixed_idx=(), fixed_vals=None, sigma=None, project_amplitude=False, t1_mode=0, tr=0., tm=0.,
                          delta_max=None, device=0, stream=None):
    """One colour update under a real weight sum (pnx_curvefit_grid_posterior_wfield_f64): `grid_posterior_field` with field_w
    (n_vox,) float64 on the device in field_n's place, l = l0 + field - 1/2 W_v r_g.  With field_w = field_n as doubles it returns
    the bytes of `grid_posterior_field`.  Returns `out`."""
    for name, t in (("y", y), ("field_q", field_q), ("field_w", field_w), ("out['mean']", (out or {}).get("mean"))):
        if not _is_torch(t):
            raise ValueError(f"grid_posterior_wfield works in place on device tensors: {name} is not a torch tensor")
    n_vox, n_b = y.shape
    o, b, atoms, fv, lo, hi, lp = _mrf_host_inputs("grid_posterior_wfield", model, b, n_b, atoms, lo, hi, fixed_idx, fixed_vals, sigma, t1_mode,
                                                   tr, tm, log_prior)
    pr = _mrf_precision(precision, o.n_free)
    count = n_vox - int(first) if count is None else int(count)
    check(load().pnx_curvefit_grid_posterior_wfield_f64(C.byref(o), int(n_vox), ptr(b), ptr(y), int(atoms.shape[1]), ptr(atoms), ptr(fv), ptr(lo),
                                                        ptr(hi), int(bool(project_amplitude)), ptr(lp), float(noise_sd), int(first), count,
                                                        ptr(field_q), ptr(field_w), ptr(pr), ptr(out["mean"]), ptr(out.get("sd")),
                                                        ptr(out.get("map_atom")), ptr(out.get("map_p")), ptr(out.get("log_evidence")),
                                                        ptr(out.get("ess")), ptr(delta_max), MEM_DEVICE, int(device), stream))
    return out


def grid_posterior_tmrf(model, b, y, atoms, lo, hi, neighbours, colour_start, precision, dof, *, n_sweeps=4, tol=0.0, log_prior=None,
                        noise_sd=0.0, fixed_idx=(), fixed_vals=None, sigma=None, project_amplitude=False, t1_mode=0, tr=0., tm=0., device=0,
                        out=None, stream=None):
    """The grid posterior under the edge-preserving (Student-t) neighbourhood prior (pnx_curvefit_grid_posterior_tmrf_f64; method:
    include/pnx.h): `grid_posterior_mrf` with dof > 0, the degrees of freedom of the pair potential -- every
    neighbour enters with the weight (dof + K) / (dof + s_uv), small across an edge of the image; dof -> infinity is the Gaussian
    prior.  Returns the dict of `grid_posterior_mrf` with "field_w" (n_vox,) the weight sum and "field_n" (n_vox,) int32 the
    present neighbours of every voxel at its last update (0 where no sweep updated it)."""
    dev = _is_torch(y)
    if dev != _is_torch(neighbours):
        raise ValueError("y and neighbours must both be numpy arrays or both torch tensors")
    if not dev:
        _lib.require_device()
        y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
        neighbours = np.ascontiguousarray(neighbours, np.int32)
    n_vox, n_b = y.shape
    o, b, atoms, fv, lo, hi, lp = _mrf_host_inputs("grid_posterior_tmrf", model, b, n_b, atoms, lo, hi, fixed_idx, fixed_vals, sigma, t1_mode, tr,
                                                   tm, log_prior)
    n = o.n_free
    if neighbours.ndim != 2 or neighbours.shape[0] != n_vox:
        raise ValueError(f"neighbours must have shape ({n_vox}, n_nb), got {tuple(neighbours.shape)}")
    pr = _mrf_precision(precision, n)
    cs = np.ascontiguousarray(colour_start, np.int64)
    if cs.ndim != 1 or cs.size < 2:
        raise ValueError("colour_start must hold n_colours + 1 offsets")
    n_sweeps = int(n_sweeps)
    if dev:
        import torch

        mk = lambda key, shape, dt: (out or {}).get(key) if (out or {}).get(key) is not None else torch.empty(shape, dtype=dt, device=y.device)
        res = {key: mk(key, (n, n_vox), torch.float64) for key in ("mean", "sd", "map_p")}
        res["map_atom"], res["field_n"] = mk("map_atom", (n_vox,), torch.int32), mk("field_n", (n_vox,), torch.int32)
        for key in ("log_evidence", "ess", "field_w"):
            res[key] = mk(key, (n_vox,), torch.float64)
    else:
        res = {key: _out(out, key, (n, n_vox), np.float64) for key in ("mean", "sd", "map_p")}
        res["map_atom"], res["field_n"] = _out(out, "map_atom", (n_vox,), np.int32), _out(out, "field_n", (n_vox,), np.int32)
        for key in ("log_evidence", "ess", "field_w"):
            res[key] = _out(out, key, (n_vox,), np.float64)
    delta = np.full(min(max(n_sweeps, 0), GRID_MRF_MAX_SWEEPS), np.nan)  # outside 0..100 the library refuses before it writes
    done = C.c_int(0)
    check(load().pnx_curvefit_grid_posterior_tmrf_f64(C.byref(o), int(n_vox), ptr(b), ptr(y), int(atoms.shape[1]), ptr(atoms), ptr(fv), ptr(lo),
                                                      ptr(hi), int(bool(project_amplitude)), ptr(lp), float(noise_sd), int(neighbours.shape[1]),
                                                      ptr(neighbours), int(cs.size - 1), ptr(cs), ptr(pr), float(dof), n_sweeps, float(tol),
                                                      ptr(res["mean"]), ptr(res["sd"]), ptr(res["map_atom"]), ptr(res["map_p"]),
                                                      ptr(res["log_evidence"]), ptr(res["ess"]), ptr(res["field_w"]), ptr(res["field_n"]),
                                                      ptr(delta), C.byref(done), MEM_DEVICE if dev else MEM_HOST, int(device), stream))
    res["delta"], res["n_sweeps"] = delta, int(done.value)
    return res


GRID_MARGINAL_MAX_BINS = 128  # kGridMarginalMaxBins of csrc/pnx_grid_marginal_args.hpp
GRID_MARGINAL_MAX_PROBS = 8


def grid_marginal_bins(atoms, skip_rows=()):
    """The binning of `grid_marginals` derived from the atoms: per row k of atoms (n_free, n_atoms) np.unique(atoms[k],
    return_inverse=True) -- the ascending distinct values and the bin of every atom among them; a Cartesian grid need not be
    complete nor ordered.  skip_rows: rows without a marginal (n_bins = 0; the projected S0 row).  Returns (n_bins (n_free,) int32,
    bin_of (n_free, n_atoms) int32, bin_value (B,) float64)."""
    atoms = np.asarray(atoms, np.float64)
    if atoms.ndim != 2:
        raise ValueError("atoms must have shape (n_free, n_atoms)")
    n_bins = np.zeros(atoms.shape[0], np.int32)
    bin_of = np.zeros(atoms.shape, np.int32)
    values = []
    for k in range(atoms.shape[0]):
        if k in skip_rows:
            continue
        val, inv = np.unique(atoms[k], return_inverse=True)
        n_bins[k] = val.size
        bin_of[k] = inv.reshape(-1)
        values.append(val)
    return n_bins, bin_of, np.concatenate(values) if values else np.zeros(0)


def _marginal_bins(o, model, atoms, project_amplitude, bins):
    """(n_bins, bin_of, bin_value) as contiguous arrays of the ABI's types: the caller's, or derived from the atoms."""
    n = o.n_free
    if bins is None:
        skip = ()
        if project_amplitude and "S0" in MODEL_PARAM_NAMES[model]:
            pos = MODEL_PARAM_NAMES[model].index("S0")
            skip = tuple(k for k in range(n) if o.free_idx[k] == pos)
        bins = grid_marginal_bins(atoms, skip)
    n_bins, bin_of, bin_value = bins
    n_bins = np.ascontiguousarray(n_bins, np.int32)
    bin_of = np.ascontiguousarray(bin_of, np.int32)
    bin_value = np.ascontiguousarray(bin_value, np.float64)
    if n_bins.shape != (n,) or bin_of.shape != atoms.shape or (n_bins < 0).any() or bin_value.shape != (int(n_bins.sum()),):
        raise ValueError(f"bins must be (n_bins ({n},) >= 0, bin_of {atoms.shape}, bin_value (sum n_bins,))")
    return n_bins, bin_of, bin_value


def _marginal_probs(quantiles):
    return np.ascontiguousarray([] if quantiles is None else quantiles, np.float64).reshape(-1)


def _marginal_result(names, n_bins, bin_value, probs, marginal, quantile, log_evidence):
    """The flat (B, n_vox) and (n_q, n_free, n_vox) outputs split per parameter with a marginal, keyed by its position among the
    free parameters (or its name when `names` is given)."""
    off = np.concatenate([[0], np.cumsum(n_bins)])
    key = (lambda k: k) if names is None else (lambda k: names[k])
    rows = [k for k in range(len(n_bins)) if n_bins[k]]
    return dict(marginal={key(k): marginal[off[k]:off[k + 1]] for k in rows}, values={key(k): bin_value[off[k]:off[k + 1]] for k in rows},
                quantiles={} if quantile is None else {key(k): quantile[:, k] for k in rows}, quantile_probs=probs, log_evidence=log_evidence)


def grid_marginals(model, b, y, atoms, lo, hi, *, log_prior=None, noise_sd=0.0, bins=None, quantiles=(0.025, 0.5, 0.975), fixed_idx=(),
                   fixed_vals=None, sigma=None, project_amplitude=False, t1_mode=0, tr=0., tm=0., device=0):
    """Marginal posterior of every free parameter over a dictionary on host (numpy) arrays, and quantiles from it
    (pnx_curvefit_grid_marginals_f64; method: include/pnx.h).  The arguments of `grid_posterior`, and
    bins: None -- derived from the atoms by `grid_marginal_bins` (np.unique per parameter; no marginal for a projected S0) -- or
        (n_bins (n_free,), bin_of (n_free, n_atoms), bin_value (sum n_bins,)) as the ABI takes them; at most 128 bins in all;
    quantiles: up to 8 levels in the open interval (0, 1), or () / None for none.
    Returns dict(marginal {k: (n_bins_k, n_vox)}, values {k: (n_bins_k,)} the ascending grid values, quantiles {k: (n_q, n_vox)}
    -- the grid value of the first bin whose cumulative mass reaches the level, not interpolated --, keyed by the position k of the
    parameter among the free ones (parameters without a marginal are absent), quantile_probs (n_q,), log_evidence (n_vox,)).  A
    voxel with a non-finite signal holds NaN everywhere."""
    _lib.require_device()
    b = np.ascontiguousarray(b, np.float64)
    y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
    n_vox, n_b = y.shape
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    atoms, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (atoms, lo, hi))
    fv = None
    if len(fixed_idx):
        fv = np.ascontiguousarray(fixed_vals, np.float64)
        if fv.ndim != 1:
            raise ValueError("grid_marginals takes shared fixed values (n_fixed,): per-voxel fixed maps are not built")
    o = make_opts(model, n_b, fixed_idx, jac="analytic", t1_mode=t1_mode, tr=tr, tm=tm, sigma=sigma)
    n = o.n_free
    if atoms.ndim != 2 or atoms.shape[0] != n or lo.shape != (n,) or hi.shape != (n,):
        raise ValueError(f"atoms must have shape ({n}, n_atoms), lo / hi ({n},)")
    if fv is not None and fv.shape != (o.n_fixed,):
        raise ValueError("fixed_vals has the wrong shape")
    lp = _posterior_log_prior(log_prior, atoms.shape[1])
    n_bins, bin_of, bin_value = _marginal_bins(o, model, atoms, project_amplitude, bins)
    probs = _marginal_probs(quantiles)
    marginal = np.empty((int(n_bins.sum()), n_vox), np.float64)
    quantile = np.empty((probs.size, n, n_vox), np.float64)
    log_evidence = np.empty(n_vox, np.float64)
    check(load().pnx_curvefit_grid_marginals_f64(C.byref(o), n_vox, ptr(b), ptr(y), int(atoms.shape[1]), ptr(atoms), ptr(fv), ptr(lo), ptr(hi),
                                                 int(bool(project_amplitude)), ptr(lp), float(noise_sd), ptr(n_bins), ptr(bin_of),
                                                 ptr(bin_value), int(probs.size), ptr(probs) if probs.size else None, ptr(marginal),
                                                 ptr(quantile) if probs.size else None, ptr(log_evidence), MEM_HOST, int(device), None))
    return _marginal_result(None, n_bins, bin_value, probs, marginal, quantile, log_evidence)


def grid_marginals_device(opts, n_vox, b, y, atoms, fixed, lo, hi, project_amplitude, log_prior, noise_sd, n_bins, bin_of, bin_value, probs,
                          marginal, quantile, log_evidence, device, stream=None):
    """Enqueue the marginals on HBM-resident float64 torch tensors (asynchronous; caller synchronises): y (n_vox, n_b), marginal
    (sum n_bins, n_vox), quantile (n_q, n_free, n_vox) or None when probs is empty, log_evidence (n_vox,) or None on the device; b,
    atoms (n_free, n_atoms), shared fixed values, lo, hi, log_prior (n_atoms,) or None, the binning (`grid_marginal_bins`) and probs
    are host arrays.  `opts` from make_opts.  Returns the dict of `grid_marginals` over views of the caller's tensors."""
    b, atoms, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (b, atoms, lo, hi))
    if fixed is not None:
        fixed = np.ascontiguousarray(fixed, np.float64)
    if atoms.ndim != 2:
        raise ValueError("atoms must have shape (n_free, n_atoms)")
    lp = _posterior_log_prior(log_prior, atoms.shape[1])
    n_bins = np.ascontiguousarray(n_bins, np.int32)
    bin_of = np.ascontiguousarray(bin_of, np.int32)
    bin_value = np.ascontiguousarray(bin_value, np.float64)
    probs = _marginal_probs(probs)
    if n_bins.shape != (atoms.shape[0],) or bin_of.shape != atoms.shape or (n_bins < 0).any() or bin_value.shape != (int(n_bins.sum()),):
        raise ValueError(f"the binning must be n_bins ({atoms.shape[0]},) >= 0, bin_of {atoms.shape}, bin_value (sum n_bins,)")
    check(load().pnx_curvefit_grid_marginals_f64(C.byref(opts), int(n_vox), ptr(b), ptr(y), int(atoms.shape[1]), ptr(atoms), ptr(fixed), ptr(lo),
                                                 ptr(hi), int(bool(project_amplitude)), ptr(lp), float(noise_sd), ptr(n_bins), ptr(bin_of),
                                                 ptr(bin_value), int(probs.size), ptr(probs) if probs.size else None, ptr(marginal),
                                                 ptr(quantile) if probs.size else None, ptr(log_evidence), MEM_DEVICE, int(device), stream))
    return _marginal_result(None, n_bins, bin_value, probs, marginal, quantile if probs.size else None, log_evidence)


VARPRO_COMPARTMENTS = {"mono": 1, "bi_reduced": 2, "bi_s0": 2, "bi_full": 2, "tri_reduced": 3, "tri_s0": 3, "tri_full": 3}


def varpro_linear_names(model):
    """The linear parameters of a layout (fractions and S0), which pnx_curvefit_varpro_f64 solves in closed form."""
    return [n for n in MODEL_PARAM_NAMES[model] if not n.startswith("D")]


def varpro_slab_atoms(n_b, k):
    """Atoms per LDS slab of the variable-projection kernel (varpro_slab of csrc/pnx_varpro_args.hpp): the widest multiple of 16, at
    most 256, whose k blocks of dictionary rows ([n_b padded to 4][stride], stride = 16 mod 32) and k (k + 1) constants per atom
    fit 64 KB."""
    kpad, k, width = (int(n_b) + 3) & ~3, int(k), 16
    for w in range(16, 257, 16):
        if k * kpad * (w if w & 16 else w + 16) + k * (k + 1) * w <= 8192:
            width = w
    return width


def _varpro_args(model, n_b, nl_atoms, lo, hi, fallback, fixed_idx, fixed_vals, sigma, t1_mode, tr, tm):
    nl_atoms, lo, hi, fallback = (np.ascontiguousarray(a, np.float64) for a in (nl_atoms, lo, hi, fallback))
    fv = None
    if len(fixed_idx):
        fv = np.ascontiguousarray(fixed_vals, np.float64)
        if fv.ndim != 1:
            raise ValueError("varpro takes shared fixed values (n_fixed,): per-voxel fixed maps are not built")
    o = make_opts(model, n_b, fixed_idx, jac="analytic", t1_mode=t1_mode, tr=tr, tm=tm, sigma=sigma)
    n = o.n_free
    if nl_atoms.ndim != 2 or lo.shape != (n,) or hi.shape != (n,) or fallback.shape != (n,):
        raise ValueError(f"nl_atoms must have shape (n_nonlinear_free, n_atoms), lo / hi / fallback ({n},)")
    if fv is not None and fv.shape != (o.n_fixed,):
        raise ValueError("fixed_vals has the wrong shape")
    lin = {MODEL_PARAM_NAMES[model].index(name) for name in varpro_linear_names(model)}
    n_nl = sum(1 for k in range(n) if o.free_idx[k] not in lin)
    if nl_atoms.shape[0] != n_nl:
        raise ValueError(f"nl_atoms has {nl_atoms.shape[0]} rows, the model has {n_nl} free non-linear parameters (rates, T1)")
    return o, nl_atoms, lo, hi, fallback, fv


def varpro(model, b, y, nl_atoms, lo, hi, fallback, *, fixed_idx=(), fixed_vals=None, sigma=None, t1_mode=0, tr=0., tm=0., device=0,
           out=None):
    """Variable-projection dictionary fit on host (numpy) arrays (pnx_curvefit_varpro_f64; method: include/pnx.h): only the
    non-linear parameters are on the grid, the fractions and S0 of every voxel and atom come in closed form, clipped into lo / hi.

    nl_atoms (n_nonlinear_free, n_atoms <= 4096): the free rates (and T1) of every atom, one row per free non-linear parameter in
    the model's order; lo, hi, fallback (n_free,) for every free parameter; fixed_idx / fixed_vals (rates and T1 only) and sigma
    as `curvefit` takes them (shared values only).  Returns dict(params (n_free, n_vox) -- a per-voxel start for `curvefit` --,
    atom (n_vox,) int32 index of the chosen atom, -1 for a non-finite signal (whose params are `fallback`), cost (n_vox,)
    0.5 ||(y - model(params)) / sigma||^2, clipped (n_vox,) int8: a clip was active at the winner).
    `out`: optional dict of preallocated result arrays under the same keys."""
    _lib.require_device()
    b = np.ascontiguousarray(b, np.float64)
    y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
    n_vox, n_b = y.shape
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    o, nl_atoms, lo, hi, fallback, fv = _varpro_args(model, n_b, nl_atoms, lo, hi, fallback, fixed_idx, fixed_vals, sigma, t1_mode, tr, tm)
    res = dict(params=_out(out, "params", (o.n_free, n_vox), np.float64), atom=_out(out, "atom", (n_vox,), np.int32),
               cost=_out(out, "cost", (n_vox,), np.float64), clipped=_out(out, "clipped", (n_vox,), np.int8))
    check(load().pnx_curvefit_varpro_f64(C.byref(o), n_vox, ptr(b), ptr(y), int(nl_atoms.shape[1]), ptr(nl_atoms), ptr(fv), ptr(lo), ptr(hi),
                                         ptr(fallback), ptr(res["params"]), ptr(res["atom"]), ptr(res["cost"]), ptr(res["clipped"]),
                                         MEM_HOST, int(device), None))
    return res


def varpro_device(opts, n_vox, b, y, nl_atoms, fixed, lo, hi, fallback, params, atom, cost, clipped, device, stream=None):
    """Enqueue the variable-projection fit on HBM-resident float64 torch tensors (asynchronous; caller synchronises): y (n_vox, n_b),
    params (n_free, n_vox), atom (n_vox,) int32 or None, cost (n_vox,) or None, clipped (n_vox,) int8 or None on the device; b,
    nl_atoms (n_nonlinear_free, n_atoms), shared fixed values, lo, hi, fallback are host arrays.  `opts` from make_opts."""
    b, nl_atoms, lo, hi, fallback = (np.ascontiguousarray(a, np.float64) for a in (b, nl_atoms, lo, hi, fallback))
    if fixed is not None:
        fixed = np.ascontiguousarray(fixed, np.float64)
    if nl_atoms.ndim != 2:
        raise ValueError("nl_atoms must have shape (n_nonlinear_free, n_atoms)")
    check(load().pnx_curvefit_varpro_f64(C.byref(opts), int(n_vox), ptr(b), ptr(y), int(nl_atoms.shape[1]), ptr(nl_atoms), ptr(fixed), ptr(lo),
                                         ptr(hi), ptr(fallback), ptr(params), ptr(atom), ptr(cost), ptr(clipped), MEM_DEVICE, int(device),
                                         stream))


def varpro_posterior_slab_atoms(n_b, k):
    """Atoms per LDS slab of the variable-projection posterior kernel (varpro_posterior_slab of csrc/pnx_varpro_posterior_args.hpp):
    the variable projection's rule with k + 2 more values per atom (the log-weight and the k + 1 centred non-linear values)."""
    kpad, k, width = (int(n_b) + 3) & ~3, int(k), 16
    for w in range(16, 257, 16):
        if k * kpad * (w if w & 16 else w + 16) + (k * (k + 1) + k + 2) * w <= 8192:
            width = w
    return width


def varpro_posterior(model, b, y, nl_atoms, lo, hi, *, log_prior=None, noise_sd=0.0, marginal_amplitudes=True, fixed_idx=(), fixed_vals=None,
                     sigma=None, t1_mode=0, tr=0., tm=0., device=0, out=None):
    """Posterior of every voxel over a variable-projection dictionary on host (numpy) arrays (pnx_curvefit_varpro_posterior_f64;
    method: include/pnx.h): only the rates (and a free T1) are on the grid, the fractions and S0 of every voxel and atom are
    eliminated in closed form.  nl_atoms, lo, hi, fixed_idx / fixed_vals, sigma and the T1 factor as `varpro` takes them, and
    log_prior: None (uniform) or (n_atoms,) log prior weights, finite or -inf (an atom at -inf is excluded);
    noise_sd: > 0 a known Gaussian noise sd in the units of the (sigma-weighted) signal, 0 (default) marginalises the noise scale;
    marginal_amplitudes: True (default) weighs an atom by the marginal over its amplitudes (the Occam term -0.5 log det N; a
    Laplace-style approximation where a clip is active), False by the profile over them.
    Returns dict(mean, sd, map_p (n_free, n_vox), map_atom (n_vox,) int32 (-1 for a non-finite signal, whose floating outputs are
    NaN), log_evidence, ess, clipped_mass (n_vox,): the posterior share that rests on clipped amplitudes).  The sd of a fraction /
    S0 row is the between-atom spread only (a known understatement).  `out`: optional dict of preallocated result arrays.
    There is no `mem` keyword: as with `varpro` and `grid_posterior`, this function is the host-memory call (PNX_MEM_HOST, the
    chunk ring) and `varpro_posterior_device` the device-memory one (PNX_MEM_DEVICE, enqueue only)."""
    _lib.require_device()
    b = np.ascontiguousarray(b, np.float64)
    y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
    n_vox, n_b = y.shape
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    o, nl_atoms, lo, hi, _, fv = _varpro_args(model, n_b, nl_atoms, lo, hi, lo, fixed_idx, fixed_vals, sigma, t1_mode, tr, tm)
    lp = _posterior_log_prior(log_prior, nl_atoms.shape[1])
    n = o.n_free
    res = {key: _out(out, key, (n, n_vox), np.float64) for key in ("mean", "sd", "map_p")}
    res["map_atom"] = _out(out, "map_atom", (n_vox,), np.int32)
    for key in ("log_evidence", "ess", "clipped_mass"):
        res[key] = _out(out, key, (n_vox,), np.float64)
    check(load().pnx_curvefit_varpro_posterior_f64(C.byref(o), n_vox, ptr(b), ptr(y), int(nl_atoms.shape[1]), ptr(nl_atoms), ptr(fv), ptr(lo),
                                                   ptr(hi), ptr(lp), float(noise_sd), int(bool(marginal_amplitudes)), ptr(res["mean"]),
                                                   ptr(res["sd"]), ptr(res["map_atom"]), ptr(res["map_p"]), ptr(res["log_evidence"]),
                                                   ptr(res["ess"]), ptr(res["clipped_mass"]), MEM_HOST, int(device), None))
    return res


def varpro_posterior_device(opts, n_vox, b, y, nl_atoms, fixed, lo, hi, log_prior, noise_sd, marginal_amplitudes, mean, sd, map_atom, map_p,
                            log_evidence, ess, clipped_mass, device, stream=None):
    """Enqueue the variable-projection posterior on HBM-resident float64 torch tensors (asynchronous; caller synchronises):
    y (n_vox, n_b), mean / sd / map_p (n_free, n_vox), map_atom (n_vox,) int32, log_evidence / ess / clipped_mass (n_vox,) on the
    device, all but mean may be None; b, nl_atoms (n_nonlinear_free, n_atoms), shared fixed values, lo, hi and log_prior
    (n_atoms,) or None are host arrays.  `opts` from make_opts."""
    b, nl_atoms, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (b, nl_atoms, lo, hi))
    if fixed is not None:
        fixed = np.ascontiguousarray(fixed, np.float64)
    if nl_atoms.ndim != 2:
        raise ValueError("nl_atoms must have shape (n_nonlinear_free, n_atoms)")
    lp = _posterior_log_prior(log_prior, nl_atoms.shape[1])
    check(load().pnx_curvefit_varpro_posterior_f64(C.byref(opts), int(n_vox), ptr(b), ptr(y), int(nl_atoms.shape[1]), ptr(nl_atoms), ptr(fixed),
                                                   ptr(lo), ptr(hi), ptr(lp), float(noise_sd), int(bool(marginal_amplitudes)), ptr(mean), ptr(sd),
                                                   ptr(map_atom), ptr(map_p), ptr(log_evidence), ptr(ess), ptr(clipped_mass), MEM_DEVICE,
                                                   int(device), stream))


def varpro_mrf_slab_atoms(n_b, k):
    """Atoms per LDS slab of the variable-projection field posterior (varpro_mrf_slab of csrc/pnx_varpro_mrf_args.hpp): the
    posterior's rule with one more value per atom (r_g) and the 8 doubles of the delta reduction."""
    kpad, k, width = (int(n_b) + 3) & ~3, int(k), 16
    for w in range(16, 257, 16):
        if k * kpad * (w if w & 16 else w + 16) + (k * (k + 1) + k + 3) * w + 8 <= 8192:
            width = w
    return width


def varpro_mrf_centre(nl_atoms, nonlinear, log_prior=None):
    """The centres the variable-projection posterior accumulates its moments about (varpro_posterior_check_args), per free
    parameter: min + (max - min) / 2 of the row of nl_atoms over the admissible atoms where `nonlinear` (n_free,) bool is set (a
    rate, T1; the rows of nl_atoms in order), 0 for a fraction / S0 row.  What `grid_neighbour_field` takes as `centre` in front
    of `varpro_posterior_field`."""
    nl_atoms = np.asarray(nl_atoms, np.float64)
    nonlinear = np.asarray(nonlinear, bool)
    if int(nonlinear.sum()) != nl_atoms.shape[0]:
        raise ValueError(f"nonlinear marks {int(nonlinear.sum())} rows, nl_atoms has {nl_atoms.shape[0]}")
    adm = np.ones(nl_atoms.shape[1], bool) if log_prior is None else np.asarray(log_prior, np.float64) > -np.inf
    mn, mx = nl_atoms[:, adm].min(axis=1), nl_atoms[:, adm].max(axis=1)
    centre = np.zeros(nonlinear.size)
    centre[nonlinear] = mn + 0.5 * (mx - mn)
    return centre


def varpro_posterior_field(model, b, y, nl_atoms, lo, hi, field_q, field_n, precision, out, *, first=0, count=None, log_prior=None,
                           noise_sd=0.0, marginal_amplitudes=True, fixed_idx=(), fixed_vals=None, sigma=None, t1_mode=0, tr=0., tm=0.,
                           delta_max=None, device=0, stream=None):
    """One colour update of the neighbourhood prior over a variable-projection dictionary (pnx_curvefit_varpro_posterior_field_f64;
    method: include/pnx.h): the posterior of the voxels [first, first + count) with the field inside l_g, written in place into the
    full-length tensors of `out`.  Device only, asynchronous (the caller synchronises): y (n_vox, n_b), field_q (n_free, n_vox),
    field_n (n_vox,) int32 and out["mean"] (required, and read: delta compares against it), out["sd"], out["map_p"] (n_free,
    n_vox), out["map_atom"] (n_vox,) int32, out["log_evidence"], out["ess"], out["clipped_mass"] (n_vox,) are torch tensors on the
    device; delta_max: a one-element float64 device tensor or None.  The other arguments are `varpro_posterior`'s host arrays and
    precision (n_free,), 0 on every fraction / S0 row.  Returns `out`."""
    for name, t in (("y", y), ("field_q", field_q), ("field_n", field_n), ("out['mean']", (out or {}).get("mean"))):
        if not _is_torch(t):
            raise ValueError(f"varpro_posterior_field works in place on device tensors: {name} is not a torch tensor")
    n_vox, n_b = y.shape
    b = np.ascontiguousarray(b, np.float64)
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    o, nl_atoms, lo, hi, _, fv = _varpro_args(model, n_b, nl_atoms, lo, hi, lo, fixed_idx, fixed_vals, sigma, t1_mode, tr, tm)
    lp = _posterior_log_prior(log_prior, nl_atoms.shape[1])
    pr = _mrf_precision(precision, o.n_free)
    count = n_vox - int(first) if count is None else int(count)
    check(load().pnx_curvefit_varpro_posterior_field_f64(C.byref(o), int(n_vox), ptr(b), ptr(y), int(nl_atoms.shape[1]), ptr(nl_atoms), ptr(fv),
                                                         ptr(lo), ptr(hi), ptr(lp), float(noise_sd), int(bool(marginal_amplitudes)), int(first),
                                                         count, ptr(field_q), ptr(field_n), ptr(pr), ptr(out["mean"]), ptr(out.get("sd")),
                                                         ptr(out.get("map_atom")), ptr(out.get("map_p")), ptr(out.get("log_evidence")),
                                                         ptr(out.get("ess")), ptr(out.get("clipped_mass")), ptr(delta_max), MEM_DEVICE,
                                                         int(device), stream))
    return out


def varpro_posterior_mrf(model, b, y, nl_atoms, lo, hi, neighbours, colour_start, precision, *, n_sweeps=4, tol=0.0, log_prior=None,
                         noise_sd=0.0, marginal_amplitudes=True, fixed_idx=(), fixed_vals=None, sigma=None, t1_mode=0, tr=0., tm=0., device=0,
                         out=None, stream=None):
    """The variable-projection posterior under a neighbourhood (MRF) prior on its rates (and a free T1) by coloured mean-field
    sweeps (pnx_curvefit_varpro_posterior_mrf_f64; method: include/pnx.h).  The arguments of `varpro_posterior`, and neighbours,
    colour_start, n_sweeps and tol as `grid_posterior_mrf` takes them; precision (n_free,) >= 0, 0 on every fraction / S0 row.
    y and neighbours are numpy arrays (staged once) or torch tensors on the device (read in place; `out` may hold preallocated
    result tensors); the call synchronises either way.  Returns the dict of `varpro_posterior` -- log_evidence is the local
    normaliser of the last update, not a model evidence -- with "delta" (n_sweeps,) the largest relative move of a mean per sweep,
    NaN past "n_sweeps", the sweeps done."""
    dev = _is_torch(y)
    if dev != _is_torch(neighbours):
        raise ValueError("y and neighbours must both be numpy arrays or both torch tensors")
    if not dev:
        _lib.require_device()
        y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
        neighbours = np.ascontiguousarray(neighbours, np.int32)
    n_vox, n_b = y.shape
    b = np.ascontiguousarray(b, np.float64)
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    o, nl_atoms, lo, hi, _, fv = _varpro_args(model, n_b, nl_atoms, lo, hi, lo, fixed_idx, fixed_vals, sigma, t1_mode, tr, tm)
    lp = _posterior_log_prior(log_prior, nl_atoms.shape[1])
    n = o.n_free
    if neighbours.ndim != 2 or neighbours.shape[0] != n_vox:
        raise ValueError(f"neighbours must have shape ({n_vox}, n_nb), got {tuple(neighbours.shape)}")
    pr = _mrf_precision(precision, n)
    cs = np.ascontiguousarray(colour_start, np.int64)
    if cs.ndim != 1 or cs.size < 2:
        raise ValueError("colour_start must hold n_colours + 1 offsets")
    n_sweeps = int(n_sweeps)
    if dev:
        import torch

        mk = lambda key, shape, dt: (out or {}).get(key) if (out or {}).get(key) is not None else torch.empty(shape, dtype=dt, device=y.device)
        res = {key: mk(key, (n, n_vox), torch.float64) for key in ("mean", "sd", "map_p")}
        res["map_atom"] = mk("map_atom", (n_vox,), torch.int32)
        for key in ("log_evidence", "ess", "clipped_mass"):
            res[key] = mk(key, (n_vox,), torch.float64)
    else:
        res = {key: _out(out, key, (n, n_vox), np.float64) for key in ("mean", "sd", "map_p")}
        res["map_atom"] = _out(out, "map_atom", (n_vox,), np.int32)
        for key in ("log_evidence", "ess", "clipped_mass"):
            res[key] = _out(out, key, (n_vox,), np.float64)
    delta = np.full(min(max(n_sweeps, 0), GRID_MRF_MAX_SWEEPS), np.nan)  # outside 0..100 the library refuses before it writes
    done = C.c_int(0)
    check(load().pnx_curvefit_varpro_posterior_mrf_f64(C.byref(o), int(n_vox), ptr(b), ptr(y), int(nl_atoms.shape[1]), ptr(nl_atoms), ptr(fv),
                                                       ptr(lo), ptr(hi), ptr(lp), float(noise_sd), int(bool(marginal_amplitudes)),
                                                       int(neighbours.shape[1]), ptr(neighbours), int(cs.size - 1), ptr(cs), ptr(pr), n_sweeps,
                                                       float(tol), ptr(res["mean"]), ptr(res["sd"]), ptr(res["map_atom"]), ptr(res["map_p"]),
                                                       ptr(res["log_evidence"]), ptr(res["ess"]), ptr(res["clipped_mass"]), ptr(delta),
                                                       C.byref(done), MEM_DEVICE if dev else MEM_HOST, int(device), stream))
    res["delta"], res["n_sweeps"] = delta, int(done.value)
    return res


def varpro_logmrf_slab_atoms(n_b, k):
    """Atoms per LDS slab of the log-field posterior (varpro_logmrf_slab of csrc/pnx_varpro_logmrf_args.hpp): `varpro_mrf_slab_atoms`'s
    rule with k + 1 more values per atom, the centred field rows beside the centred moment rows."""
    kpad, k, width = (int(n_b) + 3) & ~3, int(k), 16
    for w in range(16, 257, 16):
        if k * kpad * (w if w & 16 else w + 16) + (k * (k + 1) + 2 * k + 4) * w + 8 <= 8192:
            width = w
    return width


def _logmrf_coupling(coupling, n_free):
    c = np.ascontiguousarray(coupling, np.int32).reshape(-1)
    if c.shape != (n_free,):
        raise ValueError(f"coupling has {c.size} entries for {n_free} free parameters (0: linear, 1: log)")
    return c


def varpro_logmrf_centre(nl_atoms, nonlinear, coupling, log_prior=None):
    """(fcentre, frange), each (n_free,): min + (max - min) / 2 and max - min of f over the admissible atoms, f = the row of
    nl_atoms where coupling is 0 and its logarithm where it is 1; 0 for a fraction / S0 row.  fcentre is what
    `grid_neighbour_field` takes as `centre` in front of `varpro_posterior_logfield`; strength / frange^2 is the solver's precision."""
    nl_atoms = np.asarray(nl_atoms, np.float64)
    nonlinear = np.asarray(nonlinear, bool)
    coupling = _logmrf_coupling(coupling, nonlinear.size)
    if int(nonlinear.sum()) != nl_atoms.shape[0]:
        raise ValueError(f"nonlinear marks {int(nonlinear.sum())} rows, nl_atoms has {nl_atoms.shape[0]}")
    if (coupling[~nonlinear] != 0).any():
        raise ValueError("coupling must be 0 on a fraction / S0 row")
    adm = np.ones(nl_atoms.shape[1], bool) if log_prior is None else np.asarray(log_prior, np.float64) > -np.inf
    centre, rng = np.zeros(nonlinear.size), np.zeros(nonlinear.size)
    for j, k in enumerate(np.flatnonzero(nonlinear)):
        f = nl_atoms[j, adm]
        if coupling[k]:
            if not (f > 0).all():
                raise ValueError(f"coupling[{k}]=1 (log) needs positive values on row {j} of nl_atoms")
            f = np.log(f)
        centre[k], rng[k] = f.min() + 0.5 * (f.max() - f.min()), f.max() - f.min()
    return centre, rng


def varpro_posterior_logfield(model, b, y, nl_atoms, lo, hi, field_q, field_n, precision, coupling, out, *, first=0, count=None,
                              log_prior=None, noise_sd=0.0, marginal_amplitudes=True, fixed_idx=(), fixed_vals=None, sigma=None, t1_mode=0,
                              tr=0., tm=0., delta_max=None, device=0, stream=None):
    """One colour update of the neighbourhood prior with a per-row linear (0) or log (1) coupling
    (pnx_curvefit_varpro_posterior_logfield_f64; method: include/pnx.h).  `varpro_posterior_field`'s arguments, coupling (n_free,)
    and one more required device tensor out["field_mean"] (n_free, n_vox): the mean of f under the weights behind out["mean"],
    read (delta compares against it) and written in place.  Returns `out`."""
    for name, t in (("y", y), ("field_q", field_q), ("field_n", field_n), ("out['mean']", (out or {}).get("mean")),
                    ("out['field_mean']", (out or {}).get("field_mean"))):
        if not _is_torch(t):
            raise ValueError(f"varpro_posterior_logfield works in place on device tensors: {name} is not a torch tensor")
    n_vox, n_b = y.shape
    b = np.ascontiguousarray(b, np.float64)
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    o, nl_atoms, lo, hi, _, fv = _varpro_args(model, n_b, nl_atoms, lo, hi, lo, fixed_idx, fixed_vals, sigma, t1_mode, tr, tm)
    lp = _posterior_log_prior(log_prior, nl_atoms.shape[1])
    pr = _mrf_precision(precision, o.n_free)
    cp = _logmrf_coupling(coupling, o.n_free)
    count = n_vox - int(first) if count is None else int(count)
    check(load().pnx_curvefit_varpro_posterior_logfield_f64(C.byref(o), int(n_vox), ptr(b), ptr(y), int(nl_atoms.shape[1]), ptr(nl_atoms),
                                                            ptr(fv), ptr(lo), ptr(hi), ptr(lp), float(noise_sd), int(bool(marginal_amplitudes)),
                                                            int(first), count, ptr(field_q), ptr(field_n), ptr(pr), ptr(cp), ptr(out["mean"]),
                                                            ptr(out.get("sd")), ptr(out.get("map_atom")), ptr(out.get("map_p")),
                                                            ptr(out.get("log_evidence")), ptr(out.get("ess")), ptr(out.get("clipped_mass")),
                                                            ptr(out["field_mean"]), ptr(delta_max), MEM_DEVICE, int(device), stream))
    return out


def varpro_posterior_logmrf(model, b, y, nl_atoms, lo, hi, neighbours, colour_start, precision, coupling, *, n_sweeps=4, tol=0.0,
                            log_prior=None, noise_sd=0.0, marginal_amplitudes=True, fixed_idx=(), fixed_vals=None, sigma=None, t1_mode=0,
                            tr=0., tm=0., device=0, out=None, stream=None):
    """`varpro_posterior_mrf` with a per-row linear (0) or log (1) coupling (pnx_curvefit_varpro_posterior_logmrf_f64; method:
    include/pnx.h): coupling (n_free,), 0 on every fraction / S0 row and where precision is 0.  Returns `varpro_posterior_mrf`'s dict
    with "field_mean" (n_free, n_vox): the mean of log theta on a log row, the bytes of "mean" on every other row."""
    dev = _is_torch(y)
    if dev != _is_torch(neighbours):
        raise ValueError("y and neighbours must both be numpy arrays or both torch tensors")
    if not dev:
        _lib.require_device()
        y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
        neighbours = np.ascontiguousarray(neighbours, np.int32)
    n_vox, n_b = y.shape
    b = np.ascontiguousarray(b, np.float64)
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    o, nl_atoms, lo, hi, _, fv = _varpro_args(model, n_b, nl_atoms, lo, hi, lo, fixed_idx, fixed_vals, sigma, t1_mode, tr, tm)
    lp = _posterior_log_prior(log_prior, nl_atoms.shape[1])
    n = o.n_free
    if neighbours.ndim != 2 or neighbours.shape[0] != n_vox:
        raise ValueError(f"neighbours must have shape ({n_vox}, n_nb), got {tuple(neighbours.shape)}")
    pr = _mrf_precision(precision, n)
    cp = _logmrf_coupling(coupling, n)
    cs = np.ascontiguousarray(colour_start, np.int64)
    if cs.ndim != 1 or cs.size < 2:
        raise ValueError("colour_start must hold n_colours + 1 offsets")
    n_sweeps = int(n_sweeps)
    if dev:
        import torch

        mk = lambda key, shape, dt: (out or {}).get(key) if (out or {}).get(key) is not None else torch.empty(shape, dtype=dt, device=y.device)
        res = {key: mk(key, (n, n_vox), torch.float64) for key in ("mean", "sd", "map_p", "field_mean")}
        res["map_atom"] = mk("map_atom", (n_vox,), torch.int32)
        for key in ("log_evidence", "ess", "clipped_mass"):
            res[key] = mk(key, (n_vox,), torch.float64)
    else:
        res = {key: _out(out, key, (n, n_vox), np.float64) for key in ("mean", "sd", "map_p", "field_mean")}
        res["map_atom"] = _out(out, "map_atom", (n_vox,), np.int32)
        for key in ("log_evidence", "ess", "clipped_mass"):
            res[key] = _out(out, key, (n_vox,), np.float64)
    delta = np.full(min(max(n_sweeps, 0), GRID_MRF_MAX_SWEEPS), np.nan)  # outside 0..100 the library refuses before it writes
    done = C.c_int(0)
    check(load().pnx_curvefit_varpro_posterior_logmrf_f64(C.byref(o), int(n_vox), ptr(b), ptr(y), int(nl_atoms.shape[1]), ptr(nl_atoms), ptr(fv),
                                                          ptr(lo), ptr(hi), ptr(lp), float(noise_sd), int(bool(marginal_amplitudes)),
                                                          int(neighbours.shape[1]), ptr(neighbours), int(cs.size - 1), ptr(cs), ptr(pr), ptr(cp),
                                                          n_sweeps, float(tol), ptr(res["mean"]), ptr(res["sd"]), ptr(res["map_atom"]),
                                                          ptr(res["map_p"]), ptr(res["log_evidence"]), ptr(res["ess"]), ptr(res["clipped_mass"]),
                                                          ptr(res["field_mean"]), ptr(delta), C.byref(done), MEM_DEVICE if dev else MEM_HOST,
                                                          int(device), stream))
    res["delta"], res["n_sweeps"] = delta, int(done.value)
    return res


def varpro_prior_slab_atoms(n_b, k):
    """Atoms per LDS slab of the two EM passes over the variable-projection dictionary (varpro_prior_slab of
    csrc/pnx_varpro_prior_args.hpp): the variable projection's rule with 5 more values per atom -- the log-weight and the four
    wave-private rows of the accumulate pass, which take the place of the posterior's k + 1 centred non-linear values.  Equal to
    `varpro_posterior_slab_atoms` at three compartments, at most as wide below (80 against 96 at two compartments and 32 b-values)."""
    kpad, k, width = (int(n_b) + 3) & ~3, int(k), 16
    for w in range(16, 257, 16):
        if k * kpad * (w if w & 16 else w + 16) + (k * (k + 1) + 5) * w <= 8192:
            width = w
    return width


def _varpro_prior_em_call(o, n_vox, b, y, nl_atoms, fv, lo, hi, lp, noise_sd, marginal_amplitudes, n_iter, pseudo_count, rel_tol, mem, device,
                          stream):
    n_iter = int(n_iter)
    out = np.empty(nl_atoms.shape[1], np.float64)
    loglik = np.full(min(max(n_iter, 0), 1000) + 1, np.nan)  # outside 1..1000 the library refuses before it writes
    done, n_eff = C.c_int(0), C.c_int64(0)
    check(load().pnx_curvefit_varpro_prior_em_f64(C.byref(o), int(n_vox), ptr(b), ptr(y), int(nl_atoms.shape[1]), ptr(nl_atoms), ptr(fv), ptr(lo),
                                                  ptr(hi), ptr(lp), float(noise_sd), int(bool(marginal_amplitudes)), n_iter,
                                                  float(pseudo_count), float(rel_tol), ptr(out), ptr(loglik), C.byref(done), C.byref(n_eff),
                                                  mem, int(device), stream))
    return dict(log_prior=out, loglik=loglik, n_iter=int(done.value), n_eff=int(n_eff.value))


def varpro_prior_em(model, b, y, nl_atoms, lo, hi, *, log_prior=None, noise_sd=0.0, marginal_amplitudes=True, n_iter=20, pseudo_count=0.0,
                    rel_tol=1e-6, fixed_idx=(), fixed_vals=None, sigma=None, t1_mode=0, tr=0., tm=0., device=0):
    """The prior of `varpro_posterior` learned from the voxels themselves on host (numpy) arrays (pnx_curvefit_varpro_prior_em_f64;
    method: include/pnx.h): the maximum-likelihood mixture over the rate atoms by EM, pi_g <- mean over the voxels that take part
    of their posterior weight on atom g.  The Occam term of `marginal_amplitudes` belongs to the likelihood, not to the learned
    table.  The arguments of `varpro_posterior` (log_prior is the start: None is uniform, an atom at -inf stays excluded, as does
    an atom the variable projection cannot solve under marginal_amplitudes), and n_iter, pseudo_count, rel_tol as `grid_prior_em`
    takes them.  Returns `grid_prior_em`'s dict: log_prior (n_atoms,) -- ready for `varpro_posterior(..., log_prior=...)` --,
    loglik (n_iter + 1,), NaN past n_iter, n_iter the updates done, n_eff the voxels that took part.  The prior needs many voxels:
    a few dozen over-fit."""
    _lib.require_device()
    b = np.ascontiguousarray(b, np.float64)
    y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
    n_vox, n_b = y.shape
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    o, nl_atoms, lo, hi, _, fv = _varpro_args(model, n_b, nl_atoms, lo, hi, lo, fixed_idx, fixed_vals, sigma, t1_mode, tr, tm)
    lp = _posterior_log_prior(log_prior, nl_atoms.shape[1])
    return _varpro_prior_em_call(o, n_vox, b, y, nl_atoms, fv, lo, hi, lp, noise_sd, marginal_amplitudes, n_iter, pseudo_count, rel_tol, MEM_HOST,
                                 device, None)


def varpro_prior_em_device(opts, n_vox, b, y, nl_atoms, fixed, lo, hi, log_prior, noise_sd, marginal_amplitudes, n_iter, pseudo_count, rel_tol,
                           device, stream=None):
    """`varpro_prior_em` on an HBM-resident float64 torch tensor y (n_vox, n_b), read in place; b, nl_atoms (n_nonlinear_free,
    n_atoms), shared fixed values, lo, hi and log_prior (n_atoms,) or None are host arrays, `opts` from make_opts.  The results are
    small host arrays, so unlike `varpro_posterior_device` the call synchronises `stream` before it returns the same dict."""
    b, nl_atoms, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (b, nl_atoms, lo, hi))
    if fixed is not None:
        fixed = np.ascontiguousarray(fixed, np.float64)
    if nl_atoms.ndim != 2:
        raise ValueError("nl_atoms must have shape (n_nonlinear_free, n_atoms)")
    lp = _posterior_log_prior(log_prior, nl_atoms.shape[1])
    return _varpro_prior_em_call(opts, n_vox, b, y, nl_atoms, fixed, lo, hi, lp, noise_sd, marginal_amplitudes, n_iter, pseudo_count, rel_tol,
                                 MEM_DEVICE, device, stream)


def varpro_class_slab_atoms(n_b, k, n_classes, extra):
    """Atoms per LDS slab of the per-label kernels over the variable-projection dictionary (varpro_class_slab of
    csrc/pnx_varpro_class_args.hpp): the variable projection's rule with n_classes + extra more values per atom -- the rows of
    log-weights and, as extra, the posterior's k + 1 centred non-linear values or the 4 n_classes wave-private rows of both EM
    passes.  At one class these are `varpro_posterior_slab_atoms` and `varpro_prior_slab_atoms`."""
    kpad, k, width = (int(n_b) + 3) & ~3, int(k), 16
    for w in range(16, 257, 16):
        if k * kpad * (w if w & 16 else w + 16) + (k * (k + 1) + int(n_classes) + int(extra)) * w <= 8192:
            width = w
    return width


def _varpro_class_host_inputs(model, b, y, nl_atoms, lo, hi, labels, fixed_idx, fixed_vals, sigma, t1_mode, tr, tm):
    b = np.ascontiguousarray(b, np.float64)
    y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
    n_vox, n_b = y.shape
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    o, nl_atoms, lo, hi, _, fv = _varpro_args(model, n_b, nl_atoms, lo, hi, lo, fixed_idx, fixed_vals, sigma, t1_mode, tr, tm)
    return o, n_vox, b, y, nl_atoms, fv, lo, hi, _class_labels(labels, n_vox)


def varpro_posterior_classes(model, b, y, nl_atoms, lo, hi, labels, n_classes, *, log_prior=None, noise_sd=0.0, marginal_amplitudes=True,
                             fixed_idx=(), fixed_vals=None, sigma=None, t1_mode=0, tr=0., tm=0., device=0, out=None):
    """`varpro_posterior` with one prior row per segmentation label on host (numpy) arrays
    (pnx_curvefit_varpro_posterior_classes_f64; method: include/pnx.h).  The arguments of `varpro_posterior`, and
    labels (n_vox,) integers: the row of the table each voxel is judged under; a label outside [0, n_classes) -- background, -1 by
        convention -- gives the voxel NaN outputs and map_atom -1, as a non-finite signal does;
    n_classes: 1..16;  log_prior: None (every row uniform) or (n_classes, n_atoms), finite or -inf, every row with a finite entry.
    Returns the dict of `varpro_posterior`."""
    _lib.require_device()
    o, n_vox, b, y, nl_atoms, fv, lo, hi, lab = _varpro_class_host_inputs(model, b, y, nl_atoms, lo, hi, labels, fixed_idx, fixed_vals, sigma,
                                                                          t1_mode, tr, tm)
    n = o.n_free
    lp = _class_table(log_prior, n_classes, nl_atoms.shape[1])
    res = {key: _out(out, key, (n, n_vox), np.float64) for key in ("mean", "sd", "map_p")}
    res["map_atom"] = _out(out, "map_atom", (n_vox,), np.int32)
    for key in ("log_evidence", "ess", "clipped_mass"):
        res[key] = _out(out, key, (n_vox,), np.float64)
    check(load().pnx_curvefit_varpro_posterior_classes_f64(C.byref(o), n_vox, ptr(b), ptr(y), int(nl_atoms.shape[1]), ptr(nl_atoms), ptr(fv),
                                                           ptr(lo), ptr(hi), int(n_classes), ptr(lab), ptr(lp), float(noise_sd),
                                                           int(bool(marginal_amplitudes)), ptr(res["mean"]), ptr(res["sd"]),
                                                           ptr(res["map_atom"]), ptr(res["map_p"]), ptr(res["log_evidence"]), ptr(res["ess"]),
                                                           ptr(res["clipped_mass"]), MEM_HOST, int(device), None))
    return res


def varpro_posterior_classes_device(opts, n_vox, b, y, nl_atoms, fixed, lo, hi, labels, n_classes, log_prior, noise_sd, marginal_amplitudes,
                                    mean, sd, map_atom, map_p, log_evidence, ess, clipped_mass, device, stream=None):
    """Enqueue `varpro_posterior_classes` on HBM-resident torch tensors (asynchronous; caller synchronises): the tensors of
    `varpro_posterior_device` and labels (n_vox,) int32 on the device; log_prior (n_classes, n_atoms) or None is a host array."""
    b, nl_atoms, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (b, nl_atoms, lo, hi))
    if fixed is not None:
        fixed = np.ascontiguousarray(fixed, np.float64)
    if nl_atoms.ndim != 2:
        raise ValueError("nl_atoms must have shape (n_nonlinear_free, n_atoms)")
    lp = _class_table(log_prior, n_classes, nl_atoms.shape[1])
    check(load().pnx_curvefit_varpro_posterior_classes_f64(C.byref(opts), int(n_vox), ptr(b), ptr(y), int(nl_atoms.shape[1]), ptr(nl_atoms),
                                                           ptr(fixed), ptr(lo), ptr(hi), int(n_classes), ptr(labels), ptr(lp), float(noise_sd),
                                                           int(bool(marginal_amplitudes)), ptr(mean), ptr(sd), ptr(map_atom), ptr(map_p),
                                                           ptr(log_evidence), ptr(ess), ptr(clipped_mass), MEM_DEVICE, int(device), stream))


def _varpro_prior_em_classes_call(o, n_vox, b, y, nl_atoms, fv, lo, hi, labels, n_classes, lp, noise_sd, marginal_amplitudes, n_iter,
                                  pseudo_count, rel_tol, mem, device, stream):
    n_iter, n_classes = int(n_iter), int(n_classes)
    out = np.empty((n_classes, nl_atoms.shape[1]), np.float64)
    n_t = min(max(n_iter, 0), 1000) + 1  # outside 1..1000 the library refuses before it writes
    loglik, loglik_class = np.full(n_t, np.nan), np.full((n_t, n_classes), np.nan)
    done, n_eff = C.c_int(0), np.zeros(n_classes, np.int64)
    check(load().pnx_curvefit_varpro_prior_em_classes_f64(C.byref(o), int(n_vox), ptr(b), ptr(y), int(nl_atoms.shape[1]), ptr(nl_atoms), ptr(fv),
                                                          ptr(lo), ptr(hi), n_classes, ptr(labels), ptr(lp), float(noise_sd),
                                                          int(bool(marginal_amplitudes)), n_iter, float(pseudo_count), float(rel_tol),
                                                          ptr(out), ptr(loglik), ptr(loglik_class), C.byref(done), ptr(n_eff), mem,
                                                          int(device), stream))
    return dict(log_prior=out, loglik=loglik, loglik_class=loglik_class, n_iter=int(done.value), n_eff=n_eff)


def varpro_prior_em_classes(model, b, y, nl_atoms, lo, hi, labels, n_classes, *, log_prior=None, noise_sd=0.0, marginal_amplitudes=True,
                            n_iter=20, pseudo_count=0.0, rel_tol=1e-6, fixed_idx=(), fixed_vals=None, sigma=None, t1_mode=0, tr=0., tm=0.,
                            device=0):
    """`varpro_prior_em` with one prior row per segmentation label, every row learned from its own voxels in one pass pair over the
    volume (pnx_curvefit_varpro_prior_em_classes_f64; method: include/pnx.h).  The arguments of `varpro_prior_em`, labels and
    n_classes as `varpro_posterior_classes` takes them (a label outside [0, n_classes) takes no part), log_prior None or
    (n_classes, n_atoms): the start.  Returns `grid_prior_em_classes`' dict: log_prior (n_classes, n_atoms) every row normalised --
    ready for `varpro_posterior_classes` --, loglik (n_iter + 1,) the sum over the classes, loglik_class (n_iter + 1, n_classes),
    n_iter the updates done, n_eff (n_classes,) the voxels of each class that took part; a class without one keeps its normalised
    start row."""
    _lib.require_device()
    o, n_vox, b, y, nl_atoms, fv, lo, hi, lab = _varpro_class_host_inputs(model, b, y, nl_atoms, lo, hi, labels, fixed_idx, fixed_vals, sigma,
                                                                          t1_mode, tr, tm)
    lp = _class_table(log_prior, n_classes, nl_atoms.shape[1])
    return _varpro_prior_em_classes_call(o, n_vox, b, y, nl_atoms, fv, lo, hi, lab, n_classes, lp, noise_sd, marginal_amplitudes, n_iter,
                                         pseudo_count, rel_tol, MEM_HOST, device, None)


def varpro_prior_em_classes_device(opts, n_vox, b, y, nl_atoms, fixed, lo, hi, labels, n_classes, log_prior, noise_sd, marginal_amplitudes,
                                   n_iter, pseudo_count, rel_tol, device, stream=None):
    """`varpro_prior_em_classes` on HBM-resident torch tensors y (n_vox, n_b) float64 and labels (n_vox,) int32, read in place; the
    other arguments are host arrays, `opts` from make_opts.  Synchronises `stream` before it returns the same dict."""
    b, nl_atoms, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (b, nl_atoms, lo, hi))
    if fixed is not None:
        fixed = np.ascontiguousarray(fixed, np.float64)
    if nl_atoms.ndim != 2:
        raise ValueError("nl_atoms must have shape (n_nonlinear_free, n_atoms)")
    lp = _class_table(log_prior, n_classes, nl_atoms.shape[1])
    return _varpro_prior_em_classes_call(opts, n_vox, b, y, nl_atoms, fixed, lo, hi, labels, n_classes, lp, noise_sd, marginal_amplitudes,
                                         n_iter, pseudo_count, rel_tol, MEM_DEVICE, device, stream)


def _varpro_marginal_bins(o, model, nl_atoms, bins):
    """(n_bins, bin_of, bin_value) of `varpro_marginals` over ALL free parameters, as contiguous arrays of the ABI's types.  bins:
    None -- `grid_marginal_bins(nl_atoms)`, one entry per row of nl_atoms, spread over the free parameters (a fraction or S0 holds
    n_bins = 0 and a row of zeros in bin_of) -- or the caller's (n_bins (n_free,), bin_of (n_free, n_atoms), bin_value)."""
    n, G = o.n_free, nl_atoms.shape[1]
    if bins is None:
        lin = {MODEL_PARAM_NAMES[model].index(name) for name in varpro_linear_names(model)}
        rows = [k for k in range(n) if o.free_idx[k] not in lin]  # free parameter of every row of nl_atoms
        nb, of, bin_value = grid_marginal_bins(nl_atoms)
        n_bins, bin_of = np.zeros(n, np.int32), np.zeros((n, G), np.int32)
        n_bins[rows], bin_of[rows] = nb, of
        bins = (n_bins, bin_of, bin_value)
    n_bins, bin_of, bin_value = bins
    n_bins = np.ascontiguousarray(n_bins, np.int32)
    bin_of = np.ascontiguousarray(bin_of, np.int32)
    bin_value = np.ascontiguousarray(bin_value, np.float64)
    if n_bins.shape != (n,) or bin_of.shape != (n, G) or (n_bins < 0).any() or bin_value.shape != (int(n_bins.sum()),):
        raise ValueError(f"bins must be (n_bins ({n},) >= 0, bin_of ({n}, {G}), bin_value (sum n_bins,))")
    return n_bins, bin_of, bin_value


def _varpro_marginal_result(n_bins, bin_value, probs, marginal, quantile, geo_mean, log_evidence):
    res = _marginal_result(None, n_bins, bin_value, probs, marginal, quantile, log_evidence)
    res["geo_mean"] = {k: geo_mean[k] for k in range(len(n_bins)) if n_bins[k]}
    return res


def varpro_marginals(model, b, y, nl_atoms, lo, hi, *, log_prior=None, noise_sd=0.0, marginal_amplitudes=True, bins=None,
                     quantiles=(0.025, 0.5, 0.975), fixed_idx=(), fixed_vals=None, sigma=None, t1_mode=0, tr=0., tm=0., device=0):
    """Marginal posterior of every free rate (and a free T1) over a variable-projection dictionary on host (numpy) arrays, quantiles
    and a geometric posterior mean from it (pnx_curvefit_varpro_marginals_f64; method: include/pnx.h).  The arguments of
    `varpro_posterior`, and
    bins: None -- derived from the atoms by `grid_marginal_bins(nl_atoms)` (np.unique per row; a fraction or S0 has no marginal: its
        value belongs to the voxel-atom pair) -- or (n_bins (n_free,), bin_of (n_free, n_atoms), bin_value (sum n_bins,)) as the
        ABI takes them, n_bins = 0 for every fraction and S0; at most 128 bins in all;
    quantiles: up to 8 levels in the open interval (0, 1), or () / None for none.
    Returns the dict of `grid_marginals` -- marginal {k: (n_bins_k, n_vox)}, values {k: (n_bins_k,)}, quantiles {k: (n_q, n_vox)},
    keyed by the position k of the parameter among the free ones, quantile_probs, log_evidence (n_vox,) -- plus geo_mean
    {k: (n_vox,)}: exp of the posterior mean of log(parameter k), NaN where a grid value is <= 0.  A voxel with a non-finite signal
    holds NaN everywhere."""
    _lib.require_device()
    b = np.ascontiguousarray(b, np.float64)
    y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
    n_vox, n_b = y.shape
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    o, nl_atoms, lo, hi, _, fv = _varpro_args(model, n_b, nl_atoms, lo, hi, lo, fixed_idx, fixed_vals, sigma, t1_mode, tr, tm)
    lp = _posterior_log_prior(log_prior, nl_atoms.shape[1])
    n = o.n_free
    n_bins, bin_of, bin_value = _varpro_marginal_bins(o, model, nl_atoms, bins)
    probs = _marginal_probs(quantiles)
    marginal = np.empty((int(n_bins.sum()), n_vox), np.float64)
    quantile = np.empty((probs.size, n, n_vox), np.float64)
    geo_mean = np.empty((n, n_vox), np.float64)
    log_evidence = np.empty(n_vox, np.float64)
    check(load().pnx_curvefit_varpro_marginals_f64(C.byref(o), n_vox, ptr(b), ptr(y), int(nl_atoms.shape[1]), ptr(nl_atoms), ptr(fv), ptr(lo),
                                                   ptr(hi), ptr(lp), float(noise_sd), int(bool(marginal_amplitudes)), ptr(n_bins), ptr(bin_of),
                                                   ptr(bin_value), int(probs.size), ptr(probs) if probs.size else None, ptr(marginal),
                                                   ptr(quantile) if probs.size else None, ptr(geo_mean), ptr(log_evidence), MEM_HOST,
                                                   int(device), None))
    return _varpro_marginal_result(n_bins, bin_value, probs, marginal, quantile, geo_mean, log_evidence)


def varpro_marginals_device(opts, n_vox, b, y, nl_atoms, fixed, lo, hi, log_prior, noise_sd, marginal_amplitudes, n_bins, bin_of, bin_value,
                            probs, marginal, quantile, geo_mean, log_evidence, device, stream=None):
    """Enqueue the marginals on HBM-resident float64 torch tensors (asynchronous; caller synchronises): y (n_vox, n_b), marginal
    (sum n_bins, n_vox), quantile (n_q, n_free, n_vox) or None when probs is empty, geo_mean (n_free, n_vox) or None, log_evidence
    (n_vox,) or None on the device; b, nl_atoms (n_nonlinear_free, n_atoms), shared fixed values, lo, hi, log_prior (n_atoms,) or
    None, the binning over all free parameters (n_bins (n_free,), bin_of (n_free, n_atoms), bin_value) and probs are host arrays.
    `opts` from make_opts.  Returns the dict of `varpro_marginals` over views of the caller's tensors."""
    b, nl_atoms, lo, hi = (np.ascontiguousarray(a, np.float64) for a in (b, nl_atoms, lo, hi))
    if fixed is not None:
        fixed = np.ascontiguousarray(fixed, np.float64)
    if nl_atoms.ndim != 2:
        raise ValueError("nl_atoms must have shape (n_nonlinear_free, n_atoms)")
    lp = _posterior_log_prior(log_prior, nl_atoms.shape[1])
    n_bins = np.ascontiguousarray(n_bins, np.int32)
    bin_of = np.ascontiguousarray(bin_of, np.int32)
    bin_value = np.ascontiguousarray(bin_value, np.float64)
    probs = _marginal_probs(probs)
    n = opts.n_free
    if n_bins.shape != (n,) or bin_of.shape != (n, nl_atoms.shape[1]) or (n_bins < 0).any() or bin_value.shape != (int(n_bins.sum()),):
        raise ValueError(f"the binning must be n_bins ({n},) >= 0, bin_of ({n}, {nl_atoms.shape[1]}), bin_value (sum n_bins,)")
    check(load().pnx_curvefit_varpro_marginals_f64(C.byref(opts), int(n_vox), ptr(b), ptr(y), int(nl_atoms.shape[1]), ptr(nl_atoms), ptr(fixed),
                                                   ptr(lo), ptr(hi), ptr(lp), float(noise_sd), int(bool(marginal_amplitudes)), ptr(n_bins),
                                                   ptr(bin_of), ptr(bin_value), int(probs.size), ptr(probs) if probs.size else None,
                                                   ptr(marginal), ptr(quantile) if probs.size else None, ptr(geo_mean), ptr(log_evidence),
                                                   MEM_DEVICE, int(device), stream))
    if geo_mean is None:
        geo_mean = {k: None for k in range(n)}
    return _varpro_marginal_result(n_bins, bin_value, probs, marginal, quantile if probs.size else None, geo_mean, log_evidence)


LOGLINEAR_WEIGHTING = {"none": 0, "signal2": 1}  # w = 1 / w = y^2 (include/pnx.h)
LOGLINEAR_MAX_REWEIGHT = 8  # kLogLinMaxReweight of csrc/pnx_loglin_args.hpp


def _b_values(b, n_b, dt):
    b = np.ascontiguousarray(b, dt)
    if b.shape != (n_b,):
        raise ValueError(f"b has shape {b.shape}, expected ({n_b},)")
    return b


def _weighting_and_clip(dt, weighting, clip, n, clip_text):
    """The weighting code and lo / hi (n,) in the storage type `dt`, or None: what _loglinear_args and _peel_args check alike."""
    if weighting not in LOGLINEAR_WEIGHTING:
        raise ValueError(f"weighting must be one of {sorted(LOGLINEAR_WEIGHTING)}, got {weighting!r}")
    lo = hi = None
    if clip is not None:
        lo, hi = (np.ascontiguousarray(a, dt) for a in clip)
        if lo.shape != (n,) or hi.shape != (n,):
            raise ValueError(clip_text)
    return LOGLINEAR_WEIGHTING[weighting], lo, hi


def _loglinear_args(b, n_b, dt, bvalue_mask, weighting, clip):
    """The small host arguments of pnx_loglinear_f64 / _f32 in the storage type `dt`: b, the uint8 mask or None, the weighting
    code, lo / hi (2,) or None."""
    b = _b_values(b, n_b, dt)
    use = None
    if bvalue_mask is not None:
        use = np.ascontiguousarray(np.asarray(bvalue_mask) != 0, np.uint8)
        if use.shape != (n_b,):
            raise ValueError(f"bvalue_mask has shape {use.shape}, expected ({n_b},)")
    return (b, use, *_weighting_and_clip(dt, weighting, clip, 2, "clip must be (lo, hi) with two entries each: the bounds of S0 and D"))


def _loglinear_call(f32, args, n_reweight, y, params, pcov, status, n_used, ss_res, mem, device, stream):
    """pnx_loglinear_f64, or _f32 where the storage type is float32, on host arrays or device tensors; args: what _loglinear_args
    made of the small host arguments."""
    b, use, wcode, lo, hi = args
    n_vox, n_b = (int(s) for s in y.shape)
    fn = load().pnx_loglinear_f32 if f32 else load().pnx_loglinear_f64
    check(fn(n_vox, n_b, ptr(b), ptr(use), wcode, int(n_reweight), int(lo is not None), ptr(lo), ptr(hi), ptr(y), ptr(params),
             ptr(pcov), ptr(status), ptr(n_used), ptr(ss_res), mem, int(device), stream))


def loglinear(b, y, *, bvalue_mask=None, weighting="signal2", n_reweight=0, clip=None, want_pcov=True, device=0, out=None):
    """Log-linear mono-exponential fit ln S = ln S0 - b D per voxel on host (numpy) arrays (pnx_loglinear_f64; method, status
    codes and outputs: include/pnx.h).  A float32 signal selects the fp32-storage entry point (pnx_loglinear_f32: every data
    array float32 in and out, fp64 arithmetic on the device).

    bvalue_mask (n_b,) bool or None: the b-values that take part (one mask for the call); weighting "signal2" (w = y^2) or "none";
    n_reweight 0 .. 8 further passes with w = exp(a - b D)^2; clip: None or (lo, hi), two entries each for S0 and D.
    Returns dict(params (2, n_vox) [S0, D], pcov (n_vox, 2, 2) | None, status int8, n_used int32, ss_res).
    `out`: optional dict of preallocated result arrays ("params", "pcov", "status", "n_used", "ss_res")."""
    _lib.require_device()
    dt = np.float32 if getattr(y, "dtype", None) == np.float32 else np.float64
    y = np.ascontiguousarray(np.atleast_2d(y), dt)
    n_vox, n_b = y.shape
    args = _loglinear_args(b, n_b, dt, bvalue_mask, weighting, clip)
    params = _out(out, "params", (2, n_vox), dt)
    pcov = _out(out, "pcov", (n_vox, 2, 2), dt) if want_pcov else None
    status = _out(out, "status", (n_vox,), np.int8)
    n_used = _out(out, "n_used", (n_vox,), np.int32)
    ss_res = _out(out, "ss_res", (n_vox,), dt)
    _loglinear_call(dt is np.float32, args, n_reweight, y, params, pcov, status, n_used, ss_res, MEM_HOST, device, None)
    return dict(params=params, pcov=pcov, status=status, n_used=n_used, ss_res=ss_res)


def loglinear_device(b, y, params, pcov, status, n_used, ss_res, device, *, bvalue_mask=None, weighting="signal2", n_reweight=0,
                     clip=None, stream=None):
    """Enqueue the log-linear fit on HBM-resident torch tensors (asynchronous; caller synchronises): y (n_vox, n_b), params
    (2, n_vox), and -- each may be None -- pcov (n_vox, 2, 2), status int8, n_used int32, ss_res (n_vox,).  float32 tensors select
    pnx_loglinear_f32.  b, bvalue_mask and the clip bounds are host arrays, as `loglinear` takes them."""
    f32 = "float32" in str(getattr(y, "dtype", ""))
    args = _loglinear_args(b, int(y.shape[1]), np.float32 if f32 else np.float64, bvalue_mask, weighting, clip)
    _loglinear_call(f32, args, n_reweight, y, params, pcov, status, n_used, ss_res, MEM_DEVICE, device, stream)


PEEL_STAGES = {"mono": 1, "bi_reduced": 2, "bi_s0": 2, "bi_full": 2, "tri_reduced": 3, "tri_s0": 3, "tri_full": 3}  # exponentials


def peel_masks(b, model, b_thresholds):
    """The (K, n_b) uint8 stage masks of `peel` from K - 1 ascending thresholds [t_1 < ... < t_{K-1}]: stage 0 (the slowest
    compartment, fitted first) takes b >= t_{K-1}, a middle stage k (K = 3 only) t_{K-1-k} <= b < t_{K-k}, the last stage
    b < t_1.  K = 1: every b-value."""
    K = PEEL_STAGES[model]
    b = np.asarray(b, float)
    t = np.atleast_1d(np.asarray([] if b_thresholds is None else b_thresholds, float))
    if t.shape != (K - 1,) or not (np.diff(t) > 0).all() or not np.isfinite(t).all():
        raise ValueError(f"b_thresholds must hold {K - 1} ascending values for {model!r}, got {b_thresholds!r}")
    edges = np.concatenate([[-np.inf], t, [np.inf]])  # stage k: edges[K-1-k] <= b < edges[K-k]
    return np.ascontiguousarray(np.stack([(b >= edges[K - 1 - k]) & (b < edges[K - k]) for k in range(K)]), np.uint8)


def _peel_args(b, n_b, dt, model, masks, b_thresholds, weighting, clip, fallback):
    """The small host arguments of pnx_peel_f64 / _f32 in the storage type `dt`: b, the (K, n_b) uint8 masks, the weighting code,
    lo / hi (n_params,) or None, fallback (n_params,) or None."""
    if model not in PEEL_STAGES:
        raise ValueError(f"model must be one of {sorted(PEEL_STAGES)}, got {model!r}")
    K, n = PEEL_STAGES[model], len(MODEL_PARAM_NAMES[model])
    b = _b_values(b, n_b, dt)
    if (masks is None) == (b_thresholds is None) and not (K == 1 and masks is None):
        raise ValueError("peel takes either masks (K, n_b) or b_thresholds (K - 1 ascending values)")
    if masks is None:
        use = peel_masks(b, model, b_thresholds)
    else:
        use = np.ascontiguousarray(np.atleast_2d(np.asarray(masks)) != 0, np.uint8)
        if use.shape != (K, n_b):
            raise ValueError(f"masks has shape {use.shape}, expected ({K}, {n_b})")
    wcode, lo, hi = _weighting_and_clip(dt, weighting, clip, n,
                                        f"clip must be (lo, hi) with {n} entries each: the bounds of {MODEL_PARAM_NAMES[model]}")
    if fallback is not None:
        fallback = np.ascontiguousarray(fallback, dt)
        if fallback.shape != (n,):
            raise ValueError(f"fallback must have {n} entries: {MODEL_PARAM_NAMES[model]}")
    return b, use, wcode, lo, hi, fallback


def _peel_call(f32, args, model, y, params, status, n_used, ss_res, mem, device, stream):
    """pnx_peel_f64, or _f32 where the storage type is float32, on host arrays or device tensors; args: what _peel_args made of the
    small host arguments."""
    b, use, wcode, lo, hi, fb = args
    n_vox, n_b = (int(s) for s in y.shape)
    fn = load().pnx_peel_f32 if f32 else load().pnx_peel_f64
    check(fn(MODEL_IDS[model], n_vox, n_b, ptr(b), ptr(use), wcode, int(lo is not None), ptr(lo), ptr(hi), ptr(fb), ptr(y), ptr(params),
             ptr(status), ptr(n_used), ptr(ss_res), mem, int(device), stream))


def peel(b, y, model, *, masks=None, b_thresholds=None, weighting="signal2", clip=None, fallback=None, device=0, out=None):
    """Exponential peeling of a mono-, bi- or tri-exponential layout per voxel on host (numpy) arrays (pnx_peel_f64; method, status
    codes and outputs: include/pnx.h).  A float32 signal selects the fp32-storage entry point (pnx_peel_f32).

    model: a key of MODEL_IDS; masks (K, n_b) 0/1, row k the b-values of stage k (stage 0 = the slowest compartment), or
    b_thresholds, K - 1 ascending values (`peel_masks`); weighting "signal2" (w = r^2) or "none"; clip: None or (lo, hi) with one
    entry per parameter; fallback: None or the vector a voxel that could not be fitted returns instead of NaN.
    Returns dict(params (n_params, n_vox), status int8, n_used (K, n_vox) int32, ss_res).
    `out`: optional dict of preallocated result arrays ("params", "status", "n_used", "ss_res")."""
    _lib.require_device()
    dt = np.float32 if getattr(y, "dtype", None) == np.float32 else np.float64
    y = np.ascontiguousarray(np.atleast_2d(y), dt)
    n_vox, n_b = y.shape
    args = _peel_args(b, n_b, dt, model, masks, b_thresholds, weighting, clip, fallback)
    params = _out(out, "params", (len(MODEL_PARAM_NAMES[model]), n_vox), dt)
    status = _out(out, "status", (n_vox,), np.int8)
    n_used = _out(out, "n_used", (PEEL_STAGES[model], n_vox), np.int32)
    ss_res = _out(out, "ss_res", (n_vox,), dt)
    _peel_call(dt is np.float32, args, model, y, params, status, n_used, ss_res, MEM_HOST, device, None)
    return dict(params=params, status=status, n_used=n_used, ss_res=ss_res)


def peel_device(b, y, model, params, status, n_used, ss_res, device, *, masks=None, b_thresholds=None, weighting="signal2", clip=None,
                fallback=None, stream=None):
    """Enqueue the peeling fit on HBM-resident torch tensors (asynchronous; caller synchronises): y (n_vox, n_b), params
    (n_params, n_vox), and -- each may be None -- status int8, n_used (K, n_vox) int32, ss_res (n_vox,).  float32 tensors select
    pnx_peel_f32.  b, the masks or thresholds, the clip bounds and the fallback are host arrays, as `peel` takes them."""
    f32 = "float32" in str(getattr(y, "dtype", ""))
    args = _peel_args(b, int(y.shape[1]), np.float32 if f32 else np.float64, model, masks, b_thresholds, weighting, clip, fallback)
    _peel_call(f32, args, model, y, params, status, n_used, ss_res, MEM_DEVICE, device, stream)


class NnlsPlan:
    """Shared part of one NNLS fit: A = [basis; reg] uploaded and reduced to its Gram form once."""

    def __init__(self, basis, reg=None, device=0):
        _lib.require_device()
        basis = np.ascontiguousarray(basis, np.float64)
        if basis.ndim != 2:
            raise ValueError("basis must be 2-D (n_meas, n_bins)")
        self.n_meas, self.n_bins = basis.shape
        n_reg = 0
        if reg is not None:
            reg = np.ascontiguousarray(reg, np.float64)
            if reg.ndim != 2 or reg.shape[1] != self.n_bins:
                raise ValueError("reg must be (n_reg, n_bins)")
            n_reg = reg.shape[0]
        self.device = device
        self._h = C.c_void_p()
        check(load().pnx_nnls_plan_create(C.byref(self._h), self.n_meas, self.n_bins, ptr(basis), ptr(reg), n_reg,
                                          device))

    def solve(self, y, max_iter=250, out=None):
        """`out`: optional dict of preallocated result arrays ("coefficients", "residual", "status", "iters")."""
        dt = np.float32 if getattr(y, "dtype", None) == np.float32 else np.float64  # float32 in -> float32 out
        y = np.ascontiguousarray(np.atleast_2d(y), dt)
        n_vox = y.shape[0]
        if y.shape[1] != self.n_meas:
            raise ValueError(f"signal has {y.shape[1]} measurements, basis has {self.n_meas}")
        coeff = _out(out, "coefficients", (n_vox, self.n_bins), dt)
        rnorm = _out(out, "residual", (n_vox,), dt)
        status = _out(out, "status", (n_vox,), np.int8)
        iters = _out(out, "iters", (n_vox,), np.int32)
        fn = load().pnx_nnls_solve_f32 if dt is np.float32 else load().pnx_nnls_solve_f64
        check(fn(self._h, n_vox, ptr(y), int(max_iter), ptr(coeff), ptr(rnorm), ptr(status),
                                        ptr(iters), MEM_HOST, None))
        return dict(coefficients=coeff, residual=rnorm, status=status, iters=iters)

    def solve_device(self, n_vox, y, max_iter, coeff, rnorm, status, iters, stream=None):
        fn = load().pnx_nnls_solve_f32 if "float32" in str(getattr(y, "dtype", "")) else load().pnx_nnls_solve_f64
        check(fn(self._h, int(n_vox), ptr(y), int(max_iter), ptr(coeff), ptr(rnorm),
                                        ptr(status), ptr(iters), MEM_DEVICE, stream))

    def aty_device(self, n_vox, y, aty=None, stream=None):
        """Enqueue the MFMA Gram step alone: aty (n_vox, 256) = y @ basis (None: into the plan's own scratch)."""
        check(load().pnx_nnls_aty_f64(self._h, int(n_vox), ptr(y), ptr(aty), stream))

    def fit_stats(self, y, coeff, want_pred=False):
        """Data-term residual of a batch of spectra on the device (pnx_nnls_fit_stats_f64): dict(ss_res (n_vox,) =
        sum_j (y - coeff @ basis.T)^2 over the measurements -- not `residual`^2 of a regularised solve, which contains the
        regulariser rows -- and pred (n_vox, n_meas) = coeff @ basis.T when want_pred, else None).  y None: the prediction
        alone (ss_res None).  numpy arrays, or torch device tensors for both (then the outputs are tensors and the call only
        enqueues)."""
        tensor = _is_torch(coeff)
        if y is None and not want_pred:
            raise ValueError("nothing to compute: no signal y for ss_res and want_pred=False")
        if y is not None and tensor != _is_torch(y):
            raise ValueError("y and coeff must both be numpy arrays or both be device tensors")
        if not tensor:
            y = None if y is None else np.ascontiguousarray(np.atleast_2d(y), np.float64)
            coeff = np.ascontiguousarray(np.atleast_2d(coeff), np.float64)
        if len(coeff.shape) != 2 or coeff.shape[1] != self.n_bins:
            raise ValueError(f"coeff has shape {tuple(coeff.shape)}, expected (n_vox, {self.n_bins})")
        n_vox = int(coeff.shape[0])
        if y is not None and tuple(y.shape) != (n_vox, self.n_meas):
            raise ValueError(f"signal has shape {tuple(y.shape)}, expected ({n_vox}, {self.n_meas})")
        if tensor:
            import torch

            for t in (y, coeff):
                if t is not None and (t.dtype != torch.float64 or not t.is_contiguous()):
                    raise ValueError("device tensors must be contiguous float64")
            ss = torch.empty(n_vox, dtype=torch.float64, device=coeff.device) if y is not None else None
            pred = torch.empty((n_vox, self.n_meas), dtype=torch.float64, device=coeff.device) if want_pred else None
            stream = torch.cuda.current_stream(coeff.device).cuda_stream
        else:
            ss = np.empty(n_vox) if y is not None else None
            pred = np.empty((n_vox, self.n_meas)) if want_pred else None
            stream = None
        check(load().pnx_nnls_fit_stats_f64(self._h, n_vox, ptr(y), ptr(coeff), ptr(ss), ptr(pred), MEM_DEVICE if tensor else MEM_HOST,
                                            int(self.device), stream))
        return dict(ss_res=ss, pred=pred)

    def solve_peaks(self, y, bins, max_iter=250, height=0.1, regularized=False, rel_height=0.5, max_peaks=8, cutoffs=None,
                    with_ss_res=False):
        """Solve and reduce every spectrum to its peak table on the device (pnx_nnls_solve_peaks_f64): the (n_vox, n_bins)
        spectra never cross PCIe.  Returns dict(n_peaks, d_values, f_values (n_vox, max_peaks) NaN padded, d_cut, f_cut
        (n_vox, n_cut) or None, residual, status, iters).  with_ss_res: also ss_res (n_vox,), the data-term residual
        sum_j (y - B x)^2 of every spectrum, reduced while it is resident (pnx_nnls_solve_peaks_stats_f64)."""
        y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
        n_vox = y.shape[0]
        if y.shape[1] != self.n_meas:
            raise ValueError(f"signal has {y.shape[1]} measurements, basis has {self.n_meas}")
        bins = np.ascontiguousarray(bins, np.float64)
        if bins.shape != (self.n_bins,):
            raise ValueError(f"bins has shape {bins.shape}, expected ({self.n_bins},)")
        cut = None if cutoffs is None else np.ascontiguousarray(cutoffs, np.float64).reshape(-1, 2)
        n_cut = 0 if cut is None else cut.shape[0]
        out = dict(n_peaks=np.empty(n_vox, np.int32), d_values=np.empty((n_vox, max_peaks)), f_values=np.empty((n_vox, max_peaks)),
                   d_cut=np.empty((n_vox, n_cut)) if n_cut else None, f_cut=np.empty((n_vox, n_cut)) if n_cut else None,
                   residual=np.empty(n_vox), status=np.empty(n_vox, np.int8), iters=np.empty(n_vox, np.int32))
        args = (self._h, n_vox, ptr(y), int(max_iter), ptr(bins), float(height), int(bool(regularized)),
                float(rel_height), int(max_peaks), ptr(out["n_peaks"]), ptr(out["d_values"]),
                ptr(out["f_values"]), n_cut, ptr(cut), ptr(out["d_cut"]), ptr(out["f_cut"]),
                ptr(out["residual"]), ptr(out["status"]), ptr(out["iters"]), MEM_HOST, None)
        if with_ss_res:
            out["ss_res"] = np.empty(n_vox)
            check(load().pnx_nnls_solve_peaks_stats_f64(*args, ptr(out["ss_res"])))
        else:
            check(load().pnx_nnls_solve_peaks_f64(*args))
        return out

    def close(self):
        if self._h:
            load().pnx_nnls_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


NNLSPlan = NnlsPlan

PREDICT_MAX_X = 128  # PNX_MAX_BVALUES


def predict(model, x, params, fixed_idx=(), fixed_vals=None, y=None, want_pred=True, t1_mode=0, tr=0.0, tm=0.0, device=0, out=None):
    """Forward model of a parametric layout for all voxels on the device (pnx_curvefit_predict_f64).

    x (n_x <= 128,) need not be the fitted b-values; params (n_free, n_vox) parameter-major as `curvefit` returns popt;
    fixed_idx / fixed_vals ((n_fixed,) or (n_fixed, n_vox)) as `curvefit` takes them; y (n_vox, n_x) optional signal.
    Returns dict(pred (n_vox, n_x) or None when not want_pred, ss_res (n_vox,) = sum_i (pred_i - y_i)^2 or None without y).
    numpy arrays, or torch device tensors for params / per-voxel fixed_vals / y (then the outputs are tensors and the call
    only enqueues).  `out`: optional dict of preallocated numpy result arrays ("pred", "ss_res")."""
    tensor = _is_torch(params)
    x = np.ascontiguousarray(x, np.float64)
    if x.ndim != 1 or not 1 <= x.size <= PREDICT_MAX_X:
        raise ValueError(f"x must be 1-D with 1 .. {PREDICT_MAX_X} values, got shape {x.shape}")
    if not want_pred and y is None:
        raise ValueError("nothing to compute: want_pred=False and no signal y for ss_res")
    if model not in MODEL_IDS:
        raise ValueError(f"unknown model {model!r}")
    if not tensor:
        params = np.ascontiguousarray(params, np.float64)
    fpv = False
    fv = None
    if len(fixed_idx):
        if fixed_vals is None:
            raise ValueError("fixed_idx without fixed_vals")
        fv = fixed_vals if _is_torch(fixed_vals) else np.ascontiguousarray(fixed_vals, np.float64)
        fpv = len(fv.shape) == 2
    o = make_opts(model, x.size, fixed_idx, False, fpv, jac="analytic", t1_mode=t1_mode, tr=tr, tm=tm)
    if len(params.shape) != 2 or params.shape[0] != o.n_free:
        raise ValueError(f"params has shape {tuple(params.shape)}, expected ({o.n_free}, n_vox)")
    n_vox = int(params.shape[1])
    if fv is not None and tuple(fv.shape) != ((o.n_fixed, n_vox) if fpv else (o.n_fixed,)):
        raise ValueError("fixed_vals has the wrong shape")
    if fv is not None and _is_torch(fv) != (tensor and fpv):
        raise ValueError("per-voxel fixed_vals live where params live; shared fixed_vals are a host array")
    if y is not None:
        if _is_torch(y) != tensor:
            raise ValueError("y and params must both be numpy arrays or both be device tensors")
        if not tensor:
            y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
        if tuple(y.shape) != (n_vox, x.size):
            raise ValueError(f"y has shape {tuple(y.shape)}, expected ({n_vox}, {x.size})")
    if tensor:
        import torch

        for t in (params, y, fv if fpv else None):
            if t is not None and (t.dtype != torch.float64 or not t.is_contiguous()):
                raise ValueError("device tensors must be contiguous float64")
        pred = torch.empty((n_vox, x.size), dtype=torch.float64, device=params.device) if want_pred else None
        ss = torch.empty(n_vox, dtype=torch.float64, device=params.device) if y is not None else None
        device = params.device.index
        stream = torch.cuda.current_stream(params.device).cuda_stream
    else:
        pred = _out(out, "pred", (n_vox, x.size), np.float64) if want_pred else None
        ss = _out(out, "ss_res", (n_vox,), np.float64) if y is not None else None
        stream = None
    _lib.require_device()
    check(load().pnx_curvefit_predict_f64(C.byref(o), n_vox, int(x.size), ptr(x), ptr(params), ptr(fv), ptr(y), ptr(pred), ptr(ss),
                                          MEM_DEVICE if tensor else MEM_HOST, int(device), stream))
    return dict(pred=pred, ss_res=ss)


def nnls(basis, reg, y, max_iter=250, device=0, out=None):
    plan = NnlsPlan(basis, reg, device)
    try:
        return plan.solve(y, max_iter, out=out)
    finally:
        plan.close()


def nnls_bins(d_min, d_max, n_bins):
    out = np.empty(int(n_bins))
    check(load().pnx_nnls_bins(float(d_min), float(d_max), int(n_bins), ptr(out)))
    return out


def nnls_regularization_matrix(n_bins, order, mu=1.0):
    out = np.empty((int(n_bins), int(n_bins)))
    check(load().pnx_nnls_regularization_matrix(int(n_bins), int(order), float(mu), ptr(out)))
    return out


def nnls_basis(b, bins, device=0):
    _lib.require_device()
    b = np.ascontiguousarray(b, np.float64)
    bins = np.ascontiguousarray(bins, np.float64)
    out = np.empty((b.size, bins.size))
    check(load().pnx_nnls_basis(b.size, ptr(b), bins.size, ptr(bins), ptr(out), device))
    return out


SPECTRUM_MAX_PEAKS = 64  # kMaxPeaks of csrc/pnx_spectrum.hip (one peak per lane of the wave that owns the spectrum)


def spectrum_peaks(spectrum, bins, height=0.1, regularized=False, rel_height=0.5, max_peaks=8, cutoffs=None, device=0):
    """find_spectrum_peaks (+ apply_cutoffs) of utility/spectrum.py for every row of `spectrum` (n_vox, n_bins) at once, on
    the device.  numpy arrays in and out, or torch-cuda tensors for `spectrum` (then the outputs are torch tensors)."""
    _lib.require_device()
    tensor = _is_torch(spectrum)
    if not tensor:
        spectrum = np.ascontiguousarray(np.atleast_2d(spectrum), np.float64)
    n_vox, n_bins = spectrum.shape
    bins = np.ascontiguousarray(bins, np.float64)
    if bins.shape != (n_bins,):
        raise ValueError(f"bins has shape {bins.shape}, expected ({n_bins},)")
    cut = None if cutoffs is None else np.ascontiguousarray(cutoffs, np.float64).reshape(-1, 2)
    n_cut = 0 if cut is None else cut.shape[0]
    if tensor:
        import torch

        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=spectrum.device)
        out = dict(n_peaks=mk(n_vox, torch.int32), d_values=mk((n_vox, max_peaks), torch.float64),
                   f_values=mk((n_vox, max_peaks), torch.float64),
                   d_cut=mk((n_vox, n_cut), torch.float64) if n_cut else None, f_cut=mk((n_vox, n_cut), torch.float64) if n_cut else None)
        device = spectrum.device.index
        stream = torch.cuda.current_stream(spectrum.device).cuda_stream
    else:
        out = dict(n_peaks=np.empty(n_vox, np.int32), d_values=np.empty((n_vox, max_peaks)), f_values=np.empty((n_vox, max_peaks)),
                   d_cut=np.empty((n_vox, n_cut)) if n_cut else None, f_cut=np.empty((n_vox, n_cut)) if n_cut else None)
        stream = None
    check(load().pnx_nnls_spectrum_peaks_f64(n_vox, n_bins, ptr(spectrum), ptr(bins), float(height), int(bool(regularized)),
                                             float(rel_height), int(max_peaks), ptr(out["n_peaks"]), ptr(out["d_values"]),
                                             ptr(out["f_values"]), n_cut, ptr(cut), ptr(out["d_cut"]), ptr(out["f_cut"]),
                                             MEM_DEVICE if tensor else MEM_HOST, int(device), stream))
    if not tensor and n_vox:
        # rows the device table could not hold: more than 64 peaks, or more than 16 in a spectrum with a flat-topped rise
        over = out["n_peaks"] > SPECTRUM_MAX_PEAKS
        if max_peaks:
            over |= (out["n_peaks"] > 16) & np.isnan(out["d_values"][:, 0])
        if over.any():
            import warnings

            warnings.warn(f"{int(over.sum())} spectra have more than {SPECTRUM_MAX_PEAKS} peaks (the device table's size; 16 for a spectrum "
                          f"with a flat-topped rise): their peak and cutoff rows are NaN; n_peaks holds the count", RuntimeWarning, stacklevel=2)
    return out


def scatter_maps(values, pixel_indices, spatial_shape, device=0):
    """float32 volume `spatial_shape (+ values.shape[1:])`, zero outside the fitted voxels, values[i] at pixel_indices[i]
    (io/nifti.py:279-312 reconstruct_maps) -- laid out on the device (pnx_scatter_maps_f32)."""
    _lib.require_device()
    values = np.ascontiguousarray(values, np.float64)
    idx = np.asarray(pixel_indices)
    spatial_shape = tuple(int(s) for s in spatial_shape)
    lin = np.ascontiguousarray(np.ravel_multi_index(tuple(idx.T), spatial_shape), np.int64)
    n_px = values.shape[0]
    k = int(np.prod(values.shape[1:], dtype=np.int64)) if values.ndim > 1 else 1
    out = np.empty(spatial_shape + values.shape[1:], np.float32)
    check(load().pnx_scatter_maps_f32(ptr(values), ptr(lin), n_px, k, int(np.prod(spatial_shape)), ptr(out), MEM_HOST, int(device), None))
    return out


_RESIZE_METHODS = {"linear": 0, "cubic": 1}


def resize2d(array, target_shape, method="cubic", device=0):
    """Resize the first two axes of a float64 numpy array (X, Y, ...) on the device (pnx_resize2d_f64, host arrays)."""
    _lib.require_device()
    a = np.ascontiguousarray(array, np.float64)
    tx, ty = int(target_shape[0]), int(target_shape[1])
    c = int(np.prod(a.shape[2:], dtype=np.int64)) if a.ndim > 2 else 1
    out = np.empty((tx, ty) + a.shape[2:])
    check(load().pnx_resize2d_f64(ptr(a), a.shape[0], a.shape[1], c, ptr(out), tx, ty, _RESIZE_METHODS[method], MEM_HOST,
                                  int(device), None))
    return out


def resize2d_device(src, x, y, c, dst, tx, ty, method, device, stream=None):
    """Enqueue the resize on HBM-resident float64 tensors: src (x, y, c) -> dst (tx, ty, c)."""
    check(load().pnx_resize2d_f64(ptr(src), int(x), int(y), int(c), ptr(dst), int(tx), int(ty), _RESIZE_METHODS[method],
                                  MEM_DEVICE, int(device), stream))


def ideal_bounds_device(param_map, n_px, lo, hi, tol, p0, lower, upper, device, stream=None):
    """Enqueue p0 / lower / upper (n_params, n_px) of the next IDEAL level from a resized map (n_px, n_params)."""
    lo, hi, tol = (np.ascontiguousarray(a, np.float64) for a in (lo, hi, tol))
    check(load().pnx_ideal_bounds_f64(ptr(param_map), int(n_px), int(lo.size), ptr(lo), ptr(hi), ptr(tol), ptr(p0), ptr(lower),
                                      ptr(upper), int(device), stream))


def ideal_bounds_simplex_device(param_map, n_px, lo, hi, tol, i_f1, i_f2, p0, lower, upper, device, stream=None):
    """`ideal_bounds_device` for a level fitted under f1 + f2 <= 1 (pnx_ideal_bounds_simplex_f64): the clipped start values of
    the fraction rows i_f1 / i_f2 are moved onto the face where their sum exceeds 1, before the windows are built."""
    lo, hi, tol = (np.ascontiguousarray(a, np.float64) for a in (lo, hi, tol))
    check(load().pnx_ideal_bounds_simplex_f64(ptr(param_map), int(n_px), int(lo.size), ptr(lo), ptr(hi), ptr(tol), int(i_f1), int(i_f2),
                                              ptr(p0), ptr(lower), ptr(upper), int(device), stream))


def mask_select_device(mask, threshold, idx, device, stream=None) -> int:
    """idx[:k] = C-order indices of mask > threshold (float64 tensor, any shape); returns k (synchronises the stream)."""
    k = C.c_int64(0)
    check(load().pnx_mask_select_f64(ptr(mask), int(mask.numel()), float(threshold), ptr(idx), C.byref(k), int(device), stream))
    return int(k.value)


def gather_rows_device(src, c, idx, n_sel, dst, device, stream=None):
    check(load().pnx_gather_rows_f64(ptr(src), int(c), ptr(idx), int(n_sel), ptr(dst), int(device), stream))


def scatter_rows_t_device(popt, idx, n_sel, k, n_total, pmap, device, stream=None):
    check(load().pnx_scatter_rows_t_f64(ptr(popt), ptr(idx), int(n_sel), int(k), int(n_total), ptr(pmap), int(device), stream))


def queue_order_device(key, order, device, stream=None):
    """order (int32 tensor) = voxel indices by descending `key` (float64 tensor of predicted evaluation counts), ties in index
    order: what `curvefit_device(..., order=)` takes."""
    check(load().pnx_queue_order_f64(ptr(key), int(key.numel()), ptr(order), int(device), stream))
    return order


def row_ss_tot_device(y, n, c, out, device, stream=None):
    check(load().pnx_row_ss_tot_f64(ptr(y), int(n), int(c), ptr(out), int(device), stream))


def row_ss_tot(y, device=0):
    """sum_j (y_ij - mean_i)^2 per row of a host array (n, c), reduced on the device (pnx_row_ss_tot_f64) in pieces of 2^20 rows:
    the SS_tot of R^2 (fitters/base.py:179-183)."""
    import torch

    _lib.require_device()
    y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
    n, c = y.shape
    out = np.empty(n)
    dev = torch.device("cuda", int(device))
    stream = torch.cuda.current_stream(dev).cuda_stream
    for a in range(0, n, 1 << 20):
        e = min(n, a + (1 << 20))
        y_d = upload(y[a:e], torch.empty((e - a, c), dtype=torch.float64, device=dev), int(device), stream)
        ss_d = torch.empty(e - a, dtype=torch.float64, device=dev)
        row_ss_tot_device(y_d, e - a, c, ss_d, int(device), stream)
        out[a:e] = download(ss_d, int(device), stream)
    return out


LABEL_TABLE_MAX = 8192  # n_labels * (c + 1) entries of the kernel's 64 KB LDS table


def label_sums(rows, label_pos, n_labels, device=0):
    """(sums (n_labels, c), counts (n_labels,)) of the rows per label position (host arrays in and out, pnx_label_sums_f64)."""
    rows = np.ascontiguousarray(rows, np.float64)
    lab = np.ascontiguousarray(label_pos, np.int32)
    n, c = rows.shape
    if lab.shape != (n,):
        raise ValueError(f"label_pos must have shape ({n},), got {lab.shape}")
    sums = np.empty((int(n_labels), c))
    counts = np.empty(int(n_labels), dtype=np.int64)
    check(load().pnx_label_sums_f64(ptr(rows), ptr(lab), n, c, int(n_labels), ptr(sums), ptr(counts), MEM_HOST, int(device), None))
    return sums, counts


def upload(array, tensor, device, stream=None, threads=0):
    """Host numpy array -> device tensor of the same byte size (pnx_upload: a few threads, 32 MiB pieces)."""
    a = np.ascontiguousarray(array)
    nbytes = int(tensor.numel()) * int(tensor.element_size())
    if a.nbytes != nbytes:
        raise ValueError(f"upload: {a.nbytes} host bytes into a {nbytes}-byte tensor")
    check(load().pnx_upload(ptr(tensor), ptr(a), nbytes, int(device), stream, int(threads)))
    return tensor


def download(tensor, device, stream=None, threads=0, dtype=None):
    """Contiguous device tensor -> fresh numpy array of the same shape (pnx_download: destination pages touched ahead of the
    copy, a few threads).  dtype: numpy dtype of the result (default: from the tensor's element size and kind)."""
    import torch

    if not tensor.is_contiguous():
        tensor = tensor.contiguous()
    if dtype is None:
        dtype = {torch.float64: np.float64, torch.float32: np.float32, torch.int8: np.int8, torch.int32: np.int32,
                 torch.int64: np.int64, torch.uint8: np.uint8}[tensor.dtype]
    out = np.empty(tuple(tensor.shape), dtype=dtype)
    if out.nbytes:
        check(load().pnx_download(ptr(out), ptr(tensor), out.nbytes, int(device), stream, int(threads)))
    return out


def sweep_device(model, n_vox, b, y, params, cost, g, jtj, device, stream=None):
    """Enqueue one residual/Jacobian/normal-equation sweep on HBM-resident torch tensors (f32 or f64)."""
    import torch

    f64 = y.dtype == torch.float64
    b = np.ascontiguousarray(b, np.float64 if f64 else np.float32)
    fn = load().pnx_sweep_f64 if f64 else load().pnx_sweep_f32
    check(fn(MODEL_IDS[model], int(n_vox), int(b.size), ptr(b), ptr(y), ptr(params), ptr(cost), ptr(g), ptr(jtj),
             int(device), stream))

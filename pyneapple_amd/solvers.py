"""Pyneapple solver plugins backed by the MI355X HIP library (no CPU fallback).

`HipCurveFitSolver` mirrors `pyneapple.solvers.CurveFitSolver` (reference src/pyneapple/solvers/curvefit.py)
and `HipNNLSSolver` mirrors `pyneapple.solvers.NNLSSolver` (src/pyneapple/solvers/nnls_solver.py): same
constructor arguments, same `fit()` signature, same fitted state (`params_`, `diagnostics_`,
`pixel_results_`), same error behaviour -- only `_fit_data` runs all voxels at once through the C ABI.

`HipConstrainedCurveFitSolver` mirrors `ConstrainedCurveFitSolver` (solvers/constrained_curvefit.py) in its constructor and
its constraint sum(f_i) <= 1, not in its algorithm (pnx_curvefit_simplex_f64).

`HipLogLinearSolver` has no counterpart in the reference: the linearised mono-exponential fit as a closed form
(pnx_loglinear_f64), with the reference's solver contract.  `HipPeelSolver` likewise: exponential peeling of the bi- and
tri-exponential models (pnx_peel_f64).  `HipBayesGridSolver` likewise: posterior mean and sd over a parameter grid
(pnx_curvefit_grid_posterior_f64).  `HipVarProSolver` likewise: rates on a grid, fractions and S0 in closed form
(pnx_curvefit_varpro_f64); `HipBayesVarProSolver` the posterior over that dictionary (pnx_curvefit_varpro_posterior_f64).

Registered under the `pyneapple.solvers` entry-point group (pyproject.toml) as `hip_curvefit` / `hip_nnls` /
`hip_constrained_curvefit` / `hip_loglinear` / `hip_peel` / `hip_bayes_grid` / `hip_varpro` / `hip_bayes_varpro`;
extra scalar keys of `[Fitting.solver]` arrive as keyword arguments (io/toml.py:328-338): `device`,
`n_gpus`, `jacobian`.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from typing import Any

import numpy as np

from . import api
from .sharding import pinned_to_gpu
from ._compat import HAVE_PYNEAPPLE, CurveFitBase, NNLSBase, PixelResultsView, RefBaseSolver

_CURVEFIT_MESSAGES = {
    0: "Optimal parameters not found: The maximum number of function evaluations is exceeded.",
    -1: "Each lower bound must be strictly less than each upper bound.",
    -2: "array must not contain infs or NaNs",
    -3: "Initial guess is outside of provided bounds",
    -4: "Residuals are not finite in the initial point.",
}
# scipy.optimize.curve_fit / least_squares arguments whose SciPy default is what the kernel computes
_CURVE_FIT_DEFAULTS = {"check_finite": True, "nan_policy": None, "loss": "linear",
                       "x_scale": 1.0, "f_scale": 1.0, "tr_solver": None, "full_output": False}
_NNLS_MESSAGES = {0: "Maximum number of iterations reached.", -2: "array must not contain infs or NaNs"}


def _validate_parameter_names(parameters: dict, param_names: list[str]):
    # utility/validation.py:153-173
    missing = set(param_names) - set(parameters.keys())
    if missing:
        raise ValueError(f"Missing bounds for required parameters: {missing}. Required: {param_names}")


def _validate_data_shapes(xdata: np.ndarray, ydata: np.ndarray):
    # utility/validation.py:84-112
    if xdata.ndim != 1:
        raise ValueError(f"xdata must be a 1D array, but got shape {xdata.shape}.")
    if ydata.ndim == 1:
        if ydata.shape[0] != xdata.shape[0]:
            raise ValueError(f"ydata length {ydata.shape[0]} does not match xdata length {xdata.shape[0]}.")
    elif ydata.ndim >= 2:
        if ydata.shape[-1] != xdata.shape[0]:
            raise ValueError(f"ydata second dimension {ydata.shape[-1]} does not match xdata length {xdata.shape[0]}.")
    else:
        raise ValueError(f"ydata must be 1D or 2D array, but got shape {ydata.shape}.")


def kernel_model_key(model) -> str:
    """Map a (reference or stand-in) parametric model object to the library's model id (T1 suffix ignored)."""
    names = list(model._all_param_names)
    if names and names[-1] == "T1":
        names = names[:-1]
    for key, ref in api.MODEL_PARAM_NAMES.items():
        if names == ref:
            return key
    raise NotImplementedError(f"model with parameters {list(model._all_param_names)} is not supported by the HIP backend")


def kernel_t1(model) -> dict:
    """T1 / STEAM settings of a model object (models/*.py: fit_t1, fit_t1_steam, repetition_time, mixing_time)."""
    steam = bool(getattr(model, "fit_t1_steam", False))
    t1 = bool(getattr(model, "fit_t1", False)) or steam
    if not t1:
        return dict(t1_mode=0, tr=0.0, tm=0.0)
    tr = getattr(model, "repetition_time", None)
    tm = getattr(model, "mixing_time", None)
    if tr is None:
        raise ValueError("repetition_time is required when fit_t1=True.")
    if steam and tm is None:
        raise ValueError("mixing_time is required when fit_t1_steam=True.")
    return dict(t1_mode=2 if steam else 1, tr=float(tr), tm=float(tm) if steam else 0.0)


def _io_dtype(name):
    name = str(np.dtype(name)) if not isinstance(name, str) else name
    if name not in ("float64", "float32"):
        raise ValueError("io_dtype must be 'float64' or 'float32'")
    return np.float32 if name == "float32" else np.float64


def _shard_device(first: int, k: int) -> int:
    """Device of shard k.  PNX_SHARE_DEVICE=1 (rehearsal on a one-GPU box, used by the GPU tests) maps every shard to the
    first device: the per-device host threads then run against one card, which is what the C ABI's thread-safety promise
    (include/pnx.h) has to carry anyway."""
    import os

    return first if os.environ.get("PNX_SHARE_DEVICE") == "1" else first + k


def _split(n: int, parts: int):
    edges = np.linspace(0, n, parts + 1).astype(np.int64)
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:]) if b > a]


def _grid_atoms(what, model, kernel_model, p0, bounds, grid, project, project_name=None):
    """The atoms of a dictionary from a grid dict (`p0_grid` of HipCurveFitSolver, `grid` of HipBayesGridSolver; `what` names the
    argument in the messages): the Cartesian product of the sequences in `model.param_names` order, the last parameter fastest; a
    parameter the dict does not name takes its scalar `p0`.  Returns (grid as lists, project, atoms (n_free, n_atoms))."""
    import itertools

    names = list(model.param_names)
    if not isinstance(grid, dict):
        raise ValueError(f"{what} must be a dict from parameter name to a sequence of candidate values")
    unknown = [n for n in grid if n not in names]
    if unknown:
        raise ValueError(f"{what} names parameters the model does not fit: {unknown} (free parameters: {names})")
    has_s0 = "S0" in names and kernel_model in api.PROJECT_MODELS
    if project is None:
        project = has_s0
    if project and not has_s0:
        raise ValueError(f"{project_name or what + '_project'}=True needs a model with a free amplitude S0 {api.PROJECT_MODELS}, not {kernel_model!r}")
    axes = []
    for n in names:
        vals = np.atleast_1d(np.asarray(grid[n], float)) if n in grid else np.array([float(p0[n])])
        lo, hi = bounds[n]
        if vals.ndim != 1 or vals.size < 1:
            raise ValueError(f"{what}[{n!r}] must be a non-empty 1-D sequence of values")
        if not ((vals >= lo) & (vals <= hi)).all():
            raise ValueError(f"{what}[{n!r}] holds a value outside the bounds ({lo}, {hi}) of {n}")
        axes.append(vals)
    n_atoms = int(np.prod([a.size for a in axes], dtype=np.int64))
    if n_atoms > api.GRID_MAX_ATOMS:
        raise ValueError(f"{what} spans {n_atoms} atoms, more than the {api.GRID_MAX_ATOMS} the dictionary search takes")
    atoms = np.ascontiguousarray(np.array(list(itertools.product(*axes)), float).T)  # (n_free, n_atoms)
    return {n: list(map(float, np.atleast_1d(v))) for n, v in grid.items()}, bool(project), atoms


def _varpro_atoms(what, model, kernel_model, p0, bounds, rates, ordered):
    """The atoms of a variable-projection dictionary from a dict of rate lists (`rates` of HipVarProSolver, `p0_varpro["rates"]` of
    HipCurveFitSolver; `what` names the argument in the messages): the Cartesian product of the sequences over the model's free
    NON-LINEAR parameters (the rates, a free T1) in `model.param_names` order, the last one fastest; one the dict does not name
    takes its scalar `p0`.  ordered: keep only the atoms with D1 > D2 > D3 (fixed rates included).  Returns (rates as lists,
    the non-linear names, nl_atoms (n_nonlinear_free, n_atoms))."""
    import itertools

    linear = api.varpro_linear_names(kernel_model)
    names = [n for n in model.param_names if n not in linear]
    if not isinstance(rates, dict):
        raise ValueError(f"{what} must be a dict from the name of a non-linear parameter (a rate, T1) to a sequence of candidate values")
    unknown = [n for n in rates if n not in names]
    if unknown:
        raise ValueError(f"{what} names {unknown}: not free non-linear parameters of the model (those are {names}; fractions and S0 are "
                         "solved in closed form)")
    fixed_lin = [n for n in linear if n not in model.param_names]
    if fixed_lin:
        raise ValueError(f"{what}: the variable projection is not built with a fixed fraction or a fixed S0 ({fixed_lin}): the linear "
                         "structure changes; fix rates or T1 only")
    axes = []
    for n in names:
        if n not in rates and n not in (p0 or {}):
            raise ValueError(f"neither {what} nor p0 holds a value for {n!r}")
        vals = np.atleast_1d(np.asarray(rates[n], float)) if n in rates else np.array([float(p0[n])])
        lo, hi = bounds[n]
        if vals.ndim != 1 or vals.size < 1:
            raise ValueError(f"{what}[{n!r}] must be a non-empty 1-D sequence of values")
        if not ((vals >= lo) & (vals <= hi)).all():
            raise ValueError(f"{what}[{n!r}] holds a value outside the bounds ({lo}, {hi}) of {n}")
        axes.append(vals)
    full = int(np.prod([a.size for a in axes], dtype=np.int64))
    if full > 1 << 24:
        raise ValueError(f"{what} spans {full} combinations: too many to enumerate")
    atoms = np.array(list(itertools.product(*axes)), float).reshape(full, len(names)).T  # (n_nl, n_atoms)
    if ordered:
        fixed = getattr(model, "fixed_params", None) or {}
        d_names = sorted(n for n in model._all_param_names if n.startswith("D") and n[1:].isdigit())
        cols = [atoms[names.index(n)] if n in names else np.full(full, float(fixed[n])) for n in d_names]
        keep = np.ones(full, bool)
        for a, b in zip(cols[:-1], cols[1:]):
            keep &= a > b
        atoms = atoms[:, keep]
    n_atoms = atoms.shape[1]
    if n_atoms < 1:
        raise ValueError(f"{what} leaves no atom" + (" with D1 > D2 > D3 (ordered=True)" if ordered else ""))
    if n_atoms > api.GRID_MAX_ATOMS:
        raise ValueError(f"{what} spans {n_atoms} atoms, more than the {api.GRID_MAX_ATOMS} the dictionary search takes")
    return {n: list(map(float, np.atleast_1d(v))) for n, v in rates.items()}, names, np.ascontiguousarray(atoms)


class HipCurveFitSolver(CurveFitBase):
    """Batched bounded NLLS on MI355X with SciPy `curve_fit(method="trf")` semantics.

    Args mirror CurveFitSolver (curvefit.py:36-89).  `use_jacobian` is stored and, as in the reference (curvefit.py:289-293
    passes `jac_fn`, which is None without fixed parameters), does not select the Jacobian: finite differences without
    fixed parameters, the analytic model Jacobian with them.  `multi_threading` / `n_pools` describe the reference's
    joblib pool and have no meaning here.  Extra keyword arguments:
        xtol, gtol: least_squares tolerances (SciPy default 1e-8); any other curve_fit argument is refused.
        jacobian: "fd" (default; SciPy 2-point finite differences, what the reference uses when no parameter
            is fixed) or "analytic" (model Jacobian; always used when parameters are fixed, like the reference).
        device: first HIP device index (default 0).  n_gpus: number of devices to shard voxels over (default 1).
        io_dtype: "float64" (default, the reference's array types) or "float32": signals, start values, bounds and
            fixed maps cross the ABI as float32 and results come back as float32 (pnx_curvefit_batch_f32); the
            arithmetic stays fp64 -- for float32 images this is what the reference computes, without the float64
            host copy.
        precision: "float64" (default) or "float32": fp32 ARITHMETIC on a separate kernel (pnx_curvefit_fast_f32).  Implies
            float32 arrays across the ABI and the analytic Jacobian; results are float32-quality minima, not SciPy-parity
            results.  Not built there, hence a ValueError: jacobian="fd", fixed parameters, a T1 model, sigma.
        p0_grid: None (default: every voxel starts from `p0`, as in the reference) or a dict from parameter name to a sequence
            of candidate values (TOML: arrays under [Fitting.solver.p0_grid]).  The candidates ("atoms") are the Cartesian
            product of the sequences in `model.param_names` order, the last parameter varying fastest; a parameter the dict
            does not name takes its scalar `p0`.  Each voxel then starts from the atom whose model signal is closest to its
            own (pnx_curvefit_grid_start_f64) unless `fit()` is given an explicit `p0`; `diagnostics_` gains "p0_atom" (int32
            index of the atom, -1 for a non-finite signal) and "p0_cost".  At most 4096 atoms, every value inside `bounds`.
            Not built with it, hence a ValueError: precision / io_dtype "float32", per-pixel fixed parameters, per-voxel bounds.
        p0_peel: None (default) or {"b_thresholds": [...], "weighting": "signal2"}: every voxel of
            `fit()` starts from its exponential-peeling estimate (pnx_peel_f64, api.peel_masks for the thresholds), clipped into
            `bounds`; a voxel the peel could not fit starts from `p0`.  `diagnostics_` gains "p0_status" (the peel's int8 status).
            Not built with it, hence a ValueError: together with p0_grid, an explicit per-voxel p0, fixed parameters (model or per
            pixel), a T1 / STEAM model, per-voxel bounds, precision / io_dtype "float32", HipConstrainedCurveFitSolver.
        p0_varpro: None (default) or {"rates": {name: [...]}, "ordered": True}: every voxel of `fit()` starts from its
            variable-projection estimate (pnx_curvefit_varpro_f64; the meaning of HipVarProSolver's `rates` and `ordered`): only
            the rates (and a free T1) are on the grid, fractions and S0 come in closed form, clipped into `bounds`; a voxel with a
            non-finite signal starts from `p0`.  `diagnostics_` gains "p0_atom", "p0_cost" and "p0_clipped".  Opt-in.  Not built
            with it, hence a ValueError: together with p0_grid or p0_peel, an explicit per-voxel p0, per-pixel fixed parameters, a
            fixed fraction or S0, per-voxel bounds, precision / io_dtype "float32", HipConstrainedCurveFitSolver.
        p0_grid_project: fit the amplitude S0 per voxel and atom, clipped to its bounds, instead of taking it from the atoms
            (so S0 needs no entry in p0_grid).  Default: True exactly when the model has a free S0.
    """

    def __init__(self, model: Any, max_iter: int, tol: float, p0: dict[str, float],
                 bounds: dict[str, tuple[float, float]], verbose: bool = False, method: str = "trf",
                 multi_threading: bool = False, use_jacobian: bool = True, **solver_kwargs):
        self.device = int(solver_kwargs.pop("device", 0))
        self.n_gpus = int(solver_kwargs.pop("n_gpus", 1))
        self.precision = solver_kwargs.pop("precision", "float64")
        fast = api._precision(self.precision)
        explicit_jac = "jacobian" in solver_kwargs
        self.jacobian_mode = str(solver_kwargs.pop("jacobian", "analytic" if fast else "fd"))
        self.io_dtype = _io_dtype(solver_kwargs.pop("io_dtype", "float32" if fast else "float64"))
        if self.jacobian_mode not in ("fd", "analytic"):
            raise ValueError("jacobian must be 'fd' or 'analytic'")
        if fast:
            if explicit_jac and self.jacobian_mode == "fd":
                raise ValueError("precision='float32' fits with the analytic Jacobian (SciPy's 2-point step is below fp32 "
                                 "resolution); jacobian='fd' cannot be honoured")
            self.io_dtype = np.float32  # fp32 arithmetic reads and writes float32 arrays
        # The reference forwards every remaining key into scipy.optimize.curve_fit (curvefit.py:295-306).  The kernel
        # implements least_squares' xtol / gtol; anything else would change SciPy's result and there is no CPU path to
        # honour it, so it is refused instead of being dropped silently (keys at their SciPy default are accepted).
        p0_grid = solver_kwargs.pop("p0_grid", None)
        p0_grid_project = solver_kwargs.pop("p0_grid_project", None)
        p0_peel = solver_kwargs.pop("p0_peel", None)
        p0_varpro = solver_kwargs.pop("p0_varpro", None)
        self.xtol = float(solver_kwargs.pop("xtol", 1e-8))
        self.gtol = float(solver_kwargs.pop("gtol", 1e-8))
        # sigma / absolute_sigma: the two curve_fit arguments the reference's docstring names (curvefit.py:33).  A scalar or 1-D
        # sigma (one standard deviation per b-value, shared by the voxels) runs in the kernel; a 2-D sigma (covariance matrix of
        # the measurements: SciPy whitens with its Cholesky factor) is not implemented and refused here, not per voxel
        self.sigma = solver_kwargs.pop("sigma", None)
        self.absolute_sigma = bool(solver_kwargs.pop("absolute_sigma", False))
        if self.sigma is not None:
            self.sigma = np.asarray(self.sigma, float)
            if self.sigma.ndim > 1 and self.sigma.size != 1:
                raise ValueError("HipCurveFitSolver implements a scalar or 1-D sigma (one standard deviation per b-value); "
                                 "a 2-D sigma is not implemented")
            self.sigma = self.sigma.reshape(-1)
            if fast:
                raise ValueError("precision='float32' is not built with sigma; use precision='float64'")
        for key, default in _CURVE_FIT_DEFAULTS.items():
            if key in solver_kwargs:
                v = solver_kwargs.pop(key)
                if not (v is default or v == default):
                    raise ValueError(f"HipCurveFitSolver does not implement curve_fit({key}={v!r}); only the SciPy "
                                     f"default ({default!r}) is supported")
        unknown = set(solver_kwargs) - {"n_pools"}
        if unknown:
            raise ValueError(f"HipCurveFitSolver got solver arguments it cannot honour: {sorted(unknown)} "
                             "(supported: sigma, absolute_sigma, xtol, gtol, jacobian, device, n_gpus, io_dtype, precision, p0_grid, "
                             "p0_grid_project, p0_peel, p0_varpro, n_pools)")
        if method != "trf":
            raise ValueError(f"HipCurveFitSolver implements method='trf' only (got {method!r}); "
                             "use the reference CurveFitSolver for 'dogbox' / 'lm'.")
        if HAVE_PYNEAPPLE:
            super().__init__(model=model, max_iter=max_iter, tol=tol, p0=p0, bounds=bounds, verbose=verbose,
                             method=method, multi_threading=multi_threading, use_jacobian=use_jacobian,
                             **solver_kwargs)
        else:
            RefBaseSolver.__init__(self, model=model, max_iter=max_iter, tol=tol, verbose=verbose)
            self.method = method
            self.multi_threading = multi_threading
            self.use_jacobian = use_jacobian and hasattr(model, "jacobian")
            self.n_pools = solver_kwargs.pop("n_pools", None)
            self.solver_kwargs = solver_kwargs
            # curvefit.py:75-89
            if isinstance(p0[self.model.param_names[0]], (int, float, np.ndarray)):
                _validate_parameter_names(p0, self.model.param_names)
                self.p0 = p0
            else:
                raise ValueError("p0 must be a dict with parameter names as keys and initial values as values.")
            if isinstance(bounds[self.model.param_names[0]], tuple):
                _validate_parameter_names(bounds, self.model.param_names)
                self.bounds = bounds
            else:
                raise ValueError(
                    "bounds must be a dict with parameter names as keys and (lower, upper) tuples as values.")
        self._kernel_model = kernel_model_key(model)  # fail early and loudly for unsupported models
        self._kernel_t1 = kernel_t1(model)
        if fast:
            if self._kernel_t1["t1_mode"]:
                raise ValueError("precision='float32' is not built with the T1 / STEAM factor; use precision='float64'")
            if getattr(model, "fixed_params", None):
                raise ValueError("precision='float32' is not built with fixed parameters; use precision='float64'")
        self._set_p0_grid(p0_grid, p0_grid_project)
        self._set_p0_peel(p0_peel)
        self._set_p0_varpro(p0_varpro)

    # ------------------------------------------------------------------ p0_grid: the atoms of the dictionary search
    def _set_p0_grid(self, p0_grid, project):
        """Validates `p0_grid` / `p0_grid_project` and builds the atoms (n_free, n_atoms); nothing is set up without p0_grid."""
        self.p0_grid, self.p0_grid_project, self._p0_atoms = None, False, None
        if p0_grid is None:
            if project:
                raise ValueError("p0_grid_project=True needs a p0_grid")
            return
        if self.precision == "float32" or self.io_dtype is not np.float64:
            raise ValueError("p0_grid is built for precision='float64' and io_dtype='float64': the dictionary search reads and "
                             "writes float64 arrays")
        self.p0_grid, self.p0_grid_project, self._p0_atoms = _grid_atoms("p0_grid", self.model, self._kernel_model, self.p0, self.bounds, p0_grid, project)

    # ------------------------------------------------------------------ p0_peel: start values from the peeling fit
    def _set_p0_peel(self, p0_peel):
        """Validates `p0_peel` ({"b_thresholds": [...], "weighting": "signal2"}); nothing is set up without it."""
        self.p0_peel = None
        if p0_peel is None:
            return
        if self._p0_atoms is not None:
            raise ValueError("p0_peel and p0_grid both choose the per-voxel start values; give one of them")
        if not isinstance(p0_peel, dict) or set(p0_peel) - {"b_thresholds", "weighting"}:
            raise ValueError("p0_peel must be a dict with the keys 'b_thresholds' and (optionally) 'weighting'")
        _peel_refusals("p0_peel", self.model)
        if self.precision == "float32" or self.io_dtype is not np.float64:
            raise ValueError("p0_peel is built for precision='float64' and io_dtype='float64': its start values are float64 arrays")
        weighting = p0_peel.get("weighting", "signal2")
        if weighting not in api.LOGLINEAR_WEIGHTING:
            raise ValueError(f"p0_peel: weighting must be one of {sorted(api.LOGLINEAR_WEIGHTING)}, got {weighting!r}")
        thresholds = p0_peel.get("b_thresholds")
        try:
            api.peel_masks(np.zeros(1), self._kernel_model, thresholds)  # count and order
        except ValueError as e:
            raise ValueError(f"p0_peel: {e}") from None
        self.p0_peel = {"b_thresholds": None if thresholds is None else [float(t) for t in np.atleast_1d(thresholds)],
                        "weighting": weighting}

    # ------------------------------------------------------------------ p0_varpro: start values from the variable projection
    def _set_p0_varpro(self, p0_varpro):
        """Validates `p0_varpro` ({"rates": {...}, "ordered": True}) and builds the atoms; nothing is set up without it."""
        self.p0_varpro, self._varpro_nl_atoms = None, None
        if p0_varpro is None:
            return
        if self._p0_atoms is not None or self.p0_peel is not None:
            raise ValueError("p0_varpro, p0_grid and p0_peel each choose the per-voxel start values; give one of them")
        if not isinstance(p0_varpro, dict) or "rates" not in p0_varpro or set(p0_varpro) - {"rates", "ordered"}:
            raise ValueError("p0_varpro must be a dict with the keys 'rates' and (optionally) 'ordered'")
        if self.precision == "float32" or self.io_dtype is not np.float64:
            raise ValueError("p0_varpro is built for precision='float64' and io_dtype='float64': the variable projection reads and "
                             "writes float64 arrays")
        ordered = bool(p0_varpro.get("ordered", True))
        rates, _, self._varpro_nl_atoms = _varpro_atoms("p0_varpro['rates']", self.model, self._kernel_model, self.p0, self.bounds,
                                                        p0_varpro["rates"], ordered)
        self.p0_varpro = {"rates": rates, "ordered": ordered}

    # ------------------------------------------------------------------ p0 / bounds (curvefit.py:319-392)
    def _prepare_p0_bounds(self, p0, bounds, n_pixels):
        names = self.model.param_names
        if p0 is not None:
            if isinstance(p0, dict):
                first = p0[names[0]]
                if isinstance(first, np.ndarray):
                    raise ValueError(
                        "p0 should either be a basic dict with scalar values or a single np.ndarray of initial values "
                        "for all parameters. Spatial non-uniform p0 should be handled separately before calling fit().")
                elif isinstance(first, (int, float)):
                    _validate_parameter_names(p0, names)
                    p0 = np.array([p0[n] for n in names], dtype=float)
                else:
                    raise ValueError("p0 dict values must be either all scalars or a single np.ndarray of initial "
                                     "values for all parameters.")
            elif isinstance(p0, np.ndarray):
                pass
            else:
                raise ValueError("p0 must be either a dict or a single np.ndarray.")
        else:
            _validate_parameter_names(self.p0, names)
            p0 = np.array([self.p0[n] for n in names], dtype=float)

        if bounds is not None:
            if isinstance(bounds, dict):
                if isinstance(bounds[names[0]], tuple):
                    _validate_parameter_names(bounds, names)
                    bounds = (np.array([bounds[n][0] for n in names], float),
                              np.array([bounds[n][1] for n in names], float))
                else:
                    raise ValueError("bounds dict values must be tuples of (lower, upper) for each parameter.")
            elif isinstance(bounds, tuple) and len(bounds) == 2:
                if not all(isinstance(b, np.ndarray) for b in bounds):
                    raise ValueError("bounds tuple must contain two np.ndarrays (lower, upper) of shape "
                                     "(n_params, n_pixels).")
            else:
                raise ValueError("bounds must be either a dict with parameter names as keys and (lower, upper) tuples "
                                 "as values, or a tuple of (lower, upper) np.ndarrays.")
        else:
            _validate_parameter_names(self.bounds, names)
            bounds = (np.array([self.bounds[n][0] for n in names], float),
                      np.array([self.bounds[n][1] for n in names], float))

        # the reference tiles everything to (n_params, n_pixels); shared vectors stay (n_params,) here
        # and the tiling happens implicitly on the device
        if p0.ndim == 2 and p0.shape[1] != n_pixels:
            raise ValueError(f"p0 shape {p0.shape} does not match number of voxels in ydata {n_pixels}.")
        lo, hi = bounds
        for arr in (lo, hi):
            if arr.ndim == 2 and arr.shape[1] != n_pixels:
                raise ValueError(
                    f"bounds shape {lo.shape} and {hi.shape} do not match number of voxels in ydata {n_pixels}.")
        per_voxel = p0.ndim == 2 or lo.ndim == 2 or hi.ndim == 2
        if per_voxel:
            def tile(a):
                a = np.asarray(a, float)
                return np.ascontiguousarray(a if a.ndim == 2 else np.repeat(a[:, None], n_pixels, axis=1))
            p0, lo, hi = tile(p0), tile(lo), tile(hi)
        return np.asarray(p0, float), np.asarray(lo, float), np.asarray(hi, float), per_voxel

    # ------------------------------------------------------------------ device memory kept between fits
    def close(self) -> None:
        """Give back what host-array fits keep on the device between calls: the staging slab of a streamed fit (the size of the
        volume: 2.1 GB for 256 x 256 x 64 x 32), its pinned block and its streams (`pnx_release_staging`).  The next fit builds
        them again (2-3 ms).  Called when the solver is garbage collected; safe to call twice."""
        if getattr(self, "_closed", True):
            return
        self._closed = True
        for dev in sorted({_shard_device(int(self.device), k) for k in range(max(1, int(getattr(self, "n_gpus", 1))))}):
            try:  # per device: one that is busy (another solver's call is using the set) or gone must not keep the others' slabs alive
                api.release_staging(dev)
            except Exception:
                pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    # ------------------------------------------------------------------ fit (curvefit.py:91-159)
    def fit(self, xdata: np.ndarray, ydata: np.ndarray, p0=None, bounds=None,
            pixel_fixed_params: dict[str, np.ndarray] | None = None, **fit_kwargs) -> "HipCurveFitSolver":
        self._closed = False  # from here on there may be something to give back
        # **fit_kwargs: accepted and unused, exactly like the reference (curvefit.py:91-159 never reads them)
        self._reset_state()
        xdata = np.asarray(xdata)
        ydata = np.asarray(ydata)
        _validate_data_shapes(xdata, ydata)
        n_pixels = ydata.shape[0] if ydata.ndim > 1 else 1
        if ydata.ndim == 1:
            ydata = ydata[np.newaxis, :]
        if ydata.ndim > 2:
            raise ValueError(f"ydata must be 1D or 2D array, but got shape {ydata.shape}.")
        p0_a, lo_a, hi_a, per_voxel = self._prepare_p0_bounds(p0, bounds, n_pixels)
        if self.sigma is not None and self.sigma.size not in (1, xdata.shape[0]):
            # curve_fit raises "`sigma` has incorrect shape." (scipy:_minpack_py.py:969), which the reference turns into a failed
            # fit of every voxel with one warning each (curvefit.py:308-317); a usage error is reported once here instead
            raise ValueError(f"`sigma` has incorrect shape: {self.sigma.size} values for {xdata.shape[0]} b-values.")

        all_names = list(self.model._all_param_names)
        # curvefit.py:274: per-pixel fixed values win, else the model's scalar fixed parameters
        fixed = pixel_fixed_params if pixel_fixed_params else (getattr(self.model, "fixed_params", None) or None)
        free_names = list(self.model.param_names)
        fixed_idx, fixed_vals, jac = [], None, self.jacobian_mode
        if fixed and self.precision == "float32":
            raise ValueError("precision='float32' is not built with fixed parameters (pixel_fixed_params); use precision='float64'")
        if fixed:
            free_idx = [i for i, n in enumerate(all_names) if n not in fixed]
            fixed_idx = [i for i, n in enumerate(all_names) if n in fixed]
            if len(free_idx) < p0_a.shape[0]:  # curvefit.py:285-288
                p0_a, lo_a, hi_a = p0_a[free_idx], lo_a[free_idx], hi_a[free_idx]
            if pixel_fixed_params:
                free_names = [n for n in free_names if n not in pixel_fixed_params]
                fv = []
                for i in fixed_idx:
                    v = np.asarray(fixed[all_names[i]], float)
                    if v.shape != (n_pixels,):
                        raise ValueError(f"pixel_fixed_params[{all_names[i]!r}] must have shape ({n_pixels},)")
                    fv.append(v)
                fixed_vals = np.ascontiguousarray(np.stack(fv, axis=0))
            else:
                fixed_vals = np.array([float(fixed[all_names[i]]) for i in fixed_idx])
            jac = "analytic"  # the reference passes model.jacobian_with_fixed here (curvefit.py:279-281)

        grid = self._p0_atoms is not None and p0 is None  # an explicit p0 wins (IDEAL and Segmented pass their own)
        if grid:
            if pixel_fixed_params:
                raise ValueError("p0_grid is not built with per-pixel fixed parameters (the dictionary would differ from voxel to voxel)")
            if per_voxel:
                raise ValueError("p0_grid works with shared bounds: one dictionary serves the whole call")
        peel = self.p0_peel is not None
        if peel:  # the start of every voxel is the peel estimate; a shared p0 (the solver's, or fit()'s) serves the failed voxels
            if isinstance(p0, np.ndarray) and p0.ndim == 2:
                raise ValueError("p0_peel chooses the per-voxel start values itself: an explicit per-voxel p0 cannot be honoured")
            if pixel_fixed_params or fixed:
                raise ValueError("p0_peel is not built with fixed parameters (pixel_fixed_params): every stage fits its own "
                                 "amplitude and diffusivity")
            if per_voxel:
                raise ValueError("p0_peel works with shared bounds: the peel estimate is clipped into one box for the whole call")
        varpro = self.p0_varpro is not None
        if varpro:  # as p0_peel: a shared p0 (the solver's, or fit()'s) serves the voxels with a non-finite signal
            if isinstance(p0, np.ndarray) and p0.ndim == 2:
                raise ValueError("p0_varpro chooses the per-voxel start values itself: an explicit per-voxel p0 cannot be honoured")
            if pixel_fixed_params:
                raise ValueError("p0_varpro is not built with per-pixel fixed parameters (the dictionary would differ from voxel to voxel)")
            if per_voxel:
                raise ValueError("p0_varpro works with shared bounds: one dictionary serves the whole call")
        res = self._run(xdata, np.ascontiguousarray(ydata, self.io_dtype), p0_a, lo_a, hi_a, per_voxel, fixed_idx,
                        fixed_vals, jac, grid, peel, varpro)
        self._pack(res, n_pixels, free_names)
        return self

    def _pack(self, res, n_pixels, free_names):
        """Result dict of the batch call -> the reference's solver state (curvefit.py:150-159, 214-244)."""
        popt, pcov, status = res["popt"], res["pcov"], res["status"]
        success = status > 0
        params_rows = popt.T  # (n_px, n_free) strided view: a record's params is one column of popt, no 168 MB transpose
        self.pixel_results_ = PixelResultsView(
            params_rows, pcov, success,
            lambda i, st=status: None if st[i] > 0 else _CURVEFIT_MESSAGES.get(int(st[i]), "fit failed"))
        self.params_ = {name: [float(popt[i, 0])] if n_pixels == 1 else popt[i] for i, name in enumerate(free_names)}
        self.diagnostics_ = {"pcov": (pcov[0] if n_pixels == 1 else pcov) if pcov is not None else None, "n_pixels": n_pixels,
                             "status": status, "nfev": res["nfev"], "cost": res["cost"]}
        for key in ("p0_atom", "p0_cost", "p0_status", "p0_clipped"):  # a fit that started from p0_grid / p0_peel / p0_varpro
            if key in res:
                self.diagnostics_[key] = res[key]

    _extra_outputs: dict = {}  # further per-voxel result arrays of a subclass's batch call: key -> dtype

    def _batch_fit(self, *args, **kw):
        """The array-level call of one shard (a subclass swaps in another one with api.curvefit's signature)."""
        return api.curvefit(*args, **kw)

    def _grid_fit(self, xdata, ydata, lo, hi, fixed_vals, device, kw, out=None):
        """One shard with p0_grid: the dictionary search, then the fit from its per-voxel start values under the shared bounds."""
        out = out or {}
        gs = api.grid_start(self._kernel_model, xdata, ydata, self._p0_atoms, lo, hi, fixed_idx=kw["fixed_idx"], fixed_vals=fixed_vals,
                            sigma=self.sigma, project_amplitude=self.p0_grid_project, device=device, **self._kernel_t1,
                            out={"best": out.get("p0_atom"), "cost": out.get("p0_cost")})
        tile = lambda a: np.ascontiguousarray(np.repeat(a[:, None], ydata.shape[0], axis=1))
        res = self._batch_fit(self._kernel_model, xdata, ydata, gs["p0"], tile(lo), tile(hi), fixed_vals=fixed_vals, device=device,
                              out=out or None, **kw)
        return dict(res, p0_atom=gs["best"], p0_cost=gs["cost"])

    def _peel_fit(self, xdata, ydata, p0, lo, hi, device, kw, out=None):
        """One shard with p0_peel: the peeling fit clipped into the shared bounds (failed voxels: the shared p0), then the fit from
        these per-voxel start values.  A start that the clip left exactly on a bound is moved inside by the fit itself, as
        SciPy's least_squares does (make_strictly_feasible, rstep 1e-10)."""
        out = out or {}
        pe = api.peel(xdata, ydata, self._kernel_model, b_thresholds=self.p0_peel["b_thresholds"], weighting=self.p0_peel["weighting"],
                      clip=(lo, hi), fallback=p0, device=device, out={"status": out.get("p0_status")})
        tile = lambda a: np.ascontiguousarray(np.repeat(a[:, None], ydata.shape[0], axis=1))
        res = self._batch_fit(self._kernel_model, xdata, ydata, pe["params"], tile(lo), tile(hi), fixed_vals=None, device=device,
                              out=out or None, **kw)
        return dict(res, p0_status=pe["status"])

    def _varpro_fit(self, xdata, ydata, p0, lo, hi, fixed_vals, device, kw, out=None):
        """One shard with p0_varpro: the variable-projection estimate (a non-finite voxel: the shared p0), then the fit from these
        per-voxel start values under the shared bounds.  A start on a bound is moved inside by the fit itself, as p0_peel's."""
        out = out or {}
        vp = api.varpro(self._kernel_model, xdata, ydata, self._varpro_nl_atoms, lo, hi, p0, fixed_idx=kw["fixed_idx"], fixed_vals=fixed_vals,
                        sigma=self.sigma, device=device, **self._kernel_t1,
                        out={"atom": out.get("p0_atom"), "cost": out.get("p0_cost"), "clipped": out.get("p0_clipped")})
        tile = lambda a: np.ascontiguousarray(np.repeat(a[:, None], ydata.shape[0], axis=1))
        res = self._batch_fit(self._kernel_model, xdata, ydata, vp["params"], tile(lo), tile(hi), fixed_vals=fixed_vals, device=device,
                              out=out or None, **kw)
        return dict(res, p0_atom=vp["atom"], p0_cost=vp["cost"], p0_clipped=vp["clipped"])

    def _run(self, xdata, ydata, p0, lo, hi, per_voxel, fixed_idx, fixed_vals, jac, grid=False, peel=False, varpro=False):
        n_vox = ydata.shape[0]
        kw = dict(max_nfev=int(self.max_iter), ftol=float(self.tol), xtol=self.xtol, gtol=self.gtol, jac=jac,
                  fixed_idx=fixed_idx, sigma=self.sigma, absolute_sigma=self.absolute_sigma, **self._kernel_t1)
        if self.precision == "float32":
            kw["precision"] = "float32"
        n_dev = max(1, min(self.n_gpus, n_vox))
        if n_dev == 1:
            if grid:
                return self._grid_fit(xdata, ydata, lo, hi, fixed_vals, self.device, kw)
            if peel:
                return self._peel_fit(xdata, ydata, p0, lo, hi, self.device, kw)
            if varpro:
                return self._varpro_fit(xdata, ydata, p0, lo, hi, fixed_vals, self.device, kw)
            return self._batch_fit(self._kernel_model, xdata, ydata, p0, lo, hi, fixed_vals=fixed_vals,
                                   device=self.device, **kw)
        parts = _split(n_vox, n_dev)
        # the shards write their voxel-major results straight into row ranges of the full arrays (pcov is 200 B per triexp voxel:
        # concatenating it afterwards would cost more than the fit); popt is parameter-major and is joined afterwards
        n = p0.shape[0]
        dt = ydata.dtype
        full = {"pcov": np.empty((n_vox, n, n), dt), "status": np.empty(n_vox, np.int8), "nfev": np.empty(n_vox, np.int32),
                "cost": np.empty(n_vox, dt), **{key: np.empty(n_vox, d) for key, d in self._extra_outputs.items()}}
        if grid:
            full.update(p0_atom=np.empty(n_vox, np.int32), p0_cost=np.empty(n_vox, np.float64))
        if peel:
            full.update(p0_status=np.empty(n_vox, np.int8))
        if varpro:
            full.update(p0_atom=np.empty(n_vox, np.int32), p0_cost=np.empty(n_vox, np.float64), p0_clipped=np.empty(n_vox, np.int8))

        def work(k):
            a, b = parts[k]
            sl = slice(a, b)
            fv = fixed_vals
            if fv is not None and fv.ndim == 2:
                fv = np.ascontiguousarray(fv[:, sl])
            pv = (np.ascontiguousarray(p0[:, sl]), np.ascontiguousarray(lo[:, sl]),
                  np.ascontiguousarray(hi[:, sl])) if per_voxel else (p0, lo, hi)
            dev_k = _shard_device(self.device, k)
            with pinned_to_gpu(dev_k):  # this thread and the call's helper threads stay on the NUMA node of their GPU
                if grid:
                    return self._grid_fit(xdata, ydata[sl], lo, hi, fv, dev_k, kw, out={key: v[sl] for key, v in full.items()})["popt"]
                if peel:
                    return self._peel_fit(xdata, ydata[sl], p0, lo, hi, dev_k, kw, out={key: v[sl] for key, v in full.items()})["popt"]
                if varpro:
                    return self._varpro_fit(xdata, ydata[sl], p0, lo, hi, fv, dev_k, kw, out={key: v[sl] for key, v in full.items()})["popt"]
                return self._batch_fit(self._kernel_model, xdata, ydata[sl], *pv, fixed_vals=fv,
                                       device=dev_k, out={key: v[sl] for key, v in full.items()}, **kw)["popt"]

        with ThreadPoolExecutor(len(parts)) as ex:  # ctypes releases the GIL during the call
            popts = list(ex.map(work, range(len(parts))))
        return dict(full, popt=np.concatenate(popts, axis=1))


class HipConstrainedCurveFitSolver(HipCurveFitSolver):
    """`HipCurveFitSolver` with the volume-fraction constraint sum(f_i) <= 1 of the reference's ConstrainedCurveFitSolver
    (solvers/constrained_curvefit.py:23-119), same constructor contract: `p0` and `bounds` come first, `fraction_constraint=True`
    needs a `fit_reduced` model with at least two fraction parameters (names starting with "f") -- the reduced tri-exponential
    models [f1, D1, f2, D2, D3 (, S0)] --, `fraction_constraint=False` behaves as the parent, `method` is accepted and ignored.

    The constrained PROBLEM is solved, not the reference's SLSQP iteration (pnx_curvefit_simplex_f64): the parent's bounded fit;
    voxels whose result has f1 + f2 > 1 are fitted again on the face f1 + f2 = 1 (the bi-exponential model) and certified by
    the multiplier of the constraint.  `diagnostics_` gains "lambda" (0 for an interior voxel) and "face" (0 interior: the
    parent's result bit for bit; 1 face, lambda >= 0; 2 face, not certified); pcov of a face voxel is NaN.
    Not built with the constraint, hence a ValueError: fixed parameters (model or per pixel), a T1 model, sigma,
    precision / io_dtype "float32".  Extra keyword arguments as the parent's."""

    def __init__(self, model: Any, p0: dict[str, float], bounds: dict[str, tuple[float, float]], max_iter: int = 250,
                 tol: float = 1e-8, fraction_constraint: bool = True, verbose: bool = False, method: str = "SLSQP",
                 multi_threading: bool = False, use_jacobian: bool = True, **solver_kwargs):
        if solver_kwargs.get("p0_grid") is not None or solver_kwargs.get("p0_grid_project") is not None:
            raise ValueError("p0_grid is not built for HipConstrainedCurveFitSolver: the dictionary knows nothing of the constraint "
                             "f1 + f2 <= 1 and the constrained fit takes one shared start; use HipCurveFitSolver")
        if solver_kwargs.get("p0_peel") is not None:
            raise ValueError("p0_peel is not built for HipConstrainedCurveFitSolver: the peel estimate knows nothing of the constraint "
                             "f1 + f2 <= 1 and the constrained fit takes one shared start; use HipCurveFitSolver")
        if solver_kwargs.get("p0_varpro") is not None:
            raise ValueError("p0_varpro is not built for HipConstrainedCurveFitSolver: the projected amplitudes know nothing of the "
                             "constraint f1 + f2 <= 1 and the constrained fit takes one shared start; use HipCurveFitSolver")
        if fraction_constraint and not getattr(model, "fit_reduced", False):  # constrained_curvefit.py:72-79
            raise ValueError("fraction_constraint=True requires fit_reduced=True. In reduced mode the signal is normalised to S0=1 "
                             "before fitting, so the hard constraint sum(f_i) <= 1 is physically meaningful. Use fit_reduced=True "
                             "(or fit_s0=True) with the constrained solver.")
        super().__init__(model=model, max_iter=max_iter, tol=tol, p0=p0, bounds=bounds, verbose=verbose, method="trf",
                         multi_threading=multi_threading, use_jacobian=use_jacobian, **solver_kwargs)
        self.method = "SLSQP"  # the reference's attribute value (constrained_curvefit.py:96); no SLSQP runs here
        self.fraction_constraint = bool(fraction_constraint)
        self._fraction_names = [n for n in self.model.param_names if n.startswith("f")] if fraction_constraint else []
        self._fraction_indices = [self.model.param_names.index(n) for n in self._fraction_names]
        if not fraction_constraint:
            return
        if len(self._fraction_names) < 2:
            raise ValueError(f"fraction_constraint=True requires at least 2 fraction parameters. Found: {self._fraction_names}")
        if self._kernel_model not in api.CONSTRAINED_MODELS:
            raise ValueError(f"the constrained fit is built for the models {api.CONSTRAINED_MODELS}, not {self._kernel_model!r}")
        if self.precision != "float64" or self.io_dtype is not np.float64:
            raise ValueError("the constrained fit is built for precision='float64' and io_dtype='float64' only")
        if self.sigma is not None:
            raise ValueError("the constrained fit is not built with sigma")
        if self._kernel_t1["t1_mode"]:
            raise ValueError("the constrained fit is not built with the T1 / STEAM factor")
        if getattr(model, "fixed_params", None):
            raise ValueError("the constrained fit is not built with fixed parameters")
        self._extra_outputs = {"lambda": np.float64, "face": np.int8}

    def _batch_fit(self, *args, **kw):
        return api.curvefit_constrained(*args, **kw) if self.fraction_constraint else api.curvefit(*args, **kw)

    def fit(self, xdata, ydata, p0=None, bounds=None, pixel_fixed_params=None, **fit_kwargs):
        if self.fraction_constraint and (pixel_fixed_params or getattr(self.model, "fixed_params", None)):
            raise ValueError("the constrained fit is not built with fixed parameters (pixel_fixed_params)")
        return super().fit(xdata, ydata, p0=p0, bounds=bounds, pixel_fixed_params=pixel_fixed_params, **fit_kwargs)

    def _pack(self, res, n_pixels, free_names):
        super()._pack(res, n_pixels, free_names)
        for key in self._extra_outputs:
            self.diagnostics_[key] = res[key]


_LOGLINEAR_MESSAGES = {0: "Fewer than two usable (positive) samples at distinct b-values: no line to fit.",
                       -2: "array must not contain infs or NaNs"}


class HipLogLinearSolver(RefBaseSolver):
    """Linearised mono-exponential fit ln S = ln S0 - b D by (weighted) linear least squares per voxel (pnx_loglinear_f64,
    include/pnx.h): the ADC map, step 1 of a segmented IVIM fit, a cheap source of S0 / D start values.  Registered as
    `hip_loglinear`.

    model: the plain mono-exponential layout ([S0, D], nothing fixed, no T1 / STEAM factor).  `max_iter` and `tol` are accepted
    because the TOML loader always passes them; a closed form has no use for either.  Keyword arguments:
        p0: None or {"S0": .., "D": ..}: what a voxel that could not be fitted (status <= 0) reports as its parameters, the
            reference's failure convention (NaN without p0).
        bounds: None or {"S0": (lo, hi), "D": (lo, hi)}; read only with clip=True.
        weighting: "signal2" (default, w = y^2: the usual weights of log-transformed data) or "none".
        n_reweight: 0 .. 8 further passes with the weights of the estimate before (iteratively re-weighted LLS).
        clip: clip S0 and D into `bounds` after the fit (status 2 for a voxel that was moved).
        device, io_dtype ("float32": float32 arrays across the ABI, fp64 arithmetic) as HipCurveFitSolver's.
    Any other keyword (the reference's solver arguments: method, multi_threading, ...) is accepted and ignored.
    fit(xdata, ydata, bvalue_mask=None): `bvalue_mask` (n_b,) bool restricts the fit to a subset of the b-values without slicing
    the signal array.  After fit: params_ {"S0", "D"}, diagnostics_ {"pcov", "n_pixels", "status", "n_used", "ss_res"} (ss_res in
    the signal domain over the masked-in samples), pixel_results_."""

    supports_bvalue_mask = True

    def __init__(self, model: Any, max_iter: int = 250, tol: float = 1e-8, p0: dict[str, float] | None = None,
                 bounds: dict[str, tuple[float, float]] | None = None, weighting: str = "signal2", n_reweight: int = 0,
                 clip: bool = False, device: int = 0, io_dtype: str = "float64", **ignored_reference_kwargs):
        RefBaseSolver.__init__(self, model=model, max_iter=max_iter, tol=tol, verbose=bool(ignored_reference_kwargs.pop("verbose", False)))
        names = list(getattr(model, "_all_param_names", []))
        if names != ["S0", "D"] or getattr(model, "fixed_params", None) or kernel_t1(model)["t1_mode"]:
            raise ValueError(f"HipLogLinearSolver fits the plain mono-exponential model [S0, D] (nothing fixed, no T1 / STEAM factor), "
                             f"not {type(model).__name__} with parameters {names} and fixed {dict(getattr(model, 'fixed_params', None) or {})}")
        if weighting not in api.LOGLINEAR_WEIGHTING:
            raise ValueError(f"weighting must be one of {sorted(api.LOGLINEAR_WEIGHTING)}, got {weighting!r}")
        if not 0 <= int(n_reweight) <= api.LOGLINEAR_MAX_REWEIGHT:
            raise ValueError(f"n_reweight must lie in 0 .. {api.LOGLINEAR_MAX_REWEIGHT}, got {n_reweight}")
        for name, d in (("p0", p0), ("bounds", bounds)):
            if d is not None:
                _validate_parameter_names(d, names)
        if clip and bounds is None:
            raise ValueError("clip=True needs bounds: {'S0': (lo, hi), 'D': (lo, hi)}")
        self.p0 = p0
        self.bounds = bounds
        self.weighting = weighting
        self.n_reweight = int(n_reweight)
        self.clip = bool(clip)
        self.device = int(device)
        self.io_dtype = _io_dtype(io_dtype)
        self.solver_kwargs = ignored_reference_kwargs

    def fit(self, xdata: np.ndarray, ydata: np.ndarray, bvalue_mask=None, pixel_fixed_params=None, **fit_kwargs) -> "HipLogLinearSolver":
        if pixel_fixed_params:
            raise ValueError("HipLogLinearSolver fits both parameters of the line: pixel_fixed_params cannot be honoured")
        self._reset_state()
        xdata = np.asarray(xdata)
        ydata = np.asarray(ydata)
        _validate_data_shapes(xdata, ydata)
        if ydata.ndim == 1:
            ydata = ydata[np.newaxis, :]
        if ydata.ndim > 2:
            raise ValueError(f"ydata must be 1D or 2D array, but got shape {ydata.shape}.")
        n_pixels = ydata.shape[0]
        clip = None
        if self.clip:
            clip = ([self.bounds["S0"][0], self.bounds["D"][0]], [self.bounds["S0"][1], self.bounds["D"][1]])
        res = api.loglinear(xdata, np.ascontiguousarray(ydata, self.io_dtype), bvalue_mask=bvalue_mask, weighting=self.weighting,
                            n_reweight=self.n_reweight, clip=clip, device=self.device)
        params, pcov, status = res["params"], res["pcov"], res["status"]
        success = status > 0
        if self.p0 is not None and not success.all():  # the reference's failure convention: p0, NaN covariance (already NaN)
            params[0, ~success] = float(self.p0["S0"])
            params[1, ~success] = float(self.p0["D"])
        self.pixel_results_ = PixelResultsView(
            params.T, pcov, success,
            lambda i, st=status: None if st[i] > 0 else _LOGLINEAR_MESSAGES.get(int(st[i]), "fit failed"))
        self.params_ = {name: [float(params[i, 0])] if n_pixels == 1 else params[i] for i, name in enumerate(("S0", "D"))}
        self.diagnostics_ = {"pcov": pcov[0] if n_pixels == 1 else pcov, "n_pixels": n_pixels, "status": status,
                             "n_used": res["n_used"], "ss_res": res["ss_res"]}
        return self


_PEEL_MESSAGES = {0: "A peeling stage had fewer than two positive residuals at distinct b-values: no line to fit.",
                  -2: "array must not contain infs or NaNs"}


def _peel_refusals(who, model):
    """What the peeling fit is not built with, refused by name: the T1 / STEAM factor and fixed parameters."""
    if kernel_t1(model)["t1_mode"]:
        raise ValueError(f"{who} is not built with the T1 / STEAM factor (fit_t1 / fit_t1_steam)")
    if getattr(model, "fixed_params", None):
        raise ValueError(f"{who} is not built with fixed parameters (fixed_params {dict(model.fixed_params)}): every stage fits its own "
                         "amplitude and diffusivity")


class HipPeelSolver(RefBaseSolver):
    """Exponential peeling ("curve stripping", the fully segmented IVIM estimate) of a mono-, bi- or tri-exponential model per voxel
    (pnx_peel_f64, include/pnx.h): the slowest compartment is fitted log-linearly on the high b-values and subtracted, the next
    faster one on what is left of the lower b-values, once more for a third.  Registered as `hip_peel`; no counterpart in the
    reference, whose solver contract it keeps.

    model: any of the seven layouts, nothing fixed, no T1 / STEAM factor.  `max_iter` and `tol` are accepted because the TOML loader
    always passes them; a closed form has no use for either.  Keyword arguments:
        b_thresholds: K - 1 ascending b-values for K exponentials (api.peel_masks): the slowest compartment is fitted on
            b >= the last threshold, the fastest on b < the first.  Not needed for the mono-exponential model.
        weighting: "signal2" (default, w = r^2) or "none".
        bounds: None or {name: (lo, hi)} for every parameter: the result is clipped into them (status 2 for a voxel that was moved).
        p0: None or {name: value}: what a voxel that could not be fitted (status <= 0) reports as its parameters, the reference's
            failure convention (NaN without p0).
        device, io_dtype ("float32": float32 arrays across the ABI, fp64 arithmetic) as HipCurveFitSolver's.
    Any other keyword (the reference's solver arguments: method, multi_threading, ...) is accepted and ignored.
    After fit: params_ keyed by the model's names, diagnostics_ {"n_pixels", "status", "n_used" (K, n_pixels), "ss_res"} (ss_res in
    the signal domain over the b-values of every stage), pixel_results_ (no covariance: peeling has no honest closed form)."""

    def __init__(self, model: Any, max_iter: int = 250, tol: float = 1e-8, p0: dict[str, float] | None = None,
                 bounds: dict[str, tuple[float, float]] | None = None, b_thresholds=None, weighting: str = "signal2", device: int = 0,
                 io_dtype: str = "float64", **ignored_reference_kwargs):
        RefBaseSolver.__init__(self, model=model, max_iter=max_iter, tol=tol, verbose=bool(ignored_reference_kwargs.pop("verbose", False)))
        _peel_refusals("HipPeelSolver", model)
        self._kernel_model = kernel_model_key(model)
        names = api.MODEL_PARAM_NAMES[self._kernel_model]
        if weighting not in api.LOGLINEAR_WEIGHTING:
            raise ValueError(f"weighting must be one of {sorted(api.LOGLINEAR_WEIGHTING)}, got {weighting!r}")
        K = api.PEEL_STAGES[self._kernel_model]
        if K > 1 and b_thresholds is None:
            raise ValueError(f"b_thresholds is required: {K - 1} ascending b-values that separate the {K} compartments")
        api.peel_masks(np.zeros(1), self._kernel_model, b_thresholds)  # count and order of b_thresholds
        for d in (p0, bounds):
            if d is not None:
                _validate_parameter_names(d, names)
        self.p0 = p0
        self.bounds = bounds
        self.b_thresholds = None if b_thresholds is None else [float(t) for t in np.atleast_1d(b_thresholds)]
        self.weighting = weighting
        self.device = int(device)
        self.io_dtype = _io_dtype(io_dtype)
        self.solver_kwargs = ignored_reference_kwargs

    def fit(self, xdata: np.ndarray, ydata: np.ndarray, pixel_fixed_params=None, **fit_kwargs) -> "HipPeelSolver":
        if pixel_fixed_params:
            raise ValueError("HipPeelSolver fits every parameter of its stages: pixel_fixed_params cannot be honoured")
        self._reset_state()
        xdata = np.asarray(xdata)
        ydata = np.asarray(ydata)
        _validate_data_shapes(xdata, ydata)
        if ydata.ndim == 1:
            ydata = ydata[np.newaxis, :]
        if ydata.ndim > 2:
            raise ValueError(f"ydata must be 1D or 2D array, but got shape {ydata.shape}.")
        n_pixels = ydata.shape[0]
        names = api.MODEL_PARAM_NAMES[self._kernel_model]
        clip = None if self.bounds is None else ([self.bounds[n][0] for n in names], [self.bounds[n][1] for n in names])
        fallback = None if self.p0 is None else [float(self.p0[n]) for n in names]
        res = api.peel(xdata, np.ascontiguousarray(ydata, self.io_dtype), self._kernel_model, b_thresholds=self.b_thresholds,
                       weighting=self.weighting, clip=clip, fallback=fallback, device=self.device)
        params, status = res["params"], res["status"]
        self.pixel_results_ = PixelResultsView(
            params.T, None, status > 0, lambda i, st=status: None if st[i] > 0 else _PEEL_MESSAGES.get(int(st[i]), "fit failed"))
        self.params_ = {name: [float(params[i, 0])] if n_pixels == 1 else params[i] for i, name in enumerate(names)}
        self.diagnostics_ = {"n_pixels": n_pixels, "status": status, "n_used": res["n_used"], "ss_res": res["ss_res"]}
        return self


_BAYES_MESSAGES = {-2: "array must not contain infs or NaNs",
                   -4: "refine: no atom of the fine grid is admitted (the box lies beyond f1 + f2 = 1)"}


class HipBayesGridSolver(RefBaseSolver):
    """Bayesian grid fit per voxel (pnx_curvefit_grid_posterior_f64, include/pnx.h): posterior mean and standard deviation of every
    parameter over a grid of parameter vectors, with a per-atom prior table and a known or marginalised noise scale -- the estimator
    for noisy IVIM data, where a non-linear fit ends in a tail of stragglers and a point estimate says nothing of its uncertainty.
    No iteration: the cost does not depend on the noise.  Registered as `hip_bayes_grid`; no counterpart in the reference, whose
    solver contract it keeps.

    model: any of the seven layouts, with shared fixed parameters and the T1 / STEAM factor as the curve fit takes them.  `max_iter`,
    `tol` are accepted because the TOML loader always passes them; a closed form has no use for either.  Arguments:
        grid: dict from parameter name to a sequence of values, the meaning and the rules of HipCurveFitSolver's `p0_grid`: the
            atoms are the Cartesian product in `model.param_names` order, the last parameter fastest; a parameter the dict does not
            name takes its scalar `p0`; every value inside `bounds`; at most 4096 atoms.
        p0: {name: value} for the parameters `grid` does not name.  bounds: {name: (lo, hi)} for every parameter.
        noise_sd: None / 0 (default) marginalises the noise scale under a Jeffreys prior; > 0 is a known Gaussian noise sd in the
            units of the (sigma-weighted) signal.
        log_prior: None (uniform) or (n_atoms,) log weights in the order of the atoms (itertools.product over `model.param_names`);
            -inf excludes an atom.  Or (n_classes, n_atoms), n_classes <= 16: one row per segmentation label
            (pnx_curvefit_grid_posterior_classes_f64); `fit` then needs `labels`, and row c serves the voxels whose label is c.
        project: fit the amplitude S0 per voxel and atom, clipped to its bounds, instead of taking it from the grid.  Default:
            True exactly when the model has a free S0 (as p0_grid_project).
        sigma: None, a scalar or (n_b,), as HipCurveFitSolver's.  device: HIP device index.
        empirical_prior: None / False (default): the posterior under `log_prior`, as before.  True, or a dict with any of
            {"n_iter": 20, "pseudo_count": 0.0, "rel_tol": 1e-6, "max_voxels": None} (TOML: a table [Fitting.solver.empirical_prior];
            an unknown key is a ValueError): `fit` first learns the prior over the atoms from `ydata` itself by EM
            (pnx_curvefit_grid_prior_em_f64: the maximum-likelihood mixture over the grid), started from `log_prior`, then reports
            every voxel's posterior under the learned table.  max_voxels: learn from the evenly strided subset
            ydata[::step], step = ceil(n_pixels / max_voxels).  The prior is learned from the very voxels it is applied to and
            needs many of them: on a narrow population, 1000 voxels at 5 % noise halve the median error of f1 and D1 against the
            uniform prior, while 37 voxels against 384 atoms fit their own noise and the gain is unreliable or gone (DESIGN.md
            4.1j); where the truths are uniform over the grid's ranges it does not help.  `self.log_prior` stays the caller's
            prior; the learned one is in diagnostics_ only.
            "per_label": True (TOML: [Fitting.solver.empirical_prior] per_label = true) learns one table per segmentation label
            instead (pnx_curvefit_grid_prior_em_classes_f64: the narrow-population case, per tissue): `fit` needs `labels`
            (n_pixels,) integers -- HipPixelWiseFitter passes segmentation[mask] --, maps the distinct non-negative label values of
            the call to rows 0..C-1 in ascending order (diagnostics_["prior_labels"]; more than 16 of them is a ValueError; a
            negative label is background: NaN results, success False) and starts every row from `log_prior` (a 2-D `log_prior`
            must then have C rows).  Each label needs as many voxels as a whole volume does for the single table.  Not built with
            per-label priors: `marginals` and max_voxels (a ValueError that says so), hip_bayes_varpro, neighbourhood (MRF) priors.
        spatial_prior: None / False (default): every voxel is judged on its own.  A dict {"strength": s or {name: s}, "n_sweeps": 4,
            "tol": 0.0, "connectivity": 6} (TOML: a table [Fitting.solver.spatial_prior]; an unknown key, a negative strength or an
            unknown parameter name is a ValueError): a pairwise Gaussian neighbourhood (MRF) prior between adjacent voxels, by
            coloured mean-field sweeps (pnx_curvefit_grid_posterior_mrf_f64).  The precision of parameter k is
            strength_k / (range of its grid values over the admitted atoms)^2, 0 for a one-value axis and for a projected S0;
            strength 0 is the plain posterior.  `fit` then needs `neighbours` (n_pixels, n_nb) and `colours` (n_pixels,) --
            HipPixelWiseFitter passes api.grid_neighbours(mask, connectivity) (4 / 8: in-plane, 6: 3-D) --, sorts the voxels stably
            by colour, runs the sweeps and returns the results in the caller's order.  Worth it at low SNR: on a two-region
            phantom at 5 % noise strength 64 cuts the median errors by a quarter to a third; at 2 % noise strength 4 gains a few
            per cent and strength 64 over-smooths and LOSES up to 18 % (README).  With empirical_prior (single table) the table is
            learned first, without the spatial term.  Refused by name: together with a per-label or 2-D prior, or with marginals.
            This solver's own keys "potential" and "dof" (TOML: potential = "student_t", dof = 4.0 in the same table): "gaussian"
            (default: the path above, byte for byte) or "student_t", an edge-preserving pair potential with `dof` > 0 degrees of
            freedom (pnx_curvefit_grid_posterior_tmrf_f64): every neighbour enters with the weight
            (dof + K) / (dof + s), s the expected squared difference of the two voxels in units of the precisions, K the parameters
            that carry one -- near (dof + K) / dof inside a tissue, small across a boundary; dof -> infinity is the Gaussian.  At 5 %
            noise, dof 4 roughly halves the error of D1 and D2 at the region's edge against the Gaussian prior and costs some f1
            there; a small dof (1 and below) is unstable inside a region; at 2 % noise it helps as little as the Gaussian (README).
            dof with "gaussian", a "student_t" without a finite dof > 0, or another potential is a ValueError.  diagnostics_ gains
            "spatial_potential", "spatial_dof" and, under "student_t", "spatial_edge_weight" (n_pixels,): the mean over a voxel's
            present neighbours of dof / (dof + s) at its last update -- W_v / n_v scaled by dof / (dof + K) --, near 1 where the
            prior smooths as the Gaussian would, near 0 at an edge, NaN for a voxel without a present neighbour.
        marginals: None / False (default): nothing more.  True, or a dict {"quantiles": [0.025, 0.5, 0.975]} (TOML: a table
            [Fitting.solver.marginals]; an unknown key is a ValueError; up to 8 levels inside (0, 1)): `fit` also reports the
            marginal posterior of every gridded parameter over its grid values and these quantiles of it
            (pnx_curvefit_grid_marginals_f64; the grid value of the first bin whose cumulative mass reaches the level, not
            interpolated) -- under the learned table with `empirical_prior`.  A marginal with all its mass on one grid value says
            that parameter's grid is too coarse; one with two humps says the mean estimates nothing.  At most 128 grid values in
            all; a projected S0 has none (its value is fitted, not gridded).
        noise_model: "gaussian" (default: everything above, byte for byte) or "rician" (TOML: noise_model = "rician" under
            [Fitting.solver]): the likelihood of magnitude data, y_i ~ Rice(model_i, noise_sd), whose mean sits above the model by
            about noise_sd^2 / (2 model) once the model falls to a few noise_sd -- the high b-values, which carry the slow rate and
            the small fractions (pnx_curvefit_grid_posterior_rician_f64).  `fit` then calls that entry and
            diagnostics_ gains "noise_model".  It needs the known `noise_sd` of the real and imaginary channels and a free S0 on
            the grid (`project` defaults to False here).  A ValueError "noise_model 'rician' is not built with ...": noise_sd None /
            0, project=True, sigma, empirical_prior, spatial_prior, marginals, a 2-D log_prior.  Any other value is a ValueError.
            A voxel with a negative signal entry is reported as one with a non-finite signal.  About 27 times the cost of the
            Gaussian call at 32 b-values (README).
        refine: None / False (default: everything above, byte for byte).  True, or a dict with any of {"points": 5, "levels": 1,
            "span": 1.0, "n_sd": 2.0} (TOML: a table [Fitting.solver.refine]; an unknown key is a ValueError): after the coarse
            posterior (level 0, unchanged) every voxel gets `levels` (1..3) fine grids of its own, each a box around the previous
            level's mean with `points` (1..9; a number, or {name: int}) values per gridded axis, a uniform prior and the direct cost
            (pnx_curvefit_grid_refine_f64): resolution where the voxel's posterior sits, which a 4-value axis
            cannot give.  half_width_k = max(span * cell_k, n_sd * sd_k): cell_k is, at level 1, the width of the coarse grid cell
            that holds the mean (the gap between the two neighbouring grid values, the end gap at the ends), afterwards the previous
            level's point spacing; sd_k the previous level's posterior sd.  The box is cut at `bounds`; an axis with one coarse value
            (and a projected S0) keeps one value; at most 4096 atoms per voxel.  Atoms of a reduced layout with f1 + f2 > 1 are
            dropped.  params_, posterior_sd and map then are the LAST level's; diagnostics_ gains "refine_levels",
            "refine_edge_mass" {name: (n_pixels,)} (the posterior share on the two ends of the last box: large values say the box
            truncates the posterior) and "refine_ess", and keeps the coarse "ess", "map_atom" and "log_evidence" (still the model
            evidence; a fine grid has none).  A voxel whose fine box holds no admitted atom (a coarse mean beyond f1 + f2 = 1) gets
            NaN parameters and success False.  Every level is one host call: the signal is uploaded and the level's results come
            back per level.  Helps at 1 % noise, where the coarse grid is the limit, and does little at 5 %
            (README).  A ValueError "refine is not built with ...": noise_model="rician", spatial_prior, empirical_prior, marginals,
            per-label priors, a non-uniform log_prior, sigma, the T1 / STEAM factor.
    Not built, hence a ValueError: per-pixel fixed parameters (the dictionary would differ from voxel to voxel), io_dtype or
    precision "float32" (the posterior reads and writes float64 arrays and exponentiates in fp64).
    Any other keyword (the reference's solver arguments: method, multi_threading, ...) is accepted and ignored.
    After fit: params_ = the posterior mean keyed by the model's names; diagnostics_ {"posterior_sd", "map" (dicts name ->
    (n_pixels,)), "map_atom", "log_evidence", "ess", "n_pixels"} (no "pcov": the sd is the uncertainty; ess near 1 says the grid
    is too coarse for it), with empirical_prior also {"log_prior" (n_atoms,) the learned table, "prior_loglik" the EM's
    log-likelihood trace, "prior_n_iter" the updates it ran, "prior_n_voxels" the voxels it learned from} -- with per_label
    "log_prior" is (C, n_atoms), "prior_loglik" (n_iter + 1, C) with its sum over the labels in "prior_loglik_total", and
    {"prior_n_eff" (C,), "prior_labels" the label value of every row} come with them --, with marginals also
    {"marginal" {name: (n_bins, n_pixels)}, "marginal_values" {name: (n_bins,)}, "quantiles" {name: (n_q, n_pixels)},
    "quantile_probs"} (a projected S0 is absent from the three dicts), with spatial_prior also {"spatial_sweeps" the sweeps run,
    "spatial_delta" (n_sweeps,) the largest move of a mean per sweep in units of its grid range, "spatial_precision" {name: lambda}}
    and "log_evidence" is then the local normaliser of the last update, not a model evidence; pixel_results_ with success = the
    voxel's signal was finite."""

    _MARGINALS_DEFAULTS = {"quantiles": (0.025, 0.5, 0.975)}
    _EMPIRICAL_PRIOR_DEFAULTS = {"n_iter": 20, "pseudo_count": 0.0, "rel_tol": 1e-6, "max_voxels": None}
    _EMPIRICAL_PRIOR_PER_LABEL = {"per_label": False}  # reported among the options only when it is on
    _SPATIAL_PRIOR_DEFAULTS = {"strength": None, "n_sweeps": 4, "tol": 0.0, "connectivity": 6}
    _REFINE_DEFAULTS = {"points": 5, "levels": 1, "span": 1.0, "n_sd": 2.0}

    def __init__(self, model: Any, grid=None, max_iter: int = 250, tol: float = 1e-8, p0: dict[str, float] | None = None,
                 bounds: dict[str, tuple[float, float]] | None = None, noise_sd: float | None = None, log_prior=None, project=None,
                 sigma=None, device: int = 0, io_dtype: str = "float64", precision: str = "float64", empirical_prior=None,
                 marginals=None, spatial_prior=None, noise_model: str = "gaussian", refine=None, **ignored_reference_kwargs):
        RefBaseSolver.__init__(self, model=model, max_iter=max_iter, tol=tol, verbose=bool(ignored_reference_kwargs.pop("verbose", False)))
        self._kernel_model = kernel_model_key(model)
        self._kernel_t1 = kernel_t1(model)
        self.refine = self._refine_options(refine, list(model.param_names))
        if noise_model not in ("gaussian", "rician"):
            raise ValueError(f"noise_model must be 'gaussian' or 'rician', got {noise_model!r}")
        self.noise_model = noise_model
        if noise_model == "rician" and project is None:
            project = False  # the amplitude cannot be projected under this likelihood: a free S0 sits on the grid
        spatial_prior, self.spatial_potential, self.spatial_dof = self._potential_option(spatial_prior)
        self.spatial_prior = self._spatial_prior_options(spatial_prior, list(model.param_names))
        self.empirical_prior = self._empirical_prior_options(empirical_prior)
        self.marginals = self._marginals_options(marginals)
        if _io_dtype(io_dtype) is not np.float64 or precision != "float64":
            raise ValueError("HipBayesGridSolver is built for precision='float64' and io_dtype='float64': the posterior reads and writes "
                             "float64 arrays and exponentiates in fp64")
        if grid is None:
            raise ValueError("grid is required: a dict from parameter name to a sequence of values")
        names = list(model.param_names)
        if bounds is None:
            raise ValueError(f"bounds is required: {{name: (lo, hi)}} for every parameter of {names}")
        _validate_parameter_names(bounds, names)
        if isinstance(grid, dict):
            missing = [n for n in names if n not in grid and n not in (p0 or {})]
            if missing:
                raise ValueError(f"neither grid nor p0 holds a value for {missing}")
        self.grid, self.project, self._atoms = _grid_atoms("grid", model, self._kernel_model, p0 or {}, bounds, grid, project, "project")
        self.noise_sd = 0.0 if noise_sd is None else float(noise_sd)
        if not (np.isfinite(self.noise_sd) and self.noise_sd >= 0.0):
            raise ValueError(f"noise_sd must be None / 0 (marginalised) or a finite positive standard deviation, got {noise_sd!r}")
        self.log_prior = None
        if log_prior is not None:
            lp = np.ascontiguousarray(log_prior, np.float64)
            if lp.ndim == 2 and lp.shape[1] == self._atoms.shape[1] and lp.shape[0] > api.GRID_MAX_CLASSES:
                raise ValueError(f"log_prior has {lp.shape[0]} rows: at most {api.GRID_MAX_CLASSES} classes (labels) are built")
            if not (lp.ndim == 2 and lp.shape[0] >= 2 and lp.shape[1] == self._atoms.shape[1]):  # (1, n_atoms) is the one table, as before
                lp = lp.reshape(-1)
            if lp.ndim == 1 and lp.shape != (self._atoms.shape[1],):
                raise ValueError(f"log_prior has {lp.size} entries for {self._atoms.shape[1]} atoms (one per atom, in the order of "
                                 "itertools.product over model.param_names)")
            if np.isnan(lp).any() or (lp == np.inf).any() or not np.isfinite(lp).any(axis=-1).all():
                raise ValueError("log_prior entries must be finite or -inf, at least one of them finite" + (" in every row" if lp.ndim == 2 else ""))
            self.log_prior = lp
        self.sigma = None
        if sigma is not None:
            self.sigma = np.asarray(sigma, float)
            if self.sigma.ndim > 1 and self.sigma.size != 1:
                raise ValueError("HipBayesGridSolver implements a scalar or 1-D sigma (one standard deviation per b-value)")
            self.sigma = self.sigma.reshape(-1)
        self.p0 = p0
        self.bounds = bounds
        self.device = int(device)
        self.io_dtype = np.float64
        self.solver_kwargs = ignored_reference_kwargs
        per_label = bool(self.empirical_prior and self.empirical_prior.get("per_label"))
        if self.needs_labels and self.marginals:
            raise ValueError("HipBayesGridSolver: marginals are not built with per-label priors (a 2-D log_prior or empirical_prior "
                             "per_label): pnx_curvefit_grid_marginals_f64 takes one prior table")
        if per_label and self.empirical_prior["max_voxels"]:
            raise ValueError("empirical_prior max_voxels is not built with per_label: every label learns from all of its voxels")
        if self.empirical_prior and not per_label and self.log_prior is not None and self.log_prior.ndim == 2:
            raise ValueError("empirical_prior with a 2-D log_prior needs per_label: a single learned table has no single row to start from")
        if self.spatial_prior and self.needs_labels:
            raise ValueError("HipBayesGridSolver: spatial_prior is not built with per-label priors (a 2-D log_prior or empirical_prior "
                             "per_label): pnx_curvefit_grid_posterior_mrf_f64 takes one prior table")
        if self.spatial_prior and self.marginals:
            raise ValueError("HipBayesGridSolver: spatial_prior is not built with marginals: pnx_curvefit_grid_marginals_f64 knows no field")
        if self.noise_model == "rician":
            refused = [("a marginalised noise scale (noise_sd None / 0): pass the known noise sd of the magnitude data", not self.noise_sd > 0.0),
                       ("a projected S0 (project=True): put S0 on the grid", self.project),
                       ("sigma (per-b-value weights): the Rice density has one noise sd", self.sigma is not None),
                       ("empirical_prior: pnx_curvefit_grid_prior_em_f64 has the Gaussian likelihood", bool(self.empirical_prior)),
                       ("spatial_prior: the MRF calls have the Gaussian likelihood", bool(self.spatial_prior)),
                       ("marginals: pnx_curvefit_grid_marginals_f64 has the Gaussian likelihood", bool(self.marginals)),
                       ("per-label priors (a 2-D log_prior): pnx_curvefit_grid_posterior_classes_f64 has the Gaussian likelihood",
                        self.needs_labels)]
            for what, hit in refused:
                if hit:
                    raise ValueError(f"HipBayesGridSolver: noise_model 'rician' is not built with {what}")
        if self.refine:
            refused = [("noise_model='rician': the fine grid has the Gaussian likelihood", self.noise_model == "rician"),
                       ("spatial_prior: the fine grid knows no field", bool(self.spatial_prior)),
                       ("empirical_prior: a learned table has no values between the coarse atoms", bool(self.empirical_prior)),
                       ("marginals: pnx_curvefit_grid_marginals_f64 reports the coarse grid's", bool(self.marginals)),
                       ("per-label priors (a 2-D log_prior): the fine grid's prior is uniform", self.needs_labels),
                       ("a non-uniform log_prior: the fine grid's prior is uniform",
                        self.log_prior is not None and bool(np.ptp(self.log_prior) > 0.0)),
                       ("sigma (per-b-value weights)", self.sigma is not None),
                       ("the T1 / STEAM factor (fit_t1): T1 would need a table of its own per voxel", bool(self._kernel_t1.get("t1_mode")))]
            for what, hit in refused:
                if hit:
                    raise ValueError(f"HipBayesGridSolver: refine is not built with {what}")
            self._refine_points = self.refine_points()

    @classmethod
    def _refine_options(cls, value, names):
        """None when off, else {"points": {name: int} for every parameter, "levels", "span", "n_sd"}, checked."""
        if value is None or value is False:
            return None
        if value is True:
            value = {}
        if not isinstance(value, dict):
            raise ValueError(f"refine must be None, a bool or a dict of {sorted(cls._REFINE_DEFAULTS)}, got {value!r}")
        unknown = sorted(set(value) - set(cls._REFINE_DEFAULTS))
        if unknown:
            raise ValueError(f"refine has unknown keys {unknown}; it takes {sorted(cls._REFINE_DEFAULTS)}")
        opt = {**cls._REFINE_DEFAULTS, **value}
        pts = opt["points"]
        if isinstance(pts, dict):
            bad = sorted(set(pts) - set(names))
            if bad:
                raise ValueError(f"refine points names unknown parameters {bad}; the model has {names}")
            pts = {n: pts.get(n, cls._REFINE_DEFAULTS["points"]) for n in names}
        else:
            pts = {n: pts for n in names}
        for n, v in pts.items():
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= api.GRID_REFINE_MAX_POINTS:
                raise ValueError(f"refine points of {n} must be an integer in [1, {api.GRID_REFINE_MAX_POINTS}], got {v!r}")
        lv = opt["levels"]
        if isinstance(lv, bool) or not isinstance(lv, (int, np.integer)) or not 1 <= lv <= 3:
            raise ValueError(f"refine levels must be an integer in [1, 3], got {lv!r}")
        for key in ("span", "n_sd"):
            v = opt[key]
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (np.isfinite(v) and v >= 0.0):
                raise ValueError(f"refine {key} must be finite and >= 0, got {v!r}")
        if not (opt["span"] > 0.0 or opt["n_sd"] > 0.0):
            raise ValueError("refine needs span > 0 or n_sd > 0: both 0 leave a box of one value")
        return {"points": {n: int(v) for n, v in pts.items()}, "levels": int(lv), "span": float(opt["span"]), "n_sd": float(opt["n_sd"])}

    def _coarse_axes(self):
        """Per free parameter the sorted distinct coarse grid values (one value for a parameter the grid does not name)."""
        return [np.unique(row) for row in self._atoms]

    def refine_points(self):
        """n_points (n_free,) int32 of the fine grid: refine["points"] on every axis with more than one coarse value, 1 on a one-value
        axis and on a projected S0; more than 4096 atoms per voxel is a ValueError."""
        names = list(self.model.param_names)
        npts = np.array([self.refine["points"][n] if ax.size > 1 and not (self.project and n == "S0") else 1
                         for n, ax in zip(names, self._coarse_axes())], np.int32)
        total = int(np.prod(npts, dtype=np.int64))
        if total > api.GRID_MAX_ATOMS:
            raise ValueError(f"refine points span {total} atoms per voxel, more than the {api.GRID_MAX_ATOMS} a fine grid takes")
        return npts

    @staticmethod
    def coarse_cell(values, mean):
        """Width of the coarse grid cell that holds `mean` (n_pixels,): the gap between the two neighbouring grid values, the end gap
        at the ends and beyond, 0 for a one-value axis.  A NaN mean gives NaN."""
        mean = np.asarray(mean, float)
        if values.size < 2:
            return np.zeros_like(mean)
        gaps = np.diff(values)
        j = np.clip(np.searchsorted(values, np.nan_to_num(mean, nan=values[0]), side="right") - 1, 0, gaps.size - 1)
        return np.where(np.isnan(mean), np.nan, gaps[j])

    def _fit_refine(self, xdata, ydata, mean, sd, lo, hi, fixed_idx, fixed_vals):
        """The fine levels behind the coarse posterior (mean, sd (n_free, n_pixels)): the last level's result dict of api.grid_refine."""
        rf, npts = self.refine, self._refine_points
        many = npts[:, None] > 1
        cell = np.stack([self.coarse_cell(ax, mean[k]) for k, ax in enumerate(self._coarse_axes())])
        res = None
        for _ in range(rf["levels"]):
            half = np.where(many, np.maximum(rf["span"] * cell, rf["n_sd"] * sd), 0.0)
            if self.project:  # the projected S0 row is fitted per atom: its centre and half-width are not read
                half[list(self.model.param_names).index("S0")] = 0.0
            centre = np.ascontiguousarray(mean)
            res = api.grid_refine(self._kernel_model, xdata, ydata, lo, hi, npts, centre, np.ascontiguousarray(half), noise_sd=self.noise_sd,
                                  fixed_idx=fixed_idx, fixed_vals=fixed_vals, project_amplitude=self.project, device=self.device)
            a, b = np.maximum(lo[:, None], centre - half), np.minimum(hi[:, None], centre + half)
            cell = np.where(many, np.maximum(b - a, 0.0) / np.maximum(npts[:, None] - 1, 1), 0.0)
            mean, sd = res["mean"], res["sd"]
        return res

    @property
    def needs_labels(self) -> bool:
        """True when `fit` needs `labels`: a 2-D log_prior, or empirical_prior with per_label."""
        return bool((self.log_prior is not None and self.log_prior.ndim == 2) or (self.empirical_prior and self.empirical_prior.get("per_label")))

    @property
    def needs_neighbours(self) -> bool:
        """True when `fit` needs `neighbours` and `colours`: spatial_prior is on."""
        return bool(self.spatial_prior)

    @staticmethod
    def _potential_option(value):
        """(spatial_prior without its "potential" and "dof" keys -- this solver's only; the shared parser knows the four others --,
        the potential "gaussian" | "student_t", dof or None)."""
        if not isinstance(value, dict) or not ({"potential", "dof"} & set(value)):
            return value, "gaussian", None
        value = dict(value)
        potential, dof = value.pop("potential", "gaussian"), value.pop("dof", None)
        if potential not in ("gaussian", "student_t"):
            raise ValueError(f"spatial_prior potential must be 'gaussian' or 'student_t', got {potential!r}")
        if potential == "gaussian":
            if dof is not None:
                raise ValueError(f"spatial_prior dof={dof!r} is given with potential 'gaussian', which has none: it belongs to 'student_t'")
            return value, potential, None
        if isinstance(dof, bool) or not isinstance(dof, (int, float, np.integer, np.floating)) or not (np.isfinite(dof) and dof > 0.0):
            raise ValueError(f"spatial_prior potential 'student_t' needs a finite dof > 0, got {dof!r}")
        return value, potential, float(dof)

    @classmethod
    def _spatial_prior_options(cls, value, names):
        """None when off, else {"strength": {name: s} for every parameter, "n_sweeps", "tol", "connectivity"}, checked."""
        if value is None or value is False:
            return None
        if not isinstance(value, dict):
            raise ValueError(f"spatial_prior must be None or a dict of {sorted(cls._SPATIAL_PRIOR_DEFAULTS)}, got {value!r}")
        unknown = sorted(set(value) - set(cls._SPATIAL_PRIOR_DEFAULTS))
        if unknown:
            raise ValueError(f"spatial_prior has unknown keys {unknown}; it takes {sorted(cls._SPATIAL_PRIOR_DEFAULTS)}")
        opt = {**cls._SPATIAL_PRIOR_DEFAULTS, **value}
        st = opt["strength"]
        if st is None:
            raise ValueError("spatial_prior needs a strength: a number, or {parameter name: number}")
        if isinstance(st, dict):
            bad = sorted(set(st) - set(names))
            if bad:
                raise ValueError(f"spatial_prior strength names unknown parameters {bad}; the model has {names}")
            st = {n: st.get(n, 0.0) for n in names}
        else:
            st = {n: st for n in names}
        for n, v in st.items():
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (np.isfinite(v) and v >= 0.0):
                raise ValueError(f"spatial_prior strength of {n} must be finite and >= 0, got {v!r}")
        ns, tol, conn = opt["n_sweeps"], opt["tol"], opt["connectivity"]
        if isinstance(ns, bool) or int(ns) != ns or not 0 <= ns <= api.GRID_MRF_MAX_SWEEPS:
            raise ValueError(f"spatial_prior n_sweeps must be an integer in [0, {api.GRID_MRF_MAX_SWEEPS}], got {ns!r}")
        if not (np.isfinite(float(tol)) and float(tol) >= 0.0):
            raise ValueError(f"spatial_prior tol must be finite and >= 0, got {tol!r}")
        if isinstance(conn, bool) or conn not in (4, 6, 8):
            raise ValueError(f"spatial_prior connectivity must be 4, 8 (in-plane) or 6 (3-D), got {conn!r}")
        return {"strength": {n: float(v) for n, v in st.items()}, "n_sweeps": int(ns), "tol": float(tol), "connectivity": int(conn)}

    def spatial_precision(self, log_prior=None):
        """precision (n_free,) of the spatial prior under `log_prior` (None: uniform): strength / range^2 over the admitted atoms, 0
        for a one-value axis and for a projected S0."""
        names = list(self.model.param_names)
        adm = np.ones(self._atoms.shape[1], bool) if log_prior is None else np.asarray(log_prior, float) > -np.inf
        rng = self._atoms[:, adm].max(axis=1) - self._atoms[:, adm].min(axis=1)
        pr = np.zeros(len(names))
        for k, n in enumerate(names):
            if rng[k] > 0.0 and not (self.project and n == "S0"):
                pr[k] = self.spatial_prior["strength"][n] / rng[k] ** 2
        return pr

    @staticmethod
    def colour_sort(neighbours, colours, n_pixels):
        """(order, neighbours of the sorted voxels, colour_start): the voxels sorted stably by colour -- voxel order[i] of the caller
        is voxel i of the call --, the table's rows permuted and its indices remapped, and the offsets of the colour ranges."""
        nb, col = np.asarray(neighbours), np.asarray(colours)
        if nb.ndim != 2 or nb.shape[0] != n_pixels or nb.dtype.kind not in "iu" or not 1 <= nb.shape[1] <= api.GRID_MRF_MAX_NEIGHBOURS:
            raise ValueError(f"neighbours must be ({n_pixels}, 1..{api.GRID_MRF_MAX_NEIGHBOURS}) integers, got shape {nb.shape} and dtype {nb.dtype}")
        if col.shape != (n_pixels,) or col.dtype.kind not in "iu" or (col.size and (col.min() < 0 or col.max() >= api.GRID_MRF_MAX_COLOURS)):
            raise ValueError(f"colours must be {n_pixels} integers in [0, {api.GRID_MRF_MAX_COLOURS}), got shape {col.shape} and dtype {col.dtype}")
        if nb.size and (nb.min() < -1 or nb.max() >= n_pixels):
            raise ValueError(f"neighbours must hold voxel indices in [-1, {n_pixels})")
        order = np.argsort(col, kind="stable")
        place = np.empty(n_pixels, np.int64)
        place[order] = np.arange(n_pixels)
        rows = nb[order]
        sorted_nb = np.where(rows >= 0, place[np.maximum(rows, 0)], -1).astype(np.int32)
        n_colours = int(col.max()) + 1 if col.size else 1
        start = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n_colours))]).astype(np.int64)
        return order, np.ascontiguousarray(sorted_nb), start

    def _fit_spatial(self, xdata, ydata, neighbours, colours, lo, hi, log_prior, common):
        """The posterior under the neighbourhood prior, in the caller's voxel order."""
        n_pixels = ydata.shape[0]
        if neighbours is None or colours is None:
            raise ValueError("HipBayesGridSolver: neighbours (n_pixels, n_nb) and colours (n_pixels,) are required with spatial_prior "
                             "(api.grid_neighbours(mask, connectivity); HipPixelWiseFitter passes them)")
        precision = self.spatial_precision(log_prior)
        sp = self.spatial_prior
        if self.spatial_potential == "student_t":
            return self.in_colour_order(
                ydata, neighbours, colours, precision, ("mean", "sd", "map_p", "map_atom", "log_evidence", "ess", "field_w", "field_n"),
                lambda y, nb, start: api.grid_posterior_tmrf(self._kernel_model, xdata, y, self._atoms, lo, hi, nb, start, precision,
                                                             self.spatial_dof, n_sweeps=sp["n_sweeps"], tol=sp["tol"], log_prior=log_prior,
                                                             **common))
        return self.in_colour_order(
            ydata, neighbours, colours, precision, ("mean", "sd", "map_p", "map_atom", "log_evidence", "ess"),
            lambda y, nb, start: api.grid_posterior_mrf(self._kernel_model, xdata, y, self._atoms, lo, hi, nb, start, precision,
                                                        n_sweeps=sp["n_sweeps"], tol=sp["tol"], log_prior=log_prior, **common))

    @classmethod
    def in_colour_order(cls, ydata, neighbours, colours, precision, keys, run):
        """`run(y, neighbours, colour_start)` on the voxels sorted by colour (colour_sort), its per-voxel results `keys` put back
        into the caller's order, with "delta", "n_sweeps" and `precision` beside them: the sort and un-sort both Bayes solvers use."""
        n_pixels = ydata.shape[0]
        order, nb, start = cls.colour_sort(neighbours, colours, n_pixels)
        res = run(np.ascontiguousarray(ydata[order]), nb, start)
        back = np.empty(n_pixels, np.int64)
        back[order] = np.arange(n_pixels)
        out = {k: np.ascontiguousarray(v[..., back]) for k, v in res.items() if k in keys}
        out.update(delta=res["delta"], n_sweeps=res["n_sweeps"], precision=precision)
        return out

    @classmethod
    def _empirical_prior_options(cls, value):
        """None when off, else the four options with their defaults filled in and their values checked."""
        if value is None or value is False:
            return None
        if value is True:
            value = {}
        if not isinstance(value, dict):
            raise ValueError(f"empirical_prior must be None, a bool or a dict of {sorted(cls._EMPIRICAL_PRIOR_DEFAULTS)}, got {value!r}")
        known = {**cls._EMPIRICAL_PRIOR_DEFAULTS, **getattr(cls, "_EMPIRICAL_PRIOR_PER_LABEL", {})}  # the grid solver's own option
        unknown = sorted(set(value) - set(known))
        if unknown:
            raise ValueError(f"empirical_prior has unknown keys {unknown}; it takes {sorted(cls._EMPIRICAL_PRIOR_DEFAULTS)}")
        opt = {"per_label": False, **known, **value}
        if not isinstance(opt["per_label"], (bool, np.bool_)):
            raise ValueError(f"empirical_prior per_label must be a bool, got {opt['per_label']!r}")
        n_iter, mv = opt["n_iter"], opt["max_voxels"]
        if isinstance(n_iter, bool) or int(n_iter) != n_iter or not 1 <= n_iter <= 1000:
            raise ValueError(f"empirical_prior n_iter must be an integer in [1, 1000], got {n_iter!r}")
        for key in ("pseudo_count", "rel_tol"):
            if not (np.isfinite(float(opt[key])) and float(opt[key]) >= 0.0):
                raise ValueError(f"empirical_prior {key} must be finite and >= 0, got {opt[key]!r}")
        if mv is not None and (isinstance(mv, bool) or int(mv) != mv or mv < 1):
            raise ValueError(f"empirical_prior max_voxels must be None or a positive integer, got {mv!r}")
        res = {"n_iter": int(n_iter), "pseudo_count": float(opt["pseudo_count"]), "rel_tol": float(opt["rel_tol"]),
               "max_voxels": None if mv is None else int(mv)}
        if opt["per_label"]:
            res["per_label"] = True
        return res

    @classmethod
    def _marginals_options(cls, value):
        """None when off, else {"quantiles": tuple of levels}, checked."""
        if value is None or value is False:
            return None
        if value is True:
            value = {}
        if not isinstance(value, dict):
            raise ValueError(f"marginals must be None, a bool or a dict of {sorted(cls._MARGINALS_DEFAULTS)}, got {value!r}")
        unknown = sorted(set(value) - set(cls._MARGINALS_DEFAULTS))
        if unknown:
            raise ValueError(f"marginals has unknown keys {unknown}; it takes {sorted(cls._MARGINALS_DEFAULTS)}")
        try:
            q = tuple(float(p) for p in np.asarray({**cls._MARGINALS_DEFAULTS, **value}["quantiles"], float).reshape(-1))
        except (TypeError, ValueError):
            raise ValueError(f"marginals quantiles must be a sequence of numbers, got {value['quantiles']!r}") from None
        if len(q) > api.GRID_MARGINAL_MAX_PROBS or not all(0.0 < p < 1.0 for p in q):
            raise ValueError(f"marginals quantiles must be at most {api.GRID_MARGINAL_MAX_PROBS} levels inside the open interval (0, 1), got {list(q)}")
        return {"quantiles": q}

    @staticmethod
    def label_rows(labels, n_pixels):
        """(distinct non-negative label values ascending, row of every voxel as int32 with -1 for a negative label)."""
        lab = np.asarray(labels)
        if lab.dtype.kind == "f" and lab.size and np.isfinite(lab).all() and (lab == np.round(lab)).all():
            lab = lab.astype(np.int64)  # a segmentation read from an image file is often stored as floats
        if lab.shape != (n_pixels,) or lab.dtype.kind not in "iu":
            raise ValueError(f"labels must be {n_pixels} integers (one per pixel), got shape {lab.shape} and dtype {lab.dtype}")
        values = np.unique(lab[lab >= 0])
        if values.size > api.GRID_MAX_CLASSES:
            raise ValueError(f"labels hold {values.size} distinct non-negative values: more than {api.GRID_MAX_CLASSES} classes are "
                             "not built (merge labels, or fit the tissues in separate calls)")
        rows = np.where(lab >= 0, np.searchsorted(values, np.maximum(lab, 0)), -1).astype(np.int32)
        return values, rows

    def _fit_labelled(self, xdata, ydata, labels, lo, hi, common):
        """(posterior result, learned or None) under one prior row per label."""
        n_pixels = ydata.shape[0]
        if labels is None:
            raise ValueError("HipBayesGridSolver: labels (n_pixels,) is required with a 2-D log_prior or empirical_prior per_label")
        per_label = bool(self.empirical_prior and self.empirical_prior.get("per_label"))
        table = self.log_prior
        if per_label:
            values, rows = self.label_rows(labels, n_pixels)
            n_classes = max(int(values.size), 1)
            if table is not None and table.ndim == 2 and table.shape[0] != n_classes:
                raise ValueError(f"log_prior has {table.shape[0]} rows for the {n_classes} distinct labels of this call")
            if table is not None and table.ndim == 1:
                table = np.ascontiguousarray(np.broadcast_to(table, (n_classes, table.size)))
        else:  # the caller's table: label c is row c, anything else is background
            n_classes = table.shape[0]
            lab = np.asarray(labels)
            if lab.shape != (n_pixels,) or lab.dtype.kind not in "iuf":
                raise ValueError(f"labels must be {n_pixels} integers (one per pixel), got shape {lab.shape} and dtype {lab.dtype}")
            rows = np.where((lab >= 0) & (lab < n_classes) & (lab == np.floor(lab)), lab, -1).astype(np.int32)
        learned = None
        if per_label:
            ep = self.empirical_prior
            learned = api.grid_prior_em_classes(self._kernel_model, xdata, ydata, self._atoms, lo, hi, rows, n_classes, log_prior=table,
                                                n_iter=ep["n_iter"], pseudo_count=ep["pseudo_count"], rel_tol=ep["rel_tol"], **common)
            learned["n_voxels"] = n_pixels
            learned["labels"] = values
            table = learned["log_prior"]
        res = api.grid_posterior_classes(self._kernel_model, xdata, ydata, self._atoms, lo, hi, rows, n_classes, log_prior=table, **common)
        return res, learned

    def fit(self, xdata: np.ndarray, ydata: np.ndarray, pixel_fixed_params=None, labels=None, neighbours=None, colours=None,
            **fit_kwargs) -> "HipBayesGridSolver":
        if pixel_fixed_params:
            raise ValueError("HipBayesGridSolver is not built with per-pixel fixed parameters (pixel_fixed_params): the dictionary "
                             "would differ from voxel to voxel")
        self._reset_state()
        xdata = np.asarray(xdata)
        ydata = np.asarray(ydata)
        _validate_data_shapes(xdata, ydata)
        if ydata.ndim == 1:
            ydata = ydata[np.newaxis, :]
        if ydata.ndim > 2:
            raise ValueError(f"ydata must be 1D or 2D array, but got shape {ydata.shape}.")
        n_pixels = ydata.shape[0]
        names = list(self.model.param_names)
        all_names = list(self.model._all_param_names)
        fixed = getattr(self.model, "fixed_params", None) or {}
        fixed_idx = [i for i, n in enumerate(all_names) if n in fixed]
        fixed_vals = np.array([float(fixed[all_names[i]]) for i in fixed_idx]) if fixed_idx else None
        lo = np.array([self.bounds[n][0] for n in names], float)
        hi = np.array([self.bounds[n][1] for n in names], float)
        common = dict(noise_sd=self.noise_sd, fixed_idx=fixed_idx, fixed_vals=fixed_vals, sigma=self.sigma, project_amplitude=self.project,
                      device=self.device, **self._kernel_t1)
        log_prior, learned = self.log_prior, None
        if self.needs_labels:
            res, learned = self._fit_labelled(xdata, ydata, labels, lo, hi, common)
        elif self.empirical_prior:
            ep = self.empirical_prior
            step = 1 if ep["max_voxels"] is None else -(-n_pixels // ep["max_voxels"])
            sample = ydata[::step]
            learned = api.grid_prior_em(self._kernel_model, xdata, sample, self._atoms, lo, hi, log_prior=self.log_prior, n_iter=ep["n_iter"],
                                        pseudo_count=ep["pseudo_count"], rel_tol=ep["rel_tol"], **common)
            learned["n_voxels"] = sample.shape[0]
            log_prior = learned["log_prior"]
        if self.spatial_prior:
            res = self._fit_spatial(xdata, ydata, neighbours, colours, lo, hi, log_prior, common)
        elif self.noise_model == "rician":
            res = api.grid_posterior_rician(self._kernel_model, xdata, ydata, self._atoms, lo, hi, noise_sd=self.noise_sd, log_prior=log_prior,
                                            fixed_idx=fixed_idx, fixed_vals=fixed_vals, device=self.device, **self._kernel_t1)
        elif not self.needs_labels:
            res = api.grid_posterior(self._kernel_model, xdata, ydata, self._atoms, lo, hi, log_prior=log_prior, **common)
        mean, atom = res["mean"], res["map_atom"]
        fine = None
        if self.refine:
            fine = self._fit_refine(xdata, np.ascontiguousarray(ydata, np.float64), mean, res["sd"], lo, hi, fixed_idx, fixed_vals)
            mean = fine["mean"]
            res = {**res, "sd": fine["sd"], "map_p": fine["map_p"]}
        # with refine a voxel can also lose every fine atom to the fraction-sum rule (a coarse mean beyond the face f1 + f2 = 1)
        good = atom >= 0 if fine is None else (atom >= 0) & np.isfinite(mean).all(axis=0)
        self.pixel_results_ = PixelResultsView(mean.T, None, good,
                                               lambda i, a=atom, g=good: None if g[i] else _BAYES_MESSAGES[-2 if a[i] < 0 else -4])
        self.params_ = {name: [float(mean[i, 0])] if n_pixels == 1 else mean[i] for i, name in enumerate(names)}
        self.diagnostics_ = {"posterior_sd": {n: res["sd"][i] for i, n in enumerate(names)},
                             "map": {n: res["map_p"][i] for i, n in enumerate(names)}, "map_atom": atom,
                             "log_evidence": res["log_evidence"], "ess": res["ess"], "n_pixels": n_pixels}
        if fine is not None:
            self.diagnostics_.update({"refine_levels": self.refine["levels"], "refine_ess": fine["ess"],
                                      "refine_edge_mass": {n: fine["edge_mass"][i] for i, n in enumerate(names)}})
        if self.noise_model != "gaussian":
            self.diagnostics_["noise_model"] = self.noise_model
        if learned is not None:
            self.diagnostics_.update({"log_prior": learned["log_prior"], "prior_loglik": learned["loglik"], "prior_n_iter": learned["n_iter"],
                                      "prior_n_voxels": learned["n_voxels"]})
            if "labels" in learned:
                self.diagnostics_.update({"prior_loglik": learned["loglik_class"], "prior_loglik_total": learned["loglik"],
                                          "prior_n_eff": learned["n_eff"], "prior_labels": [int(v) for v in learned["labels"]]})
        if self.spatial_prior:
            self.diagnostics_.update({"spatial_sweeps": res["n_sweeps"], "spatial_delta": res["delta"],
                                      "spatial_precision": {n: float(res["precision"][i]) for i, n in enumerate(names)},
                                      "spatial_potential": self.spatial_potential, "spatial_dof": self.spatial_dof})
            if self.spatial_potential == "student_t":
                # the mean over a voxel's present neighbours of nu / (nu + s_uv): W_v / n_v scaled by nu / (nu + K), so that 1 is the
                # Gaussian prior's weight at a vanishing difference and 0 an edge
                k_rows = int((res["precision"] > 0).sum())
                with np.errstate(invalid="ignore", divide="ignore"):
                    ew = res["field_w"] / res["field_n"] * (self.spatial_dof / (self.spatial_dof + k_rows))
                self.diagnostics_["spatial_edge_weight"] = np.where(res["field_n"] > 0, ew, np.nan)
        if self.marginals:
            mg = api.grid_marginals(self._kernel_model, xdata, ydata, self._atoms, lo, hi, log_prior=log_prior,
                                    quantiles=self.marginals["quantiles"], **common)
            self.diagnostics_.update({"marginal": {names[k]: m for k, m in mg["marginal"].items()},
                                      "marginal_values": {names[k]: v for k, v in mg["values"].items()},
                                      "quantiles": {names[k]: q for k, q in mg["quantiles"].items()},
                                      "quantile_probs": mg["quantile_probs"]})
        return self


_VARPRO_MESSAGES = {-2: "array must not contain infs or NaNs"}


class HipVarProSolver(RefBaseSolver):
    """Variable-projection dictionary fit per voxel (VARPRO, separable least squares; pnx_curvefit_varpro_f64, include/pnx.h): only
    the rates (and a free T1) are on a grid, the fractions and S0 of every voxel and atom come in closed form and are clipped into
    `bounds`.  A coarse estimator over decades of rates without a per-voxel prior, and a start for the non-linear fit
    (HipCurveFitSolver's `p0_varpro`).  Registered as `hip_varpro`; no counterpart in the reference, whose solver contract it keeps.

    model: any of the seven layouts; shared fixed rates / T1 and the T1 / STEAM factor as the curve fit takes them; a fixed fraction
    or a fixed S0 is refused.  `max_iter`, `tol` are accepted because the TOML loader always passes them.  Arguments:
        rates: dict from the name of a non-linear parameter (D1, D2, D3, D, T1) to a sequence of values (TOML: arrays under
            [Fitting.solver.rates]).  The atoms are the Cartesian product in `model.param_names` order, the last one fastest; a
            non-linear parameter the dict does not name takes its scalar `p0`; every value inside `bounds`; at most 4096 atoms.
        ordered: True (default) keeps only the atoms with D1 > D2 > D3.
        bounds: {name: (lo, hi)} for every parameter, required: the box the amplitudes are clipped into; lo of S0 >= 0.
        p0: {name: value}: the non-linear parameters `rates` does not name, and the default `fallback`.
        fallback: {name: value} for every parameter, inside `bounds`: what a voxel with a non-finite signal reports.  Default: p0.
        sigma: None, a scalar or (n_b,), as HipCurveFitSolver's.  device: HIP device index.
    Not built, hence a ValueError: per-pixel fixed parameters, io_dtype or precision "float32".
    Any other keyword (the reference's solver arguments: method, multi_threading, ...) is accepted and ignored.
    After fit: params_ keyed by the model's names; diagnostics_ {"atom", "cost", "clipped", "n_pixels"}; pixel_results_ with
    success = the voxel's signal was finite."""

    def __init__(self, model: Any, rates=None, max_iter: int = 250, tol: float = 1e-8, p0: dict[str, float] | None = None,
                 bounds: dict[str, tuple[float, float]] | None = None, ordered: bool = True, fallback: dict[str, float] | None = None,
                 sigma=None, device: int = 0, io_dtype: str = "float64", precision: str = "float64", **ignored_reference_kwargs):
        RefBaseSolver.__init__(self, model=model, max_iter=max_iter, tol=tol, verbose=bool(ignored_reference_kwargs.pop("verbose", False)))
        self._kernel_model = kernel_model_key(model)
        self._kernel_t1 = kernel_t1(model)
        if _io_dtype(io_dtype) is not np.float64 or precision != "float64":
            raise ValueError("HipVarProSolver is built for precision='float64' and io_dtype='float64': the variable projection reads and "
                             "writes float64 arrays")
        if rates is None:
            raise ValueError("rates is required: a dict from the name of a non-linear parameter to a sequence of values")
        names = list(model.param_names)
        if bounds is None:
            raise ValueError(f"bounds is required: {{name: (lo, hi)}} for every parameter of {names}")
        _validate_parameter_names(bounds, names)
        self.ordered = bool(ordered)
        self.rates, self._nl_names, self._nl_atoms = _varpro_atoms("rates", model, self._kernel_model, p0, bounds, rates, self.ordered)
        fallback = fallback if fallback is not None else p0
        if fallback is None or [n for n in names if n not in fallback]:
            raise ValueError(f"fallback (default: p0) must hold a value for every parameter of {names}: it is what a voxel with a "
                             "non-finite signal reports")
        for n in names:
            if not bounds[n][0] <= float(fallback[n]) <= bounds[n][1]:
                raise ValueError(f"fallback[{n!r}] = {fallback[n]} lies outside the bounds {tuple(bounds[n])} of {n}")
        if "S0" in names and not bounds["S0"][0] >= 0:
            raise ValueError(f"the lower bound of S0 must be >= 0 (the fraction bounds scale with S0), got {bounds['S0'][0]}")
        self.sigma = None
        if sigma is not None:
            self.sigma = np.asarray(sigma, float)
            if self.sigma.ndim > 1 and self.sigma.size != 1:
                raise ValueError("HipVarProSolver implements a scalar or 1-D sigma (one standard deviation per b-value)")
            self.sigma = self.sigma.reshape(-1)
        self.p0 = p0
        self.fallback = {n: float(fallback[n]) for n in names}
        self.bounds = bounds
        self.device = int(device)
        self.io_dtype = np.float64
        self.solver_kwargs = ignored_reference_kwargs

    def fit(self, xdata: np.ndarray, ydata: np.ndarray, pixel_fixed_params=None, **fit_kwargs) -> "HipVarProSolver":
        if pixel_fixed_params:
            raise ValueError("HipVarProSolver is not built with per-pixel fixed parameters (pixel_fixed_params): the dictionary "
                             "would differ from voxel to voxel")
        self._reset_state()
        xdata = np.asarray(xdata)
        ydata = np.asarray(ydata)
        _validate_data_shapes(xdata, ydata)
        if ydata.ndim == 1:
            ydata = ydata[np.newaxis, :]
        if ydata.ndim > 2:
            raise ValueError(f"ydata must be 1D or 2D array, but got shape {ydata.shape}.")
        n_pixels = ydata.shape[0]
        names = list(self.model.param_names)
        all_names = list(self.model._all_param_names)
        fixed = getattr(self.model, "fixed_params", None) or {}
        fixed_idx = [i for i, n in enumerate(all_names) if n in fixed]
        fixed_vals = np.array([float(fixed[all_names[i]]) for i in fixed_idx]) if fixed_idx else None
        lo = np.array([self.bounds[n][0] for n in names], float)
        hi = np.array([self.bounds[n][1] for n in names], float)
        fb = np.array([self.fallback[n] for n in names], float)
        res = api.varpro(self._kernel_model, xdata, ydata, self._nl_atoms, lo, hi, fb, fixed_idx=fixed_idx, fixed_vals=fixed_vals,
                         sigma=self.sigma, device=self.device, **self._kernel_t1)
        params, atom = res["params"], res["atom"]
        self.pixel_results_ = PixelResultsView(params.T, None, atom >= 0,
                                               lambda i, a=atom: None if a[i] >= 0 else _VARPRO_MESSAGES[-2])
        self.params_ = {name: [float(params[i, 0])] if n_pixels == 1 else params[i] for i, name in enumerate(names)}
        self.diagnostics_ = {"atom": atom, "cost": res["cost"], "clipped": res["clipped"], "n_pixels": n_pixels}
        return self


class HipBayesVarProSolver(RefBaseSolver):
    """Bayesian fit per voxel over a variable-projection dictionary (pnx_curvefit_varpro_posterior_f64, include/pnx.h; Bretthorst's
    treatment of sums of exponentials): only the rates (and a free T1) are on a grid, the fractions and S0 of every voxel and atom
    are eliminated in closed form, and the posterior -- mean, standard deviation, evidence, effective sample size -- lives on the
    rate grid alone: about 19 values per axis where HipBayesGridSolver's full grid has 4, and no per-voxel prior on fractions
    and S0.  No iteration: the cost does not depend on the noise.  Registered as `hip_bayes_varpro`; no counterpart in the
    reference, whose solver contract it keeps.

    model: any of the seven layouts; shared fixed rates / T1 and the T1 / STEAM factor as the curve fit takes them; a fixed fraction
    or a fixed S0 is refused.  `max_iter`, `tol` are accepted because the TOML loader always passes them.  Arguments:
        rates, ordered, bounds, p0: as HipVarProSolver takes them (TOML: arrays under [Fitting.solver.rates]); at most 4096 atoms;
            bounds is the box the amplitudes are clipped into; lo of S0 >= 0.
        noise_sd: None / 0 (default) marginalises the noise scale under a Jeffreys prior; > 0 is a known Gaussian noise sd in the
            units of the (sigma-weighted) signal.
        log_prior: None (uniform) or (n_atoms,) log weights in the order of the atoms; -inf excludes an atom.  (C, n_atoms), 2 <= C
            <= 16: one row per label, label c judged under row c (pnx_curvefit_varpro_posterior_classes_f64); `fit` then needs
            labels, and any other label is background (NaN outputs).
        marginal_amplitudes: True (default) weighs an atom by the marginal over its amplitudes under a flat prior (the Occam term
            -0.5 log det N); False by the profile over them.
        sigma: None, a scalar or (n_b,), as HipCurveFitSolver's.  device: HIP device index.
    Two stated approximations: where a clip into `bounds` is active the marginal weight is a Laplace-style approximation at the
    clipped point (diagnostics_["clipped_mass"] says how much of the posterior rests on such atoms); and the sd of a fraction or of
    S0 is the between-atom spread only -- the conditional variance of the amplitudes given the rates is left out, a known
    understatement.
    Not built, hence a ValueError: per-pixel fixed parameters (the dictionary would differ from voxel to voxel), io_dtype or
    precision "float32".  Any other keyword (the reference's solver arguments: method, multi_threading, ...) is accepted and ignored.
        marginals: None / False (default): nothing more.  True, or a dict {"quantiles": [0.025, 0.5, 0.975]} (TOML: a table
            [Fitting.solver.marginals]; HipBayesGridSolver's option, the same rules and messages): `fit` also reports the marginal
            posterior of every free rate (and a free T1) over its grid values, these quantiles of it (the grid value of the first
            bin whose cumulative mass reaches the level, not interpolated) and the geometric posterior mean exp E[log D]
            (pnx_curvefit_varpro_marginals_f64) -- on a log-spaced rate axis the estimate the arithmetic mean drags upward.  At
            most 128 grid values in all; a fraction or S0 has none (its value is solved per voxel and atom, not gridded).
        empirical_prior: None / False (default): the posterior under `log_prior`, as before.  True, or a dict with any of
            {"n_iter": 20, "pseudo_count": 0.0, "rel_tol": 1e-6, "max_voxels": None} (TOML: a table [Fitting.solver.empirical_prior];
            HipBayesGridSolver's option, the same rules and messages): `fit` first learns the prior over the rate atoms from the
            volume by EM (pnx_curvefit_varpro_prior_em_f64; `log_prior` is its start, the Occam term of `marginal_amplitudes` stays
            in the likelihood) on ydata[::ceil(n / max_voxels)], then reports the posterior -- and the marginals -- under the
            learned table.  It needs many voxels: a few dozen over-fit.  With "per_label": True (HipBayesGridSolver's option, the
            same TOML table) `fit(..., labels=...)` learns one table per distinct non-negative label, rows in ascending label order
            (pnx_curvefit_varpro_prior_em_classes_f64; at most 16 labels, a negative label is background), and reports the
            posterior of every voxel under its label's table; the diagnostics are then the grid solver's per-label set:
            "log_prior" (C, n_atoms), "prior_loglik" (n_iter + 1, C), "prior_loglik_total", "prior_n_eff" (C,), "prior_labels".
            Refused by name: marginals together with labels, max_voxels with per_label, a 2-D log_prior without per_label.
        spatial_prior: None / False (default): every voxel is judged on its own.  HipBayesGridSolver's option, the same dict,
            rules, messages and TOML table [Fitting.solver.spatial_prior]: a pairwise Gaussian neighbourhood (MRF) prior between
            adjacent voxels on the RATES (and a free T1), by coloured mean-field sweeps (pnx_curvefit_varpro_posterior_mrf_f64,
            DESIGN.md 4.1q).  A numeric strength applies to the non-linear names only; {name: s} with s > 0 on a fraction or S0
            is a ValueError (its value is solved per voxel and atom: there is no grid value to pull towards).  The precision of a
            rate is strength / (range of its row over the admitted atoms)^2, 0 for a one-value row.  `fit` then needs
            `neighbours` and `colours` (HipPixelWiseFitter passes api.grid_neighbours(mask, connectivity)) and returns the
            results in the caller's order.  With a single-table empirical_prior the table is learned first, without the field.
            Refused by name: together with a per-label or 2-D prior, or with marginals.
            This solver's own key "coupling" (TOML: coupling = "log" in the same table): "linear" (default: the path above, byte for
            byte), "log", or {name: "linear" | "log"} over the non-linear names.  A log-coupled rate is pulled towards its
            neighbours' E[log rate] (pnx_curvefit_varpro_posterior_logmrf_f64), its precision is strength /
            (range of log rate)^2; params_ and posterior_sd stay the moments of the linear rate.  On a geometric rate axis this
            is the coupling to use.  A fraction / S0 name, an unknown value, or a non-positive admitted rate on a log row is a
            ValueError, and so is, from `fit`, three compartments with S0 and a free T1 above 32 b-values (no kernel form);
            diagnostics_ gains "spatial_coupling" {name: str} and, for the log rows that carry a precision, "geo_mean" {name:
            exp E[log rate] per pixel}.  "geo_mean" has two sources that never meet (spatial_prior with marginals is refused):
            here E[log rate] under the field's weights, out of the fold; with `marginals` the same quantity from the marginal.
    After fit: params_ = the posterior mean keyed by the model's names; diagnostics_ {"posterior_sd", "map" (dicts name ->
    (n_pixels,)), "map_atom", "log_evidence", "ess", "clipped_mass", "n_pixels"}, with spatial_prior also {"spatial_sweeps",
    "spatial_delta", "spatial_precision"} as HipBayesGridSolver reports them ("log_evidence" is then the local normaliser of the
    last update), with marginals also {"marginal" {name: (n_bins,
    n_pixels)}, "marginal_values" {name: (n_bins,)}, "quantiles" {name: (n_q, n_pixels)}, "quantile_probs", "geo_mean" {name:
    (n_pixels,)}} (the rates and a free T1 only), with empirical_prior also {"log_prior" (n_atoms,) the learned table, "prior_loglik"
    the EM's log-likelihood trace, "prior_n_iter", "prior_n_voxels"}; pixel_results_ with success = the voxel's signal was finite."""

    _MARGINALS_DEFAULTS = HipBayesGridSolver._MARGINALS_DEFAULTS
    _marginals_options = classmethod(HipBayesGridSolver._marginals_options.__func__)  # one set of rules and messages
    _EMPIRICAL_PRIOR_DEFAULTS = HipBayesGridSolver._EMPIRICAL_PRIOR_DEFAULTS
    _empirical_prior_options = classmethod(HipBayesGridSolver._empirical_prior_options.__func__)  # likewise
    _SPATIAL_PRIOR_DEFAULTS = HipBayesGridSolver._SPATIAL_PRIOR_DEFAULTS
    _spatial_prior_options = classmethod(HipBayesGridSolver._spatial_prior_options.__func__)  # likewise
    colour_sort = staticmethod(HipBayesGridSolver.colour_sort)  # one sort by colour, one way back, for both solvers
    in_colour_order = classmethod(HipBayesGridSolver.in_colour_order.__func__)

    def __init__(self, model: Any, rates=None, max_iter: int = 250, tol: float = 1e-8, p0: dict[str, float] | None = None,
                 bounds: dict[str, tuple[float, float]] | None = None, ordered: bool = True, noise_sd: float | None = None, log_prior=None,
                 marginal_amplitudes: bool = True, sigma=None, device: int = 0, io_dtype: str = "float64", precision: str = "float64",
                 marginals=None, empirical_prior=None, spatial_prior=None, **ignored_reference_kwargs):
        RefBaseSolver.__init__(self, model=model, max_iter=max_iter, tol=tol, verbose=bool(ignored_reference_kwargs.pop("verbose", False)))
        self._kernel_model = kernel_model_key(model)
        self._kernel_t1 = kernel_t1(model)
        spatial_prior, self.spatial_coupling = self._coupling_option(spatial_prior, list(model.param_names))
        self.spatial_prior = self._spatial_prior_options(self._nonlinear_strength(spatial_prior, list(model.param_names)),
                                                         list(model.param_names))
        per_label = False
        if isinstance(empirical_prior, dict) and "per_label" in empirical_prior:  # the grid solver's option, taken out here: the
            empirical_prior = dict(empirical_prior)                               # shared classmethod knows the four others
            per_label = empirical_prior.pop("per_label")
            if not isinstance(per_label, (bool, np.bool_)):
                raise ValueError(f"empirical_prior per_label must be a bool, got {per_label!r}")
        self.empirical_prior = self._empirical_prior_options(empirical_prior)
        if per_label:
            self.empirical_prior["per_label"] = True
        self.marginals = self._marginals_options(marginals)
        if _io_dtype(io_dtype) is not np.float64 or precision != "float64":
            raise ValueError("HipBayesVarProSolver is built for precision='float64' and io_dtype='float64': the posterior reads and "
                             "writes float64 arrays and exponentiates in fp64")
        if rates is None:
            raise ValueError("rates is required: a dict from the name of a non-linear parameter to a sequence of values")
        names = list(model.param_names)
        if bounds is None:
            raise ValueError(f"bounds is required: {{name: (lo, hi)}} for every parameter of {names}")
        _validate_parameter_names(bounds, names)
        self.ordered = bool(ordered)
        self.rates, self._nl_names, self._nl_atoms = _varpro_atoms("rates", model, self._kernel_model, p0, bounds, rates, self.ordered)
        if "S0" in names and not bounds["S0"][0] >= 0:
            raise ValueError(f"the lower bound of S0 must be >= 0 (the fraction bounds scale with S0), got {bounds['S0'][0]}")
        self.noise_sd = 0.0 if noise_sd is None else float(noise_sd)
        if not (np.isfinite(self.noise_sd) and self.noise_sd >= 0.0):
            raise ValueError(f"noise_sd must be None / 0 (marginalised) or a finite positive standard deviation, got {noise_sd!r}")
        self.log_prior = None
        if log_prior is not None:
            lp = np.ascontiguousarray(log_prior, np.float64)
            if lp.ndim == 2 and lp.shape[1] == self._nl_atoms.shape[1] and lp.shape[0] > api.GRID_MAX_CLASSES:
                raise ValueError(f"log_prior has {lp.shape[0]} rows: at most {api.GRID_MAX_CLASSES} classes (labels) are built")
            if not (lp.ndim == 2 and lp.shape[0] >= 2 and lp.shape[1] == self._nl_atoms.shape[1]):  # (1, n_atoms) is the one table, as before
                lp = lp.reshape(-1)
            if lp.ndim == 1 and lp.shape != (self._nl_atoms.shape[1],):
                raise ValueError(f"log_prior has {lp.size} entries for {self._nl_atoms.shape[1]} atoms (one per atom, in the order of the "
                                 "atoms)")
            if np.isnan(lp).any() or (lp == np.inf).any() or not np.isfinite(lp).any(axis=-1).all():
                raise ValueError("log_prior entries must be finite or -inf, at least one of them finite" + (" in every row" if lp.ndim == 2 else ""))
            self.log_prior = lp
        self.marginal_amplitudes = bool(marginal_amplitudes)
        self.sigma = None
        if sigma is not None:
            self.sigma = np.asarray(sigma, float)
            if self.sigma.ndim > 1 and self.sigma.size != 1:
                raise ValueError("HipBayesVarProSolver implements a scalar or 1-D sigma (one standard deviation per b-value)")
            self.sigma = self.sigma.reshape(-1)
        self.p0 = p0
        self.bounds = bounds
        self.device = int(device)
        self.io_dtype = np.float64
        self.solver_kwargs = ignored_reference_kwargs
        if self.needs_labels and self.marginals:
            raise ValueError("HipBayesVarProSolver: marginals are not built with per-label priors (a 2-D log_prior or empirical_prior "
                             "per_label): pnx_curvefit_varpro_marginals_f64 takes one prior table")
        if per_label and self.empirical_prior["max_voxels"]:
            raise ValueError("empirical_prior max_voxels is not built with per_label: every label learns from all of its voxels")
        if self.empirical_prior and not per_label and self.log_prior is not None and self.log_prior.ndim == 2:
            raise ValueError("empirical_prior with a 2-D log_prior needs per_label: a single learned table has no single row to start from")
        if self.spatial_prior and self.needs_labels:
            raise ValueError("HipBayesVarProSolver: spatial_prior is not built with per-label priors (a 2-D log_prior or empirical_prior "
                             "per_label): pnx_curvefit_varpro_posterior_mrf_f64 takes one prior table")
        if self.spatial_prior and self.marginals:
            raise ValueError("HipBayesVarProSolver: spatial_prior is not built with marginals: pnx_curvefit_varpro_marginals_f64 knows no field")
        if self.spatial_prior and self._log_coupled():
            adm = np.ones(self._nl_atoms.shape[1], bool) if self.log_prior is None else self.log_prior > -np.inf
            for j, n in enumerate(self._nl_names):
                if self.spatial_coupling[n] == "log" and not (self._nl_atoms[j, adm] > 0).all():
                    raise ValueError(f"spatial_prior coupling of {n} is 'log', which needs positive values: its admitted atoms reach "
                                     f"{float(self._nl_atoms[j, adm].min())!r}")

    @property
    def needs_labels(self) -> bool:
        """True when `fit` needs `labels`: a 2-D log_prior, or empirical_prior with per_label."""
        return bool((self.log_prior is not None and self.log_prior.ndim == 2) or (self.empirical_prior and self.empirical_prior.get("per_label")))

    @property
    def needs_neighbours(self) -> bool:
        """True when `fit` needs `neighbours` and `colours`: spatial_prior is on."""
        return bool(self.spatial_prior)

    @staticmethod
    def _coupling_option(value, names):
        """(spatial_prior without its "coupling" key -- this solver's only; the shared parser knows the four others --, {name:
        "linear" | "log"} for every parameter).  "linear" (the default) and "log" apply to the non-linear names (the rates, T1); a
        dict gives them by name.  A fraction or S0 is never coupled: naming one is refused."""
        linear = [n for n in names if n.startswith("f") or n == "S0"]
        coupling = {n: "linear" for n in names}
        if not isinstance(value, dict) or "coupling" not in value:
            return value, coupling
        value = dict(value)
        c = value.pop("coupling")
        if isinstance(c, str):
            c = {n: c for n in names if n not in linear}
        if not isinstance(c, dict):
            raise ValueError(f"spatial_prior coupling must be 'linear', 'log' or {{parameter name: 'linear' | 'log'}}, got {c!r}")
        bad = sorted(set(c) - set(names))
        if bad:
            raise ValueError(f"spatial_prior coupling names unknown parameters {bad}; the model has {names}")
        for n, v in c.items():
            if n in linear:
                raise ValueError(f"spatial_prior coupling of {n} cannot be set: a fraction or S0 is solved in closed form per voxel and atom "
                                 "and is not coupled")
            if not isinstance(v, str) or v not in ("linear", "log"):
                raise ValueError(f"spatial_prior coupling of {n} must be 'linear' or 'log', got {v!r}")
            coupling[n] = v
        return value, coupling

    def _log_coupled(self):
        return any(v == "log" for v in self.spatial_coupling.values())

    @staticmethod
    def _nonlinear_strength(value, names):
        """spatial_prior with its strength spelled out per parameter: a number applies to the non-linear names (the rates, T1)
        only; a dict that gives a fraction or S0 a positive strength is refused -- its value is solved per voxel and atom, so there
        is no grid value to pull towards.  Everything else is left to the shared option parser."""
        if not isinstance(value, dict) or value.get("strength") is None:
            return value
        st = value["strength"]
        linear = [n for n in names if n.startswith("f") or n == "S0"]
        if isinstance(st, dict):
            for n in linear:
                v = st.get(n, 0.0)
                if isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and v > 0:
                    raise ValueError(f"spatial_prior strength of {n} must be 0: a fraction or S0 is solved in closed form per voxel and atom "
                                     f"and has no grid value for a neighbourhood prior to pull towards, got {v!r}")
            return value
        if isinstance(st, bool) or not isinstance(st, (int, float, np.integer, np.floating)):
            return value  # the shared parser names the fault
        return {**value, "strength": {n: (0.0 if n in linear else st) for n in names}}

    def spatial_precision(self, log_prior=None):
        """precision (n_free,) of the spatial prior under `log_prior` (None: uniform): strength / range^2 of the row of the rate
        atoms over the admitted atoms, 0 for a one-value row and for every fraction / S0."""
        names = list(self.model.param_names)
        adm = np.ones(self._nl_atoms.shape[1], bool) if log_prior is None else np.asarray(log_prior, float) > -np.inf
        rng = self._nl_atoms[:, adm].max(axis=1) - self._nl_atoms[:, adm].min(axis=1)
        if self._log_coupled():  # a log-coupled row: the range of log theta
            cp = [int(self.spatial_coupling[n] == "log") for n in names]
            frange = api.varpro_logmrf_centre(self._nl_atoms, [n in self._nl_names for n in names], cp, log_prior)[1]
            rng = np.array([frange[names.index(n)] for n in self._nl_names])
        pr = np.zeros(len(names))
        for j, n in enumerate(self._nl_names):
            if rng[j] > 0.0:
                pr[names.index(n)] = self.spatial_prior["strength"][n] / rng[j] ** 2
        return pr

    label_rows = staticmethod(HipBayesGridSolver.label_rows)  # one mapping from label values to rows for both solvers

    def _fit_labelled(self, xdata, ydata, labels, lo, hi, common):
        """(posterior result, learned or None) under one prior row per label: HipBayesGridSolver._fit_labelled over the rate atoms."""
        n_pixels = ydata.shape[0]
        if labels is None:
            raise ValueError("HipBayesVarProSolver: labels (n_pixels,) is required with a 2-D log_prior or empirical_prior per_label")
        per_label = bool(self.empirical_prior and self.empirical_prior.get("per_label"))
        table = self.log_prior
        if per_label:
            values, rows = self.label_rows(labels, n_pixels)
            n_classes = max(int(values.size), 1)
            if table is not None and table.ndim == 2 and table.shape[0] != n_classes:
                raise ValueError(f"log_prior has {table.shape[0]} rows for the {n_classes} distinct labels of this call")
            if table is not None and table.ndim == 1:
                table = np.ascontiguousarray(np.broadcast_to(table, (n_classes, table.size)))
        else:  # the caller's table: label c is row c, anything else is background
            n_classes = table.shape[0]
            lab = np.asarray(labels)
            if lab.shape != (n_pixels,) or lab.dtype.kind not in "iuf":
                raise ValueError(f"labels must be {n_pixels} integers (one per pixel), got shape {lab.shape} and dtype {lab.dtype}")
            rows = np.where((lab >= 0) & (lab < n_classes) & (lab == np.floor(lab)), lab, -1).astype(np.int32)
        learned = None
        if per_label:
            ep = self.empirical_prior
            learned = api.varpro_prior_em_classes(self._kernel_model, xdata, ydata, self._nl_atoms, lo, hi, rows, n_classes, log_prior=table,
                                                  n_iter=ep["n_iter"], pseudo_count=ep["pseudo_count"], rel_tol=ep["rel_tol"], **common)
            learned["n_voxels"] = n_pixels
            learned["labels"] = values
            table = learned["log_prior"]
        res = api.varpro_posterior_classes(self._kernel_model, xdata, ydata, self._nl_atoms, lo, hi, rows, n_classes, log_prior=table, **common)
        return res, learned

    def fit(self, xdata: np.ndarray, ydata: np.ndarray, pixel_fixed_params=None, labels=None, neighbours=None, colours=None,
            **fit_kwargs) -> "HipBayesVarProSolver":
        if pixel_fixed_params:
            raise ValueError("HipBayesVarProSolver is not built with per-pixel fixed parameters (pixel_fixed_params): the dictionary "
                             "would differ from voxel to voxel")
        self._reset_state()
        xdata = np.asarray(xdata)
        ydata = np.asarray(ydata)
        _validate_data_shapes(xdata, ydata)
        if ydata.ndim == 1:
            ydata = ydata[np.newaxis, :]
        if ydata.ndim > 2:
            raise ValueError(f"ydata must be 1D or 2D array, but got shape {ydata.shape}.")
        n_pixels = ydata.shape[0]
        names = list(self.model.param_names)
        all_names = list(self.model._all_param_names)
        fixed = getattr(self.model, "fixed_params", None) or {}
        fixed_idx = [i for i, n in enumerate(all_names) if n in fixed]
        fixed_vals = np.array([float(fixed[all_names[i]]) for i in fixed_idx]) if fixed_idx else None
        lo = np.array([self.bounds[n][0] for n in names], float)
        hi = np.array([self.bounds[n][1] for n in names], float)
        if self.spatial_prior and self._log_coupled() and self._kernel_model == "tri_s0" and self._nl_atoms.shape[0] == 4 and xdata.size > 32:
            raise ValueError(f"spatial_prior coupling 'log' is not built for three compartments with S0 and a free T1 above 32 b-values "
                             f"(got {xdata.size}): its fold does not fit the register file; coupling 'linear' takes this layout")
        log_prior, learned, coupled = self.log_prior, None, None
        if self.needs_labels:
            res, learned = self._fit_labelled(xdata, ydata, labels, lo, hi,
                                              dict(noise_sd=self.noise_sd, marginal_amplitudes=self.marginal_amplitudes, fixed_idx=fixed_idx,
                                                   fixed_vals=fixed_vals, sigma=self.sigma, device=self.device, **self._kernel_t1))
        elif self.empirical_prior:
            ep = self.empirical_prior
            step = 1 if ep["max_voxels"] is None else -(-n_pixels // ep["max_voxels"])
            sample = ydata[::step]
            learned = api.varpro_prior_em(self._kernel_model, xdata, sample, self._nl_atoms, lo, hi, log_prior=self.log_prior,
                                          noise_sd=self.noise_sd, marginal_amplitudes=self.marginal_amplitudes, n_iter=ep["n_iter"],
                                          pseudo_count=ep["pseudo_count"], rel_tol=ep["rel_tol"], fixed_idx=fixed_idx, fixed_vals=fixed_vals,
                                          sigma=self.sigma, device=self.device, **self._kernel_t1)
            learned["n_voxels"] = sample.shape[0]
            log_prior = learned["log_prior"]
        if self.spatial_prior:
            if neighbours is None or colours is None:
                raise ValueError("HipBayesVarProSolver: neighbours (n_pixels, n_nb) and colours (n_pixels,) are required with spatial_prior "
                                 "(api.grid_neighbours(mask, connectivity); HipPixelWiseFitter passes them)")
            precision, sp = self.spatial_precision(log_prior), self.spatial_prior
            # the flags the device sees: a row without a precision (strength 0, a one-value row) is not coupled at all
            coupled = np.array([int(self.spatial_coupling[n] == "log" and precision[i] > 0) for i, n in enumerate(names)], np.int32)
            call = api.varpro_posterior_mrf if not self._log_coupled() else (
                lambda *a, **kw: api.varpro_posterior_logmrf(*a, coupled, **kw))  # all linear: the linear entry point, as before
            res = self.in_colour_order(
                ydata, neighbours, colours, precision,
                ("mean", "sd", "map_p", "map_atom", "log_evidence", "ess", "clipped_mass", "field_mean"),
                lambda y, nb, start: call(self._kernel_model, xdata, y, self._nl_atoms, lo, hi, nb, start, precision,
                                          n_sweeps=sp["n_sweeps"], tol=sp["tol"], log_prior=log_prior,
                                          noise_sd=self.noise_sd, marginal_amplitudes=self.marginal_amplitudes,
                                          fixed_idx=fixed_idx, fixed_vals=fixed_vals, sigma=self.sigma, device=self.device,
                                          **self._kernel_t1))
        elif not self.needs_labels:
            res = api.varpro_posterior(self._kernel_model, xdata, ydata, self._nl_atoms, lo, hi, log_prior=log_prior, noise_sd=self.noise_sd,
                                       marginal_amplitudes=self.marginal_amplitudes, fixed_idx=fixed_idx, fixed_vals=fixed_vals,
                                       sigma=self.sigma, device=self.device, **self._kernel_t1)
        mean, atom = res["mean"], res["map_atom"]
        self.pixel_results_ = PixelResultsView(mean.T, None, atom >= 0,
                                               lambda i, a=atom: None if a[i] >= 0 else _BAYES_MESSAGES[-2])
        self.params_ = {name: [float(mean[i, 0])] if n_pixels == 1 else mean[i] for i, name in enumerate(names)}
        self.diagnostics_ = {"posterior_sd": {n: res["sd"][i] for i, n in enumerate(names)},
                             "map": {n: res["map_p"][i] for i, n in enumerate(names)}, "map_atom": atom,
                             "log_evidence": res["log_evidence"], "ess": res["ess"], "clipped_mass": res["clipped_mass"],
                             "n_pixels": n_pixels}
        if learned is not None:
            self.diagnostics_.update({"log_prior": learned["log_prior"], "prior_loglik": learned["loglik"], "prior_n_iter": learned["n_iter"],
                                      "prior_n_voxels": learned["n_voxels"]})
            if "labels" in learned:
                self.diagnostics_.update({"prior_loglik": learned["loglik_class"], "prior_loglik_total": learned["loglik"],
                                          "prior_n_eff": learned["n_eff"], "prior_labels": [int(v) for v in learned["labels"]]})
        if self.spatial_prior:
            self.diagnostics_.update({"spatial_sweeps": res["n_sweeps"], "spatial_delta": res["delta"],
                                      "spatial_precision": {n: float(res["precision"][i]) for i, n in enumerate(names)},
                                      "spatial_coupling": dict(self.spatial_coupling)})
            if coupled is not None and "field_mean" in res:  # exp E[log theta] of the rows the device coupled in the logarithm; NaN where mean is
                self.diagnostics_["geo_mean"] = {n: np.exp(res["field_mean"][i]) for i, n in enumerate(names) if coupled[i]}
        if self.marginals:
            mg = api.varpro_marginals(self._kernel_model, xdata, ydata, self._nl_atoms, lo, hi, log_prior=log_prior, noise_sd=self.noise_sd,
                                      marginal_amplitudes=self.marginal_amplitudes, quantiles=self.marginals["quantiles"], fixed_idx=fixed_idx,
                                      fixed_vals=fixed_vals, sigma=self.sigma, device=self.device, **self._kernel_t1)
            self.diagnostics_.update({"marginal": {names[k]: m for k, m in mg["marginal"].items()},
                                      "marginal_values": {names[k]: v for k, v in mg["values"].items()},
                                      "quantiles": {names[k]: q for k, q in mg["quantiles"].items()},
                                      "quantile_probs": mg["quantile_probs"],
                                      "geo_mean": {names[k]: g for k, g in mg["geo_mean"].items()}})
        return self


class HipNNLSSolver(NNLSBase):
    """Batched regularised NNLS on MI355X with `scipy.optimize.nnls` semantics (nnls_solver.py:18-210)."""

    def __init__(self, model: Any, reg_order: int = 0, mu: float = 0.02, max_iter: int = 250, tol: float = 1e-8,
                 verbose=False, multi_threading: bool = False, **solver_kwargs: Any) -> None:
        self.device = int(solver_kwargs.pop("device", 0))
        self.n_gpus = int(solver_kwargs.pop("n_gpus", 1))
        self.io_dtype = _io_dtype(solver_kwargs.pop("io_dtype", "float64"))  # "float32": fp32 signal in / spectra out
        if HAVE_PYNEAPPLE:
            super().__init__(model, reg_order=reg_order, mu=mu, max_iter=max_iter, tol=tol, verbose=verbose,
                             multi_threading=multi_threading, **solver_kwargs)
        else:
            RefBaseSolver.__init__(self, model, max_iter, tol, verbose)
            self.multi_threading = multi_threading
            self.n_pools = solver_kwargs.pop("n_pools", None)
            self.reg_order = reg_order
            self.mu = mu

    def get_regularization_matrix(self) -> np.ndarray:
        """(n_bins, n_bins) Tikhonov matrix, model_functions/nnls.py:46-85."""
        return api.nnls_regularization_matrix(self.model.n_bins, self.reg_order, self.mu)

    def _build_regularized_basis(self, xdata: np.ndarray) -> np.ndarray:
        return np.concatenate([self.model.get_basis(xdata), self.get_regularization_matrix()], axis=0)

    def _extend_signal(self, signal: np.ndarray) -> np.ndarray:
        """Kept for interface parity (nnls_solver.py:75-86); the HIP path never materialises it."""
        return np.concatenate((signal, np.zeros((signal.shape[0], self.model.n_bins))), axis=1)

    def fit_peaks(self, xdata: np.ndarray, signal: np.ndarray, height: float = 0.1, cutoffs=None, max_peaks: int = 8,
                  regularized: bool | None = None, r_squared: bool = False) -> "HipNNLSSolver":
        """Fit and reduce every spectrum to its peak table on the device (pnx_nnls_solve_peaks_f64): what a caller of the
        reference does with `fit` followed by a Python loop over `find_spectrum_peaks` / `apply_cutoffs`
        (utility/spectrum.py:51-215), without the (n_pixels, n_bins) coefficient array -- 8.4 GB for a 256 x 256 x 64
        volume -- crossing PCIe.  `regularized` defaults to reg_order != 0 (spectrum.py:68-71).
        params_: "d_values", "f_values" (n_pixels, max_peaks) NaN padded, "n_peaks", and with `cutoffs` "d_cut", "f_cut".
        r_squared: also reduce every spectrum's data-term residual while it is resident (pnx_nnls_solve_peaks_stats_f64) and
        SS_tot on the device; diagnostics_ then carries "ss_res" and "r_squared" (NaN for a constant signal, fitters/base.py:179-183)."""
        self._reset_state()
        xdata = np.asarray(xdata, float)
        signal = np.asarray(signal, float)
        basis = np.asarray(self.model.get_basis(xdata), float)
        if signal.ndim == 1:
            signal = signal[np.newaxis, :]
        if signal.ndim != 2 or signal.shape[1] != basis.shape[0]:
            raise ValueError(f"signal shape {signal.shape} does not match the basis ({basis.shape[0]} measurements)")
        self.n_pixels = signal.shape[0]
        plan = api.NnlsPlan(basis, self.get_regularization_matrix(), self.device)
        try:
            res = plan.solve_peaks(np.ascontiguousarray(signal), np.asarray(self.model.bins, float),
                                   int(self.max_iter) if self.max_iter else 0, height=height,
                                   regularized=bool(self.reg_order) if regularized is None else regularized,
                                   max_peaks=max_peaks, cutoffs=cutoffs, **({"with_ss_res": True} if r_squared else {}))
        finally:
            plan.close()
        for key in ("d_values", "f_values", "n_peaks", "d_cut", "f_cut"):
            if res[key] is not None:
                self.params_[key] = res[key]
        self.diagnostics_.update(residual=res["residual"], status=res["status"], iters=res["iters"])
        if r_squared:
            ss_tot = api.row_ss_tot(signal, self.device)
            with np.errstate(divide="ignore", invalid="ignore"):
                r2 = np.where(ss_tot > 0, 1.0 - res["ss_res"] / ss_tot, np.nan)
            self.diagnostics_.update(ss_res=res["ss_res"], r_squared=r2)
        return self

    def fit(self, xdata: np.ndarray, signal: np.ndarray, pixel_fixed_params=None, **kwargs) -> "HipNNLSSolver":
        self._reset_state()
        xdata = np.asarray(xdata, float)
        signal = np.asarray(signal, self.io_dtype)
        basis = np.asarray(self.model.get_basis(xdata), float)
        reg = self.get_regularization_matrix()
        if signal.ndim == 1:
            signal = signal[np.newaxis, :]
        if signal.ndim != 2 or signal.shape[1] != basis.shape[0]:
            raise ValueError(f"signal shape {signal.shape} does not match the basis ({basis.shape[0]} measurements)")
        self.n_pixels = signal.shape[0]
        signal = np.ascontiguousarray(signal)
        n_dev = max(1, min(self.n_gpus, self.n_pixels))
        # SciPy: `if not maxiter: maxiter = 3*n` (scipy/optimize/_nnls.py:93-94)
        max_iter = int(self.max_iter) if self.max_iter else 0
        if n_dev == 1:
            res = api.nnls(basis, reg, signal, max_iter, self.device)
        else:
            parts = _split(self.n_pixels, n_dev)
            # every result is voxel-major: the shards write into row ranges of the full arrays (the spectra are 2 KB per voxel)
            res = {"coefficients": np.empty((self.n_pixels, basis.shape[1]), signal.dtype), "residual": np.empty(self.n_pixels, signal.dtype),
                   "status": np.empty(self.n_pixels, np.int8), "iters": np.empty(self.n_pixels, np.int32)}
            def work(k):
                dev_k = _shard_device(self.device, k)
                with pinned_to_gpu(dev_k):  # this thread and the call's helper threads stay on the NUMA node of their GPU
                    api.nnls(basis, reg, signal[parts[k][0]:parts[k][1]], max_iter, dev_k,
                             out={key: v[parts[k][0]:parts[k][1]] for key, v in res.items()})

            with ThreadPoolExecutor(len(parts)) as ex:
                list(ex.map(work, range(len(parts))))
        status = res["status"]
        self.pixel_results_ = PixelResultsView(
            res["coefficients"], None, status == 1,
            lambda i, st=status: None if st[i] == 1 else _NNLS_MESSAGES.get(int(st[i]), "fit failed"),
            residual=res["residual"])
        self.params_["coefficients"] = res["coefficients"]
        self.diagnostics_["residual"] = res["residual"]
        self.diagnostics_["status"] = status
        self.diagnostics_["iters"] = res["iters"]
        return self

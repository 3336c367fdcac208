"""ctypes binding of libpnx_hip.so (the C ABI in include/pnx.h).

The product path has no CPU fallback: if the HIP library is missing or no MI355X is visible the
functions below raise -- they never route through oracle/ or SciPy.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PNX_LIB") or os.path.join(_HERE, "libpnx_hip.so")  # PNX_LIB: load another build (kernel-variant experiments)

PNX_MAX_PARAMS = 8
MEM_HOST, MEM_DEVICE = 0, 1
JAC_FD, JAC_ANALYTIC = 0, 1

# every symbol include/pnx.h declares (tests/test_abi.py checks the library exports all of them)
ABI_SYMBOLS = [
    "pnx_version", "pnx_device_count", "pnx_last_error", "pnx_model_n_params", "pnx_curvefit_batch_f64",
    "pnx_curvefit_batch_f32", "pnx_nnls_solve_f32",
    "pnx_nnls_plan_create", "pnx_nnls_plan_destroy", "pnx_nnls_solve_f64", "pnx_nnls_aty_f64", "pnx_nnls_batch_f64",
    "pnx_nnls_bins", "pnx_nnls_basis", "pnx_nnls_regularization_matrix", "pnx_sweep_f32", "pnx_sweep_f64",
    "pnx_resize2d_f64", "pnx_ideal_bounds_f64", "pnx_nnls_spectrum_peaks_f64", "pnx_nnls_solve_peaks_f64", "pnx_scatter_maps_f32",
    "pnx_mask_select_f64", "pnx_gather_rows_f64", "pnx_scatter_rows_t_f64", "pnx_row_ss_tot_f64", "pnx_upload", "pnx_download",
    "pnx_label_sums_f64", "pnx_release_staging", "pnx_queue_order_f64",
    "pnx_nnls_fit_stats_f64", "pnx_nnls_solve_peaks_stats_f64", "pnx_curvefit_predict_f64", "pnx_curvefit_fast_f32",
    "pnx_curvefit_simplex_f64", "pnx_ideal_bounds_simplex_f64", "pnx_curvefit_grid_start_f64",
    "pnx_curvefit_grid_posterior_f64", "pnx_curvefit_grid_prior_em_f64", "pnx_curvefit_varpro_f64", "pnx_curvefit_varpro_posterior_f64",
    "pnx_curvefit_grid_marginals_f64", "pnx_curvefit_varpro_marginals_f64", "pnx_curvefit_varpro_prior_em_f64",
    "pnx_loglinear_f64", "pnx_loglinear_f32", "pnx_peel_f64", "pnx_peel_f32",
    "pnx_curvefit_grid_posterior_classes_f64", "pnx_curvefit_grid_prior_em_classes_f64",
    "pnx_curvefit_varpro_posterior_classes_f64", "pnx_curvefit_varpro_prior_em_classes_f64",
    "pnx_curvefit_grid_neighbour_field_f64", "pnx_curvefit_grid_posterior_field_f64", "pnx_curvefit_grid_posterior_mrf_f64",
    "pnx_curvefit_varpro_posterior_field_f64", "pnx_curvefit_varpro_posterior_mrf_f64",
    "pnx_curvefit_varpro_posterior_logfield_f64", "pnx_curvefit_varpro_posterior_logmrf_f64",
    "pnx_curvefit_grid_neighbour_wfield_f64", "pnx_curvefit_grid_posterior_wfield_f64", "pnx_curvefit_grid_posterior_tmrf_f64",
    "pnx_curvefit_grid_posterior_rician_f64", "pnx_log_i0e_f64", "pnx_curvefit_grid_refine_f64",
]


class PnxError(RuntimeError):
    """A call through the C ABI failed (code < 0)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"pnx error {code}: {msg}")
        self.code = code


class CurvefitOpts(C.Structure):
    _fields_ = [
        ("model", C.c_int32), ("n_b", C.c_int32), ("n_free", C.c_int32), ("n_fixed", C.c_int32),
        ("free_idx", C.c_int32 * PNX_MAX_PARAMS), ("fixed_idx", C.c_int32 * PNX_MAX_PARAMS),
        ("per_voxel_p0_bounds", C.c_int32), ("fixed_per_voxel", C.c_int32), ("max_nfev", C.c_int32),
        ("jac_mode", C.c_int32), ("t1_mode", C.c_int32), ("absolute_sigma", C.c_int32), ("tr", C.c_double),
        ("tm", C.c_double), ("ftol", C.c_double), ("xtol", C.c_double), ("gtol", C.c_double),
        ("sigma", C.c_void_p),        # (n_b,) float64 on the host, or None
        ("queue_order", C.c_void_p),  # (n_vox,) int32 on the device, or None (device-mode calls only)
    ]


_lib = None


def _preload_hip_runtime():
    """Make libpnx_hip.so and PyTorch share ONE HIP runtime.

    PyTorch-ROCm wheels bundle their own `libamdhip64.so` (SONAME libamdhip64.so.7).  If libpnx_hip.so were
    loaded first it would pull in /opt/rocm's copy, torch would then load its bundled one, and the process would
    hold two HIP runtimes (streams / device pointers of one are meaningless to the other; the second one does
    not even see the GPU).  Loading torch's copy first registers the SONAME, so libpnx_hip.so binds to it.
    Without PyTorch installed the system ROCm runtime is used.
    """
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """Load libpnx_hip.so (building it is __graft_entry__.build()'s / `python -m pyneapple_amd._build`'s job)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP extension first (python -m pyneapple_amd._build). "
            "pyneapple_amd has no CPU fallback.")
    _preload_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    vp, dp, fp = C.c_void_p, C.c_void_p, C.c_void_p
    lib.pnx_version.restype = C.c_int
    lib.pnx_release_staging.argtypes = [C.c_int]
    lib.pnx_queue_order_f64.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
    lib.pnx_queue_order_f64.restype = C.c_int
    lib.pnx_release_staging.restype = C.c_int
    lib.pnx_device_count.restype = C.c_int
    lib.pnx_last_error.restype = C.c_int
    lib.pnx_last_error.argtypes = [C.c_char_p, C.c_int]
    lib.pnx_model_n_params.restype = C.c_int
    lib.pnx_model_n_params.argtypes = [C.c_int]
    lib.pnx_curvefit_batch_f64.restype = C.c_int
    lib.pnx_curvefit_batch_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, dp, dp, dp, dp, dp, dp, vp, vp,
                                           dp, C.c_int, C.c_int, vp]
    lib.pnx_curvefit_batch_f32.restype = C.c_int
    lib.pnx_curvefit_batch_f32.argtypes = lib.pnx_curvefit_batch_f64.argtypes  # all data pointers are void*
    lib.pnx_curvefit_fast_f32.restype = C.c_int
    lib.pnx_curvefit_fast_f32.argtypes = lib.pnx_curvefit_batch_f64.argtypes
    lib.pnx_curvefit_simplex_f64.restype = C.c_int  # pnx_curvefit_batch_f64's arguments, then lambda and face in front of mem
    lib.pnx_curvefit_simplex_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, dp, dp, dp, dp, dp, dp, vp, vp,
                                             dp, dp, vp, C.c_int, C.c_int, vp]
    lib.pnx_curvefit_grid_start_f64.restype = C.c_int  # opts, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project, p0_out, best, cost
    lib.pnx_curvefit_grid_start_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, C.c_int, dp, vp, dp,
                                                C.c_int, C.c_int, vp]
    lib.pnx_curvefit_grid_posterior_f64.restype = C.c_int  # grid start's inputs, log_prior, noise_sd, mean, sd, map_atom, map_p, log_evidence, ess
    lib.pnx_curvefit_grid_posterior_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, C.c_int, dp, C.c_double,
                                                    dp, dp, vp, dp, dp, dp, C.c_int, C.c_int, vp]
    # the posterior's inputs, n_iter, pseudo_count, rel_tol, log_prior_out, loglik, n_iter_done, n_eff
    lib.pnx_curvefit_grid_prior_em_f64.restype = C.c_int
    lib.pnx_curvefit_grid_prior_em_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, C.c_int, dp, C.c_double,
                                                   C.c_int, C.c_double, C.c_double, dp, dp, C.POINTER(C.c_int), C.POINTER(C.c_int64),
                                                   C.c_int, C.c_int, vp]
    # the Rician likelihood: the posterior's arguments without project_amplitude; log I0e per element
    lib.pnx_curvefit_grid_posterior_rician_f64.restype = C.c_int
    lib.pnx_curvefit_grid_posterior_rician_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, dp, C.c_double,
                                                           dp, dp, vp, dp, dp, dp, C.c_int, C.c_int, vp]
    lib.pnx_curvefit_grid_refine_f64.restype = C.c_int
    lib.pnx_curvefit_grid_refine_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, dp, dp, dp, C.c_int, C.c_double, vp, dp, dp, dp, dp, dp,
                                                 dp, dp, dp, C.c_int, C.c_int, vp]
    lib.pnx_log_i0e_f64.restype = C.c_int
    lib.pnx_log_i0e_f64.argtypes = [C.c_int64, dp, dp, C.c_int, C.c_int, vp]
    # the unlabelled calls' arguments with n_classes, labels in front of log_prior (n_classes, n_atoms); the EM's loglik_class behind loglik
    lib.pnx_curvefit_grid_posterior_classes_f64.restype = C.c_int
    lib.pnx_curvefit_grid_posterior_classes_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, C.c_int, C.c_int,
                                                            vp, dp, C.c_double, dp, dp, vp, dp, dp, dp, C.c_int, C.c_int, vp]
    lib.pnx_curvefit_grid_prior_em_classes_f64.restype = C.c_int
    lib.pnx_curvefit_grid_prior_em_classes_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, C.c_int, C.c_int,
                                                           vp, dp, C.c_double, C.c_int, C.c_double, C.c_double, dp, dp, dp,
                                                           C.POINTER(C.c_int), vp, C.c_int, C.c_int, vp]
    # the neighbourhood (MRF) prior: the gather; the posterior's arguments with first, count, field_q, field_n, precision in front of
    # the outputs and delta_max behind them; the driver with n_nb, neighbours, n_colours, colour_start, precision, n_sweeps, tol
    lib.pnx_curvefit_grid_neighbour_field_f64.restype = C.c_int
    lib.pnx_curvefit_grid_neighbour_field_f64.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, vp, dp, dp, dp, dp, vp, vp,
                                                          C.c_int, C.c_int, vp]
    lib.pnx_curvefit_grid_posterior_field_f64.restype = C.c_int
    lib.pnx_curvefit_grid_posterior_field_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, C.c_int, dp,
                                                          C.c_double, C.c_int64, C.c_int64, dp, vp, dp, dp, dp, vp, dp, dp, dp, dp, C.c_int,
                                                          C.c_int, vp]
    lib.pnx_curvefit_grid_posterior_mrf_f64.restype = C.c_int
    lib.pnx_curvefit_grid_posterior_mrf_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, C.c_int, dp,
                                                        C.c_double, C.c_int, vp, C.c_int, vp, dp, C.c_int, C.c_double, dp, dp, vp, dp, dp, dp,
                                                        dp, C.POINTER(C.c_int), C.c_int, C.c_int, vp]
    # the edge-preserving (Student-t) prior: the gather with sd behind mean, dof behind precision, field_w and edge_weight; the field
    # posterior with field_w (double) in field_n's place; the driver with dof behind precision and field_w, field_n in front of delta
    lib.pnx_curvefit_grid_neighbour_wfield_f64.restype = C.c_int
    lib.pnx_curvefit_grid_neighbour_wfield_f64.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, vp, dp, dp, dp, dp, C.c_double,
                                                           dp, dp, vp, dp, vp, C.c_int, C.c_int, vp]
    lib.pnx_curvefit_grid_posterior_wfield_f64.restype = C.c_int
    lib.pnx_curvefit_grid_posterior_wfield_f64.argtypes = list(lib.pnx_curvefit_grid_posterior_field_f64.argtypes)
    lib.pnx_curvefit_grid_posterior_tmrf_f64.restype = C.c_int
    lib.pnx_curvefit_grid_posterior_tmrf_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, C.c_int, dp,
                                                         C.c_double, C.c_int, vp, C.c_int, vp, dp, C.c_double, C.c_int, C.c_double, dp, dp, vp,
                                                         dp, dp, dp, dp, vp, dp, C.POINTER(C.c_int), C.c_int, C.c_int, vp]
    # the posterior's inputs, n_bins, bin_of, bin_value, n_q, probs, marginal, quantile, log_evidence
    lib.pnx_curvefit_grid_marginals_f64.restype = C.c_int
    lib.pnx_curvefit_grid_marginals_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, C.c_int, dp, C.c_double,
                                                    vp, vp, dp, C.c_int, dp, dp, dp, dp, C.c_int, C.c_int, vp]
    lib.pnx_curvefit_varpro_f64.restype = C.c_int  # opts, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, fallback, p_out, best, cost, clipped
    lib.pnx_curvefit_varpro_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, dp, dp, vp, dp, vp,
                                            C.c_int, C.c_int, vp]
    # the variable projection's inputs (no fallback), log_prior, noise_sd, marginal_amplitudes, mean, sd, map_atom, map_p, log_evidence, ess, clipped_mass
    lib.pnx_curvefit_varpro_posterior_f64.restype = C.c_int
    lib.pnx_curvefit_varpro_posterior_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, dp, C.c_double, C.c_int,
                                                      dp, dp, vp, dp, dp, dp, dp, C.c_int, C.c_int, vp]
    # the neighbourhood (MRF) prior: the varpro posterior's arguments with first, count, field_q, field_n, precision in front of the
    # outputs and delta_max behind them; the driver with n_nb, neighbours, n_colours, colour_start, precision, n_sweeps, tol
    lib.pnx_curvefit_varpro_posterior_field_f64.restype = C.c_int
    lib.pnx_curvefit_varpro_posterior_field_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, dp, C.c_double,
                                                            C.c_int, C.c_int64, C.c_int64, dp, vp, dp, dp, dp, vp, dp, dp, dp, dp, dp, C.c_int,
                                                            C.c_int, vp]
    lib.pnx_curvefit_varpro_posterior_mrf_f64.restype = C.c_int
    lib.pnx_curvefit_varpro_posterior_mrf_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, dp, C.c_double,
                                                          C.c_int, C.c_int, vp, C.c_int, vp, dp, C.c_int, C.c_double, dp, dp, vp, dp, dp, dp, dp,
                                                          dp, C.POINTER(C.c_int), C.c_int, C.c_int, vp]
    # the same two with coupling (int32, host) behind precision and field_mean behind clipped_mass
    lib.pnx_curvefit_varpro_posterior_logfield_f64.restype = C.c_int
    lib.pnx_curvefit_varpro_posterior_logfield_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, dp,
                                                               C.c_double, C.c_int, C.c_int64, C.c_int64, dp, vp, dp, vp, dp, dp, vp, dp, dp,
                                                               dp, dp, dp, dp, C.c_int, C.c_int, vp]
    lib.pnx_curvefit_varpro_posterior_logmrf_f64.restype = C.c_int
    lib.pnx_curvefit_varpro_posterior_logmrf_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, dp, C.c_double,
                                                             C.c_int, C.c_int, vp, C.c_int, vp, dp, vp, C.c_int, C.c_double, dp, dp, vp, dp, dp,
                                                             dp, dp, dp, dp, C.POINTER(C.c_int), C.c_int, C.c_int, vp]
    # the varpro posterior's inputs, n_iter, pseudo_count, rel_tol, log_prior_out, loglik, n_iter_done, n_eff
    lib.pnx_curvefit_varpro_prior_em_f64.restype = C.c_int
    lib.pnx_curvefit_varpro_prior_em_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, dp, C.c_double, C.c_int,
                                                     C.c_int, C.c_double, C.c_double, dp, dp, C.POINTER(C.c_int), C.POINTER(C.c_int64),
                                                     C.c_int, C.c_int, vp]
    # the unlabelled varpro calls' arguments with n_classes, labels in front of log_prior (n_classes, n_atoms); the EM's loglik_class behind loglik
    lib.pnx_curvefit_varpro_posterior_classes_f64.restype = C.c_int
    lib.pnx_curvefit_varpro_posterior_classes_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, C.c_int, vp, dp,
                                                              C.c_double, C.c_int, dp, dp, vp, dp, dp, dp, dp, C.c_int, C.c_int, vp]
    lib.pnx_curvefit_varpro_prior_em_classes_f64.restype = C.c_int
    lib.pnx_curvefit_varpro_prior_em_classes_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, C.c_int, vp, dp,
                                                             C.c_double, C.c_int, C.c_int, C.c_double, C.c_double, dp, dp, dp,
                                                             C.POINTER(C.c_int), vp, C.c_int, C.c_int, vp]
    # the posterior's inputs, n_bins, bin_of, bin_value, n_q, probs, marginal, quantile, geo_mean, log_evidence
    lib.pnx_curvefit_varpro_marginals_f64.restype = C.c_int
    lib.pnx_curvefit_varpro_marginals_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, dp, dp, C.c_int, dp, dp, dp, dp, dp, C.c_double, C.c_int,
                                                      vp, vp, dp, C.c_int, dp, dp, dp, dp, dp, C.c_int, C.c_int, vp]
    lib.pnx_loglinear_f64.restype = C.c_int  # n_vox, n_b, b, use, weighting, n_reweight, clip, lo, hi, y, params, pcov, status, n_used, ss_res
    lib.pnx_loglinear_f64.argtypes = [C.c_int64, C.c_int, dp, vp, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, dp, vp, vp, dp,
                                      C.c_int, C.c_int, vp]
    lib.pnx_loglinear_f32.restype = C.c_int
    lib.pnx_loglinear_f32.argtypes = lib.pnx_loglinear_f64.argtypes  # all data pointers are void*
    lib.pnx_peel_f64.restype = C.c_int  # model, n_vox, n_b, b, use, weighting, clip, lo, hi, fallback, y, params, status, n_used, ss_res
    lib.pnx_peel_f64.argtypes = [C.c_int, C.c_int64, C.c_int, dp, vp, C.c_int, C.c_int, dp, dp, dp, dp, dp, vp, vp, dp,
                                 C.c_int, C.c_int, vp]
    lib.pnx_peel_f32.restype = C.c_int
    lib.pnx_peel_f32.argtypes = lib.pnx_peel_f64.argtypes  # all data pointers are void*
    lib.pnx_nnls_plan_create.restype = C.c_int
    lib.pnx_nnls_plan_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, dp, dp, C.c_int, C.c_int]
    lib.pnx_nnls_plan_destroy.restype = C.c_int
    lib.pnx_nnls_plan_destroy.argtypes = [vp]
    lib.pnx_nnls_solve_f64.restype = C.c_int
    lib.pnx_nnls_solve_f64.argtypes = [vp, C.c_int64, dp, C.c_int, dp, dp, vp, vp, C.c_int, vp]
    lib.pnx_resize2d_f64.restype = C.c_int
    lib.pnx_resize2d_f64.argtypes = [vp, C.c_int, C.c_int, C.c_int64, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    lib.pnx_ideal_bounds_f64.restype = C.c_int
    lib.pnx_ideal_bounds_f64.argtypes = [vp, C.c_int64, C.c_int, dp, dp, dp, vp, vp, vp, C.c_int, vp]
    lib.pnx_ideal_bounds_simplex_f64.restype = C.c_int  # pnx_ideal_bounds_f64's arguments, i_f1 and i_f2 behind tol
    lib.pnx_ideal_bounds_simplex_f64.argtypes = [vp, C.c_int64, C.c_int, dp, dp, dp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp]
    lib.pnx_nnls_solve_f32.restype = C.c_int
    lib.pnx_nnls_solve_f32.argtypes = lib.pnx_nnls_solve_f64.argtypes
    lib.pnx_nnls_aty_f64.restype = C.c_int
    lib.pnx_nnls_aty_f64.argtypes = [vp, C.c_int64, vp, vp, vp]
    lib.pnx_nnls_batch_f64.restype = C.c_int
    lib.pnx_nnls_batch_f64.argtypes = [C.c_int64, C.c_int, C.c_int, dp, dp, C.c_int, dp, C.c_int, dp, dp, vp, vp,
                                       C.c_int]
    lib.pnx_nnls_bins.restype = C.c_int
    lib.pnx_nnls_bins.argtypes = [C.c_double, C.c_double, C.c_int, dp]
    lib.pnx_nnls_basis.restype = C.c_int
    lib.pnx_nnls_basis.argtypes = [C.c_int, dp, C.c_int, dp, dp, C.c_int]
    lib.pnx_nnls_regularization_matrix.restype = C.c_int
    lib.pnx_nnls_regularization_matrix.argtypes = [C.c_int, C.c_int, C.c_double, dp]
    lib.pnx_nnls_spectrum_peaks_f64.restype = C.c_int
    lib.pnx_nnls_spectrum_peaks_f64.argtypes = [C.c_int64, C.c_int, vp, dp, C.c_double, C.c_int, C.c_double, C.c_int, vp, vp, vp,
                                                C.c_int, dp, vp, vp, C.c_int, C.c_int, vp]
    lib.pnx_nnls_solve_peaks_f64.restype = C.c_int
    lib.pnx_nnls_solve_peaks_f64.argtypes = [vp, C.c_int64, vp, C.c_int, dp, C.c_double, C.c_int, C.c_double, C.c_int, vp, vp, vp,
                                             C.c_int, dp, vp, vp, vp, vp, vp, C.c_int, vp]
    lib.pnx_nnls_solve_peaks_stats_f64.restype = C.c_int
    lib.pnx_nnls_solve_peaks_stats_f64.argtypes = [*lib.pnx_nnls_solve_peaks_f64.argtypes, vp]
    lib.pnx_nnls_fit_stats_f64.restype = C.c_int
    lib.pnx_nnls_fit_stats_f64.argtypes = [vp, C.c_int64, vp, vp, vp, vp, C.c_int, C.c_int, vp]
    lib.pnx_curvefit_predict_f64.restype = C.c_int
    lib.pnx_curvefit_predict_f64.argtypes = [C.POINTER(CurvefitOpts), C.c_int64, C.c_int, dp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp]
    lib.pnx_scatter_maps_f32.restype = C.c_int
    lib.pnx_scatter_maps_f32.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_int64, vp, C.c_int, C.c_int, vp]
    lib.pnx_mask_select_f64.restype = C.c_int
    lib.pnx_mask_select_f64.argtypes = [vp, C.c_int64, C.c_double, vp, C.POINTER(C.c_int64), C.c_int, vp]
    lib.pnx_gather_rows_f64.restype = C.c_int
    lib.pnx_gather_rows_f64.argtypes = [vp, C.c_int64, vp, C.c_int64, vp, C.c_int, vp]
    lib.pnx_scatter_rows_t_f64.restype = C.c_int
    lib.pnx_scatter_rows_t_f64.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_int64, vp, C.c_int, vp]
    lib.pnx_row_ss_tot_f64.restype = C.c_int
    lib.pnx_row_ss_tot_f64.argtypes = [vp, C.c_int64, C.c_int, vp, C.c_int, vp]
    lib.pnx_label_sums_f64.restype = C.c_int
    lib.pnx_label_sums_f64.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp]
    for f in (lib.pnx_upload, lib.pnx_download):
        f.restype = C.c_int
        f.argtypes = [vp, vp, C.c_int64, C.c_int, vp, C.c_int]
    lib.pnx_sweep_f32.restype = C.c_int
    lib.pnx_sweep_f32.argtypes = [C.c_int, C.c_int64, C.c_int, fp, fp, fp, fp, fp, fp, C.c_int, vp]
    lib.pnx_sweep_f64.restype = C.c_int
    lib.pnx_sweep_f64.argtypes = [C.c_int, C.c_int64, C.c_int, dp, dp, dp, dp, dp, dp, C.c_int, vp]
    _lib = lib
    return lib


def last_error() -> str:
    buf = C.create_string_buffer(512)
    load().pnx_last_error(buf, 512)
    return buf.value.decode("utf-8", "replace")


def check(rc: int):
    if rc != 0:
        raise PnxError(rc, last_error())


def ptr(a):
    """Address of a C-contiguous numpy array / a torch tensor / None."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data
    return a.data_ptr()  # torch tensor


def device_count() -> int:
    return int(load().pnx_device_count())


def require_device():
    if device_count() < 1:
        raise PnxError(-3, "no HIP device visible: pyneapple_amd needs an MI355X (there is no CPU fallback)")

// pnx_grid_tmrf_args.hpp -- the host half of the edge-preserving (Student-t) neighbourhood prior of the grid posterior that needs
// no device (pnx_curvefit_grid_neighbour_wfield_f64, pnx_curvefit_grid_posterior_wfield_f64, pnx_curvefit_grid_posterior_tmrf_f64;
// DESIGN.md 4.1s): the checks of dof and sd in front of the Gaussian calls' own checks (pnx_grid_mrf_args.hpp), and K, the number
// of rows that carry a precision.  Free of HIP types: pnx_api.hip uses it, tests/host_stub/grid_tmrf_args_stub.cpp builds the same
// code for the CPU under AddressSanitizer / UBSan.
#pragma once
#include "pnx_grid_mrf_args.hpp"

namespace pnx {

// dof: the degrees of freedom nu of the Student-t pair potential, finite and > 0 (the Gaussian prior is its limit, not a value).
inline int grid_tmrf_check_dof(const char *who, double dof) {
    if (!(dof > 0.0) || std::isinf(dof)) return set_error(PNX_ERR_INVALID, "%s: dof=%g must be finite and > 0", who, dof);
    return PNX_OK;
}

// K: the rows with a positive precision -- the dimension of the edge difference the Student-t sees.
inline int grid_tmrf_rows(int n_free, const double *precision) {
    int K = 0;
    for (int k = 0; k < n_free; ++k) K += precision[k] > 0.0;
    return K;
}

// The weighted gather: the Gaussian gather's checks (field_w in field_n's place among the required outputs), then sd and dof.
inline int grid_tmrf_field_check_args(int64_t n_vox, int64_t first, int64_t count, int n_free, int n_nb, const int32_t *neighbours,
                                      const double *mean, const double *sd, const double *centre, const double *precision, double dof,
                                      const double *field_q, const double *field_w, const int32_t *field_n, int mem) {
    const char *who = "grid neighbour wfield";
    if (int rc = grid_tmrf_check_dof(who, dof)) return rc;
    if (int rc = grid_mrf_field_check_args(n_vox, first, count, n_free, n_nb, neighbours, mean, centre, precision, field_q, field_n, mem)) return rc;
    if (n_vox && (!sd || !field_w)) return set_error(PNX_ERR_INVALID, "%s: NULL data pointer (sd and field_w are required)", who);
    return PNX_OK;
}

// One weighted colour update: the Gaussian one's checks with field_w in field_n's place.
inline int grid_tmrf_posterior_field_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                                const double *atoms, const double *fixed, const double *lo, const double *hi,
                                                int project_amplitude, const double *log_prior, double noise_sd, int64_t first, int64_t count,
                                                const double *field_q, const double *field_w, const double *precision, const double *mean,
                                                int mem, GridPosteriorHost *H, GridMrfHost *M) {
    static const int32_t present = 0;  // stands for field_n in the Gaussian check, which only asks whether it is there
    if (int rc = grid_mrf_posterior_field_check_args(o, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project_amplitude, log_prior, noise_sd, first,
                                                     count, field_q, &present, precision, mean, mem, H, M))
        return rc;
    if (n_vox && !field_w) return set_error(PNX_ERR_INVALID, "grid posterior wfield: field_w is NULL");
    return PNX_OK;
}

// The driver: dof and sd, then everything the Gaussian driver refuses.
inline int grid_tmrf_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms, const double *atoms,
                                const double *fixed, const double *lo, const double *hi, int project_amplitude, const double *log_prior,
                                double noise_sd, int n_nb, const int32_t *neighbours, int n_colours, const int64_t *colour_start,
                                const double *precision, double dof, int n_sweeps, double tol, const double *mean, const double *sd, int mem,
                                GridPosteriorHost *H, GridMrfHost *M) {
    const char *who = "grid posterior tmrf";
    if (int rc = grid_tmrf_check_dof(who, dof)) return rc;
    if (!sd) return set_error(PNX_ERR_INVALID, "%s: sd is NULL (the edge weights need the posterior variances)", who);
    return grid_mrf_check_args(o, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project_amplitude, log_prior, noise_sd, n_nb, neighbours, n_colours,
                               colour_start, precision, n_sweeps, tol, mean, mem, H, M);
}
}  // namespace pnx

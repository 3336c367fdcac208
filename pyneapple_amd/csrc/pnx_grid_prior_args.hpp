// pnx_grid_prior_args.hpp -- the host half of pnx_curvefit_grid_prior_em_f64 that needs no device: the checks of its arguments
// in front of any device work (the posterior's, shared, then the four of the EM), the normalised start prior, the stopping rule,
// what a call without a finite voxel reports, and the sizing of the EM kernels' LDS slab.  Free of HIP types, like
// pnx_grid_posterior_args.hpp: pnx_api.hip and pnx_grid_prior.hip use it, tests/host_stub/grid_prior_args_stub.cpp builds the same
// code for the CPU under AddressSanitizer / UBSan.
#pragma once
#include <cmath>
#include <cstdint>

#include "pnx_grid_posterior_args.hpp"

namespace pnx {

constexpr int kGridPriorMaxIter = 1000;

// The four arguments of an EM over a dictionary, each refusal naming its argument; `who` opens the message ("grid prior",
// "varpro prior": pnx_varpro_prior_args.hpp applies the same rules).
inline int prior_em_check_args(const char *who, int n_iter, double pseudo_count, double rel_tol, const double *log_prior_out) {
    if (!log_prior_out) return set_error(PNX_ERR_INVALID, "%s: log_prior_out is NULL (the one output that is not optional)", who);
    if (n_iter < 1 || n_iter > kGridPriorMaxIter)
        return set_error(PNX_ERR_INVALID, "%s: n_iter=%d out of range [1,%d]", who, n_iter, kGridPriorMaxIter);
    if (!(pseudo_count >= 0.0) || std::isinf(pseudo_count))
        return set_error(PNX_ERR_INVALID, "%s: pseudo_count=%g must be finite and >= 0", who, pseudo_count);
    if (!(rel_tol >= 0.0) || std::isinf(rel_tol)) return set_error(PNX_ERR_INVALID, "%s: rel_tol=%g must be finite and >= 0", who, rel_tol);
    return PNX_OK;
}

// The four arguments of the EM first (prior_em_check_args), then grid_posterior_check_args with log_prior_out in
// the place of `mean`: the posterior's refusals, weighting and prior rules hold unchanged.  H->log_prior_norm normalises the start.
inline int grid_prior_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                 const double *atoms, const double *fixed, const double *lo, const double *hi, int project_amplitude,
                                 const double *log_prior, double noise_sd, int n_iter, double pseudo_count, double rel_tol,
                                 const double *log_prior_out, int mem, GridPosteriorHost *H) {
    if (int rc = prior_em_check_args("grid prior", n_iter, pseudo_count, rel_tol, log_prior_out)) return rc;
    return grid_posterior_check_args(o, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project_amplitude, log_prior, noise_sd, log_prior_out, mem, H);
}

// start[g] = log_prior[g] - norm (norm = log sum_g exp(log_prior_g) from the check; NULL: the uniform prior, -log(n_atoms)):
// the prior every iteration starts from sums to 1 over its finite entries.  Returns the number of admissible (finite) atoms.
inline int grid_prior_start(int n_atoms, const double *log_prior, double norm, double *start) {
    int adm = 0;
    for (int g = 0; g < n_atoms; ++g) {
        start[g] = (log_prior ? log_prior[g] : 0.0) - norm;  // -inf stays -inf
        adm += start[g] > -HUGE_VAL;
    }
    return adm;
}

// After update t >= 1 (loglik[t] under the prior that update t - 1 produced): stop when the gain of the last update is at most
// rel_tol |loglik[t]|.  rel_tol = 0 never stops: all n_iter updates run.
inline bool grid_prior_converged(const double *loglik, int t, double rel_tol) {
    return t >= 1 && rel_tol > 0.0 && loglik[t] - loglik[t - 1] <= rel_tol * std::fabs(loglik[t]);
}

// The optional outputs of a call that ended after `done` updates: entries of the trace past `done` are NaN.
inline void grid_prior_report(int n_iter, int done, int64_t finite_voxels, double *loglik, int *n_iter_done, int64_t *n_eff) {
    if (loglik)
        for (int t = done + 1; t <= n_iter; ++t) loglik[t] = NAN;
    if (n_iter_done) *n_iter_done = done;
    if (n_eff) *n_eff = finite_voxels;
}

// The LDS image of a slab in both passes of the EM: [kpad][stride] doubles of the dictionary, then per atom ||s||^2, its inverse
// and log_prior, then the four wave-private rows of the accumulate pass -- the posterior's slab at four parameter rows, whatever
// n_free is (grid_posterior_slab: width a multiple of 16, stride = 16 mod 32, inside 64 KB).
inline GridSlab grid_prior_slab(int n_b) { return grid_posterior_slab(n_b, 4); }
}  // namespace pnx

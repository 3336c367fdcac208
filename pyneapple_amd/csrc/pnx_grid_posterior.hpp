// pnx_grid_posterior.hpp -- internal interface of the grid posterior behind pnx_curvefit_grid_posterior_f64 (see
// pnx_grid_posterior.hip).  The dictionary is grid start's (pnx_grid.hpp: grid_dict_build); this adds what the fold reads per atom.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnx_grid.hpp"
#include "pnx_grid_posterior_args.hpp"

namespace pnx {
// Per-atom inputs of the fold on the device, carved from one buffer of grid_posterior_bytes() bytes.
struct GridPosterior {
    const double *theta = nullptr;    // (n_free, gp) atoms minus the row's centre, 0 for padded atoms
    const double *lp = nullptr;       // (gp) log_prior, 0 for the uniform prior, -inf for padded atoms
    const double *max_nrm = nullptr;  // (1) max_g ||s_g||^2
    double centre[PNX_MAX_PARAMS] = {};
    double log_prior_norm = 0.0, noise_sd = 0.0;
};
size_t grid_posterior_bytes(int n_free, int n_atoms);
// Enqueues the upload of log_prior (host, may be null) and the preparation of theta / lp / max_nrm behind grid_dict_build on `stream`.
int grid_posterior_prepare(const GridDict &D, const GridPosteriorHost &H, const double *log_prior_host, double noise_sd, void *buffer_d,
                           GridPosterior *P, hipStream_t stream);
// The outputs of n_vox voxels, device pointers, enqueued on `stream`; every output but mean may be null.
int grid_posterior_device(const GridDict &D, const GridPosterior &P, int64_t n_vox, const double *y_d, double *mean_d, double *sd_d,
                          int32_t *map_atom_d, double *map_p_d, double *log_evidence_d, double *ess_d, int cus, hipStream_t stream);
}  // namespace pnx

// pnx_grid_rician.hpp -- internal interface of the grid posterior under a Rician likelihood behind
// pnx_curvefit_grid_posterior_rician_f64, and of pnx_log_i0e_f64 (see pnx_grid_rician.hip).  The dictionary and the per-atom inputs
// are the Gaussian posterior's (pnx_grid.hpp: grid_dict_build, pnx_grid_posterior.hpp: grid_posterior_prepare).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnx_grid_posterior.hpp"
#include "pnx_grid_rician_args.hpp"

namespace pnx {
// The outputs of n_vox voxels, device pointers, enqueued on `stream`; every output but mean may be null.  P.noise_sd > 0.
int grid_rician_posterior_device(const GridDict &D, const GridPosterior &P, int64_t n_vox, const double *y_d, double *mean_d, double *sd_d,
                                 int32_t *map_atom_d, double *map_p_d, double *log_evidence_d, double *ess_d, int cus, hipStream_t stream);
// out[i] = log_i0e(z[i]) (pnx_bessel.hpp), NaN for a negative or NaN input; device pointers, one lane per element.
int log_i0e_device(int64_t n, const double *z_d, double *out_d, hipStream_t stream);
}  // namespace pnx

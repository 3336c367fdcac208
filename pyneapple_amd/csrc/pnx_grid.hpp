// pnx_grid.hpp -- internal interface of the dictionary search behind pnx_curvefit_grid_start_f64 (see pnx_grid.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pnx.h"

namespace pnx {
// The dictionary of one call on the device, carved from one buffer of grid_dict_bytes() bytes.
struct GridDict {
    const double *atoms = nullptr;  // (n_free, n_atoms) as the caller passed them
    const double *st = nullptr;     // (kpad, gp): s_g weighted, k-major; rows >= n_b and atoms >= n_atoms zero
    const double *nrm = nullptr;    // (gp) ||s_g||^2
    const double *inv = nullptr;    // (gp) 1 / ||s_g||^2, 0 for an all-zero row
    const double *w = nullptr;      // (kpad) 1 / sigma_i, 1 without sigma
    int n_b = 0, n_free = 0, n_atoms = 0, gp = 0;  // gp: n_atoms padded to a multiple of 16
    int s0_row = -1;                               // row of S0 among the free parameters when the amplitude is projected
    double lo_s0 = 0.0, hi_s0 = 0.0;
};
size_t grid_dict_bytes(int n_free, int n_atoms, int n_b);
// Enqueues the upload of the atoms, the forward model of every atom (model_predict_device: the fit's own arithmetic) and the
// weighting / transposition / norms on `stream`.  o: validated, shared fixed values; s0_row >= 0: the dictionary is built with S0 = 1.
int grid_dict_build(const pnx_curvefit_opts *o, const double *b, int n_atoms, const double *atoms_host, const double *fixed_host,
                    const double *lo, const double *hi, int s0_row, void *buffer_d, GridDict *D, hipStream_t stream);
// best / cost / p0_out of n_vox voxels against the dictionary, device pointers, enqueued on `stream`; best and cost may be null.
int grid_match_device(const GridDict &D, int64_t n_vox, const double *y_d, double *p0_out_d, int32_t *best_d, double *cost_d, int cus,
                      hipStream_t stream);
}  // namespace pnx

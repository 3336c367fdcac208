// pnx_grid_refine.hpp -- internal interface of the per-voxel fine grid behind pnx_curvefit_grid_refine_f64 (see
// pnx_grid_refine.hip).  No dictionary: every voxel's atoms are built inside the kernel from its own centre and half-width.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnx_grid_refine_args.hpp"

namespace pnx {
// The outputs of n_vox voxels, device pointers, enqueued on `stream`; every output but mean may be null.  o, H: checked by
// grid_refine_check_args; b, fixed, lo, hi, n_points are host arrays and travel as kernel arguments.
int grid_refine_device(const pnx_curvefit_opts *o, const GridRefineHost &H, int64_t n_vox, const double *b, const double *y_d,
                       const double *fixed, const double *lo, const double *hi, double noise_sd, const int32_t *n_points,
                       const double *centre_d, const double *half_width_d, double *mean_d, double *sd_d, double *map_p_d, double *ess_d,
                       double *log_norm_d, double *edge_mass_d, int cus, hipStream_t stream);
}  // namespace pnx

// pnx_predict.hpp -- internal interface of the prediction / goodness-of-fit kernels (see pnx_predict.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pnx.h"

namespace pnx {
struct NnlsPlanData;

// pred (n_vox, n_meas) = coeff (n_vox, n_bins) . basis^T and ss_res (n_vox) = sum_j (y - pred)^2 over the plan's data rows,
// device pointers, enqueued on `stream`.  ss_res or pred may be null (not both); y may be null when ss_res is.
int nnls_fit_stats_device(const NnlsPlanData *P, int64_t n_vox, const double *y_d, const double *coeff_d, double *ss_res_d,
                          double *pred_d, hipStream_t stream);

// pred (n_vox, n_x) = model(x; params) and / or ss_res (n_vox) = sum_i (pred - y)^2, device pointers, enqueued on `stream`.
// params (n_free, n_vox) device; fixed (n_fixed,) HOST or (n_fixed, n_vox) device when o->fixed_per_voxel; x (n_x,) host.
// The caller has validated o (model, index lists, t1_mode) and 1 <= n_x <= PNX_MAX_BVALUES.
int model_predict_device(const pnx_curvefit_opts *o, int64_t n_vox, int n_x, const double *x, const double *params_d,
                         const double *fixed, const double *y_d, double *pred_d, double *ss_res_d, hipStream_t stream);
}  // namespace pnx

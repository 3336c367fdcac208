// pnx_loglin.hpp -- internal interface of the log-linear mono-exponential fit behind pnx_loglinear_f64 / _f32 (see pnx_loglin.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnx_loglin_args.hpp"

namespace pnx {
// The fit of n_vox voxels on device pointers, enqueued on `stream`.  T = double or float: the storage type of y, params, pcov and
// ss_res (the arithmetic is fp64 for both).  params (2, n_vox); pcov, status, n_used, ss_res may be null.
template <typename T>
int loglinear_device(const LogLinOpts &o, int64_t n_vox, const T *y_d, T *params_d, T *pcov_d, int8_t *status_d, int32_t *n_used_d,
                     T *ss_res_d, hipStream_t stream);
}  // namespace pnx

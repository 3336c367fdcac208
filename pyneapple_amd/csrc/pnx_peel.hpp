// pnx_peel.hpp -- internal interface of the exponential-peeling fit behind pnx_peel_f64 / _f32 (see pnx_peel.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnx_peel_args.hpp"

namespace pnx {
// The fit of n_vox voxels on device pointers, enqueued on `stream`.  T = double or float: the storage type of y, params and ss_res
// (the arithmetic is fp64 for both).  params (n_params, n_vox); status, n_used (n_stage, n_vox), ss_res may be null.
template <typename T>
int peel_device(const PeelOpts &o, int64_t n_vox, const T *y_d, T *params_d, int8_t *status_d, int32_t *n_used_d, T *ss_res_d,
                hipStream_t stream);
}  // namespace pnx

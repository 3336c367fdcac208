// pnx_simplex.hpp -- internal interface of the streaming kernels around the constrained curve fit (see pnx_simplex.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pnx.h"

namespace pnx {

// Violators of f1 + f2 <= 1 among the n_vox results of a tri-exponential fit (popt (n_free, n_vox), rows 0 and 2 are f1, f2):
// status > 0 and f1 + f2 > 1.  flags (n_vox bytes) and idx (n_vox int64) are scratch of the caller; idx receives the
// violators' indices in ascending order.  Every voxel's lambda is set to 0 and its face to 0 (either may be null).
// *n_viol = their number, *min_nfev = the smallest phase-1 evaluation count among them.  Synchronises `stream` (once per 2^30 voxels).
int simplex_select(const double *popt_d, int64_t n_vox, const int8_t *status_d, const int32_t *nfev_d, unsigned char *flags_d,
                   int64_t *idx_d, double *lambda_d, int8_t *face_d, int64_t *n_viol, int *min_nfev, hipStream_t stream);

// The bi-exponential problem of the m violators, parameter-major (n2, m) with n2 = 3 (model tri_reduced) or 4 (tri_s0):
// y2 (m, n_b) = y[idx, :], start values f1 / (f1 + f2), D1, D2 [, S0] of the phase-1 result (the first clipped into its
// bounds), bounds of the tri-exponential problem with those of f1 intersected with 1 - those of f2.
// lo / hi: (n_free,) HOST when !per_voxel, (n_free, n_vox) device otherwise.  Enqueued only.
int simplex_gather(int model, int n_b, const double *y_d, const double *popt_d, int64_t n_vox, const int64_t *idx_d, int64_t m,
                   int per_voxel, const double *lo, const double *hi, double *y2_d, double *p0_2_d, double *lo2_d, double *hi2_d,
                   hipStream_t stream);

// The face results back into the tri-exponential arrays, with the multiplier of the constraint (pnx_simplex.hip).
// p0: (n_free,) HOST when !per_voxel, (n_free, n_vox) device otherwise (the sentinel of a failed phase 2).  pcov, lambda, face
// may be null.  Enqueued only.
int simplex_merge(int model, int n_b, const double *b_host, int64_t m, const int64_t *idx_d, const double *y2_d,
                  const double *popt2_d, const int8_t *status2_d, const int32_t *nfev2_d, const double *cost2_d, int per_voxel,
                  const double *p0, int64_t n_vox, double *popt_d, double *pcov_d, int8_t *status_d, int32_t *nfev_d, double *cost_d,
                  double *lambda_d, int8_t *face_d, hipStream_t stream);

}  // namespace pnx

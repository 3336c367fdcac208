// pnx_varpro_marginal.hpp -- internal interface of the per-parameter marginals of the posterior over the variable-projection
// dictionary behind pnx_curvefit_varpro_marginals_f64 (see pnx_varpro_marginal.hip).  The dictionary is the variable projection's
// (varpro_dict_build), the per-atom log-weight and the cancellation floor are the posterior's (varpro_posterior_prepare); this adds
// the one pass that forms the weights about a running maximum and sums them per bin, and the quantiles.
//
// Determinism: no atomics.  A voxel's sums depend on the order of the atoms only -- not on the grid size, the number of voxels
// in the call or where its signal lives -- so results are bit-identical between two calls and between PNX_MEM_HOST and
// PNX_MEM_DEVICE.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnx_varpro_marginal_args.hpp"
#include "pnx_varpro_posterior.hpp"

namespace pnx {
// The binning on the device: the table of grid_marginal_table, carved from one buffer of varpro_marginal_bytes() bytes.
struct VarproMarginal {
    const int32_t *table = nullptr;  // (n_rows, gp)
    GridMarginalHost host;
};
size_t varpro_marginal_bytes(int n_free, int n_atoms);
// Builds the table on the host and enqueues its upload on `stream`.
int varpro_marginal_prepare(const VarproDict &D, const GridMarginalHost &M, const int32_t *bin_of_host, void *buffer_d, VarproMarginal *G,
                            hipStream_t stream);
// marginal (B, n_vox); lv_d (n_vox) work: L_v, NaN for a voxel without a weight; quantile (n_q, n_free, n_vox) or null; geo_mean
// (n_free, n_vox) or null; log_evidence (n_vox) or null; device pointers, enqueued on `stream`.  bin_value (B) and probs (n_q) are
// host arrays, passed to the kernel by value.
int varpro_marginal_device(const VarproDict &D, const VarproPosterior &P, const VarproMarginal &G, int64_t n_vox, const double *y_d,
                           const double *bin_value, int n_q, const double *probs, double *marginal_d, double *lv_d, double *quantile_d,
                           double *geo_mean_d, double *log_evidence_d, int cus, hipStream_t stream);
}  // namespace pnx

// pnx_grid_marginal.hpp -- internal interface of the per-parameter marginals of the grid posterior behind
// pnx_curvefit_grid_marginals_f64 (see pnx_grid_marginal.hip).  The dictionary is grid start's, the per-atom log prior and the
// cancellation floor are the posterior's, the normaliser pass (L_v per voxel) is the EM's (pnx_grid_prior.hpp:
// grid_prior_normalise); this adds the pass that re-forms the weights and sums them per bin, and the quantiles.
//
// Determinism: no atomics.  A voxel's sums depend on the order of the atoms only -- not on the grid size, the number of voxels
// in the call or where its signal lives -- so results are bit-identical between two calls and between PNX_MEM_HOST and
// PNX_MEM_DEVICE.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnx_grid_marginal_args.hpp"
#include "pnx_grid_prior.hpp"

namespace pnx {
// The binning on the device: the table of grid_marginal_table, carved from one buffer of grid_marginal_bytes() bytes.
struct GridMarginal {
    const int32_t *table = nullptr;  // (n_rows, gp)
    GridMarginalHost host;
};
size_t grid_marginal_bytes(int n_free, int n_atoms);
// Builds the table on the host and enqueues its upload on `stream`.
int grid_marginal_prepare(const GridDict &D, const GridMarginalHost &M, const int32_t *bin_of_host, void *buffer_d, GridMarginal *G,
                          hipStream_t stream);
// Behind grid_prior_normalise on the same stream (W.lv holds L_v): marginal (B, n_vox); quantile (n_q, n_free, n_vox) or null;
// log_evidence (n_vox) or null; device pointers, enqueued on `stream`.  bin_value (B) and probs (n_q) are host arrays, passed to the
// kernel by value.
int grid_marginal_device(const GridDict &D, const GridPosterior &P, const GridMarginal &G, int64_t n_vox, const double *y_d,
                         const GridPriorWork &W, const double *bin_value, int n_q, const double *probs, double *marginal_d, double *quantile_d,
                         double *log_evidence_d, hipStream_t stream);
}  // namespace pnx

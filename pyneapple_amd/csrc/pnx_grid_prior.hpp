// pnx_grid_prior.hpp -- internal interface of the empirical-Bayes prior over the grid behind pnx_curvefit_grid_prior_em_f64 (see
// pnx_grid_prior.hip).  The dictionary is grid start's (pnx_grid.hpp: grid_dict_build), the per-atom log prior and the
// cancellation floor are the posterior's (pnx_grid_posterior.hpp: grid_posterior_prepare); this adds the two passes of an EM
// iteration and what they leave on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnx_grid_posterior.hpp"
#include "pnx_grid_prior_args.hpp"

namespace pnx {
// What the normaliser pass reports of the whole volume under the current prior.
struct GridPriorStats {
    double loglik;       // sum of L_v over the voxels with a finite L_v
    long long n_finite;  // their number
};
// Device scratch of one call, carved from one buffer of grid_prior_bytes() bytes.
struct GridPriorWork {
    double *lv = nullptr;        // (n_vox) L_v = log sum_g exp(l_g) under the current prior, NaN for a non-finite voxel
    double *partial = nullptr;   // (blocks, gp) per block sum_v W_vg of its voxels
    double *block_l = nullptr;   // (blocks) per block sum of its finite L_v
    long long *block_n = nullptr;  // (blocks) and their number
    GridPriorStats *stats = nullptr;
    int blocks = 0;              // min(groups of 64 voxels, 2 x CUs): the grid of both passes; fixes the order of every sum
};
size_t grid_prior_bytes(int64_t n_vox, int n_atoms, int cus);
void grid_prior_carve(int64_t n_vox, int n_atoms, int cus, void *buffer_d, GridPriorWork *W);
// Normaliser pass: W.lv and W.stats under the prior in P.lp, enqueued on `stream`.
int grid_prior_normalise(const GridDict &D, const GridPosterior &P, int64_t n_vox, const double *y_d, const GridPriorWork &W, hipStream_t stream);
// Accumulate pass and finish behind a normaliser pass under the same prior: P.lp <- log((S_g + pseudo_count) / (n_finite +
// pseudo_count n_admissible)) in place (the buffer grid_posterior_prepare carved is this call's own), -inf where it was -inf.
int grid_prior_update(const GridDict &D, const GridPosterior &P, int64_t n_vox, const double *y_d, const GridPriorWork &W, double pseudo_count,
                      int n_admissible, hipStream_t stream);
}  // namespace pnx

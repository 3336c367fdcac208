// pnx_grid_tmrf.hpp -- internal interface of the edge-preserving (Student-t) neighbourhood prior behind
// pnx_curvefit_grid_neighbour_wfield_f64, pnx_curvefit_grid_posterior_wfield_f64 and pnx_curvefit_grid_posterior_tmrf_f64 (see
// pnx_grid_tmrf.hip).  Everything per call is the Gaussian prior's (pnx_grid_mrf.hpp: GridMrf, r_g, the colour
// check, delta); this adds the gather with one weight per edge and the field posterior that takes a real weight sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnx_grid_mrf.hpp"
#include "pnx_grid_tmrf_args.hpp"

namespace pnx {
// field_q (n_free, n_vox), field_w (n_vox), field_n (n_vox) and, where `edge` is not null, edge (n_vox, n_nb) of the voxels
// [first, first + count) from mean and sd (n_free, n_vox): device pointers, enqueued on `stream`.  flag as GridMrfFieldArgs'.
struct GridTmrfFieldArgs {
    const int32_t *nb;
    const double *mean, *sd;
    double *q, *w, *edge;
    int32_t *n;
    int32_t *flag;
    long long n_vox, first, count;
    int n_free, n_nb;
    double dof, dof_k;  // nu and nu + K
    double centre[PNX_MAX_PARAMS], precision[PNX_MAX_PARAMS];
};
int grid_tmrf_field_device(const GridTmrfFieldArgs &a, hipStream_t stream);
// grid_mrf_posterior_device with field_w_d (n_vox) doubles in field_n_d's place.
int grid_tmrf_posterior_device(const GridDict &D, const GridPosterior &P, const GridMrf &F, int64_t n_vox, int64_t first, int64_t count,
                               const double *y_d, const double *field_q_d, const double *field_w_d, double *mean_d, double *sd_d,
                               int32_t *map_atom_d, double *map_p_d, double *log_evidence_d, double *ess_d, double *delta_d, bool accumulate,
                               int cus, hipStream_t stream);
}  // namespace pnx

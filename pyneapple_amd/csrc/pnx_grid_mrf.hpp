// pnx_grid_mrf.hpp -- internal interface of the neighbourhood (MRF) prior behind pnx_curvefit_grid_neighbour_field_f64,
// pnx_curvefit_grid_posterior_field_f64 and pnx_curvefit_grid_posterior_mrf_f64 (see pnx_grid_mrf.hip).  The
// dictionary is grid start's, theta / log_prior / the cancellation floor are the posterior's (grid_posterior_prepare); this adds
// the per-atom row r_g on the device, the gather of the neighbours' means, the posterior fold with the field inside l_g over a
// voxel range, the reduction of delta and the check of a colouring.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnx_grid_mrf_args.hpp"
#include "pnx_grid_posterior.hpp"

namespace pnx {
// What the field kernels read beside GridPosterior, carved from one buffer of grid_mrf_bytes() bytes.
struct GridMrf {
    double *r = nullptr;        // (gp) r_g, 0 for padded atoms
    double *block = nullptr;    // (blocks) per block the maximum of delta over its voxels
    int32_t *flags = nullptr;   // (2) lowest voxel with a neighbour index outside [-1, n_vox) / with a neighbour of its own colour
    int blocks = 0;             // 2 x CUs: the most blocks a field posterior launches
    bool any = false;           // a precision is positive: otherwise the field is exactly zero whatever field_q / field_n hold
    double scale[PNX_MAX_PARAMS] = {};  // grid_mrf_delta_scale
};
size_t grid_mrf_bytes(int n_atoms, int cus);
// Enqueues the upload of r_g (computed on the host from the atoms, H.centre and precision) and the reset of the flags on `stream`.
int grid_mrf_prepare(const GridDict &D, const GridPosteriorHost &H, const GridMrfHost &M, const double *atoms_host, const double *precision,
                     int cus, void *buffer_d, GridMrf *F, hipStream_t stream);
// field_q (n_free, n_vox) and field_n (n_vox) of the voxels [first, first + count) from mean (n_free, n_vox): device pointers,
// enqueued on `stream`.  flag (device int32, may be null) receives by atomicMin the lowest voxel of the range with an index
// outside [-1, n_vox); such an index is never dereferenced.
struct GridMrfFieldArgs {
    const int32_t *nb;
    const double *mean;
    double *q;
    int32_t *n;
    int32_t *flag;
    long long n_vox, first, count;
    int n_free, n_nb;
    double centre[PNX_MAX_PARAMS], precision[PNX_MAX_PARAMS];
};
int grid_mrf_field_device(const GridMrfFieldArgs &a, hipStream_t stream);
// flags[0] / flags[1] (atomicMin) over all voxels: an index outside [-1, n_vox) / a neighbour inside the voxel's own colour range.
int grid_mrf_colour_check_device(int64_t n_vox, int n_nb, const int32_t *nb_d, int n_colours, const int64_t *colour_start, int32_t *flags_d,
                                 hipStream_t stream);
// grid_posterior_device on the voxels [first, first + count) with the field inside l_g, written in place into the full-length
// outputs.  delta_d (device scalar, may be null): max over the range of |mean_new - mean_old| / F.scale, merged with the value it
// holds when `accumulate`.
int grid_mrf_posterior_device(const GridDict &D, const GridPosterior &P, const GridMrf &F, int64_t n_vox, int64_t first, int64_t count,
                              const double *y_d, const double *field_q_d, const int32_t *field_n_d, double *mean_d, double *sd_d,
                              int32_t *map_atom_d, double *map_p_d, double *log_evidence_d, double *ess_d, double *delta_d, bool accumulate,
                              int cus, hipStream_t stream);
// *delta_d = max over block_d[0 .. blocks) (merged with the value it holds when `accumulate`): the tail of a field posterior, shared
// with the weighted one (pnx_grid_tmrf.hip).
int grid_mrf_delta_device(const double *block_d, int blocks, double *delta_d, bool accumulate, hipStream_t stream);
}  // namespace pnx

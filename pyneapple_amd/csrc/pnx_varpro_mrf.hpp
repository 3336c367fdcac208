// pnx_varpro_mrf.hpp -- internal interface of the neighbourhood (MRF) prior of the posterior over the variable projection's
// dictionary behind pnx_curvefit_varpro_posterior_field_f64 and pnx_curvefit_varpro_posterior_mrf_f64 (see pnx_varpro_mrf.hip,
// DESIGN.md 4.1q).  The dictionary is the variable projection's, theta / lw / the cancellation floor are the posterior's
// (varpro_posterior_prepare); the gather, the colour check and the reduction of delta over the blocks are the grid prior's
// (pnx_grid_mrf.hpp: they know nothing of the dictionary).  This adds the per-atom row r_g on the device and the posterior fold
// with the field inside l_g over a voxel range.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnx_grid_mrf.hpp"
#include "pnx_varpro_mrf_args.hpp"
#include "pnx_varpro_posterior.hpp"

namespace pnx {
// What the field kernel reads beside VarproPosterior, carved from one buffer of varpro_mrf_bytes() bytes.
struct VarproMrf {
    double *r = nullptr;        // (gp) r_g, 0 for padded atoms
    double *block = nullptr;    // (blocks) per block the maximum of delta over its voxels
    int32_t *flags = nullptr;   // (2) what grid_mrf_colour_check_device reports into
    int blocks = 0;             // 2 x CUs: the most blocks a field posterior launches
    bool any = false;           // a precision is positive: otherwise the field is exactly zero whatever field_q / field_n hold
    double scale[PNX_MAX_PARAMS] = {};  // grid_mrf_delta_scale
};
size_t varpro_mrf_bytes(int n_atoms, int cus);
// Enqueues the upload of r_g (computed on the host from nl_atoms, H.centre and precision) and the reset of the flags on `stream`.
int varpro_mrf_prepare(const VarproDict &D, const VarproPosteriorHost &H, const VarproMrfHost &M, const double *nl_atoms_host,
                       const double *precision, int cus, void *buffer_d, VarproMrf *F, hipStream_t stream);
// varpro_posterior_device on the voxels [first, first + count) with the field inside l_g, written in place into the full-length
// outputs.  delta_d (device scalar, may be null): max over the range of |mean_new - mean_old| / F.scale, merged with the value it
// holds when `accumulate`.
int varpro_mrf_posterior_device(const VarproDict &D, const VarproPosterior &P, const VarproMrf &F, int64_t n_vox, int64_t first, int64_t count,
                                const double *y_d, const double *field_q_d, const int32_t *field_n_d, double *mean_d, double *sd_d,
                                int32_t *map_atom_d, double *map_p_d, double *log_evidence_d, double *ess_d, double *clipped_mass_d,
                                double *delta_d, bool accumulate, int cus, hipStream_t stream);
}  // namespace pnx

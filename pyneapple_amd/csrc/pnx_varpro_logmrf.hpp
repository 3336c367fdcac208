// pnx_varpro_logmrf.hpp -- internal interface of the neighbourhood (MRF) prior of the variable-projection posterior with a
// per-row linear or log coupling behind pnx_curvefit_varpro_posterior_logfield_f64 and pnx_curvefit_varpro_posterior_logmrf_f64
// (see pnx_varpro_logmrf.hip).  The dictionary is the variable projection's, theta / lw / the cancellation floor
// are the posterior's (varpro_posterior_prepare); the gather, the colour check and the reduction of delta over the blocks are the
// grid prior's (pnx_grid_mrf.hpp).  This adds the centred field rows fc and the per-atom row r_g on the device and the posterior
// fold that reports the moments over theta and the mean of f from the same weights.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnx_grid_mrf.hpp"
#include "pnx_varpro_logmrf_args.hpp"
#include "pnx_varpro_posterior.hpp"

namespace pnx {
// What the log-field kernel reads beside VarproPosterior, carved from one buffer of varpro_logmrf_bytes() bytes.
struct VarproLogMrf {
    double *r = nullptr;        // (gp) r_g, 0 for padded atoms
    double *fc = nullptr;       // (n_nl, gp) f - fcentre, 0 for padded atoms
    double *block = nullptr;    // (blocks) per block the maximum of delta over its voxels
    int32_t *flags = nullptr;   // (2) what grid_mrf_colour_check_device reports into
    int blocks = 0;             // 2 x CUs: the most blocks a field posterior launches
    bool any = false;           // a precision is positive: otherwise the field is exactly zero whatever field_q / field_n hold
    double scale[PNX_MAX_PARAMS] = {};    // varpro_logmrf_delta_scale
    double fcentre[PNX_MAX_PARAMS] = {};  // per free row
};
size_t varpro_logmrf_bytes(int n_nl, int n_atoms, int cus);
// Enqueues the upload of fc and r_g (computed on the host from nl_atoms, G.fcentre, precision and coupling) and the reset of the
// flags on `stream`.
int varpro_logmrf_prepare(const VarproDict &D, const VarproLogMrfHost &G, const double *nl_atoms_host, const double *precision,
                          const int32_t *coupling, int cus, void *buffer_d, VarproLogMrf *F, hipStream_t stream);
// varpro_posterior_device on the voxels [first, first + count) with the field inside l_g, written in place into the full-length
// outputs; field_mean_d (n_free, n_vox) receives the mean of f of a non-linear row and the value of mean on a fraction / S0 row.
// use_field false: the field is exactly zero whatever field_q_d / field_n_d hold (they may be null).  delta_d (device scalar, may
// be null): max over the range of |field_mean_new - field_mean_old| / F.scale, merged with the value it holds when `accumulate`.
int varpro_logmrf_posterior_device(const VarproDict &D, const VarproPosterior &P, const VarproLogMrf &F, bool use_field, int64_t n_vox,
                                   int64_t first, int64_t count, const double *y_d, const double *field_q_d, const int32_t *field_n_d,
                                   double *mean_d, double *sd_d, int32_t *map_atom_d, double *map_p_d, double *log_evidence_d, double *ess_d,
                                   double *clipped_mass_d, double *field_mean_d, double *delta_d, bool accumulate, int cus, hipStream_t stream);
}  // namespace pnx

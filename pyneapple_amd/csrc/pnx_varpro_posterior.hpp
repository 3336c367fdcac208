// pnx_varpro_posterior.hpp -- internal interface of the posterior over the variable-projection dictionary behind
// pnx_curvefit_varpro_posterior_f64 (see pnx_varpro_posterior.hip).  The dictionary is the variable projection's (pnx_varpro.hpp:
// varpro_dict_build); this adds what the fold reads per atom.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnx_varpro.hpp"
#include "pnx_varpro_posterior_args.hpp"

namespace pnx {
// Per-atom inputs of the fold on the device, carved from one buffer of varpro_posterior_bytes() bytes.
struct VarproPosterior {
    const double *theta = nullptr;    // (n_nl, gp) nl_atoms minus the row's centre, 0 for padded atoms
    const double *lw = nullptr;       // (gp) log_prior (+ the Occam term -0.5 log det N), -inf for padded and excluded atoms
    const double *max_nrm = nullptr;  // (1) max_{g,j} ||phi_j||^2
    double centre[PNX_MAX_PARAMS] = {};
    double log_prior_norm = 0.0, noise_sd = 0.0, amp_l1 = 0.0;
    int marginal_amplitudes = 0;
};
size_t varpro_posterior_bytes(int n_nl, int n_atoms);
// Enqueues the upload of log_prior (host, may be null) and the preparation of theta / lw / max_nrm behind varpro_dict_build on `stream`.
int varpro_posterior_prepare(const VarproDict &D, const VarproPosteriorHost &H, const double *log_prior_host, double noise_sd,
                             int marginal_amplitudes, void *buffer_d, VarproPosterior *P, hipStream_t stream);
// The outputs of n_vox voxels, device pointers, enqueued on `stream`; every output but mean may be null.
int varpro_posterior_device(const VarproDict &D, const VarproPosterior &P, int64_t n_vox, const double *y_d, double *mean_d, double *sd_d,
                            int32_t *map_atom_d, double *map_p_d, double *log_evidence_d, double *ess_d, double *clipped_mass_d, int cus,
                            hipStream_t stream);
}  // namespace pnx

// pnx_varpro_prior.hpp -- internal interface of the empirical-Bayes prior over the variable-projection dictionary behind
// pnx_curvefit_varpro_prior_em_f64 (see pnx_varpro_prior.hip).  The dictionary is the variable projection's (pnx_varpro.hpp:
// varpro_dict_build), the Occam term and the cancellation floor are the posterior's (pnx_varpro_posterior.hpp:
// varpro_posterior_prepare, called WITHOUT a prior, so that its lw is the Occam term alone); this adds the table being learned,
// the two passes of an EM iteration and what they leave on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnx_varpro_posterior.hpp"
#include "pnx_varpro_prior_args.hpp"

namespace pnx {
// What the normaliser pass reports of the whole volume under the current prior: the 16 bytes the host reads per update.
struct VarproPriorStats {
    double loglik;       // sum of L_v over the voxels that take part
    long long n_finite;  // their number
};
// Device scratch of one call, carved from one buffer of varpro_prior_bytes() bytes.
struct VarproPriorWork {
    double *lp = nullptr;        // (gp) log pi_g, the table being learned; -inf for inadmissible and padded atoms
    double *lw = nullptr;        // (gp) lp + occ: what both passes read in the place of the posterior's lw
    double *start = nullptr;     // (n_atoms) staging of the normalised start
    double *lv = nullptr;        // (n_vox) L_v = log sum_g exp(l_g) under the current prior, NaN / -inf for a voxel that takes no part
    double *partial = nullptr;   // (blocks, gp) per block sum_v W_vg of its voxels
    double *block_l = nullptr;   // (blocks) per block sum of its finite L_v
    long long *block_n = nullptr;  // (blocks) and their number
    VarproPriorStats *stats = nullptr;
    int *n_adm = nullptr;        // (1) admissible atoms: a finite start and a finite Occam term
    int blocks = 0;              // min(groups of 64 voxels, 2 x CUs): the grid of both passes; fixes the order of every sum
};
size_t varpro_prior_bytes(int64_t n_vox, int n_atoms, int cus);
void varpro_prior_carve(int64_t n_vox, int n_atoms, int cus, void *buffer_d, VarproPriorWork *W);
// Enqueues the upload of the normalised start (host, n_atoms) and the first lp / lw / n_adm behind varpro_posterior_prepare on
// `stream`; P.lw is the Occam term (prepared with a null prior).
int varpro_prior_begin(const VarproDict &D, const VarproPosterior &P, const double *start_host, const VarproPriorWork &W, hipStream_t stream);
// Normaliser pass: W.lv and W.stats under the table in W.lp, enqueued on `stream`.
int varpro_prior_normalise(const VarproDict &D, const VarproPosterior &P, int64_t n_vox, const double *y_d, const VarproPriorWork &W,
                           hipStream_t stream);
// Accumulate pass and finish behind a normaliser pass under the same table: W.lp <- log((S_g + pseudo_count) / (n_finite +
// pseudo_count n_adm)) in place, -inf where it was -inf, and W.lw <- W.lp + occ.
int varpro_prior_update(const VarproDict &D, const VarproPosterior &P, int64_t n_vox, const double *y_d, const VarproPriorWork &W,
                        double pseudo_count, hipStream_t stream);
}  // namespace pnx

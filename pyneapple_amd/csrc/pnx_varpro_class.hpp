// pnx_varpro_class.hpp -- internal interface of the per-label prior over the variable-projection dictionary behind
// pnx_curvefit_varpro_posterior_classes_f64 and pnx_curvefit_varpro_prior_em_classes_f64 (see pnx_varpro_class.hip, DESIGN.md
// 4.1o).  The dictionary is the variable projection's, the Occam term, theta and the cancellation floor are the posterior's
// (varpro_posterior_prepare WITHOUT a prior, so that its lw is the Occam term alone); this adds the (n_classes, gp) tables on the
// device, the posterior fold under a voxel's own row and the two passes of an EM iteration with a class axis.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnx_varpro_class_args.hpp"
#include "pnx_varpro_posterior.hpp"

namespace pnx {
// The tables of one call on the device, carved from one buffer of varpro_class_table_bytes() bytes.
struct VarproClassTable {
    double *lp = nullptr;     // (n_classes, gp) log pi_cg; -inf for excluded, inadmissible and padded atoms
    double *lw = nullptr;     // (n_classes, gp) lp + occ: what every pass reads
    double *lp_in = nullptr;  // (n_classes, n_atoms) staging of the host table
    int *n_adm = nullptr;     // (kGridMaxClasses) per row the atoms with a finite entry and a finite Occam term
    int n_classes = 0;
    double norm[kGridMaxClasses] = {};
};
size_t varpro_class_table_bytes(int n_classes, int n_atoms);
// Enqueues the upload of the table (host, may be null: every row uniform) and lp / lw / n_adm behind varpro_posterior_prepare on
// `stream`; P.lw is the Occam term (prepared with a null prior).
int varpro_class_table_prepare(const VarproDict &D, const VarproPosterior &P, const GridClassHost &K, int n_classes,
                               const double *log_prior_host, void *buffer_d, VarproClassTable *T, hipStream_t stream);
// varpro_posterior_device under the row labels_d[v] of T; a label outside [0, n_classes) is a non-finite voxel.
int varpro_class_posterior_device(const VarproDict &D, const VarproPosterior &P, const VarproClassTable &T, int64_t n_vox, const double *y_d,
                                  const int32_t *labels_d, double *mean_d, double *sd_d, int32_t *map_atom_d, double *map_p_d,
                                  double *log_evidence_d, double *ess_d, double *clipped_mass_d, int cus, hipStream_t stream);

// What the normaliser pass reports of the whole volume under the current table.
struct VarproClassStats {
    double loglik;                         // the sum of loglik_class in class order
    double loglik_class[kGridMaxClasses];  // per class the sum of L_v over its voxels with a finite L_v
    long long n_finite[kGridMaxClasses];   // their number
};
// Device scratch of one EM call, carved from one buffer of varpro_class_prior_bytes() bytes.
struct VarproClassWork {
    double *lv = nullptr;          // (n_vox) L_v under the voxel's row, NaN / -inf for a voxel that takes no part
    double *partial = nullptr;     // (blocks, n_classes, gp) per block and class sum_v W_vg of its voxels
    double *block_l = nullptr;     // (blocks, n_classes) per block and class the sum of its finite L_v
    long long *block_n = nullptr;  // (blocks, n_classes) and their number
    VarproClassStats *stats = nullptr;
    int blocks = 0;                // min(groups of 64 voxels, 2 x CUs): the grid of every pass; fixes the order of every sum
};
size_t varpro_class_prior_bytes(int64_t n_vox, int n_atoms, int n_classes, int cus);
void varpro_class_prior_carve(int64_t n_vox, int n_atoms, int n_classes, int cus, void *buffer_d, VarproClassWork *W);
// Normaliser pass: W.lv and W.stats under the table T.lw, enqueued on `stream`.
int varpro_class_prior_normalise(const VarproDict &D, const VarproPosterior &P, const VarproClassTable &T, int64_t n_vox, const double *y_d,
                                 const int32_t *labels_d, const VarproClassWork &W, hipStream_t stream);
// Accumulate pass and finish behind a normaliser pass under the same table: per class c with a voxel that takes part,
// T.lp[c, g] <- log((S_cg + pseudo_count) / (n_finite_c + pseudo_count n_adm[c])) in place, -inf where it was -inf, and
// T.lw <- T.lp + occ.
int varpro_class_prior_update(const VarproDict &D, const VarproPosterior &P, const VarproClassTable &T, int64_t n_vox, const double *y_d,
                              const int32_t *labels_d, const VarproClassWork &W, double pseudo_count, hipStream_t stream);
}  // namespace pnx

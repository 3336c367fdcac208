// pnx_varpro.hpp -- internal interface of the variable-projection dictionary fit behind pnx_curvefit_varpro_f64 (see pnx_varpro.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnx_varpro_args.hpp"

namespace pnx {
// The dictionary of one call on the device, carved from one buffer of varpro_dict_bytes() bytes.
struct VarproDict {
    const double *nl = nullptr;   // (n_nl, n_atoms) as the caller passed them
    const double *st = nullptr;   // (k, kpad, gp): the unit columns weighted, k-major per compartment; padding zero
    const double *cst = nullptr;  // (varpro_const_rows(k), gp): M packed, then what the solve reads; padded atoms zero
    const double *w = nullptr;    // (kpad) 1 / sigma_i, 1 without sigma
    int n_b = 0, n_free = 0, n_atoms = 0, gp = 0;  // gp: n_atoms padded to a multiple of 16
    VarproLayout L;
    double fallback[PNX_MAX_PARAMS] = {};
};
size_t varpro_dict_bytes(int n_free, int n_nl, int k, int n_atoms, int n_b);
// Enqueues the upload of the atoms, the one-hot parameter vectors, the forward model of every column (model_predict_device: the
// fit's own arithmetic), the weighting / transposition and the per-atom constants on `stream`.  o: validated, shared fixed values.
int varpro_dict_build(const pnx_curvefit_opts *o, const VarproLayout &L, const double *b, int n_atoms, const double *nl_atoms_host,
                      const double *fixed_host, const double *fallback, void *buffer_d, VarproDict *D, hipStream_t stream);
// p_out / best / cost / clipped of n_vox voxels against the dictionary, device pointers, enqueued on `stream`; best, cost and
// clipped may be null.
int varpro_match_device(const VarproDict &D, int64_t n_vox, const double *y_d, double *p_out_d, int32_t *best_d, double *cost_d,
                        int8_t *clipped_d, int cus, hipStream_t stream);
}  // namespace pnx

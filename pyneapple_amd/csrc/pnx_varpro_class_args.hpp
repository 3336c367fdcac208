// pnx_varpro_class_args.hpp -- the host half of pnx_curvefit_varpro_posterior_classes_f64 and pnx_curvefit_varpro_prior_em_classes_f64
// (one prior row per segmentation label over the variable-projection dictionary) that needs no device: the checks
// of n_classes, labels and the (n_classes, n_atoms) table in front of any device work (grid_class_check_table, called as it
// stands), behind them the unlabelled calls' own checks; the centres of the moment accumulation; and the sizing of the kernels'
// LDS slab as a function of n_classes.  The per-row starts (grid_class_start), the stopping rule (grid_prior_converged) and the
// report of an EM call (grid_class_report) are the grid's, called as they stand.  Free of HIP types, like its neighbours:
// pnx_api.hip and pnx_varpro_class.hip use it, tests/host_stub/varpro_class_args_stub.cpp builds the same code for the CPU under
// AddressSanitizer / UBSan.
#pragma once
#include <cmath>
#include <cstdint>

#include "pnx_grid_class_args.hpp"
#include "pnx_varpro_prior_args.hpp"

namespace pnx {

// The centres of the non-linear rows: mid-range of the atoms that ANY row admits (grid_class_centres' rule; with one row, or rows
// that exclude the same atoms, these are the unlabelled call's centres).  Linear rows stay 0.
inline void varpro_class_centres(const pnx_curvefit_opts *o, const VarproLayout &L, int n_classes, int n_atoms, const double *nl_atoms,
                                 const double *log_prior, VarproPosteriorHost *H) {
    for (int r = 0; r < o->n_free; ++r) {
        H->centre[r] = 0.0;
        if (L.row_src[r] < 0) continue;
        double mn = HUGE_VAL, mx = -HUGE_VAL;
        for (int g = 0; g < n_atoms; ++g) {
            bool any = !log_prior;
            for (int c = 0; c < n_classes && !any; ++c) any = log_prior[(size_t)c * n_atoms + g] != -HUGE_VAL;
            if (!any) continue;
            const double a = nl_atoms[(size_t)L.row_src[r] * n_atoms + g];
            mn = a < mn ? a : mn;
            mx = a > mx ? a : mx;
        }
        H->centre[r] = mn + 0.5 * (mx - mn);
    }
}

// n_classes first, then varpro_posterior_check_args under the uniform prior (the variable projection's refusals, noise_sd,
// marginal_amplitudes, mean), then the labels and the table, then the centres over the table.
inline int varpro_class_posterior_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                             const double *nl_atoms, const double *fixed, const double *lo, const double *hi, int n_classes,
                                             const int32_t *labels, const double *log_prior, double noise_sd, int marginal_amplitudes,
                                             const double *mean, int mem, VarproLayout *L, VarproPosteriorHost *H, GridClassHost *K) {
    if (n_classes < 1 || n_classes > kGridMaxClasses)
        return set_error(PNX_ERR_INVALID, "varpro posterior: n_classes=%d out of range [1,%d]", n_classes, kGridMaxClasses);
    if (int rc = varpro_posterior_check_args(o, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, nullptr, noise_sd, marginal_amplitudes, mean, mem,
                                             L, H))
        return rc;
    if (int rc = grid_class_check_table("varpro posterior", n_classes, labels, n_vox, n_atoms, log_prior, K)) return rc;
    varpro_class_centres(o, *L, n_classes, n_atoms, nl_atoms, log_prior, H);
    return PNX_OK;
}

// The EM's four arguments first, then the above with log_prior_out in the place of `mean`.
inline int varpro_class_prior_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                         const double *nl_atoms, const double *fixed, const double *lo, const double *hi, int n_classes,
                                         const int32_t *labels, const double *log_prior, double noise_sd, int marginal_amplitudes, int n_iter,
                                         double pseudo_count, double rel_tol, const double *log_prior_out, int mem, VarproLayout *L,
                                         VarproPosteriorHost *H, GridClassHost *K) {
    if (int rc = prior_em_check_args("varpro prior", n_iter, pseudo_count, rel_tol, log_prior_out)) return rc;
    if (n_classes < 1 || n_classes > kGridMaxClasses)
        return set_error(PNX_ERR_INVALID, "varpro prior: n_classes=%d out of range [1,%d]", n_classes, kGridMaxClasses);
    if (int rc = varpro_posterior_check_args(o, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, nullptr, noise_sd, marginal_amplitudes,
                                             log_prior_out, mem, L, H))
        return rc;
    if (int rc = grid_class_check_table("varpro prior", n_classes, labels, n_vox, n_atoms, log_prior, K)) return rc;
    varpro_class_centres(o, *L, n_classes, n_atoms, nl_atoms, log_prior, H);
    return PNX_OK;
}

// The LDS image of a slab with n_classes rows of log-weights: the variable projection's (k blocks of [kpad][stride],
// varpro_const_rows(k) rows of constants), then n_classes rows lw and `extra` more -- the posterior's k + 1 centred non-linear rows
// or the EM's 4 n_classes wave-private accumulator rows (both passes) -- each `width` wide.  varpro_prior_slab's rule otherwise; at
// n_classes = 1 these are varpro_posterior_slab and varpro_prior_slab.  Sixteen atoms fit for every n_b <= 128, k <= 3,
// n_classes <= 16: the worst case, the EM at k = 3, 128 b-values and 16 classes, is 384 16 + 92 16 = 7616 <= 8192 doubles.
inline GridSlab varpro_class_slab(int n_b, int k, int n_classes, int extra) {
    GridSlab s;
    const int rows = varpro_const_rows(k) + n_classes + extra;
    s.kpad = (n_b + 3) & ~3;
    s.width = 16;
    for (int w = 16; w <= 256; w += 16) {
        const int stride = (w & 16) ? w : w + 16;
        if (k * s.kpad * stride + rows * w <= 8192) s.width = w;
    }
    s.stride = (s.width & 16) ? s.width : s.width + 16;
    s.lds_doubles = k * s.kpad * s.stride + rows * s.width;
    return s;
}
inline GridSlab varpro_class_posterior_slab(int n_b, int k, int n_classes) { return varpro_class_slab(n_b, k, n_classes, k + 1); }
inline GridSlab varpro_class_prior_slab(int n_b, int k, int n_classes) { return varpro_class_slab(n_b, k, n_classes, kVarproPriorWaves * n_classes); }
}  // namespace pnx

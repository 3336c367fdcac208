// pnx_grid_class_args.hpp -- the host half of pnx_curvefit_grid_posterior_classes_f64 and pnx_curvefit_grid_prior_em_classes_f64
// (one prior row per segmentation label) that needs no device: the checks of n_classes, labels and the
// (n_classes, n_atoms) table in front of any device work, behind them the unlabelled calls' own checks; the per-row normalisers
// and starts; the centres of the moment accumulation; what an EM call reports; and the sizing of the kernels' LDS slab as a
// function of n_classes.  Free of HIP types, like its neighbours: pnx_api.hip and pnx_grid_class.hip use it,
// tests/host_stub/grid_class_args_stub.cpp builds the same code for the CPU under AddressSanitizer / UBSan.
#pragma once
#include <cmath>
#include <cstdint>

#include "pnx_grid_prior_args.hpp"

namespace pnx {

constexpr int kGridMaxClasses = 16;

// What the host derives from the table once per call, beside GridPosteriorHost.
struct GridClassHost {
    double norm[kGridMaxClasses] = {};  // per row log sum_g exp(log_prior[c, g]): log(n_atoms) for a uniform row
    int n_adm[kGridMaxClasses] = {};    // per row the number of finite entries
};

// n_classes, labels and the table.  Every row: each entry finite or -inf, at least one finite; a refusal names the row.  The
// normaliser of a row is posterior_check_log_prior's, so a row gives the bytes the unlabelled call gives for the same table.
inline int grid_class_check_table(const char *who, int n_classes, const int32_t *labels, int64_t n_vox, int n_atoms, const double *log_prior,
                                  GridClassHost *K) {
    if (n_classes < 1 || n_classes > kGridMaxClasses)
        return set_error(PNX_ERR_INVALID, "%s: n_classes=%d out of range [1,%d]", who, n_classes, kGridMaxClasses);
    if (n_vox > 0 && !labels) return set_error(PNX_ERR_INVALID, "%s: labels is NULL (one int32 per voxel)", who);
    for (int c = 0; c < n_classes; ++c) {
        const double *row = log_prior ? log_prior + (size_t)c * n_atoms : nullptr;
        int adm = n_atoms;
        if (row) {
            adm = 0;
            for (int g = 0; g < n_atoms; ++g) {
                const double l = row[g];
                if (std::isnan(l) || l == HUGE_VAL)
                    return set_error(PNX_ERR_INVALID, "%s: log_prior[%d, %d]=%g must be finite or -inf", who, c, g, l);
                adm += l > -HUGE_VAL;
            }
            if (!adm)
                return set_error(PNX_ERR_INVALID, "%s: log_prior row %d excludes every atom (all %d entries are -inf)", who, c, n_atoms);
        }
        K->n_adm[c] = adm;
        if (int rc = posterior_check_log_prior(who, n_atoms, row, &K->norm[c])) return rc;
    }
    return PNX_OK;
}

// The centres of the moment accumulation: mid-range of the atoms that ANY row admits (one set of centred parameter values serves
// every class; with one row, or rows that exclude the same atoms, these are the unlabelled call's centres).
inline void grid_class_centres(const pnx_curvefit_opts *o, int n_classes, int n_atoms, const double *atoms, const double *log_prior,
                               GridPosteriorHost *H) {
    for (int k = 0; k < o->n_free; ++k) {
        double mn = HUGE_VAL, mx = -HUGE_VAL;
        for (int g = 0; g < n_atoms; ++g) {
            bool any = !log_prior;
            for (int c = 0; c < n_classes && !any; ++c) any = log_prior[(size_t)c * n_atoms + g] != -HUGE_VAL;
            if (!any) continue;
            const double a = atoms[(size_t)k * n_atoms + g];
            mn = a < mn ? a : mn;
            mx = a > mx ? a : mx;
        }
        H->centre[k] = k == H->s0_row ? 0.0 : mn + 0.5 * (mx - mn);
    }
}

// The label checks first, then grid_posterior_check_args under the uniform prior (grid start's refusals, noise_sd, mean), then
// the centres over the table.
inline int grid_class_posterior_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                           const double *atoms, const double *fixed, const double *lo, const double *hi, int project_amplitude,
                                           int n_classes, const int32_t *labels, const double *log_prior, double noise_sd, const double *mean,
                                           int mem, GridPosteriorHost *H, GridClassHost *K) {
    if (n_classes < 1 || n_classes > kGridMaxClasses)
        return set_error(PNX_ERR_INVALID, "grid posterior: n_classes=%d out of range [1,%d]", n_classes, kGridMaxClasses);
    if (int rc = grid_posterior_check_args(o, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project_amplitude, nullptr, noise_sd, mean, mem, H))
        return rc;
    if (int rc = grid_class_check_table("grid posterior", n_classes, labels, n_vox, n_atoms, log_prior, K)) return rc;
    grid_class_centres(o, n_classes, n_atoms, atoms, log_prior, H);
    return PNX_OK;
}

// The EM's four arguments first, then the above with log_prior_out in the place of `mean`.
inline int grid_class_prior_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                       const double *atoms, const double *fixed, const double *lo, const double *hi, int project_amplitude,
                                       int n_classes, const int32_t *labels, const double *log_prior, double noise_sd, int n_iter,
                                       double pseudo_count, double rel_tol, const double *log_prior_out, int mem, GridPosteriorHost *H,
                                       GridClassHost *K) {
    if (int rc = prior_em_check_args("grid prior", n_iter, pseudo_count, rel_tol, log_prior_out)) return rc;
    if (n_classes < 1 || n_classes > kGridMaxClasses)
        return set_error(PNX_ERR_INVALID, "grid prior: n_classes=%d out of range [1,%d]", n_classes, kGridMaxClasses);
    if (int rc = grid_posterior_check_args(o, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project_amplitude, nullptr, noise_sd, log_prior_out, mem, H))
        return rc;
    if (int rc = grid_class_check_table("grid prior", n_classes, labels, n_vox, n_atoms, log_prior, K)) return rc;
    grid_class_centres(o, n_classes, n_atoms, atoms, log_prior, H);
    return PNX_OK;
}

// start[c, g] = log_prior[c, g] - norm[c]: grid_prior_start per row.
inline void grid_class_start(int n_classes, int n_atoms, const double *log_prior, const GridClassHost &K, double *start) {
    for (int c = 0; c < n_classes; ++c)
        grid_prior_start(n_atoms, log_prior ? log_prior + (size_t)c * n_atoms : nullptr, K.norm[c], start + (size_t)c * n_atoms);
}

// The optional outputs of an EM call that ended after `done` updates: entries of both traces past `done` are NaN.
inline void grid_class_report(int n_iter, int done, int n_classes, const int64_t *finite_voxels, double *loglik, double *loglik_class,
                              int *n_iter_done, int64_t *n_eff) {
    for (int t = done + 1; t <= n_iter; ++t) {
        if (loglik) loglik[t] = NAN;
        if (loglik_class)
            for (int c = 0; c < n_classes; ++c) loglik_class[(size_t)t * n_classes + c] = NAN;
    }
    if (n_iter_done) *n_iter_done = done;
    if (n_eff)
        for (int c = 0; c < n_classes; ++c) n_eff[c] = finite_voxels ? finite_voxels[c] : 0;
}

// The LDS image of a slab with n_classes prior rows: [kpad][stride] doubles of the dictionary, then per atom ||s||^2, its inverse,
// n_classes log-prior values and `extra` more -- the posterior's n_free centred parameter values (grid_class_posterior_slab) or
// the EM's 4 n_classes wave-private accumulator rows (grid_class_prior_slab, both passes).  grid_posterior_slab's rule otherwise
// (width a multiple of 16, stride = 16 mod 32, inside 64 KB); at n_classes = 1 these are the unlabelled kernels' slabs.
inline GridSlab grid_class_slab(int n_b, int n_classes, int extra) {
    GridSlab s;
    const int per_atom = 2 + n_classes + extra;
    s.kpad = (n_b + 3) & ~3;
    s.width = 16;
    for (int w = 16; w <= 256; w += 16) {
        const int stride = (w & 16) ? w : w + 16;
        if (s.kpad * stride + per_atom * w <= 8192) s.width = w;
    }
    s.stride = (s.width & 16) ? s.width : s.width + 16;
    s.lds_doubles = s.kpad * s.stride + per_atom * s.width;
    return s;
}
inline GridSlab grid_class_posterior_slab(int n_b, int n_free, int n_classes) { return grid_class_slab(n_b, n_classes, n_free); }
inline GridSlab grid_class_prior_slab(int n_b, int n_classes) { return grid_class_slab(n_b, n_classes, 4 * n_classes); }
}  // namespace pnx

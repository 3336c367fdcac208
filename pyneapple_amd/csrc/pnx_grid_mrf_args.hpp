// pnx_grid_mrf_args.hpp -- the host half of the neighbourhood (MRF) prior of the grid posterior that needs no device
// (pnx_curvefit_grid_neighbour_field_f64, pnx_curvefit_grid_posterior_field_f64, pnx_curvefit_grid_posterior_mrf_f64; DESIGN.md
// 4.1p): the checks of the voxel range, the neighbour table's shape, the colour ranges, the precisions and the sweep options in
// front of any device work, behind them the posterior's own checks; the per-row ranges that scale delta; the per-atom row
// r_g = sum_k precision_k (atoms[k, g] - centre_k)^2; the stopping rule and the report of a driver call; and the sizing of the
// field kernel's LDS slab.  Free of HIP types, like its neighbours: pnx_api.hip and pnx_grid_mrf.hip use it,
// tests/host_stub/grid_mrf_args_stub.cpp builds the same code for the CPU under AddressSanitizer / UBSan.
#pragma once
#include <cmath>
#include <cstdint>

#include "pnx_grid_posterior_args.hpp"

namespace pnx {

constexpr int kGridMrfMaxNeighbours = 8;
constexpr int kGridMrfMaxColours = 8;
constexpr int kGridMrfMaxSweeps = 100;
constexpr int kGridMrfReduceDoubles = 8;  // the tail of the slab: one partial maximum of delta per wave

// What the host derives for the field beside GridPosteriorHost.
struct GridMrfHost {
    double range[PNX_MAX_PARAMS] = {};  // per free parameter max - min of the atoms' values over the admissible atoms (0 for a projected S0)
};

// precision (n_free,): finite, >= 0, and 0 on the row of a projected S0 (that row has no grid value to pull towards).
inline int grid_mrf_check_precision(const char *who, int n_free, int s0_row, const double *precision) {
    if (!precision) return set_error(PNX_ERR_INVALID, "%s: precision is NULL (one value per free parameter)", who);
    for (int k = 0; k < n_free; ++k) {
        if (!(precision[k] >= 0.0) || std::isinf(precision[k]))
            return set_error(PNX_ERR_INVALID, "%s: precision[%d]=%g must be finite and >= 0", who, k, precision[k]);
        if (k == s0_row && precision[k] > 0.0)
            return set_error(PNX_ERR_INVALID, "%s: precision[%d]=%g on the projected S0 row must be 0 (a projected amplitude has no grid value)", who,
                             k, precision[k]);
    }
    return PNX_OK;
}

// The voxel range [first, first + count) of n_vox voxels; the neighbour table indexes voxels with int32.
inline int grid_mrf_check_range(const char *who, int64_t n_vox, int64_t first, int64_t count) {
    if (n_vox < 0 || n_vox > INT32_MAX) return set_error(PNX_ERR_INVALID, "%s: n_vox=%lld out of range [0,%d] (neighbours are int32)", who, (long long)n_vox, INT32_MAX);
    if (first < 0 || count < 0 || first > n_vox || count > n_vox - first)
        return set_error(PNX_ERR_INVALID, "%s: the range first=%lld, count=%lld does not lie inside the %lld voxels", who, (long long)first,
                         (long long)count, (long long)n_vox);
    return PNX_OK;
}

inline int grid_mrf_check_n_nb(const char *who, int n_nb) {
    if (n_nb < 1 || n_nb > kGridMrfMaxNeighbours) return set_error(PNX_ERR_INVALID, "%s: n_nb=%d out of range [1,%d]", who, n_nb, kGridMrfMaxNeighbours);
    return PNX_OK;
}

// The gather.
inline int grid_mrf_field_check_args(int64_t n_vox, int64_t first, int64_t count, int n_free, int n_nb, const int32_t *neighbours,
                                     const double *mean, const double *centre, const double *precision, const double *field_q,
                                     const int32_t *field_n, int mem) {
    const char *who = "grid neighbour field";
    if (n_free < 1 || n_free > PNX_MAX_PARAMS) return set_error(PNX_ERR_INVALID, "%s: n_free=%d out of range [1,%d]", who, n_free, PNX_MAX_PARAMS);
    if (int rc = grid_mrf_check_n_nb(who, n_nb)) return rc;
    if (int rc = grid_mrf_check_range(who, n_vox, first, count)) return rc;
    if (mem != PNX_MEM_HOST && mem != PNX_MEM_DEVICE) return set_error(PNX_ERR_INVALID, "mem=%d", mem);
    if (!centre) return set_error(PNX_ERR_INVALID, "%s: centre is NULL (one value per free parameter)", who);
    if (int rc = grid_mrf_check_precision(who, n_free, -1, precision)) return rc;
    for (int k = 0; k < n_free; ++k)
        if (!std::isfinite(centre[k])) return set_error(PNX_ERR_INVALID, "%s: centre[%d]=%g must be finite", who, k, centre[k]);
    if (n_vox && (!neighbours || !mean || !field_q || !field_n))
        return set_error(PNX_ERR_INVALID, "%s: NULL data pointer (neighbours, mean, field_q and field_n are all required)", who);
    return PNX_OK;
}

// max - min of every free parameter over the admissible atoms: what delta is measured in.
inline void grid_mrf_ranges(int n_free, int n_atoms, const double *atoms, const double *log_prior, int s0_row, GridMrfHost *M) {
    for (int k = 0; k < n_free; ++k) {
        double mn = HUGE_VAL, mx = -HUGE_VAL;
        for (int g = 0; g < n_atoms; ++g) {
            if (log_prior && log_prior[g] == -HUGE_VAL) continue;
            const double a = atoms[(size_t)k * n_atoms + g];
            mn = a < mn ? a : mn;
            mx = a > mx ? a : mx;
        }
        M->range[k] = k == s0_row ? 0.0 : mx - mn;
    }
}

// One colour update: the posterior's checks first, then the range, the field and the precisions.  Device memory only.
inline int grid_mrf_posterior_field_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                               const double *atoms, const double *fixed, const double *lo, const double *hi,
                                               int project_amplitude, const double *log_prior, double noise_sd, int64_t first, int64_t count,
                                               const double *field_q, const int32_t *field_n, const double *precision, const double *mean,
                                               int mem, GridPosteriorHost *H, GridMrfHost *M) {
    const char *who = "grid posterior field";
    if (int rc = grid_posterior_check_args(o, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project_amplitude, log_prior, noise_sd, mean, mem, H))
        return rc;
    if (mem != PNX_MEM_DEVICE) return set_error(PNX_ERR_INVALID, "%s: mem=%d: the call works in place on device arrays (PNX_MEM_DEVICE) only", who, mem);
    if (int rc = grid_mrf_check_range(who, n_vox, first, count)) return rc;
    if (n_vox && (!field_q || !field_n)) return set_error(PNX_ERR_INVALID, "%s: field_q or field_n is NULL", who);
    if (int rc = grid_mrf_check_precision(who, o->n_free, H->s0_row, precision)) return rc;
    grid_mrf_ranges(o->n_free, n_atoms, atoms, log_prior, H->s0_row, M);
    return PNX_OK;
}

// The driver: everything the posterior refuses, then n_nb, n_colours, n_sweeps, tol, the colour ranges and the precisions.
inline int grid_mrf_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms, const double *atoms,
                               const double *fixed, const double *lo, const double *hi, int project_amplitude, const double *log_prior,
                               double noise_sd, int n_nb, const int32_t *neighbours, int n_colours, const int64_t *colour_start,
                               const double *precision, int n_sweeps, double tol, const double *mean, int mem, GridPosteriorHost *H,
                               GridMrfHost *M) {
    const char *who = "grid posterior mrf";
    if (int rc = grid_posterior_check_args(o, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project_amplitude, log_prior, noise_sd, mean, mem, H))
        return rc;
    if (int rc = grid_mrf_check_n_nb(who, n_nb)) return rc;
    if (n_colours < 1 || n_colours > kGridMrfMaxColours)
        return set_error(PNX_ERR_INVALID, "%s: n_colours=%d out of range [1,%d]", who, n_colours, kGridMrfMaxColours);
    if (n_sweeps < 0 || n_sweeps > kGridMrfMaxSweeps)
        return set_error(PNX_ERR_INVALID, "%s: n_sweeps=%d out of range [0,%d]", who, n_sweeps, kGridMrfMaxSweeps);
    if (!(tol >= 0.0) || std::isinf(tol)) return set_error(PNX_ERR_INVALID, "%s: tol=%g must be finite and >= 0", who, tol);
    if (int rc = grid_mrf_check_range(who, n_vox, 0, n_vox)) return rc;
    if (n_vox && !neighbours) return set_error(PNX_ERR_INVALID, "%s: neighbours is NULL ((n_vox, n_nb) int32, -1 where empty)", who);
    if (!colour_start) return set_error(PNX_ERR_INVALID, "%s: colour_start is NULL (n_colours + 1 offsets)", who);
    if (colour_start[0] != 0 || colour_start[n_colours] != n_vox)
        return set_error(PNX_ERR_INVALID, "%s: colour_start must run from 0 to n_vox=%lld, got %lld .. %lld", who, (long long)n_vox,
                         (long long)colour_start[0], (long long)colour_start[n_colours]);
    for (int c = 0; c < n_colours; ++c)
        if (colour_start[c + 1] < colour_start[c])
            return set_error(PNX_ERR_INVALID, "%s: colour_start is not ascending at colour %d (%lld > %lld)", who, c, (long long)colour_start[c],
                             (long long)colour_start[c + 1]);
    if (int rc = grid_mrf_check_precision(who, o->n_free, H->s0_row, precision)) return rc;
    grid_mrf_ranges(o->n_free, n_atoms, atoms, log_prior, H->s0_row, M);
    return PNX_OK;
}

// r_g = sum_k precision_k (atoms[k, g] - centre_k)^2, k ascending, for the gp padded atoms (0 for a padded one).  The difference
// is the very subtraction the posterior's preparation does on the device, so r_g belongs to the theta the kernel reads.
inline void grid_mrf_r(int n_free, int n_atoms, int gp, const double *atoms, const double *centre, const double *precision, double *r) {
    for (int g = 0; g < gp; ++g) {
        double s = 0.0;
        for (int k = 0; k < n_free && g < n_atoms; ++k) {
            const double t = atoms[(size_t)k * n_atoms + g] - centre[k];
            s += precision[k] * (t * t);
        }
        r[g] = s;
    }
}

// What delta of a row is divided by: its range where the row takes part (precision > 0 and more than one grid value), else 0.
inline void grid_mrf_delta_scale(int n_free, const double *precision, const GridMrfHost &M, double *scale) {
    for (int k = 0; k < PNX_MAX_PARAMS; ++k) scale[k] = (k < n_free && precision[k] > 0.0 && M.range[k] > 0.0) ? M.range[k] : 0.0;
}

inline bool grid_mrf_any_precision(int n_free, const double *precision) {
    for (int k = 0; k < n_free; ++k)
        if (precision[k] > 0.0) return true;
    return false;
}

// The optional outputs of a driver call that ended after `done` sweeps: entries of delta past `done` are NaN.
inline void grid_mrf_report(int n_sweeps, int done, const double *trace, double *delta, int *n_sweeps_done) {
    if (delta)
        for (int s = 0; s < n_sweeps; ++s) delta[s] = s < done ? trace[s] : NAN;
    if (n_sweeps_done) *n_sweeps_done = done;
}

// The LDS image of a slab of the field posterior: [kpad][stride] doubles of the dictionary, then per atom ||s||^2, its inverse,
// log_prior, r_g and the n_free centred parameter values, then kGridMrfReduceDoubles for the block's reduction of delta.
// grid_posterior_slab's rule otherwise (width a multiple of 16, stride = 16 mod 32, inside 64 KB).
inline GridSlab grid_mrf_slab(int n_b, int n_free) {
    GridSlab s;
    const int per_atom = 4 + n_free;
    s.kpad = (n_b + 3) & ~3;
    s.width = 16;
    for (int w = 16; w <= 256; w += 16) {
        const int stride = (w & 16) ? w : w + 16;
        if (s.kpad * stride + per_atom * w + kGridMrfReduceDoubles <= 8192) s.width = w;
    }
    s.stride = (s.width & 16) ? s.width : s.width + 16;
    s.lds_doubles = s.kpad * s.stride + per_atom * s.width + kGridMrfReduceDoubles;
    return s;
}
}  // namespace pnx

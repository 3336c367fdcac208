// pnx_varpro_mrf_args.hpp -- the host half of the neighbourhood (MRF) prior of the posterior over the variable projection's
// dictionary that needs no device (pnx_curvefit_varpro_posterior_field_f64, pnx_curvefit_varpro_posterior_mrf_f64; DESIGN.md
// 4.1q): the posterior's own checks, behind them the voxel range, the neighbour table's shape, the colour ranges, the sweep options
// and the precisions (0 on every fraction / S0 row: its value belongs to the voxel-atom pair, not to the grid); the per-row ranges
// that scale delta; the per-atom row r_g = sum_k precision_k (nl_atoms[row_k, g] - centre_k)^2 over the non-linear rows; and the
// sizing of the field kernel's LDS slab.  The range, n_nb, delta-scale and report helpers and the limits kGridMrfMax* are the grid
// driver's (pnx_grid_mrf_args.hpp).  Free of HIP types, like its neighbours: pnx_api.hip and pnx_varpro_mrf.hip use it,
// tests/host_stub/varpro_mrf_args_stub.cpp builds the same code for the CPU under AddressSanitizer / UBSan.
#pragma once
#include <cmath>
#include <cstdint>

#include "pnx_grid_mrf_args.hpp"
#include "pnx_varpro_posterior_args.hpp"

namespace pnx {

// What the host derives for the field beside VarproPosteriorHost.
struct VarproMrfHost {
    double range[PNX_MAX_PARAMS] = {};  // per free parameter max - min of the row of nl_atoms over the admissible atoms; 0 for a linear row
};

// precision (n_free,): finite, >= 0, and 0 on a fraction / S0 row.
inline int varpro_mrf_check_precision(const char *who, int n_free, const VarproLayout &L, const double *precision) {
    if (!precision) return set_error(PNX_ERR_INVALID, "%s: precision is NULL (one value per free parameter)", who);
    for (int k = 0; k < n_free; ++k) {
        if (!(precision[k] >= 0.0) || std::isinf(precision[k]))
            return set_error(PNX_ERR_INVALID, "%s: precision[%d]=%g must be finite and >= 0", who, k, precision[k]);
        if (L.row_src[k] < 0 && precision[k] > 0.0)
            return set_error(PNX_ERR_INVALID, "%s: precision[%d]=%g on a fraction / S0 row must be 0 (an amplitude solved per voxel and atom has no "
                                              "grid value)", who, k, precision[k]);
    }
    return PNX_OK;
}

// max - min of every non-linear free parameter over the admissible atoms: what delta is measured in.
inline void varpro_mrf_ranges(int n_free, const VarproLayout &L, int n_atoms, const double *nl_atoms, const double *log_prior, VarproMrfHost *M) {
    for (int k = 0; k < n_free; ++k) {
        M->range[k] = 0.0;
        if (L.row_src[k] < 0) continue;
        double mn = HUGE_VAL, mx = -HUGE_VAL;
        for (int g = 0; g < n_atoms; ++g) {
            if (log_prior && log_prior[g] == -HUGE_VAL) continue;
            const double a = nl_atoms[(size_t)L.row_src[k] * n_atoms + g];
            mn = a < mn ? a : mn;
            mx = a > mx ? a : mx;
        }
        M->range[k] = mx - mn;
    }
}

// One colour update: the posterior's checks first, then the range, the field and the precisions.  Device memory only.
inline int varpro_mrf_posterior_field_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                                 const double *nl_atoms, const double *fixed, const double *lo, const double *hi,
                                                 const double *log_prior, double noise_sd, int marginal_amplitudes, int64_t first, int64_t count,
                                                 const double *field_q, const int32_t *field_n, const double *precision, const double *mean,
                                                 int mem, VarproLayout *L, VarproPosteriorHost *H, VarproMrfHost *M) {
    const char *who = "varpro posterior field";
    if (int rc = varpro_posterior_check_args(o, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, log_prior, noise_sd, marginal_amplitudes, mean, mem,
                                             L, H))
        return rc;
    if (mem != PNX_MEM_DEVICE) return set_error(PNX_ERR_INVALID, "%s: mem=%d: the call works in place on device arrays (PNX_MEM_DEVICE) only", who, mem);
    if (int rc = grid_mrf_check_range(who, n_vox, first, count)) return rc;
    if (n_vox && (!field_q || !field_n)) return set_error(PNX_ERR_INVALID, "%s: field_q or field_n is NULL", who);
    if (int rc = varpro_mrf_check_precision(who, o->n_free, *L, precision)) return rc;
    varpro_mrf_ranges(o->n_free, *L, n_atoms, nl_atoms, log_prior, M);
    return PNX_OK;
}

// The driver: everything the posterior refuses, then n_nb, n_colours, n_sweeps, tol, the colour ranges and the precisions.
inline int varpro_mrf_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms, const double *nl_atoms,
                                 const double *fixed, const double *lo, const double *hi, const double *log_prior, double noise_sd,
                                 int marginal_amplitudes, int n_nb, const int32_t *neighbours, int n_colours, const int64_t *colour_start,
                                 const double *precision, int n_sweeps, double tol, const double *mean, int mem, VarproLayout *L,
                                 VarproPosteriorHost *H, VarproMrfHost *M) {
    const char *who = "varpro posterior mrf";
    if (int rc = varpro_posterior_check_args(o, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, log_prior, noise_sd, marginal_amplitudes, mean, mem,
                                             L, H))
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
    if (int rc = varpro_mrf_check_precision(who, o->n_free, *L, precision)) return rc;
    varpro_mrf_ranges(o->n_free, *L, n_atoms, nl_atoms, log_prior, M);
    return PNX_OK;
}

// r_g = sum_k precision_k (nl_atoms[row_k, g] - centre_k)^2 over the free rows k ascending (a linear row has no grid value and
// adds nothing), for the gp padded atoms (0 for a padded one).  The difference is the very subtraction the posterior's preparation
// does on the device, so r_g belongs to the theta the kernel reads.
inline void varpro_mrf_r(int n_free, const VarproLayout &L, int n_atoms, int gp, const double *nl_atoms, const double *centre,
                         const double *precision, double *r) {
    for (int g = 0; g < gp; ++g) {
        double s = 0.0;
        for (int k = 0; k < n_free && g < n_atoms; ++k) {
            if (L.row_src[k] < 0) continue;
            const double t = nl_atoms[(size_t)L.row_src[k] * n_atoms + g] - centre[k];
            s += precision[k] * (t * t);
        }
        r[g] = s;
    }
}

// The LDS image of a slab of the field posterior: varpro_posterior_slab's (k blocks of [kpad][stride], the constants, lw and the
// k + 1 centred non-linear values) with one more per-atom row, r_g, then kGridMrfReduceDoubles for the block's reduction of delta.
inline GridSlab varpro_mrf_slab(int n_b, int k) {
    GridSlab s;
    const int rows = varpro_const_rows(k) + varpro_posterior_extra_rows(k) + 1;
    s.kpad = (n_b + 3) & ~3;
    s.width = 16;
    for (int w = 16; w <= 256; w += 16) {
        const int stride = (w & 16) ? w : w + 16;
        if (k * s.kpad * stride + rows * w + kGridMrfReduceDoubles <= 8192) s.width = w;
    }
    s.stride = (s.width & 16) ? s.width : s.width + 16;
    s.lds_doubles = k * s.kpad * s.stride + rows * s.width + kGridMrfReduceDoubles;
    return s;
}
}  // namespace pnx

// pnx_varpro_logmrf_args.hpp -- the host half of the neighbourhood (MRF) prior of the variable-projection posterior with a
// per-row choice of the coupled quantity (pnx_curvefit_varpro_posterior_logfield_f64, pnx_curvefit_varpro_posterior_logmrf_f64;
// DESIGN.md 4.1r) that needs no device.  Every free non-linear row k couples f_k = nl_atoms[row_k] (coupling 0) or
// f_k = log nl_atoms[row_k] (coupling 1); the checks of pnx_varpro_mrf_args.hpp stay in front, behind them the coupling flags; then
// the centres and ranges of f over the admissible atoms, the centred field rows fc_kg = f_kg - fcentre_k, the per-atom row
// r_g = sum_k precision_k fc_kg^2 and the sizing of the kernel's LDS slab (the field rows sit beside the moment rows).  On a
// coupling-0 row fcentre, the range, fc and that row's share of r_g are the bytes pnx_varpro_mrf_args.hpp and the posterior's
// preparation derive.  Free of HIP types, like its neighbours: pnx_api.hip and pnx_varpro_logmrf.hip use it.
#pragma once
#include <cmath>
#include <cstdint>

#include "pnx_varpro_mrf_args.hpp"

namespace pnx {

// What the host derives for the coupled rows beside VarproPosteriorHost and VarproMrfHost.
struct VarproLogMrfHost {
    double fcentre[PNX_MAX_PARAMS] = {};  // per free parameter min + (max - min) / 2 of f over the admissible atoms; 0 for a fraction / S0 row
    double frange[PNX_MAX_PARAMS] = {};   // per free parameter max - min of f over the admissible atoms; 0 for a fraction / S0 row
};

// f of one atom of a row
inline double varpro_logmrf_f(int coupling, double a) { return coupling ? std::log(a) : a; }

// coupling (n_free,): 0 or 1; 0 on a fraction / S0 row and where the precision is 0; a log row needs every admissible atom > 0.
// Fills fcentre and frange.
inline int varpro_logmrf_check_coupling(const char *who, int n_free, const VarproLayout &L, int n_atoms, const double *nl_atoms,
                                        const double *log_prior, const double *precision, const int32_t *coupling, VarproLogMrfHost *G) {
    if (!coupling) return set_error(PNX_ERR_INVALID, "%s: coupling is NULL (one flag per free parameter: 0 linear, 1 log)", who);
    for (int k = 0; k < n_free; ++k) {
        G->fcentre[k] = G->frange[k] = 0.0;
        if (coupling[k] != 0 && coupling[k] != 1)
            return set_error(PNX_ERR_INVALID, "%s: coupling[%d]=%d must be 0 (linear) or 1 (log)", who, k, (int)coupling[k]);
        if (L.row_src[k] < 0) {
            if (coupling[k])
                return set_error(PNX_ERR_INVALID, "%s: coupling[%d]=1 on a fraction / S0 row must be 0 (an amplitude solved per voxel and atom "
                                                  "is not coupled)", who, k);
            continue;
        }
        if (coupling[k] && !(precision[k] > 0.0))
            return set_error(PNX_ERR_INVALID, "%s: coupling[%d]=1 with precision[%d]=0 must be 0 (a row that is not coupled has no coupled "
                                              "quantity)", who, k, k);
        double mn = HUGE_VAL, mx = -HUGE_VAL;
        for (int g = 0; g < n_atoms; ++g) {
            if (log_prior && log_prior[g] == -HUGE_VAL) continue;
            const double a = nl_atoms[(size_t)L.row_src[k] * n_atoms + g];
            if (coupling[k] && !(a > 0.0))
                return set_error(PNX_ERR_INVALID, "%s: coupling[%d]=1 (log) needs positive values: nl_atoms[%d, %d]=%g", who, k, L.row_src[k], g, a);
            const double f = varpro_logmrf_f(coupling[k], a);
            mn = f < mn ? f : mn;
            mx = f > mx ? f : mx;
        }
        G->fcentre[k] = mn + 0.5 * (mx - mn);
        G->frange[k] = mx - mn;
    }
    return PNX_OK;
}

// The one layout the fold has no form for: three compartments with S0 and a free T1 above 32 b-values.  Even with one voxel row
// per sweep and the means of fc in a pass of their own its state does not fit the register file, and no form may use scratch
// (DESIGN.md 4.1r).  The linear calls take it.
inline int varpro_logmrf_check_layout(const char *who, const VarproLayout &L, int n_b) {
    if (L.k == 3 && L.cls == kVarproS0 && L.n_nl > L.k && n_b > 32)
        return set_error(PNX_ERR_UNSUPPORTED, "%s: three compartments with S0 and a free T1 at n_b=%d > 32 is not built (its fold does not fit "
                                              "the register file); pnx_curvefit_varpro_posterior_mrf_f64 takes this layout", who, n_b);
    return PNX_OK;
}

// One colour update: pnx_curvefit_varpro_posterior_field_f64's checks, then coupling and field_mean.
inline int varpro_logmrf_posterior_field_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                                    const double *nl_atoms, const double *fixed, const double *lo, const double *hi,
                                                    const double *log_prior, double noise_sd, int marginal_amplitudes, int64_t first,
                                                    int64_t count, const double *field_q, const int32_t *field_n, const double *precision,
                                                    const int32_t *coupling, const double *mean, const double *field_mean, int mem,
                                                    VarproLayout *L, VarproPosteriorHost *H, VarproMrfHost *M, VarproLogMrfHost *G) {
    const char *who = "varpro posterior logfield";
    if (int rc = varpro_mrf_posterior_field_check_args(o, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, log_prior, noise_sd, marginal_amplitudes,
                                                       first, count, field_q, field_n, precision, mean, mem, L, H, M))
        return rc;
    if (!field_mean) return set_error(PNX_ERR_INVALID, "%s: field_mean is NULL ((n_free, n_vox), read for delta and written in place)", who);
    if (int rc = varpro_logmrf_check_layout(who, *L, o->n_b)) return rc;
    return varpro_logmrf_check_coupling(who, o->n_free, *L, n_atoms, nl_atoms, log_prior, precision, coupling, G);
}

// The driver: pnx_curvefit_varpro_posterior_mrf_f64's checks, then coupling (field_mean is optional there).
inline int varpro_logmrf_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                    const double *nl_atoms, const double *fixed, const double *lo, const double *hi, const double *log_prior,
                                    double noise_sd, int marginal_amplitudes, int n_nb, const int32_t *neighbours, int n_colours,
                                    const int64_t *colour_start, const double *precision, const int32_t *coupling, int n_sweeps, double tol,
                                    const double *mean, int mem, VarproLayout *L, VarproPosteriorHost *H, VarproMrfHost *M,
                                    VarproLogMrfHost *G) {
    if (int rc = varpro_mrf_check_args(o, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, log_prior, noise_sd, marginal_amplitudes, n_nb, neighbours,
                                       n_colours, colour_start, precision, n_sweeps, tol, mean, mem, L, H, M))
        return rc;
    if (int rc = varpro_logmrf_check_layout("varpro posterior logmrf", *L, o->n_b)) return rc;
    return varpro_logmrf_check_coupling("varpro posterior logmrf", o->n_free, *L, n_atoms, nl_atoms, log_prior, precision, coupling, G);
}

// fc (n_nl, gp): fc[row_k, g] = f_kg - fcentre_k, 0 for a padded atom and for a row of nl_atoms that is not free;
// r (gp): r_g = sum_k precision_k fc_kg^2 over the free rows k ascending (a fraction / S0 row adds nothing), 0 for a padded atom.
// On a coupling-0 row the difference is the very subtraction the posterior's preparation does on the device and the sum is
// varpro_mrf_r's, so with every coupling 0 both are the bytes the linear field reads.
inline void varpro_logmrf_rows(int n_free, const VarproLayout &L, int n_atoms, int gp, const double *nl_atoms, const double *fcentre,
                               const double *precision, const int32_t *coupling, double *fc, double *r) {
    for (size_t i = 0; i < (size_t)L.n_nl * gp; ++i) fc[i] = 0.0;
    for (int g = 0; g < gp; ++g) {
        double s = 0.0;
        for (int k = 0; k < n_free && g < n_atoms; ++k) {
            if (L.row_src[k] < 0) continue;
            const double a = nl_atoms[(size_t)L.row_src[k] * n_atoms + g];
            // a non-positive value on a log row belongs to an excluded atom (checked): it is skipped by the fold and holds 0 here
            const double t = (coupling[k] && !(a > 0.0)) ? 0.0 : varpro_logmrf_f(coupling[k], a) - fcentre[k];
            fc[(size_t)L.row_src[k] * gp + g] = t;
            s += precision[k] * (t * t);
        }
        r[g] = s;
    }
}

// What delta of a row is divided by: the range of f where the row takes part (precision > 0 and more than one value), else 0.
inline void varpro_logmrf_delta_scale(int n_free, const double *precision, const VarproLogMrfHost &G, double *scale) {
    for (int k = 0; k < PNX_MAX_PARAMS; ++k) scale[k] = (k < n_free && precision[k] > 0.0 && G.frange[k] > 0.0) ? G.frange[k] : 0.0;
}

// The LDS image of a slab of the log-field posterior: varpro_mrf_slab's with k + 1 more per-atom rows, the centred field rows fc
// beside the centred moment rows theta, then kGridMrfReduceDoubles for the block's reduction of delta.
inline GridSlab varpro_logmrf_slab(int n_b, int k) {
    GridSlab s;
    const int rows = varpro_const_rows(k) + varpro_posterior_extra_rows(k) + 1 + (k + 1);
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

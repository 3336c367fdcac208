// pnx_grid_posterior_args.hpp -- the host half of pnx_curvefit_grid_posterior_f64 that needs no device: the checks of its
// arguments in front of any device work (grid start's, then log_prior and noise_sd), the normaliser of the prior, the per-row
// centres of the moment accumulation and the sizing of the posterior kernel's LDS slab.  Free of HIP types, like
// pnx_grid_args.hpp: pnx_api.hip and pnx_grid_posterior.hip use it, tests/host_stub/grid_posterior_args_stub.cpp builds the
// same code for the CPU under AddressSanitizer / UBSan.
#pragma once
#include <cmath>
#include <cstdint>

#include "pnx_grid_args.hpp"

namespace pnx {

// What the host derives from the arguments once per call.
struct GridPosteriorHost {
    int s0_row = -1;             // row of S0 among the free parameters when the amplitude is projected
    double log_prior_norm = 0.0; // log sum_g exp(log_prior_g): log(n_atoms) for the uniform prior
    double centre[PNX_MAX_PARAMS] = {};  // per free parameter: mid-range of the admissible atoms (0 for a projected S0 row)
};

// The prior of a posterior over a dictionary (`who` in front of a message): NULL is uniform; every entry finite or -inf, at least
// one finite.  *norm = log sum_g exp(log_prior_g) by a two-pass log-sum-exp, log(n_atoms) for the uniform prior.
inline int posterior_check_log_prior(const char *who, int n_atoms, const double *log_prior, double *norm) {
    if (!log_prior) {
        *norm = std::log((double)n_atoms);
        return PNX_OK;
    }
    double top = -HUGE_VAL;
    for (int g = 0; g < n_atoms; ++g) {
        const double l = log_prior[g];
        if (std::isnan(l) || l == HUGE_VAL) return set_error(PNX_ERR_INVALID, "%s: log_prior[%d]=%g must be finite or -inf", who, g, l);
        top = l > top ? l : top;
    }
    if (top == -HUGE_VAL) return set_error(PNX_ERR_INVALID, "%s: log_prior excludes every atom (all %d entries are -inf)", who, n_atoms);
    double s = 0.0;
    for (int g = 0; g < n_atoms; ++g) s += std::exp(log_prior[g] - top);
    *norm = top + std::log(s);
    return PNX_OK;
}

// grid_check_args (the refusals and the atom / bounds checks of grid start, unchanged), then the two new inputs.  Every refusal
// names its argument.  `mean` takes the place of p0_out: the one output that may not be NULL.
inline int grid_posterior_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                     const double *atoms, const double *fixed, const double *lo, const double *hi, int project_amplitude,
                                     const double *log_prior, double noise_sd, const double *mean, int mem, GridPosteriorHost *H) {
    if (!mean) return set_error(PNX_ERR_INVALID, "grid posterior: mean is NULL (the one output that is not optional)");
    if (!(noise_sd >= 0.0) || std::isinf(noise_sd))
        return set_error(PNX_ERR_INVALID, "grid posterior: noise_sd=%g must be finite and > 0 (known noise) or 0 (marginalised)", noise_sd);
    if (int rc = grid_check_args(o, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project_amplitude, mean, mem, &H->s0_row)) return rc;
    if (int rc = posterior_check_log_prior("grid posterior", n_atoms, log_prior, &H->log_prior_norm)) return rc;
    // centres: min + (max - min) / 2 over the admissible atoms, exact when they all hold one value
    for (int k = 0; k < o->n_free; ++k) {
        double mn = HUGE_VAL, mx = -HUGE_VAL;
        for (int g = 0; g < n_atoms; ++g) {
            if (log_prior && log_prior[g] == -HUGE_VAL) continue;
            const double a = atoms[(size_t)k * n_atoms + g];
            mn = a < mn ? a : mn;
            mx = a > mx ? a : mx;
        }
        H->centre[k] = k == H->s0_row ? 0.0 : mn + 0.5 * (mx - mn);
    }
    return PNX_OK;
}

// The posterior kernel's LDS image of a slab: [kpad][stride] doubles of the dictionary, then per atom ||s||^2, its inverse,
// log_prior and the n_free centred parameter values.  width and stride follow grid_slab's rule (stride = 16 mod 32).
inline GridSlab grid_posterior_slab(int n_b, int n_free) {
    GridSlab s;
    s.kpad = (n_b + 3) & ~3;
    s.width = 16;
    for (int w = 16; w <= 256; w += 16) {
        const int stride = (w & 16) ? w : w + 16;
        if (s.kpad * stride + (3 + n_free) * w <= 8192) s.width = w;
    }
    s.stride = (s.width & 16) ? s.width : s.width + 16;
    s.lds_doubles = s.kpad * s.stride + (3 + n_free) * s.width;
    return s;
}
}  // namespace pnx

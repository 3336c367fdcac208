// pnx_grid_marginal_args.hpp -- the host half of pnx_curvefit_grid_marginals_f64 that needs no device: the checks of its
// arguments in front of any device work (the outputs and the quantile levels, the posterior's, shared, then the binning), the
// table of global bin indices the kernel reads per atom, and the choice of its instantiation.  Free of HIP types, like
// pnx_grid_prior_args.hpp: pnx_api.hip and pnx_grid_marginal.hip use it, tests/host_stub/grid_marginal_args_stub.cpp builds the
// same code for the CPU under AddressSanitizer / UBSan.
#pragma once
#include <cmath>
#include <cstdint>

#include "pnx_grid_prior_args.hpp"

namespace pnx {

constexpr int kGridMarginalMaxBins = 128;  // B = sum n_bins: eight 16-bin chunks of accumulators per lane
constexpr int kGridMarginalMaxProbs = 8;

// What the host derives from the binning once per call.
struct GridMarginalHost {
    int n_bins_total = 0;             // B
    int n_rows = 0;                   // free parameters with a marginal: the rows of the table
    int n_bins[PNX_MAX_PARAMS] = {};  // per free parameter, 0: none
    int off[PNX_MAX_PARAMS] = {};     // per free parameter: its first bin among the B
};

// The outputs and the quantile levels first, then grid_posterior_check_args with `marginal` in the place of `mean` (the
// posterior's refusals, weighting and prior rules hold unchanged), then the binning.  Every refusal names its first offender.
inline int grid_marginal_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                    const double *atoms, const double *fixed, const double *lo, const double *hi, int project_amplitude,
                                    const double *log_prior, double noise_sd, const int32_t *n_bins, const int32_t *bin_of,
                                    const double *bin_value, int n_q, const double *probs, const double *marginal, const double *quantile,
                                    int mem, GridPosteriorHost *H, GridMarginalHost *M) {
    if (!marginal) return set_error(PNX_ERR_INVALID, "grid marginals: marginal is NULL (the one output that is not optional)");
    if (n_q < 0 || n_q > kGridMarginalMaxProbs)
        return set_error(PNX_ERR_INVALID, "grid marginals: n_q=%d out of range [0,%d]", n_q, kGridMarginalMaxProbs);
    if (n_q && !probs) return set_error(PNX_ERR_INVALID, "grid marginals: probs is NULL but n_q=%d", n_q);
    if (n_q && !quantile) return set_error(PNX_ERR_INVALID, "grid marginals: quantile is NULL but n_q=%d", n_q);
    for (int i = 0; i < n_q; ++i)
        if (!(probs[i] > 0.0 && probs[i] < 1.0))
            return set_error(PNX_ERR_INVALID, "grid marginals: probs[%d]=%g must lie in the open interval (0, 1)", i, probs[i]);
    if (!n_bins || !bin_of || !bin_value) return set_error(PNX_ERR_INVALID, "grid marginals: n_bins, bin_of or bin_value is NULL");
    if (int rc = grid_posterior_check_args(o, n_vox, b, y, n_atoms, atoms, fixed, lo, hi, project_amplitude, log_prior, noise_sd, marginal, mem, H))
        return rc;
    long long total = 0;
    for (int k = 0; k < o->n_free; ++k) {
        if (n_bins[k] < 0) return set_error(PNX_ERR_INVALID, "grid marginals: n_bins[%d]=%d is negative", k, n_bins[k]);
        total += n_bins[k];
    }
    if (total < 1 || total > kGridMarginalMaxBins)
        return set_error(PNX_ERR_INVALID, "grid marginals: B = sum n_bins = %lld out of range [1,%d]", total, kGridMarginalMaxBins);
    if (H->s0_row >= 0 && n_bins[H->s0_row] != 0)
        return set_error(PNX_ERR_INVALID, "grid marginals: n_bins[%d]=%d for the projected S0 row must be 0 (its value is the fitted "
                                          "amplitude, not a grid value)", H->s0_row, n_bins[H->s0_row]);
    *M = GridMarginalHost();
    M->n_bins_total = (int)total;
    for (int k = 0, off = 0; k < o->n_free; ++k) {
        M->n_bins[k] = n_bins[k];
        M->off[k] = off;
        off += n_bins[k];
        M->n_rows += n_bins[k] > 0;
    }
    for (int k = 0; k < o->n_free; ++k) {
        const int nb = M->n_bins[k], off = M->off[k];
        for (int j = 0; j < nb; ++j) {
            if (std::isnan(bin_value[off + j])) return set_error(PNX_ERR_INVALID, "grid marginals: bin_value[%d] is NaN", off + j);
            if (j && !(bin_value[off + j] > bin_value[off + j - 1]))
                return set_error(PNX_ERR_INVALID, "grid marginals: bin_value[%d]=%g is not above bin_value[%d]=%g (free parameter %d: "
                                                  "strictly ascending)", off + j, bin_value[off + j], off + j - 1, bin_value[off + j - 1], k);
        }
        for (int g = 0; g < n_atoms && nb; ++g) {
            const int bin = bin_of[(size_t)k * n_atoms + g];
            if (bin < 0 || bin >= nb)
                return set_error(PNX_ERR_INVALID, "grid marginals: bin_of[%d, %d]=%d out of range [0,%d)", k, g, bin, nb);
            const double a = atoms[(size_t)k * n_atoms + g];
            if (!(a == bin_value[off + bin]))
                return set_error(PNX_ERR_INVALID, "grid marginals: atom %d, free parameter %d = %.17g is not bin_value[%d]=%.17g of its bin %d",
                                 g, k, a, off + bin, bin_value[off + bin], bin);
        }
    }
    return PNX_OK;
}

// table (n_rows, gp): per free parameter with a marginal, in their order, and atom the global bin index off_k + bin_of[k, g];
// -1 for the padded atoms g >= n_atoms, which no bin matches.
inline void grid_marginal_table(int n_free, int n_atoms, int gp, const GridMarginalHost &M, const int32_t *bin_of, int32_t *table) {
    int row = 0;
    for (int k = 0; k < n_free; ++k) {
        if (!M.n_bins[k]) continue;
        for (int g = 0; g < gp; ++g) table[(size_t)row * gp + g] = g < n_atoms ? M.off[k] + bin_of[(size_t)k * n_atoms + g] : -1;
        ++row;
    }
}

// 16-bin chunks of accumulators the kernel is instantiated with: 2, 4 or 8 for B <= 32, 64, 128.
inline int grid_marginal_chunks(int n_bins_total) { return n_bins_total <= 32 ? 2 : n_bins_total <= 64 ? 4 : 8; }

// The LDS image of a slab in the marginal pass: the EM's slab (grid_prior_slab), with the table of global bin indices -- at most
// PNX_MAX_PARAMS rows of `width` int32, four doubles per atom -- in the place of the four wave-private rows.
inline GridSlab grid_marginal_slab(int n_b) { return grid_prior_slab(n_b); }
static_assert(PNX_MAX_PARAMS * sizeof(int32_t) <= 4 * sizeof(double), "the table must fit the four rows of the EM's slab");
}  // namespace pnx

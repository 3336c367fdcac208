// pnx_varpro_marginal_args.hpp -- the host half of pnx_curvefit_varpro_marginals_f64 that needs no device: the checks of its
// arguments in front of any device work (the outputs and the quantile levels, the variable-projection posterior's, shared, then
// the binning of the non-linear rows), the table of global bin indices the kernel reads per atom (grid_marginal_table, reused) and
// the choice of its instantiation.  Free of HIP types, like pnx_grid_marginal_args.hpp: pnx_api.hip and pnx_varpro_marginal.hip use
// it, tests/host_stub/varpro_marginal_args_stub.cpp builds the same code for the CPU under AddressSanitizer / UBSan.
#pragma once
#include <cmath>
#include <cstdint>

#include "pnx_grid_marginal_args.hpp"
#include "pnx_varpro_posterior_args.hpp"

namespace pnx {

// The outputs and the quantile levels first, then varpro_posterior_check_args with `marginal` in the place of `mean` (the
// posterior's refusals, atom and prior rules hold unchanged), then the binning: only a non-linear row (a rate, a free T1) can hold
// bins -- the value of a fraction or of S0 belongs to the voxel-atom pair, not to the atom.  Every refusal names its first offender.
inline int varpro_marginal_check_args(const pnx_curvefit_opts *o, int64_t n_vox, const double *b, const double *y, int n_atoms,
                                      const double *nl_atoms, const double *fixed, const double *lo, const double *hi, const double *log_prior,
                                      double noise_sd, int marginal_amplitudes, const int32_t *n_bins, const int32_t *bin_of,
                                      const double *bin_value, int n_q, const double *probs, const double *marginal, const double *quantile,
                                      int mem, VarproLayout *L, VarproPosteriorHost *H, GridMarginalHost *M) {
    if (!marginal) return set_error(PNX_ERR_INVALID, "varpro marginals: marginal is NULL (the one output that is not optional)");
    if (n_q < 0 || n_q > kGridMarginalMaxProbs)
        return set_error(PNX_ERR_INVALID, "varpro marginals: n_q=%d out of range [0,%d]", n_q, kGridMarginalMaxProbs);
    if (n_q && !probs) return set_error(PNX_ERR_INVALID, "varpro marginals: probs is NULL but n_q=%d", n_q);
    if (n_q && !quantile) return set_error(PNX_ERR_INVALID, "varpro marginals: quantile is NULL but n_q=%d", n_q);
    for (int i = 0; i < n_q; ++i)
        if (!(probs[i] > 0.0 && probs[i] < 1.0))
            return set_error(PNX_ERR_INVALID, "varpro marginals: probs[%d]=%g must lie in the open interval (0, 1)", i, probs[i]);
    if (!n_bins || !bin_of || !bin_value) return set_error(PNX_ERR_INVALID, "varpro marginals: n_bins, bin_of or bin_value is NULL");
    if (int rc = varpro_posterior_check_args(o, n_vox, b, y, n_atoms, nl_atoms, fixed, lo, hi, log_prior, noise_sd, marginal_amplitudes, marginal,
                                             mem, L, H))
        return rc;
    long long total = 0;
    for (int k = 0; k < o->n_free; ++k) {
        if (n_bins[k] < 0) return set_error(PNX_ERR_INVALID, "varpro marginals: n_bins[%d]=%d is negative", k, n_bins[k]);
        if (L->row_src[k] < 0 && n_bins[k] != 0)
            return set_error(PNX_ERR_INVALID, "varpro marginals: n_bins[%d]=%d for a linear row (a fraction or S0) must be 0: its value is "
                                              "solved per voxel and atom, not a grid value", k, n_bins[k]);
        total += n_bins[k];
    }
    if (total < 1 || total > kGridMarginalMaxBins)
        return set_error(PNX_ERR_INVALID, "varpro marginals: B = sum n_bins = %lld out of range [1,%d]", total, kGridMarginalMaxBins);
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
            if (std::isnan(bin_value[off + j])) return set_error(PNX_ERR_INVALID, "varpro marginals: bin_value[%d] is NaN", off + j);
            if (j && !(bin_value[off + j] > bin_value[off + j - 1]))
                return set_error(PNX_ERR_INVALID, "varpro marginals: bin_value[%d]=%g is not above bin_value[%d]=%g (free parameter %d: "
                                                  "strictly ascending)", off + j, bin_value[off + j], off + j - 1, bin_value[off + j - 1], k);
        }
        for (int g = 0; g < n_atoms && nb; ++g) {
            const int bin = bin_of[(size_t)k * n_atoms + g];
            if (bin < 0 || bin >= nb)
                return set_error(PNX_ERR_INVALID, "varpro marginals: bin_of[%d, %d]=%d out of range [0,%d)", k, g, bin, nb);
            const double a = nl_atoms[(size_t)L->row_src[k] * n_atoms + g];
            if (!(a == bin_value[off + bin]))
                return set_error(PNX_ERR_INVALID, "varpro marginals: atom %d, free parameter %d = %.17g is not bin_value[%d]=%.17g of its bin %d",
                                 g, k, a, off + bin, bin_value[off + bin], bin);
        }
    }
    return PNX_OK;
}

// 16-bin chunks of accumulators the kernel is instantiated with: 4 or 8 for B <= 64, 128.  A 2-chunk instantiation is not built:
// at one wave per SIMD (the K chains and the y fragments fill the rest of the register file) it would not add a wave.
inline int varpro_marginal_chunks(int n_bins_total) { return grid_marginal_chunks(n_bins_total) <= 4 ? 4 : 8; }

// The LDS image of a slab is the posterior's (varpro_posterior_slab, called): the table of global bin indices -- at most k + 1 rows
// of `width` int32, one per non-linear row with bins -- takes the place of its k + 1 rows of centred non-linear values.
inline GridSlab varpro_marginal_slab(int n_b, int k) { return varpro_posterior_slab(n_b, k); }
}  // namespace pnx
